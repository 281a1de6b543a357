"""The checks of tests/test_gpu_attn_ops.py judged on the CPU: an fp32 torch emulation of each formula
stands in for the kernel.  Unmodified it passes every check; each of eight one-line mistakes in it (the
mutations of profiles/attention_op_tests.md) is rejected, by the check named here."""
import pytest

import test_gpu_attn_ops as M

EXPECT = {"mask_le": "a past the length", "no_wc_cov": "'a'", "F_not_scaled_back": "'a'", "b_mod_rep": "a past the length",
          "tie_lt": "'de'", "S_without_dctx_ctx": "'de'", "de_1e-5": "'de'", "cov_keep_own_row": "cov_keep != cov_src[gidx]"}


def test_the_table_in_the_module_covers_a_fresh_measurement():
    """8 x a table entry is the only free term of a bound.  The fp32 formulas' errors, measured again here on
    three forward cases, two backward cases and one attn_bwd_feat case, stay within the entries (the maxima
    over all cases), and reach at least a quarter of each forward entry."""
    fwd = [("score", lambda: M._score_case(1024, 9, 4, 300, True, True), 8),
           ("score", lambda: M._score_case(64, 2, 4, 1024, True, False), 8),
           ("row", lambda: M._row_case(512, 8, 4, 300, False), 12)]
    bwd = [("bwd", lambda: M._bwd_case(512, 16, 300, 512, True, M.BWD_BOUNDS)), ("bwd", lambda: M._bwd_case(64, 8, 41, 64, True))]
    feat = [("feat", lambda: M._feat_case(5, 512, 12, 41, True))]
    got = M.measure(fwd, bwd, feat, verbose=False)
    assert set(got) == set(M.FP32_TORCH_ERR)
    for q, e in got.items():
        assert 0 < e <= M.FP32_TORCH_ERR[q], (q, e, M.FP32_TORCH_ERR[q])
    for q in ("e", "a", "ctx"):
        assert got[q] >= 0.25 * M.FP32_TORCH_ERR[q], (q, got[q], M.FP32_TORCH_ERR[q])
    assert M.BOUND == {q: 8.0 * e for q, e in M.FP32_TORCH_ERR.items()}


@pytest.mark.parametrize("kind", ["score", "row", "rowp"])
def test_the_emulation_passes_the_forward_checks(kind):
    x = {"score": lambda: M._score_case(128, 10, 2, 300, True, False), "row": lambda: M._row_case(512, 8, 3, 7, False),
         "rowp": lambda: M._row_case(512, 8, 1, 41, False, cov=True, EW=M.EG)}[kind]()
    got = M._emul_fwd(x, nw=12 if kind == "row" else 16)
    if kind == "score":  # e on its own, then the softmax from that e
        M._assert_bounds("emulation", M._fwd_errors(x, got, teacher=True))
    del got["e"]
    M._assert_bounds("emulation", M._fwd_errors(x, got))


@pytest.mark.parametrize("EW", [64, M.EG])
def test_the_emulation_passes_the_backward_checks(EW):
    x = M._bwd_case(64 if EW == 64 else 512, 8, 41, EW, True)
    M._assert_bounds("emulation", M._bwd_errors(x, M._emul_bwd(x)))


def test_the_emulation_passes_the_feat_checks():
    x = M._feat_case(5, 192, 12, 41, True)
    M._assert_bounds("emulation", M._feat_errors(x, M._emul_feat(x), 36))


def test_every_mutation_is_rejected():
    caught = M.mutation_failures()
    passing = {m for m in caught if isinstance(m, tuple)}
    assert passing == {("fwd", None), ("bwd", None), ("keep", None)} and all(caught[m] is None for m in passing)
    assert set(caught) - passing == set(EXPECT)
    for mut, want in EXPECT.items():
        assert caught[mut] is not None and want in caught[mut], (mut, caught[mut])


def test_the_old_max_norm_measure_passes_the_small_de_mistake():
    """1e-5 on one small de element: the elementwise bound rejects it (above), max |got - ref| / max |ref| < 2e-3
    of tests/test_gpu_attention_ops.py would not have."""
    x = M._bwd_case(512, 8, 41, 512, True)
    assert M.old_max_norm_error(x, M._emul_bwd(x, "de_1e-5")["de"], M._bwd_ref(x)["de"]) < 2e-3
