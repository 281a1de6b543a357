"""The checks of tests/test_gpu_gemm_ops.py judged on the CPU: a torch emulation of each op (fp32 products in 64-wide
K blocks, the gather, merge and split logic in plain Python) stands in for the kernel.  Unmodified it passes every
check on both input kinds, so the float64 reference alone stays inside the bounds and the exact inputs are exact;
each one-line mistake planted in it (the mutations of profiles/gemm_op_tests.md) is rejected, by the check named here."""
import pytest

import test_gpu_gemm_ops as M

E = M.Emu

# mutation -> (runner, case, the check that must reject it on the exact inputs)
MUTATIONS = {
    "drop_block": (M.run_plain, (300, 384, 192, False, False, True, True), "exact"),
    "double_block": (M.run_plain, (257, 512, 64, False, False, True, False), "exact"),
    "chunk_swap": (M.run_plain, (255, 256, 128, True, True, False, False), "exact"),
    "swap_rows": (M.run_plain, (300, 128, 192, False, True, False, False), "exact"),
    "last_split_twice": (M.run_splitk, (257, 128, 2112, False, 2), "exact"),
    "row_past_M": (M.run_plain, (300, 256, 128, False, True, True, True), "sentinel"),
    "rev_wrong_half": (M.run_merge, (2, 40, 7, 64, 384, 0), "exact"),
    "xsf_ntn": (M.run_frame, (True, 1, 40, 7, 384, 192, False, True, False, True, False), "xsf"),
    "ctx_tail": (M.run_ctx_fwd, (3, 72, 17, 256), "exact"),
    "acc_overwrite": (M.run_plain, (256, 384, 192, False, True, True, False), "exact"),
    "one_elem_1e-3": (M.run_plain, (300, 512, 128, False, True, False, False), "exact"),
}
GENERAL = {"row_past_M": "sentinel", "xsf_ntn": "xsf"}  # on the general inputs: these, else the elementwise bound


def _rejected_by(run, case, mut, kind):
    try:
        run(E(mut), "cpu", kind, *case)
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("kind", M.KINDS)
def test_the_emulation_passes_every_check(kind):
    runs = [(M.run_plain, M.PLAIN), (M.run_frame, M.FRAME), (M.run_merge, M.MERGE), (M.run_splitk, M.SPLITK),
            (M.run_wgrad_tt, M.WGRAD_TT), (M.run_wgrad_tn, M.WGRAD_TN), (M.run_ctx_fwd, M.CTX)]
    for run, cases in runs:
        for case in cases:
            run(E(), "cpu", kind, *case)
    for case in M.CTX:
        for flag in (False, True):
            M.run_ctx_da(E(), "cpu", kind, *case, flag)
            M.run_ctx_de(E(), "cpu", kind, *case, flag)


def test_the_split_rules_give_the_shapes_the_cases_are_meant_to_reach():
    assert [M.splits_bt(1, 128, K) for K in (1984, 2048, 2112, 3072)] == [1, 2, 2, 3]
    assert [M.splits_tt(512, 384, K) for K in (64, 320, 4160)] == [1, 5, 33]  # 4160: 32 splits of 2 steps, one of 1
    assert M.splits_tt(256, 256, 192) == 3 and M.splits_tt(256, 128, 64) == 1
    assert [M.splits_tn(256, 200, K) for K in (1, 65, 1100)] == [1, 1, 3]


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_mutation_is_rejected_by_the_named_check(mut):
    run, case, want = MUTATIONS[mut]
    assert _rejected_by(run, case, None, "exact") is None and _rejected_by(run, case, None, "general") is None
    got = _rejected_by(run, case, mut, "exact")
    assert got is not None and f": {want}: " in got, (mut, got)
    got = _rejected_by(run, case, mut, "general")
    assert got is not None and f": {GENERAL.get(mut, 'bound')}: " in got, (mut, got)


def test_the_old_max_norm_measure_passes_the_small_mistake(monkeypatch):
    """Every mutation's case on the general inputs, judged by max |got - ref| / max |ref| < 2e-3 (1e-2 for a bf16
    output) of tests/test_gpu_gemm.py on every output the runner compares.  It passes 1e-3 on the smallest element of
    a product, which the elementwise bound rejects (above), and the two listed mistakes that leave the compared
    output alone (the stray row past M, the xsf interleave); every other one changes some element by a whole term
    and fails it too."""
    seen = []

    def record(tag, got, ref, mag, K, kind, adds=(), out_bf16=False, **kw):
        full = ref.clone()
        for a in adds:
            full = full + a.double()
        seen.append(M.old_max_norm_error(got, full) < (1e-2 if out_bf16 else 2e-3))

    monkeypatch.setattr(M, "_check", record)  # the runners' own checks off: the old measure in their place
    monkeypatch.setattr(M.Out, "intact", lambda *a, **k: None)
    passes = set()
    for mut, (run, case, _) in MUTATIONS.items():
        del seen[:]
        try:
            run(E(mut), "cpu", "general", *case)
        except AssertionError as e:
            assert ": xsf: " in str(e), (mut, e)  # the one check a runner makes itself
        assert seen, mut
        if all(seen):
            passes.add(mut)
    assert passes == {"one_elem_1e-3", "row_past_M", "xsf_ntn"}, passes
