"""The checks of tests/test_gpu_lstm_ops.py judged on the CPU: the fp32 emulation of the recurrence
stands in for the kernel.  Unmodified it passes every check; each of five one-line mistakes in it
(the mutations of profiles/lstm_op_tests.md) is rejected, by the check named here."""
import pytest

import test_gpu_lstm_ops as L

EXPECT = {"no_forget_bias": "'f'", "gate_swap": "'j'", "bw_at_s": "out != hs[s+1]", "cs_1e-4": "'c'",
          "dh_fin_late": "'dz'"}


def test_the_table_in_the_module_covers_a_fresh_measurement():
    """8 x a table entry is the only free term of a bound.  The fp32 formulas' errors, measured again
    here on three of the module's cases, stay within the entries (which are the maxima over all cases),
    and reach at least a quarter of each forward entry: the table is neither typed in too small nor
    far above what the formulas give."""
    got = L.measure(fwd=[(64, 19, 5, False), (64, 19, 5, True)], bwd_step=[(96, 19)], bwd=[(64, 19, 5)], verbose=False)[5]
    tab = L.FP32_TORCH_ERR[5]
    assert set(got) == set(tab)
    for q, e in got.items():
        assert 0 < e <= tab[q], (q, e, tab[q])
    for q in "ijfoch":
        assert got[q] >= 0.25 * tab[q], (q, got[q], tab[q])
    assert L.BOUND == {T: {q: 8.0 * e for q, e in t.items()} for T, t in L.FP32_TORCH_ERR.items()}


@pytest.mark.parametrize("fx", [False, True])
def test_the_emulation_passes_the_forward_checks(fx):
    x = L._fwd_case(64, 19, 5, fx)
    got = L._emul_fwd(x)
    del got["h32"]
    L._assert_bounds("emulation", x, L._fwd_errors(x, got))


@pytest.mark.parametrize("step", [False, True])
def test_the_emulation_passes_the_backward_checks(step):
    x = L._bwd_case(64, 19, 5)
    got = L._emul_bwd(x, step)
    got.update(dz=got.pop("dz_operand"), dz_bf16=1.0)
    L._assert_bwd_bounds("emulation", x, L._bwd_errors(x, got), step=step)


def test_every_mutation_is_rejected():
    caught = L.mutation_failures()
    assert set(caught) == set(EXPECT)
    for mut, why in caught.items():
        assert why is not None and EXPECT[mut] in why, (mut, why)
