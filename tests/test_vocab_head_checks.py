"""The checks of tests/test_gpu_vocab_head_ops.py judged on the CPU: a torch fp32 emulation of the head (logits in
64-wide K blocks, per-group (max, sum exp), the select through the K best tiles, the hash as a dict) stands in for the
kernels.  Unmodified it passes every case on both input kinds; each mistake planted in it (the mutations of
profiles/vocab_head_op_tests.md) is rejected by the check named here.  A second test shows which of them the earlier
measure (ids against final_topk_wide over the stored logits, |dlp| < 1e-3) lets through."""
import pytest
import torch

import test_gpu_vocab_head_ops as M

E = M.Emu
CASE = (3000, 128, 5, 4, 8, 96, "rand", "randn", None)
ODD = (601, 256, 63, 1, 2, 96, "rand", "randn", None)

# mutation -> (case, form, the check that rejects it on the exact inputs, on the general inputs)
MUTATIONS = {
    "tie_larger_id": (CASE, "baseline", "order", None),
    "lse_last_tile": (ODD, "baseline", "lp", "lp"),
    "group_twice": (CASE, "pointer", "lp", "lp"),
    "mass_to_T": (CASE, "pointer", "range", "range"),
    "dup_once": (CASE, "pointer", "lp", "lp"),
    "oov_vocab_term": (CASE, "pointer", "lp", "lp"),
    "copied_kept": (CASE, "pointer", "dup", "dup"),
    "pg_swapped": (CASE, "pointer", "lp", "lp"),
    "drop_kth_tile": (CASE, "baseline", "order", None),
    "article_mod": (CASE, "pointer", "lp", "lp"),
    "logit_1e-3": (CASE, "baseline", "exact", "bound"),
}


def _rejected_by(case, form, mut, kind, old_style=False):
    try:
        M.run_head_form(E(mut), "cpu", M.head_case(kind, *case, old_style=old_style), form, "m")
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("kind", M.KINDS)
def test_the_emulation_passes_every_check(kind):
    for case in M.SPAN + M.TILE:
        M.run_head(E(), "cpu", case, kinds=(kind,), rerun=True)
    for case in M.TOPK:
        M.run_topk(E(), "cpu", case, False, kinds=(kind,))
    for case in M.TOPK_WIDE:
        M.run_topk(E(), "cpu", case, True, kinds=(kind,))
    for case in M.LINEAR2:
        M.run_linear2(E(), "cpu", kind, *case)
    for case in M.PAIR:
        M.run_linear2_pair(E(), "cpu", kind, *case)
    for width in M.WIDTHS:
        for R in (1, 3, 30):
            M.run_pgen(E(), "cpu", kind, R, *width)


def test_the_host_rules_give_the_lines_the_cases_are_meant_to_reach():
    assert [M.vp_rows(H) for H in (128, 256, 512)] == [448, 256, 128]  # the chunk loop: R = 449, 257, 129
    assert [M.vp_groups(V) for V in (16, 48, 600, 601, 32784, 66000)] == [1, 1, 5, 5, 256, 258]
    assert M.vp_ni_max(32768) == 1 and M.vp_ni_max(32784) == 2 and M.vp_ni_max(66000) == 2
    assert [M.topk_split(V) for V in (8191, 8192, 8193)] == [1, 1, 2]
    ids = M.chain_ids(40, 12000 + 2048)  # asserts the collisions and the wrap on the mirror of vhslot
    assert len(set(ids)) == 40 and M.vhslot(1) == (2654435761 >> 21) & 2047
    assert M.head_parts(9000, 64) == 36 and M.head_parts(601, 512, tile=True) == 5 and M.head_parts(601, 256, tile=True) == 3


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_mutation_is_rejected_by_the_named_check(mut):
    case, form, exact, general = MUTATIONS[mut]
    assert _rejected_by(case, form, None, "exact") is None and _rejected_by(case, form, None, "general") is None
    got = _rejected_by(case, form, mut, "exact")
    assert got is not None and f": {exact}: " in got, (mut, got)
    got = _rejected_by(case, form, mut, "general")
    if general is None:  # tie order: only equal values show it, and only the exact inputs have them
        assert got is None, (mut, got)
    else:
        assert got is not None and f": {general}: " in got, (mut, got)


def test_the_old_measure_passes_the_shared_mistakes():
    """The measure of tests/test_gpu_wide_fused.py: the fused op's ids equal final_topk_wide's over the logits the op
    stored, |dlp| < 1e-3, on inputs of the old kind (zero attention and valid ids past len).  The emulation with the
    same mistake stands in for the other kernel where the two kernels share the code (the hash, the order, the
    union); a mistake in the fused head's own partials is not in it."""
    passes = set()
    for mut, (case, form, _, _) in MUTATIONS.items():
        ok = True
        for kind in M.KINDS:
            c = M.head_case(kind, *case, old_style=True)
            R, V, H, T, K, beam = c["R"], c["V"], c["H"], c["T"], c["K"], c["beam"]
            ptr = form == "pointer"
            pg, attn = (c["pg"], c["attn"]) if ptr else (None, None)
            ids, lp, lg = torch.zeros(R, K, dtype=M.I32), torch.zeros(R, K), torch.zeros(R, V)
            E(mut).vocab_topk(c["X"], c["WT"], c["bias"], pg, attn, c["ext"], c["lens"], ids, lp, lg, torch.zeros(R, 1, 2), R, V,
                              H, T, K, beam)
            ids2, lp2 = torch.zeros(R, K, dtype=M.I32), torch.zeros(R, K)
            E(mut).final_topk_wide(lg, torch.zeros(V), pg, attn, c["ext"], c["lens"], ids2, lp2, torch.zeros(R, 1, 2),
                                   torch.zeros(R, 1, K), torch.zeros(R, 1, K, dtype=M.I32), R, V, T, K, beam)
            ok &= torch.equal(ids, ids2) and bool(((lp - lp2).abs() < 1e-3).all())
        if ok:
            passes.add(mut)
    assert passes == {"tie_larger_id", "mass_to_T", "dup_once", "oov_vocab_term", "copied_kept", "pg_swapped", "article_mod",
                      "logit_1e-3"}, passes
