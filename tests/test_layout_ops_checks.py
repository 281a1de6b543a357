"""The checks of tests/test_gpu_layout_ops.py judged on the CPU: a torch emulation of each op, written in the kernels'
own index form (flat thread index -> element, fp32 adds in the kernels' order for the column sums, the job-row
interpreter of pack_cast on arena offsets), stands in for the kernel.  Unmodified it passes every check on both input
kinds, so the references alone stay inside the bounds and the exact inputs are exact; each one-line mistake planted in
it (the mutations of profiles/layout_op_tests.md) is rejected, by the check named here.  The host classifier
pack_job_rows runs here on CPU tensors for every pair shape of the GPU module."""
import pytest
import torch

import test_gpu_layout_ops as M
from textsummarization_on_flink_amd.models.pointer_generator import pack_job_rows

E = M.Emu
PACK = M.pack_cases()


def _pack(name):
    return lambda k, dev: M.run_pack(k, dev, name, PACK[name])


def _kinds(run, *case):
    """a column-sum runner on both input kinds"""
    def go(k, dev):
        for kind in M.KINDS:
            run(k, dev, kind, *case)
    return go


# mutation -> (the run, the check that must reject it)
MUTATIONS = {
    "rev_on_fw": (lambda k, dev: M.run_to_step_frame(k, dev, True, True, 7, 9, 128, 0), "exact"),
    "doff_dropped": (lambda k, dev: M.run_to_step_frame(k, dev, False, False, 7, 9, 64, 64), "exact"),
    "one_trip": (lambda k, dev: M.run_to_step_frame(k, dev, *M.TO_FRAME_BIG), "exact"),
    "bw_at_t": (lambda k, dev: M.run_from_step_frame(k, dev, 7, 9, 64), "exact"),
    "hop_bw_not_reversed": (lambda k, dev: M.run_step_frame_hop(k, dev, 7, 9, 64), "exact"),
    "acc_overwrite": (lambda k, dev: M.run_tr01(k, dev, 3, 7, 12, "acc"), "exact"),
    "vec_store_past_T": (lambda k, dev: M.run_transpose_bta(k, dev, 3, 101, 64), "sentinel"),
    "rowgroup_clamped": (_kinds(M.run_cast_colsum, 3, 4), "exact"),
    "last_chunk_twice": (_kinds(M.run_colsum, 130, 260, False, False), "exact"),
    "finish1_first_partial": (_kinds(M.run_colsum, 130, 3, True, True), "exact"),
    "bf16_truncate": (lambda k, dev: M.run_tr01(k, dev, 3, 7, 12, "outb"), "bf16"),
    "tail_8_past_n": (_pack("k1 n=2049"), "sentinel"),
    "k2_rowlen_C": (_pack("k2 63x65"), "exact"),
    "search_job_before": (_pack("large and one-workgroup jobs"), "exact"),
    "scale_after_cast": (_pack("k3 5x520"), "exact"),
    "unk_modulo": (lambda k, dev: M.run_beam_gather(k, dev, 64, 128, 7, 32, True, True), "exact"),
    "parent_identity": (lambda k, dev: M.run_beam_gather(k, dev, 64, 128, 7, 32, True, False), "exact"),
}
# on the general inputs the column sums are judged by the bound
GENERAL = {"rowgroup_clamped": "bound", "last_chunk_twice": "bound", "finish1_first_partial": "bound"}


def _rejections(run, mut):
    """the messages of the checks that reject the run, one per input kind where the run has kinds"""
    try:
        run(E(mut), "cpu")
    except AssertionError as e:
        return str(e)
    return None


def test_the_emulation_passes_every_frame_and_gather_check():
    k = E()
    for case in M.TO_FRAME:
        M.run_to_step_frame(k, "cpu", *case)
    for case in M.FROM_FRAME:
        M.run_from_step_frame(k, "cpu", *case)
    for case in M.HOP:
        M.run_step_frame_hop(k, "cpu", *case)
    for case in M.TR01:
        for mode in M.TR01_MODES:
            M.run_tr01(k, "cpu", *case, mode)
    for case in M.BTA:
        M.run_transpose_bta(k, "cpu", *case)
    for case in M.GATHER:
        for cov in (False, True):
            for step in (False, True):
                M.run_beam_gather(k, "cpu", *case, cov, step)


def test_the_emulation_passes_the_second_trip_cases():
    assert M.run_to_step_frame(E(), "cpu", *M.TO_FRAME_BIG) > M.GRID_CAP
    assert M.run_from_step_frame(E(), "cpu", *M.FRAME_BIG_BT, 512) > M.GRID_CAP
    assert M.run_step_frame_hop(E(), "cpu", *M.FRAME_BIG_BT, 256) > M.GRID_CAP


def test_the_emulation_refuses_what_the_bindings_refuse():
    k = E()
    M.run_tr01_refusals(k, "cpu")
    M.run_alignment_refusals(k, "cpu")
    M.run_beam_gather_refusals(k, "cpu")
    M.run_pack_refusals(k, "cpu")
    M._refused("transpose_bta A = 96", lambda: M.run_transpose_bta(k, "cpu", 1, 3, 96))
    for C in (12, 2048):
        M._refused(f"cast_colsum C = {C}", lambda: M.run_cast_colsum(k, "cpu", "exact", 3, C))
    with pytest.raises(AssertionError, match="refusal"):
        M._refused("accepted", lambda: None)


@pytest.mark.parametrize("kind", M.KINDS + ("special",))
def test_the_emulation_passes_every_column_sum_check(kind):
    for case in M.CAST_COLSUM:
        M.run_cast_colsum(E(), "cpu", kind, *case)
    if kind == "special":
        return
    for N, C in M.COLSUM:
        for bf in (False, True):
            for acc in (False, True):
                M.run_colsum(E(), "cpu", kind, N, C, bf, acc)


def test_the_split_rules_give_the_shapes_the_cases_are_meant_to_reach():
    M.test_the_split_rules_reach_the_lines_the_cases_are_meant_for()
    assert M.cast_colsum_depth(3, 4) == 1 + 255 + 1 + 16 and M.cast_colsum_depth(300, 1024) == 2 + 0 + 16 + 16
    assert M.colsum_depth(4225, 4) == 17 + 3 + 1 + 256 and M.colsum_depth(130, 514) == 17 + 3 + 1 + 16


@pytest.mark.parametrize("name", list(PACK))
def test_the_emulation_passes_every_pack_check_and_the_classifier_holds(name):
    """run_pack asserts, per pair, the kind, the first workgroup and (through the total) the workgroup count the case
    declares, then validates the table on the host, before the interpreter runs it"""
    rows, total = M.run_pack(E(), "cpu", name, PACK[name])
    assert total == rows[-1][11] + {1: -(-rows[-1][14] // 2048), 3: -(-rows[-1][14] // 2048), 0: -(-rows[-1][14] // 256),
                                   2: -(-rows[-1][3] // 64) * -(-rows[-1][4] // 64)}[rows[-1][12]]


def test_the_pack_cases_reach_every_kind_and_the_last_two_transposes_are_contiguous():
    kinds = {}
    for name, build in PACK.items():
        ar = M.Arenas()
        build(ar)
        kinds[name] = [sp["kind"] for sp in ar.specs]
    assert kinds["k2 1x200"] == [(1, 1)] * 4 and kinds["k2 200x1"] == [(1, 1)] * 4  # a 1 x n transpose view is contiguous
    assert kinds["k2 130x70"] == [(2, 6)] * 4 and kinds["k2 63x65"] == [(2, 2)] * 4 and kinds["k2 64x64"] == [(2, 1)] * 4
    assert kinds["k1 n=2049"] == [(1, 2)] * 4 and kinds["k3 5x520"] == [(3, 2)] * 4 and kinds["k3 300x24"] == [(3, 4)] * 4
    assert kinds["k0 unaligned source"] == [(0, 1)] * 4 + [(0, 2)] * 4 and kinds["k0 gates 32x20"] == [(0, 10)] * 8
    assert len(kinds["64 one-workgroup jobs"]) == 64 and {n for _, n in kinds["64 one-workgroup jobs"]} == {1}
    assert {kd for kd, _ in kinds["64 one-workgroup jobs"]} == {0, 1, 2, 3}
    mixed = kinds["large and one-workgroup jobs"]
    assert {kd for kd, _ in mixed} == {0, 1, 2, 3} and any(n == 1 for _, n in mixed) and any(n > 3 for _, n in mixed)


def test_the_classifier_keeps_the_kinds_of_the_engines_pairs():
    """the view shapes of HipPointerGenerator._pack_job_pairs on small CPU weights"""
    Ed, H, A, V, Vp = 24, 16, 32, 40, 128
    f = lambda *s: torch.randn(*s)
    b = lambda *s: torch.empty(*s, dtype=torch.bfloat16)
    Kd = f(Ed + H, 4 * H)
    Kx01, WcT2, ovb = b(A, 8 * H), b(4 * H, A + H), b(H, Vp)
    pairs = [(b(V, Ed), f(V, Ed)), (b(Ed, 4 * H), Kd[:Ed]),
             (b(Ed, 4 * H).view(Ed, H, 4), Kd[:Ed].view(Ed, 4, H).permute(0, 2, 1)),
             (b(4 * H, Ed).view(H, 4, Ed), Kd[:Ed].view(Ed, 4, H).permute(2, 1, 0)),
             (b(2, H, 4 * H)[1], Kd[Ed:]), (b(2, 4 * H, H)[1], Kd[Ed:].t()), (torch.empty(2, 4 * H)[1], f(4 * H)),
             (Kx01[:, 4 * H:], f(A + H, 4 * H)[:A]), (b(A, A), f(A, A), M.K2LOG2E),
             (b(A, A), f(A, A).t(), M.K2LOG2E), (WcT2[:, :A], f(A, 4 * H).t()), (WcT2[:, A:], f(Ed + H, 4 * H)[Ed:].t()),
             (ovb[:, :V], f(H, V))]
    rows, total = pack_job_rows(pairs)
    assert [r[12] for r in rows] == [1, 1, 0, 0, 1, 2, 1, 3, 1, 2, 0, 0, 3]
    assert rows[8][15] == rows[9][15] == 0x4038aa3b and rows[0][15] == 0  # the fp32 bits of 2 log2(e); 0 = no scale
    starts = [r[11] for r in rows]
    assert starts == sorted(starts) and starts[0] == 0 and total > starts[-1]
    assert pack_job_rows(pairs, len(pairs) - 1) == (None, 0) and pack_job_rows(pairs, len(pairs))[1] == total


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_mutation_is_rejected_by_the_named_check(mut):
    run, want = MUTATIONS[mut]
    assert _rejections(run, None) is None
    got = _rejections(run, mut)
    assert got is not None and f": {want}: " in got, (mut, got)


@pytest.mark.parametrize("mut", sorted(GENERAL))
def test_the_column_sum_mutations_are_rejected_by_the_bound_on_general_inputs(mut):
    run = {"rowgroup_clamped": lambda k: M.run_cast_colsum(k, "cpu", "general", 3, 4),
           "last_chunk_twice": lambda k: M.run_colsum(k, "cpu", "general", 130, 260, False, False),
           "finish1_first_partial": lambda k: M.run_colsum(k, "cpu", "general", 130, 3, True, True)}[mut]
    run(E())
    with pytest.raises(AssertionError, match=": bound: "):
        run(E(mut))


def test_the_validator_rejects_a_wrong_table():
    """a kind 3 row whose destination stride was swapped for the source's, a kind 1 row one element too long"""
    ar = M.Arenas()
    M.geom_rows(ar, 5, 16, 0, None)
    M.geom_k1(ar, 100, 1, None)
    ar.build(M._gen(1), "cpu")
    rows, total = pack_job_rows(ar.pairs())
    ar.validate("ok", rows, total)
    bad = [list(r) for r in rows]
    bad[0][9] = bad[0][6]
    with pytest.raises(AssertionError, match="validator"):
        ar.validate("stride", bad, total)
    bad = [list(r) for r in rows]
    bad[1][14] += 1
    with pytest.raises(AssertionError, match="validator"):
        ar.validate("count", bad, total)
