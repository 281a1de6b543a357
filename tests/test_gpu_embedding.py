"""Embedding-gradient kernels (csrc/kernels/embedding.hip) against a float64 index_add_, EXACTLY.

The source rows hold multiples of 1/256 in [-4, 4] and an id receives at most 1000 rows, so every
partial sum is a multiple of 1/256 below 2^24 / 256: exactly representable in fp32 whatever the
summation order.  emb_grad (one wave per row, atomics), emb_grad_sorted (64 id-sorted rows per
wave, 8 at a time, atomics where the id changes) and emb_grad_det (no atomics: chunk-local
segments stored, chunk-crossing segments through the pf / pl scratch rows and a chaining second
pass) must all equal the reference bit for bit.

Paths, by parameter:
  E = 8 / 64 / 128 / 200 / 512    PER = 1 with a partial width / 1 / 2 / 4 with a partial width / 8
  n = 1, 63, 64, 65               one row; one chunk short of / exactly / one row past 64
  n = 70                          a last chunk of 6 rows: the sorted kernel's 8-row batch runs its
                                  -1 sentinel tail there
  n = 200, 1000                   4 and 16 chunks
  n0 is never a multiple of 64: the switch between the two source tensors falls inside a chunk.
Id patterns (hand-built sorted lists; the row permutation is random, and the same ids are also
sent through the project's host routine emb_sort):
  one_id     every row the same id: the pl + pf chain of emb_grad_det runs over every chunk
             (4 at n = 200, 16 at n = 1000: first, "middle" and last chunks)
  spread     ids as distinct as V = 50 allows (all distinct up to n = 50, else segments of
             ceil(n / 50) rows)
  aligned    a segment that starts on a 64-row boundary and ends on one (one and two chunks long)
  mid_span   a segment from the middle of chunk 0 to the middle of chunk 2
  both_cont  chunk 1's first segment began in chunk 0 AND its last one continues into chunk 2
             (pf and pl written by one wave)
  zipf       a Zipf-like draw
Ids outside [0, V) are out of contract and not fed.
"""
import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.models.host_inputs import emb_sort
from textsummarization_on_flink_amd.ops import ops

pytestmark = pytest.mark.gpu

V = 50
N0 = {1: 1, 63: 20, 64: 37, 65: 33, 70: 65, 200: 100, 1000: 333}  # rows of the first source tensor


def _segments(n, segs, rest_from):
    """Sorted ids from (id, length) segments, then ids rest_from, rest_from + 1, ... in runs of 3."""
    out = []
    for i, ln in segs:
        out += [i] * ln
    assert len(out) <= n and all(a <= b for a, b in zip(out, out[1:]))
    k = 0
    while len(out) < n:
        out.append(min(rest_from + k // 3, V - 1))
        k += 1
    return np.array(out[:n], dtype=np.int64)


def _pattern(name, n):
    """Sorted id list of the pattern, or None where n is too small to build it."""
    rng = np.random.RandomState(n)
    if name == "one_id":
        return np.full(n, 7, dtype=np.int64)
    if name == "spread":
        return np.sort(np.arange(n) % V).astype(np.int64)
    if name == "zipf":
        return np.sort(np.minimum(rng.zipf(1.3, n) - 1, V - 1)).astype(np.int64)
    if n < 200:
        return None
    if name == "aligned":    # id 5: rows [64, 128); id 9: rows [128, 256) when they exist
        return _segments(n, [(3, 64), (5, 64)] + ([(9, 128)] if n >= 320 else []), 20)
    if name == "mid_span":   # id 5: rows [30, 150)
        return _segments(n, [(2, 30), (5, 120)], 10)
    if name == "both_cont":  # id 4: rows [40, 80); id 6: [80, 100); id 8: [100, 140)
        return _segments(n, [(1, 40), (4, 40), (6, 20), (8, 40)], 12)
    raise KeyError(name)


PATTERNS = ["one_id", "spread", "zipf", "aligned", "mid_span", "both_cont"]
CASES = [(n, p) for n in N0 for p in PATTERNS if _pattern(p, n) is not None and not (n == 1 and p != "one_id")]


def _case(E, n, pattern):
    """ids per source row (unsorted), the two source tensors, a hand-built (sid, perm) and the
    float64 reference."""
    rng = np.random.RandomState(1000 * E + n)
    sid = _pattern(pattern, n)
    perm = rng.permutation(n)
    ids = np.empty(n, dtype=np.int64)
    ids[perm] = sid                        # sorted row r reads source row perm[r]
    gen = torch.Generator().manual_seed(E * 7 + n)
    src = torch.randint(-1024, 1025, (n, E), generator=gen).float() / 256
    src[torch.rand(n, E, generator=gen) < 0.2] = 0.0   # the atomic kernels skip zero addends
    ref = torch.zeros(V, E, dtype=torch.float64).index_add_(0, torch.from_numpy(ids), src.double())
    assert float(ref.abs().max()) * 256 < 2 ** 24      # the exactness premise
    assert int(np.bincount(ids, minlength=V).max()) <= 4000
    n0 = N0[n]
    assert n0 % 64 != 0
    return ids, src[:n0].contiguous(), src[n0:].contiguous(), sid.astype(np.int32), perm.astype(np.int32), ref


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _prefill(E):
    return (torch.arange(V * E).reshape(V, E) % 7 - 3).float()


def _orders(ids, n0, sid, perm):
    """The hand-built sorted order and the project's own (emb_sort: stable)."""
    s2, p2 = emb_sort(ids[:n0], ids[n0:])
    assert np.array_equal(s2, sid)
    return [("hand", sid, perm), ("emb_sort", s2, p2)]


@pytest.mark.parametrize("n,pattern", CASES)
@pytest.mark.parametrize("E", [8, 64, 128, 200, 512])
def test_atomic_kernels_add_exactly(E, n, pattern):
    """emb_grad and emb_grad_sorted ADD the per-id row sums onto what gemb holds."""
    k = ops()
    ids, s0, s1, sid, perm, ref = _case(E, n, pattern)
    n0 = s0.shape[0]
    pre = _prefill(E)
    want = (ref + pre.double()).float()
    s0d, s1d = s0.cuda(), s1.cuda()
    gemb = pre.cuda()
    k.emb_grad(gemb, torch.from_numpy(ids[:n0]).cuda(), s0d, torch.from_numpy(ids[n0:]).cuda(), s1d)
    assert torch.equal(gemb.cpu(), want), "emb_grad"
    for tag, s, p in _orders(ids, n0, sid, perm):
        gemb = pre.cuda()
        k.emb_grad_sorted(gemb, _i32(s), _i32(p), s0d, s1d)
        assert torch.equal(gemb.cpu(), want), f"emb_grad_sorted ({tag} order)"


@pytest.mark.parametrize("n,pattern", CASES)
@pytest.mark.parametrize("E", [8, 64, 128, 200, 512])
def test_det_kernel_stores_exactly(E, n, pattern):
    """emb_grad_det STORES the per-id sums: the rows of the ids that occur are overwritten, the
    others are not touched.  The engine's contract is "gemb is zero before the call": the backward
    pass clears the whole flat gradient buffer first (``p.grad.zero_()``) and backward_tail_emb
    hands this kernel the embedding's view of it, with no other writer of that view -- so on a
    zeroed gemb the result is the full gradient.  On a pre-filled gemb the rows of absent ids must
    keep their values.  Two runs into fresh buffers give the same bits."""
    k = ops()
    ids, s0, s1, sid, perm, ref = _case(E, n, pattern)
    n0 = s0.shape[0]
    s0d, s1d = s0.cuda(), s1.cuda()
    nc = int(k.emb_grad_det_chunks(n))
    assert nc == (n + 63) // 64
    present = torch.from_numpy(np.bincount(ids, minlength=V) > 0)
    pre = _prefill(E)
    want_pre = torch.where(present[:, None], ref.float(), pre)
    for tag, s, p in _orders(ids, n0, sid, perm):
        outs = []
        for fill in (None, None, pre):
            gemb = torch.zeros(V, E, device="cuda") if fill is None else fill.cuda()
            # scratch rows start as NaN: a chunk partial that is read without having been written shows
            pf = torch.full((nc, E), float("nan"), device="cuda")
            pl = torch.full((nc, E), float("nan"), device="cuda")
            k.emb_grad_det(gemb, _i32(s), _i32(p), s0d, s1d, pf, pl)
            outs.append(gemb.cpu())
        assert torch.equal(outs[0], ref.float()), f"zeroed gemb ({tag} order)"
        assert torch.equal(outs[0], outs[1]), f"two runs differ ({tag} order)"
        assert torch.equal(outs[2], want_pre), f"pre-filled gemb ({tag} order)"
