"""The decode vocab head one op at a time against float64 torch on the CPU: vocab_topk / vocab_topk_pg
(csrc/kernels/vocab_topk.hip: span and tile logits kernels, the select at KL = 8 and 32), final_topk / final_topk_wide
(beam.hip, partial and merge kernels), linear2, linear2_pair and the pgen forward (decoder.hip).  Every op is called
through ops(); no reference goes through another kernel or an fp32 matmul.

    z      = X.double() @ WT.double().T + bias.double()                 [R][V]
    lse    = logsumexp(z, 1)
    fd[r]  = pg[r] exp(z[r] - lse[r]) on ids < V, 0 on ids V .. V + T
    fd[r, ext[a][i]] += (1 - pg[r]) attn[r][i]     for i < lens[a], a = r // beam   (pg = 1, no copy: the baseline form)
    order  = value descending, id ascending
    pg (vocab_topk_pg) = sigmoid([ctx, c, h.float(), x] . w + b)

Two kinds of input for every case.
  exact    X and WT in {-1, 0, 1} (bf16), integer bias: every logit and partial sum is an integer below 2^24
           (_assert_exact of the GEMM tests, on the reference), the spread of a row within 60 and min(z - lse) > -80, so
           no fp32 probability underflows into a false tie.  The stored logits equal the reference in every element;
           in the baseline form out_ids equal the reference ids IN ORDER on every row (integer logits tie at every
           rank: the id-ascending rule everywhere); attention weights are multiples of a power of two whose sums are
           exact, so a second run gives the same bits.
  general  randn X, W scaled by H^-1/2, randn or zipf bias.  logits within (H + 4) U sum|x w| + U |z|, U = 2^-24.

out_lp against a per-row absolute bound (profiles/vocab_head_op_tests.md derives it; nothing is measured):
    e_n = (H + 4) U max_k sum_j |x_j w_kj| + U max_k |z_k|          a logit, and the lse built from such logits (0: exact)
    e_r = 2 e_n + (len + 8) U + 3 * 2e-6 + 2 U (|L_K| + 1) + d_pg / min(pg, 1 - pg)
and ids by the gap rule on the reference log-probs L (L_K the K-th): every id with L > L_K + 2 e_r is in the output,
every output id has L >= L_K - 2 e_r, no duplicates, no id outside [0, V + T), out_lp within e_r of L[out_ids] and
non-increasing.  A row whose smallest non-zero reference gap across the cut is below 2 e_r is a near tie: at most 1
row in 10 of a case (asserted on the reference alone, reported); on every other row the id set equals the reference's.

Sentinels: every output is a view inside a NaN / id-sentinel allocation compared bit for bit outside the view; attn
past lens[a] is NaN, ext past lens[a] alternates -1 and 2^30; X and WT sit in NaN-padded allocations.

The runners take the op table k (ops(), or Emu: fp32 torch with the kernel's group partials, tile pruning and a dict
for the hash) and the device, so tests/test_vocab_head_checks.py runs the same checks on the CPU and plants mistakes."""
import math
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_gemm_ops as G
from test_gpu_gemm_ops import BF, F32, NAN, PAD, U24, _assert_exact, _gen, _inflat, _sync

pytestmark = pytest.mark.gpu

F64 = torch.float64
I32 = torch.int32
ID_SENT = -7777
KINDS = ("exact", "general")
FORMS = ("pointer", "baseline", "pg")
LOG_EPS = 2e-6          # an exp2 / __logf evaluation, absolute on a log (profiles/train_tail_tests.md section 3)
VM_HASH = 2048


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


# ------------------------------------------------------------------ host-side rules (ports of the launchers')
def vhslot(w):
    """vhslot / hslot (vocab_topk.hip, beam.hip)"""
    return (((w * 2654435761) & 0xffffffff) >> 21) & (VM_HASH - 1)


def vp_rows(H):
    sub = 32 if H >= 512 else 64
    return 150 * 1024 // (2 * H + 64) // sub * sub


def vp_groups(V):
    nt16 = (V + 15) // 16
    g = (nt16 + 15) // 16 if nt16 > 4096 else 256
    return min(g, (nt16 + 7) // 8)


def vp_ni_max(V):
    """the largest number of 16-column tiles one wave of the span kernel owns"""
    nt16, nw = (V + 15) // 16, 8 * vp_groups(V)
    return max((q + 1) * nt16 // nw - q * nt16 // nw for q in range(nw))


def head_parts(V, H, tile=False):
    """vocab_topk_tiles"""
    if H in (128, 256, 512) and not tile:
        return vp_groups(V)
    cols = 256 if H <= 256 else 128
    return (V + cols - 1) // cols


def topk_split(V):
    return (V + 8191) // 8192


# ------------------------------------------------------------------ guarded outputs
def _bits(t):
    return t.view({BF: torch.int16, F32: I32, I32: I32}[t.dtype])


class Guard:
    """a contiguous output of the given shape inside a NaN (float) / ID_SENT (int) allocation, PAD elements around it"""

    def __init__(self, shape, dtype, dev):
        self.n = 1
        for s in shape:
            self.n *= s
        self.flat = torch.full((2 * PAD + self.n,), ID_SENT if dtype == I32 else NAN, dtype=dtype).to(dev)
        self.view = self.flat[PAD:PAD + self.n].view(*shape)
        self.before = _bits(self.flat).cpu().clone()

    def intact(self, tag):
        bad = _bits(self.flat).cpu() != self.before
        bad[PAD:PAD + self.n] = False
        assert not bool(bad.any()), f"{tag}: sentinel: {int(bad.sum())} elements outside the output changed, first at flat " \
                                    f"index {int(bad.nonzero()[0])} (output is [{PAD}, {PAD + self.n}))"

    def cpu(self):
        return self.view.detach().cpu().clone()


def _same_bits(tag, a, b):
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), f"{tag}: rerun: not bit-identical"


# ------------------------------------------------------------------ inputs
def _head_xw(g, kind, R, V, H, bias_kind):
    if bias_kind == "flat":  # all logits of a row equal (both kinds): every column survives every pruning bound
        return (torch.randint(-1, 2, (R, H), generator=g).float().bfloat16(), torch.zeros(V, H, dtype=BF),
                torch.ones(V))
    if kind == "exact":
        p = min(1.0, 4.0 / math.sqrt(H))  # sum of H products in {-1, 0, 1}: sd 4 whatever H
        X = (torch.randint(-1, 2, (R, H), generator=g) * (torch.rand(R, H, generator=g) < p)).float().bfloat16()
        WT = (torch.randint(-1, 2, (V, H), generator=g) * (torch.rand(V, H, generator=g) < p)).float().bfloat16()
        return X, WT, torch.randint(-3, 4, (V,), generator=g).float()
    X = torch.randn(R, H, generator=g).bfloat16()
    WT = (torch.randn(V, H, generator=g) * H ** -0.5).bfloat16()
    bias = torch.randn(V, generator=g)
    if bias_kind == "zipf":
        bias = -1.5 * torch.log1p(torch.arange(V, dtype=F32)) + 0.05 * bias
    return X, WT, bias


def chain_ids(n_ids, limit):
    """ids below limit whose home slot is one of the table's last 8: more than 8 of them wrap round to slot 0"""
    ids = [w for w in range(limit) if vhslot(w) >= VM_HASH - 8][:n_ids]
    assert len(ids) == n_ids and all(VM_HASH - 8 <= vhslot(w) < VM_HASH for w in ids), (len(ids), limit)
    table = {}
    for w in ids:  # linear probing, as the kernels'
        h = vhslot(w)
        while h in table:
            h = (h + 1) & (VM_HASH - 1)
        table[h] = w
    assert sum(1 for h in table if h < VM_HASH - 8) == n_ids - 8 and 0 in table  # the chain wraps
    return ids


def _copy_inputs(g, kind, z, Na, beam, V, T, ext_kind, pgv, old_style=False):
    """lens, ext, attn, pg.  lens: T, 1, then random; ext rows: duplicates, OOV ids V .. V + T - 1, and the best
    plain word of the article's first row twice (a copied id that is also in the plain top-K)."""
    R = Na * beam
    lens = ([T, 1] + torch.randint(1, T + 1, (max(Na - 2, 0),), generator=g).tolist())[:Na]
    ext = torch.randint(0, V + T, (Na, T), generator=g)
    if ext_kind == "distinct":
        lens = [T] * Na
        for a in range(Na):
            ext[a] = torch.randperm(V + T, generator=g)[:T]
    elif ext_kind == "one":
        lens = [T] * Na
        ext[:] = torch.randint(0, V + T, (Na, 1), generator=g)
    elif ext_kind == "chain":
        lens = [60] * Na
        ext[:, :40] = torch.tensor(chain_ids(40, V + T))
    else:
        n4 = T // 4
        ext[:, :n4] = ext[:, n4:2 * n4]  # duplicates
        ext[:, 2 * n4:2 * n4 + min(n4, T)] = V + torch.arange(T - min(n4, T), T)  # OOV ids up to V + T - 1
    if ext_kind in ("rand", "chain"):
        for a in range(Na):
            best = int(z[a * beam].argmax())
            ext[a, 41 if ext_kind == "chain" else 0] = best
            if lens[a] > 50:
                ext[a, 45] = best
    lens_t = torch.tensor(lens, dtype=I32)
    live = torch.arange(T)[None, :] < lens_t.repeat_interleave(beam)[:, None]
    if kind == "exact":  # multiples of 2^-(12 + p) with 2^p >= T: every partial sum exact (< 2^24 units), the row's sum <= 1
        attn = torch.randint(1, 4097, (R, T), generator=g).float() / (4096 * 2 ** math.ceil(math.log2(max(T, 2))))
    else:
        attn = torch.rand(R, T, generator=g) + 1e-3
        attn = attn / (attn * live).sum(1, keepdim=True)
    if old_style:  # the existing tests' inputs: zeros and valid ids past len
        attn = attn * live
    else:
        attn = torch.where(live, attn, torch.full_like(attn, NAN))
        fill = torch.where(torch.arange(T) % 2 == 0, torch.tensor(-1), torch.tensor(2 ** 30))[None, :].expand(Na, T)
        ext = torch.where(torch.arange(T)[None, :] < lens_t[:, None], ext, fill)
    pg = torch.full((R,), float(pgv)) if pgv is not None else torch.rand(R, generator=g) * 0.96 + 0.02
    return lens_t, ext.to(I32), attn, pg


def _pg_inputs(g, R, A, H, E):
    """[ctx, c, h, x] small integers, w zero but for 8 multiples of 1/16 that touch both ends of every segment: the
    pre-activation is exact in fp32 in any order, so d_pg is the sigmoid's own error alone"""
    n = A + 2 * H + E
    f = torch.randint(-4, 5, (R, n), generator=g).float()
    w = torch.zeros(n)
    at = [0, A - 1, A, A + H - 1, A + H, A + 2 * H - 1, A + 2 * H, n - 1]
    w[at] = (torch.randint(1, 3, (8,), generator=g) * (2 * torch.randint(0, 2, (8,), generator=g) - 1)).float() / 16
    b = torch.tensor([0.25])
    pre = f.double() @ w.double() + 0.25
    pg = torch.sigmoid(pre)
    assert float(pg.min()) >= 0.02 and float(pg.max()) <= 0.98, (float(pg.min()), float(pg.max()))
    return dict(ctx=f[:, :A].contiguous(), c=f[:, A:A + H].contiguous(), h=f[:, A + H:A + 2 * H].contiguous().bfloat16(),
                x=f[:, A + 2 * H:].contiguous(), w=w, b=b, pg=pg)


# ------------------------------------------------------------------ reference and checks
def fd_reference(z, pg, attn, ext, lens, beam, T):
    """log of the final distribution over V + T ids, float64; pg None: the baseline form"""
    R, V = z.shape
    p = torch.softmax(z, 1)
    fd = torch.zeros(R, V + T, dtype=F64)
    if pg is None:
        fd[:, :V] = p
        return fd.log()
    pg = pg.double()
    fd[:, :V] = pg[:, None] * p
    for r in range(R):
        n = int(lens[r // beam])
        fd[r].scatter_add_(0, ext[r // beam, :n].long(), (1 - pg[r]) * attn[r, :n].double())
    return fd.log()


def row_bounds(L, K, e_n, lens_rows, d_pg):
    """L_K and e_r per row (module docstring)"""
    LK = torch.sort(L, dim=1, descending=True, stable=True)[0][:, K - 1]
    e = 2 * e_n + (lens_rows.double() + 8) * U24 + 3 * LOG_EPS + 2 * U24 * (LK.abs() + 1) + d_pg
    return LK, e


def near_ties(tag, L, K, e):
    """rows whose smallest non-zero gap across the cut is below 2 e_r; the reference's sets.  On the reference alone."""
    R, W = L.shape
    Ls, order = torch.sort(L, dim=1, descending=True, stable=True)
    near = torch.zeros(R, dtype=torch.bool)
    for r in range(R):
        LK = Ls[r, K - 1]
        if W > K and Ls[r, K] == LK:  # an exact tie at the cut (same logit, neither word copied): id ascending decides
            lo, hi = Ls[r][Ls[r] < LK], Ls[r][Ls[r] > LK]
            gap = min(float(LK - lo[0]) if lo.numel() else math.inf, float(hi[-1] - LK) if hi.numel() else math.inf)
        else:
            gap = float(LK - Ls[r, K]) if W > K else math.inf
        near[r] = gap < 2 * float(e[r])
    n = int(near.sum())
    print(f"NEAR {tag} {n} of {R}")
    assert 10 * n <= R, f"{tag}: near-tie: {n} of {R} rows are near ties at the cut (reference alone; change the seed or scale)"
    return near, order[:, :K]


def check_logits(tag, kind, got, z, mag, H, bias):
    got = got.detach().cpu()
    assert got.shape == z.shape and got.dtype == F32, (tag, got.shape, got.dtype)
    if kind == "exact":
        _assert_exact(H, 1, 1, z - bias.double(), mag, z)
        want = z.float()
        bad = ~(got == want)
        if bool(bad.any()):
            at = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{tag}: exact: {int(bad.sum())} of {bad.numel()} logits differ, first at {list(at)}: got "
                                 f"{float(got[at])}, want {float(want[at])}")
        return
    bound = (H + 4) * U24 * mag + U24 * z.abs()
    err = (got.double() - z).abs()
    ok = err <= bound
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=math.inf).max())
    print(f"ERR/BOUND {tag} logits {ratio:.4f}")
    assert bool(ok.all()), f"{tag}: bound: {int((~ok).sum())} of {ok.numel()} logits outside the bound, largest err / bound " \
                           f"{ratio:.3g}, first at {(~ok).nonzero()[0].tolist()}"


def check_topk(tag, ids, lp, L, K, e, near, ref_ids, in_order):
    """the gap rule; in_order: the ids equal the reference's at every rank"""
    ids, lp = ids.detach().cpu().long(), lp.detach().cpu().double()
    R, W = L.shape
    assert ids.shape == (R, K) and lp.shape == (R, K), (tag, ids.shape)
    ok = (ids >= 0) & (ids < W)
    assert bool(ok.all()), f"{tag}: range: row {int((~ok).nonzero()[0][0])} holds the id {int(ids[~ok][0])} outside [0, {W})"
    srt = torch.sort(ids, 1)[0]
    dup = (srt[:, 1:] == srt[:, :-1]).any(1) if K > 1 else torch.zeros(R, dtype=torch.bool)
    assert not bool(dup.any()), f"{tag}: dup: row {int(dup.nonzero()[0])} holds an id twice: {ids[int(dup.nonzero()[0])].tolist()}"
    Lo = torch.gather(L, 1, ids)
    err = (lp - Lo).abs()
    bad = ~(err <= e[:, None])  # a NaN fails
    ratio = float((err / e[:, None]).nan_to_num(nan=math.inf).max())
    print(f"ERR/BOUND {tag} lp {ratio:.4f}")
    assert not bool(bad.any()), f"{tag}: lp: {int(bad.sum())} log-probs outside e_r, largest err / e_r {ratio:.3g}, first at " \
                                f"{bad.nonzero()[0].tolist()}"
    assert bool((lp[:, 1:] <= lp[:, :-1]).all()), f"{tag}: sorted: out_lp increases along a row"
    if in_order:
        bad = (ids != ref_ids).any(1)
        assert not bool(bad.any()), f"{tag}: order: {int(bad.sum())} rows differ from the reference ids in order, first row " \
                                    f"{int(bad.nonzero()[0])}: got {ids[int(bad.nonzero()[0])].tolist()}, want " \
                                    f"{ref_ids[int(bad.nonzero()[0])].tolist()}"
        return
    LK = torch.sort(L, dim=1, descending=True, stable=True)[0][:, K - 1]
    low = Lo < (LK - 2 * e)[:, None]
    assert not bool(low.any()), f"{tag}: gap: row {int(low.nonzero()[0][0])} holds an id more than 2 e_r below the K-th value"
    taken = torch.zeros(R, W, dtype=torch.bool).scatter_(1, ids, True)
    miss = (L > (LK + 2 * e)[:, None]) & ~taken
    assert not bool(miss.any()), f"{tag}: gap: row {int(miss.nonzero()[0][0])} lacks the id {int(miss.nonzero()[0][1])}, more " \
                                 f"than 2 e_r above the K-th value"
    want = torch.zeros(R, W, dtype=torch.bool).scatter_(1, ref_ids, True)
    diff = (taken != want).any(1) & ~near
    assert not bool(diff.any()), f"{tag}: set: {int(diff.sum())} rows off a near tie differ from the reference set, first row " \
                                 f"{int(diff.nonzero()[0])}"


# ------------------------------------------------------------------ the emulation (CPU, fp32 torch)
class Emu:
    """The ops under test in fp32 torch on the CPU; mut plants one mistake (tests/test_vocab_head_checks.py)."""

    SHARED = ("tie_larger_id", "mass_to_T", "dup_once", "oov_vocab_term", "copied_kept", "pg_swapped", "article_mod")

    def __init__(self, mut=None):
        self.mut = mut

    def vocab_topk_parts(self, V, H):
        return head_parts(V, H)

    def topk_parts(self, V):
        return topk_split(V)

    @staticmethod
    def _mm(A, Bt):
        A, Bt = A.float(), Bt.float()
        acc = torch.zeros(A.shape[0], Bt.shape[0])
        for kb in range(0, A.shape[1], 64):
            acc += A[:, kb:kb + 64] @ Bt[:, kb:kb + 64].t()
        return acc

    def _slots(self, ext_row, n):
        """the hash: id -> slot, and the slot of every source position (-1: not counted)"""
        table, pos = {}, []
        for i in range(n):
            w = int(ext_row[i])
            if w < 0:
                pos.append(-1)
                continue
            first = w not in table
            s = table.setdefault(w, len(table))
            pos.append(s if first or self.mut != "dup_once" else -1)
        return table, torch.tensor(pos, dtype=torch.long)

    def _select(self, lg, pgen, attn, ext, lens, out_ids, out_lp, V, T, K, beam, tcols, own=True):
        """lg [R][V] fp32 (bias in).  own: the fused head's own partials (mistakes in them are not final_topk's)"""
        R = lg.shape[0]
        Na = R // beam
        mut = self.mut if own or self.mut in self.SHARED else None
        nt = (V + tcols - 1) // tcols
        pad = torch.full((R, nt * tcols - V), -math.inf)
        zt = torch.cat([lg, pad], 1).view(R, nt, tcols)
        m_g = zt.max(2)[0]
        ex = torch.exp(zt - m_g[:, :, None])
        if mut == "lse_last_tile" and V % 16:
            ex.view(R, -1)[:, V // 16 * 16:] = 0
        s_g = ex.sum(2)
        if mut == "group_twice":
            s_g[:, 0] *= 2
        M = m_g.max(1)[0]
        lse = M + torch.log((s_g * torch.exp(m_g - M[:, None])).sum(1))
        ptr = pgen is not None
        tables = {}
        for r in range(R):
            z = lg[r]
            tm, tq = torch.sort(m_g[r], descending=True, stable=True)  # the K tiles with the largest maxima
            if mut == "tie_larger_id":
                tm, tq = torch.sort(m_g[r].flip(0), descending=True, stable=True)
                tq = nt - 1 - tq
            keep = tq[:K]
            if mut == "drop_kth_tile" and nt >= K >= 2 and tm[K - 1] == tm[K - 2]:
                keep, tm = tq[:K - 1], torch.full_like(tm, -math.inf)  # (its K - 1 tiles still fill K ranks)
            tau = tm[K - 1] if nt >= K else -math.inf
            cols = (keep.sort()[0][:, None] * tcols + torch.arange(tcols)[None, :]).reshape(-1)
            cols = cols[cols < V]
            cols = cols[z[cols] >= tau]
            if mut == "tie_larger_id":
                cols = cols.flip(0)
            plain = cols[torch.sort(z[cols], descending=True, stable=True)[1][:K]]
            pg = float(pgen[r]) if ptr else 1.0
            if mut == "pg_swapped" and ptr:
                pg = 1.0 - pg
            pg = torch.tensor(pg, dtype=F32)
            cid, cval = plain, pg * torch.exp(z[plain] - lse[r])
            if ptr:
                a = r % Na if mut == "article_mod" else r // beam
                n = T if mut == "mass_to_T" else int(lens[a])
                if a not in tables:
                    tables[a] = self._slots(ext[a], n)
                table, pos = tables[a]
                mass = torch.zeros(max(len(table), 1)).index_add_(0, pos[pos >= 0], attn[r, :n][pos >= 0].float())
                w = torch.tensor(list(table.keys()), dtype=torch.long)
                if mut != "copied_kept":
                    keepp = ~torch.isin(cid, w)
                    cid, cval = cid[keepp], cval[keepp]
                inv = w < V
                zw = z[torch.where(inv, w, w % V if mut == "oov_vocab_term" else torch.zeros_like(w))]
                pv = torch.where(inv | (mut == "oov_vocab_term"), torch.exp(zw - lse[r]), torch.zeros(()))
                cid = torch.cat([cid, w])
                cval = torch.cat([cval, pg * pv + (1 - pg) * mass[:len(table)]])
            o = torch.sort(cid, descending=mut == "tie_larger_id", stable=True)[1]
            cid, cval = cid[o], cval[o]
            o = torch.sort(cval.nan_to_num(nan=math.inf), descending=True, stable=True)[1][:K]
            got = cid[o].clamp(-2 ** 31, 2 ** 31 - 1).to(I32)
            out_ids[r, :got.numel()] = got
            out_lp[r, :got.numel()] = torch.log(cval[o])
        return m_g, s_g

    def vocab_topk(self, X, WT, bias, pgen, attn, ext, lens, out_ids, out_lp, logits, part_ms, R, V, H, T, K, beam):
        lg = self._mm(X, WT) + bias
        if self.mut == "logit_1e-3":
            flat = lg.view(-1)
            flat[int(flat.abs().argmin())] += 1e-3
        logits.copy_(lg)
        part_ms.zero_()
        self._select(lg, pgen, attn, ext.view(-1, T), lens, out_ids.view(R, K), out_lp.view(R, K), V, T, K, beam, 256)

    def vocab_topk_pg(self, X, WT, bias, ctx, c, h, x, pg_w, pg_b, pg_out, attn, ext, lens, out_ids, out_lp, logits,
                      part_ms, R, V, H, T, K, beam, A, E):
        self.pgen(ctx, c, h, x, pg_w, pg_b, pg_out, R, A, H, E)
        self.vocab_topk(X, WT, bias, pg_out, attn, ext, lens, out_ids, out_lp, logits, part_ms, R, V, H, T, K, beam)

    def final_topk(self, logits, bias, pgen, attn, ext, lens, out_ids, out_lp, part_ms, part_v, part_i, R, V, T, K, beam):
        lg = logits.view(R, V) + bias
        part_ms.zero_()
        part_v.zero_()
        part_i.zero_()
        self._select(lg, pgen, attn, ext.view(-1, T), lens, out_ids.view(R, K), out_lp.view(R, K), V, T, K, beam, 8192,
                     own=False)

    final_topk_wide = final_topk

    def _lin(self, a1, K1, a2, K2, Wt, bias, add, out, outb, B, N):
        A = a1.view(B, K1) if K2 == 0 else torch.cat([a1.view(B, K1), a2.view(B, K2)], 1)
        v = self._mm(A, Wt.view(N, K1 + K2))
        if bias is not None:
            v = v + bias
        if add is not None:
            v = v + add.view(B, N)
        if out is not None:
            out.view(B, N).copy_(v)
        if outb is not None:
            outb.view(B, N).copy_(v)

    def linear2(self, a1, K1, a2, K2, Wt, bias, add, out, outb, B, N):
        self._lin(a1, K1, a2, K2, Wt, bias, add, out, outb, B, N)

    def linear2_pair(self, a1, K1, a2, K2, Wt, bias, add, out, outb, N, c1, L1, c2, L2, Vt, vbias, vadd, vout, voutb, M, B):
        self._lin(a1, K1, a2, K2, Wt, bias, add, out, outb, B, N)
        self._lin(c1, L1, c2, L2, Vt, vbias, vadd, vout, voutb, B, M)

    def pgen(self, ctx, c, h, x, w, b, pg, R, A, H, E):
        f = torch.cat([ctx.view(R, A), c.view(R, H), h.view(R, H).float(), x.view(R, E)], 1)
        pg.copy_(torch.sigmoid(f @ w + b))


# ------------------------------------------------------------------ runners
def head_case(kind, V, H, Na, beam, K, T, ext_kind, bias_kind, pgv, old_style=False):
    """inputs and the float64 reference of one case and input kind, shared by the three forms"""
    g = _gen(31, V, H, Na, beam, K, T, len(ext_kind), len(bias_kind), int(100 * (pgv or 0)), kind == "exact")
    R = Na * beam
    assert V >= 2 * K and R % beam == 0 and T <= 2048
    X, WT, bias = _head_xw(g, kind, R, V, H, bias_kind)
    z = X.double() @ WT.double().t() + bias.double()
    mag = X.double().abs() @ WT.double().abs().t()
    lens, ext, attn, pg = _copy_inputs(g, kind, z, Na, beam, V, T, ext_kind, pgv, old_style)
    A, E = 2 * H, 32
    pgi = _pg_inputs(g, R, A, H, E)
    exact = kind == "exact" or bias_kind == "flat"
    if exact:
        assert float((z.max(1)[0] - z.min(1)[0]).max()) <= 60
        assert float((z - torch.logsumexp(z, 1, keepdim=True)).min()) > -80
    e_n = torch.zeros(R, dtype=F64) if exact else (H + 4) * U24 * mag.max(1)[0] + U24 * z.abs().max(1)[0]
    return dict(kind="exact" if exact else "general", V=V, H=H, Na=Na, beam=beam, K=K, T=T, R=R, A=A, E=E, X=X, WT=WT, bias=bias,
                z=z, mag=mag, lens=lens, ext=ext, attn=attn, pg=pg, pgi=pgi, e_n=e_n)


def run_head_form(k, dev, c, form, tag, rerun=False):
    """one form of the op on one case: logits, ids by the gap rule (in order: baseline on exact inputs), sentinels"""
    R, V, H, T, K, beam = c["R"], c["V"], c["H"], c["T"], c["K"], c["beam"]
    tag = f"{tag}/{form}/{c['kind']}"
    pg = {"pointer": c["pg"], "baseline": None, "pg": c["pgi"]["pg"]}[form]
    L = fd_reference(c["z"], pg, c["attn"], c["ext"], c["lens"], beam, T)
    lens_rows = c["lens"].repeat_interleave(beam) if form != "baseline" else torch.zeros(R)
    d_pg = 16 * U24 / torch.minimum(pg, 1 - pg).double() if form == "pg" else 0.0
    LK, e = row_bounds(L, K, c["e_n"], lens_rows, d_pg)
    near, ref_ids = near_ties(tag, L, K, e)
    nt = int(k.vocab_topk_parts(V, H))
    Xd, WTd = _inflat(c["X"], dev), _inflat(c["WT"], dev)
    bias, ext, lens = c["bias"].to(dev), c["ext"].to(dev), c["lens"].to(dev)
    attn = _inflat(c["attn"], dev)

    def call():
        o = dict(ids=Guard((R, K), I32, dev), lp=Guard((R, K), F32, dev), lg=Guard((R, V), F32, dev),
                 ms=Guard((R, nt, 2), F32, dev), pgo=Guard((R,), F32, dev))
        if form == "pg":
            p = c["pgi"]
            k.vocab_topk_pg(Xd, WTd, bias, _inflat(p["ctx"], dev), _inflat(p["c"], dev), _inflat(p["h"], dev),
                            _inflat(p["x"], dev), p["w"].to(dev), p["b"].to(dev), o["pgo"].view, attn, ext, lens, o["ids"].view,
                            o["lp"].view, o["lg"].view, o["ms"].view, R, V, H, T, K, beam, c["A"], c["E"])
        else:
            ptr = form == "pointer"
            k.vocab_topk(Xd, WTd, bias, c["pg"].to(dev) if ptr else None, attn if ptr else None, ext, lens, o["ids"].view,
                         o["lp"].view, o["lg"].view, o["ms"].view, R, V, H, T, K, beam)
        _sync(dev)
        return o

    o = call()
    check_logits(tag, c["kind"], o["lg"].view, c["z"], c["mag"], H, c["bias"])
    if form == "pg":
        got = o["pgo"].cpu().double()
        bad = ~((got - pg).abs() <= 16 * U24)
        assert not bool(bad.any()), f"{tag}: pg_out: row {int(bad.nonzero()[0])} is {float(got[bad][0])}, want {float(pg[bad][0])}"
    check_topk(tag, o["ids"].view, o["lp"].view, L, K, e, near, ref_ids, form == "baseline" and c["kind"] == "exact")
    for name, gd in o.items():
        gd.intact(f"{tag} {name}")
    if rerun and c["kind"] == "exact":
        o2 = call()
        for name in ("ids", "lp", "lg"):
            _same_bits(f"{tag} {name}", o2[name].cpu(), o[name].cpu())


def run_head(k, dev, case, kinds=KINDS, forms=FORMS, rerun=False):
    tag = "vocab_topk" + str(tuple(case))
    for kind in kinds:
        if case[7] == "flat" and kind == "general":
            continue  # the flat row is the same in both kinds
        c = head_case(kind, *case)
        for form in forms:
            run_head_form(k, dev, c, form, tag, rerun)


def topk_case(kind, V, Na, beam, K, T, ext_kind, zkind, with_bias, pgv=None):
    g = _gen(32, V, Na, beam, K, T, len(ext_kind), len(zkind), with_bias, kind == "exact")
    R = Na * beam
    if kind == "exact":
        lg = torch.randint(-20, 1, (R, V), generator=g).float()
        bias = torch.randint(-3, 4, (V,), generator=g).float() if with_bias else torch.zeros(V)
        if zkind == "ties":  # more than 2048 equal maxima inside one split, none of them in the split's first ids
            lg[:, 1100:3600] = 8.0 - bias[1100:3600]
    else:
        lg = torch.randn(R, V, generator=g) * 3
        bias = torch.randn(V, generator=g) if with_bias else torch.zeros(V)
    z = lg.double() + bias.double()
    lens, ext, attn, pg = _copy_inputs(g, kind, z, Na, beam, V, T, ext_kind, pgv)
    if kind == "exact":
        assert float((z.max(1)[0] - z.min(1)[0]).max()) <= 60
        assert float((z - torch.logsumexp(z, 1, keepdim=True)).min()) > -80
        assert torch.equal(z.float().double(), z)
    e_n = torch.zeros(R, dtype=F64) if kind == "exact" else U24 * z.abs().max(1)[0]
    return dict(kind=kind, V=V, Na=Na, beam=beam, K=K, T=T, R=R, lg=lg, bias=bias, z=z, lens=lens, ext=ext, attn=attn, pg=pg,
                e_n=e_n)


def run_topk(k, dev, case, wide, kinds=KINDS, forms=("pointer", "baseline")):
    name = "final_topk_wide" if wide else "final_topk"
    fn = getattr(k, name)
    for kind in kinds:
        c = topk_case(kind, *case)
        R, V, T, K, beam = c["R"], c["V"], c["T"], c["K"], c["beam"]
        S = int(k.topk_parts(V))
        assert S == topk_split(V)
        lgd, bias, ext, lens = _inflat(c["lg"], dev), c["bias"].to(dev), c["ext"].to(dev), c["lens"].to(dev)
        attn = _inflat(c["attn"], dev)
        for form in forms:
            tag = f"{name}{tuple(case)}/{form}/{kind}"
            ptr = form == "pointer"
            L = fd_reference(c["z"], c["pg"] if ptr else None, c["attn"], c["ext"], c["lens"], beam, T)
            lens_rows = c["lens"].repeat_interleave(beam) if ptr else torch.zeros(R)
            LK, e = row_bounds(L, K, c["e_n"], lens_rows, 0.0)
            near, ref_ids = near_ties(tag, L, K, e)

            def call():
                o = dict(ids=Guard((R, K), I32, dev), lp=Guard((R, K), F32, dev), ms=Guard((R, S, 2), F32, dev),
                         pv=Guard((R, S, K), F32, dev), pi=Guard((R, S, K), I32, dev))
                fn(lgd, bias, c["pg"].to(dev) if ptr else None, attn if ptr else None, ext, lens, o["ids"].view, o["lp"].view,
                   o["ms"].view, o["pv"].view, o["pi"].view, R, V, T, K, beam)
                _sync(dev)
                return o

            o = call()
            check_topk(tag, o["ids"].view, o["lp"].view, L, K, e, near, ref_ids, not ptr and kind == "exact")
            for nm, gd in o.items():
                gd.intact(f"{tag} {nm}")
            if kind == "exact":
                o2 = call()
                for nm in ("ids", "lp"):
                    _same_bits(f"{tag} {nm}", o2[nm].cpu(), o[nm].cpu())


def _lin_inputs(g, kind, B, K1, K2, N, with_bias, with_add):
    a1, a2 = G._vals(g, (B, K1), kind), G._vals(g, (B, K2), kind) if K2 else None
    Wt = G._vals(g, (N, K1 + K2), kind, (K1 + K2) ** -0.5)
    bias = G._addend(g, (N,), kind) if with_bias else None
    add = G._addend(g, (B, N), kind, 64) if with_add else None
    A = a1 if a2 is None else torch.cat([a1, a2], 1)
    ref, mag = G._mmref(A, Wt)
    return a1, a2, Wt, bias, add, ref, mag


def _lin_check(tag, kind, K, o, ob, ref, mag, bias, add, B, N):
    adds = ([bias[None, :].expand(B, N)] if bias is not None else []) + ([add] if add is not None else [])
    G._check(tag, o.view, ref, mag, K, kind, adds)
    G._check(tag + "/bf16", ob.view, ref, mag, K, kind, adds, out_bf16=True)
    assert torch.equal(_bits(ob.cpu()), _bits(o.cpu().bfloat16())), f"{tag}: outb: not out rounded once"
    o.intact(tag)
    ob.intact(tag + " outb")


def run_linear2(k, dev, kind, B, K1, K2, N, with_bias, alias):
    """alias: add is out itself (the in-place x-merge)"""
    g = _gen(33, B, K1, K2, N, with_bias, alias, kind == "exact")
    a1, a2, Wt, bias, add, ref, mag = _lin_inputs(g, kind, B, K1, K2, N, with_bias, alias)
    o, ob = Guard((B, N), F32, dev), Guard((B, N), BF, dev)
    if alias:
        o.view.copy_(add)
    k.linear2(_inflat(a1, dev), K1, _inflat(a2, dev) if K2 else None, K2, _inflat(Wt, dev), bias.to(dev) if with_bias else None,
              o.view if alias else None, o.view, ob.view, B, N)
    _sync(dev)
    _lin_check(f"linear2({B},{K1},{K2},{N},bias={with_bias},alias={alias})", kind, K1 + K2, o, ob, ref, mag, bias, add, B, N)


def run_linear2_pair(k, dev, kind, B, K1, K2, N, L1, L2, M):
    """problem 0: [a1, a2] . Wt + bias -> out, outb; problem 1: c . Vt + vout in place (add aliased to out)"""
    g = _gen(34, B, K1, K2, N, L1, L2, M, kind == "exact")
    a1, a2, Wt, bias, _, ref0, mag0 = _lin_inputs(g, kind, B, K1, K2, N, True, False)
    c1, c2, Vt, _, add, ref1, mag1 = _lin_inputs(g, kind, B, L1, L2, M, False, True)
    o0, ob0 = Guard((B, N), F32, dev), Guard((B, N), BF, dev)
    o1, ob1 = Guard((B, M), F32, dev), Guard((B, M), BF, dev)
    o1.view.copy_(add)
    k.linear2_pair(_inflat(a1, dev), K1, _inflat(a2, dev) if K2 else None, K2, _inflat(Wt, dev), bias.to(dev), None, o0.view,
                   ob0.view, N, _inflat(c1, dev), L1, _inflat(c2, dev) if L2 else None, L2, _inflat(Vt, dev), None, o1.view, o1.view,
                   ob1.view, M, B)
    _sync(dev)
    tag = f"linear2_pair({B},{K1},{K2},{N},{L1},{L2},{M})"
    _lin_check(tag + "[0]", kind, K1 + K2, o0, ob0, ref0, mag0, bias, None, B, N)
    _lin_check(tag + "[1]", kind, L1 + L2, o1, ob1, ref1, mag1, None, add, B, M)


def run_pgen(k, dev, kind, R, A, H, E):
    g = _gen(35, R, A, H, E, kind == "exact")
    n = A + 2 * H + E
    if kind == "exact":
        p = _pg_inputs(g, R, A, H, E)
        f = torch.cat([p["ctx"], p["c"], p["h"].float(), p["x"]], 1)
        w, b = p["w"], p["b"]
    else:
        f = torch.randn(R, n, generator=g)
        f[:, A + H:A + 2 * H] = f[:, A + H:A + 2 * H].bfloat16().float()
        w, b = torch.randn(n, generator=g) * n ** -0.5, torch.randn(1, generator=g)
    pre = f.double() @ w.double() + b.double()
    ref = torch.sigmoid(pre)
    # an n-term fp32 sum in any order and the bias add through a sigmoid (slope <= 1/4), then exp, add and reciprocal
    bound = 16 * U24 + (0.0 if kind == "exact" else 0.25 * ((n + 4) * U24 * (f.double().abs() @ w.double().abs()) + U24 * pre.abs()))
    o = Guard((R,), F32, dev)
    k.pgen(_inflat(f[:, :A].contiguous(), dev), _inflat(f[:, A:A + H].contiguous(), dev),
           _inflat(f[:, A + H:A + 2 * H].contiguous().bfloat16(), dev), _inflat(f[:, A + 2 * H:].contiguous(), dev), w.to(dev),
           b.to(dev), o.view, R, A, H, E)
    _sync(dev)
    tag = f"pgen({R},{A},{H},{E})/{kind}"
    err = (o.cpu().double() - ref).abs()
    print(f"ERR/BOUND {tag} {float((err / bound).nan_to_num(nan=math.inf).max()):.4f}")
    assert bool((err <= bound).all()), f"{tag}: bound: largest err / bound {float((err / bound).max()):.3g}"
    o.intact(tag)


# ------------------------------------------------------------------ the cases (profiles/vocab_head_op_tests.md: what each reaches)
# V, H, Na, beam, K, T, ext, bias, p_gen (None: random in [0.02, 0.98])
SPAN = [(16, 128, 1, 1, 8, 96, "rand", "randn", None), (601, 256, 63, 1, 2, 96, "rand", "randn", None),
        (2053, 512, 65, 1, 1, 96, "rand", "randn", None), (600, 128, 449, 1, 8, 24, "rand", "randn", None),
        (600, 256, 257, 1, 2, 24, "rand", "randn", None), (600, 512, 129, 1, 9, 24, "rand", "randn", None),
        (3000, 128, 5, 4, 8, 96, "rand", "randn", 0.02), (3000, 256, 3, 16, 32, 96, "rand", "randn", 0.98),
        (3000, 128, 5, 6, 12, 96, "rand", "zipf", None), (32784, 256, 2, 6, 12, 96, "rand", "zipf", None),
        (66000, 128, 2, 1, 9, 96, "rand", "zipf", None), (48, 128, 2, 4, 8, 96, "rand", "randn", None),
        (3000, 128, 3, 4, 8, 2048, "distinct", "randn", 0.05), (3000, 256, 2, 1, 2, 2048, "one", "randn", None),
        (12000, 128, 2, 4, 8, 2048, "chain", "zipf", None), (66000, 256, 2, 2, 32, 96, "rand", "flat", None)]
TILE = [(255, 32, 1, 1, 1, 96, "rand", "randn", None), (256, 64, 65, 1, 8, 24, "rand", "randn", None),
        (257, 96, 129, 1, 2, 24, "rand", "randn", None), (601, 160, 13, 5, 12, 96, "rand", "randn", None),
        (512, 64, 32, 4, 8, 24, "rand", "randn", None), (9000, 64, 2, 16, 32, 96, "rand", "flat", None)]
# V, Na, beam, K, T, ext, logits, bias
TOPK = [(8191, 2, 4, 8, 96, "rand", "rand", False), (8192, 2, 1, 1, 96, "rand", "rand", True),
        (8193, 2, 8, 16, 96, "rand", "rand", True), (3001, 3, 4, 8, 96, "rand", "rand", True),
        (16, 2, 4, 8, 96, "rand", "rand", False), (8192, 2, 2, 8, 96, "rand", "ties", False),
        (8193, 2, 2, 16, 96, "rand", "ties", True), (8192, 2, 1, 1, 96, "rand", "ties", False),
        (3000, 3, 4, 8, 2048, "distinct", "rand", True, 0.05), (3000, 2, 1, 2, 2048, "one", "rand", False),
        (12000, 2, 4, 8, 2048, "chain", "rand", True)]
TOPK_WIDE = [(8193, 2, 4, 8, 96, "rand", "rand", True), (8191, 2, 1, 17, 96, "rand", "rand", False),
             (3001, 2, 16, 32, 96, "rand", "rand", True), (8192, 2, 2, 32, 96, "rand", "ties", True),
             (8193, 2, 2, 8, 96, "rand", "ties", False), (12000, 2, 4, 17, 2048, "chain", "rand", False)]
# B, K1, K2, N, bias, add aliased to out
LINEAR2 = [(1, 32, 0, 16, False, False), (15, 256, 512, 64, True, False), (16, 512, 0, 128, False, True),
           (17, 256, 256, 48, True, True), (37, 1024, 1024, 32, True, False), (37, 96, 32, 16, False, True)]
# B, K1, K2, N, L1, L2, M  (M < N: problem 1's column tiles past M exit at once)
PAIR = [(1, 64, 64, 64, 32, 0, 16), (15, 256, 256, 128, 512, 0, 32), (17, 128, 128, 32, 64, 0, 32), (37, 256, 256, 512, 512, 0, 128)]
WIDTHS = [(100, 36, 20), (160, 96, 48), (512, 256, 128)]  # tests/test_gpu_pgen.py


@pytest.mark.parametrize("case", SPAN, ids=str)
def test_vocab_topk_span_kernel(case):
    run_head(_ops(), "cuda", case, rerun=True)


@pytest.mark.parametrize("case", TILE, ids=str)
def test_vocab_topk_tile_kernel(case):
    run_head(_ops(), "cuda", case, rerun=True)


@pytest.mark.parametrize("case", TOPK, ids=str)
def test_final_topk(case):
    run_topk(_ops(), "cuda", case, False)


@pytest.mark.parametrize("case", TOPK_WIDE, ids=str)
def test_final_topk_wide(case):
    run_topk(_ops(), "cuda", case, True)


@pytest.mark.parametrize("case", LINEAR2, ids=str)
def test_linear2(case):
    for kind in KINDS:
        run_linear2(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", PAIR, ids=str)
def test_linear2_pair(case):
    for kind in KINDS:
        run_linear2_pair(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("R", [1, 3, 30])
@pytest.mark.parametrize("width", WIDTHS, ids=str)
def test_pgen_forward(width, R):
    for kind in KINDS:
        run_pgen(_ops(), "cuda", kind, R, *width)


CHILD_CASES = [(601, 65, 1, 8), (512, 32, 4, 12)]  # V, Na, beam, K at H = 128, 256, 512


def _child_tile_kernel():
    """in a fresh process started with TSAMD_VL_TILE=1 (vp_use reads it once): the tile kernel at H = 128 / 256 / 512"""
    assert os.environ.get("TSAMD_VL_TILE") == "1"
    k = _ops()
    for H in (128, 256, 512):
        for V, Na, beam, K in CHILD_CASES:
            assert int(k.vocab_topk_parts(V, H)) == head_parts(V, H, tile=True)
            for kind in KINDS:
                c = head_case(kind, V, H, Na, beam, K, 24, "rand", "randn", None)
                for form in ("pointer", "baseline"):
                    run_head_form(k, "cuda", c, form, f"tile_switch({V},{H},{Na},{beam},{K})")


def test_tile_kernel_behind_the_switch_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_vocab_head_ops as m; m._child_tile_kernel()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TSAMD_VL_TILE="1"), capture_output=True, text=True,
                       timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
