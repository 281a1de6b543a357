"""The pointer-generator loss kernels against one float64 reference of the mixture loss and its
gradients: ptr_loss (csrc/kernels/loss.hip: fp32 two-pass and bf16 one-pass) and the fused vocab
head vocab_train_fwd -> ptr_rowfin -> vocab_train_bwd (csrc/kernels/vocab_train.hip), called as
the engine's _head_forward calls them.

Per decoder row n = (t, b), with z the logits row (bias included), w the gold id, g the row's
weight, pg = p_gen (1 without it), a the attention row:

    lse = logsumexp(z);  pv = exp(z_w - lse) [w < V];  c = sum_{i < len_b} a_i [ext_bi == w]
    P = pg pv + (1 - pg) c;  loss = -log P;  alpha = g pg pv / P
    dz_k = alpha (softmax_k - [k == w]);  dpre = -g (pv - c) / P pg (1 - pg)
    dA_i = -g (1 - pg) / P [i < len_b and ext_bi == w];  everything 0 where g == 0

The reference sees exactly the values the kernel receives (bf16 operands upcast).  P == 0 with
g != 0 is out of contract (as in the model this follows); the test asserts P > 1e-6 on its inputs.

Article rows (B = 5, T = 70, lens 1 / 70 / 23 / 47 / 64) and the gold ids of the rows (by t % 3):
  b = 0  len 1    an in-article OOV id at the only live position | an id found only past len |
                  the same, g = 0
  b = 1  len T    an id at positions 0, 33 and T - 1 | an id found once | an OOV id found twice
  b = 2  len 23   an id found only at positions >= len (the first one AT len) | an id found three
                  times inside and once past len | an OOV id found only past len (P = 0), g = 0
  b = 3  len 47   an id that is not in the article | an id at len - 1 and at len | an OOV id twice
  b = 4  len 64   id 0 (several times) | id V - 1, not in the article (the last logits column: in
                  the partial 8-group / vocab tile when V has one) | an id at len - 1
The attention rows are non-zero past len too, so a copy mass summed over T instead of len shows.

Bounds (derived in profiles/train_tail_tests.md, not measured):
  dz (bf16)              |dz - ref| <= 2^-8 |ref| + 2^-8 alpha_ref 1e-4 per element
  ptr_loss scalars       2e-5 relative (+ 2e-6 absolute for loss_row)
  fused head             e_n = 4 H 2^-24 max_k sum_j |x_nj| |w_kj| per row (fp32 MFMA accumulation
                         over K = H): loss_row, lse absolute e_n + 2e-6; alpha, dpre, dA relative
                         e_n + 2e-5
  dbias                  |dbias_k - sum_n dz_ref| <= 2^-8 sum_n |dz_ref| + 1e-7
  structural zeros       exactly 0.0
"""
import functools
import math

import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.ops import ops

pytestmark = pytest.mark.gpu

B, T = 5, 70
LENS = [1, 70, 23, 47, 64]
POOL = 16                      # the random article ids come from [0, POOL)
ZERO_G = {(2, 0), (2, 2)}      # (t % 3, b) of the rows with g = 0
BF = torch.bfloat16
NAN = float("nan")


def _gold(V):
    """Gold id of row (t, b) by [b][t % 3]."""
    return [[V + 2, 18, 17], [17, 16, V], [18, 17, V + 1], [33, 17, V + 1], [0, V - 1, 16]]


def _article(V, gen):
    ext = torch.randint(0, POOL, (B, T), generator=gen).int()

    def put(b, pos, i):
        ext[b, torch.tensor(pos)] = i
    put(0, [0], V + 2); put(0, [3, 10, 41], 17); put(0, [1, 20], 18)
    put(1, [5], 16); put(1, [0, 33, T - 1], 17); put(1, [7, 40], V)
    put(2, [22], 16); put(2, [2, 9, 21, 30], 17); put(2, [23, 50], 18); put(2, [4], V); put(2, [40], V + 1)
    put(3, [11], 16); put(3, [46, 47], 17); put(3, [12, 30], V + 1)
    put(4, [63], 16); put(4, [64], 18)
    return ext


def _rows(D, V, seed, pointer, dlen=None):
    """Host inputs of the N = D * B rows that do not depend on the logits."""
    gen = torch.Generator().manual_seed(seed)
    N = D * B
    ext = _article(V, gen)
    lens = torch.tensor(LENS, dtype=torch.int32)
    t, b = torch.arange(N) // B, torch.arange(N) % B
    gold = torch.tensor(_gold(V))
    target = gold[b, t % 3].int()
    rowg = (0.005 + 0.045 * torch.rand(N, generator=gen)).float()
    for (t3, bb) in ZERO_G:
        rowg[(t % 3 == t3) & (b == bb)] = 0.0
    if dlen is not None:  # dead decoder steps: t >= dlen[b]
        rowg[t >= torch.tensor(dlen)[b]] = 0.0
    pgen = (0.06 + 0.88 * torch.rand(N, generator=gen)).float()
    u = 0.2 + 0.8 * torch.rand(N, T, generator=gen)
    u = torch.where((ext[b] >= POOL) | (ext[b] == 0), 10 * u, u)  # weight on the positions gold ids sit at
    live = torch.arange(T)[None, :] < lens[b].long()[:, None]
    attn = (u / (u * live).sum(1, keepdim=True)).float()
    if not pointer:  # baseline mode: p_gen = 1, every gold id must be in the vocabulary
        target = torch.where(target >= V, torch.full_like(target, 19), target)
    return dict(N=N, D=D, V=V, ext=ext, lens=lens, target=target, rowg=rowg,
                pgen=pgen if pointer else None, attn=attn if pointer else None)


def _reference(z, r):
    """float64 loss and gradients of logits z [N][V] (float64) and the row inputs r."""
    N, V = z.shape
    b = torch.arange(N) % B
    w = r["target"].long()
    g = r["rowg"].double()
    lse = torch.logsumexp(z, 1)
    sm = torch.exp(z - lse[:, None])
    inv = w < V
    pv = torch.where(inv, sm[torch.arange(N), w.clamp(max=V - 1)], torch.zeros(N, dtype=torch.float64))
    if r["pgen"] is None:
        pg = torch.ones(N, dtype=torch.float64)
        hit = torch.zeros(N, T, dtype=torch.bool)
        c = torch.zeros(N, dtype=torch.float64)
    else:
        pg = r["pgen"].double()
        hit = (r["ext"][b] == r["target"][:, None]) & (torch.arange(T)[None, :] < r["lens"][b].long()[:, None])
        c = (r["attn"].double() * hit).sum(1)
    P = pg * pv + (1 - pg) * c
    on = g != 0
    assert bool((P[on] > 1e-6).all()), "inputs out of contract: P <= 1e-6 on a weighted row"
    zero = torch.zeros(N, dtype=torch.float64)
    Ps = torch.where(on, P, torch.ones_like(P))
    onehot = torch.zeros(N, V, dtype=torch.float64)
    onehot[inv, w[inv]] = 1.0
    alpha = torch.where(on, g * pg * pv / Ps, zero)
    return dict(lse=lse, pv=pv, c=c, P=P, on=on, hit=hit,
                loss=torch.where(on, -torch.log(Ps), zero), alpha=alpha,
                dz=alpha[:, None] * (sm - onehot),
                dpre=torch.where(on, -g * (pv - c) / Ps * pg * (1 - pg), zero),
                dA=torch.where(on[:, None] & hit, (-g * (1 - pg) / Ps)[:, None], torch.zeros(N, T, dtype=torch.float64)))


def _well_conditioned(ref):
    """dpre carries pv - c: the 2e-5 relative bound presumes no cancellation between the two."""
    on = ref["on"]
    d = (ref["pv"] - ref["c"]).abs()[on]
    assert bool((d >= 0.25 * torch.maximum(ref["pv"], ref["c"])[on]).all()), "pv ~ c on a weighted row"


def _within(x, ref, rel, floor=0.0):
    """(ok, worst error / bound) of |x - ref| <= rel |ref| + floor per element; rel and floor
    broadcast.  A zero bound demands an exact match (NaN never passes)."""
    x = x.detach().double().cpu()
    err = (x - ref).abs()
    tol = rel * ref.abs() + floor
    ok = bool((err <= tol).all())
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    return ok, float(ratio.nan_to_num(nan=float("inf")).max())


def _check(name, tag, x, ref, rel, floor=0.0):
    ok, ratio = _within(x, ref, rel, floor)
    print(f"[train-tail] {tag} {name}: worst error / bound = {ratio:.3g}")
    if not ok:
        x = x.detach().double().cpu()
        bad = ((x - ref).abs() > rel * ref.abs() + floor) | torch.isnan(x)
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} elements off, first at {i}: "
                             f"{float(x[tuple(i)])!r} vs {float(ref[tuple(i)])!r}")


def _check_dz(tag, dz, ref, rows=None):
    want, al = ref["dz"], ref["alpha"]
    if rows is not None:
        want, al = want[rows], al[rows]
    _check("dz", tag, dz, want, 2.0 ** -8, 2.0 ** -8 * 1e-4 * al[:, None])


def _cuda(r):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()}


# =========================================================================== 3a. ptr_loss
D3 = 3
# V -> the path it is there for
VOCABS = {37: "fp32 scalar passes; bf16 one partial 8-group only", 2000: "aligned; bf16 CH=4",
          2052: "fp32 float4 pass 1 + scalar pass 2", 2053: "fp32 scalar both passes; bf16 partial 8-group",
          8200: "bf16 CH=8", 16392: "bf16 CH=16", 32776: "bf16 CH=25", 51208: "bf16 CH=32"}


@functools.lru_cache(maxsize=None)
def _loss_case(V, pointer, bf):
    """Inputs and reference of one ptr_loss case (computed once, never modified).  The gold logit is
    set 4.5 below the row maximum: p_vocab(w) stays far above the 1e-6 floor at every V and well
    below the copy mass of the rows that have one (no cancellation in pv - c)."""
    r = _rows(D3, V, 100 + V, pointer)
    gen = torch.Generator().manual_seed(V)
    N = r["N"]
    z = 3.0 * torch.randn(N, V, generator=gen)
    bias = 0.5 * torch.randn(V, generator=gen)
    w = r["target"].long()
    inv = w < V
    top = (z + bias).max(1).values
    z[inv, w[inv]] = (top - 4.5 - bias[w.clamp(max=V - 1)])[inv]
    if bf:  # the bf16 kernel's logits carry their bias
        logits, bias = (z + bias).to(BF), None
        ref = _reference(logits.double(), r)
    else:
        logits = z
        ref = _reference(z.double() + bias.double(), r)
    if pointer:
        _well_conditioned(ref)
    return r, logits, bias, ref


def _check_loss_outputs(tag, ref, pointer, loss_row, dz, dpre, dA):
    _check("loss_row", tag, loss_row, ref["loss"], 2e-5, torch.where(ref["on"], 2e-6, 0.0).double())
    if dz is not None:
        _check_dz(tag, dz, ref)
    if pointer and dpre is not None:
        _check("dpre", tag, dpre, ref["dpre"], 2e-5)
        _check("dA", tag, dA.view(-1, T), ref["dA"], 2e-5)  # exactly 0 off the gold positions and past len


@pytest.mark.parametrize("pointer", [True, False], ids=["pgen", "nopgen"])
@pytest.mark.parametrize("V", list(VOCABS))
def test_ptr_loss_fp32(V, pointer):
    """fp32 logits + bias (two-pass kernel).  V = 37 and 2053: scalar fall-backs of both passes;
    V = 2052: float4 pass 1, scalar pass 2; the others: float4 / 8-wide passes."""
    k = ops()
    r, logits, bias, ref = _loss_case(V, pointer, False)
    d = _cuda(r)
    N = r["N"]
    loss_row = torch.full((N,), NAN, device="cuda")
    dz = torch.full((N, V), NAN, dtype=BF, device="cuda")
    dpre = torch.full((N,), NAN, device="cuda") if pointer else None
    dA = torch.full((N, T), NAN, device="cuda") if pointer else None
    k.ptr_loss(logits.cuda(), bias.cuda(), d["target"], d["rowg"], d["pgen"], d["attn"], d["ext"], d["lens"],
               loss_row, dz, dpre, dA, N, B, T, V)
    _check_loss_outputs(f"ptr_loss fp32 V={V} {'pgen' if pointer else 'nopgen'}", ref, pointer, loss_row, dz, dpre, dA)
    # forward only
    loss2 = torch.full((N,), NAN, device="cuda")
    k.ptr_loss(logits.cuda(), bias.cuda(), d["target"], d["rowg"], d["pgen"], d["attn"], d["ext"], d["lens"],
               loss2, None, None, None, N, B, T, V)
    assert torch.equal(loss2, loss_row)


@pytest.mark.parametrize("mode", ["out", "inplace", "fwd"])
@pytest.mark.parametrize("pointer", [True, False], ids=["pgen", "nopgen"])
@pytest.mark.parametrize("V", list(VOCABS))
def test_ptr_loss_bf16(V, pointer, mode):
    """bf16 logits (one-pass kernel, CH = 4 / 8 / 16 / 25 / 32 by ceil(V / 2048); V = 37 and 2053 end
    in a partial 8-group): dlogits out of place, aliasing the logits, and absent (forward only:
    nothing but loss_row is written)."""
    k = ops()
    r, logits, _, ref = _loss_case(V, pointer, True)
    d = _cuda(r)
    N = r["N"]
    ch = -(-V // 2048)
    assert {37: 1, 2000: 1, 2052: 2, 2053: 2, 8200: 5, 16392: 9, 32776: 17, 51208: 26}[V] == ch
    tag = f"ptr_loss bf16 V={V} {'pgen' if pointer else 'nopgen'} {mode}"
    lg = logits.cuda()
    loss_row = torch.full((N,), NAN, device="cuda")
    dpre = torch.full((N,), NAN, device="cuda") if pointer else None
    dA = torch.full((N, T), NAN, device="cuda") if pointer else None
    if mode == "fwd":
        k.ptr_loss(lg, None, d["target"], d["rowg"], d["pgen"], d["attn"], d["ext"], d["lens"], loss_row, None,
                   dpre, dA, N, B, T, V)
        _check_loss_outputs(tag, ref, pointer, loss_row, None, None, None)
        assert torch.equal(lg.cpu(), logits)
        if pointer:
            assert bool(torch.isnan(dpre).all()) and bool(torch.isnan(dA).all())
        return
    dz = lg if mode == "inplace" else torch.full((N, V), NAN, dtype=BF, device="cuda")
    k.ptr_loss(lg, None, d["target"], d["rowg"], d["pgen"], d["attn"], d["ext"], d["lens"], loss_row, dz, dpre, dA,
               N, B, T, V)
    _check_loss_outputs(tag, ref, pointer, loss_row, dz, dpre, dA)
    if mode == "out":
        assert torch.equal(lg.cpu(), logits)


# =========================================================================== 3b. fused head
D14 = 14
N70 = D14 * B
SPECIAL = [0, 16, 17, 18, 19, 33]  # in-vocabulary gold ids (and V - 1)
DLEN = {"A": [12, 9, 3, 6, 1],     # blocks 0 and 1 live, block 2 (rows 64..69) dead
        "B": [14, 2, 0, 5, 5],     # every block live
        "C": [6, 5, 2, 6, 1]}      # block 0 only


def _blocks(dlen, D):
    """vlive / vblk / vblk_n of the 32-row blocks, as host_inputs (models/host_inputs.py)
    builds them from the live decoder steps per row."""
    dlen = np.asarray(dlen)
    nb = (D * len(dlen) + 31) // 32
    lr = np.zeros(nb * 32, dtype=bool)
    lr[:D * len(dlen)] = (np.arange(D)[:, None] < dlen[None, :]).reshape(-1)
    vlive = lr.reshape(nb, 32).any(1)
    vblk = np.full(nb, nb, dtype=np.int32)
    live_ids = np.nonzero(vlive)[0]
    vblk[:len(live_ids)] = live_ids
    return vlive.astype(np.int32), vblk, np.array([len(live_ids)], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _head_operands(H, V):
    """X [N][H + 8] (the 8 pad columns hold data the kernel must not read as activations), W^T and
    bias.  The rows of W^T of the gold ids are small and their bias is 7, so that p_vocab(w) stays
    far above 1e-6 whatever the row; the other logits have a standard deviation of ~3."""
    gen = torch.Generator().manual_seed(H + V)
    X = torch.randn(N70, H + 8, generator=gen).to(BF)
    WT = torch.randn(V, H, generator=gen) * (3.0 / math.sqrt(H))
    bias = 0.5 * torch.randn(V, generator=gen)
    sp = torch.tensor(SPECIAL + [V - 1])
    WT[sp] *= 0.05
    bias[sp] = 7.0
    WT = WT.to(BF)
    Xd, Wd = X[:, :H].double(), WT.double()
    z = Xd @ Wd.T + bias.double()
    e_n = 4 * H * 2.0 ** -24 * (Xd.abs() @ Wd.abs().T).max(1).values
    return X, WT, bias, z, e_n


@functools.lru_cache(maxsize=None)
def _head_case(H, V, live):
    X, WT, bias, z, e_n = _head_operands(H, V)
    r = _rows(D14, V, 7 * H + V, True, dlen=None if live is None else DLEN[live])
    ref = _reference(z, r)
    return r, ref


class _Head:
    """Device buffers of the fused head, allocated once and reused across calls like the engine's."""

    def __init__(self, k, H, V, ldd=None, fill=0.0):
        self.k, self.H, self.V = k, H, V
        X, WT, bias, _, _ = _head_operands(H, V)
        self.X, self.WT, self.bias = X.cuda(), WT.cuda(), bias.cuda()
        N = N70
        self.part = torch.zeros(int(k.vocab_train_tiles(V, H)) * N * 2, device="cuda")
        self.zg, self.lse, self.pv = (torch.zeros(N, device="cuda") for _ in range(3))
        self.loss_row, self.alpha, self.dpre = (torch.full((N,), NAN, device="cuda") for _ in range(3))
        self.dA = torch.full((N, T), NAN, device="cuda")
        self.dl = torch.full((N, ldd or V), fill, dtype=BF, device="cuda")
        self.dbias = torch.zeros(V, device="cuda")

    def run(self, r, vblk=None, vblk_n=None, vlive=None, vstate=None, dbias=True):
        k, H, V, N = self.k, self.H, self.V, N70
        d = _cuda(r)
        k.vocab_train_fwd(self.X, self.WT, self.bias, d["target"], self.part, self.zg, self.lse, self.pv, N, V, H,
                          H + 8, vblk, vblk_n)
        k.ptr_rowfin(self.pv, d["target"], d["rowg"], d["pgen"], d["attn"], d["ext"], d["lens"], self.loss_row,
                     self.alpha, self.dpre, self.dA, N, B, T)
        self.dbias.zero_()
        k.vocab_train_bwd(self.X, self.WT, self.bias, d["target"], self.lse, self.alpha, self.dl,
                          self.dbias if dbias else None, N, V, H, H + 8, vblk, vblk_n, vlive, vstate)
        torch.cuda.synchronize()

    def check_rows(self, tag, ref, live_rows=None):
        """loss_row, alpha, dpre and dA are written for every row (0 on g == 0 rows, dead ones
        included: ptr_rowfin runs over all N rows); lse is defined on the rows of the enumerated
        blocks only (pass 1 skips the others, whose partials are stale)."""
        e_n = _head_operands(self.H, self.V)[4]
        on = ref["on"]
        _check("loss_row", tag, self.loss_row, ref["loss"], 0.0, torch.where(on, e_n + 2e-6, 0.0))
        rows = torch.arange(N70) if live_rows is None else live_rows
        _check("lse", tag, self.lse[rows.cuda()], ref["lse"][rows], 0.0, (e_n + 2e-6)[rows])
        rel = e_n + 2e-5
        _check("alpha", tag, self.alpha, ref["alpha"], rel)
        _check("dpre", tag, self.dpre, ref["dpre"], rel)
        _check("dA", tag, self.dA, ref["dA"], rel[:, None])

    def check_dbias(self, tag, ref):
        dz = ref["dz"]
        _check("dbias", tag, self.dbias, dz.sum(0), 0.0, 2.0 ** -8 * dz.abs().sum(0) + 1e-7)


HV = [(128, 300), (256, 300), (512, 300), (128, 1000), (256, 1000), (512, 1000)]
HV_IDS = [f"H{h}-V{v}" for h, v in HV]


@pytest.mark.parametrize("H,V", HV + [(128, 301), (512, 301)], ids=HV_IDS + ["H128-V301", "H512-V301"])
def test_fused_head_every_block(H, V):
    """Mode 1, no block list: dlogits [N][V] for all 70 rows (a partial last 32-row block, a partial
    last vocab tile at both tile widths; V = 301 adds the per-element store path of V % 4 != 0), the
    row outputs, dbias (atomic mode, pre-zeroed) against the column sums of the reference; then the
    same with a padded row length ldd = 128 ceil(V / 128), whose padding columns stay zero, and with
    dbias = None, which changes nothing in dlogits."""
    k = ops()
    r, ref = _head_case(H, V, None)
    tag = f"fused H={H} V={V} every-block"
    h = _Head(k, H, V, fill=NAN)
    h.run(r)
    h.check_rows(tag, ref)
    _check_dz(tag, h.dl, ref)
    h.check_dbias(tag, ref)
    ldd = 128 * (-(-V // 128))
    hp = _Head(k, H, V, ldd=ldd)
    hp.run(r, dbias=False)
    assert torch.equal(hp.dl[:, :V], h.dl), "padded rows / dbias=None change dlogits"
    assert bool((hp.dl[:, V:] == 0).all()), "padding columns written"
    assert bool((hp.dbias == 0).all())


@pytest.mark.parametrize("H,V", HV, ids=HV_IDS)
def test_fused_head_compacted(H, V):
    """Mode 2, vblk + vblk_n: live block j lands at rows 32 j; rows past the live blocks are not
    written.  First the list host_inputs builds from a dlen with dead steps (blocks 0, 1 live, 2
    dead); then a hand-built list [0, 2] over rows whose block 1 carries no weight, where the
    compaction really moves a block (rows 64..69 -> 32..37)."""
    k = ops()
    r, ref = _head_case(H, V, "A")
    vlive, vblk, vn = _blocks(DLEN["A"], D14)
    assert vlive.tolist() == [1, 1, 0] and vblk.tolist() == [0, 1, 3]
    tag = f"fused H={H} V={V} compacted"
    h = _Head(k, H, V, fill=5.0)
    h.run(r, torch.from_numpy(vblk).cuda(), torch.from_numpy(vn).cuda())
    live_rows = torch.arange(64)
    h.check_rows(tag, ref, live_rows)
    _check_dz(tag, h.dl[:64], ref, live_rows)
    assert bool((h.dl[64:] == 5.0).all()), "rows past the live blocks written"
    h.check_dbias(tag, ref)
    # hand-built: block 1 without weight and not listed
    r2 = dict(_head_case(H, V, None)[0])
    r2["rowg"] = r2["rowg"].clone()
    r2["rowg"][32:64] = 0.0
    ref2 = _reference(_head_operands(H, V)[3], r2)
    assert bool(ref2["on"][64:].any())
    h = _Head(k, H, V, fill=5.0)
    h.run(r2, torch.tensor([0, 2, 3], dtype=torch.int32).cuda(), torch.tensor([2], dtype=torch.int32).cuda())
    live_rows = torch.cat([torch.arange(32), torch.arange(64, 70)])
    h.check_rows(tag + " [0,2]", ref2, live_rows)
    _check_dz(tag + " [0,2]", h.dl[:38], ref2, live_rows)
    assert bool((h.dl[38:] == 5.0).all()), "rows past the live blocks written"
    h.check_dbias(tag + " [0,2]", ref2)


@pytest.mark.parametrize("H,V", HV, ids=HV_IDS)
def test_fused_head_in_place_keeps_dead_blocks_zero(H, V):
    """Mode 3, vlive + vstate: three calls on the SAME buffers with the live sets {0, 1}, {0} and
    {0, 1, 2}.  After each, the live blocks hold this call's dlogits, every dead block reads all
    zero (block 1 was written by call 1 and is dead in call 2) and vstate is the call's vlive."""
    k = ops()
    h = _Head(k, H, V, fill=0.0)
    vstate = torch.zeros(3, dtype=torch.int32, device="cuda")
    for name, nlive in (("A", 2), ("C", 1), ("B", 3)):
        r, ref = _head_case(H, V, name)
        vlive, vblk, vn = _blocks(DLEN[name], D14)
        assert int(vlive.sum()) == nlive == int(vn[0])
        tag = f"fused H={H} V={V} in-place {name}"
        h.run(r, torch.from_numpy(vblk).cuda(), torch.from_numpy(vn).cuda(), torch.from_numpy(vlive).cuda(), vstate)
        nr = min(32 * nlive, N70)
        live_rows = torch.arange(nr)
        h.check_rows(tag, ref, live_rows)
        _check_dz(tag, h.dl[:nr], ref, live_rows)
        assert bool((h.dl[nr:] == 0).all()), "a dead block is not zero"
        assert bool((ref["dz"][nr:] == 0).all())
        assert vstate.cpu().tolist() == vlive.tolist()
        h.check_dbias(tag, ref)
