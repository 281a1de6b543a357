"""The attention kernels (csrc/kernels/attention.hip, attention_row.hip, attn_rowp_fwd.h) one by one
against float64 torch: attn_score + attn_softmax_ctx (multi-block forward), attn_fwd_row, attn_fwd_row_beam,
attn_fwd_rowp, attn_bwd_step, attn_bwd_row, attn_bwd_rowp and attn_bwd_feat.  Every kernel is called through
ops(); no reference goes through the engine or another kernel; bf16 operands are upcast; every reference is
evaluated on exactly the values the kernel receives.

Semantics (header comments of attention.hip / attention_row.hip).  Row b of B, feature row fr = b / rep (the rep
hypotheses of an article share F and E), position i < len_fr, feature k < A:

    u_ik  = F_k[fr][i][k] / (2 log2 e) + s[b][k] + w_c[k] cov[b][i]      (F_k: the kernel operand, stored x 2 log2 e)
    e_i   = sum_k v_k tanh(u_ik)
    a     = softmax of e over i < len, 0 at i >= len ; a row of length 1 has a == 1.0 exactly
    ctx   = sum_i a_i E[fr][i]            (projected form: g = sum_i a_i G[b][i], G [B][T][128])
    cov'  = cov + a  (= cov bit for bit at i >= len) ; covloss = sum_i min(a_i, cov_i)
    beam  : cov = cov_src[g] + a_src[g], g = gidx[b]; cov_keep receives it at every i < T; no cov' / covloss

    r_i   = Ga_i + dcov_next_i + g_cl [a_i <= cov_i]                     (a, cov are INPUTS of the backward)
    da_i  = r_i + dctx . E_i                                             (projected form: da_i = r_i + dx . G_i)
    S     = sum_j a_j r_j + dctx . ctx                                   (the ctx / gv that is PASSED IN; dx = None: no term)
    de_i  = a_i (da_i - S)                       , 0 at i >= len
    ds_k  = v_k sum_i de_i sech^2(u_ik)          (attn_bwd_step ADDS it into ds, the row kernels store it)
    dcov_i= dcov_next_i + g_cl [a_i > cov_i] + de_i sum_k v_k w_k sech^2(u_ik)   , dcov_next_i bit for bit at i >= len
    rowp, step >= dlen[b] (dead row): forward a = g = covloss = 0 and cov' = cov; backward de = ds = dcov = 0

attn_bwd_feat, over the D steps t (step t of row b counts while t < dlen[b]; de_all is zero past it):
    dF[b][i][k] = v_k sum_t de[t][b][i] sech^2(u_tik)     (r-form: 4 v sum de r (1 - r)), 0 at i >= len
    dv_k        = sum_{t,b,i} de tanh(u_tik)              (r-form: sum de - 2 sum de r)
    dwc_k       = v_k sum_{t,b,i} de cov sech^2(u_tik)    (r-form: 4 v sum de cov r (1 - r))
dv / dwc arrive as [nslot][A] partial rows; the reference is the slot sum.  dF is the gradient of the loss with
respect to the UNSCALED feature W_h enc_out = F_k / (2 log2 e), the additive term of u: attn_bwd_feat_kernel
accumulates v sech^2(u) de with no factor 2 log2 e, and pointer_generator.py multiplies it by the unscaled W_h
(dW_h = enc_out^T dF, dE += dF W_h^T), not by the scaled operand of the F GEMM.

Inputs are dyadic where that buys exactness: bf16 operands multiples of 1/16 (F_k in [-1, 1], E / G in [-2, 2], w_c
in [-1/4, 1/4]; v multiples of 1/64 in [-1/16, 1/16], in the wide-score cases of 1/16 up to 256 / A), fp32 addends
(s, cov, Ga, dcov_next, g_cl, the ctx / gv passed in, the ds prefill) multiples of 2^-10, dctx / dx multiples of 1/64
in [-1, 1].  dctx . E_i and dx . G_i are then exact in fp32 in any order (_assert_exact on the reference) and get no
accumulation allowance; r_i and r_i + dot_i are exact too.  a (backward) is a general fp32 softmax output.

Bounds (absolute, per element; d. is the bound of .; U = 2^-24).  A sum of K fp32 terms in any order is off by at most
(K + 4) U sum |terms|; the 4 counts the products' own roundings where they are not fused, the merge of the partial
sums of lanes / waves / blocks, and the final scale or subtraction (two roundings).
    argument: y = F_k + (2 log2 e)(s + w cov) costs four roundings, du = 4 U (|F_k| / (2 log2 e) + |s| + |w cov|);
              tanh and sech^2 are 1-Lipschitz, so d tanh, d sech^2 <= du
    e     : (2A + 4) U sum_k |v_k| (1 + 2 r_k) + sum_k |v_k| du_ik + 8 TAB[e] sum |v|       (terms v_k and 2 v_k r_k)
    a     : a_i (exp(2 max_j de_j) - 1) + a_i ((len + 4) U + 8 TAB[a] (1 + m - e_i)) + 2^-126  (the sum and the
            division; exp of an argument rounded at magnitude m - e_i; fp32 exp2 flushes below 2^-126)
    ctx, g: sum_i da_i |E_ik| + ((len + 4) U + 8 TAB[ctx]) sum_i a_i |E_ik|
    cov'  : da_i + U |cov'| ; covloss: sum_i da_i + (T + 4) U covloss
    S     : (len + width + 4) U (sum_j |a_j r_j| + sum_k |dctx_k ctx_k|)
    de    : a_i (dS + 3 U (|r_i + dot_i| + |S|)) + U |de_i|
    ds    : |v_k| sum_i (d de_i sech^2 + |de_i| du_ik) + (len + blocks + 4) U (|v_k| sum_i |de_i| sech^2 + |prefill|)
            + 8 TAB[ds] |v_k| sum_i |de_i|
    dcov  : d de_i |h_i| + |de_i| ((A + 4) U sum_k |v_k w_k| sech^2 + sum_k |v_k w_k| du_ik + 8 TAB[dcov] sum_k |v_k w_k|)
            + 3 U (|dcov_next_i| + g_cl + |de_i h_i|),   h_i = sum_k v_k w_k sech^2(u_ik)
    dF    : |v_k| ((D + 4) U sum_t |de_t| sech^2 + sum_t |de_t| du + 8 TAB[dF] sum_t |de_t|) + 2^-8 |ref|
    dv    : (2N + workgroups + 4) U sum |de| (2 - tanh) + sum |de| du + 8 TAB[dv] sum |de|       (N terms (t, b, i))
    dwc   : |v_k| ((N + workgroups + 5) U sum |de cov| sech^2 + sum |de cov| du + 8 TAB[dwc] sum |de cov|)
bf16 outputs (ctx_bf, gx_bf, a_bf, dF) get 2^-8 |ref| more; ctx_bf, gx_bf and a_bf must also equal their fp32 twin
rounded, bit for bit.  TAB is FP32_TORCH_ERR below: the error of the kernel's own formulas (r = 1 / (1 + 2^y),
tanh = 1 - 2r, sech^2 = 4 r (1 - r), e = sum v - 2 sum v r, the online-softmax merge of per-wave (max, sum, context)
partials) in fp32 torch on the CPU against float64, divided by the scale it multiplies above, maximum over this
module's cases; running this file as a script reprints it (no GPU needed).  The softmax entries are measured
teacher-forced (from the emulation's own e), so they hold the softmax arithmetic alone.
attn_softmax_ctx is judged from the kernel's own e (teacher forcing: no d e term); the row kernels keep e in LDS
and are judged end to end.  In the backward [a <= cov] is exact (inputs; rows with designed ties a_i == cov_i and a row
with cov == 0); in the forward min(a, cov) is continuous.
"""
import functools
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
BF = torch.bfloat16
F64 = torch.float64
SENT = 12288.0  # trailing sentinel blocks (exact in bf16)
PAD = 4096
KF = 2.8853900817779268  # 2 log2(e)
L2E = 1.4426950408889634
U24 = 2.0 ** -24
EG = 128
ROW_MAX_T = 2048  # kRowMaxT (attn_rowp_fwd.h)
FLUSH = 2.0 ** -126 * 2 * ROW_MAX_T  # the table ignores errors below it: sum_i 2^-126 |E_ik| at its largest

# max over the cases of this module of |fp32 torch - float64| / scale (module docstring), measured on the CPU:
# see __main__
FP32_TORCH_ERR = {"e": 2.73e-7, "a": 2.04e-7, "ctx": 2.61e-7,                       # forward
                  "ds": 5.99e-7, "dcov": 5.10e-8, "dF": 4.08e-7, "dv": 1.27e-7, "dwc": 7.79e-8}  # backward
BOUND = {q: 8.0 * e for q, e in FP32_TORCH_ERR.items()}


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


# ------------------------------------------------------------------ dyadic inputs
def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ri(g, lo, hi, shape, den):
    """multiples of 1 / den in [lo / den, hi / den]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float() / den


def _assert_exact(ref, mag):
    """The exactness premise of a linear output: every term a multiple of 2^-10 (so is the sum) and
    sum |terms| < 2^14, i.e. every partial sum has at most 24 bits: exact in fp32 in any order."""
    assert float(mag.max()) < 2 ** 14
    assert torch.equal((ref * 1024).round(), ref * 1024)
    assert torch.equal(ref.float().double(), ref)


def _lens(g, n, T, bounds):
    """n lengths in [1, T]: 2, 3, 4, 5, one on each side of every boundary, T - 1 and T are present; row 0 is T
    and the last row 1."""
    want = []
    for v in [T, 2, 3, 4, 5] + [w for b in bounds for w in (b, b + 1)] + [T - 1]:
        if 1 <= v <= T and v not in want:
            want.append(v)
    tail = [] if 1 in want else [1]
    fill = n - len(want) - len(tail)
    assert fill >= 0, (n, want)
    mid = [T] * min(fill, 1) + torch.randint(1, T + 1, (max(fill - 1, 0),), generator=g).tolist()
    return torch.tensor(want + mid + tail, dtype=torch.int32)


def _saturate(s, A):
    """A few features whose 2^y saturates: r = 1 / (1 + 2^y) is 0 or 1 to fp32 at |s| = 40, and 2^y itself
    overflows to inf / underflows to 0 at |s| = 64 (y = +-185)"""
    s[..., 3], s[..., A // 2 + 1], s[..., A - 2], s[..., A // 4] = 40.0, -40.0, 64.0, -64.0
    return s


def _v(g, A, wide):
    return _ri(g, -_vmax16(A), _vmax16(A), (A,), 16) if wide else _ri(g, -4, 4, (A,), 64)


def _vmax16(A):
    """wide-score cases: v multiples of 1/16 up to 256 / A, so that sum |v| is about 128 at every A"""
    return max(4096 // A, 1)


def _mask(lens, T):
    return torch.arange(T)[None, :] < lens.long()[:, None]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------ forward: cases, reference, emulation, checks
@functools.lru_cache(maxsize=3)
def _fwd_case(A, Na, rep, T, cov, EW, bounds=(), wide=False, lens=None):
    """F_k [Na][T][A], E (or G) [Na][T][EW], s / cov [B][..] for the B = Na rep hypothesis rows.  wide: large v, and
    one article whose features alternate +-8 sign(v) by position, so that its scores span more than 100."""
    g = _gen(A, Na, rep, T, int(cov), EW, int(wide), 1)
    B = Na * rep
    x = {"A": A, "Na": Na, "rep": rep, "T": T, "B": B, "EW": EW, "cov_on": cov, "wide": wide}
    x["lens"] = torch.tensor(lens, dtype=torch.int32) if lens else _lens(g, Na, T, bounds)
    x["F"] = _ri(g, -16, 16, (Na, T, A), 16)
    x["E"] = _ri(g, -32, 32, (Na, T, EW), 16).bfloat16()
    x["s"] = _saturate(_ri(g, -1024, 1024, (B, A), 1024), A)
    x["v"] = _v(g, A, wide)
    x["wc"] = _ri(g, -4, 4, (A,), 16) if cov else torch.zeros(A)
    x["cov"] = _ri(g, 0, 1024, (B, T), 1024) if cov else torch.zeros(B, T)
    if B > 1:
        x["cov"][1] = 0.0  # the first decoder step has zero coverage
    if wide:
        art = int((x["lens"] == T).nonzero()[-1])
        sign = torch.where(x["v"] >= 0, 1.0, -1.0)
        alt = torch.where(torch.arange(T) % 2 == 0, 8.0, -8.0)
        x["F"][art] += alt[:, None] * sign[None, :]
        x["span_rows"] = list(range(art * rep, art * rep + rep))
    x["F"] = x["F"].bfloat16()
    assert torch.equal(x["F"].float().bfloat16(), x["F"])
    return x


def _rows(x):
    """hypothesis row -> feature row"""
    return torch.arange(x["B"]) // x["rep"]


def _u64(F, rows, s, wc, cov):
    return F.double()[rows] / KF + s.double()[:, None, :] + wc.double()[None, None, :] * cov.double()[:, :, None]


def _du(F, rows, s, wc, cov, w):
    """sum_k w_k du_ik [B][T] for non-negative weights w [A]: the four roundings of the score argument"""
    w = w.double()
    return 4 * U24 * ((F.double().abs() @ w)[rows] / KF + (s.double().abs() @ w)[:, None]
                      + cov.double().abs() * float((wc.double().abs() * w).sum()))


def _softmax_ref(x, e, be):
    """float64 a, ctx, cov', covloss and their bounds from the scores e [B][T] (the reference's, with their bound
    be, or the kernel's own, be = None)"""
    Na, rep, T, B, EW = x["Na"], x["rep"], x["T"], x["B"], x["EW"]
    rl = x["lens"].long().repeat_interleave(rep)
    mask = _mask(rl, T)
    em = e.masked_fill(~mask, -INF)
    m = em.max(1, keepdim=True)[0]
    a = torch.softmax(em, 1)
    rel = (rl[:, None] + 4) * U24 + BOUND["a"] * (1 + (m - em).masked_fill(~mask, 0.0))
    if be is not None:
        rel = rel + torch.expm1(2 * be.masked_fill(~mask, 0.0).max(1, keepdim=True)[0])
    ba = (a * rel + 2.0 ** -126) * mask
    E = x["E"].double()
    ctx = torch.einsum("nrt,ntk->nrk", a.view(Na, rep, T), E).reshape(B, EW)
    sc = torch.einsum("nrt,ntk->nrk", a.view(Na, rep, T), E.abs()).reshape(B, EW)
    bctx = torch.einsum("nrt,ntk->nrk", ba.view(Na, rep, T), E.abs()).reshape(B, EW) + ((rl[:, None] + 4) * U24 + BOUND["ctx"]) * sc
    cov = x["cov"].double()
    cl = torch.minimum(a, cov).sum(1)
    return {"mask": mask, "m": m, "a": a, "ba": ba, "ctx": ctx, "bctx": bctx, "sctx": sc, "cov_out": cov + a,
            "bcov_out": ba + U24 * (cov + a).abs(), "covloss": cl, "bcovloss": ba.sum(1) + (T + 4) * U24 * cl}


def _fwd_ref(x):
    if "ref" not in x:
        A, rows = x["A"], _rows(x)
        th = torch.tanh(_u64(x["F"], rows, x["s"], x["wc"], x["cov"]))
        v = x["v"].double()
        e = th @ v
        mag = (2.0 - th) @ v.abs()  # sum |v_k| (1 + 2 r_k), 2 r = 1 - tanh
        del th
        se = float(v.abs().sum())
        be = (2 * A + 4) * U24 * mag + _du(x["F"], rows, x["s"], x["wc"], x["cov"], v.abs()) + BOUND["e"] * se
        x["ref"] = {"e": e, "be": be, "se": se, "sm": _softmax_ref(x, e, be)}
        if x["wide"]:
            for b in x["span_rows"]:
                n = int(x["lens"][b // x["rep"]])
                assert n < 2 or float(e[b, :n].max() - e[b, :n].min()) > 100.0, "the wide row's scores span less than 100"
    return x["ref"]


def _fwd_errors(x, got, teacher=False):
    """Bit-exact properties of one forward result (asserted) and {quantity: (err, bound, scale)} over EVERY
    element.  got: a, ctx and optionally e, ctx_bf, a_bf, cov_out, covloss (ctx / ctx_bf are g / g_bf of the
    projected kernel).  teacher: the softmax is judged from got's own e."""
    ref = _fwd_ref(x)
    sm = _softmax_ref(x, got["e"].double(), None) if teacher else ref["sm"]
    mask, res = sm["mask"], {}
    if "e" in got:
        assert bool(torch.isnan(got["e"][~mask]).all()), "e past the length was written"
        z = torch.zeros((), dtype=F64)
        res["e"] = (torch.where(mask, (got["e"].double() - ref["e"]).abs(), z), torch.where(mask, ref["be"], z), ref["se"])
    a = got["a"]
    assert bool((a[~mask] == 0).all()), "a past the length is not zero"
    one = x["lens"].long().repeat_interleave(x["rep"]) == 1
    assert bool((a[one, 0] == 1.0).all()), "a row of length 1 does not have a == 1.0"
    scale_a = sm["a"] * (1 + (sm["m"] - got["e"].double())) if teacher else None
    res["a"] = ((a.double() - sm["a"]).abs(), sm["ba"], scale_a)
    res["ctx"] = ((got["ctx"].double() - sm["ctx"]).abs(), sm["bctx"], sm["sctx"])
    if "ctx_bf" in got:
        assert torch.equal(_bits(got["ctx_bf"]), _bits(got["ctx"].bfloat16())), "ctx_bf != ctx rounded to bf16"
        res["ctx_bf"] = (_beyond_bf16(got["ctx_bf"], sm["ctx"]), sm["bctx"], None)
    if "a_bf" in got:
        assert torch.equal(_bits(got["a_bf"]), _bits(a.bfloat16())), "a_bf != a rounded to bf16"
        res["a_bf"] = (_beyond_bf16(got["a_bf"], sm["a"]), sm["ba"], None)
    if "cov_out" in got:
        assert torch.equal(_bits(got["cov_out"])[~mask], _bits(x["cov"])[~mask]), "cov_out past the length != cov"
        res["cov_out"] = ((got["cov_out"].double() - sm["cov_out"]).abs(), sm["bcov_out"], None)
        res["covloss"] = ((got["covloss"].double() - sm["covloss"]).abs(), sm["bcovloss"], None)
    return res


def _beyond_bf16(got, ref):
    """the error of a bf16 output beyond its own rounding 2^-8 |ref|, to be held to the rest of its bound"""
    return ((got.double() - ref).abs() - 2.0 ** -8 * ref.abs()).clamp_min(0.0)


def _note(tag, q, ratio):
    print(f"[attn-ops] {tag}: {q} err/bound={float(ratio):.3g}")


def _assert_bounds(tag, res):
    for q, (err, bound, _) in res.items():
        if bound is None:
            continue
        ok = bound > 0
        ratio = torch.where(ok, err / bound.clamp_min(1e-300), torch.where(err > 0, INF, 0.0).to(F64)).max()
        _note(tag, q, ratio)
        assert float(ratio) <= 1.0, (tag, q, float(ratio))


def _rsig32(y):
    return 1.0 / (1.0 + torch.exp2(y))


def _y32(F, rows, s, wc, cov, mut=None):
    """the kernels' score argument in fp32: F_k + ((2 log2 e) w cov + (2 log2 e) s)"""
    t = s[:, None, :] * KF
    if mut != "no_wc_cov":
        t = (wc * KF)[None, None, :] * cov[:, :, None] + t
    F = F.float()[rows]
    return (F * KF if mut == "F_not_scaled_back" else F) + t


def _emul_fwd(x, mut=None, nw=16):
    """The forward with the kernels' formulas in fp32 torch on the CPU (the bound table, and the stand-in
    kernel of the mutation checks): r-form scores, then the online softmax as nw per-wave (max, sum, context)
    partials over the 4-position groups dealt round-robin, merged as the row kernels merge them."""
    Na, rep, T, B, EW = x["Na"], x["rep"], x["T"], x["B"], x["EW"]
    rows = torch.arange(B) % rep if mut == "b_mod_rep" else _rows(x)
    v, cov = x["v"], x["cov"]
    r = _rsig32(_y32(x["F"], rows, x["s"], x["wc"], cov, mut))
    e = v.sum() - 2.0 * (r @ v)
    del r
    rl = x["lens"].long()[rows]
    pos = torch.arange(T)[None, :]
    mask = (pos <= rl[:, None]) if mut == "mask_le" else (pos < rl[:, None])
    if mut == "mask_le":
        mask = mask & (pos < T)
    wv = (torch.arange(T) // 4) % nw
    em = e.masked_fill(~mask, -INF)
    E = x["E"].float()[rows]
    mw = torch.stack([em[:, wv == w].max(1)[0] if bool((wv == w).any()) else torch.full((B,), -INF) for w in range(nw)], 1)
    mwp = mw[:, wv]
    p = torch.where(mask, torch.exp2((em - torch.where(mwp == -INF, 0.0, mwp)) * L2E), 0.0)
    m = mw.max(1, keepdim=True)[0]
    wsc = torch.where(mw == -INF, 0.0, torch.exp2((mw - m) * L2E))
    L = torch.zeros(B)
    ctx = torch.zeros(B, EW)
    for w in range(nw):
        pw = p * (wv == w)
        L = L + pw.sum(1) * wsc[:, w]
        ctx = ctx + torch.einsum("bt,btk->bk", pw, E) * wsc[:, w:w + 1]
    inv = 1.0 / L
    a = torch.where(mask, torch.exp2((em - m) * L2E) * inv[:, None], 0.0)
    ctx = ctx * inv[:, None]
    got = {"e": e.masked_fill(~mask, NAN), "a": a, "ctx": ctx, "ctx_bf": ctx.bfloat16(), "a_bf": a.bfloat16()}
    if x["cov_on"]:
        got.update(cov_out=cov + a, covloss=torch.minimum(a, cov).sum(1))
    return got


# ------------------------------------------------------------------ device buffers
def _dev_buf(shape, dtype, fill):
    """A device tensor prefilled with ``fill`` and the sentinel block allocated behind it"""
    n = 1
    for v in shape:
        n *= v
    full = torch.full((n + PAD,), SENT, dtype=dtype, device="cuda")
    full[:n].fill_(fill)
    return full[:n].view(shape), full[n:]


class _Outs:
    """NaN-prefilled outputs, each with its sentinel block"""

    def __init__(self):
        self.t, self.tails = {}, []

    def new(self, name, shape, dtype=torch.float32, fill=NAN):
        buf, tail = _dev_buf(shape, dtype, fill)
        self.t[name] = buf
        self.tails.append(tail)
        return buf

    def cpu(self):
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in self.tails), "a sentinel block behind an output was written"
        return {n: b.cpu() for n, b in self.t.items()}


def _cu(x, *names):
    return [x[n].cuda() for n in names]


def _cov_args(x, zeros):
    """(w_c, cov) as the model passes them: None without coverage; zeros: zero tensors in their place"""
    if x["cov_on"] or zeros:
        return x["wc"].cuda(), x["cov"].cuda()
    return None, None


def _run_score_ctx(k, x, zeros=False):
    """attn_score, then attn_softmax_ctx on the e it wrote"""
    A, T, B, rep = x["A"], x["T"], x["B"], x["rep"]
    Ft = x["F"].transpose(1, 2).contiguous().cuda()  # [Na][A][T]
    E, s, v, lens = _cu(x, "E", "s", "v", "lens")
    wc, cov = _cov_args(x, zeros)
    o = _Outs()
    e, a, ctx, cb = o.new("e", (B, T)), o.new("a", (B, T)), o.new("ctx", (B, A)), o.new("ctx_bf", (B, A), BF)
    co, cl = (o.new("cov_out", (B, T)), o.new("covloss", (B,))) if cov is not None else (None, None)
    k.attn_score(Ft, s, v, wc, cov, lens, e, B, T, A, rep)
    k.attn_softmax_ctx(e, E, lens, cov, a, co, cl, ctx, cb, B, T, A, rep)
    return o.cpu()


def _run_fwd_row(k, x, zeros=False, beam=None):
    """attn_fwd_row; beam = (cov_src, a_src, gidx): attn_fwd_row_beam"""
    A, T, B, rep = x["A"], x["T"], x["B"], x["rep"]
    F, E, s, v, lens = _cu(x, "F", "E", "s", "v", "lens")
    wc, cov = _cov_args(x, zeros)
    o = _Outs()
    a, ctx, cb = o.new("a", (B, T)), o.new("ctx", (B, A)), o.new("ctx_bf", (B, A), BF)
    if beam is not None:
        keep = o.new("cov_keep", (B, T)) if x["cov_on"] else None
        src = [t.cuda() for t in beam[:2]] if x["cov_on"] else [None, None]
        k.attn_fwd_row_beam(F, E, s, v, wc, src[0], src[1], keep, beam[2].cuda(), lens, a, ctx, cb, B, T, A, rep)
    else:
        co, cl = (o.new("cov_out", (B, T)), o.new("covloss", (B,))) if cov is not None else (None, None)
        k.attn_fwd_row(F, E, s, v, wc, cov, lens, a, co, cl, ctx, cb, B, T, A, rep)
    return o.cpu()


def _run_fwd_rowp(k, x, zeros=False, dlen=None, step=0):
    A, T, B = x["A"], x["T"], x["B"]
    F, G, s, v, lens = _cu(x, "F", "E", "s", "v", "lens")
    wc, cov = _cov_args(x, zeros)
    o = _Outs()
    a, ab = o.new("a", (B, T)), o.new("a_bf", (B, T), BF)
    gx, gb = o.new("ctx", (B, EG)), o.new("ctx_bf", (B, EG), BF)
    co, cl = (o.new("cov_out", (B, T)), o.new("covloss", (B,))) if cov is not None else (None, None)
    k.attn_fwd_rowp(F, G, s, v, wc, cov, lens, a, co, cl, gx, gb, B, T, A, None if dlen is None else dlen.cuda(), step, ab)
    return o.cpu()


def _same_bits(p, q, names, why):
    for n in names:
        assert torch.equal(_bits(p[n]), _bits(q[n])), (n, why)


# ------------------------------------------------------------------ forward tests
# (A, Na, rep, T, coverage, wide scores); grid = ceil(T / 128) * Na blocks, reordered over the XCDs when % 8 == 0;
# rep > 1 and A % 128 == 0: the 16-wave score kernel, otherwise the 8-wave one
SCORE = [(64, 16, 1, 300, True, True), (128, 10, 1, 300, False, False), (512, 8, 2, 130, True, False),
         (1024, 9, 4, 300, True, True), (64, 4, 4, 2, True, False), (512, 8, 4, 2, False, True),
         (1024, 9, 1, 130, False, False), (128, 10, 2, 300, True, False),
         (64, 2, 4, 1024, True, False), (64, 5, 1, 2048, True, True)]


def _score_id(c):
    A, Na, rep, T, cov, wide = c
    blocks = (T + 127) // 128 * Na
    return (f"A{A}-{'16w' if rep > 1 and A % 128 == 0 else '8w'}-rep{rep}-T{T}-blocks{blocks}"
            f"{'-xcd' if blocks % 8 == 0 else '-plain'}{'-cov' if cov else '-nocov'}{'-wide' if wide else ''}")


def _score_case(A, Na, rep, T, cov, wide):
    if T > 300:  # the caps: a handful of rows
        lens = {1024: (1024, 1023), 2048: (2048, 1, 2047, 1025, 2048)}[T]
        return _fwd_case(A, Na, rep, T, cov, A, (), wide, lens)
    return _fwd_case(A, Na, rep, T, cov, A, (128,), wide)


@pytest.mark.parametrize("case", SCORE, ids=_score_id)
def test_attn_score_softmax_ctx(case):
    """The multi-block forward.  e is judged on its own (and is left unwritten past the length), then
    attn_softmax_ctx from the e it read.  Without coverage w_c, cov, cov_out and covloss are None; zero tensors
    in their place give the same e, a and ctx bits."""
    k, x = _ops(), _score_case(*case)
    got = _run_score_ctx(k, x)
    _assert_bounds(f"score+softmax_ctx {_score_id(case)}", _fwd_errors(x, got, teacher=True))
    if not x["cov_on"]:
        _same_bits(got, _run_score_ctx(k, x, zeros=True), ("e", "a", "ctx", "ctx_bf"), "None vs zero coverage tensors")


# (A, Na, rep, T, wide); rep > 1: Na = 8 takes the XCD-grouped row map (B % 8 == 0 and (B / 8) % rep == 0), Na = 7
# the identity map; A = 512: 16 waves at rep = 1, 12 waves at rep > 1; A = 1024: 8 waves
FWD_ROW = [(512, 9, 1, 300, True), (512, 8, 4, 300, False), (512, 7, 4, 300, False), (512, 8, 3, 7, False),
           (512, 7, 10, 7, False), (512, 8, 16, 7, True), (512, 2, 16, 1, False), (1024, 9, 1, 300, False),
           (1024, 8, 4, 300, True), (1024, 7, 3, 7, False), (1024, 8, 10, 1, False), (1024, 7, 16, 7, False),
           (512, 2, 1, ROW_MAX_T, False), (1024, 2, 1, ROW_MAX_T, False)]


def _row_id(c):
    A, Na, rep, T, wide = c
    B = Na * rep
    xcd = rep > 1 and B % 8 == 0 and (B // 8) % rep == 0
    waves = 8 if A == 1024 else (12 if rep > 1 else 16)
    return f"A{A}-{waves}w-rep{rep}-rows{B}-{'xcd' if xcd else 'identity'}-T{T}{'-wide' if wide else ''}"


def _row_case(A, Na, rep, T, wide, cov=True, EW=None):
    waves = 8 if A == 1024 else (12 if rep > 1 else 16)
    lens = (T, T - 3) if T == ROW_MAX_T else ((1,) * Na if T == 1 else None)
    return _fwd_case(A, Na, rep, T, cov, EW or A, (4 * waves,) if Na >= 9 else (), wide, lens)


@pytest.mark.parametrize("case", FWD_ROW, ids=_row_id)
def test_attn_fwd_row(case):
    k, x = _ops(), _row_case(*case)
    assert bool(k.attn_row_ok(x["A"], x["T"])) and not bool(k.attn_row_ok(x["A"], ROW_MAX_T + 1))
    _assert_bounds(f"fwd_row {_row_id(case)}", _fwd_errors(x, _run_fwd_row(k, x)))


@pytest.mark.parametrize("A", [512, 1024])
def test_attn_fwd_row_without_coverage(A):
    """w_c, cov, cov_out, covloss = None (the no-coverage model): a and ctx within bound, and the same bits as
    with zero tensors in their place."""
    k, x = _ops(), _row_case(A, 8, 4, 41, False, cov=False)
    got = _run_fwd_row(k, x)
    assert "cov_out" not in got
    _assert_bounds(f"fwd_row nocov A={A}", _fwd_errors(x, got))
    _same_bits(got, _run_fwd_row(k, x, zeros=True), ("a", "ctx", "ctx_bf"), "None vs zero coverage tensors")


def test_attn_fwd_row_12_waves_and_16_waves_meet_one_reference():
    """A = 512: rep = 4 takes the 12-wave kernel; the same rows with F / E written out per hypothesis at rep = 1
    take the 16-wave one.  Both meet the one float64 reference."""
    k, x = _ops(), _row_case(512, 8, 4, 300, False)
    _assert_bounds("fwd_row 12 waves (rep=4)", _fwd_errors(x, _run_fwd_row(k, x)))
    rows = _rows(x)
    x1 = dict(x, Na=x["B"], rep=1, F=x["F"][rows].contiguous(), E=x["E"][rows].contiguous(), lens=x["lens"][rows].contiguous())
    x1.pop("ref", None)
    got = _run_fwd_row(k, x1)
    _assert_bounds("fwd_row 16 waves (rep=1), its own reference", _fwd_errors(x1, got))
    _assert_bounds("fwd_row 16 waves (rep=1), the rep=4 reference", _fwd_errors(x, got))


def _beam_inputs(x):
    """cov_src, a_src (multiples of 2^-10: their sum is exact) and a non-identity gidx with repeated parents
    inside each article; x's cov becomes the gathered coverage"""
    g = _gen(x["A"], x["B"], 9)
    B, T, rep = x["B"], x["T"], x["rep"]
    cov_src, a_src = _ri(g, 0, 1024, (B, T), 1024), _ri(g, 0, 256, (B, T), 1024)
    gidx = (torch.arange(B) // rep) * rep + torch.randint(0, rep, (B,), generator=g)
    gidx[0], gidx[1], gidx[2] = 1, 1, 0
    assert not torch.equal(gidx, torch.arange(B)) and gidx.unique().numel() < B
    gidx = gidx.int()
    xb = {n: t for n, t in x.items() if n != "ref"}
    xb["cov"] = cov_src[gidx.long()] + a_src[gidx.long()]
    return xb, (cov_src, a_src, gidx)


@pytest.mark.parametrize("A", [512, 1024])
def test_attn_fwd_row_beam(A):
    """cov = cov_src[g] + a_src[g] feeds the scores and lands in cov_keep bit for bit at every position; no
    cov_out / covloss.  The no-coverage form (cov_src, a_src, cov_keep = None) equals attn_fwd_row's."""
    k = _ops()
    xb, beam = _beam_inputs(_row_case(A, 8, 4, 41, False))
    got = _run_fwd_row(k, xb, beam=beam)
    assert torch.equal(_bits(got.pop("cov_keep")), _bits(xb["cov"])), "cov_keep != cov_src[gidx] + a_src[gidx]"
    _assert_bounds(f"fwd_row_beam A={A}", _fwd_errors(xb, got))
    xn = _row_case(A, 8, 4, 41, False, cov=False)
    gn = _run_fwd_row(k, xn, beam=beam)
    _assert_bounds(f"fwd_row_beam nocov A={A}", _fwd_errors(xn, gn))
    _same_bits(gn, _run_fwd_row(k, xn), ("a", "ctx", "ctx_bf"), "beam form without coverage vs attn_fwd_row")


ROWP = [(512, 300, True), (512, 300, False), (1024, 300, True), (1024, 41, False), (512, 7, True), (1024, 1, True)]


@pytest.mark.parametrize("A,T,cov", ROWP)
def test_attn_fwd_rowp(A, T, cov):
    """g = sum_i a_i G_i, a and its bf16 twin, coverage; then dlen / step: dead rows (step >= dlen) write exact
    zeros and pass the coverage through, live rows keep the bits of the dlen = None run."""
    k = _ops()
    assert bool(k.attn_rowp_ok(A, T, EG)) and not bool(k.attn_rowp_ok(A, T, 64))
    Na = 9 if T == 300 else 8
    x = _row_case(A, Na, 1, T, T == 300 and A == 512, cov=cov, EW=EG)
    got = _run_fwd_rowp(k, x)
    _assert_bounds(f"fwd_rowp A={A} T={T} cov={cov}", _fwd_errors(x, got))
    if not cov:
        _same_bits(got, _run_fwd_rowp(k, x, zeros=True), ("a", "a_bf", "ctx", "ctx_bf"), "None vs zero coverage tensors")
    step = 3
    for name, dlen in (("mixed", torch.tensor([0, 3, 4, 100, 2, 9, 3, 4, 1][:Na])), ("dead", torch.zeros(Na)), ("live", torch.full((Na,), 4))):
        dlen = dlen.int()
        run = _run_fwd_rowp(k, x, dlen=dlen, step=step)
        dead = step >= dlen.long()
        for n, t in run.items():
            want = x["cov"] if n == "cov_out" else torch.zeros_like(t)
            assert torch.equal(_bits(t[dead]), _bits(want.to(t.dtype)[dead])), (name, n, "dead row")
            assert torch.equal(_bits(t[~dead]), _bits(got[n][~dead])), (name, n, "live row changed by dlen")


# ------------------------------------------------------------------ backward: cases, reference, emulation, checks
@functools.lru_cache(maxsize=3)
def _bwd_case(A, B, T, EW, cov, bounds=()):
    """E-form (EW = A: dctx, ctx) or projected form (EW = 128: dx, gv).  Rows b % 3 == 0 have exact ties
    a_i == cov_i at every third position, row 1 has cov == 0, row 2 a softmax peaked until its tail underflows
    to exact zeros; a, cov, Ga past the length hold finite junk."""
    g = _gen(A, B, T, EW, int(cov), 2)
    x = {"A": A, "B": B, "T": T, "EW": EW, "cov_on": cov, "rep": 1, "lens": _lens(g, B, T, bounds)}
    mask = _mask(x["lens"], T)
    x["F"] = _ri(g, -16, 16, (B, T, A), 16).bfloat16()
    x["E"] = _ri(g, -32, 32, (B, T, EW), 16).bfloat16()
    x["s"] = _saturate(_ri(g, -1024, 1024, (B, A), 1024), A)
    x["v"] = _ri(g, -8, 8, (A,), 16)
    x["wc"] = _ri(g, -4, 4, (A,), 16) if cov else torch.zeros(A)
    logits = 2.0 * torch.randn(B, T, generator=g)
    if B > 2:
        logits[2] *= 60.0
    a = torch.softmax(logits.masked_fill(~mask, -INF), 1)
    c = _ri(g, 0, 1024, (B, T), 1024) * (2.0 / x["lens"].float())[:, None]  # of the size of a
    if cov:
        c[0::3, 0::3] = a[0::3, 0::3]
        if B > 1:
            c[1] = 0.0
    else:
        c = torch.zeros(B, T)
    x["a"], x["cov"] = torch.where(mask, a, torch.full_like(a, 0.25)), c
    x["vec"] = _ri(g, -64, 64, (B, EW), 64)          # dctx / dx
    x["cvec"] = _ri(g, -2048, 2048, (B, EW), 1024)   # the ctx / gv that is passed in
    x["Ga"], x["dn"] = _ri(g, -1024, 1024, (B, T), 1024), _ri(g, -1024, 1024, (B, T), 1024)
    x["gcl"] = _ri(g, 1, 1024, (B,), 1024)
    x["ds0"] = _ri(g, -1024, 1024, (B, A), 1024)     # attn_bwd_step adds into ds
    return x


def _bwd_ref(x, key="ref", vec=True, Ga=True, dn=True, gcl=True):
    """float64 de, ds, dcov with their bounds (module docstring); the switches drop optional arguments"""
    if key in x:
        return x[key]
    A, B, T, EW = x["A"], x["B"], x["T"], x["EW"]
    ln = x["lens"].long()[:, None]
    mask = _mask(x["lens"], T)
    z = torch.zeros(B, T, dtype=F64)
    a, cov = x["a"].double() * mask, x["cov"].double()
    Gav, dnv = (x["Ga"].double() if Ga else z), (x["dn"].double() if dn else z)
    gv = x["gcl"].double()[:, None] if gcl else torch.zeros(B, 1, dtype=F64)
    vec_ = x["vec"].double() if vec else torch.zeros(B, EW, dtype=F64)
    r = Gav + dnv + gv * (x["a"] <= x["cov"])
    E = x["E"].double()
    dot = torch.einsum("btk,bk->bt", E, vec_)
    _assert_exact(dot, torch.einsum("btk,bk->bt", E.abs(), vec_.abs()))
    _assert_exact(r + dot, r.abs() + dot.abs())
    cv = vec_ * x["cvec"].double()
    S = (a * r).sum(1, keepdim=True) + cv.sum(1, keepdim=True)
    bS = (ln + EW + 4) * U24 * ((a * r).abs().sum(1, keepdim=True) + cv.abs().sum(1, keepdim=True))
    de = a * (r + dot - S) * mask
    bde = (a * (bS + 3 * U24 * ((r + dot).abs() + S.abs())) + U24 * de.abs()) * mask
    rows = torch.arange(B)
    th = torch.tanh(_u64(x["F"], rows, x["s"], x["wc"], x["cov"]))
    sech2 = 1.0 - th * th
    del th
    v, wc = x["v"].double(), x["wc"].double()
    av, avw = v.abs(), (v * wc).abs()
    ade = de.abs()
    ds = v * torch.einsum("bt,btk->bk", de, sech2)
    ds_mag = av * torch.einsum("bt,btk->bk", ade, sech2)
    # sum_i |de_i| du_ik: the argument roundings, per feature
    du_ds = 4 * U24 * (torch.einsum("bt,btk->bk", ade, x["F"].double().abs()) / KF + x["s"].double().abs() * ade.sum(1, keepdim=True)
                       + wc.abs()[None, :] * (ade * cov.abs()).sum(1, keepdim=True))
    bds = av * (torch.einsum("bt,btk->bk", bde, sech2) + du_ds) + BOUND["ds"] * av * ade.sum(1, keepdim=True)
    hc = sech2 @ (v * wc)
    hmag = sech2 @ avw
    del sech2
    live_dcov = gv * (x["a"] > x["cov"]) + de * hc
    dcov = dnv + live_dcov * mask
    bdcov = (bde * hc.abs() + ade * ((A + 4) * U24 * hmag + _du(x["F"], rows, x["s"], x["wc"], x["cov"], avw) + BOUND["dcov"] * float(avw.sum()))
             + 3 * U24 * (dnv.abs() + gv + (de * hc).abs())) * mask
    x[key] = {"mask": mask, "de": de, "bde": bde, "ds": ds, "bds": bds, "ds_mag": ds_mag, "dcov": dcov, "bdcov": bdcov,
              "dn": dnv, "sde": a * (S.abs() + (r + dot).abs()), "sds": av * ade.sum(1, keepdim=True),
              "hc": hc, "shc": torch.full_like(hc, float(avw.sum()))}
    return x[key]


def _bwd_errors(x, got, ref=None, blocks=1, added=False):
    """Bit-exact properties of one backward result (asserted) and {quantity: (err, bound, scale)} over every
    element.  added: ds was added into the prefill ds0 by ``blocks`` workgroups per row."""
    ref = ref or _bwd_ref(x)
    mask, res = ref["mask"], {}
    assert bool((got["de"][~mask] == 0).all()), "de past the length is not zero"
    res["de"] = ((got["de"].double() - ref["de"]).abs(), ref["bde"], ref["sde"])
    pre = x["ds0"].double() if added else torch.zeros(())
    ln = x["lens"].long()[:, None]
    res["ds"] = ((got["ds"].double() - (pre + ref["ds"])).abs(), ref["bds"] + (ln + blocks + 4) * U24 * (ref["ds_mag"] + pre.abs()), ref["sds"])
    if "dcov" in got:
        assert torch.equal(_bits(got["dcov"])[~mask], _bits(ref["dn"].float())[~mask]), "dcov past the length != dcov_next"
        res["dcov"] = ((got["dcov"].double() - ref["dcov"]).abs(), ref["bdcov"], None)
    if "hc" in got:  # the emulation's h_i = sum_k v_k w_k sech^2: the table entry of dcov, no bound of its own
        res["hc"] = (((got["hc"].double() - ref["hc"]) * mask).abs(), None, ref["shc"])
    return res


def _emul_bwd(x, mut=None, de_given=None):
    """The backward step with the kernels' formulas in fp32 torch on the CPU: r-form sech^2 = 4 (r - r^2).
    de_given (the table): ds and dcov from that de instead of the emulation's own, so that their entries hold
    the sech^2 arithmetic alone."""
    B, T = x["B"], x["T"]
    mask = _mask(x["lens"], T)
    r = _rsig32(_y32(x["F"], torch.arange(B), x["s"], x["wc"], x["cov"]))
    q = r - r * r
    del r
    a, cov, g = x["a"], x["cov"], x["gcl"][:, None]
    tie = (a < cov) if mut == "tie_lt" else (a <= cov)
    rr = x["Ga"] + x["dn"] + g * tie
    dot = torch.einsum("btk,bk->bt", x["E"].float(), x["vec"])
    S = (a * rr * mask).sum(1, keepdim=True)
    if mut != "S_without_dctx_ctx":
        S = S + (x["vec"] * x["cvec"]).sum(1, keepdim=True)
    de = torch.where(mask, a * (rr + dot - S), 0.0)
    if mut == "de_1e-5":
        de = _nudge_small_de(x, de)
    if de_given is not None:
        de = de_given
    v, wc = x["v"], x["wc"]
    ds = 4.0 * v * torch.einsum("bt,btk->bk", de, q)
    hc = q @ (4.0 * v * wc)
    dcov = x["dn"] + torch.where(mask, de * hc + g * (a > cov), 0.0)
    return {"de": de, "ds": ds, "dcov": dcov, "hc": hc}


def _nudge_small_de(x, de):
    """1e-5 added to the smallest non-zero |de| of a live position in the rows of full length"""
    de = de.clone()
    b = int((x["lens"] == x["T"]).nonzero()[-1])
    mag = de[b].abs().masked_fill(de[b] == 0, INF)
    de[b, int(mag.argmin())] += 1e-5
    return de


def _bwd_args(x, vec=True, Ga=True, dn=True, gcl=True, zeros=False):
    """the optional arguments as tensors, None, or (zeros) zero tensors in place of the None ones"""
    def opt(t, on):
        return t.cuda() if on else (torch.zeros_like(t).cuda() if zeros else None)
    wc, cov = _cov_args(x, zeros)
    return wc, cov, opt(x["vec"], vec), opt(x["Ga"], Ga), opt(x["dn"], dn), opt(x["gcl"], gcl)


def _run_bwd(k, x, kind, dcov_out=True, dlen=None, step=0, **sw):
    """kind: step (adds into the ds0 prefill), row, rowp"""
    A, B, T = x["A"], x["B"], x["T"]
    W, F, s, v, a, cvec, lens = _cu(x, "E", "F", "s", "v", "a", "cvec", "lens")
    wc, cov, vec, Ga, dn, gcl = _bwd_args(x, **sw)
    o = _Outs()
    de, ds = o.new("de", (B, T)), o.new("ds", (B, A))
    dcov = o.new("dcov", (B, T)) if dcov_out else None
    if kind == "step":
        ds.copy_(x["ds0"])
        k.attn_bwd_step(W, F, s, v, wc, cov, a, vec, cvec, Ga, dn, gcl, lens, de, ds, dcov, B, T, A)
    elif kind == "row":
        k.attn_bwd_row(W, F, s, v, wc, cov, a, vec, cvec, Ga, dn, gcl, lens, de, ds, dcov, B, T, A)
    else:
        k.attn_bwd_rowp(W, F, s, v, wc, cov, a, vec, cvec, Ga, dn, gcl, lens, de, ds, dcov, B, T, A,
                        None if dlen is None else dlen.cuda(), step)
    return o.cpu()


BWD_BOUNDS = (32, 64, 128, 256)  # a wave's 32 / 64 positions, a block's 128 (A <= 512) / 256 (A = 1024)
# (A, B, T): A = 64 and 192 run attn_bwd_step<NK = 1> with lanes past A; 512 fills the 64 lanes; 1024 is NK = 2
BWD = [(64, 16, 300), (192, 16, 300), (512, 16, 300), (1024, 16, 300), (512, 8, 7), (1024, 3, 1), (64, 8, 41)]


def _step_blocks(A, T):
    return (T + 127) // 128 if A <= 512 else (T + 255) // 256


@pytest.mark.parametrize("A,B,T", BWD, ids=lambda v: str(v))
def test_attn_bwd_step_and_row(A, B, T):
    """attn_bwd_step (adds into a non-zero ds) and, at A in {512, 1024}, attn_bwd_row (stores into a NaN ds) on
    identical inputs against the one reference; then the optional arguments one by one."""
    k, x = _ops(), _bwd_case(A, B, T, A, True, BWD_BOUNDS if T == 300 else ())
    assert int(k.attn_chunks(T)) == (T + 63) // 64
    blocks = _step_blocks(A, T)
    got = _run_bwd(k, x, "step")
    _assert_bounds(f"bwd_step A={A} T={T}", _bwd_errors(x, got, blocks=blocks, added=True))
    kinds = ["step"] + (["row"] if bool(k.attn_row_ok(A, T)) else [])
    assert (len(kinds) == 2) == (A in (512, 1024))
    full = {"step": got}
    if "row" in kinds:
        full["row"] = _run_bwd(k, x, "row")
        _assert_bounds(f"bwd_row A={A} T={T}", _bwd_errors(x, full["row"]))
    for kind in kinds:
        st = kind == "step"
        det = ("de", "dcov") + (() if st and blocks > 1 else ("ds",))  # several blocks add into ds in any order
        # dcov_out = None leaves de and ds as they were
        _same_bits(full[kind], _run_bwd(k, x, kind, dcov_out=False), [n for n in det if n != "dcov"], f"{kind}: dcov_out = None")
        # Ga, dcov_next, g_cl = None: the reference without them, and the bits of zero tensors in their place
        sw = {"Ga": False, "dn": False, "gcl": False}
        none = _run_bwd(k, x, kind, **sw)
        _assert_bounds(f"bwd_{kind} A={A} T={T} Ga, dcov_next, gcl = None",
                       _bwd_errors(x, none, _bwd_ref(x, "ref_none", **sw), blocks=blocks, added=st))
        _same_bits(none, _run_bwd(k, x, kind, zeros=True, **sw), det, f"{kind}: None vs zero tensors")


@pytest.mark.parametrize("A", [512, 1024])
def test_attn_bwd_without_coverage(A):
    """The no-coverage model: w_c, cov, Ga?, dcov_next, g_cl, dcov_out all None (Ga stays: it carries the
    output-projection gradient)."""
    k, x = _ops(), _bwd_case(A, 8, 41, A, False)
    sw = {"dn": False, "gcl": False}
    ref = _bwd_ref(x, "ref_nocov", **sw)
    for kind in ("step", "row"):
        got = _run_bwd(k, x, kind, dcov_out=False, **sw)
        assert "dcov" not in got
        _assert_bounds(f"bwd_{kind} nocov A={A}", _bwd_errors(x, got, ref, added=kind == "step"))
        _same_bits(got, _run_bwd(k, x, kind, dcov_out=False, zeros=True, **sw), ("de", "ds"), f"{kind}: None vs zero tensors")


@pytest.mark.parametrize("A,T,dx,cov", [(512, 300, True, True), (512, 300, False, True), (1024, 300, True, True),
                                        (1024, 41, False, False), (512, 41, True, False), (1024, 7, True, True), (512, 1, True, True)])
def test_attn_bwd_rowp(A, T, dx, cov):
    """da_i = r_i + dx . G_i, S = sum a r + dx . gv (dx = None, the last decoder step: neither term); dead rows
    (step >= dlen) write exact zeros, live rows keep the bits of the dlen = None run."""
    k = _ops()
    assert bool(k.attn_rowp_ok(A, T, EG))
    B = 16 if T == 300 else 8
    x = _bwd_case(A, B, T, EG, cov, BWD_BOUNDS if T == 300 else ())
    sw = {"vec": dx} if cov else {"vec": dx, "dn": False, "gcl": False}
    ref = _bwd_ref(x, f"ref_rowp_{dx}", **sw)
    got = _run_bwd(k, x, "rowp", dcov_out=cov, **sw)
    _assert_bounds(f"bwd_rowp A={A} T={T} dx={dx} cov={cov}", _bwd_errors(x, got, ref))
    _same_bits(got, _run_bwd(k, x, "rowp", dcov_out=cov, zeros=True, **sw), got.keys(), "None vs zero tensors")
    step = 3
    for name, dlen in (("mixed", torch.tensor(([0, 3, 4, 100, 2, 9, 3, 4] * 2)[:B])), ("dead", torch.zeros(B)), ("live", torch.full((B,), 4))):
        dlen = dlen.int()
        run = _run_bwd(k, x, "rowp", dcov_out=cov, dlen=dlen, step=step, **sw)
        dead = step >= dlen.long()
        for n, t in run.items():
            assert bool((_bits(t[dead]) == 0).all()), (name, n, "dead row is not exact zeros")
            assert torch.equal(_bits(t[~dead]), _bits(got[n][~dead])), (name, n, "live row changed by dlen")


# ------------------------------------------------------------------ attn_bwd_feat
@functools.lru_cache(maxsize=2)
def _feat_case(D, A, B, T, cov):
    """de_all [D][B][T] is zero past the length and from step dlen[b] on (what the backward loop leaves there)"""
    g = _gen(D, A, B, T, int(cov), 3)
    x = {"D": D, "A": A, "B": B, "T": T, "cov_on": cov, "lens": _lens(g, B, T, (16, 32))}
    mask = _mask(x["lens"], T)
    x["F"] = _ri(g, -16, 16, (B, T, A), 16).bfloat16()
    x["S"] = _saturate(_ri(g, -1024, 1024, (D, B, A), 1024), A)
    x["v"] = _ri(g, -8, 8, (A,), 16)
    x["wc"] = _ri(g, -4, 4, (A,), 16) if cov else torch.zeros(A)
    x["cov"] = _ri(g, 0, 1024, (D, B, T), 1024) if cov else torch.zeros(D, B, T)
    x["dlen"] = torch.randint(0, D + 1, (B,), generator=g).int()
    x["dlen"][0], x["dlen"][B - 1] = D, 0
    if B > 2:
        x["dlen"][1], x["dlen"][2] = D, max(D - 1, 0)
    on = mask[None] & (torch.arange(D)[:, None, None] < x["dlen"].long()[None, :, None])
    x["de"] = 0.1 * torch.randn(D, B, T, generator=g) * torch.exp2(-_ri(g, 0, 12, (D, B, T), 1)) * on
    x["on"] = on
    return x


def _feat_ref(x, wgs):
    if "ref" in x:
        return x["ref"]
    D, A, B, T = x["D"], x["A"], x["B"], x["T"]
    v, wc = x["v"].double(), x["wc"].double()
    av = v.abs()
    rows = torch.arange(B)
    zBTA, zA = torch.zeros(B, T, A, dtype=F64), torch.zeros(A, dtype=F64)
    acc = {n: zBTA.clone() for n in ("dF", "dF_mag", "dF_du")}
    acc.update({n: zA.clone() for n in ("dv", "dv_mag", "dv_du", "dw", "dw_mag", "dw_du")})
    Fa = x["F"].double().abs() / KF
    for t in range(D):
        de, cov = x["de"][t].double(), x["cov"][t].double()
        ade, dc = de.abs(), de * cov
        th = torch.tanh(_u64(x["F"], rows, x["S"][t], x["wc"], x["cov"][t]))
        sech2 = 1.0 - th * th
        du = 4 * U24 * (Fa + x["S"][t].double().abs()[:, None, :] + wc.abs()[None, None, :] * cov.abs()[:, :, None])
        acc["dF"] += de[:, :, None] * sech2
        acc["dF_mag"] += ade[:, :, None] * sech2
        acc["dF_du"] += ade[:, :, None] * du
        acc["dv"] += torch.einsum("bt,btk->k", de, th)
        acc["dv_mag"] += torch.einsum("bt,btk->k", ade, 2.0 - th)
        acc["dv_du"] += torch.einsum("bt,btk->k", ade, du)
        acc["dw"] += torch.einsum("bt,btk->k", dc, sech2)
        acc["dw_mag"] += torch.einsum("bt,btk->k", dc.abs(), sech2)
        acc["dw_du"] += torch.einsum("bt,btk->k", dc.abs(), du)
    N = int(x["on"].sum())
    sde = x["de"].double().abs().sum(0)[:, :, None] * av        # [B][T][A]
    sdv = float(x["de"].double().abs().sum())
    sdw = float((x["de"].double() * x["cov"].double()).abs().sum()) * av
    dF = v * acc["dF"]
    ref = {"dF": dF, "sdF": sde, "sdv": torch.full((A,), sdv, dtype=F64), "sdwc": sdw,
           "bdF": av * ((D + 4) * U24 * acc["dF_mag"] + acc["dF_du"]) + BOUND["dF"] * sde,  # beyond 2^-8 |ref|
           "dv": acc["dv"], "bdv": (2 * N + wgs + 4) * U24 * acc["dv_mag"] + acc["dv_du"] + BOUND["dv"] * sdv,
           "dwc": v * acc["dw"], "bdwc": av * ((N + wgs + 5) * U24 * acc["dw_mag"] + acc["dw_du"]) + BOUND["dwc"] * sdw}
    x["ref"] = ref
    return ref


def _feat_errors(x, got, wgs):
    ref = _feat_ref(x, wgs)
    dead = ~_mask(x["lens"], x["T"])
    assert bool((_bits(got["dF"])[dead] == 0).all()), "dF past the length is not zero"
    res = {"dF": (_beyond_bf16(got["dF"], ref["dF"]), ref["bdF"], ref["sdF"]),
           "dv": ((got["dv"].double().sum(0) - ref["dv"]).abs(), ref["bdv"], ref["sdv"])}
    if "dwc" in got:
        res["dwc"] = ((got["dwc"].double().sum(0) - ref["dwc"]).abs(), ref["bdwc"], ref["sdwc"])
    return res


def _emul_feat(x):
    """attn_bwd_feat's r-form in fp32 torch on the CPU (dF32: dF before its bf16 rounding)"""
    D, B = x["D"], x["B"]
    v, wc, rows = x["v"], x["wc"], torch.arange(B)
    aF, aV, aW, sde = 0.0, 0.0, 0.0, 0.0
    for t in range(D):
        de, cov = x["de"][t], x["cov"][t]
        r = _rsig32(_y32(x["F"], rows, x["S"][t], wc, cov))
        q = r - r * r
        aF = aF + de[:, :, None] * q
        aV = aV + torch.einsum("bt,btk->k", de, r)
        aW = aW + torch.einsum("bt,btk->k", de * cov, q)
        sde = sde + de.sum()
    dF = torch.where(_mask(x["lens"], x["T"])[:, :, None], 4.0 * v * aF, 0.0)
    return {"dF32": dF, "dF": dF.bfloat16(), "dv": (sde - 2.0 * aV)[None, :], "dwc": (4.0 * v * aW)[None, :]}


def _run_feat(k, x, nslot, dlen=False, dwc=True, poison=False, zeros=False):
    D, A, B, T = x["D"], x["A"], x["B"], x["T"]
    F, S, v, lens = _cu(x, "F", "S", "v", "lens")
    de, cov = x["de"].clone(), x["cov"].clone()
    if poison:  # steps from dlen on are not read
        off = torch.arange(D)[:, None, None] >= x["dlen"].long()[None, :, None]
        de[off.expand_as(de)], cov[off.expand_as(cov)] = NAN, NAN
    on = x["cov_on"] or zeros
    o = _Outs()
    dF = o.new("dF", (B, T, A), BF)
    dv = o.new("dv", (nslot, A), fill=0.0)
    dw = o.new("dwc", (nslot, A), fill=0.0) if dwc and on else None
    k.attn_bwd_feat(F, S, v, x["wc"].cuda() if on else None, cov.cuda() if on else None, de.cuda(), lens, dF, dv, dw,
                    D, B, T, A, x["dlen"].cuda() if dlen else None)
    return o.cpu()


@pytest.mark.parametrize("D,A,cov", [(1, 64, True), (5, 192, True), (5, 512, True), (5, 1024, True), (1, 1024, False), (5, 64, False)])
def test_attn_bwd_feat(D, A, cov):
    """dF, dv, dwc at T = 41 (three 16-position workgroups per row, the last one partial).  One writer per slot
    (nslot >= workgroups): two runs are bit-identical, dlen changes no bit, and steps from dlen on are not
    read; nslot = 1: every workgroup adds into the one row; dwc = None leaves dF and dv alone."""
    k, B, T = _ops(), 12, 41
    x = _feat_case(D, A, B, T, cov)
    wgs = (T + 15) // 16 * B
    det = 64
    assert det >= wgs
    got = _run_feat(k, x, det)
    _assert_bounds(f"bwd_feat D={D} A={A} cov={cov} nslot={det}", _feat_errors(x, got, wgs))
    _same_bits(got, _run_feat(k, x, det), got.keys(), "one writer per slot: two runs")
    _same_bits(got, _run_feat(k, x, det, dlen=True, poison=True), got.keys(), "dlen, steps from dlen on poisoned")
    one = _run_feat(k, x, 1, dlen=True, dwc=False)
    assert "dwc" not in one
    _assert_bounds(f"bwd_feat D={D} A={A} cov={cov} nslot=1 dlen dwc=None", _feat_errors(x, one, wgs))
    _same_bits(got, one, ("dF",), "nslot = 1, dwc = None")
    if not cov:
        _same_bits(got, _run_feat(k, x, det, zeros=True), ("dF", "dv"), "None vs zero coverage tensors")


# ------------------------------------------------------------------ perturbed kernel outputs
def _a_at_len(x, a):
    """the mask mistake on the output side: a small weight at position len of every row shorter than T"""
    a = a.clone()
    rl = x["lens"].long().repeat_interleave(x["rep"])
    short = rl < x["T"]
    a[short, rl[short]] = 1e-6
    return a


def test_perturbed_kernel_outputs_are_rejected():
    """What attn_bwd_row and attn_fwd_row wrote passes; the same tensors with 1e-5 added to one small de
    element, and with a weight at position len, do not."""
    k, x = _ops(), _bwd_case(512, 16, 300, 512, True, BWD_BOUNDS)
    got = _run_bwd(k, x, "row")
    _assert_bounds("unperturbed", _bwd_errors(x, got))
    with pytest.raises(AssertionError, match="'de'"):
        _assert_bounds("de + 1e-5", _bwd_errors(x, dict(got, de=_nudge_small_de(x, got["de"]))))
    xf = _row_case(512, 8, 4, 41, False)
    gf = _run_fwd_row(k, xf)
    _assert_bounds("unperturbed", _fwd_errors(xf, gf))
    with pytest.raises(AssertionError, match="a past the length"):
        _fwd_errors(xf, dict(gf, a=_a_at_len(xf, gf["a"])))


# ------------------------------------------------------------------ script: the bound table, mutations
def _fwd_cases():
    for c in SCORE:
        yield "score " + _score_id(c), (lambda c=c: _score_case(*c)), 8
    for c in FWD_ROW:
        yield "row " + _row_id(c), (lambda c=c: _row_case(*c)), 8 if c[0] == 1024 else (12 if c[2] > 1 else 16)
    for A, T, cov in ROWP:
        yield f"rowp A={A} T={T}", (lambda A=A, T=T, cov=cov: _row_case(A, 9 if T == 300 else 8, 1, T, T == 300 and A == 512, cov=cov, EW=EG)), 8 if A == 1024 else 16


def _bwd_cases():
    for A, B, T in BWD:
        yield f"bwd A={A} T={T}", (lambda A=A, B=B, T=T: _bwd_case(A, B, T, A, True, BWD_BOUNDS if T == 300 else ()))
    for A, T in ((512, 300), (1024, 300), (1024, 7)):
        yield f"bwd rowp A={A} T={T}", (lambda A=A, T=T: _bwd_case(A, 16 if T == 300 else 8, T, EG, True, BWD_BOUNDS if T == 300 else ()))


def _feat_cases():
    for D, A in ((1, 64), (5, 192), (5, 512), (5, 1024)):
        yield f"feat D={D} A={A}", (lambda D=D, A=A: _feat_case(D, A, 12, 41, True))


def _worst(res, worst, line, verbose):
    row = {}
    for q, (err, _, scale) in res.items():
        q = {"hc": "dcov"}.get(q, q)
        if scale is None or q not in worst:
            continue
        scale = torch.as_tensor(scale, dtype=F64)
        ok = scale > 0
        err = (err - FLUSH).clamp_min(0.0)  # what fp32 flushes to zero is covered by the 2^-126 term of the bounds
        row[q] = float(torch.where(ok, err / scale.clamp_min(1e-300), torch.zeros((), dtype=F64)).max())
        worst[q] = max(worst[q], row[q])
    if verbose:
        print(line + ": " + " ".join(f"{q}={e:.3g}" for q, e in row.items()), flush=True)


def measure(fwd=None, bwd=None, feat=None, verbose=True):
    """{quantity: max |fp32 torch - float64| / scale} over the given cases (default: every case of the module)"""
    worst = {q: 0.0 for q in FP32_TORCH_ERR}
    for name, make, nw in (_fwd_cases() if fwd is None else fwd):
        x = make()
        _worst(_fwd_errors(x, _emul_fwd(x, nw=nw), teacher=True), worst, name, verbose)
        x.pop("ref", None)
    for name, make in (_bwd_cases() if bwd is None else bwd):
        x = make()
        _worst(_bwd_errors(x, _emul_bwd(x, de_given=_bwd_ref(x)["de"].float())), worst, name, verbose)
        x.pop("ref", None)
    for name, make in (_feat_cases() if feat is None else feat):
        x = make()
        got = _emul_feat(x)
        res = _feat_errors(x, got, (x["T"] + 15) // 16 * x["B"])
        res["dF"] = ((got["dF32"].double() - x["ref"]["dF"]).abs(), None, res["dF"][2])  # before the bf16 rounding
        _worst(res, worst, name, verbose)
        x.pop("ref", None)
    return worst


FWD_MUTATIONS = ("mask_le", "no_wc_cov", "F_not_scaled_back", "b_mod_rep")
BWD_MUTATIONS = ("tie_lt", "S_without_dctx_ctx", "de_1e-5")


def mutation_failures():
    """{mutation: the check that rejects it (None: passed)}, the fp32 emulation standing in for the kernel
    (CPU); the key None is the unmodified emulation."""
    caught = {}

    def judge(mut, fn):
        try:
            fn()
        except AssertionError as e:
            caught[mut] = str(e.args[0]) if e.args else "assert"
        else:
            caught[mut] = None

    xf = _row_case(512, 8, 4, 41, False)
    xb = _bwd_case(512, 8, 41, 512, True)
    for mut in (None,) + FWD_MUTATIONS:
        def fwd(mut=mut):
            got = _emul_fwd(xf, mut, nw=12)
            del got["e"]  # judged like a row kernel: end to end
            _assert_bounds(str(mut), _fwd_errors(xf, got))
        judge(("fwd", mut) if mut is None else mut, fwd)
    for mut in (None,) + BWD_MUTATIONS:
        judge(("bwd", mut) if mut is None else mut, lambda mut=mut: _assert_bounds(str(mut), _bwd_errors(xb, _emul_bwd(xb, mut))))
    xk, beam = _beam_inputs(xf)

    def keep(own_row):
        src = beam[0] + beam[1]
        got = src if own_row else src[beam[2].long()]
        assert torch.equal(_bits(got), _bits(xk["cov"])), "cov_keep != cov_src[gidx] + a_src[gidx]"
    judge(("keep", None), lambda: keep(False))
    judge("cov_keep_own_row", lambda: keep(True))
    return caught


def old_max_norm_error(x, got, ref):
    """the measure of tests/test_gpu_attention_ops.py: max |got - ref| / max |ref| over a whole tensor"""
    return float((got.double() - ref).abs().max() / ref.abs().max())


if __name__ == "__main__":  # the fp32 formulas' own rounding on the test inputs (CPU only)
    if "--mutations" in sys.argv:
        for mut, why in mutation_failures().items():
            print(f"{mut}: {'passes' if why is None else 'rejected: ' + why}")
        xb = _bwd_case(512, 8, 41, 512, True)
        print("old max-norm measure of de + 1e-5:", old_max_norm_error(xb, _emul_bwd(xb, "de_1e-5")["de"], _bwd_ref(xb)["de"]), "(< 2e-3 passes)")
    else:
        tab = measure()
        print("measured:      " + ", ".join(f'"{q}": {e:.3g}' for q, e in tab.items()))
        print("in the module: " + ", ".join(f'"{q}": {e:.3g}' for q, e in FP32_TORCH_ERR.items()))
