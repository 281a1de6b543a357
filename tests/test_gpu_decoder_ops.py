"""The decoder step kernels (csrc/kernels/decoder.hip) one by one against float64 torch:
dec_cell_fwd, dec_sproj, dec_bwd_cell, dec_bwd_dz, the reverse chain of the last two, and the
beam-decode gather variants dec_cell_fwd_beam / beam_sproj_xmerge.  No reference goes through the
engine or another kernel; bf16 operands are upcast.

    z    = XG + [ctx, h] . WcT^T ; i, j, f, o = sig(z_i), tanh(z_j), sig(z_f + 1), sig(z_o)
    c'   = f c + i j ; h' = o tanh(c')                                         (dec_cell_fwd)
    s    = [cb, hb] . WsT^T + bs                                               (dec_sproj)
    dh   = ds . Ws[H:]^T + dH_dir + dh_rec ; dc = ds . Ws[:H]^T + dC_dir + dc_carry
    dc  += dh o (1 - tanh(c')^2) ; dz = [dc j i(1-i), dc i (1-j^2), dc c f(1-f), dh tanh(c') o(1-o)]
    dc_carry <- dc f                                                           (dec_bwd_cell)
    [dx | dh_rec | dctx_prev] = dz . Wbig^T + [dX_dir | 0 | dCTX_dir_prev]     (dec_bwd_dz)

Exact linear parts.  Every bf16 operand of an MFMA sum is a dyadic rational: activations are
multiples of 1/16 in [-2, 2], weights multiples of 1/64 in [-1/8, 1/8], fp32 addends multiples of
2^-10.  Every product and partial sum is then a multiple of 2^-10; each test asserts on its float64
reference that sum_k |a_k| |w_k| + |addends| stays below 2^14 (24 significant bits), so the fp32
accumulation is exact whatever the k-slice order and every purely linear output must be
torch.equal to the reference.  The pre-activations of the cell are exact in the same way, which
leaves the activations as the only source of error in the gates.

Nonlinear outputs (gates, c, h, dz, dc_carry).  The kernel's own formulas (common.h: fsigmoid(x) =
1 / (1 + exp2(-x log2 e)), ftanh(x) = 1 - 2 / (exp2(2 clamp(x, +-15) log2 e) + 1)) evaluated in
fp32 torch on the CPU, on these very inputs, differ from the float64 reference by at most
FP32_TORCH_ERR per quantity (absolute; dc_carry relative to the reference); the kernel is allowed
8 x that (v_exp_f32, v_rcp_f32, FMA contraction: profiles/decoder_step_tests.md).  Run this file
as a script to re-measure the table; it needs no GPU.  A bf16 output with an fp32 twin written by
the same kernel (cb_out) must equal the rounded twin; one without (hb_out, dz) gets
|got - ref| <= 2^-8 |ref| + the fp32 bound (bf16 keeps 8 significant bits: round-to-nearest is
off by at most 2^-8 |ref|).

Shapes (H, A, E): (32, 32, 16): fewer than 4 k-steps at step 0, some waves get an empty slice;
(96, 160, 48): uneven slices wid * nst / 4 and gridDim.x % 8 != 0 (plain tile order);
(256, 512, 128): the shipped shape, XCD-grouped tile order; (512, 1024, 128), cell and dec_sproj
only: two load batches per wave in the cell, KB = 8 in dec_sproj; (384, 512), dec_sproj only:
K = 768, KB = 6.  B = 1, 16, 19, 33: full and partial last tiles.  Outputs are prefilled with NaN
and followed by sentinel rows up to the end of the last 16-row tile and one row more.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32, 16), (96, 160, 48), (256, 512, 128)]
CELL_SHAPES = SHAPES + [(512, 1024, 128)]
SPROJ_SHAPES = [(h, a) for h, a, _ in CELL_SHAPES] + [(384, 512)]
ROWS = [1, 16, 19, 33]
CHAIN_SHAPES = [(96, 160, 48), (256, 512, 128)]
D = 3
SENT = 12288.0  # exact in bf16
L2E = 1.4426950408889634
NAN = float("nan")
BF = torch.bfloat16
# maximum over every case below of |fp32 torch - float64| (absolute; dc_carry relative to the
# reference), measured on the CPU: see __main__
FP32_TORCH_ERR = {
    "i": 8.85e-8, "j": 1.76e-7, "f": 8.85e-8, "o": 8.85e-8, "c": 4.04e-7, "h": 2.90e-7,   # dec_cell_fwd
    "dz": 6.47e-7, "dc_carry": 1.86e-6,                                                   # dec_bwd_cell
    "chain_dz": 9.64e-7, "chain_dc_carry": 3.26e-6,                                       # reverse chain
}
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


def _acts(g, *shape):
    """bf16 activations: multiples of 1/16 in [-2, 2]"""
    return (torch.randint(-32, 33, shape, generator=g).float() / 16).bfloat16()


def _wts(g, *shape):
    """bf16 weights: multiples of 1/64 in [-1/8, 1/8]"""
    return (torch.randint(-8, 9, shape, generator=g).float() / 64).bfloat16()


def _adds(g, *shape, amp=1):
    """fp32 addends: multiples of 2^-10 in [-amp, amp]"""
    return torch.randint(-1024 * amp, 1024 * amp + 1, shape, generator=g).float() / 1024


def _assert_exact(ref, mag):
    """The exactness premise of a linear output: every term a multiple of 2^-10 (so is the sum:
    ref * 2^10 is an integer) and sum |terms| < 2^14, i.e. every partial sum has at most 24 bits."""
    assert float(mag.max()) < 2 ** 14
    assert torch.equal((ref * 1024).round(), ref * 1024)
    assert torch.equal(ref.float().double(), ref)


def _lin(a, w, add=None):
    """float64 a . w^T (+ add) and the magnitude sum |a| . |w|^T (+ |add|)"""
    a, w = a.double(), w.double()
    ref, mag = a @ w.t(), a.abs() @ w.abs().t()
    if add is not None:
        ref, mag = ref + add.double(), mag + add.double().abs()
    return ref, mag


def _out(rows, width, dtype, fill=NAN):
    """A [rows][width] device output prefilled with ``fill`` and the sentinel rows behind it (to
    the end of the last 16-row tile, plus one)."""
    alloc = (rows + 15) // 16 * 16 + 1
    full = torch.full((alloc, width), SENT, dtype=dtype, device="cuda")
    full[:rows].fill_(fill)
    return full[:rows], full[rows:]


def _untouched(*tails):
    return all(bool((t == SENT).all()) for t in tails)


def _note(tag, q, err, bound):
    print(f"[decoder-step] {tag}: {q} err={float(err):.3g} bound={bound:.3g} ratio={float(err) / bound:.3g}")


def _dlen(B, step):
    """B = 33 at ``step``: tile 0 all dead (step >= dlen), tile 1 mixed, tile 2 (row 32) live."""
    assert B == 33
    d = torch.empty(B, dtype=torch.int32)
    d[:16] = torch.arange(16, dtype=torch.int32) % (step + 1)
    d[16:32] = torch.tensor([step, step + 1] * 8, dtype=torch.int32)
    d[32] = step + 2
    return d


# ------------------------------------------------------------------ the kernel's fp32 formulas
def _fsigmoid32(x):
    return 1.0 / (1.0 + torch.exp2(-x * L2E))


def _ftanh32(x):
    return 1.0 - 2.0 / (torch.exp2(2.0 * x.clamp(-15.0, 15.0) * L2E) + 1.0)


def _cell_formulas(pre, cp, f32):
    """(i, j, f, o, c, h) from the exact pre-activations [B][4H] (forget bias included) and c_prev:
    float64 torch (the reference) or the kernel's formulas in fp32 torch."""
    H = cp.shape[1]
    if f32:
        pre, cp, sig, tanh = pre.float(), cp.float(), _fsigmoid32, _ftanh32
    else:
        pre, cp, sig, tanh = pre.double(), cp.double(), torch.sigmoid, torch.tanh
    i, j, f, o = sig(pre[:, :H]), tanh(pre[:, H:2 * H]), sig(pre[:, 2 * H:3 * H]), sig(pre[:, 3 * H:])
    c = f * cp + i * j
    return {"i": i, "j": j, "f": f, "o": o, "c": c, "h": o * tanh(c)}


def _bwd_cell_formulas(dc, dh, act, cn, cp, f32):
    """(dz [B][4H], new dc_carry) from the summed dc, dh [B][H], the gates and c_t, c_{t-1}."""
    H = cn.shape[1]
    dt = torch.float32 if f32 else torch.float64
    dc, dh, act, cn, cp = (t.to(dt) for t in (dc, dh, act, cn, cp))
    ig, jg, fg, og = act[:, :H], act[:, H:2 * H], act[:, 2 * H:3 * H], act[:, 3 * H:]
    tc = _ftanh32(cn) if f32 else torch.tanh(cn)
    dc = dc + dh * og * (1.0 - tc * tc)
    dz = torch.cat([dc * jg * ig * (1.0 - ig), dc * ig * (1.0 - jg * jg), dc * cp * fg * (1.0 - fg),
                    dh * tc * og * (1.0 - og)], 1)
    return dz, dc * fg


def _rel(x, ref):
    return float(((x.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max())


# ------------------------------------------------------------------ dec_cell_fwd
@functools.lru_cache(maxsize=None)
def _weights(H, A, E):
    g = _gen(H, A, E, 1)
    return {"WcT": _wts(g, 4 * H, A + H), "WsT": _wts(g, A, 2 * H), "Wbig": _wts(g, E + H + A, 4 * H)}


@functools.lru_cache(maxsize=None)
def _cell_case(H, A, E, B, use_ctx):
    g = _gen(H, A, B, 2)
    x = {"WcT": _weights(H, A, E)["WcT"], "XG": _adds(g, B, 4 * H),
         "ctx": _acts(g, B, A), "h": _acts(g, B, H), "c": _adds(g, B, H, amp=2)}
    a = torch.cat([x["ctx"], x["h"]], 1) if use_ctx else x["h"]
    w = x["WcT"] if use_ctx else x["WcT"][:, A:]
    pre, mag = _lin(a, w, x["XG"])
    pre[:, 2 * H:3 * H] += 1.0  # the forget bias
    _assert_exact(pre, mag + 1.0)
    x["pre"] = pre
    x["ref"] = _cell_formulas(pre, x["c"], f32=False)
    return x


def _run_cell(k, x, B, H, A, use_ctx, dlen=None, step=0):
    o = {"c": _out(B, H, torch.float32), "cb": _out(B, H, BF), "hb": _out(B, H, BF), "act": _out(B, 4 * H, torch.float32)}
    k.dec_cell_fwd(x["XG"].cuda(), x["ctx"].cuda() if use_ctx else None, x["h"].cuda(), x["c"].cuda(), x["WcT"].cuda(),
                   o["c"][0], o["cb"][0], o["hb"][0], o["act"][0], B, H, A, None if dlen is None else dlen.cuda(), step)
    torch.cuda.synchronize()
    assert _untouched(*(t for _, t in o.values())), "rows at or past B were written"
    return {n: v.cpu() for n, (v, _) in o.items()}


def _check_cell(tag, got, ref, H, rows=slice(None)):
    act = got["act"][rows].double()
    for n, q in enumerate("ijfo"):
        e = (act[:, n * H:(n + 1) * H] - ref[q][rows]).abs().max()
        _note(tag, q, e, BOUND[q])
        assert e <= BOUND[q], (q, float(e), BOUND[q])
    e = (got["c"][rows].double() - ref["c"][rows]).abs().max()
    _note(tag, "c", e, BOUND["c"])
    assert e <= BOUND["c"], ("c", float(e), BOUND["c"])
    assert torch.equal(got["cb"][rows], got["c"][rows].bfloat16()), "cb_out is not the rounded c_out"
    hr = ref["h"][rows]
    ratio = ((got["hb"][rows].double() - hr).abs() / (hr.abs() * 2.0 ** -8 + BOUND["h"])).max()
    _note(tag, "hb", ratio, 1.0)
    assert ratio <= 1.0, ("hb", float(ratio))


@pytest.mark.parametrize("use_ctx", [True, False], ids=["ctx", "step0"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H,A,E", CELL_SHAPES)
def test_dec_cell_fwd(H, A, E, B, use_ctx):
    """Gates, c and hb within the bounds, cb == bf16(c); ctxp = None is step 0 (k-range [A, A + H))."""
    x = _cell_case(H, A, E, B, use_ctx)
    got = _run_cell(_ops(), x, B, H, A, use_ctx)
    _check_cell(f"cell H={H} A={A} B={B} ctx={use_ctx}", got, x["ref"], H)


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_cell_fwd_dlen(H, A, E):
    """step >= dlen on all of tile 0: exact zeros in c, cb, hb, act; the mixed and the live tile
    equal the dlen = None run bit for bit on every row (dead rows of a live tile are computed)."""
    B, step, k = 33, 2, _ops()
    x = _cell_case(H, A, E, B, True)
    full = _run_cell(k, x, B, H, A, True)
    got = _run_cell(k, x, B, H, A, True, dlen=_dlen(B, step), step=step)
    for n in ("c", "cb", "hb", "act"):
        assert bool((got[n][:16] == 0).all()), n
        assert torch.equal(got[n][16:], full[n][16:]), n
    _check_cell(f"cell dlen H={H}", got, x["ref"], H, rows=slice(16, None))


# ------------------------------------------------------------------ dec_sproj
@functools.lru_cache(maxsize=None)
def _sproj_case(H, A, B):
    g = _gen(H, A, B, 3)
    x = {"cb": _acts(g, B, H), "hb": _acts(g, B, H), "WsT": _wts(g, A, 2 * H), "bs": _adds(g, A)}
    ref, mag = _lin(torch.cat([x["cb"], x["hb"]], 1), x["WsT"], x["bs"][None, :])
    _assert_exact(ref, mag)
    x["ref"] = ref.float()
    return x


def _run_sproj(k, x, B, H, A, dlen=None, step=0):
    s, tail = _out(B, A, torch.float32)
    k.dec_sproj(x["cb"].cuda(), x["hb"].cuda(), x["WsT"].cuda(), x["bs"].cuda(), s, B, H, A,
                None if dlen is None else dlen.cuda(), step)
    torch.cuda.synchronize()
    assert _untouched(tail)
    return s.cpu()


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H,A", SPROJ_SHAPES)
def test_dec_sproj(H, A, B):
    x = _sproj_case(H, A, B)
    assert torch.equal(_run_sproj(_ops(), x, B, H, A), x["ref"])


@pytest.mark.parametrize("H,A", SPROJ_SHAPES[:3])
def test_dec_sproj_dlen(H, A):
    """A dead tile writes nothing (the NaN prefill survives); the other rows are exact."""
    B, step = 33, 1
    x = _sproj_case(H, A, B)
    s = _run_sproj(_ops(), x, B, H, A, dlen=_dlen(B, step), step=step)
    assert bool(torch.isnan(s[:16]).all())
    assert torch.equal(s[16:], x["ref"][16:])


# ------------------------------------------------------------------ dec_bwd_cell
@functools.lru_cache(maxsize=None)
def _bwd_cell_case(H, A, B, dirs=True, general_ds=False):
    """dc_carry is chosen so that dc = ds . Ws[:H]^T + dC_dir + dc_carry has the sign of dh and
    0.25 <= |dc| <= 1.25: dc += dh o (1 - tanh(c)^2) then adds terms of one sign, and the relative
    error of the new dc_carry measures the arithmetic, not a cancellation."""
    g = _gen(H, A, B, 4)
    x = {"ds": _acts(g, B, A).float(), "Ws": _wts(g, 2 * H, A), "dC": _adds(g, B, H), "dH": _adds(g, B, H),
         "dh_rec": _adds(g, B, H), "dc_carry": _adds(g, B, H),
         "act": torch.cat([torch.sigmoid(1.5 * torch.randn(B, H, generator=g)), torch.tanh(1.5 * torch.randn(B, H, generator=g)),
                           torch.sigmoid(1.5 * torch.randn(B, H, generator=g)), torch.sigmoid(1.5 * torch.randn(B, H, generator=g))], 1),
         "cn": 1.2 * torch.randn(B, H, generator=g), "cp": 1.2 * torch.randn(B, H, generator=g)}
    if general_ds:  # any fp32: the kernel rounds it to bf16 (ld8f)
        x["ds"] = 0.7 * torch.randn(B, A, generator=g)
    dc, dh, _, _ = _bwd_cell_sums(x, dirs, H)
    want = torch.where(dh < 0, -1.0, 1.0) * (0.25 + x["dc_carry"].double().abs())
    x["dc_carry"] = (((want - (dc - x["dc_carry"].double())) * 1024).round() / 1024).float()
    return x


def _bwd_cell_sums(x, dirs, H):
    """float64 dc, dh before the cell backward, and their magnitude sums"""
    dc, mc = _lin(x["ds"], x["Ws"][:H], x["dc_carry"])
    dh, mh = _lin(x["ds"], x["Ws"][H:], x["dh_rec"])
    if dirs:
        dc, mc = dc + x["dC"].double(), mc + x["dC"].abs().double()
        dh, mh = dh + x["dH"].double(), mh + x["dH"].abs().double()
    return dc, dh, mc, mh


def _run_bwd_cell(k, x, B, H, A, dirs, dlen=None, step=0):
    dz, tail = _out(B, 4 * H, BF)
    carry, ctail = _out(B, H, torch.float32)
    carry.copy_(x["dc_carry"])
    k.dec_bwd_cell(x["ds"].cuda(), x["Ws"].cuda(), x["dC"].cuda() if dirs else None, x["dH"].cuda() if dirs else None,
                   x["dh_rec"].cuda(), carry, x["act"].cuda(), x["cn"].cuda(), x["cp"].cuda(), dz, B, H, A,
                   None if dlen is None else dlen.cuda(), step)
    torch.cuda.synchronize()
    assert _untouched(tail, ctail)
    return dz.cpu(), carry.cpu()


def _check_bwd_cell(tag, dz, carry, dz_ref, carry_ref, qz="dz", qc="dc_carry", slack_z=None, slack_c=None):
    """dz: |got - ref| <= 2^-8 |ref| + bound (+ slack (1 + 2^-8): an input perturbation of at most
    ``slack`` moves the value by that much before the bf16 rounding); dc_carry: relative bound."""
    sz = 0.0 if slack_z is None else slack_z * (1 + 2.0 ** -8)
    ratio = ((dz.double() - dz_ref).abs() / (dz_ref.abs() * 2.0 ** -8 + sz + BOUND[qz])).max()
    _note(tag, qz + "(bf16)", ratio, 1.0)
    assert ratio <= 1.0, (qz, float(ratio))
    sc = 0.0 if slack_c is None else slack_c * (1 + BOUND[qc])
    excess = ((carry.double() - carry_ref).abs() - sc) / carry_ref.abs().clamp_min(1e-30)
    _note(tag, qc, excess.max().clamp_min(0), BOUND[qc])
    assert bool((excess <= BOUND[qc]).all()), (qc, float(excess.max()), BOUND[qc])


@pytest.mark.parametrize("dirs", [True, False], ids=["dirs", "nodirs"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_bwd_cell(H, A, E, B, dirs):
    """ds bf16-representable: the two GEMM sums and the adds of the carries are exact, dz and the
    in-place dc_carry carry the activation error only."""
    x = _bwd_cell_case(H, A, B, dirs)
    dc, dh, mc, mh = _bwd_cell_sums(x, dirs, H)
    _assert_exact(dc, mc)
    _assert_exact(dh, mh)
    dz_ref, carry_ref = _bwd_cell_formulas(dc, dh, x["act"], x["cn"], x["cp"], f32=False)
    dz, carry = _run_bwd_cell(_ops(), x, B, H, A, dirs)
    _check_bwd_cell(f"bwd_cell H={H} A={A} B={B} dirs={dirs}", dz, carry, dz_ref, carry_ref)


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_bwd_cell_dlen(H, A, E):
    """Dead tile: dz exactly 0 and dc_carry untouched; the other tiles as without dlen."""
    B, step, k = 33, 1, _ops()
    x = _bwd_cell_case(H, A, B)
    dz0, carry0 = _run_bwd_cell(k, x, B, H, A, True)
    dz, carry = _run_bwd_cell(k, x, B, H, A, True, dlen=_dlen(B, step), step=step)
    assert bool((dz[:16] == 0).all())
    assert torch.equal(carry[:16], x["dc_carry"][:16])
    assert torch.equal(dz[16:], dz0[16:]) and torch.equal(carry[16:], carry0[16:])


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_bwd_cell_general_ds(H, A, E):
    """A general fp32 ds against the UNROUNDED float64 reference: the kernel rounds ds to bf16
    (round to nearest: off by at most 2^-8 |ds_k| per element), and that propagates through the
    kernel's own arithmetic as
        d(dh) = 2^-8 sum_k |ds_k| |Ws[H + u][k]|                       (the h half of the GEMM)
        d(dc) = 2^-8 sum_k |ds_k| |Ws[u][k]| + |o (1 - tanh(c)^2)| d(dh)   (dc += dh o (1 - tc^2))
        dz_i: d(dc) |j i (1 - i)|, dz_j: d(dc) |i (1 - j^2)|, dz_f: d(dc) |c_prev f (1 - f)|,
        dz_o: d(dh) |tanh(c) o (1 - o)|, dc_carry: d(dc) |f|
    on top of the bounds of the exact case (truncation instead would be off by up to 2^-7 |ds_k|)."""
    B = 33
    x = _bwd_cell_case(H, A, B, True, general_ds=True)
    dc, dh, _, _ = _bwd_cell_sums(x, True, H)
    dz_ref, carry_ref = _bwd_cell_formulas(dc, dh, x["act"], x["cn"], x["cp"], f32=False)
    ds, Ws, act = x["ds"].double().abs(), x["Ws"].double().abs(), x["act"].double()
    ig, jg, fg, og = (act[:, n * H:(n + 1) * H] for n in range(4))
    tc = torch.tanh(x["cn"].double())
    ddh = 2.0 ** -8 * ds @ Ws[H:].t()
    ddc = 2.0 ** -8 * ds @ Ws[:H].t() + (og * (1 - tc * tc)).abs() * ddh
    slack_z = torch.cat([ddc * (jg * ig * (1 - ig)).abs(), ddc * (ig * (1 - jg * jg)).abs(),
                         ddc * (x["cp"].double() * fg * (1 - fg)).abs(), ddh * (tc * og * (1 - og)).abs()], 1)
    dz, carry = _run_bwd_cell(_ops(), x, B, H, A, True)
    _check_bwd_cell(f"bwd_cell general ds H={H}", dz, carry, dz_ref, carry_ref, slack_z=slack_z, slack_c=ddc * fg.abs())


# ------------------------------------------------------------------ dec_bwd_dz
@functools.lru_cache(maxsize=None)
def _bwd_dz_case(H, A, E, B):
    g = _gen(H, A, E, B, 5)
    x = {"dz": _acts(g, B, 4 * H), "Wbig": _weights(H, A, E)["Wbig"], "dX": _adds(g, B, E), "dCTX": _adds(g, B, A)}
    ref, mag = _lin(x["dz"], x["Wbig"])
    for add, sl in ((x["dX"], slice(0, E)), (x["dCTX"], slice(E + H, None))):
        with_add = ref.clone()
        with_add[:, sl] += add.double()
        _assert_exact(with_add, mag + 1.0)
    x["ref"] = ref
    return x


def _run_bwd_dz(k, x, B, E, H, A, dirs, want_ctx=True, dlen=None, step=0, Wbig=None):
    dx, t0 = _out(B, E, torch.float32)
    dh, t1 = _out(B, H, torch.float32)
    dctx, t2 = _out(B, max(A, 1), torch.float32) if want_ctx else (None, t0)
    k.dec_bwd_dz(x["dz"].cuda(), (x["Wbig"] if Wbig is None else Wbig).cuda(), x["dX"].cuda() if dirs else None,
                 x["dCTX"].cuda() if dirs and want_ctx else None, dx, dctx, dh, B, E, H, A,
                 None if dlen is None else dlen.cuda(), step)
    torch.cuda.synchronize()
    assert _untouched(t0, t1, t2)
    return dx.cpu(), dh.cpu(), None if dctx is None else dctx.cpu()


@pytest.mark.parametrize("dirs", [True, False], ids=["dirs", "nodirs"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_bwd_dz(H, A, E, B, dirs):
    """All three column ranges exact, with and without the direct terms; dctx_prev_out = None
    (t = 0): dx and dh_rec as before and the blocks past E + H write nothing (nothing to write
    to; the sentinels behind dx and dh_rec survive); A = 0 with Wbig = W_cell alone (the call of
    the projected-context engine)."""
    k = _ops()
    x = _bwd_dz_case(H, A, E, B)
    ref = x["ref"]
    dx_ref = (ref[:, :E] + (x["dX"].double() if dirs else 0)).float()
    dh_ref = ref[:, E:E + H].float()
    dctx_ref = (ref[:, E + H:] + (x["dCTX"].double() if dirs else 0)).float()
    dx, dh, dctx = _run_bwd_dz(k, x, B, E, H, A, dirs)
    assert torch.equal(dx, dx_ref) and torch.equal(dh, dh_ref) and torch.equal(dctx, dctx_ref)
    dx, dh, dctx = _run_bwd_dz(k, x, B, E, H, A, dirs, want_ctx=False)
    assert torch.equal(dx, dx_ref) and torch.equal(dh, dh_ref)
    dx, dh, dctx = _run_bwd_dz(k, x, B, E, H, 0, dirs, want_ctx=False, Wbig=x["Wbig"][:E + H].contiguous())
    assert torch.equal(dx, dx_ref) and torch.equal(dh, dh_ref)


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_bwd_dz_dlen(H, A, E):
    """Dead tile (step >= dlen on all 16 rows): dx and dh_rec are exact zeros, and so is
    dctx_prev_out when it has no direct term; with one, dctx_prev_out is that term: it is the
    gradient of ctx_{t-1}, a row's step t - 1 may still be live (dlen == step) and dCTX_dir[t - 1]
    is all it then gets.  The other tiles are as without dlen."""
    B, step, k = 33, 2, _ops()
    x = _bwd_dz_case(H, A, E, B)
    dl = _dlen(B, step)
    for dirs in (False, True):
        dx0, dh0, dctx0 = _run_bwd_dz(k, x, B, E, H, A, dirs)
        dx, dh, dctx = _run_bwd_dz(k, x, B, E, H, A, dirs, dlen=dl, step=step)
        assert bool((dx[:16] == 0).all()) and bool((dh[:16] == 0).all())
        if dirs:
            assert torch.equal(dctx[:16], x["dCTX"][:16])
        else:
            assert bool((dctx[:16] == 0).all())
        assert torch.equal(dx[16:], dx0[16:]) and torch.equal(dh[16:], dh0[16:]) and torch.equal(dctx[16:], dctx0[16:])
    dx, dh, _ = _run_bwd_dz(k, x, B, E, H, 0, True, want_ctx=False, dlen=dl, step=step,
                            Wbig=x["Wbig"][:E + H].contiguous())
    assert bool((dx[:16] == 0).all()) and bool((dh[:16] == 0).all())
    assert torch.equal(dx[16:], dx0[16:]) and torch.equal(dh[16:], dh0[16:])


# ------------------------------------------------------------------ reverse chain
CHAIN_DLEN = [1] * 8 + [0] * 8 + [0, 1, 2, 3] * 4 + [3]  # tile 0 dead at t >= 1, tile 1 mixed, row 32 always live


@functools.lru_cache(maxsize=None)
def _chain_case(H, A, E, masked):
    B = 33
    g = _gen(H, A, E, 6)
    w = _weights(H, A, E)
    x = {"Ws": _wts(g, 2 * H, A), "Wbig": w["Wbig"], "ds": _acts(g, D, B, A).float(), "dC": _adds(g, D, B, H),
         "dH": _adds(g, D, B, H), "dX": _adds(g, D, B, E), "dCTX": _adds(g, D, B, A),
         "act": torch.cat([torch.sigmoid(1.5 * torch.randn(D, B, H, generator=g)), torch.tanh(1.5 * torch.randn(D, B, H, generator=g)),
                           torch.sigmoid(1.5 * torch.randn(D, B, H, generator=g)), torch.sigmoid(1.5 * torch.randn(D, B, H, generator=g))], 2),
         "C": 1.2 * torch.randn(D + 1, B, H, generator=g)}
    if masked:  # no upstream gradient at (t, r) with t >= dlen[r]
        dl = torch.tensor(CHAIN_DLEN)
        live = (torch.arange(D)[:, None] < dl[None, :]).float()[:, :, None]
        for n in ("ds", "dH", "dX"):
            x[n] = x[n] * live
    # dC_dir[t] as dc_carry in _bwd_cell_case: dc gets the sign of dh and 0.25 <= |dc| <= 1.25, with
    # the carries of a float64 run of the chain (the kernel's differ from them by ~1e-6)
    dh_rec, dc_carry = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    for t in reversed(range(D)):
        ds, Ws = x["ds"][t].double(), x["Ws"].double()
        gc, dh = ds @ Ws[:H].t(), dh_rec + x["dH"][t].double() + ds @ Ws[H:].t()
        want = torch.where(dh < 0, -1.0, 1.0) * (0.25 + x["dC"][t].double().abs())
        dC = ((want - gc - dc_carry) * 1024).round() / 1024
        x["dC"][t] = (dC * live[t] if masked else dC).float()
        dz, dc_carry = _bwd_cell_formulas(dc_carry + x["dC"][t].double() + gc, dh, x["act"][t], x["C"][t + 1], x["C"][t], f32=False)
        dh_rec = dz.bfloat16().double() @ x["Wbig"][E:E + H].double().t()
    return x


def _chain_gpu(k, x, H, A, E, dlen=None):
    """The reverse loop of the engine (pointer_generator._backward_mid) on shared dh_rec / dc_carry
    buffers; returns host copies of every output and of the carries before each step."""
    B = 33
    dev = {n: v.cuda() for n, v in x.items()}
    dl = None if dlen is None else torch.tensor(dlen, dtype=torch.int32, device="cuda")
    dh_rec, dc_carry = torch.zeros(B, H, device="cuda"), torch.zeros(B, H, device="cuda")
    DZ = torch.full((D, B, 4 * H), NAN, dtype=BF, device="cuda")
    DX = torch.full((D, B, E), NAN, device="cuda")
    DCTX = torch.full((D - 1, B, A), NAN, device="cuda")
    rec = {"dh_in": [None] * D, "dc_in": [None] * D, "dh_out": [None] * D, "dc_out": [None] * D}
    for t in reversed(range(D)):
        rec["dh_in"][t], rec["dc_in"][t] = dh_rec.cpu(), dc_carry.cpu()
        k.dec_bwd_cell(dev["ds"][t], dev["Ws"], dev["dC"][t], dev["dH"][t], dh_rec, dc_carry, dev["act"][t],
                       dev["C"][t + 1], dev["C"][t], DZ[t], B, H, A, dl, t)
        k.dec_bwd_dz(DZ[t], dev["Wbig"], dev["dX"][t], dev["dCTX"][t - 1] if t > 0 else None, DX[t],
                     DCTX[t - 1] if t > 0 else None, dh_rec, B, E, H, A, dl, t)
        rec["dh_out"][t], rec["dc_out"][t] = dh_rec.cpu(), dc_carry.cpu()
    torch.cuda.synchronize()
    rec.update(DZ=DZ.cpu(), DX=DX.cpu(), DCTX=DCTX.cpu())
    return rec


def _chain_fp32(x, H, A, E):
    """The same loop with the kernel's formulas in fp32 torch on the CPU (for the bound table)."""
    B = 33
    dh_rec, dc_carry = torch.zeros(B, H), torch.zeros(B, H)
    rec = {"dh_in": [None] * D, "dc_in": [None] * D, "dh_out": [None] * D, "dc_out": [None] * D,
           "DZ": torch.zeros(D, B, 4 * H, dtype=BF), "DZ32": torch.zeros(D, B, 4 * H), "DX": torch.zeros(D, B, E), "DCTX": torch.zeros(D - 1, B, A)}
    for t in reversed(range(D)):
        rec["dh_in"][t], rec["dc_in"][t] = dh_rec, dc_carry
        dc, dh = _chain_sums(x, t, dh_rec, dc_carry, H, f32=True)
        dz, dc_carry = _bwd_cell_formulas(dc, dh, x["act"][t], x["C"][t + 1], x["C"][t], f32=True)
        rec["DZ32"][t], rec["DZ"][t] = dz, dz.bfloat16()
        o = (rec["DZ"][t].double() @ x["Wbig"].double().t()).float()
        rec["DX"][t], dh_rec = o[:, :E] + x["dX"][t], o[:, E:E + H].contiguous()
        if t > 0:
            rec["DCTX"][t - 1] = o[:, E + H:] + x["dCTX"][t - 1]
        rec["dh_out"][t], rec["dc_out"][t] = dh_rec, dc_carry
    return rec


def _chain_sums(x, t, dh_rec, dc_carry, H, f32=False):
    """dc, dh of step t from the carries it received: (carry + direct term) + GEMM half, the
    kernel's order.  The carries are general fp32 values from step D - 2 on, so in fp32 the two
    adds round: that is part of what the bound covers.  The GEMM halves themselves are exact."""
    dt = torch.float32 if f32 else torch.float64
    ds, Ws = x["ds"][t].double(), x["Ws"].double()
    return ((dc_carry.to(dt) + x["dC"][t].to(dt)) + (ds @ Ws[:H].t()).to(dt),
            (dh_rec.to(dt) + x["dH"][t].to(dt)) + (ds @ Ws[H:].t()).to(dt))


def _chain_errors(x, rec, H, A, E):
    """Every step against float64 ON THE STEP'S OWN INPUTS: the carries the step received and, for
    the GEMM, the bf16 dz the step produced -- errors do not compound, the hand-off is what is
    tested.  Returns the dz error in excess of its bf16 rounding 2^-8 |ref| and the relative dc_carry
    error (maxima over the steps), and the GEMM outputs' error over their accumulation bound
        (4H + 1) 2^-23 (sum_k |dz_k| |W_k| + |addend|)
    (4H products, exact in fp32, added in any order with one rounding of at most 2^-23 relative
    per add -- twice the unit roundoff, which also covers an accumulator that truncates -- and
    the add of the direct term)."""
    ez = ec = eg = 0.0
    G = 4 * H
    for t in reversed(range(D)):
        dc, dh = _chain_sums(x, t, rec["dh_in"][t], rec["dc_in"][t], H)
        dz_ref, carry_ref = _bwd_cell_formulas(dc, dh, x["act"][t], x["C"][t + 1], x["C"][t], f32=False)
        if "DZ32" in rec:  # the fp32 evaluation on the CPU: its error before the bf16 rounding
            ez = max(ez, float((rec["DZ32"][t].double() - dz_ref).abs().max()))
        else:
            ez = max(ez, float(((rec["DZ"][t].double() - dz_ref).abs() - dz_ref.abs() * 2.0 ** -8).max()))
        ec = max(ec, _rel(rec["dc_out"][t], carry_ref))
        ref, mag = _lin(rec["DZ"][t], x["Wbig"])
        ref[:, :E] += x["dX"][t].double()
        mag[:, :E] += x["dX"][t].double().abs()
        if t > 0:
            ref[:, E + H:] += x["dCTX"][t - 1].double()
            mag[:, E + H:] += x["dCTX"][t - 1].double().abs()
        got = torch.cat([rec["DX"][t], rec["dh_out"][t]] + ([rec["DCTX"][t - 1]] if t > 0 else []), 1).double()
        n = got.shape[1]
        eg = max(eg, float(((got - ref[:, :n]).abs() / ((G + 1) * 2.0 ** -23 * mag[:, :n]).clamp_min(1e-30)).max()))
    return max(ez, 0.0), ec, eg


@pytest.mark.parametrize("H,A,E", CHAIN_SHAPES)
def test_reverse_chain(H, A, E):
    """dec_bwd_cell / dec_bwd_dz alternating for t = 2, 1, 0: dc_carry updated in place, dh_rec
    overwritten, DCTX[t - 1] seeded from dCTX_dir[t - 1]; each step against float64 on the
    kernel's own carries and bf16 dz."""
    x = _chain_case(H, A, E, False)
    rec = _chain_gpu(_ops(), x, H, A, E)
    ez, ec, eg = _chain_errors(x, rec, H, A, E)
    tag = f"chain H={H}"
    _note(tag, "chain_dz", ez, BOUND["chain_dz"])
    _note(tag, "chain_dc_carry", ec, BOUND["chain_dc_carry"])
    _note(tag, "chain_gemm", eg, 1.0)
    assert ez <= BOUND["chain_dz"] and ec <= BOUND["chain_dc_carry"] and eg <= 1.0
    assert not torch.isnan(rec["DX"]).any() and not torch.isnan(rec["DCTX"]).any()


@pytest.mark.parametrize("H,A,E", CHAIN_SHAPES)
def test_reverse_chain_skip_pad(H, A, E):
    """The skip-pad contract: with no upstream gradient (ds, dC_dir, dH_dir, dX_dir) at any (t, r)
    with t >= dlen[r], the chain run with dlen equals the chain run without it on every output
    (==, so that -0.0 counts as the zero it is)."""
    k = _ops()
    x = _chain_case(H, A, E, True)
    a, b = _chain_gpu(k, x, H, A, E), _chain_gpu(k, x, H, A, E, dlen=CHAIN_DLEN)
    for n in ("DZ", "DX", "DCTX"):
        assert bool((a[n] == b[n]).all()), n
    for t in range(D):
        assert bool((a["dh_out"][t] == b["dh_out"][t]).all()), ("dh_rec", t)
        assert bool((a["dc_out"][t] == b["dc_out"][t]).all()), ("dc_carry", t)
    # the case is not vacuous: the dead tile's rows hold zeros at the dead steps, values before
    assert bool((b["DZ"][1:, :16] == 0).all()) and bool((b["DZ"][0, :8] != 0).any())
    ez, ec, eg = _chain_errors(x, b, H, A, E)
    assert ez <= BOUND["chain_dz"] and ec <= BOUND["chain_dc_carry"] and eg <= 1.0


# ------------------------------------------------------------------ beam-decode variants
R, V, UNK = 37, 50, 1


def _beam_idx(g):
    """Parents with duplicates and in another 16-row tile than the row; tokens at or above V."""
    gidx = torch.randint(0, R, (R,), generator=g, dtype=torch.int32)
    gidx[0], gidx[1], gidx[2], gidx[20], gidx[36] = 35, 35, 17, 3, 0
    latest = torch.randint(0, V, (R,), generator=g, dtype=torch.int32)
    latest[3], latest[18], latest[36] = V, V + 7, V + 100
    return gidx, latest


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_dec_cell_fwd_beam(H, A, E):
    """The gathers inside the kernel == dec_cell_fwd on inputs gathered with torch beforehand
    (itself checked above); step[0] advances by exactly 1."""
    k = _ops()
    g = _gen(H, A, 7)
    gidx, latest = _beam_idx(g)
    tab, ctx, h, c = _adds(g, V, 4 * H), _acts(g, R, A), _acts(g, R, H), _adds(g, R, H, amp=2)
    WcT = _weights(H, A, E)["WcT"]
    tok = torch.where(latest < V, latest, torch.full_like(latest, UNK)).long()
    p = gidx.long()
    x = {"XG": tab[tok].contiguous(), "ctx": ctx[p].contiguous(), "h": h[p].contiguous(), "c": c[p].contiguous(), "WcT": WcT}
    want = _run_cell(k, x, R, H, A, True)
    o = {"c": _out(R, H, torch.float32), "cb": _out(R, H, BF), "hb": _out(R, H, BF)}
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    k.dec_cell_fwd_beam(gidx.cuda(), latest.cuda(), tab.cuda(), ctx.cuda(), h.cuda(), c.cuda(), WcT.cuda(),
                        o["c"][0], o["cb"][0], o["hb"][0], step, R, H, A, V, UNK)
    torch.cuda.synchronize()
    assert int(step.item()) == 6
    assert _untouched(*(t for _, t in o.values()))
    for n in o:
        assert torch.equal(o[n][0].cpu(), want[n]), n


@pytest.mark.parametrize("H,A,E", SHAPES)
def test_beam_sproj_xmerge(H, A, E):
    """s = [cb, hb] . WsT^T + bs and x = Xtab[tok] + ctx[gidx] . WicT^T, both exact."""
    k = _ops()
    g = _gen(H, A, E, 8)
    gidx, latest = _beam_idx(g)
    cb, hb, WsT, bs = _acts(g, R, H), _acts(g, R, H), _weights(H, A, E)["WsT"], _adds(g, A)
    ctx, WicT, Xtab = _acts(g, R, A), _wts(g, E, A), _adds(g, V, E)
    tok = torch.where(latest < V, latest, torch.full_like(latest, UNK)).long()
    s_ref, s_mag = _lin(torch.cat([cb, hb], 1), WsT, bs[None, :])
    x_ref, x_mag = _lin(ctx[gidx.long()], WicT, Xtab[tok])
    _assert_exact(s_ref, s_mag)
    _assert_exact(x_ref, x_mag)
    s, st = _out(R, A, torch.float32)
    xo, xt = _out(R, E, torch.float32)
    k.beam_sproj_xmerge(cb.cuda(), hb.cuda(), WsT.cuda(), bs.cuda(), s, ctx.cuda(), WicT.cuda(), Xtab.cuda(),
                        gidx.cuda(), latest.cuda(), xo, R, H, A, E, V, UNK)
    torch.cuda.synchronize()
    assert _untouched(st, xt)
    assert torch.equal(s.cpu(), s_ref.float()) and torch.equal(xo.cpu(), x_ref.float())


if __name__ == "__main__":  # the fp32 formulas' own rounding on the test inputs (CPU only)
    worst = {q: 0.0 for q in FP32_TORCH_ERR}
    for H, A, E in CELL_SHAPES:
        for use_ctx in (True, False):
            row = {q: 0.0 for q in "ijfoch"}
            sd = 0.0
            for B in ROWS:
                x = _cell_case(H, A, E, B, use_ctx)
                f = _cell_formulas(x["pre"], x["c"], f32=True)
                sd = max(sd, float(x["pre"].std()))
                for q in row:
                    row[q] = max(row[q], float((f[q].double() - x["ref"][q]).abs().max()))
            print(f"cell H={H:3d} A={A:4d} ctx={use_ctx!s:5} std(pre)={sd:.2f}: " + " ".join(f"{q}={e:.3g}" for q, e in row.items()))
            worst.update({q: max(worst[q], e) for q, e in row.items()})
    for H, A, E in SHAPES:
        for dirs in (True, False):
            ez = ec = 0.0
            for B in ROWS:
                x = _bwd_cell_case(H, A, B, dirs)
                dc, dh, _, _ = _bwd_cell_sums(x, dirs, H)
                dz_ref, carry_ref = _bwd_cell_formulas(dc, dh, x["act"], x["cn"], x["cp"], f32=False)
                dz, carry = _bwd_cell_formulas(dc, dh, x["act"], x["cn"], x["cp"], f32=True)
                ez, ec = max(ez, float((dz.double() - dz_ref).abs().max())), max(ec, _rel(carry, carry_ref))
            print(f"bwd_cell H={H:3d} A={A:4d} dirs={dirs!s:5}: dz={ez:.3g} dc_carry(rel)={ec:.3g}")
            worst["dz"], worst["dc_carry"] = max(worst["dz"], ez), max(worst["dc_carry"], ec)
    for H, A, E in CHAIN_SHAPES:
        for masked in (False, True):
            x = _chain_case(H, A, E, masked)
            ez, ec, eg = _chain_errors(x, _chain_fp32(x, H, A, E), H, A, E)
            print(f"chain H={H:3d} masked={masked!s:5}: dz={ez:.3g} dc_carry(rel)={ec:.3g}")
            worst["chain_dz"], worst["chain_dc_carry"] = max(worst["chain_dz"], ez), max(worst["chain_dc_carry"], ec)
    print("max:", {q: f"{e:.3g}" for q, e in worst.items()})
