"""The encoder LSTM kernels (csrc/kernels/lstm.hip, lstm_persistent.hip) one by one against float64
torch: lstm_enc_fwd_step, lstm_enc_bwd_step, lstm_fwd_persistent (4-wave, 8-wave and RT = 2
templates), lstm_fwd_persistent_fx (W_x in registers / in LDS) and lstm_bwd_persistent (16-row and
32-row BPTT, the three dout forms, with and without the gate-bias gradient).  Every kernel is called
through ops(); no reference goes through the engine or another kernel; bf16 operands are upcast.

Semantics (lstm.hip), direction d, step s, row r of length len_r, unit u:

    z    = gx[d][s][r] + bias[d] + hs[d][s][r] . Wt[d]^T            (FX: gx = xsf[d][s][r] . WxT_d^T)
    i, j, f, o = sig(z_i), tanh(z_j), sig(z_f + 1), sig(z_o) ; c' = f c + i j ; h' = o tanh(c')
    s <  len_r: hs[s+1] = bf16(h'), cs[s+1] = c', acts[s] = (i, j, f, o),
                out[r][t][d H + u] = bf16(h') at t = s (fw) or len_r - 1 - s (bw)
    s >= len_r: hs[s+1] = hs[s], cs[s+1] = cs[s] bit for bit
    dh   = dz[d][s+1][r] . Wn[d]^T + dout(d, s, r) + (s + 1 >= len_r ? dh_fin : 0)
    dc   = dc_carry + dh o (1 - tanh(c')^2)
    dz   = [dc j i (1 - i), dc i (1 - j^2), dc c f (1 - f), dh tanh(c') o (1 - o)] ; dc_carry <- dc f
    s >= len_r: dz = 0, dc_carry unchanged ; dbias += sum over rows and steps of the unrounded dz

Layouts.  Wt [2][4H][H] (row g H + u), bias [2][4H] and dz [2][T][B][4H] are gate-major; Wn [2][H][4H]
is Wt transposed per direction; gx and acts [2][T][B][H][4] are gate-interleaved; WxT_d [4H][128] has row
u 4 + g (the kernel reads ``Wx + (u * 4 + g) * 128``; pointer_generator.py packs enc0_KxiT as
K[:E].reshape(E, 4, H).permute(2, 1, 0)).  Every input here is generated gate-major ([.., 4, H]) and
permuted into the kernel's layout, every output is permuted back: a gate or layout mix-up fails.

Teacher forcing.  The kernels store every step's hs, cs, acts and dz, so each step is predicted in
float64 from the KERNEL'S OWN stored inputs of that step: hs[s], cs[s] forward, the bf16 dz[s+1]
backward (both BPTT templates feed their MFMA from the LDS copy of f2bf(dz) that is also what they
store, so the stored dz is the operand).  Nothing accumulates over the steps but dc of the persistent
BPTT, which lives in registers: the reference chains dc in float64 and its bound is chained with it.
The per-step lstm_enc_bwd_step is checked a step at a time on the dc_carry read back before it.

Inputs are dyadic: weights multiples of 1/64 in [-1/8, 1/8], xsf and hs[:, 0] multiples of 1/16 in
[-2, 2], the fp32 addends gx, bias, dh_fin, dc_carry multiples of 2^-10, dout multiples of 2^-6 in
[-1, 1] (also bf16 numbers: the three dout forms then hold the same values).  The FX input projection
and the step-0 pre-activations (forward) and the step T-1 dh (backward, no recurrent term) are exact in
fp32 in any order; the tests assert that premise on the reference (_assert_exact) and give those
steps no accumulation allowance.

Bounds (absolute).  A sum of K fp32 products plus addends, in any k-slice, partial-sum or atomic
order, is off by at most  e = (K + 4) 2^-24 (sum_k |a_k| |w_k| + |addends|)  (the 4: the adds of gx,
bias, the forget bias / of dout, dh_fin, and the peers' partials counted with the terms).  It
propagates (sigmoid is 1/4-Lipschitz, tanh 1-Lipschitz; d. is the bound of .):
    di = e_i / 4, dj = e_j, df = e_f / 4, do = e_o / 4
    dc' = |c| df + (|j| + dj) di + |i| dj                      (c is the kernel's own stored value)
    dh' = (|tanh c'| + dc') do + |o| dc'
    d(dc) = d(dc_carry) + |o (1 - tc^2)| d(dh)                  (tc = tanh(c'), from the given cs)
    d(dz) = d(dc) |j i (1 - i)|, d(dc) |i (1 - j^2)|, d(dc) |c f (1 - f)|, d(dh) |tc o (1 - o)|
    d(dc_carry) <- |f| d(dc) on a live step, unchanged on a frozen one
On top comes 8 x FP32_TORCH_ERR[T] of the quantity: the error of the kernel's own formulas (common.h
fsigmoid / ftanh) in fp32 torch on the CPU against the float64 reference, measured on these cases by
running this file as a script (no GPU needed; the recurrence is emulated in fp32 with the same teacher
forcing, see _emul_fwd / _emul_bwd; the T = 41 case has its own entries).  bf16 outputs without an fp32 twin (hs, dz) get 2^-8 |ref| more.
dbias gets the sum of its terms' bounds plus N 2^-24 sum |dz| for the N = T B + 1 fp32 / atomic adds.
"""
import functools
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
SENT = 12288.0    # trailing sentinel blocks (exact in bf16)
OUT_PRE = -24576.0  # prefill of the per-step kernel's out (it leaves positions past the length alone)
PAD = 4096
L2E = 1.4426950408889634
E_IN = 128
U24 = 2.0 ** -24

STEP_SHAPES = [(32, 1), (96, 19), (256, 33)]
# (H, B, T, forward template, BPTT rows, more than one launch)
PERSISTENT = [(64, 1, 5, "4w", 16, False), (64, 19, 5, "4w", 16, False), (128, 33, 5, "4w", 16, False),
              (256, 16, 5, "4w", 16, False), (256, 40, 5, "4w", 16, False), (256, 40, 41, "4w", 16, False),
              (512, 40, 5, "8w", 16, False), (512, 256, 5, "8w", 16, False), (512, 264, 5, "rt2", 32, False),
              (256, 520, 5, "4w", 16, True), (512, 520, 5, "rt2", 32, True)]
FX_SHAPES = [(64, 19, 5, "4w", 16, False), (256, 40, 5, "4w", 16, False), (512, 264, 5, "rt2", 32, False),
             (256, 520, 5, "4w", 16, True)]
ALL_DOUT_FORMS = [(256, 40, 5), (512, 264, 5)]
# per T, the max over the cases of that T of |fp32 torch - float64| (absolute), measured on the CPU: see
# __main__.  The one T = 41 case has entries of its own, so the T = 5 cases are held to their own errors.
FP32_TORCH_ERR = {
    5: {"i": 9.78e-8, "j": 2.04e-7, "f": 1.08e-7, "o": 9.75e-8, "c": 4.52e-7, "h": 2.87e-7,   # forward, every kernel
        "dz": 4.81e-7, "dc_carry": 6.25e-7,                                                   # persistent BPTT (dc chained)
        "step_dz": 2.47e-7, "step_dc_carry": 3.11e-7},                                        # lstm_enc_bwd_step (one step)
    41: {"i": 9.06e-8, "j": 1.89e-7, "f": 9.83e-8, "o": 9.48e-8, "c": 7.61e-7, "h": 2.32e-7, "dz": 3.59e-7, "dc_carry": 3.55e-7},
}
BOUND = {T: {q: 8.0 * e for q, e in tab.items()} for T, tab in FP32_TORCH_ERR.items()}


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


# ------------------------------------------------------------------ dyadic inputs
def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _acts16(g, *shape):
    """bf16 activations: multiples of 1/16 in [-2, 2]"""
    return (torch.randint(-32, 33, shape, generator=g).float() / 16).bfloat16()


def _wts(g, *shape):
    """bf16 weights: multiples of 1/64 in [-1/8, 1/8]"""
    return (torch.randint(-8, 9, shape, generator=g).float() / 64).bfloat16()


def _adds(g, *shape, amp=1):
    """fp32 addends: multiples of 2^-10 in [-amp, amp]"""
    return torch.randint(-1024 * amp, 1024 * amp + 1, shape, generator=g).float() / 1024


def _assert_exact(ref, mag):
    """The exactness premise of a linear output: every term a multiple of 2^-10 (so is the sum) and
    sum |terms| < 2^14, i.e. every partial sum has at most 24 bits: exact in fp32 in any order."""
    assert float(mag.max()) < 2 ** 14
    assert torch.equal((ref * 1024).round(), ref * 1024)
    assert torch.equal(ref.float().double(), ref)


def _lens(g, B, T):
    """Lengths in [1, T]: row 0 is T; 1, 2, T - 1, T present; the last two rows (inside the partial
    last tile where there is one) are T and 1.  B = 1 has the one row of length T."""
    lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    if B >= 7:
        lens[1], lens[2], lens[3], lens[4] = 1, 2, T - 1, T
        lens[B - 2], lens[B - 1] = T, 1
    lens[0] = T
    return lens


def _live(lens, T):
    """[T][B]: s < len_r"""
    return torch.arange(T)[:, None] < lens.long()[None, :]


def _tpos(lens, T):
    """[2][T][B]: the position of (direction, step, row) in the batch frame: s (fw), len_r - 1 - s (bw);
    frozen steps sit at s in both directions"""
    s = torch.arange(T)[:, None].expand(T, lens.numel())
    ln = lens.long()[None, :]
    return torch.stack([s, torch.where(s < ln, ln - 1 - s, s)])


def _to_kernel(x):
    """gate-major [..., 4, H] -> the kernels' gate-interleaved [..., H, 4]"""
    return x.transpose(-1, -2).contiguous()


def _from_kernel(x):
    """[..., H, 4] -> gate-major [..., 4, H]"""
    return x.transpose(-1, -2)


def _matmul(a, w):
    """float64 a[d] . w[d]^T and |a[d]| . |w[d]|^T for a [2][..][K], w [2][N][K]"""
    a2, w2 = a.double().reshape(2, -1, a.shape[-1]), w.double().transpose(1, 2)
    shape = a.shape[:-1] + (w.shape[1],)
    return torch.bmm(a2, w2).view(shape), torch.bmm(a2.abs(), w2.abs()).view(shape)


# ------------------------------------------------------------------ the kernel's fp32 formulas
def _fsigmoid32(x):
    return 1.0 / (1.0 + torch.exp2(-x * L2E))


def _ftanh32(x):
    return 1.0 - 2.0 / (torch.exp2(2.0 * x.clamp(-15.0, 15.0) * L2E) + 1.0)


def _cell(z, c, f32):
    """(i, j, f, o, c', h') from the pre-activations z [..., 4, H] (forget bias not yet added) and c:
    float64 torch (the reference) or the kernel's formulas in fp32 torch"""
    if f32:
        z, c, sig, tanh = z.float(), c.float(), _fsigmoid32, _ftanh32
    else:
        z, c, sig, tanh = z.double(), c.double(), torch.sigmoid, torch.tanh
    i, j, f, o = sig(z[..., 0, :]), tanh(z[..., 1, :]), sig(z[..., 2, :] + 1.0), sig(z[..., 3, :])
    cn = f * c + i * j
    return {"i": i, "j": j, "f": f, "o": o, "c": cn, "h": o * tanh(cn)}


def _cell_bwd(dc_in, dh, act, cn, cp, f32):
    """(dz [..., 4, H], dc f) from the carried dc, dh, the gates act [..., 4, H] and c', c"""
    dt = torch.float32 if f32 else torch.float64
    dc_in, dh, act, cn, cp = (t.to(dt) for t in (dc_in, dh, act, cn, cp))
    ig, jg, fg, og = (act[..., n, :] for n in range(4))
    tc = _ftanh32(cn) if f32 else torch.tanh(cn)
    dc = dc_in + dh * og * (1.0 - tc * tc)
    dz = torch.stack([dc * jg * ig * (1.0 - ig), dc * ig * (1.0 - jg * jg), dc * cp * fg * (1.0 - fg),
                      dh * tc * og * (1.0 - og)], -2)
    return dz, dc * fg


# ------------------------------------------------------------------ forward: cases, reference, checks
@functools.lru_cache(maxsize=4)
def _fwd_case(H, B, T, fx):
    g = _gen(H, B, T, int(fx), 1)
    x = {"H": H, "B": B, "T": T, "fx": fx, "lens": _lens(g, B, T), "Wt": _wts(g, 2, 4 * H, H),
         "bias": _adds(g, 2, 4, H), "hs0": _acts16(g, 2, B, H), "cs0": _adds(g, 2, B, H, amp=2)}
    if fx:
        x["xsf"] = _acts16(g, 2, T, B, E_IN)
        x["Wx"] = _wts(g, 2, 4, H, E_IN)                                       # gate-major
        x["WxT"] = x["Wx"].transpose(1, 2).reshape(2, 4 * H, E_IN).contiguous()  # row u * 4 + g
        zx, mx = _matmul(x["xsf"], x["Wx"].reshape(2, 4 * H, E_IN))
        _assert_exact(zx, mx)                                                  # the input projection is exact
        zx, mx = zx.view(2, T, B, 4, H), mx.view(2, T, B, 4, H)
    else:
        gxm = _adds(g, 2, T, B, 4, H)                                          # gate-major
        x["gx"] = _to_kernel(gxm)
        zx, mx = gxm.double(), gxm.double().abs()
    b = x["bias"].double()[:, None, None]
    x["zx"], x["mx"] = zx + b, mx + b.abs()
    x["mx"][..., 2, :] += 1.0                                                  # the forget bias
    return x


def _fwd_reference(x, hs, cs):
    """Every step from the stored hs[s], cs[s]: float64 gates, c', h' [2][T][B][H] and their
    accumulation bounds (module docstring); step 0 is asserted exact and gets none."""
    H, B, T = x["H"], x["B"], x["T"]
    rec, mag = _matmul(hs[:, :T], x["Wt"])
    z, mag = x["zx"] + rec.view(2, T, B, 4, H), x["mx"] + mag.view(2, T, B, 4, H)
    z0 = z[:, 0].clone()
    z0[..., 2, :] += 1.0
    _assert_exact(z0, mag[:, 0])
    K = H + (E_IN if x["fx"] else 0)
    e = (K + 4) * U24 * mag
    e[:, 0] = 0.0
    c = cs[:, :T].double()
    ref = _cell(z, c, f32=False)
    di, dj, df, do = e[..., 0, :] / 4, e[..., 1, :], e[..., 2, :] / 4, e[..., 3, :] / 4
    dc = c.abs() * df + (ref["j"].abs() + dj) * di + ref["i"].abs() * dj
    dh = (torch.tanh(ref["c"]).abs() + dc) * do + ref["o"].abs() * dc
    return ref, {"i": di, "j": dj, "f": df, "o": do, "c": dc, "h": dh}


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _fwd_errors(x, got):
    """Bit-exact properties of one forward run (asserted) and {quantity: (err, lin)} over the live
    (step, row) pairs: the error against float64 (for hs beyond its bf16 rounding 2^-8 |ref|) and the
    propagated accumulation bound."""
    H, B, T, lens = x["H"], x["B"], x["T"], x["lens"]
    hs, cs, acts, out = got["hs"], got["cs"], _from_kernel(got["acts"]), got["out"]
    live = _live(lens, T)
    m = live[None, :, :, None].expand(2, T, B, H)
    assert torch.equal(hs[:, 0], x["hs0"]) and torch.equal(cs[:, 0], x["cs0"]), "the initial state was written"
    assert torch.equal(_bits(hs[:, 1:])[~m], _bits(hs[:, :-1])[~m]), "frozen rows: hs[s+1] != hs[s]"
    assert torch.equal(_bits(cs[:, 1:])[~m], _bits(cs[:, :-1])[~m]), "frozen rows: cs[s+1] != cs[s]"
    # out at the mapped position is the stored hs[s+1]: pins the bw reversal per length
    o = out.view(B, T, 2, H)
    og = o[torch.arange(B)[None, None, :], _tpos(lens, T), torch.arange(2)[:, None, None]]  # [2][T][B][H]
    assert torch.equal(_bits(og)[m], _bits(hs[:, 1:])[m]), "out != hs[s+1] at t = s (fw) / len - 1 - s (bw)"
    past = (torch.arange(T)[None, :] >= lens.long()[:, None])[:, :, None].expand(B, T, 2 * H)
    if got["past_len"] == "zero":
        assert bool((out[past] == 0).all()), "out past the length is not zero"
    else:
        assert bool((out[past] == OUT_PRE).all()), "out past the length was written"
    ref, lin = _fwd_reference(x, hs, cs)
    res = {}
    for n, q in enumerate("ijfo"):
        res[q] = ((acts[..., n, :].double() - ref[q]).abs()[m], lin[q][m])
    res["c"] = ((cs[:, 1:].double() - ref["c"]).abs()[m], lin["c"][m])
    if "h32" in got:  # the fp32 emulation: h before its bf16 rounding
        eh = (got["h32"].double() - ref["h"]).abs()
    else:
        eh = (hs[:, 1:].double() - ref["h"]).abs() - 2.0 ** -8 * ref["h"].abs()
    res["h"] = (eh[m], lin["h"][m])
    return res


def _note(tag, q, ratio):
    print(f"[lstm-ops] {tag}: {q} err/bound={float(ratio):.3g}")


def _assert_bounds(tag, x, res, keys=None):
    for q, (err, lin) in res.items():
        b = BOUND[x["T"]][(keys or {}).get(q, q)]
        assert b > 0
        ratio = (err / (lin + b)).max() if err.numel() else torch.zeros(())
        _note(tag, q, ratio)
        assert float(ratio) <= 1.0, (tag, q, float(ratio))


def _emul_fwd(x, mut=None):
    """The forward recurrence with the kernel's formulas in fp32 torch on the CPU (the bound table,
    and the stand-in kernel of the mutation checks): z is the float64 sum rounded to fp32."""
    H, B, T, lens = x["H"], x["B"], x["T"], x["lens"]
    hs, cs = torch.zeros(2, T + 1, B, H, dtype=BF), torch.zeros(2, T + 1, B, H)
    hs[:, 0], cs[:, 0] = x["hs0"], x["cs0"]
    acts, out, h32 = torch.full((2, T, B, H, 4), NAN), torch.zeros(B, T, 2 * H, dtype=BF), torch.zeros(2, T, B, H)
    live, tpos = _live(lens, T), _tpos(lens, T)
    rows = torch.arange(B)
    for s in range(T):
        z = x["zx"][:, s] + _matmul(hs[:, s], x["Wt"])[0].view(2, B, 4, H)
        if mut == "no_forget_bias":
            z[..., 2, :] -= 1.0
        f = _cell(z.float(), cs[:, s], f32=True)
        a = live[s][None, :, None]
        h16, h32[:, s] = f["h"].bfloat16(), f["h"]
        hs[:, s + 1], cs[:, s + 1] = torch.where(a, h16, hs[:, s]), torch.where(a, f["c"], cs[:, s])
        g4 = torch.stack([f["i"], f["j"], f["f"], f["o"]], -1)
        if mut == "gate_swap":
            g4 = g4[..., [0, 2, 1, 3]]
        acts[:, s] = torch.where(a[..., None], g4, acts[:, s])
        for d in range(2):
            t = torch.full((B,), s) if mut == "bw_at_s" else tpos[d, s]
            r = rows[live[s]]
            out[r, t[live[s]], d * H:(d + 1) * H] = h16[d][live[s]]
    if mut == "cs_1e-4":
        cs[1, 2, 0, H // 2] += 1e-4
    return {"hs": hs, "cs": cs, "acts": acts, "out": out, "past_len": "zero", "h32": h32}


def _dev_buf(shape, dtype, fill):
    """A device tensor prefilled with ``fill`` and the sentinel block allocated behind it"""
    n = 1
    for v in shape:
        n *= v
    full = torch.full((n + PAD,), SENT, dtype=dtype, device="cuda")
    full[:n].fill_(fill)
    return full[:n].view(shape), full[n:]


def _untouched(*tails):
    return all(bool((t == SENT).all()) for t in tails)


def _xbuf(k, H, B, bwd):
    return torch.zeros(int(k.lstm_persistent_xbuf(H, B, bwd)), device="cuda", dtype=torch.long)


def _run_fwd(k, x, mode):
    """mode: step (T launches of lstm_enc_fwd_step), persistent, fx"""
    H, B, T = x["H"], x["B"], x["T"]
    hs, t0 = _dev_buf((2, T + 1, B, H), BF, NAN)
    cs, t1 = _dev_buf((2, T + 1, B, H), torch.float32, NAN)
    acts, t2 = _dev_buf((2, T, B, H, 4), torch.float32, NAN)
    out, t3 = _dev_buf((B, T, 2 * H), BF, OUT_PRE if mode == "step" else NAN)
    hs[:, 0], cs[:, 0] = x["hs0"].cuda(), x["cs0"].cuda()
    lens, bias, Wt = x["lens"].cuda(), x["bias"].reshape(2, 4 * H).cuda(), x["Wt"].cuda()
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    if mode == "step":
        gx = x["gx"].cuda()
        for s in range(T):
            k.lstm_enc_fwd_step(gx, bias, Wt, hs, cs, acts, out, lens, s, T, B, H)
    elif mode == "persistent":
        k.lstm_fwd_persistent(x["gx"].cuda(), bias, Wt, hs, cs, acts, out, lens, _xbuf(k, H, B, False), err, T, B, H)
    else:
        k.lstm_fwd_persistent_fx(x["xsf"].cuda(), x["WxT"][0].cuda(), x["WxT"][1].cuda(), bias, Wt, hs, cs, acts, out,
                                 lens, _xbuf(k, H, B, False), err, T, B, H)
    torch.cuda.synchronize()
    assert int(err.item()) == 0, "a hand-off timed out"
    assert _untouched(t0, t1, t2, t3), "a sentinel block behind an output was written"
    return {"hs": hs.cpu(), "cs": cs.cpu(), "acts": acts.cpu(), "out": out.cpu(),
            "past_len": "kept" if mode == "step" else "zero"}


def _assert_variant(k, H, B, fwd, rows_bwd, multi):
    """The case selects the templates it names, from what the library itself reports: the row tile
    of each direction shows in the hand-off buffer size, the 8-wave forward in fx_ok == False."""
    assert int(k.lstm_persistent_grid(H, B)) > 0
    NC = H // 64
    rows_f = 32 if fwd == "rt2" else 16
    assert int(k.lstm_persistent_xbuf(H, B, False)) == 2 * ((B + rows_f - 1) // rows_f) * 2 * rows_f * (H // 2)
    assert int(k.lstm_persistent_xbuf(H, B, True)) == 2 * ((B + rows_bwd - 1) // rows_bwd) * 2 * NC * NC * rows_bwd * 64
    assert bool(k.lstm_persistent_fx_ok(H, B, E_IN)) == (fwd != "8w")
    launches = int(k.lstm_persistent_launches(H, B))
    if multi and launches == 1:
        pytest.skip(f"this device holds all {int(k.lstm_persistent_grid(H, B))} workgroups of H={H}, B={B} at once "
                    f"(capacity {int(k.lstm_persistent_capacity(H))}): one launch, not several")
    assert (launches > 1) == multi, launches


@pytest.mark.parametrize("H,B", STEP_SHAPES)
def test_lstm_enc_fwd_step(H, B):
    """T launches; out past the length keeps its prefill.  (32, 1): nst = 1, three waves get an empty
    k-slice; (96, 19): uneven slices, partial tile; (256, 33): three row tiles."""
    x = _fwd_case(H, B, 5, False)
    _assert_bounds(f"fwd_step H={H} B={B}", x, _fwd_errors(x, _run_fwd(_ops(), x, "step")))


@pytest.mark.parametrize("H,B,T,fwd,rows_bwd,multi", PERSISTENT)
def test_lstm_fwd_persistent(H, B, T, fwd, rows_bwd, multi):
    k = _ops()
    _assert_variant(k, H, B, fwd, rows_bwd, multi)
    x = _fwd_case(H, B, T, False)
    _assert_bounds(f"fwd_persistent[{fwd}] H={H} B={B} T={T}", x, _fwd_errors(x, _run_fwd(k, x, "persistent")))


@pytest.mark.parametrize("H,B,T,fwd,rows_bwd,multi", FX_SHAPES)
def test_lstm_fwd_persistent_fx(H, B, T, fwd, rows_bwd, multi):
    """The input projection inside the recurrence: W_x in registers (RT = 1) / in LDS (RT = 2)."""
    k = _ops()
    _assert_variant(k, H, B, fwd, rows_bwd, multi)
    x = _fwd_case(H, B, T, True)
    _assert_bounds(f"fwd_fx[{fwd}] H={H} B={B} T={T}", x, _fwd_errors(x, _run_fwd(k, x, "fx")))


def test_fx_is_not_offered_on_the_8_wave_forward():
    assert not bool(_ops().lstm_persistent_fx_ok(512, 40, E_IN))


# ------------------------------------------------------------------ backward: cases, reference, checks
@functools.lru_cache(maxsize=4)
def _bwd_case(H, B, T):
    g = _gen(H, B, T, 2)

    def sg():
        return torch.sigmoid(1.5 * torch.randn(2, T, B, H, generator=g))

    def th():
        return torch.tanh(1.5 * torch.randn(2, T, B, H, generator=g))

    lens = _lens(g, B, T)
    x = {"H": H, "B": B, "T": T, "lens": lens, "Wt": _wts(g, 2, 4 * H, H),
         "act": torch.stack([sg(), th(), sg(), sg()], 3),                      # [2][T][B][4][H] gate-major
         "cs": 1.2 * torch.randn(2, T + 1, B, H, generator=g),
         "dE": torch.randint(-64, 65, (B, T, 2 * H), generator=g).float() / 64,  # batch frame, bf16 numbers
         "dh_fin": _adds(g, 2, B, H), "dc0": _adds(g, 2, B, H), "db0": _adds(g, 2, 4 * H)}
    x["Wn"] = x["Wt"].transpose(1, 2).contiguous()                             # as the engine passes it
    x["acts"] = _to_kernel(x["act"])
    assert torch.equal(x["dE"].bfloat16().float(), x["dE"])
    # dout(d, s, r): the batch-frame tensor read at t = s (fw) / len_r - 1 - s (bw), frozen steps at s
    x["dho"] = x["dE"].view(B, T, 2, H)[torch.arange(B)[None, None, :], _tpos(lens, T), torch.arange(2)[:, None, None]]
    return x


def _dout_form(x, form):
    """0: step frame fp32 [2][T][B][H]; 1: batch frame fp32 [B][T][2H]; 2: batch frame bf16"""
    return (x["dho"].contiguous(), x["dE"], x["dE"].bfloat16())[form]


def _bwd_errors(x, got):
    """Bit-exact properties of one backward run (asserted) and {quantity: (err, lin)}.  got: dz
    [2][T][B][4H] bf16 (or fp32 from the emulation), dc [2][B][H] after the last step, optionally
    dbias, and for the per-step kernel the carries read back before / after every launch."""
    H, B, T, lens = x["H"], x["B"], x["T"], x["lens"]
    live = _live(lens, T)
    m4 = live[None, :, :, None, None].expand(2, T, B, 4, H)
    dz = got["dz"].view(2, T, B, 4, H)
    assert bool((dz[~m4] == 0).all()), "dz of an inactive (row, step) is not zero"
    dzq = got.get("dz_operand", got["dz"])                                   # what the next step multiplies
    rec, mag = torch.zeros(2, T, B, H, dtype=torch.float64), torch.zeros(2, T, B, H, dtype=torch.float64)
    if T > 1:
        rec[:, :T - 1], mag[:, :T - 1] = _matmul(dzq[:, 1:], x["Wn"])
    fin = (torch.arange(T)[:, None] + 1 >= lens.long()[None, :])[None, :, :, None]
    dhf = x["dh_fin"].double()[:, None]
    dh = rec + x["dho"].double() + fin * dhf
    mag = mag + x["dho"].double().abs() + fin * dhf.abs()
    _assert_exact(dh[:, T - 1], mag[:, T - 1])
    edh = (4 * H + 4) * U24 * mag
    edh[:, T - 1] = 0.0
    act, cs = x["act"].double(), x["cs"].double()
    ig, jg, fg, og = (act[..., n, :] for n in range(4))
    tc = torch.tanh(cs[:, 1:])
    gdc = (og * (1 - tc * tc)).abs()
    fac = torch.stack([jg * ig * (1 - ig), ig * (1 - jg * jg), cs[:, :T] * fg * (1 - fg), tc * og * (1 - og)], 3).abs()
    dz_ref, edz = torch.zeros(2, T, B, 4, H, dtype=torch.float64), torch.zeros(2, T, B, 4, H, dtype=torch.float64)
    dc, edc = x["dc0"].double(), torch.zeros(2, B, H, dtype=torch.float64)
    step = "carry_in" in got
    ec, lc, mc = [], [], []
    for s in reversed(range(T)):
        a = live[s][None, :, None]
        if step:  # the per-step kernel: from the carry it was handed
            dc, edc = got["carry_in"][s].double(), torch.zeros_like(edc)
            assert torch.equal(_bits(got["carry_out"][s])[~a.expand(2, B, H)], _bits(got["carry_in"][s])[~a.expand(2, B, H)]), \
                "dc_carry changed on an inactive step"
        z, new = _cell_bwd(dc, dh[:, s], act[:, s], cs[:, s + 1], cs[:, s], f32=False)
        e_dc = edc + gdc[:, s] * edh[:, s]
        dz_ref[:, s] = z * a[:, :, None]
        edz[:, s, :, :3] = e_dc[:, :, None] * fac[:, s, :, :3]
        edz[:, s, :, 3] = edh[:, s] * fac[:, s, :, 3]
        dc, edc = torch.where(a, new, dc), torch.where(a, e_dc * fg[:, s].abs(), edc)
        if step:
            ec.append((got["carry_out"][s].double() - dc).abs()), lc.append(edc), mc.append(a.expand(2, B, H))
    if not step:
        ec, lc, mc = [(got["dc"].double() - dc).abs()], [edc], [torch.ones(2, B, H, dtype=torch.bool)]
    ez = (dz.double() - dz_ref).abs() - (got["dz_bf16"] * 2.0 ** -8) * dz_ref.abs()
    ec, lc, mc = torch.stack(ec), torch.stack(lc), torch.stack(mc)
    res = {"dz": (ez[m4], edz[m4]), "dc_carry": (ec[mc], lc[mc])}
    if got.get("dbias") is not None:
        # unrounded dz summed over rows and steps onto the initial contents, gate-major [2][4H]
        ref = x["db0"].double() + dz_ref.sum((1, 2)).view(2, 4 * H)
        n = T * B + 1
        term = ((edz + BOUND[T]["dz"]) * m4).sum((1, 2)).view(2, 4 * H)
        summ = n * U24 * (dz_ref.abs().sum((1, 2)).view(2, 4 * H) + x["db0"].double().abs())
        res["dbias"] = ((got["dbias"].double() - ref).abs(), term + summ)
    return res


def _assert_bwd_bounds(tag, x, res, step=False):
    keys = {"dz": "step_dz", "dc_carry": "step_dc_carry"} if step else {}
    db = res.pop("dbias", None)
    _assert_bounds(tag, x, res, keys)
    if db is not None:  # its bound carries the 8 x table term of every summand already
        ratio = (db[0] / db[1]).max()
        _note(tag, "dbias", ratio)
        assert float(ratio) <= 1.0, (tag, "dbias", float(ratio))


def _emul_bwd(x, step, mut=None):
    """The BPTT with the kernel's formulas in fp32 torch on the CPU: dh is the float64 sum over the
    emulation's own bf16 dz rounded to fp32, dc is chained in fp32; step = True also records the
    carries before and after every step, as the per-step test reads them back."""
    H, B, T, lens = x["H"], x["B"], x["T"], x["lens"]
    live = _live(lens, T)
    dz32, dz16 = torch.zeros(2, T, B, 4, H), torch.zeros(2, T, B, 4 * H, dtype=BF)
    dc = x["dc0"].clone()
    cin, cout = [None] * T, [None] * T
    for s in reversed(range(T)):
        a = live[s][None, :, None]
        rec = _matmul(dz16[:, s + 1], x["Wn"])[0] if s + 1 < T else 0.0
        last = (s >= lens.long()) if mut == "dh_fin_late" else (s + 1 >= lens.long())
        dh = (rec + x["dho"][:, s].double() + last[None, :, None] * x["dh_fin"].double()).float()
        cin[s] = dc
        z, new = _cell_bwd(dc, dh, x["act"][:, s], x["cs"][:, s + 1], x["cs"][:, s], f32=True)
        dz32[:, s] = z * a[:, :, None]
        dz16[:, s] = dz32[:, s].reshape(2, B, 4 * H).bfloat16()
        dc = torch.where(a, new, dc)
        cout[s] = dc
    got = {"dz": dz32.view(2, T, B, 4 * H), "dz_operand": dz16, "dc": dc, "dz_bf16": 0.0,
           "dbias": (x["db0"].double() + dz32.double().sum((1, 2)).view(2, 4 * H)).float()}
    if step:
        got.update(carry_in=cin, carry_out=cout)
    return got


def _run_bwd_persistent(k, x, form, with_dbias):
    H, B, T = x["H"], x["B"], x["T"]
    dz, t0 = _dev_buf((2, T, B, 4 * H), BF, NAN)
    dc, t1 = _dev_buf((2, B, H), torch.float32, NAN)
    db, t2 = _dev_buf((2, 4 * H), torch.float32, NAN)
    dc.copy_(x["dc0"])
    db.copy_(x["db0"])
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    k.lstm_bwd_persistent(dz, x["Wn"].cuda(), _dout_form(x, form).cuda(), x["dh_fin"].cuda(), dc, x["acts"].cuda(),
                          x["cs"].cuda(), x["lens"].cuda(), _xbuf(k, H, B, True), err, db if with_dbias else None,
                          T, B, H, form > 0)
    torch.cuda.synchronize()
    assert int(err.item()) == 0, "a hand-off timed out"
    assert _untouched(t0, t1, t2), "a sentinel block behind an output was written"
    if not with_dbias:
        assert torch.equal(db.cpu(), x["db0"]), "dbias = None wrote the gate-bias gradient"
    return {"dz": dz.cpu(), "dc": dc.cpu(), "dbias": db.cpu() if with_dbias else None, "dz_bf16": 1.0}


@pytest.mark.parametrize("H,B", STEP_SHAPES)
def test_lstm_enc_bwd_step(H, B):
    """s = T - 1 ... 0, dc_carry read back before and after every launch; step-frame dout."""
    k, T = _ops(), 5
    x = _bwd_case(H, B, T)
    dz, t0 = _dev_buf((2, T, B, 4 * H), BF, NAN)
    dc, t1 = _dev_buf((2, B, H), torch.float32, NAN)
    dc.copy_(x["dc0"])
    dev = [x[n].cuda() for n in ("Wn", "dh_fin", "acts", "cs", "lens")]
    dout = _dout_form(x, 0).cuda()
    cin, cout = [None] * T, [None] * T
    for s in reversed(range(T)):
        cin[s] = dc.cpu()
        k.lstm_enc_bwd_step(dz, dev[0], dout, dev[1], dc, dev[2], dev[3], dev[4], s, T, B, H)
        cout[s] = dc.cpu()
    torch.cuda.synchronize()
    assert _untouched(t0, t1)
    got = {"dz": dz.cpu(), "dc": cout[0], "carry_in": cin, "carry_out": cout, "dz_bf16": 1.0}
    _assert_bwd_bounds(f"bwd_step H={H} B={B}", x, _bwd_errors(x, got), step=True)


@pytest.mark.parametrize("H,B,T,fwd,rows_bwd,multi", PERSISTENT)
def test_lstm_bwd_persistent(H, B, T, fwd, rows_bwd, multi):
    """dz, the final dc_carry and dbias; dbias = None and the other dout forms give the same bits."""
    k = _ops()
    _assert_variant(k, H, B, fwd, rows_bwd, multi)
    x = _bwd_case(H, B, T)
    forms = [0, 1, 2] if (H, B, T) in ALL_DOUT_FORMS else [PERSISTENT.index((H, B, T, fwd, rows_bwd, multi)) % 3]
    got = _run_bwd_persistent(k, x, forms[0], True)
    for form in forms[1:] + forms[:1]:  # the remaining forms, and the first once more without dbias
        other = _run_bwd_persistent(k, x, form, False)
        assert torch.equal(_bits(other["dz"]), _bits(got["dz"])), ("dz", forms[0], form)
        assert torch.equal(_bits(other["dc"]), _bits(got["dc"])), ("dc_carry", forms[0], form)
    _assert_bwd_bounds(f"bwd_persistent[{rows_bwd}] H={H} B={B} T={T} dout={forms}", x, _bwd_errors(x, got))


# ------------------------------------------------------------------ the 16-row BPTT switch, in a child
def _bwd16_child():
    """Runs with TSAMD_LSTM_BWD32=0 (read once per process): (512, 264) then takes the 16-row BPTT
    lstm_bwd_persistent_kernel<512, 8> on 17 row tiles, the last one holding 8 rows."""
    k = _ops()
    H, B, T = 512, 264, 5
    NC, tiles = H // 64, (B + 15) // 16
    assert int(k.lstm_persistent_grid(H, B)) > 0
    assert int(k.lstm_persistent_xbuf(H, B, True)) == 2 * tiles * 2 * NC * NC * 16 * 64, "not the 16-row BPTT"
    assert int(k.lstm_persistent_xbuf(H, B, False)) == 2 * ((B + 31) // 32) * 2 * 32 * (H // 2), "forward tile changed"
    x = _bwd_case(H, B, T)
    got = _run_bwd_persistent(k, x, 0, True)
    for form in (1, 2, 0):
        other = _run_bwd_persistent(k, x, form, False)
        assert torch.equal(_bits(other["dz"]), _bits(got["dz"])), ("dz", form)
        assert torch.equal(_bits(other["dc"]), _bits(got["dc"])), ("dc_carry", form)
    _assert_bwd_bounds(f"bwd_persistent[16, TSAMD_LSTM_BWD32=0] H={H} B={B} T={T} dout=[0, 1, 2] "
                       f"launches={int(k.lstm_persistent_launches(H, B))}", x, _bwd_errors(x, got))
    print("RESULT ok")


def test_lstm_bwd_persistent_16_row_switch():
    """TSAMD_LSTM_BWD32=0 at (512, 264): the 16-row BPTT above batch 256.  The switch is read once per
    process, so the case runs in a fresh child (this file as a script), under a time limit."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TSAMD_LSTM_BWD32="0", PYTHONPATH=repo)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--bwd16-child"], env=env, capture_output=True,
                       text=True, timeout=120, cwd=repo)
    print(r.stdout)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ perturbed kernel outputs
def test_perturbed_kernel_outputs_are_rejected():
    """What lstm_fwd_persistent wrote at (64, 19) passes; the same tensors with 1e-4 added to one cs
    element, with gates j and f swapped in acts, and with the bw half of out moved to t = s do not."""
    H, B, T = 64, 19, 5
    x = _fwd_case(H, B, T, False)
    got = _run_fwd(_ops(), x, "persistent")
    _assert_bounds("unperturbed", x, _fwd_errors(x, got))
    cs = got["cs"].clone()
    cs[1, 2, 0, H // 2] += 1e-4
    with pytest.raises(AssertionError, match="'c'"):
        _assert_bounds("cs + 1e-4", x, _fwd_errors(x, dict(got, cs=cs)))
    with pytest.raises(AssertionError, match="'j'"):
        _assert_bounds("gate swap", x, _fwd_errors(x, dict(got, acts=got["acts"][..., [0, 2, 1, 3]])))
    out = got["out"].clone()
    out[:, :, H:] = 0
    for s in range(T):
        live = _live(x["lens"], T)[s]
        out[live, s, H:] = got["hs"][1, s + 1][live]
    with pytest.raises(AssertionError, match="out != hs"):
        _fwd_errors(x, dict(got, out=out))


# ------------------------------------------------------------------ script: the bound table, mutations
MUTATIONS = {"no_forget_bias": "fwd", "gate_swap": "fwd", "bw_at_s": "fwd", "cs_1e-4": "fwd", "dh_fin_late": "bwd"}


def mutation_failures(H=64, B=19, T=5):
    """{mutation: the check that rejects it}, the fp32 emulation standing in for the kernel (CPU)."""
    caught = {}
    for mut, side in MUTATIONS.items():
        try:
            if side == "fwd":
                x = _fwd_case(H, B, T, False)
                got = _emul_fwd(x, mut)
                del got["h32"]  # judged like a kernel: by the bf16 hs it stored
                _assert_bounds(mut, x, _fwd_errors(x, got))
            else:
                x = _bwd_case(H, B, T)
                got = _emul_bwd(x, False, mut)
                got.update(dz=got.pop("dz_operand"), dz_bf16=1.0)
                _assert_bwd_bounds(mut, x, _bwd_errors(x, got))
        except AssertionError as e:
            caught[mut] = str(e.args[0]) if e.args else "assert"
        else:
            caught[mut] = None
    return caught


def measure(fwd=None, bwd_step=None, bwd=None, verbose=True):
    """{T: {quantity: max |fp32 torch - float64|}} over the given cases (default: every case of the module)"""
    worst = {T: {q: 0.0 for q in tab} for T, tab in FP32_TORCH_ERR.items()}

    def upd(T, res, keys, line):
        row = {}
        for q, (err, _) in res.items():
            if q == "dbias":
                continue
            row[q] = float(err.max()) if err.numel() else 0.0
            worst[T][keys.get(q, q)] = max(worst[T][keys.get(q, q)], row[q])
        if verbose:
            print(line + " " + " ".join(f"{q}={e:.3g}" for q, e in row.items()), flush=True)

    if fwd is None:
        bwd_step, bwd = STEP_SHAPES, [c[:3] for c in PERSISTENT]
        fwd = [(H, B, 5, False) for H, B in STEP_SHAPES] + [c[:3] + (False,) for c in PERSISTENT] + [c[:3] + (True,) for c in FX_SHAPES]
    for H, B, T, fx in fwd:
        x = _fwd_case(H, B, T, fx)
        upd(T, _fwd_errors(x, _emul_fwd(x)), {}, f"fwd H={H:3d} B={B:3d} T={T:2d} fx={fx!s:5}:")
    for H, B in bwd_step:
        x = _bwd_case(H, B, 5)
        upd(5, _bwd_errors(x, _emul_bwd(x, True)), {"dz": "step_dz", "dc_carry": "step_dc_carry"}, f"bwd_step H={H:3d} B={B:3d}:")
    for H, B, T in bwd:
        x = _bwd_case(H, B, T)
        upd(T, _bwd_errors(x, _emul_bwd(x, False)), {}, f"bwd H={H:3d} B={B:3d} T={T:2d}:")
    return worst


if __name__ == "__main__":  # the fp32 formulas' own rounding on the test inputs (CPU only)
    if "--bwd16-child" in sys.argv:
        _bwd16_child()
    elif "--mutations" in sys.argv:
        for mut, why in mutation_failures().items():
            print(f"{mut}: {'NOT CAUGHT' if why is None else 'caught: ' + why}")
    else:
        for T, tab in measure().items():
            print(f"measured T={T}: " + ", ".join(f'"{q}": {e:.3g}' for q, e in tab.items()))
            print(f"in the module T={T}: " + ", ".join(f'"{q}": {e:.3g}' for q, e in FP32_TORCH_ERR[T].items()))
