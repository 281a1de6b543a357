"""reduce_states (csrc/kernels/reduce_states.hip) against float64 torch, EXACTLY:

    rs_fwd:  pre = [x_fw, x_bw] . W + b ;  c0 / h0 = relu(pre)     (x = row T of the step frames)
    rs_bwd:  dp = g [pre > 0] ;  gb += sum_rows dp ;  d_old = dp . W^T  (fw half at 0, bw at + B H)

Every MFMA operand is a dyadic rational -- states and upstream gradients multiples of 1/16 in
[-2, 2] (so the fp32 ones are bf16 numbers: the kernels round them to bf16 on load), weights
multiples of 1/64 in [-1/8, 1/8], biases and prefills multiples of 2^-10 -- and each test asserts
on its float64 reference that sum |terms| < 2^14, so every partial sum is an fp32 number whatever
the order (k-slices, atomics) and every output must be torch.equal to the reference.

H = 32, 96, 256, 512 (the kernels' limit: H % 32 == 0, H <= 512); B = 1, 16, 19, 33 (full and
partial last tiles, up to three row tiles).  Outputs are prefilled with NaN and followed by
sentinel rows.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HS = [32, 96, 256, 512]
ROWS = [1, 16, 19, 33]
SENT = 12288.0  # exact in bf16
NAN = float("nan")
BF = torch.bfloat16
TINY = 1.1754943508222875e-38  # the smallest positive normal fp32


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _acts(g, *shape):
    return torch.randint(-32, 33, shape, generator=g).float() / 16


def _wts(g, *shape):
    return (torch.randint(-8, 9, shape, generator=g).float() / 64).bfloat16()


def _adds(g, *shape):
    return torch.randint(-1024, 1025, shape, generator=g).float() / 1024


def _assert_exact(ref, mag):
    assert float(mag.max()) < 2 ** 14
    assert torch.equal((ref * 1024).round(), ref * 1024)
    assert torch.equal(ref.float().double(), ref)


def _out(rows, width, dtype, fill=NAN):
    """[rows][width] prefilled with ``fill``, and the sentinel rows behind it (to the end of the
    last 16-row tile, plus one)"""
    alloc = (rows + 15) // 16 * 16 + 1
    full = torch.full((alloc, width), SENT, dtype=dtype, device="cuda")
    full[:rows].fill_(fill)
    return full[:rows], full[rows:]


def _untouched(*tails):
    return all(bool((t == SENT).all()) for t in tails)


@functools.lru_cache(maxsize=None)
def _weights(H):
    g = _gen(H, 1)
    return {"RC": _wts(g, 2 * H, H), "RH": _wts(g, 2 * H, H), "bc": _adds(g, H), "bh": _adds(g, H)}


# ------------------------------------------------------------------ rs_fwd
@pytest.mark.parametrize("cat", [True, False], ids=["cat", "nocat"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H", HS)
def test_rs_fwd(H, B, T, cat):
    """Row T of both directions is read and no other (the rest of the frames is NaN); pre exact,
    c0 / c0b / h0b its ReLU (bf16: rounded), cat_c / cat_h the bf16 of the concatenated inputs,
    not written when None."""
    k, w = _ops(), _weights(H)
    g = _gen(H, B, T, 2)
    cs = torch.full((2, T + 1, B, H), NAN)
    hs = torch.full((2, T + 1, B, H), NAN, dtype=BF)
    cs[:, T] = _acts(g, 2, B, H)
    hs[:, T] = _acts(g, 2, B, H).bfloat16()
    xc = torch.cat([cs[0, T], cs[1, T]], 1).double()   # [B][2H]
    xh = torch.cat([hs[0, T], hs[1, T]], 1).double()
    ref = {}
    for n, x, W, b in (("c", xc, w["RC"], w["bc"]), ("h", xh, w["RH"], w["bh"])):  # W: [2H][H] (TF layout)
        pre = x @ W.double() + b.double()
        _assert_exact(pre, x.abs() @ W.double().abs() + b.double().abs())
        ref[n] = pre.float()
    o = {"pre_c": _out(B, H, torch.float32), "pre_h": _out(B, H, torch.float32), "c0": _out(B, H, torch.float32),
         "c0b": _out(B, H, BF), "h0b": _out(B, H, BF), "cat_c": _out(B, 2 * H, BF), "cat_h": _out(B, 2 * H, BF)}
    k.rs_fwd(cs.cuda(), hs.cuda(), T, w["RC"].t().contiguous().cuda(), w["RH"].t().contiguous().cuda(), w["bc"].cuda(),
             w["bh"].cuda(), o["pre_c"][0], o["pre_h"][0], o["c0"][0], o["c0b"][0], o["h0b"][0],
             o["cat_c"][0] if cat else None, o["cat_h"][0] if cat else None, B, H)
    torch.cuda.synchronize()
    assert _untouched(*(t for _, t in o.values()))
    got = {n: v.cpu() for n, (v, _) in o.items()}
    assert torch.equal(got["pre_c"], ref["c"]) and torch.equal(got["pre_h"], ref["h"])
    assert torch.equal(got["c0"], ref["c"].relu())
    assert torch.equal(got["c0b"], ref["c"].relu().bfloat16()) and torch.equal(got["h0b"], ref["h"].relu().bfloat16())
    if cat:
        assert torch.equal(got["cat_c"], xc.bfloat16()) and torch.equal(got["cat_h"], xh.bfloat16())
    else:
        assert bool(torch.isnan(got["cat_c"]).all()) and bool(torch.isnan(got["cat_h"]).all())


# ------------------------------------------------------------------ rs_bwd
def _pre(g, B, H):
    """Pre-activations of both signs with the edges of the mask pre > 0 in the first and the last
    row: exact 0.0 and -0.0 (masked), the smallest positive normal (passes)."""
    pre = torch.randn(B, H, generator=g)
    for r in (0, B - 1):
        pre[r, 0], pre[r, 1], pre[r, 2], pre[r, 3] = 0.0, -0.0, TINY, -TINY
    return pre


@pytest.mark.parametrize("bias", [True, False], ids=["gb", "nogb"])
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("H", HS)
def test_rs_bwd(H, B, bias):
    """dpc / dph = bf16(g [pre > 0]); dold_c / dold_h = dp . W^T in both halves; gbc / gbh
    accumulate the column sums of dp onto what they hold, or are not written when None."""
    k, w = _ops(), _weights(H)
    g = _gen(H, B, 3)
    x = {"gc": _acts(g, B, H), "gh": _acts(g, B, H), "pre_c": _pre(g, B, H), "pre_h": _pre(g, B, H)}
    x["gc"][:, :4] = 1.5   # a gradient behind every edge value of the mask
    x["gh"][:, :4] = -0.75
    gb0 = {"c": _adds(g, H), "h": _adds(g, H)}
    ref = {}
    for n in "ch":
        dp = (x["g" + n] * (x["pre_" + n] > 0)).double()
        W = w["R" + n.upper()].double()   # [2H][H]
        dold = dp @ W.t()                 # [B][2H]
        _assert_exact(dold, dp.abs() @ W.abs().t())
        gb = gb0[n].double() + dp.sum(0)
        _assert_exact(gb, gb0[n].double().abs() + dp.abs().sum(0))
        ref[n] = {"dp": dp.bfloat16(), "dold": torch.stack([dold[:, :H], dold[:, H:]]).float(), "gb": gb.float()}
        assert torch.equal(ref[n]["dp"].double(), dp)
    assert ref["c"]["dp"][0, 0] == 0 and ref["c"]["dp"][0, 1] == 0 and ref["c"]["dp"][0, 2] == 1.5 and ref["c"]["dp"][0, 3] == 0
    o = {"dpc": _out(B, H, BF), "dph": _out(B, H, BF), "dold_c": _out(2 * B, H, torch.float32),
         "dold_h": _out(2 * B, H, torch.float32)}
    gbc, gbct = _out(1, H, torch.float32)
    gbh, gbht = _out(1, H, torch.float32)
    gbc.copy_(gb0["c"][None])
    gbh.copy_(gb0["h"][None])
    k.rs_bwd(x["gc"].cuda(), x["gh"].cuda(), x["pre_c"].cuda(), x["pre_h"].cuda(), w["RC"].cuda(), w["RH"].cuda(),
             o["dpc"][0], o["dph"][0], gbc[0] if bias else None, gbh[0] if bias else None, o["dold_c"][0], o["dold_h"][0],
             B, H)
    torch.cuda.synchronize()
    assert _untouched(gbct, gbht, *(t for _, t in o.values()))
    assert torch.equal(o["dpc"][0].cpu(), ref["c"]["dp"]) and torch.equal(o["dph"][0].cpu(), ref["h"]["dp"])
    assert torch.equal(o["dold_c"][0].cpu().view(2, B, H), ref["c"]["dold"])
    assert torch.equal(o["dold_h"][0].cpu().view(2, B, H), ref["h"]["dold"])
    if bias:
        assert torch.equal(gbc[0].cpu(), ref["c"]["gb"]) and torch.equal(gbh[0].cpu(), ref["h"]["gb"])
    else:
        assert torch.equal(gbc[0].cpu(), gb0["c"]) and torch.equal(gbh[0].cpu(), gb0["h"])
