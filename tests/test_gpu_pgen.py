"""The p_gen gradient kernels (csrc/kernels/decoder.hip: pgen_dirs, pgen_bwd) against float64
torch, EXACTLY.  With dp = dL/d(p_gen pre-activation) [N] and the p_gen weight
w = [w_ctx | w_c | w_h | w_x] (A + 2H + E):

    pgen_dirs:  dCTX_dir += dp w_ctx,  dC_dir = dp w_c,  dH_dir += dp w_h,  dX_dir = dp w_x,
                gb += sum(dp)
    pgen_bwd:   gw[k] += sum_n dp[n] [ctx, c, h, x][n][k]

One factor of every product is a multiple of 1/16 in [-2, 2] and the other a multiple of 1/64 in
[-1/8, 1/8]; prefills are multiples of 2^-10.  Every product and partial sum is a multiple of 2^-10
and each test asserts sum |terms| < 2^14 on its float64 reference, so the results are fp32 numbers
whatever the order (row splits, 4-way unroll, atomics) and must be torch.equal to the reference.

The bindings put no constraint on the widths: (A, H, E) = (100, 36, 20) has none that is a
multiple of 64 (every lane loop has a partial trip), (160, 96, 48) gives A + 2H + E = 400 (two
column blocks of pgen_bwd, the second guarded), (512, 256, 128) is the shipped shape.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [(100, 36, 20), (160, 96, 48), (512, 256, 128)]
SENT = 12288.0
NAN = float("nan")


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _sixteenths(g, *shape):
    return torch.randint(-32, 33, shape, generator=g).float() / 16


def _sixtyfourths(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 64


def _adds(g, *shape):
    return torch.randint(-1024, 1025, shape, generator=g).float() / 1024


def _assert_exact(ref, mag):
    assert float(mag.max()) < 2 ** 14
    assert torch.equal((ref * 1024).round(), ref * 1024)
    assert torch.equal(ref.float().double(), ref)


def _out(numel, fill):
    """numel fp32 values on the device (a tensor or a fill value) and 64 sentinels behind them"""
    full = torch.full((numel + 64,), SENT, device="cuda")
    if torch.is_tensor(fill):
        full[:numel].copy_(fill.reshape(-1))
    else:
        full[:numel].fill_(fill)
    return full[:numel], full[numel:]


@pytest.mark.parametrize("bias", [True, False], ids=["gb", "nogb"])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("A,H,E", WIDTHS)
def test_pgen_dirs(A, H, E, N, bias):
    """dctx and dh accumulate onto their prefill, dc and dx are stored over NaN, gb accumulates
    sum(dp) (one atomic per workgroup of 4 rows) or is skipped when None."""
    k = _ops()
    g = _gen(A, H, E, N, 1)
    dp, w = _sixteenths(g, N), _sixtyfourths(g, A + 2 * H + E)
    pre = {"dctx": _adds(g, N, A), "dh": _adds(g, N, H)}
    gb0 = _adds(g, 1)
    d, wd = dp.double()[:, None], w.double()
    ref = {"dctx": pre["dctx"].double() + d * wd[None, :A], "dc": d * wd[None, A:A + H],
           "dh": pre["dh"].double() + d * wd[None, A + H:A + 2 * H], "dx": d * wd[None, A + 2 * H:],
           "gb": gb0.double() + dp.double().sum()}
    for r in ref.values():  # |prefill| <= 1 and |dp w| <= 1/4 per element; gb: 1 + sum |dp|
        _assert_exact(r, torch.tensor(1.0) + dp.double().abs().sum())
    o = {"dctx": _out(N * A, pre["dctx"]), "dc": _out(N * H, NAN), "dh": _out(N * H, pre["dh"]), "dx": _out(N * E, NAN),
         "gb": _out(1, gb0)}
    k.pgen_dirs(dp.cuda(), w.cuda(), o["dctx"][0], o["dc"][0], o["dh"][0], o["dx"][0], o["gb"][0] if bias else None,
                N, A, H, E)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for _, t in o.values())
    for n in ("dctx", "dc", "dh", "dx"):
        assert torch.equal(o[n][0].cpu(), ref[n].float().reshape(-1)), n
    assert torch.equal(o["gb"][0].cpu(), ref["gb"].float() if bias else gb0)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 130, 1000])
@pytest.mark.parametrize("A,H,E", WIDTHS)
def test_pgen_bwd(A, H, E, N):
    """The column sums over the row splits (pgen_bwd_splits: ceil(N / 64) of them up to 2048 per
    column block; N = 63 / 64 / 65 / 130 / 1000 give 1, 1, 2, 3 and 16 splits, the last one short,
    and row counts with every remainder of the 4-way unroll).  The launcher finishes with
    launch_colsum_det(..., acc = true): out[c] = out[c] + t, so gw ACCUMULATES -- the result is
    the prefilled gw plus the column sums (the engine hands it the zeroed gradient slot).  Two
    runs give the same bits."""
    k = _ops()
    g = _gen(A, H, E, N, 2)
    Kt = A + 2 * H + E
    ctx, c, h, x = _sixteenths(g, N, A), _sixteenths(g, N, H), _sixteenths(g, N, H).bfloat16(), _sixteenths(g, N, E)
    dp, gw0 = _sixtyfourths(g, N), _adds(g, Kt)
    feats = torch.cat([ctx, c, h.float(), x], 1).double()   # [N][Kt]
    ref = gw0.double() + dp.double() @ feats
    _assert_exact(ref, gw0.double().abs() + dp.double().abs() @ feats.abs())
    dev = [t.cuda() for t in (ctx, c, h, x, dp)]
    outs = []
    for _ in range(2):
        gw, tail = _out(Kt, gw0)
        k.pgen_bwd(*dev, gw, N, A, H, E, True)
        torch.cuda.synchronize()
        assert bool((tail == SENT).all())
        outs.append(gw.cpu())
    assert torch.equal(outs[0], ref.float())
    assert torch.equal(outs[0], outs[1])
