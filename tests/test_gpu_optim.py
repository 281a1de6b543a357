"""clip_adagrad (csrc/kernels/optim.hip: sumsq + adagrad, two launches) against the closed form
in float64:

    norm  = gscale * sqrt(sum g^2)
    scale = gscale * (max_norm / max(norm, max_norm) if max_norm > 0 else 1)
    g'    = g * scale;  acc' = acc + g'^2;  w' = w - lr * g' / sqrt(acc')

The reference is evaluated on exactly the fp32 values the kernel receives (lr, max_norm and
gscale rounded to fp32 as the binding does).

Sizes: 1, 3, 4 (tail only / one float4), 1027 (float4 loop + 3-element tail) and 1 049 779
(> 4 * 1024 * 256: second trip of the grid-stride loop, and a 3-element tail).

Bounds (profiles/train_tail_tests.md): the same formulas evaluated in fp32 torch on these very
inputs differ from the float64 reference by at most FP32_TORCH_ERR per element (run this file as
a script to re-measure); the kernel is allowed 8 x that (rsqrtf, the two-level sum order, FMA
contraction).  |g| is kept within [0.5, 2] x a common magnitude and |w| <= 0.02, so every update
is far above the rounding of w and the relative error per element is meaningful.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 1027, 1049779]
LR = 0.15
# per-element maximum over every finite-path case below of the fp32-torch evaluation against the
# float64 reference (relative error; measured on the CPU, see __main__)
FP32_TORCH_ERR = {"norm": 5.16e-8, "acc": 2.26e-7, "dw": 1.36e-6}
BOUND = {k: 8.0 * v for k, v in FP32_TORCH_ERR.items()}
CLIPS = {"noclip": 2.0, "clip20x": 0.05, "off": 0.0}  # max_norm as a multiple of the true norm


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _inputs(n, seed=0):
    gen = torch.Generator().manual_seed(1000 + n + seed)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    g = sign * (0.5 + 1.5 * torch.rand(n, generator=gen)) * 0.3
    w = (torch.rand(n, generator=gen) - 0.5) * 0.04
    acc = 0.1 + 0.05 * torch.rand(n, generator=gen)
    return w, acc, g


def _max_norm(g, gscale, clip):
    """max_norm of the case (fp32-rounded): a multiple of the step's own norm, 0 = clipping off."""
    return _f32(CLIPS[clip] * gscale * float(g.double().pow(2).sum().sqrt()))


def _formulas(w, acc, g, lr, max_norm, gscale):
    """The documented update in the dtype of the inputs (float64: the reference; float32: its own
    rounding error)."""
    norm = gscale * g.pow(2).sum().sqrt()
    scale = gscale * (max_norm / torch.clamp(norm, min=max_norm) if max_norm > 0 else 1.0)
    g2 = g * scale
    acc2 = acc + g2 * g2
    return norm, acc2, w - lr * g2 / acc2.sqrt()


def _reference(w, acc, g, lr, max_norm, gscale):
    norm, acc2, w2 = _formulas(w.double(), acc.double(), g.double(), _f32(lr), max_norm, gscale)
    return norm, acc2, w2 - w.double()


def _rel(x, ref, floor=1e-30):
    """max relative error per element; elements with |ref| below the floor are measured against
    the floor (absolute)."""
    return float(((x - ref).abs() / ref.abs().clamp_min(floor)).max())


def _errors(norm, acc2, w2, w0, ref):
    rn, ra, rd = ref
    return {"norm": _rel(norm.double().reshape(()), rn), "acc": _rel(acc2.double(), ra),
            "dw": _rel(w2.double() - w0.double(), rd)}


def _run(k, w, acc, g, lr, max_norm, gscale, flag0=0, skip=None):
    """One clip_adagrad call on fresh device copies; returns host copies of what it wrote."""
    wd, ad, gd = w.cuda(), acc.cuda(), g.cuda()
    part = torch.zeros(int(k.opt_parts()), device="cuda")
    norm = torch.full((1,), -1.0, device="cuda")
    flag = torch.full((1,), flag0, dtype=torch.int32, device="cuda")
    sk = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda")
    k.clip_adagrad(wd, ad, gd, part, lr, max_norm, gscale, norm, flag, sk)
    torch.cuda.synchronize()
    return wd.cpu(), ad.cpu(), norm.cpu(), int(flag.item())


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


@pytest.mark.parametrize("skip", [None, 0], ids=["skip=None", "skip=0"])
@pytest.mark.parametrize("gscale", [1.0, 0.25], ids=["gscale=1", "gscale=0.25"])
@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("n", SIZES)
def test_update_matches_fp64(n, clip, gscale, skip):
    """Finite path: norm_out, acc and w - w0 against float64 at every size, for norm < max_norm
    (noclip), norm = 20 max_norm (clip20x: the gradient is scaled by 1/20), max_norm = 0 (off),
    with and without the data-parallel gscale, skip absent or a zero word; flag untouched."""
    k = _ops()
    w, acc, g = _inputs(n)
    mn = _max_norm(g, gscale, clip)
    ref = _reference(w, acc, g, LR, mn, gscale)
    if clip == "clip20x":  # the branch really scales by 10 x or more
        assert float(ref[0]) >= 10 * mn > 0
    for flag0 in (0, 2):
        w2, a2, norm, flag = _run(k, w, acc, g, LR, mn, gscale, flag0=flag0, skip=skip)
        err = _errors(norm, a2, w2, w, ref)
        print(f"[train-tail] clip_adagrad n={n} {clip} gscale={gscale} skip={skip}: " +
              " ".join(f"{q}={e:.3g}" for q, e in err.items()))
        for q, e in err.items():
            assert e <= BOUND[q], (q, e, BOUND[q])
        assert flag == flag0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("n,pos", [(1, 0), (1027, 513), (1027, 1026), (1049779, 1049000), (1049779, 1049778)])
def test_nonfinite_gradient_is_not_applied(n, pos, bad):
    """NaN guard: one non-finite gradient element (in the float4 body or in the scalar tail, in the
    first or the second grid-stride trip) leaves w and acc bit-identical, sets flag bit 0 (OR-ed
    into what is there: 2 -> 3) and reports a non-finite norm."""
    k = _ops()
    w, acc, g = _inputs(n)
    g[pos] = bad
    for flag0 in (0, 2):
        w2, a2, norm, flag = _run(k, w, acc, g, LR, 2.0, 1.0, flag0=flag0, skip=0)
        assert torch.equal(w2, w) and torch.equal(a2, acc)
        assert flag == (flag0 | 1)
        assert not torch.isfinite(norm).item()


@pytest.mark.parametrize("word", [1, -7])
@pytest.mark.parametrize("n", [3, 1027, 1049779])
def test_skip_word_is_not_applied(n, word):
    """A non-zero skip word with a finite gradient: w and acc bit-identical, flag bit 1 set and
    bit 0 clear; the norm is still reported."""
    k = _ops()
    w, acc, g = _inputs(n)
    mn = _max_norm(g, 1.0, "noclip")
    w2, a2, norm, flag = _run(k, w, acc, g, LR, mn, 1.0, flag0=0, skip=word)
    assert torch.equal(w2, w) and torch.equal(a2, acc)
    assert flag == 2
    assert _rel(norm.double().reshape(()), _reference(w, acc, g, LR, mn, 1.0)[0]) <= BOUND["norm"]
    # both guards at once: both bits
    g[n // 2] = float("nan")
    w2, a2, norm, flag = _run(k, w, acc, g, LR, mn, 1.0, flag0=0, skip=word)
    assert torch.equal(w2, w) and torch.equal(a2, acc)
    assert flag == 3


@pytest.mark.parametrize("n", [1027, 1049779])
def test_flag_reports_and_does_not_latch(n):
    """optim.hip only ORs bits into *flag and never reads it back: on the same buffers, a guarded
    step (NaN gradient) followed by a finite one with the flag left set applies the finite step in
    full and leaves the flag as it was."""
    k = _ops()
    w, acc, g = _inputs(n)
    mn = _max_norm(g, 0.25, "clip20x")
    wd, ad = w.cuda(), acc.cuda()
    part = torch.zeros(int(k.opt_parts()), device="cuda")
    norm = torch.zeros(1, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    skip = torch.zeros(1, dtype=torch.int32, device="cuda")
    gbad = g.clone()
    gbad[n - 1] = float("nan")
    k.clip_adagrad(wd, ad, gbad.cuda(), part, LR, mn, 0.25, norm, flag, skip)
    assert int(flag.item()) == 1
    assert torch.equal(wd.cpu(), w) and torch.equal(ad.cpu(), acc)
    k.clip_adagrad(wd, ad, g.cuda(), part, LR, mn, 0.25, norm, flag, skip)
    assert int(flag.item()) == 1
    err = _errors(norm.cpu(), ad.cpu(), wd.cpu(), w, _reference(w, acc, g, LR, mn, 0.25))
    for q, e in err.items():
        assert e <= BOUND[q], (q, e, BOUND[q])


if __name__ == "__main__":  # the reference's own rounding: fp32 torch vs float64 on the test inputs (CPU)
    worst = {q: 0.0 for q in FP32_TORCH_ERR}
    for n in SIZES:
        for clip in CLIPS:
            for gscale in (1.0, 0.25):
                w, acc, g = _inputs(n)
                mn = _max_norm(g, gscale, clip)
                norm, a2, w2 = _formulas(w, acc, g, _f32(LR), mn, gscale)
                err = _errors(norm, a2, w2, w, _reference(w, acc, g, LR, mn, gscale))
                print(f"n={n:8d} {clip:8s} gscale={gscale:4}: " + " ".join(f"{q}={e:.3g}" for q, e in err.items()))
                worst = {q: max(worst[q], e) for q, e in err.items()}
    print("max:", {q: f"{e:.3g}" for q, e in worst.items()})
