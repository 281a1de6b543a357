"""dec_fwd_persistent (csrc/kernels/decoder_persistent.hip): the decoder forward loop as ONE
persistent launch with per-tile hand-offs, against

* the three-kernel chain it replaces (dec_cell_fwd -> dec_sproj -> attn_fwd_rowp per step): the
  kernel keeps their arithmetic and summation order, so every output must be bit-equal;
* an fp32 PyTorch computation of every step on the same bf16 operands (the step's inputs as the
  kernel saw them: h, c, g of the previous step, the coverage so far).  Bounds, from the existing
  per-kernel tests: the attention outputs 2e-3 of the largest reference magnitude (fp32) and 1e-2
  (bf16), as test_gpu_attention_ops applies to attn_fwd_rowp; S an absolute error below
  1e-3 max|ref| + 1e-4, as test_gpu_decode.py::test_linear2_matches_fp32 applies to linear2.  The
  cell (dec_cell_fwd) and dec_sproj are checked on their own against float64 in
  test_gpu_decoder_ops.py; here the cell's fp32-accumulated bf16 MFMA sums and v_exp / v_rcp
  activations are held to the attention's bounds.

Shapes: H = 256, E = 128, A = 512, D = 4, T = 24; B = 16 (one team), 48 (three teams: not a multiple
of the 8 XCDs), 144 (more than one team per XCD).  Encoder lengths include 1, 5 (not a multiple of
4) and T; dlen has a row dead from step 1, a whole tile dead from step 2, live tiles with dead rows
and rows dead from step 0.  Outputs are prefilled with NaN and followed by sentinels."""
import pytest
import torch

H, E, A, D, T = 256, 128, 512, 4, 24
KF = 2.8853900817779268  # 2 log2(e): F is stored pre-scaled by it (attn_common.h)
SENT = 12288.0  # (exact in bf16)
OUT = ("Cst", "Cb", "Hb", "ACT", "S", "COV", "ATT", "ATTb", "covloss", "GV", "GVb")


def _k():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _need(k, B):
    """The kernel's own launch rule (the engine falls back; a bare-kernel test cannot run)."""
    cap = int(k.dec_persistent_capacity())
    assert cap > 0, "the occupancy query does not admit dec_fwd_persistent"
    if int(k.dec_persistent_grid(B)) > cap:
        pytest.skip("the persistent decoder grid is not co-resident on this device")


def _inputs(B, seed, salt=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def r(*shape, s=1.0):
        return torch.randn(*shape, generator=g, device="cuda") * s

    x = {
        "XG": r(D, B, 4 * H, s=0.5), "KcT": r(4 * H, E + H, s=0.05).bfloat16(), "WsT": r(A, 2 * H, s=0.05).bfloat16(),
        "bs": r(A, s=0.1), "h0": r(B, H, s=0.5).bfloat16(), "c0": r(B, H, s=0.5),
        "F": (r(B, T, A, s=0.5) * KF).bfloat16(), "G": r(B, T, E, s=0.5).bfloat16(), "v": r(A, s=0.1),
        "wc": r(A, s=0.5),
    }
    lens = torch.tensor([1, 5, T, 22, 7, 24, 13, 2], dtype=torch.int32, device="cuda").repeat(B // 8)
    dlen = torch.full((B,), D, dtype=torch.int32, device="cuda")
    dlen[3] = 1                      # a row dead from step 1 in a live tile
    dlen[9] = 0                      # dead from step 0
    if B >= 48:
        dlen[16:32] = 2              # a whole tile dead from step 2
        dlen[20] = 1
        dlen[32:48] = torch.tensor([4, 3, 2, 1] * 4, dtype=torch.int32)  # a live tile with dead rows
    if B >= 144:
        dlen[48:64] = 0              # a tile that never runs
        dlen[128:144] = torch.randint(0, D + 1, (16,), generator=g, device="cuda").int()
    x["lens"], x["dlen"] = lens, dlen
    if salt:
        x["XG"] += 0.01 * salt
    return x


def _outputs(B, cov):
    """NaN-prefilled outputs, each followed by 64 sentinels; step 0 state and coverage set by the caller."""
    shapes = {"Cst": (D + 1, B, H), "Cb": (D + 1, B, H), "Hb": (D + 1, B, H), "ACT": (D, B, 4 * H), "S": (D, B, A),
              "COV": (D + 1, B, T), "ATT": (D, B, T), "ATTb": (D, B, T), "covloss": (D, B), "GV": (D, B, E),
              "GVb": (D, B, E)}
    o, full = {}, {}
    for n, shp in shapes.items():
        dt = torch.bfloat16 if n in ("Cb", "Hb", "ATTb", "GVb") else torch.float32
        numel = 1
        for d in shp:
            numel *= d
        full[n] = torch.full((numel + 64,), SENT, device="cuda", dtype=dt)
        o[n] = full[n][:numel].view(shp)
        o[n].fill_(float("nan"))
    o["_full"] = full
    return o


def _start(o, x):
    o["Cst"][0].copy_(x["c0"])
    o["Hb"][0].copy_(x["h0"])
    o["Cb"][0].copy_(x["c0"])
    o["COV"][0].zero_()


def _run_persistent(k, x, B, cov, o=None, err=None, xbuf=None):
    o = o or _outputs(B, cov)
    _start(o, x)
    err = torch.zeros(1, dtype=torch.int32, device="cuda") if err is None else err
    xbuf = torch.zeros(int(k.dec_persistent_xbuf(B)), dtype=torch.long, device="cuda") if xbuf is None else xbuf
    xbuf.zero_()
    k.dec_fwd_persistent(x["XG"], x["KcT"], x["WsT"], x["bs"], o["Cst"], o["Cb"], o["Hb"], o["ACT"], o["S"], x["F"],
                         x["G"], x["v"], x["wc"] if cov else None, o["COV"] if cov else None, x["lens"], o["ATT"],
                         o["ATTb"], o["covloss"] if cov else None, o["GV"], o["GVb"], x["dlen"], xbuf, err, B, T, D,
                         H, E, A)
    return o, err


def _run_chain(k, x, B, cov):
    o = _outputs(B, cov)
    _start(o, x)
    dl = x["dlen"]
    for t in range(D):
        k.dec_cell_fwd(x["XG"][t], o["GVb"][t - 1] if t > 0 else None, o["Hb"][t], o["Cst"][t], x["KcT"],
                       o["Cst"][t + 1], o["Cb"][t + 1], o["Hb"][t + 1], o["ACT"][t], B, H, E, dl, t)
        k.dec_sproj(o["Cb"][t + 1], o["Hb"][t + 1], x["WsT"], x["bs"], o["S"][t], B, H, A, dl, t)
        k.attn_fwd_rowp(x["F"], x["G"], o["S"][t], x["v"], x["wc"] if cov else None,
                        o["COV"][t] if (cov and t > 0) else None, x["lens"], o["ATT"][t],
                        o["COV"][t + 1] if cov else None, o["covloss"][t] if cov else None, o["GV"][t], o["GVb"][t],
                        B, T, A, dl, t, o["ATTb"][t])
    return o


def _same(a, b):
    return torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))


def _close(name, got, ref, tol):
    err = float((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"{name}: {err:.3e} (bound {tol:g})")
    assert err < tol, (name, err)


def _check_fp32(x, o, B, cov):
    """Every step against fp32 on the operands the kernel had for that step."""
    dl, lens = x["dlen"].long(), x["lens"].long()
    tile_last = dl.view(B // 16, 16).max(1).values.repeat_interleave(16)
    mask = torch.arange(T, device="cuda")[None, :] < lens[:, None]
    Wc, Ws, Fr = x["KcT"].float(), x["WsT"].float(), x["F"].float() / KF
    zero = torch.zeros((), device="cuda")
    for t in range(D):
        tl = (t < tile_last)[:, None]     # rows of tiles that still run
        rl = (t < dl)[:, None]            # live rows
        hp, cp = o["Hb"][t].float(), o["Cst"][t]
        z = x["XG"][t] + hp @ Wc[:, E:].t()
        if t > 0:
            z = z + o["GVb"][t - 1].float() @ Wc[:, :E].t()
        i, j = torch.sigmoid(z[:, :H]), torch.tanh(z[:, H:2 * H])
        f, og = torch.sigmoid(z[:, 2 * H:3 * H] + 1.0), torch.sigmoid(z[:, 3 * H:])
        c = f * cp + i * j
        h = og * torch.tanh(c)
        _close(f"Cst[{t + 1}]", o["Cst"][t + 1], torch.where(tl, c, zero), 2e-3)
        _close(f"Hb[{t + 1}]", o["Hb"][t + 1], torch.where(tl, h, zero), 1e-2)
        _close(f"ACT[{t}]", o["ACT"][t], torch.where(tl, torch.cat([i, j, f, og], 1), zero), 2e-3)
        assert torch.equal(o["Cb"][t + 1], o["Cst"][t + 1].bfloat16())
        s_ref = torch.cat([o["Cb"][t + 1].float(), o["Hb"][t + 1].float()], 1) @ Ws.t() + x["bs"]
        run = tl[:, 0]
        if bool(run.any()):
            serr, sbound = float((o["S"][t][run] - s_ref[run]).abs().max()), 1e-3 * float(s_ref[run].abs().max()) + 1e-4
            print(f"S[{t}]: abs {serr:.3e} (bound {sbound:.3e})")
            assert serr < sbound, (f"S[{t}]", serr, sbound)  # linear2's bound (test_linear2_matches_fp32)
        assert bool(torch.isnan(o["S"][t][~run]).all())  # a dead tile's s is never written (nor read)
        covt = o["COV"][t] if (cov and t > 0) else torch.zeros(B, T, device="cuda")
        s = torch.nan_to_num(o["S"][t])
        u = Fr + s[:, None, :] + (x["wc"][None, None, :] * covt[:, :, None] if cov else 0.0)
        e = torch.einsum("bta,a->bt", torch.tanh(u), x["v"])
        a = torch.where(rl, torch.softmax(e.masked_fill(~mask, float("-inf")), -1), zero)
        g = torch.einsum("bt,bte->be", a, x["G"].float())
        _close(f"ATT[{t}]", o["ATT"][t], a, 2e-3)
        _close(f"GV[{t}]", o["GV"][t], g, 2e-3)
        assert torch.equal(o["ATTb"][t], o["ATT"][t].bfloat16()) and torch.equal(o["GVb"][t], o["GV"][t].bfloat16())
        if cov:
            _close(f"COV[{t + 1}]", o["COV"][t + 1], covt + a, 2e-3)
            _close(f"covloss[{t}]", o["covloss"][t], torch.where(rl[:, 0], torch.minimum(a, covt).sum(1), zero), 2e-3)
    for n, full in o["_full"].items():
        assert bool((full[o[n].numel():].float() == SENT).all()), n


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [True, False])
@pytest.mark.parametrize("B", [16, 48, 144])
def test_dec_fwd_persistent_matches_chain_and_fp32(B, cov):
    k = _k()
    assert k.dec_persistent_ok(H, E, A, B, T)
    _need(k, B)
    x = _inputs(B, 100 + B)
    o, err = _run_persistent(k, x, B, cov)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    ref = _run_chain(k, x, B, cov)
    torch.cuda.synchronize()
    names = OUT if cov else [n for n in OUT if n not in ("COV", "covloss")]
    for n in names:
        assert _same(o[n], ref[n]), n
    _check_fp32(x, o, B, cov)


@pytest.mark.gpu
def test_dec_fwd_persistent_attention_bits():
    """Given the S the kernel wrote, its ATT, GV and COV are bit-equal to attn_fwd_rowp on that S."""
    k = _k()
    B = 48
    _need(k, B)
    x = _inputs(B, 7)
    o, err = _run_persistent(k, x, B, True)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for t in range(D):
        att, attb = torch.full((B, T), float("nan"), device="cuda"), torch.zeros(B, T, device="cuda").bfloat16()
        covn, cl = torch.full((B, T), float("nan"), device="cuda"), torch.zeros(B, device="cuda")
        gv, gvb = torch.full((B, E), float("nan"), device="cuda"), torch.zeros(B, E, device="cuda").bfloat16()
        k.attn_fwd_rowp(x["F"], x["G"], o["S"][t], x["v"], x["wc"], o["COV"][t] if t > 0 else None, x["lens"], att,
                        covn, cl, gv, gvb, B, T, A, x["dlen"], t, attb)
        torch.cuda.synchronize()
        assert torch.equal(att, o["ATT"][t]) and torch.equal(gv, o["GV"][t]) and torch.equal(covn, o["COV"][t + 1])
        assert torch.equal(cl, o["covloss"][t])


@pytest.mark.gpu
def test_dec_fwd_persistent_graph_replay():
    """Captured with the clear of its hand-off buffer, replayed twice with the inputs changed in
    between: both replays equal eager launches, and no hand-off timed out."""
    k = _k()
    B = 48
    _need(k, B)
    xs = [_inputs(B, 11), _inputs(B, 12, salt=3)]
    eager = [_run_persistent(k, x, B, True)[0] for x in xs]
    torch.cuda.synchronize()
    x = {n: v.clone() for n, v in xs[0].items()}
    o = _outputs(B, True)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    xbuf = torch.zeros(int(k.dec_persistent_xbuf(B)), dtype=torch.long, device="cuda")
    _run_persistent(k, x, B, True, o, err, xbuf)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run_persistent(k, x, B, True, o, err, xbuf)
    for i in range(2):
        for n in x:
            x[n].copy_(xs[i][n])
        for n in OUT:
            o[n].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for n in OUT:
            assert _same(o[n], eager[i][n]), (i, n)
    assert int(err.item()) == 0


@pytest.mark.gpu
def test_dec_persistent_grid_matches_engine_config():
    """The engine decides with engine_config.dec_persistent_grid and the binding checks the
    library's: the two must agree, or an eligible shape would raise instead of falling back."""
    from textsummarization_on_flink_amd.models.engine_config import dec_persistent_eligible, dec_persistent_grid
    k = _k()
    for B in (0, 8, 16, 24, 48, 128, 144, 250, 256, 272, 1024):
        assert int(k.dec_persistent_grid(B)) == dec_persistent_grid(B), B
    # the shape rule likewise (ample capacity on the Python side, so only the shape decides)
    for H, E, A in ((256, 128, 512), (512, 128, 1024), (256, 64, 512)):
        for B in (8, 16, 24, 32, 256, 272):
            for T in (0, 1, 2048, 2049):
                py = dec_persistent_eligible(H=H, E=E, A=A, B=B, T=T, proj_attn=True, row_attn=True, world=1,
                                             capacity=1 << 20, reserve_cus=0)
                assert bool(k.dec_persistent_ok(H, E, A, B, T)) == py, (H, E, A, B, T)


def test_dec_persistent_eligibility():
    """Pure function: the headline family with a co-resident grid only; everything else falls back
    (returns False) without raising."""
    from textsummarization_on_flink_amd.models.engine_config import (EngineConfig, dec_persistent_eligible,
                                                                     dec_persistent_grid)
    ok = dict(H=256, E=128, A=512, B=256, T=400, proj_attn=True, row_attn=True, world=1, capacity=256, reserve_cus=32)
    assert dec_persistent_eligible(**ok)
    assert EngineConfig().dec_persistent and not EngineConfig.from_env({"TSAMD_DEC_PERSISTENT": "0"}).dec_persistent
    assert dec_persistent_grid(16) == 128 and dec_persistent_grid(144) == 256 and dec_persistent_grid(256) == 256
    assert not dec_persistent_eligible(**{**ok, "H": 512, "A": 1024})      # config #5
    assert not dec_persistent_eligible(**{**ok, "B": 250})                  # not whole 16-row tiles
    assert not dec_persistent_eligible(**{**ok, "B": 8})
    assert not dec_persistent_eligible(**{**ok, "capacity": 255})           # grid larger than the capacity
    assert not dec_persistent_eligible(**{**ok, "capacity": 0})             # no device / kernel not admitted
    assert not dec_persistent_eligible(**{**ok, "B": 272})                  # 17 teams: 384 workgroups
    assert not dec_persistent_eligible(**{**ok, "world": 2})                # RCCL's CUs come off the capacity
    assert dec_persistent_eligible(**{**ok, "world": 2, "B": 128, "capacity": 256})
    assert not dec_persistent_eligible(**{**ok, "proj_attn": False})
    assert not dec_persistent_eligible(**{**ok, "row_attn": False})
    assert not dec_persistent_eligible(**{**ok, "T": 4096})
