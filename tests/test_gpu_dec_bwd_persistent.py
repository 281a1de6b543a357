"""dec_bwd_persistent (csrc/kernels/decoder_bwd_persistent.hip): the decoder backward loop as ONE
persistent launch with per-tile hand-offs, against the three-kernel chain it replaces
(attn_bwd_rowp -> dec_bwd_cell -> dec_bwd_dz per step, from t = D - 1 down).  The kernel keeps their
arithmetic and summation order, so DE, DS, DZ, DX and the final dh_rec / dc_carry must be bit-equal;
the per-step kernels themselves are checked against float64 in test_gpu_attn_ops.py and
test_gpu_decoder_ops.py.

Shapes (H = 256, E = 128, A = 512), the smallest at which each thing can go wrong:
* B = 16 (one team) and B = 32 (two teams);
* T = 24 with encoder lengths 1, 5, 22, T, ...: at most six waves have a position group, and
  positions past len but below 4 * ngrp and below T take the DE tails;
* T = 68 and T = 150 with D = 7: more than 16 groups, so every wave loops and the A / B buffers
  alternate, and more than six waves are active;
* D = 1 (no dx_{t+1}, no dcov_next), 2, 3 (first reuse of a hand-off slot) and 7;
* coverage on and off;
* dlen: a tile whose rows are all dead for the first steps of the reverse loop, a tile with one
  live row among dead ones, rows whose dlen equals t (dX_dir still added), a row that never runs.
Outputs are prefilled with NaN; the chain and the launch start from identical buffers, with
nonzero dh_rec / dc_carry start values."""
import pytest
import torch

H, E, A = 256, 128, 512
KF = 2.8853900817779268  # 2 log2(e): F is stored pre-scaled by it (attn_common.h)
OUT = ("DE", "DS", "DZ", "DX", "dh_rec", "dc_carry")


def _k():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _need(k, B):
    """The kernel's own launch rule (the engine falls back; a bare-kernel test cannot run)."""
    cap = int(k.dec_bwd_persistent_capacity())
    assert cap > 0, "the occupancy query does not admit dec_bwd_persistent"
    if int(k.dec_persistent_grid(B)) > cap:
        pytest.skip("the persistent decoder grid is not co-resident on this device")


def _dlen(B, D):
    """Live steps per row: in tile 0 row 0 alone is live for the first steps of the reverse loop (the
    others are shorter, one never runs); tile 1 (B = 32) is dead for the first steps of the reverse loop."""
    dl = torch.full((B,), D, dtype=torch.int32)
    dl[1:16] = torch.tensor([max(1, D // 3)] * 7 + [min(2, D)] * 6 + [max(1, D - 2), 0], dtype=torch.int32)
    if B >= 32:
        dl[16:32] = torch.tensor([max(1, D - 3), 1, max(1, D - 4), 2] * 4, dtype=torch.int32).clamp(max=D)
    return dl.cuda()


def _inputs(B, T, D, seed, dlen=False, salt=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def r(*shape, s=1.0):
        return torch.randn(*shape, generator=g, device="cuda") * s

    lens = torch.tensor([T, 1, 5, max(1, T - 2), min(T, 33), 7, max(1, T // 2 + 1), 2], dtype=torch.int32,
                        device="cuda").repeat(B // 8)
    pos = torch.arange(T, device="cuda")[None, None, :]
    att = torch.softmax(r(D, B, T).masked_fill(pos >= lens[None, :, None], float("-inf")), -1)
    act = torch.sigmoid(r(D, B, 4 * H))
    act[:, :, H:2 * H] = torch.tanh(r(D, B, H))
    x = {
        "G": r(B, T, E, s=0.5).bfloat16(), "F": (r(B, T, A, s=0.5) * KF).bfloat16(), "S": r(D, B, A, s=0.5),
        "v": r(A, s=0.1), "wc": r(A, s=0.5), "COV": att.cumsum(0).roll(1, 0).contiguous(), "ATT": att.contiguous(),
        "GV": r(D, B, E, s=0.3), "Ga": r(D, B, T, s=0.2), "gcl": r(D, B, s=0.1).abs(), "lens": lens,
        "Ws": r(2 * H, A, s=0.05).bfloat16(), "dC_dir": r(D, B, H, s=0.1), "dH_dir": r(D, B, H, s=0.1),
        "ACT": act.contiguous(), "Cst": r(D + 1, B, H, s=0.7), "Kc": r(E + H, 4 * H, s=0.05).bfloat16(),
        "dX_dir": r(D, B, E, s=0.1), "dh0": r(B, H, s=0.1), "dc0": r(B, H, s=0.1),
        "dlen": _dlen(B, D) if dlen else None,
    }
    x["COV"] = torch.cat([x["COV"], x["COV"][:1]], 0).contiguous()  # [D + 1, B, T]; step t reads COV[t], t > 0
    if salt:
        x["Ga"] += 0.01 * salt
        x["dH_dir"] += 0.01 * salt
    return x


def _outputs(B, T, D, x):
    o = {"DE": torch.empty(D, B, T, device="cuda"), "DS": torch.empty(D, B, A, device="cuda"),
         "DZ": torch.empty(D, B, 4 * H, device="cuda", dtype=torch.bfloat16), "DX": torch.empty(D, B, E, device="cuda")}
    for t in o.values():
        t.fill_(float("nan"))
    o["dh_rec"], o["dc_carry"] = x["dh0"].clone(), x["dc0"].clone()
    return o


def _run_chain(k, x, B, T, D, cov):
    o = _outputs(B, T, D, x)
    dcov = torch.full((2, B, T), float("nan"), device="cuda")
    dl = x["dlen"]
    for t in reversed(range(D)):
        nxt = t < D - 1
        k.attn_bwd_rowp(x["G"], x["F"], x["S"][t], x["v"], x["wc"] if cov else None,
                        x["COV"][t] if (cov and t > 0) else None, x["ATT"][t], o["DX"][t + 1] if nxt else None,
                        x["GV"][t], x["Ga"][t], dcov[(t + 1) % 2] if (cov and nxt) else None,
                        x["gcl"][t] if cov else None, x["lens"], o["DE"][t], o["DS"][t], dcov[t % 2] if cov else None,
                        B, T, A, dl, t)
        k.dec_bwd_cell(o["DS"][t], x["Ws"], x["dC_dir"][t], x["dH_dir"][t], o["dh_rec"], o["dc_carry"], x["ACT"][t],
                       x["Cst"][t + 1], x["Cst"][t], o["DZ"][t], B, H, A, dl, t)
        k.dec_bwd_dz(o["DZ"][t], x["Kc"], x["dX_dir"][t], None, o["DX"][t], None, o["dh_rec"], B, E, H, 0, dl, t)
    return o


def _run_persistent(k, x, B, T, D, cov, o=None, err=None, xbuf=None):
    o = o or _outputs(B, T, D, x)
    err = torch.zeros(1, dtype=torch.int32, device="cuda") if err is None else err
    xbuf = torch.zeros(int(k.dec_bwd_persistent_xbuf(B)), dtype=torch.long, device="cuda") if xbuf is None else xbuf
    xbuf.zero_()
    k.dec_bwd_persistent(x["G"], x["F"], x["S"], x["v"], x["wc"] if cov else None, x["COV"] if cov else None, x["ATT"],
                         x["GV"], x["Ga"], x["gcl"] if cov else None, x["lens"], o["DE"], o["DS"], x["Ws"], x["dC_dir"],
                         x["dH_dir"], o["dh_rec"], o["dc_carry"], x["ACT"], x["Cst"], o["DZ"], x["Kc"], x["dX_dir"],
                         o["DX"], x["dlen"], xbuf, err, B, T, D, H, E, A)
    return o, err


def _same(a, b):
    """Bit equality (NaN counts as a value: nothing may stay unwritten on one side only)."""
    if a.dtype == torch.bfloat16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(k, B, T, D, cov, dlen, seed):
    _need(k, B)
    x = _inputs(B, T, D, seed, dlen)
    ref = _run_chain(k, x, B, T, D, cov)
    got, err = _run_persistent(k, x, B, T, D, cov)
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    for n in OUT:
        assert not bool(torch.isnan(ref[n].float()).any()), n
        diff = int((ref[n].float() != got[n].float()).sum())
        print(f"B={B} T={T} D={D} cov={cov} dlen={dlen} {n}: {diff} of {ref[n].numel()} differ")
        assert _same(got[n], ref[n]), (n, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [True, False])
@pytest.mark.parametrize("D", [1, 2, 3, 7])
def test_dec_bwd_persistent_matches_chain(D, cov):
    _check(_k(), 16, 24, D, cov, False, 100 + D)


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [True, False])
def test_dec_bwd_persistent_two_teams_match_chain(cov):
    _check(_k(), 32, 24, 7, cov, False, 150)


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [True, False])
@pytest.mark.parametrize("B,D", [(16, 7), (32, 7), (32, 3)])
def test_dec_bwd_persistent_dead_steps_match_chain(B, D, cov):
    _check(_k(), B, 24, D, cov, True, 200 + B + D)


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [True, False])
@pytest.mark.parametrize("B,T,dlen", [(16, 68, False), (32, 68, True), (16, 150, False), (32, 150, True)])
def test_dec_bwd_persistent_long_rows_match_chain(B, T, dlen, cov):
    _check(_k(), B, T, 7, cov, dlen, 300 + T)


@pytest.mark.gpu
def test_dec_bwd_persistent_graph_replay():
    """Captured with the clear of its hand-off buffer, replayed twice with the inputs changed in
    between: both replays equal eager launches (granule zeroing, parity slots), no hand-off timed out."""
    k = _k()
    B, T, D = 32, 24, 5
    _need(k, B)
    xs = [_inputs(B, T, D, 21, True), _inputs(B, T, D, 22, True, salt=3)]
    eager = [_run_persistent(k, x, B, T, D, True)[0] for x in xs]
    torch.cuda.synchronize()
    x = {n: (v.clone() if v is not None else None) for n, v in xs[0].items()}
    o = _outputs(B, T, D, x)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    xbuf = torch.zeros(int(k.dec_bwd_persistent_xbuf(B)), dtype=torch.long, device="cuda")
    _run_persistent(k, x, B, T, D, True, o, err, xbuf)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run_persistent(k, x, B, T, D, True, o, err, xbuf)
    for i in range(2):
        for n in x:
            if x[n] is not None:
                x[n].copy_(xs[i][n])
        for n in ("DE", "DS", "DZ", "DX"):
            o[n].fill_(float("nan"))
        o["dh_rec"].copy_(xs[i]["dh0"])
        o["dc_carry"].copy_(xs[i]["dc0"])
        graph.replay()
        torch.cuda.synchronize()
        for n in OUT:
            assert _same(o[n], eager[i][n]), (i, n)
    assert int(err.item()) == 0


def test_dec_bwd_persistent_eligibility():
    """Pure function of the shape, the attention path, the world size, the side streams and the
    device's resident capacity (needs no GPU)."""
    from textsummarization_on_flink_amd.models.engine_config import EngineConfig, dec_bwd_persistent_eligible
    ok = dict(H=256, E=128, A=512, B=256, T=400, proj_attn=True, row_attn=True, world=1, capacity=256, reserve_cus=32)
    assert dec_bwd_persistent_eligible(**ok)
    assert EngineConfig().dec_bwd_persistent
    assert not EngineConfig.from_env({"TSAMD_DEC_BWD_PERSISTENT": "0"}).dec_bwd_persistent
    assert EngineConfig.from_env({"TSAMD_DEC_PERSISTENT": "0"}).dec_bwd_persistent
    assert not dec_bwd_persistent_eligible(**{**ok, "H": 512, "A": 1024})     # config #5
    assert not dec_bwd_persistent_eligible(**{**ok, "E": 64})
    assert not dec_bwd_persistent_eligible(**{**ok, "A": 1024})
    assert not dec_bwd_persistent_eligible(**{**ok, "B": 250})                 # not whole 16-row tiles
    assert not dec_bwd_persistent_eligible(**{**ok, "B": 8})
    assert not dec_bwd_persistent_eligible(**{**ok, "capacity": 255})          # grid larger than the capacity
    assert not dec_bwd_persistent_eligible(**{**ok, "capacity": 0})            # no device / kernel not admitted
    assert not dec_bwd_persistent_eligible(**{**ok, "dw_side": True})          # the vocab dW beside the loop
    assert not dec_bwd_persistent_eligible(**{**ok, "world": 2})               # RCCL's CUs come off the capacity
    assert dec_bwd_persistent_eligible(**{**ok, "world": 2, "B": 128, "capacity": 256})
    assert not dec_bwd_persistent_eligible(**{**ok, "world": 2, "B": 128, "capacity": 256, "dw_side": True})
    assert not dec_bwd_persistent_eligible(**{**ok, "proj_attn": False})
    assert not dec_bwd_persistent_eligible(**{**ok, "row_attn": False})
    assert not dec_bwd_persistent_eligible(**{**ok, "T": 4096})


@pytest.mark.gpu
def test_train_step_same_gradients_with_and_without(monkeypatch):
    """One train_step at B = 32, T = 24, D = 5 from the same seeded weights with the switch on and off.
    The library GEMMs and fp32 atomics elsewhere in the step are not bit-reproducible, so the gradient
    buffers are held to the bound test_gpu_model.py uses for two runs of one build (3e-5)."""
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.models.params import build_params
    from textsummarization_on_flink_amd.models.pointer_generator import HipPointerGenerator
    B, T, D, V = 32, 24, 5, 2000
    hps = HParams(batch_size=B, max_enc_steps=T, max_dec_steps=D, vocab_size=V, emb_dim=E, hidden_dim=H,
                  coverage=True, pointer_gen=True, trunc_norm_init_std=0.05)
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=4 * V, seed=0, art_mean=T * 0.9, art_sd=T * 0.4, sent_mean=4)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=T)[0]
    monkeypatch.setenv("TSAMD_ROW_ATTN", "1")
    got = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("TSAMD_DEC_BWD_PERSISTENT", flag)
        params = build_params(hps, vocab.size(), device="cuda", seed=0).enable_grad().enable_adagrad(
            hps.adagrad_init_acc)
        eng = HipPointerGenerator(hps, vocab.size(), params, B=B, T=T)
        if flag == "1" and int(eng.k.dec_persistent_grid(B)) > int(eng.k.dec_bwd_persistent_capacity()):
            pytest.skip("the persistent decoder grid is not co-resident on this device")
        assert eng.proj_attn and eng.dec_bwd_persistent_on() == (flag == "1")
        eng.set_batch(batch)
        out = eng.train_step()
        torch.cuda.synchronize()
        eng.check_lstm_err()
        got[flag] = (float(out["total_loss"]), params.grad.clone())
    (l0, g0), (l1, g1) = got["0"], got["1"]
    rel = float((g1 - g0).norm() / (g0.norm() + 1e-12))
    print(f"loss {l0} / {l1}, gradient distance {rel:.3e} (bound 3e-5)")
    assert float(g0.norm()) > 0
    assert abs(l1 - l0) <= 1e-6 * abs(l0)  # (the forward is the same code both times)
    assert rel < 3e-5, rel
