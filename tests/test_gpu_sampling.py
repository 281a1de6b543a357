"""Decode by sampling on the device: the Philox probe against the host bit for bit, ``sample_topk``
and ``sample_full`` against float64 CDFs (a sandwich: the picked entry's CDF interval, widened by the
fp32 error bound, holds the target), and ``DeviceSampler`` whole: greedy == beam 1, a per-step audit
of every drawn token, graph == eager, batching independence, untouched defaults.

Op inputs are ``_topk_inputs`` of test_gpu_wide_beam (T = 96, lengths 20..96, duplicated and
out-of-vocabulary ext ids, logits randn * 3), 2 samples per article; the decoder tests use the small
model of that file's end-to-end tests."""
import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.decode.sampling import sample_uniform

pytestmark = pytest.mark.gpu

DEV = "cuda"
STOP, MIN_DEC, MAX_DEC, T = 3, 3, 100, 96
ULP = 2.0 ** -24


def _i64(seed):
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def _step(t):
    return torch.tensor([t + 1], dtype=torch.int32, device=DEV)  # beam_gather advanced it: the kernels take t = step - 1


def _outs(R):
    return (torch.full((R,), -7, dtype=torch.int32, device=DEV), torch.full((R,), float("nan"), device=DEV),
            torch.full((R,), -7, dtype=torch.int32, device=DEV))


NOBOOK = (None,) * 10


# ------------------------------------------------------------------ 1. random numbers
@pytest.mark.parametrize("seed", [0, 0x1234567890abcdef, (1 << 63) + 5])
def test_sample_uniforms_equal_host_bit_for_bit(seed):
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    streams = [0, 1, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40 + 3, 2 ** 62 + 1]
    sd = torch.tensor(streams, dtype=torch.long, device=DEV)
    for t in (0, 1, 99):
        out = torch.zeros(len(streams), device=DEV)
        k.sample_uniforms(_i64(seed), sd, torch.tensor([t], dtype=torch.int32, device=DEV), out)
        want = np.array([sample_uniform(seed, s, t) for s in streams], np.float32)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
        assert len(set(want.tolist())) == len(streams)


# ------------------------------------------------------------------ 2. the two sandwiches
def _sandwich(cdf_lo, cdf_hi, W, u, eps):
    """(passes, inside a widened edge): [cdf_lo, cdf_hi] widened by eps * W holds u * W."""
    x = u * W
    ok = cdf_lo - eps * W <= x <= cdf_hi + eps * W
    return ok, ok and not (cdf_lo <= x < cdf_hi)


def _check_topk_row(ids, lps, k, temp, allow, u, pick, tok, lp, eps):
    cand = [j for j in range(k + 1) if allow or int(ids[j]) != STOP][:k]
    assert pick in cand, (pick, cand)
    w = np.exp(np.asarray(lps, np.float64)[cand] / temp)
    c = np.cumsum(w)
    j = cand.index(pick)
    ok, edge = _sandwich(c[j] - w[j], c[j], c[-1], u, eps)
    assert ok, (pick, u, (c / c[-1]).tolist())
    assert tok == int(ids[pick]) and np.float32(lp).view(np.int32) == np.float32(lps[pick]).view(np.int32)
    return edge


def _topk_lists(k, K, seed):
    """final_topk's lists for 3 articles x 2 samples at V = 3000, [STOP] planted at rank r % K of row r."""
    from test_gpu_wide_beam import _topk_inputs, _topk_run
    Na, n, V = 3, 2, 3000
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, n, V, T, seed)
    ids, lp = _topk_run(k, k.final_topk, logits, bias, pg, attn, ext, lens, Na * n, V, T, K, n)
    ids[ids == STOP] = V + 50
    for r in range(Na * n):
        ids[r, r % K] = STOP
    return ids.contiguous(), lp.contiguous()


@pytest.mark.parametrize("temp", [1.0, 0.7])
@pytest.mark.parametrize("K", [2, 9, 32])
def test_sample_topk_sandwich(K, temp):
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    kk, R, seed = K - 1, 6, 0xfeedbeef12345
    ids, lp = _topk_lists(k, K, seed=K)
    hi, hl = ids.cpu().numpy(), lp.cpu().numpy()
    eps = (K + 8) * ULP
    edges = 0
    for t in (MIN_DEC - 1, MIN_DEC):
        for base in (0, 2 ** 32 - 3, 1000):  # several draws per row
            streams = torch.arange(base, base + R, dtype=torch.long, device=DEV)
            tok, olp, pick = _outs(R)
            k.sample_topk(ids, lp, streams, _step(t), _i64(seed), tok, olp, pick, R, K, kk, temp, STOP, MIN_DEC,
                          MAX_DEC, T, *NOBOOK)
            tok, olp, pick = tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()
            for r in range(R):
                u = sample_uniform(seed, base + r, t)
                edges += _check_topk_row(hi[r], hl[r], kk, temp, t >= MIN_DEC, u, int(pick[r]), int(tok[r]),
                                         olp[r], eps)
                if t < MIN_DEC:
                    assert tok[r] != STOP
    print(f"sample_topk K={K} temp={temp}: {edges} rows inside a widened edge")


def _full_ref(logits, bias, pg, attn, ext, lens, r, n, t, pointer):
    """float64 weights, tokens and the model's probabilities of row r."""
    x = logits[r].double() + bias.double()
    sm = torch.softmax(x, 0).cpu().numpy()
    V = len(sm)
    if not pointer:
        w, toks, fd = sm.copy(), np.arange(V), sm
    else:
        L = int(lens[r // n])
        p, a = float(pg[r].double()), attn[r, :L].double().cpu().numpy()
        e = ext[r // n, :L].cpu().numpy().astype(np.int64)
        w, toks = np.concatenate([p * sm, (1 - p) * a]), np.concatenate([np.arange(V), e])
        fd = np.concatenate([p * sm, np.zeros(64)])
        np.add.at(fd, e, (1 - p) * a)
    if t < MIN_DEC:
        w[toks == STOP] = 0.0
    return w, toks, fd, float((x.max() - x.min()).item())


def _check_full_row(ref, V, L, t, u, pick, tok, lp, eps):
    w, toks, fd, _ = ref
    assert 0 <= pick < len(w), pick  # a position entry V + i has i < enc_len
    assert pick < V + L
    assert w[pick] > 0 and tok == toks[pick]
    assert t >= MIN_DEC or tok != STOP
    c = np.cumsum(w)
    ok, edge = _sandwich(c[pick] - w[pick], c[pick], c[-1], u, eps)
    assert ok, (pick, u, c[pick] / c[-1], w[pick] / c[-1])
    np.testing.assert_allclose(lp, np.log(fd[tok]), rtol=1e-4, atol=1e-5)
    return edge


def _find_stream(seed, t, lo, hi):
    return next(s for s in range(100000) if lo <= sample_uniform(seed, s, t) < hi)


@pytest.mark.parametrize("pointer", [True, False])
@pytest.mark.parametrize("V", [3000, 20000])
def test_sample_full_sandwich(V, pointer):
    """3 articles x 2 samples plus two more articles for the special rows: row 6 all-equal logits with
    the target in the last vocabulary chunk, row 7 p_gen = 0, row 8 p_gen = 1."""
    from test_gpu_wide_beam import _topk_inputs
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, n, seed = 5, 2, 0xabcdef0123
    R = Na * n
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, n, V, T, seed=V + pointer)
    ext[:, 5] = STOP
    ext[:, 15] = STOP  # [STOP] copied twice (all lengths are >= 20) ...
    logits[:, STOP] += 6.0  # ... and likely in the vocabulary part
    logits[6] = 0.5 - bias
    pg[6], pg[7], pg[8] = 0.75, 0.0, 1.0
    ncv = (V + 255) // 256
    edges, copies = 0, 0
    for t in (MIN_DEC - 1, MIN_DEC):
        refs = [_full_ref(logits, bias, pg, attn, ext, lens, r, n, t, pointer) for r in range(R)]
        rng = max(x[3] for x in refs)
        # (V = 20000: the formula gives 1.2e-3, past the 1e-3 the window may have at most: the smaller of the two)
        eps = min((V + T + 1.5 * rng + 8) * ULP, 0.999e-3)
        assert rng < 40 and eps < 1e-3
        for base in (0, 2 ** 32 - 3):
            st = list(range(base, base + R))
            w6 = refs[6][0]
            frac = w6[:(ncv - 1) * 256].sum() / w6.sum(), w6[:V].sum() / w6.sum()
            st[6] = _find_stream(seed, t, frac[0] + 1e-4, frac[1] - 1e-4)
            tok, olp, pick = _outs(R)
            k.sample_full(logits, bias, pg if pointer else None, attn if pointer else None, ext, lens,
                          torch.tensor(st, dtype=torch.long, device=DEV), _step(t), _i64(seed), tok, olp, pick, R, V, T,
                          n, STOP, MIN_DEC, MAX_DEC, *NOBOOK, None)
            tok, olp, pick = tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()
            for r in range(R):
                u = sample_uniform(seed, st[r], t)
                L = int(lens[r // n]) if pointer else 0
                edges += _check_full_row(refs[r], V, L, t, u, int(pick[r]), int(tok[r]), float(olp[r]), eps)
                copies += pick[r] >= V
            assert (ncv - 1) * 256 <= pick[6] < V
            if pointer:
                assert pick[7] >= V and pick[8] < V
    assert not pointer or copies > 2
    print(f"sample_full V={V} pointer={pointer}: {edges} rows inside a widened edge, {copies} position entries")


@pytest.mark.parametrize("V", [3000, 70000])
def test_sample_full_long_articles_and_many_chunks(V):
    """T = 400 with lengths past 256 (two position chunks) and, at V = 70000, more than 256 chunks (every
    thread of the scan then owns two): 3 articles x 2 samples, 12 draws per row and step, half the rows
    with a small p_gen so that the later position chunk is drawn from."""
    from test_gpu_wide_beam import _topk_inputs
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, n, Tl, seed = 3, 2, 400, 0x5eed5eed5eed
    R = Na * n
    logits, bias, pg, _, ext, _ = _topk_inputs(Na, n, V, Tl, seed=V)
    lens = torch.tensor([400, 300, 257], dtype=torch.int32, device=DEV)
    g = torch.Generator(device="cpu").manual_seed(V + 1)
    attn = torch.rand(R, Tl, generator=g).to(DEV)
    attn = attn * (torch.arange(Tl, device=DEV)[None] < lens.repeat_interleave(n)[:, None]).float()
    attn = attn / attn.sum(1, keepdim=True)
    pg[::2] = 0.15
    ext[:, 280] = STOP
    assert (V + 255) // 256 + 2 > 256 or V == 3000
    edges, late = 0, 0
    for t in (MIN_DEC - 1, MIN_DEC):
        refs = [_full_ref(logits, bias, pg, attn, ext, lens, r, n, t, True) for r in range(R)]
        eps = min((V + Tl + 1.5 * max(x[3] for x in refs) + 8) * ULP, 0.999e-3)  # (capped: the window stays < 1e-3)
        assert eps < 1e-3
        for base in range(0, 12 * R, R):
            tok, olp, pick = _outs(R)
            k.sample_full(logits, bias, pg, attn, ext, lens, torch.arange(base, base + R, dtype=torch.long, device=DEV),
                          _step(t), _i64(seed), tok, olp, pick, R, V, Tl, n, STOP, MIN_DEC, MAX_DEC, *NOBOOK, None)
            tok, olp, pick = tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()
            for r in range(R):
                u = sample_uniform(seed, base + r, t)
                edges += _check_full_row(refs[r], V, int(lens[r // n]), t, u, int(pick[r]), int(tok[r]),
                                         float(olp[r]), eps)
                late += pick[r] >= V + 256
    assert late >= 5, late  # the second position chunk was drawn from
    print(f"sample_full V={V} T={Tl}: {edges} rows inside a widened edge, {late} entries in the second position chunk")


def test_sample_full_reports_a_row_with_nothing_to_draw():
    """p_gen = 1 and every logit but [STOP]'s at -inf, before min_dec: every weight is 0.  The host rule
    raises; the kernel sets its error word, ends the row with [STOP] and reports entry -1.  The other rows
    draw as usual, and without such a row the word stays 0."""
    from test_gpu_wide_beam import _topk_inputs
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, n, V = 2, 2, 3000
    R = Na * n
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, n, V, T, seed=3)
    st = torch.arange(R, dtype=torch.long, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tok, olp, pick = _outs(R)
    args = (ext, lens, st, _step(0), 0, tok, olp, pick, R, V, T, n, STOP, MIN_DEC, MAX_DEC, *NOBOOK, err)
    k.sample_full(logits, bias, pg, attn, *args)
    assert int(err) == 0 and (pick >= 0).all()
    logits[2] = float("-inf")
    logits[2, STOP] = 1.0
    pg[2] = 1.0
    k.sample_full(logits, bias, pg, attn, *args)
    assert int(err) == 1 and int(pick[2]) == -1 and int(tok[2]) == STOP
    assert (pick[[0, 1, 3]] >= 0).all() and (tok[[0, 1, 3]] != STOP).all()
    err.zero_()
    k.sample_full(logits, bias, pg, attn, ext, lens, st, _step(MIN_DEC), 0, tok, olp, pick, R, V, T, n, STOP, MIN_DEC,
                  MAX_DEC, *NOBOOK, err)
    assert int(err) == 0 and int(pick[2]) == STOP == int(tok[2])  # at min_dec the [STOP] may be drawn


def test_sample_ops_refuse_bad_arguments():
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    R, K = 2, 4
    ids, lp = torch.zeros(R, K, dtype=torch.int32, device=DEV), torch.zeros(R, K, device=DEV)
    st = torch.zeros(R, dtype=torch.long, device=DEV)
    for kk, temp in ((4, 1.0), (0, 1.0), (2, 0.0)):
        with pytest.raises(RuntimeError, match="sample_topk"):
            k.sample_topk(ids, lp, st, _step(0), 0, *_outs(R), R, K, kk, temp, STOP, MIN_DEC, MAX_DEC, T, *NOBOOK)
    with pytest.raises(RuntimeError, match="together"):
        k.sample_topk(ids, lp, st, _step(0), 0, *_outs(R), R, K, 2, 1.0, STOP, MIN_DEC, MAX_DEC, T, None,
                      torch.zeros(MAX_DEC, R, dtype=torch.int32, device=DEV), *(None,) * 8)


# ------------------------------------------------------------------ 3. the decoder
def _setup(V=600, **kw):
    from test_gpu_decode import _peaked_setup
    hps, vocab, batch, params = _peaked_setup(True, V=V)
    return hps.replace(**kw), vocab, batch, params


def _sampler(hps, vocab, params, **kw):
    from textsummarization_on_flink_amd.decode.device_beam import DeviceSampler
    return DeviceSampler(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, **kw)


def _toks(samples):
    return [[h.tokens for h in hyps] for hyps in samples]


def test_greedy_sampler_equals_beam_one():
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(beam_size=1)
    d0 = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=False)
    d0.fused_step = False
    h0 = d0.decode(batch)
    d1 = _sampler(hps.replace(sampling_topk=1, n_samples=1), vocab, params, use_graph=False)
    assert d1.K == 2 == d0.K and d1.R == d0.R and not d1.fused_step and d1.fused_vocab == d0.fused_vocab
    h1 = d1.decode(batch)
    assert len(h1) == hps.batch_size and [h.tokens for h in h1] == [h.tokens for h in h0]
    np.testing.assert_allclose([sum(h.log_probs) for h in h1], [sum(h.log_probs) for h in h0], rtol=1e-4, atol=1e-5)
    for h in h1:
        assert len(h.log_probs) == len(h.tokens) == len(h.attn_dists) + 1 and h.score == h.avg_log_prob
    assert _toks(d1.sample(batch, 0)) == [[h.tokens] for h in h1]


@pytest.mark.parametrize("topk", [3, 0])
def test_sampler_per_step_audit(topk):
    """12 steps driven by hand (no graph): every recorded token passes the sandwich for its step's
    uniform over the inputs its draw kernel read, lp_hist holds the recorded log-probs, done rows
    stop changing."""
    n, seed, base = 2, 99, 7
    from textsummarization_on_flink_amd.models.pointer_generator import OV
    hps, vocab, batch, params = _setup(V=512, sampling_topk=topk, n_samples=n, sample_seed=seed, min_dec_steps=MIN_DEC)
    params[OV][STOP] += 6.0  # a [STOP] likely enough that some samples end inside the 12 steps
    d = _sampler(hps, vocab, params, use_graph=False)
    assert vocab.word2id("[STOP]") == STOP and not d.fused_step and (topk > 0 or not d.fused_vocab)
    R, V, K, Tm = d.R, d.V, d.K, d.T
    d._encode(batch)
    d.set_streams(base)
    d._prologue()
    b = d.b
    lens, ext = b["lens"].cpu(), b["ext"].clone()
    rec, edges, ndone = [], 0, 0
    for t in range(12):
        before = {x: b[x].clone() for x in ("done", "slen", "latest", "lp_sum")}
        d._step(t % 2)
        Y = d.st[1 - t % 2]
        snap = {x: b[x].clone() for x in ("s_tok", "s_lp", "s_pick", "done", "slen", "latest", "lp_sum", "top_ids",
                                          "top_lp", "logits", "PG")}
        snap["att"] = Y["ATT"].clone()
        rec.append((before, snap))
    assert int(b["step"].item()) == 12
    tok_hist, lp_hist = b["tok_hist"].cpu().numpy(), b["lp_hist"].cpu().numpy()
    att_hist = b["ATT_hist"].cpu().numpy()
    bias = d.p[OV]
    for t, (before, s) in enumerate(rec):
        was_done = before["done"].cpu().numpy()
        tok, slp, pick = s["s_tok"].cpu().numpy(), s["s_lp"].cpu().numpy(), s["s_pick"].cpu().numpy()
        if topk == 0:
            rng = float((s["logits"] + bias).max(1).values.sub((s["logits"] + bias).min(1).values).max())
            eps = (V + Tm + 1.5 * rng + 8) * ULP
            assert eps < 1e-3
        for r in range(R):
            if was_done[r]:
                ndone += 1
                assert tok_hist[t, r] == 0 and lp_hist[t, r] == 0
                for x in ("slen", "latest", "lp_sum", "done"):
                    assert s[x][r] == before[x][r]
                continue
            u = sample_uniform(seed, base + r, t)
            if topk > 0:
                edges += _check_topk_row(s["top_ids"][r].cpu().numpy(), s["top_lp"][r].cpu().numpy(), topk,
                                         hps.sampling_temp, t >= MIN_DEC, u, int(pick[r]), int(tok[r]), slp[r],
                                         (K + 8) * ULP)
            else:
                ref = _full_ref(s["logits"], bias, s["PG"], s["att"], ext, lens, r, n, t, True)
                edges += _check_full_row(ref, V, int(lens[r // n]), t, u, int(pick[r]), int(tok[r]), float(slp[r]),
                                         eps)
            assert tok_hist[t, r] == tok[r] and lp_hist[t, r] == slp[r]
            assert int(s["slen"][r]) == t + 1 and int(s["latest"][r]) == tok[r]
            assert int(s["done"][r]) == (tok[r] == STOP)
            np.testing.assert_array_equal(att_hist[t, r], s["att"][r].cpu().numpy())
    np.testing.assert_allclose(b["lp_sum"].cpu().numpy(), lp_hist.sum(0), rtol=1e-5, atol=1e-6)
    print(f"audit topk={topk}: {edges} draws inside a widened edge, {ndone} done row-steps")
    assert 0 < ndone < 11 * R  # both kinds of row were seen


def _reversed_batch(hps, vocab, batch):
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    exs = [Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, hps)
           for a in range(hps.batch_size)]
    return (Batch(exs, hps, vocab, pad_enc_to=hps.max_enc_steps),
            Batch(exs[::-1], hps, vocab, pad_enc_to=hps.max_enc_steps))


@pytest.mark.parametrize("topk", [4, 8, 0])  # (8: nine candidates, the select's 32-entry lists)
def test_sampler_graph_and_batching(topk):
    n = 4
    # (top-4 of this peaked model at temperature 1.5, so that every article's four samples differ)
    hps, vocab, batch, params = _setup(sampling_topk=topk, n_samples=n, sample_seed=5,
                                       sampling_temp=1.5 if topk else 1.0)
    Na = hps.batch_size
    fwd, rev = _reversed_batch(hps, vocab, batch)
    dg = _sampler(hps, vocab, params, use_graph=True)
    de = _sampler(hps, vocab, params, use_graph=False)
    assert dg.K == (topk + 1 if topk else 2) and dg.fused_vocab == (topk > 0) and not dg.fused_step
    sg = dg.sample(fwd, 0)
    assert len(sg) == Na and all(len(x) == n for x in sg)
    assert _toks(sg) == _toks(de.sample(fwd, 0))          # graph == eager
    assert _toks(dg.sample(fwd, 0)) == _toks(sg)          # the same batch again: the same samples
    # reversed articles, every article with its own streams
    sr = dg.sample(rev, [(Na - 1 - a) * n for a in range(Na)])
    assert _toks(sr)[::-1] == _toks(sg)
    assert all(len({tuple(h.tokens) for h in hyps}) > 1 for hyps in sg)  # no article's four samples are all equal
    d2 = _sampler(hps.replace(sample_seed=6), vocab, params, use_graph=True)
    assert _toks(d2.sample(fwd, 0)) != _toks(sg)          # another seed: other samples
    for hyps in sg:
        for h in hyps:
            body = h.tokens[1:]
            assert STOP not in body[:hps.min_dec_steps] and STOP not in body[:-1]
            assert len(body) == hps.max_dec_steps or body[-1] == STOP
            assert np.isfinite(h.log_probs).all() and max(h.log_probs) <= 1e-5
    # decode / decode_batches: best_sample per article, streams counted over the articles decoded so far
    from textsummarization_on_flink_amd.decode.sampling import best_sample
    want = [[best_sample(x).tokens for x in sg], [best_sample(x).tokens for x in dg.sample(fwd, Na * n)]]
    dg.articles_seen = 0
    assert [[h.tokens for h in hy] for hy in dg.decode_batches([fwd, fwd])] == want
    dg.articles_seen = 0
    assert [[h.tokens for h in dg.decode(fwd)] for _ in range(2)] == want


def test_default_flags_build_the_beam_decoder_unchanged():
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder, DeviceSampler, device_decoder
    hps, vocab, batch, params = _setup()
    assert hps.sampling_topk == -1
    Na, Tm = hps.batch_size, hps.max_enc_steps
    d = device_decoder(hps, vocab, params, n_articles=Na, T=Tm, use_graph=False)
    assert type(d) is DeviceBeamDecoder
    assert (d.beam, d.K, d.R, d.rep, d.wide, d.ngram, d.pen) == (4, 8, 4 * Na, 4, False, 0, None)
    assert d.fused_vocab and d.fused_step == d.row_attn
    assert not {"streams", "lp_hist", "slen", "s_tok", "s_lp", "s_pick"} & set(d.b)
    assert d.b["done"].shape == (Na,) and d.b["top_ids"].shape == (4 * Na, 8)
    assert type(d)._book is DeviceBeamDecoder._book and type(d)._select is DeviceBeamDecoder._select
    s = device_decoder(hps.replace(sampling_topk=8, n_samples=2), vocab, params, n_articles=Na, T=Tm, use_graph=False)
    assert type(s) is DeviceSampler and (s.beam, s.K, s.R, s.fused_step) == (2, 9, 2 * Na, False)
    assert s.b["done"].shape == (2 * Na,) and s.b["streams"].dtype == torch.long
    with pytest.raises(ValueError, match="sampling_topk >= 0"):
        DeviceSampler(hps, vocab, params, n_articles=Na, T=Tm)
