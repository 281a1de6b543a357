"""Beam sizes 6 to 16 on the device: ``final_topk`` with the 32-entry candidate list (K up to 32,
tie-heavy fallback included), the workgroup-wide bookkeeping ``beam_step_wide`` against a Python
mirror of the reference loop (plain, n-gram blocking, penalties), and whole decodes: the wide
path == the one-wave path at beams 2 / 4 / 5, beams 8 and 10 end to end."""
import functools

import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.config import HParams
from textsummarization_on_flink_amd.decode.beam_search import inv_len_table, ngram_blocked

pytestmark = pytest.mark.gpu

DEV = "cuda"
BLOCKED = np.float32(-1e20)
f32 = np.float32


# ------------------------------------------------------------------ 1. final_topk, K = 20 and 32
def _topk_inputs(Na, beam, V, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = Na * beam
    logits = (torch.randn(R, V, generator=g) * 3).to(DEV)
    bias = torch.randn(V, generator=g).to(DEV)
    pg = torch.rand(R, generator=g).to(DEV)
    lens = torch.randint(20, T + 1, (Na,), generator=g, dtype=torch.int32).to(DEV)
    ext = torch.randint(0, V + 20, (Na, T), generator=g, dtype=torch.int32).to(DEV)
    ext[:, :10] = ext[:, 10:20]  # duplicates
    attn = torch.rand(R, T, generator=g).to(DEV)
    attn = attn * (torch.arange(T, device=DEV)[None] < lens.repeat_interleave(beam)[:, None]).float()
    attn = attn / attn.sum(1, keepdim=True)
    return logits, bias, pg, lens, ext, attn


def _topk_ref(dist, K):
    """Top-K of a materialised distribution, equal values to the lower id (the rule of tf.nn.top_k
    and of the kernel; torch.topk's tie order is not defined, and 1.6 million random logits do
    hold two equal ones among a row's best)."""
    v, i = torch.sort(dist, dim=1, descending=True, stable=True)
    return v[:, :K], i[:, :K]


def _topk_run(k, fn, logits, bias, pg, attn, ext, lens, R, V, T, K, beam):
    S = int(k.topk_parts(V))
    ids = torch.full((R, K), -1, dtype=torch.int32, device=DEV)
    lp = torch.zeros(R, K, device=DEV)
    fn(logits, bias, pg, attn, ext, lens, ids, lp, torch.zeros(R, S, 2, device=DEV), torch.zeros(R, S, K, device=DEV),
       torch.zeros(R, S, K, dtype=torch.int32, device=DEV), R, V, T, K, beam)
    return ids, lp


@pytest.mark.parametrize("V", [3000, 20000])
@pytest.mark.parametrize("K", [20, 32])
def test_final_topk_wide_matches_materialised_distribution(K, V):
    """The shape of test_gpu_decode's final_topk test (5 articles x beam rows, T = 96, duplicates
    and in-article OOVs in ext) at K = 2 * beam = 20 and 32, one vocabulary split (V = 3000) and
    three (V = 20000), pointer and baseline mode."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, beam, T = 5, K // 2, 96
    R = Na * beam
    assert int(k.topk_parts(V)) == (1 if V == 3000 else 3)
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, beam, V, T, seed=K + V)
    ids, lp = _topk_run(k, k.final_topk, logits, bias, pg, attn, ext, lens, R, V, T, K, beam)
    vd = torch.softmax(logits + bias, 1)
    fd = torch.cat([pg[:, None] * vd, torch.zeros(R, 20, device=DEV)], 1)
    fd = fd.scatter_add(1, ext.repeat_interleave(beam, 0).long(), (1 - pg[:, None]) * attn)
    rp, ri = _topk_ref(fd, K)
    assert torch.equal(ids.long(), ri)
    torch.testing.assert_close(lp, torch.log(rp), rtol=1e-4, atol=1e-5)
    # baseline mode
    ids, lp = _topk_run(k, k.final_topk, logits, bias, None, None, ext, lens, R, V, T, K, beam)
    rp, ri = _topk_ref(vd, K)
    bad = (ids.long() != ri).any(1).nonzero().flatten().tolist()
    assert not bad, (bad, ids[bad[:2]].tolist(), ri[bad[:2]].tolist())
    torch.testing.assert_close(lp, torch.log(rp), rtol=1e-4, atol=1e-5)


def test_final_topk_wide_entry_equals_narrow_at_small_k():
    """final_topk_wide (the 32-entry list whatever K is: what the decoder's wide path calls) ==
    final_topk (the 16-entry list) at K = 8, bit for bit."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, beam, V, T, K = 5, 4, 3000, 96, 8
    R = Na * beam
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, beam, V, T, seed=1)
    for p, a in ((pg, attn), (None, None)):
        i0, l0 = _topk_run(k, k.final_topk, logits, bias, p, a, ext, lens, R, V, T, K, beam)
        i1, l1 = _topk_run(k, k.final_topk_wide, logits, bias, p, a, ext, lens, R, V, T, K, beam)
        assert torch.equal(i0, i1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32))


@pytest.mark.parametrize("V,pointer", [(3000, False), (20000, False), (3000, True)])
def test_final_topk_wide_tie_heavy_fallback(V, pointer):
    """All-equal logits plus a handful of raised ones at K = 32: every element passes the filter
    (more than 2048 survivors per block), so the partial kernel takes its fallback.  Expected order:
    by value, then by lower id (numpy lexsort; torch.topk's tie order is not defined).  Pointer
    mode: the copied ids get their combined values (distinct, far above rounding), the rest tie."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    Na, beam, T, K = 5, 16, 96, 32
    R = Na * beam
    _, _, pg, lens, ext, attn = _topk_inputs(Na, beam, V, T, seed=7)
    logits = torch.full((R, V), 0.25, device=DEV)
    bias = torch.zeros(V, device=DEV)
    raised = [5, 777, 1500, V - 1, V - 2, 2047, 2048, 40]
    for j, w in enumerate(raised):
        logits[:, w] += (1.0, 2.0, 1.0, 3.0, 0.5, 2.0, 0.5, 4.0)[j]  # equal values among the raised too
    logits[1, :] = 0.25  # one row with no raised logit at all: ids 0 .. 31
    p, a = (pg, attn) if pointer else (None, None)
    ids, lp = _topk_run(k, k.final_topk, logits, bias, p, a, ext, lens, R, V, T, K, beam)
    vd = torch.softmax(logits.double() + bias.double(), 1)
    if pointer:
        fd = torch.cat([pg.double()[:, None] * vd, torch.zeros(R, 20, device=DEV, dtype=torch.float64)], 1)
        fd = fd.scatter_add(1, ext.repeat_interleave(beam, 0).long(), (1 - pg.double()[:, None]) * attn.double())
    else:
        fd = vd
    fd = fd.cpu().numpy()
    # ties are exact in the kernel (equal logits): make them exact here by rounding to fp32
    val = fd.astype(f32)
    got = ids.cpu().numpy()
    for r in range(R):
        order = np.lexsort((np.arange(val.shape[1]), -val[r]))[:K]
        np.testing.assert_array_equal(got[r], order, err_msg=f"row {r}")
        np.testing.assert_allclose(lp[r].cpu().numpy(), np.log(fd[r, order]), rtol=1e-4, atol=1e-5)
    if not pointer:
        assert got[1].tolist() == list(range(K))


# ------------------------------------------------------------------ 2. bookkeeping against a mirror
def _key(tot, il, beta, cp):
    """pen_key in its order: two fp32 products, one fp32 difference."""
    return f32(f32(f32(tot) * f32(il)) - f32(f32(beta) * f32(cp)))


def _mirror_step(st, ids, lps, t, beam, K, stop, min_dec, n, pen):
    """beam_search.py's step (reference beam_search.py:110-156) for Na articles in fp32 on (raw sum,
    key, token sequence) state.  n: block_ngram_repeat; pen: None or (inv_len, beta, cpen) -- the
    candidates are then ranked by the key and the raw sum is carried.  Returns the number of blocked
    candidates and of articles where two reachable candidates had equal keys."""
    nblocked = nties = 0
    for a in range(len(st["done"])):
        base = a * beam
        if st["done"][a]:
            st["gidx"][base:base + beam] = np.arange(base, base + beam)
            continue
        cands = []
        for i in range(1 if t == 0 else beam):
            for j in range(K):
                w = int(ids[base + i, j])
                blk = ngram_blocked(st["seq"][base + i], w, n)
                nblocked += blk
                tot = f32(st["lp"][base + i] + (BLOCKED if blk else lps[base + i, j]))
                key = _key(tot, pen[0][t + 2], pen[1], pen[2][base + i]) if pen else tot
                cands.append((key, tot, i, w))
        order = sorted(range(len(cands)), key=lambda c: cands[c][0], reverse=True)  # stable
        new, seen = [], []
        for c in order:
            key, tot, i, tok = cands[c]
            seen.append(key)
            if tok == stop:
                if t >= min_dec:
                    st["res"][a].append((key if pen else f32(tot / f32(t + 2)), tot, t, i))
            else:
                new.append((tot, key, tok, i))
            if len(new) == beam or len(st["res"][a]) == beam:
                break
        nties += len(set(seen)) < len(seen)
        if len(st["res"][a]) >= beam:
            st["done"][a] = 1
        old = [list(s) for s in st["seq"][base:base + beam]]
        for kk in range(beam):
            tot, key, tok, i = new[min(kk, len(new) - 1)] if new else (f32(-np.inf), f32(-np.inf), stop, 0)
            st["lp"][base + kk], st["key"][base + kk] = tot, key
            st["latest"][base + kk] = tok
            st["gidx"][base + kk] = base + i
            st["par"][base + kk] = i
            st["seq"][base + kk] = old[i] + [tok]
    return nblocked, nties


def _bits(x):
    return np.asarray(x, f32).view(np.int32)


def _drive_wide(k, beam, K, mode):
    """12 steps from t = 0 of beam_step_wide, Na = 6, against the mirror at every step.

    Candidates: K distinct ids per row out of 40 ordinary ids in a noisy preference order (so the
    beams revisit a few tokens and trigrams repeat); article a's rows carry a [STOP] among their
    three best candidates with probability (0.9, 0.6, 0.3, 0.15, 0.05, 0), before and after
    min_dec = 2: the first articles finish mid-run, the last never.  Log-probs: descending
    multiples of 2^-10 per row ("dyadic": multiples of 1/4 up to 12, so that totals of different
    hypotheses are equal and the stable tie order decides).  "ng": n = 3 with one row whose K
    candidates are all blocked; "pen": wu at alpha 0.9, beta 0.5, cpen random multiples of 2^-6."""
    rng = np.random.default_rng(1000 * beam + K)
    crng = np.random.default_rng(12)
    Na, stop, start, min_dec, maxD, T = 6, 3, 2, 2, 12, 7
    n = 3 if "ng" in mode else 0
    use_pen = "pen" in mode
    beta = 0.5
    pool = 10 + np.arange(40)
    R, P = Na * beam, 16
    z = lambda s, d: torch.zeros(s, dtype=d, device=DEV)  # noqa: E731
    dev = {nm: z(s, d) for nm, s, d in [
        ("lp", (R,), torch.float32), ("latest", (R,), torch.int32), ("gidx", (R,), torch.int32),
        ("th", (maxD, R), torch.int32), ("ph", (maxD, R), torch.int32), ("done", (Na,), torch.int32),
        ("rc", (Na,), torch.int32), ("rs", (R,), torch.float32), ("rl", (R,), torch.int32),
        ("rst", (R,), torch.int32), ("rp", (R,), torch.int32), ("step", (1,), torch.int32),
        ("att", (R, T), torch.float32), ("ah", (maxD, R, T), torch.float32), ("pg", (R,), torch.float32),
        ("pgh", (maxD, R), torch.float32), ("ks", (R,), torch.float32), ("rlp", (R,), torch.float32)]}
    dev["ks"].fill_(float("nan"))
    dev["rlp"].fill_(float("nan"))
    seq = [z((R, P), torch.int32), z((R, P), torch.int32)]
    seq[0][:, 0] = start
    seq[1].fill_(-7)  # stale contents must never be read as tokens
    inv_len = inv_len_table(HParams(length_penalty="wu", length_alpha=0.9), maxD + 1)
    inv_dev = torch.from_numpy(inv_len).to(DEV)
    st = {"lp": np.zeros(R, f32), "key": np.zeros(R, f32), "latest": np.zeros(R, np.int64), "gidx": np.arange(R),
          "par": np.zeros(R, np.int64), "done": np.zeros(Na, np.int64), "res": [[] for _ in range(Na)],
          "seq": [[start] for _ in range(R)]}
    forced, nblocked, nties = None, 0, 0
    pstop = (0.9, 0.6, 0.3, 0.15, 0.05, 0.0)

    def call(t, ids, lps, cpen):
        dev["step"].fill_(t + 1)  # beam_gather advances the counter at the start of a decode step
        k.beam_step_wide(torch.from_numpy(ids).to(DEV), torch.from_numpy(lps).to(DEV), dev["lp"], dev["latest"],
                         dev["gidx"], dev["th"], dev["ph"], dev["done"], dev["rc"], dev["rs"], dev["rl"], dev["rst"],
                         dev["rp"], dev["step"], dev["att"], dev["ah"], dev["pg"], dev["pgh"], T, Na, beam, K, stop,
                         min_dec, maxD, seq[0] if n else None, seq[1] if n else None, n,
                         inv_dev if use_pen else None, torch.from_numpy(cpen).to(DEV) if use_pen else None,
                         beta if use_pen else 0.0, dev["ks"] if use_pen else None, dev["rlp"] if use_pen else None)

    def draw(t):
        ids = np.zeros((R, K), np.int32)
        for r in range(R):
            ids[r] = pool[np.argsort(np.arange(40) + rng.normal(0, 1.5, 40))][:K]
            if rng.random() < pstop[r // beam]:
                ids[r, rng.integers(0, 3)] = stop
        if mode == "dyadic":
            lps = -np.sort(np.stack([rng.choice(np.arange(1, 49), K, replace=False) for _ in range(R)]), 1) \
                .astype(f32) / 4
        else:
            lps = -np.sort(np.stack([rng.choice(np.arange(1, 3000), K, replace=False) for _ in range(R)]), 1) \
                .astype(f32) / 1024
        return ids, lps, (crng.integers(0, 256, R) / 64.0).astype(f32)

    for t in range(maxD):
        ids, lps, cpen = draw(t)
        if n > 1 and forced is None and t >= 5:
            for r in range(R):
                banned = sorted({int(w) for w in pool if ngram_blocked(st["seq"][r], int(w), n)})
                if banned and not st["done"][r // beam]:
                    ids[r] = [banned[j % len(banned)] for j in range(K)]
                    forced = (t, r)
                    break
        dev["att"].uniform_()
        dev["pg"].uniform_()
        call(t, ids, lps, cpen)
        host = {nm: v.cpu().numpy().copy() for nm, v in dev.items()}
        assert host["step"][0] == t + 1  # the kernel leaves the counter alone
        np.testing.assert_array_equal(host["ah"][t], host["att"])
        np.testing.assert_array_equal(host["pgh"][t], host["pg"])
        was_live = np.repeat(st["done"] == 0, beam)
        nb, nt = _mirror_step(st, ids, lps, t, beam, K, stop, min_dec, n, (inv_len, beta, cpen) if use_pen else None)
        nblocked, nties = nblocked + nb, nties + nt
        np.testing.assert_array_equal(host["done"], st["done"])
        np.testing.assert_array_equal(host["gidx"], st["gidx"])
        if use_pen:
            np.testing.assert_array_equal(_bits(host["lp"][was_live]), _bits(st["lp"][was_live]))
            np.testing.assert_array_equal(_bits(host["ks"][was_live]), _bits(st["key"][was_live]))
        else:
            np.testing.assert_allclose(host["lp"][was_live], st["lp"][was_live], rtol=1e-6)
        np.testing.assert_array_equal(host["latest"][was_live], st["latest"][was_live])
        np.testing.assert_array_equal(host["th"][t][was_live], st["latest"][was_live])
        np.testing.assert_array_equal(host["ph"][t][was_live], st["par"][was_live])
        assert (host["th"][t][~was_live] == 0).all() and (host["th"][t + 1:] == 0).all()
        for a in range(Na):
            res = st["res"][a]
            assert host["rc"][a] == len(res)
            sl = slice(a * beam, a * beam + len(res))
            if use_pen:
                np.testing.assert_array_equal(_bits(host["rs"][sl]), _bits([x[0] for x in res]))
                np.testing.assert_array_equal(_bits(host["rlp"][sl]), _bits([x[1] for x in res]))
            else:
                np.testing.assert_allclose(host["rs"][sl], [x[0] for x in res], rtol=1e-6)
            np.testing.assert_array_equal(host["rst"][sl], [x[2] for x in res])
            np.testing.assert_array_equal(host["rp"][sl], [x[3] for x in res])
            np.testing.assert_array_equal(host["rl"][sl], [x[2] + 2 for x in res])
            assert (host["rl"][a * beam + len(res):(a + 1) * beam] == 0).all()  # nothing past the count
        if n:
            got = seq[(t + 1) & 1].cpu().numpy()
            for r in np.nonzero(was_live)[0]:
                assert got[r, :t + 2].tolist() == st["seq"][r]
    # every branch was taken: finished hypotheses, finished articles (mid-run) and live ones
    assert st["done"].any() and (st["done"] == 0).any() and any(0 < len(x) < beam for x in st["res"]), \
        ([len(x) for x in st["res"]], st["done"])
    if mode == "dyadic":
        assert nties >= 5, nties
    if n:
        assert forced is not None and nblocked >= K, (forced, nblocked)
    # past max_dec: identity parents only
    before = {nm: v.clone() for nm, v in dev.items()}
    ids, lps, cpen = draw(maxD)
    dev["gidx"].fill_(-1)
    call(maxD, ids, lps, cpen)
    assert dev["gidx"].cpu().tolist() == list(range(R))
    for nm in ("lp", "latest", "th", "ph", "done", "rc", "rs", "rl", "rst", "rp"):
        assert torch.equal(dev[nm], before[nm]), nm


WIDE_SHAPES = [(6, 12), (10, 20), (16, 32)]  # past one wave; past 16 candidates per hypothesis; the largest


@pytest.mark.parametrize("beam,K", WIDE_SHAPES)
@pytest.mark.parametrize("mode", ["plain", "dyadic", "ng", "pen", "ng_pen"])
def test_beam_step_wide_matches_mirror(mode, beam, K):
    from textsummarization_on_flink_amd.ops import ops
    _drive_wide(ops(), beam, K, mode)


def test_beam_step_wide_refuses_out_of_range():
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    for beam, K in ((17, 32), (16, 33)):
        R = 2 * beam
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)  # noqa: E731
        zf = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
        with pytest.raises(RuntimeError, match="wide beam"):
            k.beam_step_wide(zi(R, K), zf(R, K), zf(R), zi(R), zi(R), zi(4, R), zi(4, R), zi(2), zi(2), zf(R), zi(R),
                             zi(R), zi(R), zi(1), None, None, None, None, 7, 2, beam, K, 3, 1, 4, None, None, 0, None,
                             None, 0.0, None, None)


# ------------------------------------------------------------------ 3. whole decodes
def _setup(beam, **kw):
    from test_gpu_decode import _peaked_setup
    hps, vocab, batch, params = _peaked_setup(True)
    return hps.replace(beam_size=beam, **kw), vocab, batch, params


def _pack(hyps):
    return [(h.tokens, h.avg_log_prob, h.score) for h in hyps]


OPTIONS = {"plain": {}, "ng": {"block_ngram_repeat": 3},
           "pen": {"length_penalty": "wu", "coverage_penalty_beta": 0.5}}


@pytest.mark.parametrize("beam", [2, 4, 5])
@pytest.mark.parametrize("opt", sorted(OPTIONS))
def test_wide_path_equals_one_wave_path(opt, beam):
    """At beams the one-wave kernels take, the decoder with ``wide_beam=True`` (final_topk with the
    32-entry list + beam_step_wide) == the default decoder's unfused step on materialised logits
    (fused_step and fused_vocab off, so that both sides run the same cell, attention, p_gen and
    logits kernels and differ only in the list size and the bookkeeping): tokens, avg_log_prob and
    score, bit for bit."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(beam, **OPTIONS[opt])
    Na, T = hps.batch_size, hps.max_enc_steps
    d0 = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=False)
    assert not d0.wide
    d0.fused_step = d0.fused_vocab = False
    d1 = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=False, wide_beam=True)
    assert d1.wide and not d1.fused_step and not d1.fused_vocab and d1.rep == d0.rep
    assert (d1.ngram, d1.pen is not None) == (3 if opt == "ng" else 0, opt == "pen")
    h0, h1 = d0.decode(batch), d1.decode(batch)
    assert len(h0) == Na and _pack(h0) == _pack(h1)
    for x, y in zip(h0, h1):
        np.testing.assert_array_equal(np.stack(x.attn_dists), np.stack(y.attn_dists))


@functools.lru_cache(maxsize=None)
def _graph_run(beam):
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(beam)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=True)
    assert d.wide and d.K == 2 * beam and d.rep == (beam if d.row_attn else 1)
    hg = d.decode(batch)
    # the vectorised backtracking == the per-candidate walk (results still on the device)
    for g, r in zip(d.results(), d._results_walk()):
        assert g.tokens == r.tokens and g.score == r.score
    return hps, vocab, batch, params, hg


@pytest.mark.parametrize("beam", [8, 10])
def test_wide_beam_graph_equals_eager(beam):
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params, hg = _graph_run(beam)
    de = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=False)
    he = de.decode(batch)
    assert len(hg) == hps.batch_size and [h.tokens for h in hg] == [h.tokens for h in he]
    assert len(hg[0].attn_dists) == len(hg[0].tokens) - 1


@pytest.mark.parametrize("beam", [8, 10])
def test_wide_beam_tracks_host_oracle(beam):
    """The criterion of test_device_beam_graph_equals_eager_and_tracks_oracle: the first 6 tokens
    agree with the host beam search over the fp32 oracle on at least Na - 2 articles."""
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    from textsummarization_on_flink_amd.decode.beam_search import OracleStepModel, run_beam_search
    from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator
    hps, vocab, batch, params, hg = _graph_run(beam)
    flat = params.flat
    W = {n: flat[o:o + c].view(params.view(n).shape) for n, (o, c) in params.offsets.items()}
    model = OracleStepModel(ReferencePointerGenerator(hps, vocab.size()), W, hps, device="cuda")
    hps1 = hps.replace(batch_size=hps.beam_size)
    agree = 0
    for a in range(hps.batch_size):
        ex = Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, hps1)
        b1 = Batch([ex] * hps.beam_size, hps1, vocab, pad_enc_to=hps.max_enc_steps)
        best = run_beam_search(model, vocab, b1, hps)
        n = min(len(best.tokens), len(hg[a].tokens), 6)
        agree += best.tokens[:n] == hg[a].tokens[:n]
    print("beam", beam, "first 6 tokens agree with the host oracle on", agree, "of", hps.batch_size)
    assert agree >= hps.batch_size - 2, agree


def _has_repeat(tokens, n):
    grams = [tuple(tokens[p:p + n]) for p in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


def test_beam10_with_blocking_and_penalties():
    """Beam 10 with trigram blocking, wu and the coverage penalty together: graph == eager, and no
    returned hypothesis repeats a trigram unless a blocked candidate was forced on it (its raw sum
    then carries BLOCKED_LP)."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(10, block_ngram_repeat=3, length_penalty="wu", coverage_penalty_beta=0.5)
    Na, T = hps.batch_size, hps.max_enc_steps
    out = []
    for graph in (True, False):
        d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=graph)
        assert d.wide and d.ngram == 3 and d.pen is not None and "cpen" in d.b
        out.append(_pack(d.decode(batch)))
    assert len(out[0]) == Na and out[0] == out[1]
    for toks, avg, score in out[0]:
        assert np.isfinite(score)
        assert avg < -1e18 or not _has_repeat(toks, 3)


def test_wide_beam_decode_batches_equal_batch_by_batch():
    """decode_batches (grouped encoder passes, results backtracked behind the next batch) inherits
    wide beams: == decode batch by batch at beam 10."""
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(10)
    corpus = SyntheticCorpus(vocab_size=hps.vocab_size, raw_vocab=3 * hps.vocab_size, seed=9, art_mean=40, art_sd=10,
                             sent_mean=4)
    batches = [batch] + make_batches(hps, vocab, corpus, 2, pad_enc_to=hps.max_enc_steps)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=True)
    assert d.wide and d.group_enc > 1
    seq = [_pack(d.decode(b)) for b in batches]
    piped = [_pack(hy) for hy in d.decode_batches(batches)]
    assert piped == seq


# ------------------------------------------------------------------ 4. row attention at rep = beam
@pytest.mark.parametrize("Na", [4, 8])
def test_attn_fwd_row_rep10_equals_rep2_on_replicated_features(Na):
    """attn_fwd_row shares an article's F / E rows between ``rep`` hypothesis rows.  rep = 10 on Na
    feature rows == rep = 2 on the same rows repeated 5 times (the same kernel and arithmetic per
    hypothesis row, only the feature row index differs), bit for bit; Na = 8 also takes the
    per-XCD row mapping (R / 8 a multiple of rep), Na = 4 does not at rep = 10."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    torch.manual_seed(Na)
    beam, T, A = 10, 70, 512
    R = Na * beam
    F = (torch.randn(Na, T, A, device=DEV) * 0.5).bfloat16()
    E = torch.randn(Na, T, A, device=DEV).bfloat16()
    s, v, wc = torch.randn(R, A, device=DEV) * 0.5, torch.randn(A, device=DEV) * 0.3, torch.randn(A, device=DEV) * 0.1
    cov = torch.rand(R, T, device=DEV)
    lens = torch.randint(1, T + 1, (Na,), dtype=torch.int32, device=DEV)
    lens[0] = T
    out = []
    for rep in (10, 2):
        r = beam // rep
        a, ctx = torch.zeros(R, T, device=DEV), torch.zeros(R, A, device=DEV)
        cb = torch.zeros(R, A, device=DEV, dtype=torch.bfloat16)
        k.attn_fwd_row(F.repeat_interleave(r, 0).contiguous(), E.repeat_interleave(r, 0).contiguous(), s, v, wc, cov,
                       lens.repeat_interleave(r).contiguous(), a, None, None, ctx, cb, R, T, A, rep)
        out.append((a, ctx, cb))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    a = out[0][0]
    torch.testing.assert_close(a.sum(1), torch.ones(R, device=DEV), rtol=1e-4, atol=1e-5)
    assert (a[:beam, :] > 0).all()  # article 0 has the full length


def test_wide_beam_row_attention_production_width():
    """Beam 10 at the production width (H = 256, A = 512: the row-resident attention kernel with
    rep = beam): graph == eager, token for token."""
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    from textsummarization_on_flink_amd.models.params import build_params
    Na, T, V = 8, 64, 2000
    hps = HParams(batch_size=Na, max_enc_steps=T, max_dec_steps=16, min_dec_steps=3, beam_size=10, vocab_size=V,
                  emb_dim=128, hidden_dim=256, coverage=True, pointer_gen=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3)
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=5, art_mean=50, art_sd=10, sent_mean=4)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=T)[0]
    params = build_params(hps, vocab.size(), device="cuda", seed=4)
    out = []
    for graph in (True, False):
        d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=graph)
        assert d.wide and d.row_attn and d.rep == 10
        out.append(_pack(d.decode(batch)))
    assert len(out[0]) == Na and out[0] == out[1]
