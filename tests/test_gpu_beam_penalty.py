"""Length and coverage penalties on the device: the ``cov_penalty`` kernel against float64, the
beam bookkeeping with the penalty pack against a bit-exact fp32 mirror, the default path, and the
pipelined ``decode_batches`` path, and whole decodes (fused step == unfused step, device == host
oracle) on an input where the penalties change most summaries."""
import functools
import math

import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.config import HParams
from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
from textsummarization_on_flink_amd.decode.beam_search import inv_len_table, ngram_blocked
from textsummarization_on_flink_amd.models.params import build_params

pytestmark = pytest.mark.gpu

BLOCKED = np.float32(-1e20)
f32 = np.float32


# ------------------------------------------------------------------ 1. cov_penalty against float64
@pytest.mark.parametrize("T,lens", [(7, (1, 7, 4)), (130, (1, 130, 67))])
def test_cov_penalty_matches_float64(T, lens):
    """R = 12 rows (3 articles, beam 4): a row shorter than one wave, T no multiple of 4 or 64
    (T = 130: the scalar path over more than one wave pass).  Inputs are multiples of 2^-20 below 2,
    so cov + att and the subtraction are exact in fp32 and only the sum of the non-negative terms
    rounds: at most len - 1 <= T roundings of relative 2^-24 each, bound T * 2^-23 relative."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    rng = np.random.default_rng(T)
    Na, beam = 3, 4
    R = Na * beam
    cov = (rng.integers(0, 3 << 19, (R, T)) / float(1 << 20)).astype(f32)   # [0, 1.5): around 1 with att
    att = (rng.integers(0, 1 << 19, (R, T)) / float(1 << 20)).astype(f32)   # [0, 0.5)
    for r in range(R):
        cov[r, lens[r // beam]:] = 40.0 + r   # garbage past the length: must be ignored
        att[r, lens[r // beam]:] = 3.0
    out = torch.full((R + 1,), float("nan"), device="cuda")
    out[R] = 123.0                            # sentinel past the end
    k.cov_penalty(torch.from_numpy(cov).cuda(), torch.from_numpy(att).cuda(),
                  torch.tensor(lens, dtype=torch.int32, device="cuda"), out, R, T, beam, None)
    got = out.cpu().numpy()
    assert got[R] == 123.0
    want = np.array([np.maximum(cov[r, :lens[r // beam]].astype(np.float64) + att[r, :lens[r // beam]] - 1.0, 0).sum()
                     for r in range(R)])
    assert np.isfinite(got[:R]).all()
    assert (want[beam:2 * beam] > 0).all()    # the full-length rows have something to sum
    err = np.abs(got[:R].astype(np.float64) - want)
    print("cov_penalty T", T, "max rel err", float((err / np.maximum(want, 1e-30)).max()))
    assert (err <= T * 2.0 ** -23 * want).all(), (got[:R], want)


@pytest.mark.parametrize("T", [8, 132])
def test_cov_penalty_vector_path(T):
    """T % 4 == 0: the 16-byte loads, lengths that end inside a float4 (and one on its edge); with
    the per-article vector a0 that the decoder subtracts from the coverage (multiples of 2^-20
    again, so every term is still exact)."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    rng = np.random.default_rng(100 + T)
    Na, beam = 3, 4
    R, lens = Na * beam, (1, T, T // 2 + 1)
    cov = (rng.integers(0, 3 << 19, (R, T)) / float(1 << 20)).astype(f32)
    att = (rng.integers(0, 1 << 19, (R, T)) / float(1 << 20)).astype(f32)
    a0 = (rng.integers(0, 1 << 18, (Na, T)) / float(1 << 20)).astype(f32)     # [0, 0.25)
    for r in range(R):
        cov[r, lens[r // beam]:] = 40.0 + r
    out = torch.full((R + 1,), float("nan"), device="cuda")
    out[R] = 123.0
    k.cov_penalty(torch.from_numpy(cov).cuda(), torch.from_numpy(att).cuda(),
                  torch.tensor(lens, dtype=torch.int32, device="cuda"), out, R, T, beam, torch.from_numpy(a0).cuda())
    got = out.cpu().numpy()
    want = np.array([np.maximum(cov[r, :lens[r // beam]].astype(np.float64) + att[r, :lens[r // beam]]
                                - a0[r // beam, :lens[r // beam]] - 1.0, 0).sum() for r in range(R)])
    assert (want[beam:2 * beam] > 0).all()
    assert got[R] == 123.0 and np.isfinite(got[:R]).all()
    assert (np.abs(got[:R].astype(np.float64) - want) <= T * 2.0 ** -23 * want).all(), (got[:R], want)


# ------------------------------------------------------------------ 2. bookkeeping against a mirror
def _key(tot, il, beta, cp):
    """The kernel's rank key in its order: two fp32 products, one fp32 difference."""
    return f32(f32(f32(tot) * f32(il)) - f32(f32(beta) * f32(cp)))


def _mirror_step(st, ids, lps, cpen, inv_len, beta, t, beam, K, stop, min_dec, n):
    """beam_search.py's step on (raw sum, key, token sequence) state in fp32: candidates ranked by
    the key, the raw sum carried.  Returns (blocked candidates, articles whose key order differs
    from their raw-sum order)."""
    nblocked = reordered = 0
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
                cands.append((_key(tot, inv_len[t + 2], beta, cpen[base + i]), tot, i, w))
        order = sorted(range(len(cands)), key=lambda c: cands[c][0], reverse=True)  # stable
        reordered += order != sorted(range(len(cands)), key=lambda c: cands[c][1], reverse=True)
        new = []
        for c in order:
            key, tot, i, tok = cands[c]
            if tok == stop:
                if t >= min_dec:
                    st["res"][a].append((key, tot, t, i))
            else:
                new.append((tot, key, tok, i))
            if len(new) == beam or len(st["res"][a]) == beam:
                break
        if len(st["res"][a]) >= beam:
            st["done"][a] = 1
        old = [list(s) for s in st["seq"][base:base + beam]]
        for kk in range(beam):
            tot, key, tok, i = new[min(kk, len(new) - 1)] if new else (f32(-np.inf), f32(-np.inf), stop, 0)
            st["lp"][base + kk], st["key"][base + kk] = tot, key
            st["latest"][base + kk] = tok
            st["gidx"][base + kk] = base + i
            st["seq"][base + kk] = old[i] + [tok]
    return nblocked, reordered


def _backtrack(th, ph, t, row, base, start):
    toks, slot = [], row - base
    for tl in range(t, -1, -1):
        toks.append(int(th[tl, base + slot]))
        slot = int(ph[tl, base + slot])
    return [start] + toks[::-1]


def _bits(x):
    return np.asarray(x, f32).view(np.int32)


@pytest.mark.parametrize("n", [0, 3])
def test_beam_step_pen_matches_mirror_bit_for_bit(n):
    """The data of test_gpu_ngram_block's driver (Na = 3, beam = 4, K = 8, 12 steps, log-probs
    multiples of 2^-10, article 0 finishes early, article 2 never; with n = 3 one fully blocked
    row) through beam_step_pen: cpen random multiples of 2^-6 per row and step, beta 0.5, inv_len
    of wu at alpha 0.9.  Every buffer equals the fp32 mirror at every step."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    rng = np.random.default_rng(11)
    crng = np.random.default_rng(12)
    Na, beam, K, stop, start, min_dec, maxD, V = 3, 4, 8, 3, 2, 2, 12, 50
    beta = 0.5
    pool = np.array([10, 11, 12, 13, 14, 15, V + 2, V + 7])
    R, P = Na * beam, 16
    z = lambda s, d: torch.zeros(s, dtype=d, device="cuda")  # noqa: E731
    dev = {nm: z(s, d) for nm, s, d in [
        ("lp", (R,), torch.float32), ("latest", (R,), torch.int32), ("gidx", (R,), torch.int32),
        ("th", (maxD, R), torch.int32), ("ph", (maxD, R), torch.int32), ("done", (Na,), torch.int32),
        ("rc", (Na,), torch.int32), ("rs", (R,), torch.float32), ("rl", (R,), torch.int32),
        ("rst", (R,), torch.int32), ("rp", (R,), torch.int32), ("step", (1,), torch.int32),
        ("ctr", (1,), torch.int32), ("ks", (R,), torch.float32), ("rlp", (R,), torch.float32)]}
    dev["ks"].fill_(float("nan"))
    dev["rlp"].fill_(float("nan"))
    seq = [z((R, P), torch.int32), z((R, P), torch.int32)]
    seq[0][:, 0] = start
    seq[1].fill_(-7)
    inv_len = inv_len_table(HParams(length_penalty="wu", length_alpha=0.9), maxD + 1)
    assert inv_len.dtype == f32 and len(inv_len) == maxD + 2
    inv_dev = torch.from_numpy(inv_len).cuda()
    st = {"lp": np.zeros(R, f32), "key": np.zeros(R, f32), "latest": np.zeros(R, np.int64), "gidx": np.arange(R),
          "done": np.zeros(Na, np.int64), "res": [[] for _ in range(Na)], "seq": [[start] for _ in range(R)]}
    forced, nblocked, reordered = None, 0, 0
    for t in range(maxD):
        ids = np.zeros((R, K), np.int32)
        for r in range(R):
            ids[r] = pool[np.argsort(np.arange(8) + rng.normal(0, 1.5, 8))]
            if rng.random() < (0.7, 0.2, 0.0)[r // beam]:
                ids[r, rng.integers(0, 3)] = stop
        lps = -np.sort(np.stack([rng.choice(np.arange(1, 3000), K, replace=False) for _ in range(R)]), 1) \
            .astype(f32) / 1024
        cpen = (crng.integers(0, 256, R) / 64.0).astype(f32)
        if n > 1 and forced is None and t >= 5:
            for r in range(R):
                banned = sorted({int(w) for w in pool if ngram_blocked(st["seq"][r], int(w), n)})
                if banned and not st["done"][r // beam]:
                    ids[r] = [banned[j % len(banned)] for j in range(K)]
                    forced = (t, r)
                    break
        k.beam_step_pen(torch.from_numpy(ids).cuda(), torch.from_numpy(lps).cuda(), dev["lp"], dev["latest"],
                        dev["gidx"], dev["th"], dev["ph"], dev["done"], dev["rc"], dev["rs"], dev["rl"], dev["rst"],
                        dev["rp"], dev["step"], dev["ctr"], None, None, None, None, 7, Na, beam, K, stop, min_dec, maxD,
                        seq[0] if n else None, seq[1] if n else None, n, inv_dev, torch.from_numpy(cpen).cuda(), beta,
                        dev["ks"], dev["rlp"])
        assert int(dev["step"].item()) == t + 1
        host = {nm: v.cpu().numpy().copy() for nm, v in dev.items()}
        was_live = np.repeat(st["done"] == 0, beam)
        nb, ro = _mirror_step(st, ids, lps, cpen, inv_len, beta, t, beam, K, stop, min_dec, n)
        nblocked, reordered = nblocked + nb, reordered + ro
        np.testing.assert_array_equal(host["done"], st["done"])
        live = np.repeat(st["done"] == 0, beam)
        np.testing.assert_array_equal(_bits(host["lp"][live]), _bits(st["lp"][live]))
        np.testing.assert_array_equal(_bits(host["ks"][live]), _bits(st["key"][live]))
        np.testing.assert_array_equal(host["latest"][live], st["latest"][live])
        np.testing.assert_array_equal(host["gidx"], st["gidx"])
        for a in range(Na):
            res = st["res"][a]
            assert host["rc"][a] == len(res)
            sl = slice(a * beam, a * beam + len(res))
            np.testing.assert_array_equal(_bits(host["rs"][sl]), _bits([x[0] for x in res]))
            np.testing.assert_array_equal(_bits(host["rlp"][sl]), _bits([x[1] for x in res]))
            np.testing.assert_array_equal(host["rst"][sl], [x[2] for x in res])
            np.testing.assert_array_equal(host["rp"][sl], [x[3] for x in res])
            np.testing.assert_array_equal(host["rl"][sl], [x[2] + 2 for x in res])
        for r in np.nonzero(was_live)[0]:
            want = st["seq"][r]
            assert _backtrack(host["th"], host["ph"], t, r, r // beam * beam, start) == want
            if n:
                assert seq[(t + 1) & 1][r, :t + 2].tolist() == want
    # every branch was taken: finished hypotheses, a finished article, a live one, the key order
    # different from the raw-sum order, and (n = 3) blocked candidates with one fully blocked row
    assert any(len(x) > 0 for x in st["res"]) and st["done"].any() and (st["done"] == 0).any(), \
        ([len(x) for x in st["res"]], st["done"])
    assert reordered >= 1
    if n:
        assert forced is not None and nblocked >= K, (forced, nblocked)
    else:
        assert nblocked == 0


# ------------------------------------------------------------------ 3. / 4. whole decodes
BETA, ATT_SCALE, HEAD_WIDEN = 2.0, 12.0, 0.1


def penalty_setup(n, device="cuda"):
    """ladder_setup's shape and data (Na = 16, T = 120, V = 3000, H = 256, coverage on) with two
    changes to its parameters.  The attention parameters are scaled by 12: the attention is peaked
    enough that a hypothesis' coverage passes 1 at several positions (cp of the returned
    hypotheses between 7 and 20 after 30 steps) and differs between the hypotheses of a beam.
    The ladder's best and second token are raised by 0.2 and 0.1: its first steps, 0.05 and 0.08,
    put the raw scores of competing hypotheses 0.01 to 0.02 apart once divided by L(30) = 4.9,
    while the device's score under the penalty is 1e-3 to 3e-3 relative (0.03 to 0.1 absolute)
    from the fp32 oracle's, because its attention comes from bf16 features; with the steps at
    0.15 and 0.18 the ties are no closer than that noise.  wu at alpha 0.9, beta = 2.

    Host oracle alone (OracleStepModel + run_beam_search on the CPU): against the same search with
    the penalties off, 9 of 16 articles return different tokens with n = 0 and 11 of 16 with
    n = 3; the fp32 and the fp64 oracle return the same tokens for 16 of 16 articles in both cases
    (scores within 1.4e-6 relative).  Recorded in profiles/beam_penalty.md."""
    from test_gpu_ngram_block import ladder_setup
    from textsummarization_on_flink_amd.models.pointer_generator import ATT_M, OV, VATT, WCOV, WH
    hps, vocab, batch, params = ladder_setup(True, n, device=device)
    for nm in (WH, VATT, ATT_M, WCOV):
        params.view(nm).mul_(ATT_SCALE)
    params[OV][100] += 2 * HEAD_WIDEN   # the ladder's tokens are 100 + 61 i
    params[OV][161] += HEAD_WIDEN
    return hps.replace(length_penalty="wu", coverage_penalty_beta=BETA), vocab, batch, params


def _pack(hyps):
    return ([h.tokens for h in hyps], [h.score for h in hyps], [h.avg_log_prob for h in hyps],
            [np.stack(h.attn_dists) for h in hyps])


@functools.lru_cache(maxsize=None)
def _device_runs(n):
    """Fused and unfused decodes with the penalties, and the fused decode without them."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = penalty_setup(n)
    Na, T = hps.batch_size, hps.max_enc_steps
    out = {}
    for fused in (True, False):
        d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=True)
        assert d.fused_step and d.pen is not None and "cpen" in d.b and d.ngram == n
        d.fused_step = fused
        out[fused] = _pack(d.decode(batch))
    d0 = DeviceBeamDecoder(hps.replace(length_penalty="avg", coverage_penalty_beta=0.0), vocab, params, n_articles=Na,
                           T=T, use_graph=True)
    assert d0.fused_step and d0.pen is None
    out["off"] = _pack(d0.decode(batch))
    return hps, vocab, batch, params, out


@pytest.mark.parametrize("n", [0, 3])
def test_fused_equals_unfused_with_penalties(n):
    hps, vocab, batch, params, out = _device_runs(n)
    Na = hps.batch_size
    (tok_f, sc_f, avg_f, att_f), (tok_u, sc_u, avg_u, att_u) = out[True], out[False]
    assert len(tok_f) == Na and tok_f == tok_u
    np.testing.assert_allclose(sc_f, sc_u, rtol=1e-6)
    np.testing.assert_allclose(avg_f, avg_u, rtol=1e-6)
    for x, y in zip(att_f, att_u):
        np.testing.assert_array_equal(x, y)
    # every returned hypothesis is consistent with itself: the score recomputed in float64 from
    # its average log-prob, its length and its attention distributions (fp32 sums of at most
    # 30 steps x 120 positions on the device: rtol 1e-4)
    worst = 0.0
    for a in range(Na):
        ln = len(tok_f[a])
        c = att_f[a].astype(np.float64).sum(0)[:int(batch.enc_lens[a])]
        want = avg_f[a] * ln / ((5.0 + ln) / 6.0) ** 0.9 - BETA * np.maximum(c - 1.0, 0.0).sum()
        worst = max(worst, abs(sc_f[a] - want) / abs(want))
    print("self-consistency: worst relative difference", worst)
    assert worst <= 1e-4, worst
    # the penalties change the outcome: otherwise the equality above shows nothing
    differ = sum(x != y for x, y in zip(tok_f, out["off"][0]))
    print("articles whose tokens differ from the search without penalties:", differ, "of", Na)
    assert differ >= Na // 2, differ


@pytest.mark.parametrize("n", [0, 3])
def test_device_agrees_with_host_oracle_with_penalties(n):
    """Device tokens == host oracle tokens (fp32, same weights) for at least ceil(0.9 * 16) = 15
    articles, the agreeing articles' scores within 2e-2 relative."""
    from test_gpu_decode_parity import _weights
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    from textsummarization_on_flink_amd.decode.beam_search import OracleStepModel, run_beam_search
    from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator
    hps, vocab, batch, params, out = _device_runs(n)
    Na, T = hps.batch_size, hps.max_enc_steps
    tok_d, sc_d = out[True][0], out[True][1]
    model = OracleStepModel(ReferencePointerGenerator(hps, vocab.size()), _weights(params), hps, device="cuda")
    h1 = hps.replace(batch_size=hps.beam_size)
    agree, worst = 0, 0.0
    for a in range(Na):
        ex = Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, h1)
        best = run_beam_search(model, vocab, Batch([ex] * hps.beam_size, h1, vocab, pad_enc_to=T), hps)
        if best.tokens == tok_d[a]:
            agree += 1
            rel = abs(sc_d[a] - best.score) / abs(best.score)
            worst = max(worst, rel)
    print("device == host oracle:", agree, "of", Na, "worst score difference", worst)
    assert agree >= int(math.ceil(0.9 * Na)), (agree, Na)
    assert worst <= 2e-2, worst


# ------------------------------------------------------------------ 5. the default path
def _small(**kw):
    Na, T, V = 8, 48, 600
    hps = HParams(batch_size=Na, max_enc_steps=T, max_dec_steps=20, min_dec_steps=3, beam_size=4, vocab_size=V,
                  emb_dim=64, hidden_dim=64, coverage=True, pointer_gen=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3, **kw)
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=2, art_mean=40, art_sd=10, sent_mean=4)
    vocab = corpus.vocab(V)
    batches = make_batches(hps, vocab, corpus, 3, pad_enc_to=T)
    params = build_params(hps, vocab.size(), device="cuda", seed=3)
    return hps, vocab, batches, params


def test_default_flags_allocate_nothing_and_beta_needs_coverage():
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, _, params = _small()
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=False)
    assert d.pen is None
    assert not {"cpen", "key_sum", "res_lp", "inv_len"} & set(d.b)
    with pytest.raises(ValueError):
        DeviceBeamDecoder(hps.replace(coverage_penalty_beta=0.3, coverage=False), vocab, params,
                          n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=False)
    # the length penalty alone needs no coverage penalty buffer (and no cov_penalty launch)
    d = DeviceBeamDecoder(hps.replace(length_penalty="wu"), vocab, params, n_articles=hps.batch_size,
                          T=hps.max_enc_steps, use_graph=False)
    assert d.pen is not None and "cpen" not in d.b and {"key_sum", "res_lp", "inv_len"} <= set(d.b)


# ------------------------------------------------------------------ 6. pipeline inheritance
def test_decode_batches_inherit_penalties():
    """decode_batches (grouped encoder passes, results backtracked behind the next batch) ==
    decode batch by batch with wu and a coverage penalty: tokens, avg_log_prob and score."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batches, params = _small(length_penalty="wu", coverage_penalty_beta=0.5)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=True)
    assert d.pen is not None and "cpen" in d.b and d.group_enc > 1
    seq = [[(h.tokens, h.avg_log_prob, h.score) for h in d.decode(b)] for b in batches]
    piped = [[(h.tokens, h.avg_log_prob, h.score) for h in hy] for hy in d.decode_batches(batches)]
    assert piped == seq
    assert all(np.isfinite(s) and np.isfinite(a) for b in seq for _, a, s in b)
    # the vectorised backtracking == the per-candidate walk (last batch still on the device)
    for g, r in zip(d.results(), d._results_walk()):
        assert g.tokens == r.tokens and g.score == r.score and g.avg_log_prob == r.avg_log_prob
