"""block_ngram_repeat on the device: the beam bookkeeping kernel against a Python mirror that
applies ``ngram_blocked``, the fused and unfused decode steps end to end, and the pipelined
``decode_batches`` path."""
import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.config import HParams
from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
from textsummarization_on_flink_amd.decode.beam_search import ngram_blocked
from textsummarization_on_flink_amd.models.params import build_params
from textsummarization_on_flink_amd.models.pointer_generator import OV

pytestmark = pytest.mark.gpu

HEAD = (0.05, 0.08)  # the ladder's first steps: its three best tokens nearly tie (see ladder_setup)
BLOCKED = np.float32(-1e20)


def _has_repeat(tokens, n):
    grams = [tuple(tokens[p:p + n]) for p in range(len(tokens) - n + 1)]
    return len(grams) != len(set(grams))


# ------------------------------------------------------------------ 1. kernel against a mirror
def _mirror_beam_step(state, ids, lps, t, beam, K, stop, min_dec, n):
    """beam_search.py's step for Na articles on (lp, token sequence) state, ``ngram_blocked``
    applied to each candidate before the total is formed; fp32 sums (exact: multiples of 2^-10)."""
    nblocked = 0
    for a in range(len(state["done"])):
        base = a * beam
        if state["done"][a]:
            state["gidx"][base:base + beam] = np.arange(base, base + beam)
            continue
        cands = []
        for i in range(1 if t == 0 else beam):
            for j in range(K):
                w = int(ids[base + i, j])
                blk = ngram_blocked(state["seq"][base + i], w, n)
                nblocked += blk
                cands.append((np.float32(state["lp"][base + i] + (BLOCKED if blk else lps[base + i, j])), i, w))
        order = sorted(range(len(cands)), key=lambda c: cands[c][0], reverse=True)  # stable
        new = []
        for c in order:
            v, i, tok = cands[c]
            if tok == stop:
                if t >= min_dec:
                    state["res"][a].append((v / np.float32(t + 2), t, i))
            else:
                new.append((v, tok, i))
            if len(new) == beam or len(state["res"][a]) == beam:
                break
        if len(state["res"][a]) >= beam:
            state["done"][a] = 1
        old = [list(s) for s in state["seq"][base:base + beam]]
        for kk in range(beam):
            # (no live hypothesis left -- the article just finished: parent 0, [STOP], -inf)
            v, tok, i = new[min(kk, len(new) - 1)] if new else (np.float32(-np.inf), stop, 0)
            state["lp"][base + kk] = v
            state["latest"][base + kk] = tok
            state["gidx"][base + kk] = base + i
            state["seq"][base + kk] = old[i] + [tok]
    return nblocked


def _backtrack(th, ph, t, row, base, start):
    toks, slot = [], row - base
    for tl in range(t, -1, -1):
        toks.append(int(th[tl, base + slot]))
        slot = int(ph[tl, base + slot])
    return [start] + toks[::-1]


def _drive(n, entry):
    """12 steps of the unfused bookkeeping, Na = 3, beam = 4, K = 8.  Candidates: per-row distinct
    ids from six ordinary tokens and two ids >= V (eight distinct candidates need a pool of eight)
    plus [STOP], a fixed preference order with noise so that the beams repeat themselves;
    log-probs distinct multiples of 2^-10.  From step 5 on, the first hypothesis that has a
    blocked token gets a row whose eight candidates are all blocked (drawn from its blocked
    tokens, so with repeats in that one row).  Checked against the mirror at every step."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    return _drive_with(k, n, entry)


def _drive_with(k, n, entry):
    rng = np.random.default_rng(11)
    Na, beam, K, stop, start, min_dec, maxD, V = 3, 4, 8, 3, 2, 2, 12, 50
    pool = np.array([10, 11, 12, 13, 14, 15, V + 2, V + 7])
    R, P = Na * beam, 16
    z = lambda s, d: torch.zeros(s, dtype=d, device="cuda")  # noqa: E731
    dev = {nm: z(s, d) for nm, s, d in [
        ("lp", (R,), torch.float32), ("latest", (R,), torch.int32), ("gidx", (R,), torch.int32),
        ("th", (maxD, R), torch.int32), ("ph", (maxD, R), torch.int32), ("done", (Na,), torch.int32),
        ("rc", (Na,), torch.int32), ("rs", (R,), torch.float32), ("rl", (R,), torch.int32),
        ("rst", (R,), torch.int32), ("rp", (R,), torch.int32), ("step", (1,), torch.int32),
        ("ctr", (1,), torch.int32)]}
    seq = [z((R, P), torch.int32), z((R, P), torch.int32)]
    seq[0][:, 0] = start
    seq[1].fill_(-7)  # stale contents must never be read as tokens
    st = {"lp": np.zeros(R, np.float32), "latest": np.zeros(R, np.int64), "gidx": np.arange(R),
          "done": np.zeros(Na, np.int64), "res": [[] for _ in range(Na)], "seq": [[start] for _ in range(R)]}
    forced, nblocked, trace = None, 0, []
    for t in range(maxD):
        ids = np.zeros((R, K), np.int32)
        for r in range(R):
            ids[r] = pool[np.argsort(np.arange(8) + rng.normal(0, 1.5, 8))]
            if rng.random() < (0.7, 0.2, 0.0)[r // beam]:  # article 0 finishes early, article 2 never
                ids[r, rng.integers(0, 3)] = stop
        lps = -np.sort(np.stack([rng.choice(np.arange(1, 3000), K, replace=False) for _ in range(R)]), 1) \
            .astype(np.float32) / 1024
        if n > 1 and forced is None and t >= 5:
            for r in range(R):
                banned = sorted({int(w) for w in pool if ngram_blocked(st["seq"][r], int(w), n)})
                if banned and not st["done"][r // beam]:
                    ids[r] = [banned[j % len(banned)] for j in range(K)]
                    forced = (t, r)
                    break
        args = (torch.from_numpy(ids).cuda(), torch.from_numpy(lps).cuda(), dev["lp"], dev["latest"], dev["gidx"],
                dev["th"], dev["ph"], dev["done"], dev["rc"], dev["rs"], dev["rl"], dev["rst"], dev["rp"],
                dev["step"], dev["ctr"], None, None, None, None, 7, Na, beam, K, stop, min_dec, maxD)
        if entry == "ng":
            k.beam_step_ng(*args, seq[0], seq[1], n)
        else:
            k.beam_step(*args)
        assert int(dev["step"].item()) == t + 1
        host = {nm: v.cpu().numpy().copy() for nm, v in dev.items()}
        host["seq"] = seq[(t + 1) & 1].cpu().numpy().copy()
        trace.append(host)
        if entry != "ng" or n <= 1:
            _mirror_beam_step(st, ids, lps, t, beam, K, stop, min_dec, 0)
            continue
        was_live = np.repeat(st["done"] == 0, beam)
        nblocked += _mirror_beam_step(st, ids, lps, t, beam, K, stop, min_dec, n)
        np.testing.assert_array_equal(host["done"], st["done"])
        live = np.repeat(st["done"] == 0, beam)
        np.testing.assert_array_equal(host["lp"][live], st["lp"][live])  # exact sums
        np.testing.assert_array_equal(host["latest"][live], st["latest"][live])
        np.testing.assert_array_equal(host["gidx"], st["gidx"])
        for a in range(Na):
            assert host["rc"][a] == len(st["res"][a])
            np.testing.assert_allclose(host["rs"][a * beam:a * beam + host["rc"][a]], [x[0] for x in st["res"][a]],
                                       rtol=1e-6)
        for r in np.nonzero(was_live)[0]:  # rows of articles that took this step
            want = st["seq"][r]
            assert host["seq"][r, :t + 2].tolist() == want
            assert _backtrack(host["th"], host["ph"], t, r, r // beam * beam, start) == want
    if entry == "ng" and n > 1:
        assert forced is not None and nblocked >= K, (forced, nblocked)
        # finished hypotheses, a finished article and a live one: every branch was taken
        assert any(len(x) > 0 for x in st["res"]) and st["done"].any() and (st["done"] == 0).any(), \
            ([len(x) for x in st["res"]], st["done"])
    return trace


@pytest.mark.parametrize("n", [2, 3])
def test_beam_step_ng_matches_mirror(n):
    _drive(n, "ng")


def test_beam_step_ng_off_equals_beam_step():
    """n = 0 through the new entry point == the existing entry point, bit for bit."""
    a, b = _drive(0, "ng"), _drive(0, "plain")
    for x, y in zip(a, b):
        for nm in x:
            if nm != "seq":  # (not written with blocking off)
                np.testing.assert_array_equal(x[nm].view(np.int32), y[nm].view(np.int32), err_msg=nm)


# ------------------------------------------------------------------ 2. end to end
def ladder_setup(coverage, n, device="cuda", Na=16, T=120, V=3000, H=256):
    """The shape of test_fused_decode_step_equals_unfused with the vocabulary bias raised on a
    ladder of 40 ordinary tokens (offsets descending from +30 in irregular steps of 0.5 .. 1.0,
    the first two steps 0.05 and 0.08): the decoder cycles through a few tokens, so the unblocked
    search repeats itself.

    The bias makes the model nearly context-free, so the search returns to its best token ``a``
    whenever it may.  With one clear best token the blocked search runs ``a a x a a y ..``: the
    suffix ``a a`` comes back every third step, ten times in 30 steps, but a hypothesis has only
    2 * beam = 8 candidates to follow it with, so a blocked candidate is forced near step 25 (host
    oracle: 16 of 16 articles with steps of 0.5 .. 1.0 throughout, 4 to 6 of 16 with a flat
    ladder).  Three nearly tied best tokens spread the visits over nine suffixes.  Host oracle
    (OracleStepModel + run_beam_search, fp32, coverage on and off): with n = 3 no article of 16
    is forced and none repeats a trigram, with n = 0 all 16 repeat one; the same with the head
    steps at (0.02, 0.04), (0.04, 0.09), (0.07, 0.06), (0.1, 0.12) and (0.15, 0.2)."""
    hps = HParams(mode="decode", batch_size=Na, max_enc_steps=T, max_dec_steps=30, min_dec_steps=5, beam_size=4,
                  vocab_size=V, emb_dim=128, hidden_dim=H, coverage=coverage, pointer_gen=True,
                  trunc_norm_init_std=0.05, block_ngram_repeat=n)
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=8, art_mean=100, art_sd=20, sent_mean=5)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=T)[0]
    params = build_params(hps, vocab.size(), device=device, seed=9)
    rng = np.random.default_rng(4)
    toks = 100 + 61 * np.arange(40)
    steps = rng.uniform(0.5, 1.0, 39)
    steps[:len(HEAD)] = HEAD
    offs = 30.0 - np.concatenate([[0.0], np.cumsum(steps)])
    params[OV][torch.as_tensor(toks, device=device)] += torch.as_tensor(offs, dtype=torch.float32, device=device)
    return hps, vocab, batch, params


@pytest.mark.parametrize("coverage", [True, False])
def test_fused_equals_unfused_with_trigram_blocking(coverage):
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = ladder_setup(coverage, 3)
    Na, T = hps.batch_size, hps.max_enc_steps
    res = []
    for fused in (True, False):
        d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=True)
        assert d.fused_step and d.ngram == 3  # the option does not turn the fused tail off
        d.fused_step = fused
        hy = d.decode(batch)
        res.append(([h.tokens for h in hy], [h.avg_log_prob for h in hy], [np.stack(h.attn_dists) for h in hy]))
    assert res[0][0] == res[1][0]
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-6)
    for x, y in zip(res[0][2], res[1][2]):
        np.testing.assert_array_equal(x, y)
    assert len(res[0][0]) == Na
    assert min(res[0][1]) > -1e18, "a blocked candidate was forced into a returned hypothesis"
    assert not any(_has_repeat(t, 3) for t in res[0][0])
    # the same setup without the option repeats itself: otherwise the above shows nothing
    d0 = DeviceBeamDecoder(hps.replace(block_ngram_repeat=0), vocab, params, n_articles=Na, T=T, use_graph=True)
    assert d0.fused_step and d0.ngram == 0 and d0.seq is None
    rep = sum(_has_repeat(h.tokens, 3) for h in d0.decode(batch))
    assert rep >= Na // 2, rep


# ------------------------------------------------------------------ 3. pipeline inheritance
def test_decode_batches_inherit_blocking():
    """decode_batches (grouped encoder passes, results backtracked behind the next batch) ==
    decode batch by batch with block_ngram_repeat = 3."""
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    Na, T, V = 8, 48, 600
    hps = HParams(batch_size=Na, max_enc_steps=T, max_dec_steps=20, min_dec_steps=3, beam_size=4, vocab_size=V,
                  emb_dim=64, hidden_dim=64, coverage=True, pointer_gen=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3, block_ngram_repeat=3)
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=2, art_mean=40, art_sd=10, sent_mean=4)
    vocab = corpus.vocab(V)
    batches = make_batches(hps, vocab, corpus, 3, pad_enc_to=T)
    params = build_params(hps, vocab.size(), device="cuda", seed=3)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=True)
    assert d.ngram == 3 and d.group_enc > 1
    seq = [[(h.tokens, h.avg_log_prob) for h in d.decode(b)] for b in batches]
    piped = [[(h.tokens, h.avg_log_prob) for h in hy] for hy in d.decode_batches(batches)]
    assert piped == seq
    for toks, avg in (x for b in seq for x in b):
        assert avg < -1e18 or not _has_repeat(toks, 3)
