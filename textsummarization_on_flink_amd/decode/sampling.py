"""Decode by sampling: top-k and full-distribution draws from the pointer-generator (host rule).

Not in the reference, which only runs beam search.  ``hps.sampling_topk`` = k in 1..31 draws each
token among the k most probable of the step's final (pointer-mixture) distribution, 0 draws from the
whole extended-vocabulary distribution; ``hps.n_samples`` independent samples per article, each with
its per-step model log-probs (what sample-and-rank decoding and self-critical training, Paulus et
al. 2017, need).  This module defines the semantics; the device kernels (csrc/kernels/sample.hip,
``decode.device_sampler.DeviceSampler``) follow it, the arrangement of ``ngram_blocked`` / ``hyp_score``.

Random numbers: Philox4x32-10 (Salmon et al. 2011), key (sample_seed & 0xffffffff, sample_seed >> 32),
counter (t, stream & 0xffffffff, stream >> 32, 0) with t the decode step; the uniform is output word
0, u = (x >> 8) * 2**-24 (exact in fp32, in [0, 1)).  stream = sample_base + article index in the
batch * n_samples + s: a sample's draws depend neither on decode_batch nor on what else is in the
batch.  The decode loops pass sample_base = n_samples * (articles decoded so far).

Top-k draw: the k + 1 best entries (equal values to the lower id, the select rule); while
t < min_dec_steps [STOP] is dropped from them; the first k are kept; weights w_j = exp(lp_j / temp);
the first j whose running sum exceeds u * sum(w), clamped to the last candidate if rounding overshoots.

Full draw: one inverse CDF over the vocabulary ids in ascending order, w_v = p_gen * softmax[v], then
the article positions i < enc_len in ascending order, w_{V+i} = (1 - p_gen) * a_i (token ext[i]) -- the
mixture itself, never scattered.  While t < min_dec_steps entries whose token is [STOP] weigh 0; an
entry of weight 0 is never chosen; clamped to the last positive one if rounding overshoots.

The reported step log-prob is the model's own: log(p_gen * softmax[w] * [w < V] + (1 - p_gen) *
sum over {i < enc_len, ext_i == w} of a_i), whatever the [STOP] masking and the temperature.
A sample ends when it draws [STOP], or at max_dec_steps (then without a [STOP], like a live beam).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from ..config import check_sampling, sampling_on
from ..data.vocab import START_DECODING, STOP_DECODING, UNKNOWN_TOKEN
from .beam_search import Hypothesis

_M32 = 0xFFFFFFFF
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32(counter: Sequence[int], key: Sequence[int], rounds: int = 10) -> Tuple[int, int, int, int]:
    """Philox4x32 (10 rounds) on plain Python ints: 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(rounds):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def sample_uniform(seed: int, stream: int, t: int) -> float:
    """The uniform of sample stream ``stream`` at decode step ``t``: 24 bits, exact in fp32, in [0, 1)."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    x = philox4x32((t, stream & _M32, stream >> 32, 0), (seed & _M32, seed >> 32))[0]
    return (x >> 8) * 2.0 ** -24


def _inverse_cdf(w: np.ndarray, u: float) -> int:
    """First index whose running sum of ``w`` (fp64, >= 0) exceeds u * sum(w); an entry of weight 0 is
    never chosen; the last positive one if rounding overshoots."""
    c = np.cumsum(w)
    hit = np.nonzero((c > u * c[-1]) & (w > 0))[0]
    if len(hit):
        return int(hit[0])
    pos = np.nonzero(w > 0)[0]
    if not len(pos):
        raise ValueError("nothing to draw from: every weight is 0")
    return int(pos[-1])


def draw_topk(ids, lps, k: int, temp: float, u: float, stop: int, allow_stop: bool) -> int:
    """The top-k draw over one row's candidates (best first, at least k + 1 of them unless the
    distribution has fewer): the index into ``ids`` of the drawn candidate."""
    cand = [j for j in range(min(k + 1, len(ids))) if allow_stop or int(ids[j]) != stop][:k]
    w = np.exp(np.asarray([lps[j] for j in cand], np.float64) / float(temp))
    return cand[_inverse_cdf(w, u)]


def draw_full(vocab_dist, attn, p_gen: Optional[float], ext, enc_len: int, u: float, stop: int,
              allow_stop: bool) -> Tuple[int, int]:
    """The full draw: (entry, token) with entry in [0, V) a vocabulary id and V + i article position i.
    ``p_gen`` None: no pointer, vocabulary part only."""
    vd = np.asarray(vocab_dist, np.float64)
    V = len(vd)
    if p_gen is None:
        w, toks = vd.copy(), np.arange(V)
    else:
        n = int(enc_len)
        ext = np.asarray(ext[:n], np.int64)
        w = np.concatenate([float(p_gen) * vd, (1.0 - float(p_gen)) * np.asarray(attn[:n], np.float64)])
        toks = np.concatenate([np.arange(V), ext])
    if not allow_stop:
        w[toks == stop] = 0.0
    e = _inverse_cdf(w, u)
    return e, int(toks[e])


def model_log_prob(tok: int, vocab_dist, attn, p_gen: Optional[float], ext, enc_len: int) -> float:
    """log of the model's own probability of ``tok``: generation plus every copy of it."""
    V = len(vocab_dist)
    gen = float(vocab_dist[tok]) if tok < V else 0.0
    if p_gen is None:
        return float(np.log(gen))
    n = int(enc_len)
    copy = float(np.asarray(attn[:n], np.float64)[np.asarray(ext[:n]) == tok].sum())
    return float(np.log(float(p_gen) * gen + (1.0 - float(p_gen)) * copy))


def run_sampling(model, vocab, batch, hps, sample_base: int = 0) -> List[Hypothesis]:
    """``hps.n_samples`` samples of the article in row 0 of ``batch`` over a ``StepModel``: tokens
    begin with [START], log_probs are the per-step model log-probs after a leading 0.0, attn_dists and
    p_gens as in beam search, score = avg_log_prob.  Sample s draws from stream sample_base + s."""
    check_sampling(hps)
    if not sampling_on(hps):
        raise ValueError("run_sampling needs sampling_topk >= 0")
    k, n = int(hps.sampling_topk), int(hps.n_samples)
    enc, dec_in_state = model.run_encoder(batch)
    T = batch.enc_batch.shape[1]
    start, stop, unk = vocab.word2id(START_DECODING), vocab.word2id(STOP_DECODING), vocab.word2id(UNKNOWN_TOKEN)
    V = vocab.size()
    ext, enc_len = np.asarray(batch.enc_batch_extend_vocab[0]), int(batch.enc_lens[0])
    hyps = [Hypothesis([start], [0.0], dec_in_state, [], [], np.zeros([T], np.float32)) for _ in range(n)]
    live = list(range(n))
    for t in range(hps.max_dec_steps):
        if not live:
            break
        cur = [hyps[s] for s in live]
        latest = [h.latest_token if h.latest_token < V else unk for h in cur]
        states = [h.state for h in cur]
        covs_in = [h.coverage if hps.coverage else None for h in cur]
        allow_stop = t >= hps.min_dec_steps
        if k > 0:
            ids, lps, new_states, attn, pgens, covs = model.decode_onestep(enc, latest, states, covs_in, k + 1)
        else:
            vds, new_states, attn, pgens, covs = model.decode_onestep_parts(enc, latest, states, covs_in)
        still = []
        for i, s in enumerate(live):
            u = sample_uniform(hps.sample_seed, sample_base + s, t)
            if k > 0:
                j = draw_topk(ids[i], lps[i], k, hps.sampling_temp, u, stop, allow_stop)
                tok, lp = int(ids[i][j]), float(lps[i][j])
            else:
                pg = pgens[i] if hps.pointer_gen else None
                _, tok = draw_full(vds[i], attn[i], pg, ext, enc_len, u, stop, allow_stop)
                lp = model_log_prob(tok, vds[i], attn[i], pg, ext, enc_len)
            hyps[s] = hyps[s].extend(tok, lp, new_states[i], attn[i], pgens[i], covs[i])
            if tok != stop:
                still.append(s)
        live = still
    for h in hyps:
        h.score = h.avg_log_prob
    return hyps


def best_sample(hyps: List[Hypothesis]) -> Hypothesis:
    """Sample-and-rank: the highest avg_log_prob, the lowest index among equals."""
    best = hyps[0]
    for h in hyps[1:]:
        if h.avg_log_prob > best.avg_log_prob:
            best = h
    return best
