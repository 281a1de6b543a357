"""Host beam search with the reference's exact semantics (``beam_search.py:26-173``).

Reproduced quirks:
  * all beam_size hypotheses start as copies of [START]; on step 0 only hypothesis 0 is
    expanded (``beam_search.py:127-128``);
  * each live hypothesis is extended with its top 2*beam candidates; all candidates are
    sorted by average log-prob (sum / len(tokens), len INCLUDING [START] with log-prob 0);
  * a [STOP] candidate goes to results only if steps >= min_dec_steps, otherwise it is
    discarded; collection stops at beam_size live hyps or beam_size results;
  * the loop runs while steps < max_dec_steps and len(results) < beam_size; if no result
    finished, the live hyps are used; the best by average log-prob is returned.
  * in-article OOV ids (>= vocab size) are fed back as [UNK].

Not in the reference: ``hps.block_ngram_repeat = n`` (n >= 2) blocks repeated n-grams
(``ngram_blocked``): a candidate that would complete an n-gram its hypothesis already contains
keeps its place among the hypothesis' top 2*beam candidates, but its step log-prob becomes
``BLOCKED_LP``, so it ranks behind every unblocked candidate (OpenNMT-py's block_ngram_repeat).

Also not in the reference: a length penalty and the summary coverage penalty of Gehrmann et al.
2018 (``hps.length_penalty``, ``hps.length_alpha``, ``hps.coverage_penalty_beta``; ``hyp_score``).
With them the search ranks -- at every step, for the result score and for the final pick -- by
``score(h) = log_prob / L(len(tokens)) - beta * cp(h)`` instead of the average log-prob; the
defaults (``avg``, beta 0) are the reference's rule and take the reference's path.

The step model is pluggable (``StepModel``): the PyTorch oracle on CPU, or the gfx950
decode step on GPU.  The batched device-resident version (many articles per launch,
hipGraph-captured) lives in ``decode.device_beam``, on the step trunk and batch pipeline of
``decode.device_base`` that it shares with the sampler (``decode.device_sampler``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from ..config import check_penalties
from ..data.vocab import START_DECODING, STOP_DECODING, UNKNOWN_TOKEN


@dataclass
class Hypothesis:
    tokens: List[int]
    log_probs: List[float]
    state: tuple
    attn_dists: List[np.ndarray] = field(default_factory=list)
    p_gens: List[Optional[float]] = field(default_factory=list)
    coverage: Optional[np.ndarray] = None
    score: Optional[float] = None  # the ranking score (``hyp_score``) of a returned hypothesis

    def extend(self, token, log_prob, state, attn_dist, p_gen, coverage) -> "Hypothesis":
        return Hypothesis(self.tokens + [token], self.log_probs + [log_prob], state, self.attn_dists + [attn_dist],
                          self.p_gens + [p_gen], coverage)

    @property
    def latest_token(self) -> int:
        return self.tokens[-1]

    @property
    def log_prob(self) -> float:
        return sum(self.log_probs)

    @property
    def avg_log_prob(self) -> float:
        return self.log_prob / len(self.tokens)


BLOCKED_LP = -1e20  # step log-prob of a blocked candidate (fp32: lp_sum + BLOCKED_LP == BLOCKED_LP)


def ngram_blocked(tokens, w: int, n: int) -> bool:
    """Would appending ``w`` to ``tokens`` (the hypothesis' ids as chosen, [START] first, in-article
    OOVs with their extended ids) repeat one of its n-grams?  True iff, with L = len(tokens),
    L >= n and some p in [0, L - n] has tokens[p : p+n-1] == tokens[L-n+1 :] and
    tokens[p+n-1] == w.  n <= 1 never blocks."""
    L = len(tokens)
    if n <= 1 or L < n:
        return False
    suffix = list(tokens[L - n + 1:])
    return any(tokens[p + n - 1] == w and list(tokens[p:p + n - 1]) == suffix for p in range(L - n + 1))


def sort_hyps(hyps: List[Hypothesis]) -> List[Hypothesis]:
    return sorted(hyps, key=lambda h: h.avg_log_prob, reverse=True)


def penalties_on(hps) -> bool:
    """False for the reference's rule (average log-prob, no coverage penalty)."""
    return getattr(hps, "length_penalty", "avg") != "avg" or float(getattr(hps, "coverage_penalty_beta", 0.0)) > 0


def length_norm(n: int, kind: str = "avg", alpha: float = 0.9) -> float:
    """L(n) for a hypothesis of n tokens ([START] included): ``avg`` n, ``wu`` ((5 + n) / 6) ** alpha
    (GNMT), ``none`` 1."""
    if kind == "avg":
        return float(n)
    if kind == "wu":
        return ((5.0 + n) / 6.0) ** float(alpha)
    if kind == "none":
        return 1.0
    raise ValueError(f"unknown length_penalty {kind!r}")


def inv_len_table(hps, nmax: int) -> np.ndarray:
    """1 / L(n) for n = 0 .. nmax, computed in fp64 and rounded once to fp32 (entry 0 unused): the
    table the device bookkeeping multiplies the log-prob sums with."""
    n = np.arange(nmax + 1)
    n[0] = 1
    return np.array([1.0 / length_norm(int(x), hps.length_penalty, hps.length_alpha) for x in n], np.float32)


def coverage_penalty(cov_total, enc_len: int) -> float:
    """sum over article positions i < enc_len of max(c_i - 1, 0), c = the sum of a hypothesis'
    attention distributions (OpenNMT-py's ``summary`` penalty, sum(max(cov, 1)) - src_len)."""
    c = np.asarray(cov_total, np.float64)[:int(enc_len)]
    return float(np.maximum(c - 1.0, 0.0).sum())


def hyp_score(h: Hypothesis, hps, enc_len: int) -> float:
    """The ranking score: log_prob / L(len(tokens)) - beta * cp, cp over the sum of the attention
    distributions of every step taken; plain Python floats.  (Not ``h.coverage`` plus the last
    attention: the coverage of the decode graph also holds the initial-state attention of step
    0, which is no step of the hypothesis.)"""
    s = h.log_prob / length_norm(len(h.tokens), getattr(hps, "length_penalty", "avg"),
                                 getattr(hps, "length_alpha", 0.9))
    beta = float(getattr(hps, "coverage_penalty_beta", 0.0))
    if beta > 0 and h.attn_dists:
        if not hps.coverage or h.coverage is None:
            raise ValueError("coverage_penalty_beta > 0 needs coverage=True")
        s -= beta * coverage_penalty(np.sum(np.asarray(h.attn_dists, np.float64), 0), enc_len)
    return s


def sort_by_score(hyps: List[Hypothesis]) -> List[Hypothesis]:
    return sorted(hyps, key=lambda h: h.score, reverse=True)


class OracleStepModel:
    """run_encoder / decode_onestep over ReferencePointerGenerator (model.py:347-443)."""

    def __init__(self, ref, W, hps, device="cpu"):
        self.ref, self.W, self.hps, self.device = ref, W, hps, torch.device(device)

    @torch.no_grad()
    def run_encoder(self, batch):
        enc_batch = torch.as_tensor(batch.enc_batch[:1], dtype=torch.long, device=self.device)
        lens = torch.as_tensor(batch.enc_lens[:1], dtype=torch.long, device=self.device)
        enc_out, F, (c0, h0) = self.ref.encode(self.W, enc_batch, lens)
        mask = torch.as_tensor(batch.enc_padding_mask[:1], device=self.device)
        ext = torch.as_tensor(batch.enc_batch_extend_vocab[:1], dtype=torch.long, device=self.device)
        return {"enc_out": enc_out, "F": F, "mask": mask, "ext": ext, "max_oovs": int(batch.max_art_oovs)}, \
            (c0[0], h0[0])

    def _step_inputs(self, enc, latest_tokens, states, prev_coverage):
        k = len(states)
        c = torch.stack([s[0] for s in states])
        h = torch.stack([s[1] for s in states])
        tok = torch.as_tensor(latest_tokens, dtype=torch.long, device=self.device)
        rep = lambda x: x.expand(k, *x.shape[1:])
        cov = torch.as_tensor(np.stack(prev_coverage), dtype=c.dtype, device=self.device) \
            if prev_coverage[0] is not None else None
        return k, rep, tok, c, h, cov

    @staticmethod
    def _step_outputs(k, c2, h2, a, pg, cov2):
        new_states = [(c2[i], h2[i]) for i in range(k)]
        attn = [a[i].cpu().numpy() for i in range(k)]
        pgens = [float(pg[i]) for i in range(k)] if pg is not None else [None] * k
        covs = [cov2[i].cpu().numpy() for i in range(k)] if cov2 is not None else [None] * k
        return new_states, attn, pgens, covs

    @torch.no_grad()
    def decode_onestep(self, enc, latest_tokens, states, prev_coverage, k2):
        k, rep, tok, c, h, cov = self._step_inputs(enc, latest_tokens, states, prev_coverage)
        ids, lp, c2, h2, a, pg, cov2 = self.ref.decode_onestep(
            self.W, rep(enc["enc_out"]), rep(enc["F"]), rep(enc["mask"]), rep(enc["ext"]), enc["max_oovs"], tok, c, h,
            cov, k2)
        return (ids.cpu().numpy(), lp.cpu().numpy(), *self._step_outputs(k, c2, h2, a, pg, cov2))

    @torch.no_grad()
    def decode_onestep_parts(self, enc, latest_tokens, states, prev_coverage):
        """``decode_onestep`` without the mixture and its top-k: the vocabulary softmax [k][V] in
        place of (ids, log-probs) -- the parts the full-distribution draw (decode/sampling.py) reads."""
        k, rep, tok, c, h, cov = self._step_inputs(enc, latest_tokens, states, prev_coverage)
        vd, c2, h2, a, pg, cov2 = self.ref.decode_onestep_parts(
            self.W, rep(enc["enc_out"]), rep(enc["F"]), rep(enc["mask"]), tok, c, h, cov)
        return (vd.cpu().numpy(), *self._step_outputs(k, c2, h2, a, pg, cov2))


def run_beam_search(model, vocab, batch, hps) -> Hypothesis:
    enc, dec_in_state = model.run_encoder(batch)
    T = batch.enc_batch.shape[1]
    start, stop, unk = vocab.word2id(START_DECODING), vocab.word2id(STOP_DECODING), vocab.word2id(UNKNOWN_TOKEN)
    V = vocab.size()
    hyps = [Hypothesis([start], [0.0], dec_in_state, [], [], np.zeros([T], np.float32)) for _ in range(hps.beam_size)]
    results: List[Hypothesis] = []
    steps = 0
    ngram = int(getattr(hps, "block_ngram_repeat", 0))
    pen = penalties_on(hps)
    rank = sort_by_score if pen else sort_hyps
    if pen:
        check_penalties(hps)
        enc_len = int(batch.enc_lens[0])
        for h in hyps:
            h.score = hyp_score(h, hps, enc_len)
    while steps < hps.max_dec_steps and len(results) < hps.beam_size:
        latest = [h.latest_token if h.latest_token < V else unk for h in hyps]
        ids, lps, new_states, attn, pgens, covs = model.decode_onestep(
            enc, latest, [h.state for h in hyps], [h.coverage if hps.coverage else None for h in hyps],
            2 * hps.beam_size)
        all_hyps = []
        num_orig = 1 if steps == 0 else len(hyps)
        for i in range(num_orig):
            for j in range(2 * hps.beam_size):
                tok, lp = int(ids[i, j]), float(lps[i, j])
                if ngram > 1 and ngram_blocked(hyps[i].tokens, tok, ngram):
                    lp = BLOCKED_LP
                all_hyps.append(hyps[i].extend(tok, lp, new_states[i], attn[i], pgens[i], covs[i]))
                if pen:
                    all_hyps[-1].score = hyp_score(all_hyps[-1], hps, enc_len)
        hyps = []
        for h in rank(all_hyps):
            if h.latest_token == stop:
                if steps >= hps.min_dec_steps:
                    results.append(h)
            else:
                hyps.append(h)
            if len(hyps) == hps.beam_size or len(results) == hps.beam_size:
                break
        steps += 1
    if not results:
        results = hyps
    best = rank(results)[0]
    if best.score is None:  # the reference's rule, or no step taken
        best.score = best.avg_log_prob
    return best
