"""Decode by sampling on the device: ``DeviceSampler``, the sibling of ``decode.device_beam``'s beam
search on the shared ``decode.device_base.DeviceDecoder`` (``decode.sampling`` holds the rule)."""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from ..config import check_sampling, sampling_on
from ..data.vocab import START_DECODING, STOP_DECODING
from ..models.pointer_generator import OV
from .beam_search import Hypothesis
from .device_base import F32, DeviceDecoder
from .sampling import best_sample


class DeviceSampler(DeviceDecoder):
    """``n_articles x n_samples`` rows, every row an independent sample of its article with its own
    Philox stream (``self.beam`` holds ``n_samples``: the rows per article of the shared trunk).

    The decode step is the base's unfused one up to the candidate lists and ends in ``sample_topk``
    (k in 1..31, behind the vocab head with k + 1 candidates) or, for k = 0, in ``sample_full`` behind
    the materialised head (library GEMM into the logits buffer, ``pgen``).  The draw kernels' tail
    keeps the samples' books (token / log-prob histories, done flag and length per row), so early
    exit, graph capture in chunks, the snapshot pipelining and the LSTM error check are the base's.

    ``sample(batch, sample_base)`` returns every sample; ``decode`` / ``decode_batches`` yield
    ``best_sample`` per article and count the articles decoded so far for the stream ids."""

    _rows_flag = "n_samples"
    _fused_tail = False  # the draw is the tail of the unfused step

    def __init__(self, hps, vocab, params, n_articles: int, T: int, use_graph: bool = True, chunk: int = 10,
                 keep_attn: bool = True, group_enc: int = None):
        check_sampling(hps)
        if not sampling_on(hps):
            raise ValueError("DeviceSampler needs sampling_topk >= 0 (DeviceBeamDecoder runs beam search)")
        self.topk, self.n_samples = int(hps.sampling_topk), int(hps.n_samples)
        self.articles_seen = 0  # decode / decode_batches: sample_base = n_samples * articles decoded so far
        super().__init__(hps, vocab, params, n_articles, T, use_graph=use_graph, chunk=chunk, keep_attn=keep_attn,
                         group_enc=group_enc)

    # ------------------------------------------------------------------ the plan
    def _candidates(self) -> int:
        # the smallest list the selects take that holds the k + 1 best (k = 0 reads no list)
        return self.topk + 1 if self.topk > 0 else 2

    def _fused_vocab_ok(self) -> bool:
        # the fused vocab head at every k > 0: its select takes the 32-entry lists above 8 candidates
        # at any number of rows per article; sample_full (k = 0) reads materialised logits and p_gen
        return self.topk > 0

    # ------------------------------------------------------------------ books
    def _alloc_books(self):
        R, D, b, z = self.R, self.maxD, self.b, self._zeros
        b["done"] = z(R, dt=torch.int32)  # per sample
        b["lp_hist"], b["slen"] = z(D, R), z(R, dt=torch.int32)
        b["streams"] = z(R, dt=torch.long)  # refilled per batch
        b["s_tok"], b["s_lp"], b["s_pick"] = z(R, dt=torch.int32), z(R), z(R, dt=torch.int32)

    def _reset_books(self):
        for n in ("done", "step", "tok_hist", "lp_hist", "slen", "tail_err"):
            self.b[n].zero_()  # (tail_err: the draw's "nothing to draw from" word)

    @staticmethod
    def _check_tail(err: int) -> None:
        if err:
            raise RuntimeError("sampling decode: a row had nothing to draw from (every weight of its distribution "
                               "was 0 or not a number); results discarded")

    # ------------------------------------------------------------------ the end of the step
    def _select(self, Y, pg):
        if self.topk > 0:
            return super()._select(Y, pg)
        torch.mm(self.b["outb"], self.eng.pk["ow"], out_dtype=F32, out=self.b["logits"])

    def _book(self, Y, pg):
        k, b, hps = self.k, self.b, self.hps
        hist = self.keep_attn
        seed = hps.sample_seed - (1 << 64) if hps.sample_seed >= (1 << 63) else hps.sample_seed  # as int64
        stop = self.vocab.word2id(STOP_DECODING)
        book = (b["done"], b["tok_hist"], b["lp_hist"], b["lp_sum"], b["latest"], b["slen"],
                Y["ATT"] if hist else None, b["ATT_hist"] if hist else None,
                pg if (hist and pg is not None) else None, b["PG_hist"] if (hist and pg is not None) else None)
        if self.topk > 0:
            k.sample_topk(b["top_ids"], b["top_lp"], b["streams"], b["step"], seed, b["s_tok"], b["s_lp"], b["s_pick"],
                          self.R, self.K, self.topk, float(hps.sampling_temp), stop, hps.min_dec_steps, self.maxD,
                          self.T, *book)
        else:
            k.sample_full(b["logits"], self.p[OV], pg, Y["ATT"] if pg is not None else None, b["ext"], b["lens"],
                          b["streams"], b["step"], seed, b["s_tok"], b["s_lp"], b["s_pick"], self.R, self.V, self.T,
                          self.beam, stop, hps.min_dec_steps, self.maxD, *book, b["tail_err"])

    # ------------------------------------------------------------------ driver
    def set_streams(self, sample_base) -> None:
        """Row r = article a, sample s draws from stream sample_base + a * n_samples + s; a sequence
        gives every article its own base (stream sample_base[a] + s)."""
        n = self.n_samples
        if isinstance(sample_base, (int, np.integer)):  # filled on the device: no host copy in the decode loops
            torch.arange(int(sample_base), int(sample_base) + self.R, dtype=torch.long, device=self.dev,
                         out=self.b["streams"])
            return
        ids = np.repeat(np.asarray(sample_base, np.int64), n) + np.tile(np.arange(n, dtype=np.int64), self.Na)
        if ids.shape != (self.R,):
            raise ValueError(f"sample_base: one base per article ({self.Na}) expected")
        self.b["streams"].copy_(torch.from_numpy(ids))

    def run_chunks(self, batch, pre_encoded: bool = False, next_batch=None, enc_src=None, sample_base=None):
        base = self.n_samples * self.articles_seen if sample_base is None else sample_base
        if sample_base is None:
            self.articles_seen += self._n_valid(batch)
        self.set_streams(base)
        yield from super().run_chunks(batch, pre_encoded=pre_encoded, next_batch=next_batch, enc_src=enc_src)

    def _result_names(self):
        return ["tok_hist", "lp_hist", "slen"] + (["ATT_hist", "PG_hist"] if self.keep_attn else [])

    def _samples(self, b, n_valid: int = None) -> List[List[Hypothesis]]:
        n, start = self.n_samples, self.vocab.word2id(START_DECODING)
        out = []
        for a in range(n_valid if n_valid is not None else self.Na):
            hyps = []
            for r in range(a * n, (a + 1) * n):
                L = int(b["slen"][r])
                tokens = [start] + b["tok_hist"][:L, r].tolist()
                lps = [0.0] + [float(x) for x in b["lp_hist"][:L, r]]
                atts, pgs = [], []
                if self.keep_attn:  # copies: b's arrays are views of pinned buffers that the next batch reuses
                    atts = [b["ATT_hist"][t, r].copy() for t in range(L)]
                    pgs = [float(b["PG_hist"][t, r]) if self.hps.pointer_gen else None for t in range(L)]
                h = Hypothesis(tokens, lps, None, atts, pgs, None)
                h.score = h.avg_log_prob
                hyps.append(h)
            out.append(hyps)
        return out

    def _hyps(self, b, n_valid: int = None) -> List[Hypothesis]:
        return [best_sample(hyps) for hyps in self._samples(b, n_valid)]

    def sample(self, batch, sample_base: int = 0) -> List[List[Hypothesis]]:
        """Every sample of every valid article of ``batch``: ``n_samples`` hypotheses each."""
        self._rows_ok(batch)
        for _ in self.run_chunks(batch, sample_base=sample_base):
            pass
        out = self._samples(self._fetch(self._result_names()), self._n_valid(batch))  # synchronises
        self.eng.check_lstm_err()
        self._check_tail(int(self.b["tail_err"].item()))
        return out
