"""Batched, device-resident beam search on MI355X (SURVEY PAR3, K17/K20/K25/K26, 7.5-3).

The reference decodes ONE article at a time with beam_size rows and a host round trip per
step (``beam_search.py:82-168``, one ``sess.run`` + numpy state packing per step).  Here
``n_articles x beam`` rows decode together and the whole step stays on the GPU:

  gather-by-parent (c, h, ctx*, a*, cov)  ->  cov' = cov + a*  ->  XG / x from per-token
  tables  ->  dec_cell_fwd  ->  dec_sproj  ->  attn_score / attn_softmax_ctx  ->  p_gen,
  output projection, vocab GEMM  ->  final_topk (pointer mixture + top-2k)  ->  beam_step

The step reads its index t from a device counter and the decoder state ping-pongs between
two buffer sets, so ONE captured hipGraph of two steps
is replayed up to max_dec_steps times (host checks the all-done flag every ``chunk``
replays, the only host sync).

The reference's decode-mode attention runs twice per step (initial_state_attention):
the first attention of step t recomputes attention(state_{t-1}, cov'_{t-1}), which is
exactly the parent's post-cell attention of step t-1 -- same inputs -- so it is gathered
instead of recomputed (only step 0 runs it, in the prologue).  Coverage semantics are
unchanged: cov'_t = cov'_{t-1}[parent] + a_{t-1}[parent].

Three modules: ``decode.device_base.DeviceDecoder`` holds what does not depend on how a step ends
(encoder hand-over, the step trunk up to the candidate lists, the plan of which step variant runs,
graph capture, the chunked early exit and the pipelined ``decode_batches``); ``DeviceBeamDecoder``
here adds the beam search (its books, the fused step, the four bookkeeping variants, backtracking);
``decode.device_sampler.DeviceSampler`` is its sibling that ends the step in a draw.  This module
stays the import home of all three names and of ``device_decoder``.
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from ..config import check_penalties, sampling_on
from ..data.vocab import START_DECODING, STOP_DECODING, UNKNOWN_TOKEN
from ..models.pointer_generator import ATT_B, OUT_B, OV, PG_B
from .beam_search import Hypothesis, inv_len_table, penalties_on
from .device_base import DeviceDecoder
from .device_sampler import DeviceSampler  # noqa: F401  (re-exported)


class DeviceBeamDecoder(DeviceDecoder):
    pen = None  # length / coverage penalties off unless __init__ finds them in hps
    _rows_flag = "beam_size"
    _fused_tail = True

    def __init__(self, hps, vocab, params, n_articles: int, T: int, use_graph: bool = True, chunk: int = 10,
                 keep_attn: bool = True, wide_beam: bool = False):
        """``wide_beam``: run the wide-beam step on materialised logits (library GEMM, final_topk with
        the 32-entry list, workgroup-wide bookkeeping) at any beam size (a test switch: the narrow
        kernels are the faster ones where they apply).  Beam sizes above 5 always take the wide
        bookkeeping, by default behind the fused vocab head."""
        self.wide_switch = bool(wide_beam)
        # n-gram blocking (hps.block_ngram_repeat, semantics of beam_search.ngram_blocked) in the
        # beam bookkeeping of both step variants; 0 = off (the kernels without it)
        n = int(getattr(hps, "block_ngram_repeat", 0))
        if n < 0:
            raise ValueError("block_ngram_repeat must be >= 0")
        self.ngram = n if n > 1 else 0
        # length / coverage penalties (beam_search.hyp_score) in the bookkeeping of both step variants:
        # None = the reference's rule, the kernels and buffers without them
        check_penalties(hps)
        self.pen = {"beta": float(hps.coverage_penalty_beta)} if penalties_on(hps) else None
        super().__init__(hps, vocab, params, n_articles, T, use_graph=use_graph, chunk=chunk, keep_attn=keep_attn)

    # ------------------------------------------------------------------ the plan
    def _candidates(self) -> int:
        return 2 * self.beam

    def _fused_vocab_ok(self) -> bool:
        # Beams 6 to 16 (wide by their size) take it too, with the select's 32-entry lists, in front
        # of beam_step_wide; ``wide_beam=True`` (the test switch) keeps the materialised step at
        # every beam size.  On by default for all of 6..16: bench_decode.py, 64 articles, V = 50k,
        # three alternated runs each, materialised -> fused summaries/s: beam 8 2348 -> 3587,
        # beam 10 1802 -> 2588, beam 16 915 -> 1694; with blocking and both penalties 2245 -> 3364,
        # 1749 -> 2481, 902 -> 1646; run-to-run spread under 1.5 % (profiles/wide_beam_fused.md).
        return self.K <= 32 and not self.wide_switch if self.wide else self.K <= 8

    # ------------------------------------------------------------------ books
    def _alloc_books(self):
        R, K, Na, D, b, z = self.R, self.K, self.Na, self.maxD, self.b, self._zeros
        i32 = torch.int32
        b["par_hist"], b["done"], b["res_count"] = z(D, R, dt=i32), z(Na, dt=i32), z(Na, dt=i32)
        b["res_score"], b["res_len"], b["res_step"], b["res_par"] = z(R), z(R, dt=i32), z(R, dt=i32), z(R, dt=i32)
        b["step_ctr"], b["art_ctr"] = z(1, dt=i32), z(Na, dt=i32)
        b["gran"] = z(R, K, dt=torch.long)  # tagged candidate granules of the fused beam tail
        # n-gram blocking: the hypotheses' token sequences, ping-pong like the decoder state --
        # step t reads seq[t & 1][r][0..t] ([START] first) and writes seq[(t + 1) & 1] (the kernels
        # take the parity from the device step counter, so a captured graph needs none)
        self.seq = None
        if self.ngram:
            P = (D + 1 + 3) // 4 * 4
            if self.beam * P > 4096:
                raise ValueError(f"block_ngram_repeat: beam_size * (max_dec_steps + 1) = {self.beam * (D + 1)} "
                                 "exceeds the 4096 tokens per article the beam kernels hold")
            self.seq = [z(R, P, dt=torch.int32) for _ in range(2)]
        # penalties: the rank key of every live hypothesis and the raw sum of every result (res_score
        # then holds the key), 1 / L(n) per length, this step's coverage penalty per row (beta > 0)
        if self.pen is not None:
            b["key_sum"], b["res_lp"] = z(R), z(R)
            b["inv_len"] = torch.from_numpy(inv_len_table(self.hps, D + 1)).to(self.dev)
            if self.pen["beta"] > 0:
                # (att0: the step-0 initial-state attention per article, which the coverage holds
                # but which is no step of a hypothesis)
                b["cpen"], b["att0"] = z(R), z(Na, self.T)

    def _reset_books(self):
        b = self.b
        for n in ("done", "res_count", "step", "step_ctr", "tok_hist", "par_hist", "res_len", "res_step", "res_par",
                  "art_ctr", "gran"):
            b[n].zero_()
        b["res_score"].fill_(-float("inf"))
        if self.pen is not None:
            b["key_sum"].zero_()
            b["res_lp"].fill_(-float("inf"))
            if "cpen" in b:
                b["cpen"].zero_()
                b["att0"].copy_(self.st[0]["ATT"][::self.beam])
        if self.seq is not None:
            self.seq[0].zero_()
            self.seq[0][:, 0] = self.vocab.word2id(START_DECODING)

    def _state(self):
        """The beam-state tensors every bookkeeping variant takes, in the order the ops take them."""
        b = self.b
        return (b["top_ids"], b["top_lp"], b["lp_sum"], b["latest"], b["gidx"], b["tok_hist"], b["par_hist"],
                b["done"], b["res_count"], b["res_score"], b["res_len"], b["res_step"], b["res_par"], b["step"])

    # ------------------------------------------------------------------ the end of the step
    def _book(self, Y, pg):
        """Beam bookkeeping of the unfused step; also appends a_t / p_gen to the histories
        (b["step"] was advanced by this step's beam_gather: no grid-wide counter here)."""
        k, b, hps = self.k, self.b, self.hps
        T, K = self.T, self.K
        hist = self.keep_attn
        self._cov_penalty(Y)
        args = (*self._state(), None, Y["ATT"] if hist else None, b["ATT_hist"] if hist else None,
                pg if (hist and pg is not None) else None, b["PG_hist"] if (hist and pg is not None) else None,
                T, self.Na, self.beam, K, self.vocab.word2id(STOP_DECODING), hps.min_dec_steps, self.maxD)
        if self.wide:
            seq = self.seq if self.ngram else (None, None)
            pen = self._pen_args()[3:] if self.pen is not None else (None, None, 0.0, None, None)
            k.beam_step_wide(*args[:14], *args[15:], seq[0], seq[1], self.ngram, *pen)  # (args[14]: no ctr)
        elif self.pen is not None:
            k.beam_step_pen(*args, *self._pen_args())
        elif self.ngram:
            k.beam_step_ng(*args, self.seq[0], self.seq[1], self.ngram)
        else:
            k.beam_step(*args)

    def _cov_penalty(self, Y):
        """This step's coverage penalty per row from the coverage before the step and its attention
        (after the attention, before the bookkeeping; only with beta > 0: ``cpen`` exists only then)."""
        if "cpen" in self.b:
            self.k.cov_penalty(Y["COV"], Y["ATT"], self.b["lens"], self.b["cpen"], self.R, self.T, self.beam,
                               self.b["att0"])

    def _pen_args(self):
        b = self.b
        seq = self.seq if self.ngram else (None, None)
        return (seq[0], seq[1], self.ngram, b["inv_len"], b.get("cpen"), self.pen["beta"], b["key_sum"], b["res_lp"])

    def _step_fused(self, parity: int):
        """One decode step in 6 launches (reference model.py:367-443 decode_onestep + the beam
        update of beam_search.py:110-156): cell with the parent / token gathers (and the step
        counter), attention query + x-merge, row attention with the coverage gather, output
        projection, vocab logits, vocab select + p_gen + per-article beam bookkeeping."""
        k, b, hps, eng, p = self.k, self.b, self.hps, self.eng, self.p
        R, T, H, A, E, V, K = self.R, self.T, eng.H, eng.A, eng.E, self.V, self.K
        X, Y = self.st[parity], self.st[1 - parity]
        cov = hps.coverage
        unk = self.vocab.word2id(UNKNOWN_TOKEN)
        k.dec_cell_fwd_beam(b["gidx"], b["latest"], self.XGtab, X["CTXb"], X["H"], X["C"], eng.pk["WcT2"], Y["C"],
                            b["Cb2"], Y["H"], b["step"], R, H, A, V, unk)
        if hps.pointer_gen:
            k.beam_sproj_xmerge(b["Cb2"], Y["H"], eng.pk["WsT"], p[ATT_B], b["s"], X["CTXb"], eng.pk["WicT"],
                                self.Xtab, b["gidx"], b["latest"], b["x"], R, H, A, E, V, unk)
        else:
            k.dec_sproj(b["Cb2"], Y["H"], eng.pk["WsT"], p[ATT_B], b["s"], R, H, A, None, 0)
        k.attn_fwd_row_beam(b["F"], b["E"], b["s"], eng.f32["v"], eng.f32["wc"], X["COV"] if cov else None,
                            X["ATT"] if cov else None, Y["COV"] if cov else None, b["gidx"], b["lens_att"],
                            Y["ATT"], Y["CTX"], Y["CTXb"], R, T, A, self.rep)
        self._cov_penalty(Y)
        k.linear2(Y["H"], H, Y["CTXb"], A, eng.pk["OUTmT"], p[OUT_B], None, None, b["outb"], R, H)
        ptr, hist, st = hps.pointer_gen, self.keep_attn, self._state()
        args = (b["outb"], self.owT, p[OV], Y["CTX"] if ptr else None, Y["C"] if ptr else None,
                Y["H"] if ptr else None, b["x"] if ptr else None, self.pg_w if ptr else None,
                p[PG_B] if ptr else None, b["PG"] if ptr else None, Y["ATT"] if (ptr or hist) else None,
                b["ext"], b["lens"], *st[:2], b["logits"], b["vpart_ms"], *st[2:], b["art_ctr"], b["gran"],
                b["tail_err"],
                b["ATT_hist"] if hist else None, b["PG_hist"] if (hist and ptr) else None, R, V, H, T, K,
                self.beam, A, E, self.vocab.word2id(STOP_DECODING), hps.min_dec_steps, self.maxD)
        if self.pen is not None:
            k.vocab_topk_beam_pen(*args, *self._pen_args())
        elif self.ngram:
            k.vocab_topk_beam_ng(*args, self.seq[0], self.seq[1], self.ngram)
        else:
            k.vocab_topk_beam(*args)

    @staticmethod
    def _check_tail(err: int) -> None:
        if err:
            raise RuntimeError("beam decode: a fused beam-tail poll timed out (candidates of an article never "
                               "arrived); results discarded -- set TSAMD_DEC_ROW_ATTN=0 for the unfused step")

    def _result_names(self):
        names = ["res_count", "res_score", "res_step", "res_par", "lp_sum", "tok_hist", "par_hist", "step"]
        names += ["key_sum", "res_lp"] if self.pen is not None else []
        return names + (["ATT_hist", "PG_hist"] if self.keep_attn else [])

    def _backtrack(self, b, n_valid: int = None) -> List[Hypothesis]:
        """Best hypothesis per article (host).  The winner is picked from the device scores
        first and only the winners are backtracked, vectorised over articles (one numpy
        gather per step instead of a Python walk per candidate)."""
        beam, start, stop = self.beam, self.vocab.word2id(START_DECODING), self.vocab.word2id(STOP_DECODING)
        nsteps = int(min(b["step"][0], self.maxD))
        na = n_valid if n_valid is not None else self.Na
        ar = np.arange(na)
        base = ar * beam
        nres = b["res_count"][:na].astype(np.int64)
        fin = nres > 0
        # winners: the finished hypotheses by final score, else the live beams by average
        # log-prob including [START]; argmax keeps the first of equal maxima, as the stable
        # sort of sort_hyps does
        rs = b["res_score"][:na * beam].reshape(na, beam).astype(np.float64)
        rs = np.where(np.arange(beam)[None, :] < nres[:, None], rs, -np.inf)
        q_fin = rs.argmax(1) if na else np.zeros(0, np.int64)
        lps = b["lp_sum"][:na * beam].reshape(na, beam).astype(np.float64)
        pen = self.pen is not None
        # (penalties: res_score and key_sum hold the rank keys, res_lp and lp_sum the raw sums)
        live = b["key_sum"][:na * beam].reshape(na, beam).astype(np.float64) if pen else lps / (nsteps + 1)
        q_live = live.argmax(1) if na else np.zeros(0, np.int64)
        score = np.where(fin, rs[ar, q_fin], live[ar, q_live])
        if pen:
            lp_tot = np.where(fin, b["res_lp"][base + q_fin].astype(np.float64), lps[ar, q_live])
        t_fin = b["res_step"][base + q_fin].astype(np.int64)
        tl0 = np.where(fin, t_fin - 1, nsteps - 1)
        slot = np.where(fin, b["res_par"][base + q_fin], q_live).astype(np.int64)
        L = int(tl0.max()) + 1 if na else 0
        toks = np.zeros((na, max(L, 1)), dtype=np.int64)
        arow = np.zeros((na, max(L, 1)), dtype=np.int64)  # attention / p_gen history rows (base + parent)
        for tl in range(L - 1, -1, -1):
            act = tl <= tl0
            rows = base + slot
            par = b["par_hist"][tl, rows].astype(np.int64)
            toks[act, tl] = b["tok_hist"][tl, rows][act]
            arow[act, tl] = (base + par)[act]
            slot = np.where(act, par, slot)
        out = []
        for a in range(na):
            n = int(tl0[a]) + 1
            tokens = [start] + toks[a, :n].tolist() + ([stop] if fin[a] else [])
            atts, pgs = [], []
            if self.keep_attn:
                # copies: b's arrays are views of pinned buffers that the next batch reuses
                atts = [b["ATT_hist"][tl, arow[a, tl]].copy() for tl in range(n)]
                pgs = [float(b["PG_hist"][tl, arow[a, tl]]) if self.hps.pointer_gen else None for tl in range(n)]
                if fin[a]:
                    t, par = int(t_fin[a]), int(b["res_par"][base[a] + q_fin[a]])
                    atts.append(b["ATT_hist"][t, base[a] + par].copy())
                    pgs.append(float(b["PG_hist"][t, base[a] + par]) if self.hps.pointer_gen else None)
            sc = float(score[a])
            lp = float(lp_tot[a]) if pen else sc * len(tokens)
            out.append(Hypothesis(tokens, [lp] + [0.0] * (len(tokens) - 1), None, atts, pgs, None, sc))
        return out

    def _results_walk(self, n_valid: int = None) -> List[Hypothesis]:
        """Per-candidate Python walk (the original form of ``results``; kept as the test oracle)."""
        b = {k: v.cpu().numpy() for k, v in self.b.items() if k in (
            "res_count", "res_score", "res_len", "res_step", "res_par", "lp_sum", "tok_hist", "par_hist", "step",
            "ATT_hist", "PG_hist", "done", "key_sum", "res_lp")}
        pen = self.pen is not None
        beam, start, stop = self.beam, self.vocab.word2id(START_DECODING), self.vocab.word2id(STOP_DECODING)
        nsteps = int(min(b["step"][0], self.maxD))
        out = []
        for a in range(n_valid if n_valid is not None else self.Na):
            base = a * beam

            def path(tl, slot):
                toks, atts, pgs = [], [], []
                while tl >= 0:
                    toks.append(int(b["tok_hist"][tl, base + slot]))
                    par = int(b["par_hist"][tl, base + slot])
                    if self.keep_attn:
                        atts.append(b["ATT_hist"][tl, base + par])
                        pgs.append(float(b["PG_hist"][tl, base + par]) if self.hps.pointer_gen else None)
                    slot = par
                    tl -= 1
                return toks[::-1], atts[::-1], pgs[::-1]

            cands = []
            nres = int(b["res_count"][a])
            if nres > 0:
                for q in range(nres):
                    t, par = int(b["res_step"][base + q]), int(b["res_par"][base + q])
                    toks, atts, pgs = path(t - 1, par)
                    if self.keep_attn:
                        atts = atts + [b["ATT_hist"][t, base + par]]
                        pgs = pgs + [float(b["PG_hist"][t, base + par]) if self.hps.pointer_gen else None]
                    cands.append((float(b["res_score"][base + q]), [start] + toks + [stop], atts, pgs,
                                  float(b["res_lp"][base + q]) if pen else None))
            else:
                tl = nsteps - 1
                for slot in range(beam):
                    toks, atts, pgs = path(tl, slot)
                    lp = float(b["lp_sum"][base + slot])
                    cands.append((float(b["key_sum"][base + slot]) if pen else lp / (tl + 2), [start] + toks, atts,
                                  pgs, lp))
            best = sorted(cands, key=lambda c: c[0], reverse=True)[0]  # stable, like sort_hyps
            h = Hypothesis(best[1], [best[4] if pen else best[0] * len(best[1])] + [0.0] * (len(best[1]) - 1), None,
                           list(best[2]), list(best[3]), None, best[0])
            out.append(h)
        return out

    _hyps = _backtrack


def device_decoder(hps, vocab, params, n_articles: int, T: int, **kw):
    """The device decoder ``hps`` asks for: ``DeviceSampler`` with sampling on, else ``DeviceBeamDecoder``."""
    cls = DeviceSampler if sampling_on(hps) else DeviceBeamDecoder
    return cls(hps, vocab, params, n_articles=n_articles, T=T, **kw)
