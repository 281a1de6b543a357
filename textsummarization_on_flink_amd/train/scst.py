"""Self-critical fine-tuning (Paulus et al. 2017; Rennie et al. 2017): the rule on the host, and
``ScstTrainer``, which ties the device sampler, the ROUGE reward kernel and the training step together.

The objective, with gamma = ``hps.rl_weight`` and a batch of n articles:

    L = (1 - gamma) * mean_a NLL_avg(gold_a) + gamma * mean_a (r(sample_a) - r(greedy_a)) * NLL_avg(sample_a)

``NLL_avg`` is the per-row length-averaged negative log-likelihood the engine computes for every row (the
RL term is length-normalised like the ML term, so gamma mixes like with like); r is ``hps.rl_reward`` of
the sequence against the gold summary.  A sample that beats the greedy baseline has its likelihood
raised, one that loses has it lowered.  The rewards are constants: no gradient flows through them or
through the greedy pass.  The coverage loss applies to the gold rows only.

The step trains a batch of 2n rows -- rows [0, n) the articles with their gold summaries, rows [n, 2n)
the same articles with the sample as the summary (``scst_batch``) -- with per-row multipliers
(``scst_row_scale``) that turn the engine's mean over 2n rows into L; they travel through
``models.host_inputs.host_inputs(row_scale=, cov_scale=)``, so no training kernel changes.

The first half of this module is pure numpy / Python and imports without a GPU: ``rouge_ids`` /
``rouge_f`` / ``reward`` define what ``csrc/kernels/rouge.hip`` computes, the way ``decode.sampling``
defines the draws.
"""
from __future__ import annotations

from collections import Counter
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from ..config import RL_REWARDS, check_scst
from ..data.vocab import SPECIALS, START_DECODING, STOP_DECODING, UNKNOWN_TOKEN

STOP_ID = SPECIALS.index(STOP_DECODING)  # the specials lead every vocabulary
ROUGE_MAX_LEN = 256                       # the reward kernel's limit on either sequence
F32 = np.float32


# ====================================================================== the rule
def _cut(seq, stop_id: int):
    out = []
    for x in seq:
        x = int(x)
        if x == stop_id:
            break
        out.append(x)
    return out


def _lcs_len(a, b) -> int:
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def rouge_ids(hyp: Sequence[int], ref: Sequence[int], stop_id: int = STOP_ID) -> Tuple[int, int, int, int, int]:
    """(hit1, hit2, lcs, n_hyp, n_ref) of two token-id sequences, both cut before their first [STOP]:
    clipped unigram / bigram overlap (``decode.rouge.rouge_n``) and the sequence-level LCS length.  Ids are
    compared as they are: an in-article OOV carries its extended id on both sides (``target_batch`` and
    the sampler's tokens share the article's OOV map), an abstract-only OOV is [UNK] on both."""
    h, r = _cut(hyp, stop_id), _cut(ref, stop_id)
    hits = []
    for n in (1, 2):
        ch = Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
        cr = Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        hits.append(sum(min(c, ch[g]) for g, c in cr.items()))
    return hits[0], hits[1], _lcs_len(h, r), len(h), len(r)


def rouge_f(hit, n_hyp, n_ref) -> np.float32:
    """F (alpha = 0.5) in float32, in this order: p = hit / n_hyp, r = hit / n_ref, f = 2 * p * r / (p + r);
    exactly 0 when hit == 0 (which covers an empty side)."""
    if hit <= 0:
        return F32(0.0)
    p, r = F32(hit) / F32(n_hyp), F32(hit) / F32(n_ref)
    return F32(F32(2.0) * p * r / (p + r))


def reward_from_counts(counts: Sequence[int], kind: str = "rouge_l") -> np.float32:
    """The reward ``kind`` of one (hit1, hit2, lcs, n_hyp, n_ref): a sequence of n tokens has
    max(n - 1, 0) bigrams, so ROUGE-2 of a sequence shorter than 2 is 0; rouge_mean = (f1 + f2 + fl) / 3."""
    if kind not in RL_REWARDS:
        raise ValueError(f"rl_reward must be one of {'/'.join(RL_REWARDS)}")
    hit1, hit2, lcs, nh, nr = (int(x) for x in counts)
    f1 = rouge_f(hit1, nh, nr)
    f2 = rouge_f(hit2, max(nh - 1, 0), max(nr - 1, 0))
    fl = rouge_f(lcs, nh, nr)
    if kind == "rouge_mean":
        return F32((f1 + f2 + fl) / F32(3.0))
    return {"rouge_l": fl, "rouge_1": f1, "rouge_2": f2}[kind]


def reward(hyp: Sequence[int], ref: Sequence[int], kind: str = "rouge_l", stop_id: int = STOP_ID) -> np.float32:
    return reward_from_counts(rouge_ids(hyp, ref, stop_id), kind)


def scst_row_scale(adv, gamma: float, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(row_scale, cov_scale), [2n] float64 each: the per-row multipliers that turn the engine's mean
    over 2n rows into the objective -- gold rows 2 (1 - gamma), sample rows 2 gamma (r_sample - r_greedy);
    coverage 2 (1 - gamma) on gold rows and 0 on sample rows.  ``adv`` [n] = r_sample - r_greedy."""
    adv = np.asarray(adv, dtype=np.float64)
    if adv.shape != (n,):
        raise ValueError(f"{n} advantages expected")
    if not 0.0 <= gamma <= 1.0:
        raise ValueError("rl_weight must be in [0, 1]")
    gold = np.full(n, 2.0 * (1.0 - gamma))
    return np.concatenate([gold, 2.0 * gamma * adv]), np.concatenate([gold, np.zeros(n)])


class ScstBatch:
    """The 2n-row training batch of ``scst_batch``: the arrays the engine's host inputs read."""

    def num_tokens(self) -> int:
        v = self.valid > 0
        return int(self.enc_lens[v].sum() + self.dec_padding_mask[v].sum())


def scst_batch(batch, sample_tokens, sample_lens, vocab):
    """(batch2, row_kind): rows [0, n) of ``batch2`` are ``batch``'s articles with their gold summaries,
    rows [n, 2n) the same articles with the sample as the summary; ``row_kind`` [2n] is 0 / 1.

    ``sample_tokens`` [n][D'] (ids in the article's extended vocabulary, as drawn), ``sample_lens`` [n].
    A sample row's decoder input is [START] + its tokens with ids >= V mapped to [UNK]; its target is the
    tokens as drawn ([STOP] included if one was drawn; none if it ran into max_dec_steps); its mask is 1
    for t < sample_len."""
    toks = np.asarray(sample_tokens)
    lens = np.asarray(sample_lens).astype(np.int64)
    n, D = batch.dec_batch.shape
    if toks.ndim != 2 or toks.shape[0] != n or lens.shape != (n,):
        raise ValueError(f"{n} samples expected")
    if lens.min() < 0 or lens.max() > min(D, toks.shape[1]):
        raise ValueError("sample length out of range")
    V = vocab.size()
    pad, start, unk = batch.pad_id if hasattr(batch, "pad_id") else 1, vocab.word2id(START_DECODING), \
        vocab.word2id(UNKNOWN_TOKEN)
    live = np.arange(D)[None, :] < lens[:, None]  # [n][D]
    tk = np.full((n, D), pad, dtype=np.int32)
    w = min(D, toks.shape[1])
    tk[:, :w] = toks[:, :w]
    target = np.where(live, tk, pad).astype(np.int32)
    inp = np.full((n, D), pad, dtype=np.int32)
    inp[:, 0] = start
    inp[:, 1:] = np.where(tk[:, :-1] >= V, unk, tk[:, :-1])
    inp = np.where(live, inp, pad).astype(np.int32)
    b2 = ScstBatch()
    for name in ("enc_batch", "enc_lens", "enc_padding_mask", "enc_batch_extend_vocab", "valid"):
        x = getattr(batch, name)
        setattr(b2, name, np.concatenate([x, x], 0))
    b2.dec_batch = np.concatenate([batch.dec_batch, inp], 0)
    b2.target_batch = np.concatenate([batch.target_batch, target], 0)
    b2.dec_padding_mask = np.concatenate([batch.dec_padding_mask, live.astype(batch.dec_padding_mask.dtype)], 0)
    b2.dec_lens = b2.dec_padding_mask.sum(1).astype(np.int32)
    b2.max_art_oovs = int(getattr(batch, "max_art_oovs", 0))
    b2.pad_id = pad
    return b2, np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)])


# ====================================================================== the trainer
class ScstTrainer:
    """A ``GraphTrainer`` of B = 2n rows and two ``DeviceSampler``s of n articles (one row per article):
    the greedy baseline (``sampling_topk = 1``) and the run's sampler (``hps.sampling_topk``; the default -1
    means 0 here, the model's own distribution; with a top-k value the samples come from the truncated
    policy while the log-probs are the model's).  All three read the trainer's ``FlatParams``; the
    samplers' bf16 packs and per-token tables are refreshed in place after every optimizer step.

    ``step(batch)`` (``batch``: n articles): the two sampler passes, ``rouge_reward`` for both against
    ``batch.target_batch`` on the device, the advantage, one copy of tokens / lengths / rewards to the
    host, ``scst_batch`` + ``scst_row_scale`` there (the embedding-gradient order is a host computation
    anyway), then ``GraphTrainer.step(batch2, row_scale=, cov_scale=)``.  Article a of global step s draws
    from Philox stream s * n + a keyed by ``hps.sample_seed``: a run is reproducible and a resumed run
    continues the sequence.  Returns the trainer's outputs plus ``rl_reward_sample`` / ``rl_reward_greedy``
    (batch means) and ``rl_advantage_abs``."""

    def __init__(self, hps, vocab, T: Optional[int] = None, device="cuda", info=None, params=None,
                 use_graph: Optional[bool] = None):
        import torch

        from ..decode.device_sampler import DeviceSampler
        from ..parallel.dist import DistInfo
        from .trainer import GraphTrainer
        check_scst(hps)
        if not hps.rl_weight > 0:
            raise ValueError("ScstTrainer needs rl_weight > 0 (rl_weight = 0 is GraphTrainer)")
        info = info or DistInfo()
        if info.world > 1:
            raise ValueError("rl_weight > 0 with data parallelism (world > 1) is refused: the combination is "
                             "untested")
        if not str(device).startswith("cuda") or not torch.cuda.is_available():
            raise ValueError("rl_weight > 0 is refused on the CPU backend: the sampler and the reward kernel run "
                             "on the device")
        if hps.max_dec_steps > ROUGE_MAX_LEN:
            raise ValueError(f"rl_weight > 0 needs max_dec_steps <= {ROUGE_MAX_LEN} (the reward kernel's limit)")
        self.hps, self.vocab = hps, vocab
        self.n = hps.batch_size // 2
        self.gamma = float(hps.rl_weight)
        self.kind = RL_REWARDS.index(hps.rl_reward)
        T = T or hps.max_enc_steps
        graph = hps.graph if use_graph is None else use_graph
        self.trainer = GraphTrainer(hps, vocab.size(), B=2 * self.n, T=T, device=device, info=info, params=params,
                                    use_graph=graph)
        k = int(hps.sampling_topk)
        base = hps.replace(mode="decode", batch_size=self.n, n_samples=1, coverage_penalty_beta=0.0,
                           length_penalty="avg", block_ngram_repeat=0)
        mk = lambda h: DeviceSampler(h, vocab, self.trainer.params, n_articles=self.n, T=T, use_graph=graph,  # noqa: E731
                                     keep_attn=False, group_enc=1)
        self.greedy = mk(base.replace(sampling_topk=1, sampling_temp=1.0))
        self.sampler = mk(base.replace(sampling_topk=max(k, 0)))
        self.stop = vocab.word2id(STOP_DECODING)
        dev, D = self.trainer.device, hps.max_dec_steps
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.d = {"ref": z(self.n, D), "ref_len": z(self.n), "adv": z(self.n, dt=torch.float32)}
        for s in ("s", "g"):
            self.d["counts_" + s], self.d["reward_" + s] = z(self.n, 5), z(self.n, dt=torch.float32)
        self._pin: Dict[str, "torch.Tensor"] = {}
        self.last: Dict[str, object] = {}
        self.timing = False      # phase_ms(): the split of the last step (host-synchronising)
        self._ms: Dict[str, float] = {}

    # ------------------------------------------------------------------ the trainer's interface
    params = property(lambda self: self.trainer.params)
    engine = property(lambda self: self.trainer.engine)
    host_sync_free = False  # every step reads the samples on the host

    @property
    def global_step(self) -> int:
        return self.trainer.global_step

    @global_step.setter
    def global_step(self, v: int) -> None:
        self.trainer.global_step = int(v)

    @property
    def poison_next(self):
        return self.trainer.poison_next

    @poison_next.setter
    def poison_next(self, v) -> None:
        self.trainer.poison_next = v

    def check_finite(self, out):
        return self.trainer.check_finite(out)

    def eval_step(self, batch):
        raise NotImplementedError("eval runs the plain trainer (rl_weight applies to training only)")

    def named_debug_tensors(self):
        return self.trainer.named_debug_tensors()

    # ------------------------------------------------------------------ one step
    def refresh_samplers(self) -> None:
        """The samplers' views of the current fp32 master weights (after an optimizer step or a restore)."""
        for s in (self.greedy, self.sampler):
            s.refresh_weights(in_place=True)

    def _sample(self, smp, batch, base: int) -> None:
        for _ in smp.run_chunks(batch, sample_base=base):
            pass

    def _reward(self, smp, tag: str) -> None:
        d, D = self.d, self.hps.max_dec_steps
        smp.k.rouge_reward(smp.b["tok_hist"], smp.b["slen"], d["ref"], d["ref_len"], d["counts_" + tag],
                           d["reward_" + tag], self.n, D, D, 1, self.stop, self.kind)

    def _fetch(self, srcs):
        import torch
        for name, src in srcs.items():
            h = self._pin.get(name)
            if h is None or h.shape != src.shape or h.dtype != src.dtype:
                h = self._pin[name] = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
            h.copy_(src, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return {name: self._pin[name].numpy().copy() for name in srcs}

    def step(self, batch):
        import time

        import torch
        n, D, d = self.n, self.hps.max_dec_steps, self.d
        if batch.enc_batch.shape[0] != n:
            raise ValueError(f"batch has {batch.enc_batch.shape[0]} articles, rl_weight > 0 trains batch_size / 2 = {n}")
        if getattr(batch, "host_pack", None) is not None:
            raise ValueError("rl_weight > 0 needs plain batches (the loader's prebuilt packs hold no sample rows)")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.timing else None
        d["ref"].copy_(torch.from_numpy(np.ascontiguousarray(batch.target_batch[:, :D], dtype=np.int32)))
        d["ref_len"].copy_(torch.from_numpy(batch.dec_padding_mask[:, :D].sum(1).astype(np.int32)))
        base = self.trainer.global_step * n
        if ev:
            ev[0].record()
        self._sample(self.greedy, batch, base)
        if ev:
            ev[1].record()
        self._sample(self.sampler, batch, base)
        if ev:
            ev[2].record()
        self._reward(self.greedy, "g")
        self._reward(self.sampler, "s")
        torch.sub(d["reward_s"], d["reward_g"], out=d["adv"])  # scst_advantage
        if ev:
            ev[3].record()
            torch.cuda.synchronize()
        tf = time.perf_counter()
        b = self.sampler.b
        got = self._fetch({"tok": b["tok_hist"], "slen": b["slen"], "reward_s": d["reward_s"],
                           "reward_g": d["reward_g"], "adv": d["adv"], "tok_g": self.greedy.b["tok_hist"],
                           "slen_g": self.greedy.b["slen"], "counts_s": d["counts_s"], "counts_g": d["counts_g"],
                           "tail_s": b["tail_err"], "tail_g": self.greedy.b["tail_err"]})
        for s, tag in ((self.greedy, "tail_g"), (self.sampler, "tail_s")):
            s.eng.check_lstm_err()
            s._check_tail(int(got[tag][0]))
        t0 = time.perf_counter()
        batch2, _ = scst_batch(batch, got["tok"].T, got["slen"], self.vocab)
        row_scale, cov_scale = scst_row_scale(got["adv"], self.gamma, n)
        t1 = time.perf_counter()
        out = dict(self.trainer.step(batch2, row_scale=row_scale, cov_scale=cov_scale))
        self.refresh_samplers()
        valid = batch.valid > 0
        nv = max(int(valid.sum()), 1)
        out["rl_reward_sample"] = float(got["reward_s"][valid].sum()) / nv
        out["rl_reward_greedy"] = float(got["reward_g"][valid].sum()) / nv
        out["rl_advantage_abs"] = float(np.abs(got["adv"][valid]).sum()) / nv
        self.last = dict(got, batch2=batch2, row_scale=row_scale, cov_scale=cov_scale, stream_base=base)
        if ev:
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            self._ms = {"ms_greedy": ev[0].elapsed_time(ev[1]), "ms_sample": ev[1].elapsed_time(ev[2]),
                        "ms_reward": ev[2].elapsed_time(ev[3]), "ms_fetch": (t0 - tf) * 1e3,
                        "ms_host_pack": (t1 - t0) * 1e3,
                        "ms_train_step": (t2 - t1) * 1e3}
        return out

    def phase_ms(self) -> Dict[str, float]:
        return dict(self._ms)
