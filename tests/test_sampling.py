"""Decode by sampling on the host (``decode/sampling.py``): Philox known answers, the draw rules on a
stub step model with hand-made distributions, greedy equivalence with the beam search, stream
independence, ranking, validation and flag plumbing."""
from types import SimpleNamespace

import numpy as np
import pytest

from textsummarization_on_flink_amd.config import HParams, check_hps, check_sampling, parse_hyperparam_string
from textsummarization_on_flink_amd.data.vocab import START_DECODING, STOP_DECODING, Vocab
from textsummarization_on_flink_amd.decode.beam_search import Hypothesis, run_beam_search
from textsummarization_on_flink_amd.decode.sampling import (best_sample, draw_full, draw_topk, model_log_prob,
                                                            philox4x32, run_sampling, sample_uniform)

WORDS = [f"w{i}" for i in range(20)]


@pytest.fixture
def vocab():
    return Vocab(words=WORDS)  # ids: 0-3 specials, w0 = 4 ... w19 = 23; V = 24


# ------------------------------------------------------------------ random numbers
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    assert " ".join(f"{x:08x}" for x in philox4x32(ctr, key)) == out


def test_uniform_is_24_bits_in_unit_interval():
    seed = 0x1234567890abcdef
    us = [sample_uniform(seed, s, t) for s in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7) for t in range(50)]
    for u in us:
        assert 0.0 <= u < 1.0
        assert u * 2 ** 24 == int(u * 2 ** 24) and np.float32(u) == u  # 24 bits: exact in fp32
    assert len(set(us)) > 240  # streams and steps give different numbers
    # key and counter layout: word 0 of Philox at counter (t, stream lo, stream hi, 0), key (seed lo, seed hi)
    x = philox4x32((7, 5, 3, 0), (0x90abcdef, 0x12345678))[0]
    assert sample_uniform(seed, (3 << 32) + 5, 7) == (x >> 8) * 2.0 ** -24


# ------------------------------------------------------------------ the draws
def test_topk_draw_drops_stop_before_min_dec():
    stop = 3
    ids, lps = [3, 9, 8, 7], np.log([0.5, 0.2, 0.2, 0.1])
    # k = 1 with [STOP] on top: the k + 1 = 2 best hold one other candidate
    assert draw_topk(ids, lps, 1, 1.0, 0.0, stop, allow_stop=False) == 1
    assert draw_topk(ids, lps, 1, 1.0, 0.999, stop, allow_stop=False) == 1
    assert draw_topk(ids, lps, 1, 1.0, 0.999, stop, allow_stop=True) == 0
    # k = 2: candidates {9, 8} before min_dec (weights .2, .2), {[STOP], 9} after (.5, .2)
    assert [draw_topk(ids, lps, 2, 1.0, u, stop, False) for u in (0.0, 0.49, 0.51, 0.99)] == [1, 1, 2, 2]
    assert [draw_topk(ids, lps, 2, 1.0, u, stop, True) for u in (0.0, 0.7, 0.72, 0.99)] == [0, 0, 1, 1]
    # [STOP] below the k + 1 best: the first k, entry k + 1 never drawn
    ids2 = [9, 8, 7, 3]
    assert draw_topk(ids2, lps, 2, 1.0, 0.999999, stop, False) == 1


def test_topk_draw_temperature_and_clamp():
    ids, lps = [5, 6, 7], np.log([0.6, 0.3, 0.1])
    # temp 0.5 squares the weights: .36, .09 of the two kept -> threshold 0.8
    assert [draw_topk(ids, lps, 2, 0.5, u, 3, True) for u in (0.79, 0.81)] == [0, 1]
    assert [draw_topk(ids, lps, 2, 1.0, u, 3, True) for u in (0.66, 0.67)] == [0, 1]
    # u at the largest 24-bit value: the last kept candidate, never past it
    assert draw_topk(ids, lps, 2, 1.0, 1 - 2.0 ** -24, 3, True) == 1
    # a running sum that never exceeds the target (weights that vanish beside the first): clamped to the last
    # candidate of positive weight
    assert draw_topk([5, 6], np.array([0.0, -800.0]), 2, 1.0, 1 - 2.0 ** -24, 3, True) == 0


def test_full_draw_order_masking_and_clamp():
    V, stop = 6, 3
    vd = np.array([0.1, 0.0, 0.2, 0.3, 0.4, 0.0])
    attn = np.array([0.5, 0.25, 0.25, 9.0])  # position 3 is past enc_len
    ext = np.array([4, 7, 3, 2])             # a copied in-vocabulary id, an OOV, a [STOP] copy
    pg = 0.5
    # weights: vocab .05 0 .1 .15 .2 0 | positions .25 .125 .125 ; cdf .05 .05 .15 .3 .5 .5 | .75 .875 1.0
    draw = lambda u, allow=True: draw_full(vd, attn, pg, ext, 3, u, stop, allow)  # noqa: E731
    assert draw(0.0) == (0, 0)
    assert draw(0.05) == (2, 2)      # entry 1 has weight 0: never chosen
    assert draw(0.45) == (4, 4)      # id 4 through the vocabulary part ...
    assert draw(0.6) == (V + 0, 4)   # ... and through the position part
    assert draw(0.8) == (V + 1, 7)   # an in-article OOV
    assert draw(0.9) == (V + 2, 3)
    assert draw(1 - 2.0 ** -24) == (V + 2, 3)  # never position 3 (>= enc_len)
    # before min_dec: [STOP] weighs 0 in both parts; total .725, cdf .05 .05 .15 .15 .35 .35 | .6 .725 .725
    assert draw(0.15 / 0.725 + 1e-9, False) == (4, 4)
    assert draw(0.999, False) == (V + 1, 7)
    assert draw(1 - 2.0 ** -24, False) == (V + 1, 7)
    # no pointer: the vocabulary part alone
    assert draw_full(vd, None, None, None, 0, 0.99, stop, True) == (4, 4)
    assert draw_full(vd, None, None, None, 0, 0.99, stop, False) == (4, 4)
    # the model's log-prob: generation plus every copy, whatever the masking
    assert model_log_prob(4, vd, attn, pg, ext, 3) == pytest.approx(np.log(0.5 * 0.4 + 0.5 * 0.5))
    assert model_log_prob(7, vd, attn, pg, ext, 3) == pytest.approx(np.log(0.5 * 0.25))
    assert model_log_prob(3, vd, attn, pg, ext, 3) == pytest.approx(np.log(0.5 * 0.3 + 0.5 * 0.25))
    assert model_log_prob(2, vd, attn, pg, ext, 3) == pytest.approx(np.log(0.5 * 0.2))  # position 3 does not count
    assert model_log_prob(4, vd, None, None, None, 0) == pytest.approx(np.log(0.4))


class Stub:
    """A StepModel with one hand-made distribution for every row and step."""

    def __init__(self, vd, attn, pg, T):
        self.vd, self.attn, self.pg, self.T = np.asarray(vd, np.float64), np.asarray(attn, np.float64), pg, T
        self.latest = []

    def run_encoder(self, batch):
        return {}, ("c0", "h0")

    def _rest(self, n):
        return [("c", "h")] * n, [self.attn] * n, [self.pg] * n, [np.zeros(self.T)] * n

    def final(self, ext, enc_len):
        fd = np.concatenate([self.pg * self.vd, np.zeros(8)])
        np.add.at(fd, ext[:enc_len], (1 - self.pg) * self.attn[:enc_len])
        return fd

    def decode_onestep(self, enc, latest, states, prev_cov, k2):
        self.latest.append(list(latest))
        fd = self.final(self.ext, self.enc_len)
        order = np.argsort(-fd, kind="stable")[:k2]
        n = len(latest)
        return (np.tile(order, (n, 1)), np.tile(np.log(fd[order]), (n, 1)), *self._rest(n))

    def decode_onestep_parts(self, enc, latest, states, prev_cov):
        self.latest.append(list(latest))
        n = len(latest)
        return (np.tile(self.vd, (n, 1)), *self._rest(n))


def _stub_setup(vocab, **kw):
    V, T = vocab.size(), 5
    stop = vocab.word2id(STOP_DECODING)
    vd = np.full(V, 0.1 / (V - 1))
    vd[stop] = 0.9  # [STOP] is the most probable token (0.45 of the mixture; token 10: 0.35 and a bit)
    attn = np.array([0.4, 0.3, 0.3, 0.0, 0.0])
    ext = np.array([10, V + 1, 10, 0, 0])  # a duplicate in-vocabulary id and an in-article OOV
    m = Stub(vd, attn, 0.5, T)
    m.ext, m.enc_len = ext, 3
    batch = SimpleNamespace(enc_batch=np.zeros((1, T), np.int64), enc_batch_extend_vocab=ext[None], enc_lens=[3])
    hps = HParams(max_dec_steps=8, min_dec_steps=3, coverage=False, **kw)
    return m, batch, hps, stop


@pytest.mark.parametrize("k", [0, 1, 4])
def test_run_sampling_on_a_stub(vocab, k):
    m, batch, hps, stop = _stub_setup(vocab, sampling_topk=k, n_samples=6, sample_seed=11)
    V = vocab.size()
    hyps = run_sampling(m, vocab, batch, hps)
    assert len(hyps) == 6
    fd = m.final(m.ext, 3)
    ended_early = 0
    for h in hyps:
        assert h.tokens[0] == vocab.word2id(START_DECODING) and h.log_probs[0] == 0.0
        body = h.tokens[1:]
        assert stop not in body[:3]                     # never before min_dec_steps
        assert stop not in body[:-1]                    # [STOP] ends the sample
        assert len(body) == 8 or body[-1] == stop       # ... and nothing else does before max_dec_steps
        ended_early += len(body) < 8
        assert len(h.log_probs) == len(h.tokens) == len(h.attn_dists) + 1 == len(h.p_gens) + 1
        np.testing.assert_allclose(h.log_probs[1:], np.log(fd[body]), rtol=1e-12)  # the model's own, unmasked
        assert h.score == h.avg_log_prob == sum(h.log_probs) / len(h.tokens)
        if k == 1:  # greedy: the best token that is allowed
            assert body[:3] == [10, 10, 10] and body[3] == stop
    assert ended_early >= 1
    # an in-article OOV is fed back as [UNK]
    assert all(t < V for step in m.latest for t in step)
    if k == 0:
        assert len({tuple(h.tokens) for h in hyps}) > 1
    # done samples leave the step model's batch
    assert [len(x) for x in m.latest] == sorted([len(x) for x in m.latest], reverse=True)


def test_streams_do_not_depend_on_the_batch(vocab):
    """Sample s of an article draws from stream sample_base + s: the last two of four samples are the
    two samples of a run whose base is shifted by two, and the next article's streams (base +
    n_samples) differ."""
    m, batch, hps, _ = _stub_setup(vocab, sampling_topk=0, n_samples=4, sample_seed=5)
    four = run_sampling(m, vocab, batch, hps)
    two = run_sampling(m, vocab, batch, hps.replace(n_samples=2), sample_base=2)
    assert [h.tokens for h in four[2:]] == [h.tokens for h in two]
    assert [h.log_probs for h in four[2:]] == [h.log_probs for h in two]
    nxt = run_sampling(m, vocab, batch, hps, sample_base=4)
    assert [h.tokens for h in nxt] != [h.tokens for h in four]
    again = run_sampling(m, vocab, batch, hps.replace(sample_seed=6))
    assert [h.tokens for h in again] != [h.tokens for h in four]


def test_greedy_sampling_equals_beam_one_on_the_oracle():
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.beam_search import OracleStepModel
    from textsummarization_on_flink_amd.models.params import build_params
    from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator
    Na, Tm, Vm = 3, 24, 200
    hps = HParams(mode="decode", batch_size=Na, max_enc_steps=Tm, max_dec_steps=12, min_dec_steps=3, beam_size=1,
                  vocab_size=Vm, emb_dim=16, hidden_dim=16, coverage=True, pointer_gen=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3)
    corpus = SyntheticCorpus(vocab_size=Vm, raw_vocab=3 * Vm, seed=5, art_mean=18, art_sd=4, sent_mean=4)
    vocab = corpus.vocab(Vm)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=Tm)[0]
    params = build_params(hps, vocab.size(), device="cpu", seed=6)
    Wt = {n: params.flat[o:o + c].view(params.view(n).shape) for n, (o, c) in params.offsets.items()}
    model = OracleStepModel(ReferencePointerGenerator(hps, vocab.size()), Wt, hps)
    h1 = hps.replace(batch_size=1)
    for a in range(Na):
        ex = Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, h1)
        b1 = Batch([ex], h1, vocab, pad_enc_to=Tm)
        beam = run_beam_search(model, vocab, b1, hps)
        (greedy,) = run_sampling(model, vocab, b1, hps.replace(sampling_topk=1, n_samples=1), sample_base=a)
        assert greedy.tokens == beam.tokens
        assert greedy.avg_log_prob == pytest.approx(beam.avg_log_prob, rel=1e-6)
        # the full draw runs over the same model through decode_onestep_parts
        (full,) = run_sampling(model, vocab, b1, hps.replace(sampling_topk=0, n_samples=1), sample_base=a)
        assert len(full.tokens) >= 1 + hps.min_dec_steps and np.isfinite(full.log_probs).all()


# ------------------------------------------------------------------ ranking, validation, flags
def test_best_sample_prefers_the_lowest_index_among_equals():
    mk = lambda lps: Hypothesis([2] + [5] * (len(lps) - 1), lps, None)  # noqa: E731
    a, b, c, d = mk([0.0, -1.0, -2.0]), mk([0.0, -0.5, -0.5, -1.0]), mk([0.0, -1.0]), mk([0.0, -1.0])
    assert a.avg_log_prob == -1.0 and b.avg_log_prob == -0.5 and c.avg_log_prob == -0.5
    assert best_sample([a, b, c, d]) is b
    assert best_sample([a, c, b, d]) is c
    assert best_sample([a]) is a


@pytest.mark.parametrize("kw,msg", [
    ({"sampling_topk": -2}, "sampling_topk"),
    ({"sampling_topk": 32}, "sampling_topk"),
    ({"sampling_topk": 4, "sampling_temp": 0.0}, "sampling_temp"),
    ({"sampling_topk": 4, "sampling_temp": -1.0}, "sampling_temp"),
    ({"sampling_topk": 0, "sampling_temp": 0.7}, "not defined"),
    ({"sampling_topk": 4, "n_samples": 0}, "n_samples"),
    ({"sampling_topk": 4, "n_samples": 17}, "n_samples"),
    ({"sampling_topk": 4, "block_ngram_repeat": 3}, "not built yet"),
    ({"sampling_topk": 0, "length_penalty": "wu"}, "not built yet"),
    ({"sampling_topk": 4, "coverage": True, "coverage_penalty_beta": 0.5}, "not built yet"),
])
def test_check_sampling_refuses(kw, msg):
    hps = HParams(mode="decode", **kw)
    with pytest.raises(ValueError, match=msg):
        check_sampling(hps)
    with pytest.raises(ValueError, match=msg):
        check_hps(hps)


def test_check_sampling_accepts():
    for kw in ({}, {"sampling_topk": 0}, {"sampling_topk": 31, "sampling_temp": 0.7, "n_samples": 16},
               {"block_ngram_repeat": 3, "length_penalty": "wu"}, {"sampling_topk": 1, "block_ngram_repeat": 1}):
        check_hps(HParams(mode="decode", **kw))
    with pytest.raises(ValueError, match="sampling_topk >= 0"):
        run_sampling(None, None, None, HParams())


def test_flags_round_trip_through_the_hyperparameter_string():
    d = HParams()
    assert (d.sampling_topk, d.sampling_temp, d.n_samples, d.sample_seed) == (-1, 1.0, 1, 0)
    hps = parse_hyperparam_string("run_summarization.py --mode=decode --sampling_topk=8 --sampling_temp=0.7 "
                                  "--n_samples=4 --sample_seed=12345678901234567")
    assert (hps.sampling_topk, hps.sampling_temp, hps.n_samples, hps.sample_seed) == (8, 0.7, 4, 12345678901234567)
    assert HParams.from_dict(hps.to_dict()) == hps
    again = parse_hyperparam_string(" ".join(f"--{k}={v}" for k, v in hps.to_dict().items()
                                             if k.startswith(("sampl", "n_samples"))))
    assert (again.sampling_topk, again.sampling_temp, again.n_samples, again.sample_seed) == \
        (8, 0.7, 4, 12345678901234567)


def test_decode_dir_name_carries_the_sampling_mode():
    from textsummarization_on_flink_amd.decode.decoder import get_decode_dir_name
    hps = HParams(data_path="/x/test_*", mode="decode")
    plain = get_decode_dir_name(hps, "ckpt-1")
    assert "sample" not in plain
    assert get_decode_dir_name(hps.replace(sampling_topk=8), "ckpt-1") == plain.replace("_ckpt-1", "_sample8_ckpt-1")
    assert get_decode_dir_name(hps.replace(sampling_topk=0), None) == get_decode_dir_name(hps, None) + "_sample0"
