"""Length and coverage penalties of the beam search on the host: ``hyp_score`` and
``coverage_penalty`` against hand-computed values, ``run_beam_search`` over a scripted step model
whose outcome each penalty changes, the default path against results recorded before the
penalties existed, and the flag plumbing."""
import json
import os

import numpy as np
import pytest

from textsummarization_on_flink_amd.config import HParams, check_hps, parse_flags, parse_hyperparam_string
from textsummarization_on_flink_amd.decode import beam_search as bs
from textsummarization_on_flink_amd.decode.beam_search import Hypothesis, run_beam_search

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_default_search.json")


# ------------------------------------------------------------------ the score
def _hyp(lps, atts=()):
    return Hypothesis(list(range(len(lps))), list(lps), None, list(atts), [], np.zeros(4, np.float32))


def test_score_avg_is_avg_log_prob_exactly():
    hps = HParams()
    assert not bs.penalties_on(hps)
    for lps in ([0.0, -0.1], [0.0, -1.3, -2.7, -0.4], [0.0] + [-0.37] * 6):
        h = _hyp(lps)
        assert bs.hyp_score(h, hps, 4) == h.avg_log_prob


def test_score_wu_and_none_hand_values():
    h = _hyp([0.0, -1.0, -2.0])  # n = 3, sum -3
    assert bs.hyp_score(h, HParams(length_penalty="wu", length_alpha=1.0), 4) == -3.0 / (8.0 / 6.0)  # -2.25
    assert bs.hyp_score(h, HParams(length_penalty="wu", length_alpha=1.0), 4) == pytest.approx(-2.25, rel=1e-15)
    # (8 / 6) ** 0.9 = exp(0.9 * 0.2876821) = 1.295523
    assert bs.hyp_score(h, HParams(length_penalty="wu"), 4) == pytest.approx(-3.0 / 1.295523, rel=1e-6)
    assert bs.hyp_score(h, HParams(length_penalty="wu", length_alpha=0.0), 4) == -3.0  # alpha 0: the raw sum
    assert bs.hyp_score(h, HParams(length_penalty="none"), 4) == -3.0
    assert bs.length_norm(7, "avg") == 7.0 and bs.length_norm(7, "wu", 1.0) == 2.0 and bs.length_norm(7, "none") == 1.0
    for kind in ("wu", "none"):
        assert bs.penalties_on(HParams(length_penalty=kind))
    tab = bs.inv_len_table(HParams(length_penalty="wu"), 12)
    assert tab.dtype == np.float32 and tab.shape == (13,)
    assert tab[7] == np.float32(1.0 / 2.0 ** 0.9)


def test_coverage_penalty_hand_values():
    #              below  at   above        past enc_len
    c = np.array([0.25, 1.0, 1.5, 3.0, 0.0, 7.0, 2.0], np.float32)
    assert bs.coverage_penalty(c, 5) == 0.5 + 2.0
    assert bs.coverage_penalty(c, 3) == 0.5
    assert bs.coverage_penalty(c, 7) == 0.5 + 2.0 + 6.0 + 1.0
    assert bs.coverage_penalty(np.zeros(4), 4) == 0.0
    # OpenNMT-py's summary penalty: sum(max(cov, 1)) - src_len
    assert bs.coverage_penalty(c, 5) == np.maximum(c[:5], 1.0).sum() - 5
    # in the score: the sum of the attention distributions of the steps taken
    hps = HParams(coverage=True, coverage_penalty_beta=0.5)
    assert bs.penalties_on(hps)
    a0, a1 = np.array([1.0, 0.5, 0.0, 9.0], np.float32), np.array([0.5, 0.25, 0.25, 9.0], np.float32)
    h = _hyp([0.0, -1.0, -2.0], [a0, a1])
    assert bs.hyp_score(h, hps, 3) == -1.0 - 0.5 * 0.5
    # a [START]-only hypothesis has no attention yet: cp = 0
    assert bs.hyp_score(Hypothesis([2], [0.0], None, [], [], np.zeros(4, np.float32)), hps, 3) == 0.0


# ------------------------------------------------------------------ scripted beam search
START, STOP, UNK, V, T, ENC_LEN = 2, 3, 0, 50, 4, 3
A, B, C, D, E, F, X, Y, U, W = range(10, 20)


class _Vocab:
    def word2id(self, w):
        return {"[START]": START, "[STOP]": STOP, "[UNK]": UNK}[w]

    def size(self):
        return V


class _Batch:
    enc_batch = np.zeros((1, T), np.int32)
    enc_lens = np.array([ENC_LEN], np.int32)


def _onehot(i, junk=0.0):
    a = np.zeros(T, np.float32)
    a[i] = 1.0
    a[T - 1] = junk  # past enc_len: must be ignored
    return a


class _Scripted:
    """Token driven: the candidates of a row at step t are table[(t, latest token)] (filled up to
    2 * beam with far less likely junk), its attention is att[latest token], and the coverage it
    returns is the coverage it was given plus the attention of the row's previous step (the
    decoder state), as the decode graph does."""

    def __init__(self, table, att):
        self.table, self.att, self.t, self.latest = table, att, 0, []

    def run_encoder(self, batch):
        return None, np.zeros(T, np.float32)

    def decode_onestep(self, enc, latest, states, prev_coverage, k2):
        t = self.t
        self.t += 1
        self.latest.append(list(latest))
        ids, lps = np.zeros((len(latest), k2), np.int32), np.zeros((len(latest), k2), np.float32)
        for i, w in enumerate(latest):
            cand = list(self.table.get((t, w), []))
            cand += [(30 + j, -50.0 - j) for j in range(k2 - len(cand))]
            ids[i], lps[i] = [c[0] for c in cand], [c[1] for c in cand]
        attn = [self.att[w] for w in latest]
        covs = [c + s if c is not None else None for c, s in zip(prev_coverage, states)]
        return ids, lps, attn, attn, [None] * len(latest), covs


def _search(table, att, **kw):
    hps = HParams(mode="decode", beam_size=2, **kw)
    check_hps(hps)
    model = _Scripted(table, att)
    return run_beam_search(model, _Vocab(), _Batch(), hps), model


ATT = {START: _onehot(0, 4.0), A: _onehot(0, 5.0), B: _onehot(1), C: _onehot(2), D: _onehot(1), E: _onehot(2),
       F: _onehot(1), X: _onehot(2, 3.0), Y: _onehot(2), U: _onehot(2), W: _onehot(2)}


def test_wu_changes_the_winner():
    """Two results: [S a STOP] (sum -2, 3 tokens) and [S a c d STOP] (sum -3, 5 tokens).  The
    average prefers the long one (-0.6 against -0.667), wu at alpha 0.9 the short one (-1.894
    against -1.544), and so does the raw sum."""
    table = {(0, START): [(A, -0.5), (B, -0.625)],
             (1, A): [(STOP, -1.5), (C, -0.75)], (1, B): [(E, -3.0)],
             (2, C): [(D, -0.75)], (2, E): [(F, -0.125)],
             (3, D): [(STOP, -1.0)], (3, F): [(STOP, -2.0)]}
    kw = dict(max_dec_steps=4, min_dec_steps=1)
    avg, _ = _search(table, ATT, **kw)
    assert avg.tokens == [START, A, C, D, STOP] and avg.score == avg.avg_log_prob == -3.0 / 5
    wu, _ = _search(table, ATT, length_penalty="wu", **kw)
    assert wu.tokens == [START, A, STOP]
    assert wu.score == -2.0 / ((5.0 + 3) / 6) ** 0.9 and wu.avg_log_prob == -2.0 / 3  # avg_log_prob stays the average
    none, _ = _search(table, ATT, length_penalty="none", **kw)
    assert none.tokens == [START, A, STOP] and none.score == -2.0


BETA_TABLE = {(0, START): [(A, -0.25), (B, -0.5)],
              (1, A): [(X, -0.25), (Y, -0.5)], (1, B): [(U, -1.0), (W, -1.25)],
              (2, X): [(STOP, -0.125)], (2, Y): [(STOP, -0.25)], (2, U): [(STOP, -6.0)], (2, W): [(STOP, -6.5)]}


def test_coverage_penalty_changes_the_winner_at_the_step_ranking():
    """[START] and ``a`` both attend to position 0, so every hypothesis through ``a`` has coverage 2
    there (cp = 1); the ones through ``b`` spread their attention (cp = 0).  Step 1 offers
    [S a x] -0.5, [S a y] -0.75, [S b u] -1.5, [S b w] -1.75: without the penalty the beam keeps the
    first two, with beta = 1 their keys are -1.17 and -1.25 against -0.5 and -0.58, so both are
    dropped.  The search then has to end in [S b u STOP] (sum -7.5, score -1.875) although
    [S a x STOP] would score -0.156 - 1 = -1.156 under the same penalty: the penalty acted when the
    beam was chosen, not only on the final pick."""
    kw = dict(max_dec_steps=3, min_dec_steps=2, coverage=True)
    plain, m0 = _search(BETA_TABLE, ATT, **kw)
    assert plain.tokens == [START, A, X, STOP] and plain.score == plain.avg_log_prob == -0.625 / 4
    assert sorted(m0.latest[2]) == [X, Y]
    hps1 = HParams(mode="decode", beam_size=2, coverage_penalty_beta=1.0, **kw)
    pen, m1 = _search(BETA_TABLE, ATT, coverage_penalty_beta=1.0, **kw)
    assert sorted(m1.latest[2]) == [U, W], "[S a x] survived the step ranking"
    assert pen.tokens == [START, B, U, STOP]
    assert pen.score == -7.5 / 4 and pen.avg_log_prob == -7.5 / 4  # cp = 0: attention on three positions
    assert bs.hyp_score(plain, hps1, ENC_LEN) == -0.625 / 4 - 1.0 > pen.score
    # the attention past enc_len (junk 4 + 5 + 3 at position 3) was ignored, position 0 counted twice
    total = plain.coverage + plain.attn_dists[-1]
    assert total.tolist() == [2.0, 0.0, 1.0, 12.0] and bs.coverage_penalty(total, ENC_LEN) == 1.0


def test_coverage_penalty_needs_a_coverage_model():
    with pytest.raises(ValueError):
        run_beam_search(_Scripted(BETA_TABLE, ATT), _Vocab(), _Batch(),
                        HParams(mode="decode", beam_size=2, max_dec_steps=3, min_dec_steps=2, coverage=False,
                                coverage_penalty_beta=1.0))


# ------------------------------------------------------------------ the default path
def default_search():
    """Host search over the fp32 oracle, default penalty flags: 4 short synthetic articles."""
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.beam_search import OracleStepModel
    from textsummarization_on_flink_amd.models.params import build_params
    from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator
    Na, Tm, Vm = 4, 24, 200
    hps = HParams(mode="decode", batch_size=Na, max_enc_steps=Tm, max_dec_steps=12, min_dec_steps=3, beam_size=4,
                  vocab_size=Vm, emb_dim=16, hidden_dim=16, coverage=True, pointer_gen=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3)
    corpus = SyntheticCorpus(vocab_size=Vm, raw_vocab=3 * Vm, seed=5, art_mean=18, art_sd=4, sent_mean=4)
    vocab = corpus.vocab(Vm)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=Tm)[0]
    params = build_params(hps, vocab.size(), device="cpu", seed=6)
    Wt = {n: params.flat[o:o + c].view(params.view(n).shape) for n, (o, c) in params.offsets.items()}
    model = OracleStepModel(ReferencePointerGenerator(hps, vocab.size()), Wt, hps)
    h1 = hps.replace(batch_size=hps.beam_size)
    out = []
    for a in range(Na):
        ex = Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, h1)
        out.append(run_beam_search(model, vocab, Batch([ex] * hps.beam_size, h1, vocab, pad_enc_to=Tm), hps))
    return out


def test_default_flags_search_as_recorded():
    """tests/golden/beam_default_search.json: the tokens and avg_log_prob floats this search
    returned before the penalty options existed."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = default_search()
    assert len(got) == len(want) == 4
    for h, w in zip(got, want):
        assert [int(t) for t in h.tokens] == w["tokens"]
        assert float(h.avg_log_prob) == w["avg_log_prob"]
        assert h.score == h.avg_log_prob


# ------------------------------------------------------------------ flags
def test_check_hps_refusals():
    check_hps(HParams())
    check_hps(HParams(length_penalty="wu", length_alpha=0.0, coverage=True, coverage_penalty_beta=2.0))
    check_hps(HParams(length_penalty="none"))
    for bad in (dict(length_penalty="gnmt"), dict(length_penalty=""), dict(length_alpha=-0.1),
                dict(coverage=True, coverage_penalty_beta=-1.0), dict(coverage=False, coverage_penalty_beta=0.3)):
        with pytest.raises(ValueError):
            check_hps(HParams(**bad))


def test_penalty_flags_parse():
    d = HParams()
    assert (d.length_penalty, d.length_alpha, d.coverage_penalty_beta) == ("avg", 0.9, 0.0)
    hp = parse_flags(["--length_penalty=wu", "--length_alpha=0.6", "--coverage_penalty_beta=0.25", "--coverage"])
    assert (hp.length_penalty, hp.length_alpha, hp.coverage_penalty_beta, hp.coverage) == ("wu", 0.6, 0.25, True)
    hp = parse_hyperparam_string("run_summarization.py --mode=decode --length_penalty=none --coverage=1 "
                                 "--coverage_penalty_beta=1.5 --beam_size=4")
    assert (hp.length_penalty, hp.length_alpha, hp.coverage_penalty_beta) == ("none", 0.9, 1.5)
    assert hp.mode == "decode" and hp.beam_size == 4 and hp.coverage
    check_hps(hp)


def test_hparams_json_round_trip_with_penalty_fields():
    hp = HParams(length_penalty="wu", length_alpha=0.7, coverage=True, coverage_penalty_beta=0.4)
    d = json.loads(hp.to_json())
    assert d["length_penalty"] == "wu" and d["length_alpha"] == 0.7 and d["coverage_penalty_beta"] == 0.4
    assert HParams.from_dict(d) == hp
    d0 = json.loads(HParams().to_json())
    assert (d0["length_penalty"], d0["length_alpha"], d0["coverage_penalty_beta"]) == ("avg", 0.9, 0.0)
    assert HParams.from_dict(d0) == HParams()
