"""Self-critical fine-tuning, the host side (train/scst.py): the ROUGE rule on token ids against
decode/rouge.py, the row scales, their way through ``host_inputs`` and the oracle, and the 2n-row batch."""
import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.config import HParams, check_hps
from textsummarization_on_flink_amd.data.synthetic import make_batches
from textsummarization_on_flink_amd.decode import rouge as R
from textsummarization_on_flink_amd.models.host_inputs import host_inputs
from textsummarization_on_flink_amd.models.params import build_params
from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator, batch_to_tensors
from textsummarization_on_flink_amd.train import scst as S
from helpers import tiny_corpus

STOP = S.STOP_ID


def _pairs():
    """Random pairs over small and large alphabets, then the corner cases."""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(40):
        a = int(rng.choice([3, 10, 50]))
        nh, nr = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        out.append((list(rng.integers(4, 4 + a, nh)), list(rng.integers(4, 4 + a, nr))))
    seq = list(range(10, 40))
    out += [([], []), ([], [7]), ([7], []), ([7], [7]), ([7], [8]), ([7, 8], [7, 8]), ([7, 8], [8, 7]),
            (seq, seq), (seq, [x + 100 for x in seq]), ([9] * 20, [9] * 7), ([9] * 5, [9] * 30),
            ([4, 5, 4, 5, 4], [5, 4, 5, 4, 5, 4, 4])]
    return out


def _words(ids):
    return " ".join(f"w{int(i)}" for i in ids)


def test_rouge_ids_equals_decode_rouge_on_single_sentences():
    for h, r in _pairs():
        hit1, hit2, lcs, nh, nr = S.rouge_ids(h, r)
        assert (nh, nr) == (len(h), len(r))
        for got_hit, n_h, n_r, want in ((hit1, nh, nr, R.rouge_n([_words(h)], [_words(r)], 1)),
                                        (hit2, max(nh - 1, 0), max(nr - 1, 0), R.rouge_n([_words(h)], [_words(r)], 2)),
                                        (lcs, nh, nr, R.rouge_l([_words(h)], [_words(r)]))):
            p, rec, f = want
            assert got_hit == round(p * n_h) == round(rec * n_r), (h, r)
            assert abs(float(S.rouge_f(got_hit, n_h, n_r)) - f) <= 1e-6, (h, r)
        assert lcs <= hit1 <= min(nh, nr) and hit2 <= max(min(nh, nr) - 1, 0)


def test_rouge_ids_cuts_before_the_first_stop():
    h, r = [5, 6, 7, STOP, 8, 9, STOP, 5], [5, 6, 8, 9, STOP, 1, 1]
    assert S.rouge_ids(h, r) == S.rouge_ids([5, 6, 7], [5, 6, 8, 9]) == (2, 1, 2, 3, 4)
    assert S.rouge_ids([STOP, 5], [5]) == (0, 0, 0, 0, 1)
    assert S.rouge_ids([5, 6], [5, 6]) == (2, 1, 2, 2, 2)  # no [STOP]: the whole sequence


def test_rouge_f_and_rewards():
    assert S.rouge_f(0, 0, 5) == 0 and S.rouge_f(0, 5, 0) == 0 and S.rouge_f(0, 3, 3) == 0
    assert S.rouge_f(3, 3, 3) == 1 and S.rouge_f(3, 3, 3).dtype == np.float32
    f = S.rouge_f(2, 3, 4)
    p, r = np.float32(2) / np.float32(3), np.float32(2) / np.float32(4)
    assert f == np.float32(2) * p * r / (p + r)
    c = S.rouge_ids([5, 6, 7, 8], [6, 7, 9, 5])
    f1, f2, fl = S.rouge_f(c[0], 4, 4), S.rouge_f(c[1], 3, 3), S.rouge_f(c[2], 4, 4)
    assert S.reward_from_counts(c, "rouge_1") == f1 and S.reward_from_counts(c, "rouge_2") == f2
    assert S.reward_from_counts(c, "rouge_l") == fl == S.reward([5, 6, 7, 8], [6, 7, 9, 5])
    assert S.reward_from_counts(c, "rouge_mean") == np.float32((f1 + f2 + fl) / np.float32(3))
    assert S.reward([5], [5], "rouge_2") == 0 and S.reward([5], [5], "rouge_1") == 1  # no bigram
    with pytest.raises(ValueError):
        S.reward([5], [5], "bleu")


def test_scst_row_scale_signs_and_ends():
    adv = np.array([0.25, -0.5, 0.0])
    rs, cs = S.scst_row_scale(adv, 0.75, 3)
    np.testing.assert_allclose(rs, [0.5, 0.5, 0.5, 0.375, -0.75, 0.0])
    np.testing.assert_allclose(cs, [0.5, 0.5, 0.5, 0, 0, 0])
    assert rs[3] > 0 > rs[4]  # a sample that beats greedy: positive weight on its NLL (likelihood raised)
    rs, cs = S.scst_row_scale(adv, 0.0, 3)
    assert rs.tolist() == [2, 2, 2, 0, 0, 0] and cs.tolist() == [2, 2, 2, 0, 0, 0]
    rs, cs = S.scst_row_scale(adv, 1.0, 3)
    assert rs[:3].tolist() == [0, 0, 0] and cs.tolist() == [0] * 6 and rs[3:].tolist() == [0.5, -1.0, 0.0]
    # the mean over 2n rows of scale * x is the objective
    g, nll_gold, nll_s = 0.3, np.array([1.0, 2.0, 4.0]), np.array([3.0, 5.0, 7.0])
    rs, _ = S.scst_row_scale(adv, g, 3)
    want = (1 - g) * nll_gold.mean() + g * (adv * nll_s).mean()
    assert abs((rs * np.concatenate([nll_gold, nll_s])).mean() - want) < 1e-12
    with pytest.raises(ValueError):
        S.scst_row_scale(adv, 1.5, 3)
    with pytest.raises(ValueError):
        S.scst_row_scale(adv, 0.5, 4)


def _tiny(coverage=True, B=6, pointer_gen=True):
    hps = HParams(batch_size=B, max_enc_steps=30, max_dec_steps=8, min_dec_steps=2, vocab_size=200, emb_dim=8,
                  hidden_dim=16, coverage=coverage, pointer_gen=pointer_gen)
    corpus = tiny_corpus(3)
    vocab = corpus.vocab(200)
    return hps, vocab, make_batches(hps, vocab, corpus, 1, pad_enc_to=30)[0]


@pytest.mark.parametrize("sort_rows", [False, True])
@pytest.mark.parametrize("pointer_gen", [True, False])
def test_host_inputs_row_scales(sort_rows, pointer_gen):
    hps, vocab, batch = _tiny(pointer_gen=pointer_gen)
    D, B = hps.max_dec_steps, hps.batch_size
    batch.dec_padding_mask[1, 3:] = 0  # rows of different lengths, so that the sort moves them
    base = host_inputs(batch, hps, D, sort_rows=sort_rows)
    none = host_inputs(batch, hps, D, sort_rows=sort_rows, row_scale=None, cov_scale=None)
    assert base.keys() == none.keys()
    for k in base:
        assert base[k].dtype == none[k].dtype and base[k].tobytes() == none[k].tobytes(), k
    rs = np.array([2.0, -0.5, 0.25, 1.0, -4.0, 0.125])  # (powers of two: scaling commutes with the fp32 rounding)
    cs = np.array([2.0, 2.0, 0.0, 0.0, 1.0, 0.5])
    got = host_inputs(batch, hps, D, sort_rows=sort_rows, row_scale=rs, cov_scale=cs)
    plain = host_inputs(batch, hps, D, sort_rows=False)
    src = got["row_src"]
    np.testing.assert_array_equal(got["rowg"], (plain["rowg"].astype(np.float64) * rs[None, :])[:, src].astype(np.float32))
    np.testing.assert_array_equal(got["gcl"], (plain["gcl"].astype(np.float64) * cs[None, :])[:, src].astype(np.float32))
    np.testing.assert_array_equal(got["enc_lens"], batch.enc_lens[src])
    assert (got["rowg"] < 0).any()
    # a zero-scale row is skipped like a padded row
    rs0, cs0 = rs.copy(), cs.copy()
    rs0[4] = cs0[4] = 0.0
    z = host_inputs(batch, hps, D, sort_rows=sort_rows, row_scale=rs0, cov_scale=cs0)
    e = int(np.nonzero(z["row_src"] == 4)[0][0])
    assert z["dlen"][e] == 0 and not z["rowg"][:, e].any() and not z["gcl"][:, e].any()
    assert (np.delete(z["dlen"], e) > 0).all()
    if sort_rows:
        assert e == B - 1 and (np.diff(z["dlen"]) <= 0).all()
    with pytest.raises(ValueError):
        host_inputs(batch, hps, D, row_scale=rs[:3])
    with pytest.raises(ValueError):
        host_inputs(batch, hps, D, cov_scale=np.full(B, np.nan))


@pytest.mark.parametrize("pointer_gen", [True, False])
def test_oracle_weighted_loss_is_the_sum_over_its_rows(pointer_gen):
    hps, vocab, batch = _tiny(pointer_gen=pointer_gen)
    B = hps.batch_size
    params = build_params(hps, vocab.size(), device="cpu", seed=1)
    W = {n: params.view(n) for n in params.names}
    ref = ReferencePointerGenerator(hps, vocab.size())
    bt = batch_to_tensors(batch)
    with torch.no_grad():
        plain = ref.forward(W, bt)
        again = ref.forward(W, bt, row_scale=None, cov_scale=None)
        assert torch.equal(plain["loss"], again["loss"]) and torch.equal(plain["total_loss"], again["total_loss"])
        rs = torch.tensor([2.0, -0.5, 0.25, 1.0, -3.0, 0.0])
        cs = torch.tensor([2.0, 2.0, 0.0, 0.0, 1.0, 0.5])
        out = ref.forward(W, bt, row_scale=rs, cov_scale=cs)
        # its own per-row losses: the forward of each row alone, scaled by hand
        rows_l, rows_c = [], []
        for b in range(B):
            one = torch.zeros(B)
            one[b] = 1.0
            o = ref.forward(W, bt, row_scale=one, cov_scale=one)
            rows_l.append(float(o["loss"]))
            rows_c.append(float(o["coverage_loss"]))
    assert abs(sum(rows_l) - float(plain["loss"])) < 1e-5 * abs(float(plain["loss"]))
    want_l = sum(float(rs[b]) * rows_l[b] for b in range(B))
    want_c = sum(float(cs[b]) * rows_c[b] for b in range(B))
    assert abs(float(out["loss"]) - want_l) < 1e-5 * max(abs(x) for x in rows_l) * B
    assert abs(float(out["coverage_loss"]) - want_c) < 1e-5 * max(abs(x) for x in rows_c) * B
    assert abs(float(out["total_loss"]) - (want_l + hps.cov_loss_wt * want_c)) < 1e-4


def test_scst_batch_rows_inputs_targets_masks():
    hps, vocab, batch = _tiny(B=3)
    n, D, V = 3, hps.max_dec_steps, vocab.size()
    unk, start, pad = vocab.word2id("[UNK]"), vocab.word2id("[START]"), vocab.word2id("[PAD]")
    toks = np.zeros((n, D), np.int32)  # past a sample's length: whatever the history holds (zeros)
    toks[0, :4] = [10, V + 2, 11, STOP]          # an in-article OOV, then [STOP]
    toks[1, :D] = [20 + i for i in range(D)]     # ran into max_dec_steps: no [STOP]
    toks[1, 3] = V
    toks[2, :1] = [STOP]
    lens = np.array([4, D, 1])
    b2, kind = S.scst_batch(batch, toks, lens, vocab)
    assert kind.tolist() == [0, 0, 0, 1, 1, 1]
    for name in ("enc_batch", "enc_lens", "enc_batch_extend_vocab", "enc_padding_mask", "valid"):
        x = getattr(batch, name)
        assert np.array_equal(getattr(b2, name), np.concatenate([x, x], 0)), name
    for name in ("dec_batch", "target_batch", "dec_padding_mask"):
        assert np.array_equal(getattr(b2, name)[:n], getattr(batch, name)), name
        assert getattr(b2, name).dtype == getattr(batch, name).dtype
    assert b2.dec_batch[3, :5].tolist() == [start, 10, unk, 11, pad]          # ids >= V -> [UNK] in the inputs
    assert b2.target_batch[3, :5].tolist() == [10, V + 2, 11, STOP, pad]      # ... not in the targets; [STOP] kept
    assert b2.dec_batch[4].tolist() == [start] + [20, 21, 22, unk, 24, 25, 26][:D - 1]
    assert b2.target_batch[4].tolist() == toks[1].tolist() and STOP not in b2.target_batch[4]
    assert b2.dec_batch[5].tolist() == [start] + [pad] * (D - 1) and b2.target_batch[5, 0] == STOP
    assert b2.dec_padding_mask[n:].sum(1).tolist() == [4, D, 1]
    assert b2.max_art_oovs == batch.max_art_oovs and b2.num_tokens() == batch.num_tokens() + int(
        batch.enc_lens.sum()) + 4 + D + 1
    # the engine's inputs accept it
    hi = host_inputs(b2, hps.replace(batch_size=2 * n), D, sort_rows=True,
                     row_scale=np.array([1, 1, 1, 0.5, -0.5, 0.0]), cov_scale=np.array([1, 1, 1, 0, 0, 0.0]))
    assert hi["rowg"].shape == (D, 2 * n) and sorted(hi["row_src"].tolist()) == list(range(2 * n))
    with pytest.raises(ValueError):
        S.scst_batch(batch, toks, np.array([4, D + 1, 1]), vocab)
    with pytest.raises(ValueError):
        S.scst_batch(batch, toks[:2], lens[:2], vocab)


def test_flags_and_guards():
    hps = HParams()
    assert hps.rl_weight == 0.0 and hps.rl_reward == "rouge_l"
    check_hps(hps)
    check_hps(hps.replace(rl_weight=0.5))
    check_hps(hps.replace(batch_size=15))  # rl_weight = 0: any batch size, as before
    for bad in (dict(rl_weight=-0.1), dict(rl_weight=1.5), dict(rl_reward="bleu"), dict(rl_weight=0.5, batch_size=15),
                dict(rl_weight=0.5, pointer_gen=False)):
        with pytest.raises(ValueError):
            check_hps(hps.replace(**bad))
    from textsummarization_on_flink_amd.config import parse_flags
    h = parse_flags(["--rl_weight=0.25", "--rl_reward=rouge_mean"])
    assert h.rl_weight == 0.25 and h.rl_reward == "rouge_mean"


def test_scst_trainer_refused_on_cpu_and_with_data_parallelism():
    from textsummarization_on_flink_amd.parallel.dist import DistInfo
    from textsummarization_on_flink_amd.train.loop import make_trainer
    hps, vocab, _ = _tiny(B=4)
    with pytest.raises(ValueError, match="CPU backend"):
        S.ScstTrainer(hps.replace(rl_weight=0.5), vocab, device="cpu")
    with pytest.raises(ValueError, match="CPU backend"):
        make_trainer(hps.replace(rl_weight=0.5), vocab.size(), device="cpu", vocab=vocab)
    info = DistInfo()
    info.world = 2
    with pytest.raises(ValueError, match="untested"):
        S.ScstTrainer(hps.replace(rl_weight=0.5), vocab, device="cuda", info=info)
    with pytest.raises(ValueError, match="rl_weight > 0"):
        S.ScstTrainer(hps, vocab, device="cuda")
    from textsummarization_on_flink_amd.train.cpu_trainer import CpuTrainer
    assert isinstance(make_trainer(hps, vocab.size(), device="cpu", vocab=vocab), CpuTrainer)  # rl_weight = 0
