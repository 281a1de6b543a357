"""Self-critical fine-tuning on the device (train/scst.py): the weighted training step against the
oracle with the same per-row multipliers, ``ScstTrainer`` for two steps (rewards == the host rule on the
tokens it fetched, the engine's loss weights == ``host_inputs`` of ``scst_batch`` with ``scst_row_scale``,
reproducible per seed), and ``rl_weight`` 0 / 0.5 through the command line."""
import json

import numpy as np
import pytest
import torch

from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
from textsummarization_on_flink_amd.models.host_inputs import host_inputs
from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator, batch_to_tensors
from textsummarization_on_flink_amd.train import scst as S
from helpers import GPU_FLAGS, gpu_corpus, grad_mismatches, make_dataset

pytestmark = pytest.mark.gpu

STOP = S.STOP_ID


# ------------------------------------------------------------------ 1. the weighted step
def test_weighted_step_matches_the_oracle_with_the_same_multipliers():
    """One trainer step of 8 rows with hand-picked multipliers: mixed signs, a zero loss weight on a row that
    keeps its coverage weight (3), a row with both zero (6: skipped like a padded row), coverage off on half
    the rows.  Gradients: ``grad_mismatches`` at its bounds.  Losses: test_gpu_model's 2e-2 relative per
    row; rows of opposite sign cancel in the sum, so the bound is 2e-2 of the sum of the rows' absolute
    contributions (the oracle's loss with |multipliers|), which is what 2e-2 per row adds up to."""
    from test_gpu_model import _setup
    from textsummarization_on_flink_amd.train.trainer import GraphTrainer
    hps, vocab, batch, params = _setup(True, B=8)
    V = vocab.size()
    rs = np.array([1.5, 1.0, -0.5, 0.0, 2.0, 0.75, 0.0, -1.0])
    cs = np.array([2.0, 1.0, 0.5, 1.5, 0.0, 0.0, 0.0, 0.0])
    flat = params.flat.detach().clone().requires_grad_(True)
    W = {n: flat[o:o + c].view(params.view(n).shape) for n, (o, c) in params.offsets.items()}
    ref = ReferencePointerGenerator(hps, V)
    bt = batch_to_tensors(batch, "cuda")
    t = lambda x: torch.as_tensor(x, dtype=torch.float32, device="cuda")  # noqa: E731
    want = ref.forward(W, bt, row_scale=t(rs), cov_scale=t(cs))
    want["total_loss"].backward()
    with torch.no_grad():
        mag = ref.forward(W, bt, row_scale=t(np.abs(rs)), cov_scale=t(np.abs(cs)))
    tr = GraphTrainer(hps, V, B=8, T=hps.max_enc_steps, params=params)
    out = tr.step(batch, row_scale=rs, cov_scale=cs)
    torch.cuda.synchronize()
    got = tr.check_finite(out)
    eng = tr.engine
    src = eng.w["row_src"].cpu().numpy()
    assert eng.w["dlen"].cpu().numpy()[list(src).index(6)] == 0  # the all-zero row is skipped
    print("weighted step: loss", got["loss"], float(want["loss"]), "coverage", got["coverage_loss"],
          float(want["coverage_loss"]), "bounds", 2e-2 * float(mag["loss"]), 2e-2 * float(mag["coverage_loss"]))
    assert abs(got["loss"] - float(want["loss"])) < 2e-2 * float(mag["loss"])
    assert abs(got["coverage_loss"] - float(want["coverage_loss"])) < 2e-2 * float(mag["coverage_loss"]) + 1e-4
    bad = grad_mismatches(params, params.grad, flat.grad)
    assert not bad, bad
    # the unweighted step of the same trainer is what it was: multipliers are inputs, not captured
    plain = tr.check_finite(tr.step(batch))
    assert plain["loss"] > 0 and abs(plain["loss"] - got["loss"]) > 1e-3


# ------------------------------------------------------------------ 2. ScstTrainer
N_ART = 4


def _scst_setup():
    from test_gpu_decode import _peaked_setup
    from textsummarization_on_flink_amd.models.pointer_generator import OV
    hps, vocab, _, params = _peaked_setup(True, Na=N_ART)
    corpus = SyntheticCorpus(vocab_size=600, raw_vocab=1800, seed=2, art_mean=40, art_sd=10, sent_mean=4)
    batches = make_batches(hps, vocab, corpus, 2, pad_enc_to=hps.max_enc_steps)
    params[OV][STOP] += 6.0  # a [STOP] likely enough that some samples end inside the 20 steps
    return hps.replace(batch_size=2 * N_ART, rl_weight=0.5), vocab, batches, params


def _trainer(hps, vocab, params, **kw):
    from textsummarization_on_flink_amd.models.params import build_params
    p = build_params(hps, vocab.size(), device="cuda", seed=3)  # every trainer its own copy of the weights
    p.flat.copy_(params.flat)
    return S.ScstTrainer(hps, vocab, T=hps.max_enc_steps, params=p, **kw)


def _refs(batch, D):
    lens = batch.dec_padding_mask[:, :D].sum(1).astype(int)
    return [batch.target_batch[a, :lens[a]].tolist() for a in range(batch.target_batch.shape[0])]


def _run(tr, batches):
    res = []
    for b in batches:
        out = tr.step(b)
        vals = tr.check_finite(out)
        res.append((vals, dict(tr.last), tr.engine.w["rowg"].cpu().numpy().copy(),
                    tr.engine.w["gcl"].cpu().numpy().copy()))
    return res


@pytest.mark.parametrize("reward", ["rouge_l", "rouge_mean"])
def test_scst_trainer_two_steps(monkeypatch, reward):
    """(deterministic mode: the second step samples from the weights the first step updated, and only a
    training step without fp32 atomics gives two trainers the same weights to the bit)"""
    monkeypatch.setenv("TSAMD_DETERMINISTIC", "1")
    hps, vocab, batches, params = _scst_setup()
    hps = hps.replace(rl_reward=reward, sample_seed=11)
    D, n, g = hps.max_dec_steps, N_ART, hps.rl_weight
    tr = _trainer(hps, vocab, params)
    assert tr.trainer.engine.B == 2 * n and tr.sampler.R == n == tr.greedy.R
    assert (tr.sampler.topk, tr.greedy.topk) == (0, 1) and not tr.sampler.keep_attn and not tr.greedy.keep_attn
    assert tr.sampler.p is tr.trainer.params and tr.greedy.p is tr.trainer.params
    w0 = tr.params.flat.clone()
    res = _run(tr, batches)
    assert tr.global_step == 2 and not torch.equal(w0, tr.params.flat)
    ended = 0
    for s, ((vals, L, rowg, gcl), batch) in enumerate(zip(res, batches)):
        assert L["stream_base"] == s * n
        refs = _refs(batch, D)
        for tag, tk, sl in (("s", L["tok"], L["slen"]), ("g", L["tok_g"], L["slen_g"])):
            for a in range(n):
                assert 1 <= sl[a] <= D
                hyp = tk[:sl[a], a].tolist()
                c = S.rouge_ids(hyp, refs[a], STOP)
                assert tuple(L["counts_" + tag][a]) == c, (s, tag, a)
                want = float(S.reward_from_counts(c, reward))
                assert abs(float(L["reward_" + tag][a]) - want) <= 1e-6 * want, (s, tag, a)
                ended += hyp[-1] == STOP
        adv = L["reward_s"] - L["reward_g"]  # fp32, as on the device
        assert np.array_equal(adv.view(np.int32), L["adv"].view(np.int32))
        assert vals["rl_reward_sample"] == pytest.approx(float(L["reward_s"].mean()), rel=1e-6)
        assert vals["rl_reward_greedy"] == pytest.approx(float(L["reward_g"].mean()), rel=1e-6)
        assert vals["rl_advantage_abs"] == pytest.approx(float(np.abs(adv).mean()), rel=1e-6)
        b2, kind = S.scst_batch(batch, L["tok"].T, L["slen"], vocab)
        rs, cs = S.scst_row_scale(adv, g, n)
        hi = host_inputs(b2, hps, D, sort_rows=tr.engine.skip_pad, row_scale=rs, cov_scale=cs)
        assert np.array_equal(rowg, hi["rowg"]) and np.array_equal(gcl, hi["gcl"])
        src = hi["row_src"]
        assert not gcl[:, kind[src] == 1].any() and (gcl[:, kind[src] == 0] > 0).any()
        assert (rowg[0, kind[src] == 0] > 0).all()
        for a in range(n):  # a sample that beats greedy has a positive weight on its NLL
            e = list(src).index(n + a)
            assert np.sign(rowg[0, e]) == np.sign(adv[a])
    assert ended > 0  # some sequences did end in [STOP]
    # the same seed: the same tokens, rewards and loss bits
    tr2 = _trainer(hps, vocab, params)
    res2 = _run(tr2, batches)
    for (v1, L1, rg1, _), (v2, L2, rg2, _) in zip(res, res2):
        for x in ("tok", "slen", "tok_g", "slen_g", "reward_s", "reward_g", "adv"):
            assert np.array_equal(L1[x], L2[x]), x
        assert np.array_equal(rg1, rg2)
        for x in ("loss", "coverage_loss", "total_loss"):
            assert np.float32(v1[x]).view(np.int32) == np.float32(v2[x]).view(np.int32), x
    assert torch.equal(tr.params.flat, tr2.params.flat)
    # another seed: other samples, the same greedy baseline
    tr3 = _trainer(hps.replace(sample_seed=12), vocab, params, use_graph=False)
    tr3.step(batches[0])
    L1, L3 = res[0][1], tr3.last
    assert np.array_equal(L1["tok_g"], L3["tok_g"]) and np.array_equal(L1["slen_g"], L3["slen_g"])
    assert not np.array_equal(L1["tok"], L3["tok"])


# ------------------------------------------------------------------ 3. the command line
def _flags(tmp, d, vp, *extra):
    return [f"--data_path={d}/train_*", f"--vocab_path={vp}", f"--log_root={tmp}/log", "--exp_name=exp",
            *GPU_FLAGS, "--mode=train", "--check_every=1", *extra]


def test_cli_rl_weight_zero_builds_no_sampler(tmp_path, monkeypatch):
    from textsummarization_on_flink_amd import cli
    from textsummarization_on_flink_amd.decode import device_sampler
    from textsummarization_on_flink_amd.train import loop
    from textsummarization_on_flink_amd.train.trainer import GraphTrainer

    def refuse(*a, **k):
        raise AssertionError("rl_weight = 0 must build neither the self-critical trainer nor a sampler")

    monkeypatch.setattr(S, "ScstTrainer", refuse)
    monkeypatch.setattr(device_sampler.DeviceSampler, "__init__", refuse)
    made = []
    make = loop.make_trainer
    monkeypatch.setattr(loop, "make_trainer", lambda *a, **k: made.append(make(*a, **k)) or made[-1])
    d, vp, _ = make_dataset(str(tmp_path), per_file=12, corpus=gpu_corpus())
    assert cli.main(_flags(tmp_path, d, vp, "--num_steps=2", "--rl_weight=0")) == 0
    assert len(made) == 1 and type(made[0]) is GraphTrainer
    recs = [json.loads(x) for x in open(f"{tmp_path}/log/exp/metrics_train.jsonl")]
    assert [r["step"] for r in recs] == [1, 2]
    assert not [k for r in recs for k in r if k.startswith("rl_")]
    assert {"loss", "total_loss", "global_norm"} <= set(recs[0])


def test_cli_rl_weight_logs_the_reward_fields_and_resumes_the_streams(tmp_path):
    from textsummarization_on_flink_amd import cli
    from textsummarization_on_flink_amd.train import checkpoint as ckpt
    d, vp, _ = make_dataset(str(tmp_path), per_file=12, corpus=gpu_corpus())
    rl = ("--rl_weight=0.5", "--rl_reward=rouge_mean", "--sample_seed=3")
    assert cli.main(_flags(tmp_path, d, vp, "--num_steps=2", *rl)) == 0
    assert cli.main(_flags(tmp_path, d, vp, "--num_steps=1", *rl)) == 0  # resumed: global step 2
    assert ckpt.latest_checkpoint(f"{tmp_path}/log/exp/train").endswith("model.ckpt-3")
    recs = [json.loads(x) for x in open(f"{tmp_path}/log/exp/metrics_train.jsonl")]
    assert [r["step"] for r in recs] == [1, 2, 3]
    for r in recs:
        assert np.isfinite(r["loss"]) and np.isfinite(r["total_loss"])
        assert 0 <= r["rl_reward_sample"] <= 1 and 0 <= r["rl_reward_greedy"] <= 1
        assert 0 <= r["rl_advantage_abs"] <= 1
    with pytest.raises(ValueError, match="even batch_size"):
        cli.main(_flags(tmp_path, d, vp, "--num_steps=1", "--rl_weight=0.5", "--batch_size=7"))
