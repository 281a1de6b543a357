"""The numbers of profiles/scst.md, on one device.

1. ``rouge_reward`` for 256 (hypothesis, reference) pairs of 100 tokens (ids from a Zipf-like alphabet, so
   the pairs overlap): device events around ``--launches`` launches after a warm-up; beside it the host
   rule ``train.scst.rouge_ids`` on the same pairs, and ``decode/rouge.py`` (strings, numpy LCS table) on
   ``--string_pairs`` of them scaled to 256.
2. ``ScstTrainer.step`` at the headline shape (128 articles, 256 training rows; hidden 256, emb 128, enc 400,
   max_dec 100, vocab 50k, coverage), split into the greedy pass, the sampling pass, the rewards, the
   fetch, the host pack and the training step (which includes refreshing the samplers' weights), next to
   ``GraphTrainer.step`` of 256 gold rows.  Random-init weights: [STOP] is essentially never drawn, so both
   sampler passes run all 100 steps -- the longest a pass can be.

Prints one JSON line per part."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def reward_part(args):
    import numpy as np
    import torch

    from textsummarization_on_flink_amd.decode import rouge as R
    from textsummarization_on_flink_amd.ops import ops
    from textsummarization_on_flink_amd.train import scst as S
    k = ops()
    n, L = args.pairs, 100
    rng = np.random.default_rng(0)
    p = 1.0 / np.arange(1, 2001) ** 1.07
    draw = lambda: (4 + rng.choice(2000, size=(n, L), p=p / p.sum())).astype(np.int32)  # noqa: E731
    hyp, ref = draw(), draw()
    dev = "cuda"
    tok = torch.from_numpy(np.ascontiguousarray(hyp.T)).to(dev)
    refd = torch.from_numpy(ref).to(dev)
    lens = torch.full((n,), L, dtype=torch.int32, device=dev)
    counts, reward = torch.zeros(n, 5, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
    run = lambda: k.rouge_reward(tok, lens, refd, lens, counts, reward, n, L, L, 1, S.STOP_ID, 0)  # noqa: E731
    for _ in range(10):
        run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(args.launches):
        run()
    ev[1].record()
    torch.cuda.synchronize()
    dev_us = ev[0].elapsed_time(ev[1]) * 1e3 / args.launches
    t0 = time.perf_counter()  # one launch as a step sees it: launch + copy of the rewards + synchronise
    run()
    reward.cpu()
    sync_us = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    want = np.array([S.rouge_ids(hyp[i], ref[i]) for i in range(n)])
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(counts.cpu().numpy(), want)
    m = args.string_pairs
    words = lambda ids: [" ".join(f"w{int(i)}" for i in ids)]  # noqa: E731
    t0 = time.perf_counter()
    for i in range(m):
        h, r = words(hyp[i]), words(ref[i])
        R.rouge_n(h, r, 1), R.rouge_n(h, r, 2), R.rouge_l(h, r)
    str_ms = (time.perf_counter() - t0) * 1e3 * n / m
    print(json.dumps({"part": "reward", "pairs": n, "tokens": L, "launches": args.launches,
                      "rouge_reward_us_per_launch": round(dev_us, 2), "launch_copy_sync_us": round(sync_us, 1),
                      "host_rouge_ids_ms": round(host_ms, 1), "decode_rouge_strings_ms_scaled": round(str_ms, 1),
                      "mean_lcs": float(want[:, 2].mean())}), flush=True)


def step_part(args):
    import torch

    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.train.scst import ScstTrainer
    from textsummarization_on_flink_amd.train.trainer import GraphTrainer
    n = args.articles
    hps = HParams(batch_size=2 * n, coverage=True, vocab_size=args.vocab, rl_weight=0.5, min_dec_steps=35)
    corpus = SyntheticCorpus(vocab_size=args.vocab, seed=7)
    vocab = corpus.vocab(args.vocab)
    arts = make_batches(hps.replace(batch_size=n), vocab, corpus, 4, pad_enc_to=hps.max_enc_steps)
    gold = make_batches(hps, vocab, corpus, 4, pad_enc_to=hps.max_enc_steps)
    tr = ScstTrainer(hps, vocab)
    tr.timing = True
    for i in range(args.warmup):
        tr.step(arts[i % 4])
    torch.cuda.synchronize()
    rows, wall = [], []
    for i in range(args.steps):
        t0 = time.perf_counter()
        out = tr.step(arts[i % 4])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(tr.phase_ms())
    tr.check_finite(out)
    med = {key: round(statistics.median(r[key] for r in rows), 3) for key in rows[0]}
    res = {"part": "scst_step", "articles": n, "rows": 2 * n, "steps": args.steps,
           "step_ms_median": round(statistics.median(wall), 2), "step_ms_min_max": [round(min(wall), 2), round(max(wall), 2)],
           "sample_len_mean": float(tr.last["slen"].mean()), **med}
    print(json.dumps(res), flush=True)
    del tr
    torch.cuda.empty_cache()
    gt = GraphTrainer(hps.replace(rl_weight=0.0), vocab.size(), B=2 * n, T=hps.max_enc_steps)
    for i in range(args.warmup):
        gt.step(gold[i % 4])
    torch.cuda.synchronize()
    wall = []
    for i in range(args.steps):
        t0 = time.perf_counter()
        out = gt.step(gold[i % 4])
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    gt.check_finite(out)
    print(json.dumps({"part": "graph_trainer_step", "rows": 2 * n, "steps": args.steps,
                      "step_ms_median": round(statistics.median(wall), 2),
                      "step_ms_min_max": [round(min(wall), 2), round(max(wall), 2)]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--string_pairs", type=int, default=16)
    ap.add_argument("--articles", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--skip_step", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scst_profile needs the GPU: a CPU timing says nothing about it")
    reward_part(args)
    if not args.skip_step:
        step_part(args)


if __name__ == "__main__":
    main()
