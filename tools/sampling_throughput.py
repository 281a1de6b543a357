"""Decode throughput (summaries/s) of sampling next to beam search on one device, bench_decode.py's
workload: pointer-generator + coverage, hidden 256, emb 128, enc 400, max_dec 100, vocab 50k, 64
articles per batch, random-init weights (so [STOP] is essentially never drawn: every batch runs all
100 steps).  Variants: beam 4, n_samples = 4 at sampling_topk = 8, n_samples = 4 at sampling_topk = 0;
each is timed ``--rounds`` times, alternated (a b c a b c ...), through ``decode_batches``.  Prints one
JSON line per timing and one summary line.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--articles", type=int, default=64)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=50000)
    args = ap.parse_args()
    import torch
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.device_beam import device_decoder
    from textsummarization_on_flink_amd.models.params import build_params

    base = HParams(mode="decode", batch_size=args.articles, beam_size=4, coverage=True, vocab_size=args.vocab)
    variants = {"beam4": base, "sample4_top8": base.replace(sampling_topk=8, n_samples=4),
                "sample4_full": base.replace(sampling_topk=0, n_samples=4)}
    corpus = SyntheticCorpus(vocab_size=args.vocab, seed=7)
    vocab = corpus.vocab(args.vocab)
    batches = make_batches(base, vocab, corpus, args.batches + 1, pad_enc_to=base.max_enc_steps)
    params = build_params(base, vocab.size(), device="cuda")
    decs = {}
    for name, hps in variants.items():
        decs[name] = device_decoder(hps, vocab, params, n_articles=args.articles, T=hps.max_enc_steps, keep_attn=False)
        decs[name].decode(batches[0])  # warm-up: graph capture, library picks
    torch.cuda.synchronize()
    out = {name: [] for name in variants}
    for rnd in range(args.rounds):
        for name, dec in decs.items():
            t0 = time.perf_counter()
            n = sum(len(h) for h in dec.decode_batches(batches[1:]))
            torch.cuda.synchronize()
            v = n / (time.perf_counter() - t0)
            out[name].append(round(v, 1))
            print(json.dumps({"variant": name, "round": rnd, "summaries_per_sec": round(v, 1),
                              "steps": dec.finished_steps}), flush=True)
    print(json.dumps({"summary": out, "articles_per_batch": args.articles, "batches": args.batches,
                      "vocab": args.vocab}))


if __name__ == "__main__":
    main()
