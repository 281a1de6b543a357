"""Wall-time breakdown of one training step by phase, without profiler distortion.

Builds the bench-shaped engine (defaults: pointer-gen + coverage, H=256, E=128, T=400, D=100,
V=50k, B=256), runs two eager steps so every buffer holds realistic values, then captures each
phase of the step as its own hipGraph and times its replays with HIP events:
encoder forward | decoder forward loop | head forward (+vocab loss) | backward_head |
backward_mid | backward_tail | optimizer.  Prints one JSON line (ms per phase).  When the
persistent decoder launch is in use (``dec_persistent``: TSAMD_DEC_PERSISTENT, eligible shape),
``decoder_fwd_chains`` is the same decoder forward with the switch off (the per-step chains); it
is timed after the step's phases, behind a second encoder forward so both decoder phases start
from the same cache state, and is not part of ``total``.  ``decoder_fwd_queued`` is the persistent
decoder phase timed the same way right after it: both are enqueued while the GPU still works on the
step, so neither contains the host's graph-launch time, which ``decoder_fwd`` (second phase after
an idle GPU) can.  Likewise for the decoder backward loop (``dec_bwd_persistent``:
TSAMD_DEC_BWD_PERSISTENT, eligible shape): ``backward_mid_chains`` is backward_mid with the switch
off (``dec_force_chains`` on the engine, as for the forward) and ``backward_mid_queued`` the persistent one, each
timed behind a replay of backward_head.  These extra replays come after the step's optimizer phase,
so they work on the updated weights and on gradient buffers the step has already consumed: the
same shapes, lengths and dead steps, hence the same time, but their outputs mean nothing.

  python tools/phase_micro.py [--batch B] [--hidden H] [--enc T] [--layers L]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--enc", type=int, default=400)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.models.params import build_params
    from textsummarization_on_flink_amd.models.pointer_generator import HipPointerGenerator

    V = 50000
    hps = HParams(batch_size=a.batch, max_enc_steps=a.enc, max_dec_steps=100, vocab_size=V, hidden_dim=a.hidden,
                  emb_dim=128, coverage=True, pointer_gen=True, enc_layers=a.layers)
    corpus = SyntheticCorpus(vocab_size=V, seed=3)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=a.enc)[0]
    params = build_params(hps, vocab.size(), device="cuda").enable_grad().enable_adagrad(hps.adagrad_init_acc)
    eng = HipPointerGenerator(hps, vocab.size(), params, B=a.batch, T=a.enc)
    eng.set_batch(batch)
    for _ in range(2):
        eng.train_step()
    torch.cuda.synchronize()
    phases = [("encoder_fwd", eng._encoder_forward), ("decoder_fwd", eng._decoder_forward),
              ("head_fwd", lambda: eng._head_forward(True)), ("backward_head", eng.backward_head),
              ("backward_mid", eng.backward_mid), ("backward_tail", eng.backward_tail),
              ("optimizer", eng.optimizer_step)]
    nstep = len(phases)

    def chains(direction, fn):  # fn with that decoder loop as the per-step chains
        def run():
            eng.dec_force_chains.add(direction)
            try:
                fn()
            finally:
                eng.dec_force_chains.discard(direction)
        return run

    fwd_persistent, bwd_persistent = bool(eng.dec_fwd_persistent_on()), bool(eng.dec_bwd_persistent_on())
    if fwd_persistent:
        phases.append(("decoder_fwd_chains", chains("fwd", eng._decoder_forward)))
    n_bwd = len(phases)  # index of backward_mid_chains when present
    if bwd_persistent:
        phases.append(("backward_mid_chains", chains("bwd", eng.backward_mid)))
    graphs = []
    pool = torch.cuda.graph_pool_handle()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _, fn in phases:  # warm-up on a side stream (allocations settle)
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    from textsummarization_on_flink_amd.utils.graphs import capture_guard
    with capture_guard():
        for _, fn in phases:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                fn()
            graphs.append(g)
    torch.cuda.synchronize()
    res = {"batch": a.batch, "hidden": a.hidden, "enc": a.enc, "layers": a.layers,
           "dec_persistent": fwd_persistent, "dec_bwd_persistent": bwd_persistent}
    ev_b = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tot_b = [0.0, 0.0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
    ev_x = torch.cuda.Event(enable_timing=True)
    ev_y, tot_y = [torch.cuda.Event(enable_timing=True) for _ in range(2)], 0.0
    tot = [0.0] * len(phases)
    for _ in range(a.iters):
        ev[0].record()
        for i, g in enumerate(graphs[:nstep]):
            g.replay()
            ev[i + 1].record()
        if bwd_persistent:  # backward_mid both ways, each right after a backward_head
            graphs[3].replay()
            ev_b[0].record()
            graphs[n_bwd].replay()
            ev_b[1].record()
            graphs[3].replay()
            ev_b[2].record()
            graphs[4].replay()
            ev_b[3].record()
        if fwd_persistent:  # the chains right after an encoder forward, as the persistent launch above
            graphs[0].replay()
            ev_x.record()
            graphs[nstep].replay()
            ev[nstep + 1].record()
            graphs[0].replay()
            ev_y[0].record()
            graphs[1].replay()
            ev_y[1].record()
        torch.cuda.synchronize()
        for i in range(nstep):
            tot[i] += ev[i].elapsed_time(ev[i + 1])
        if fwd_persistent:
            tot[nstep] += ev_x.elapsed_time(ev[nstep + 1])
            tot_y += ev_y[0].elapsed_time(ev_y[1])
        if bwd_persistent:
            tot_b[0] += ev_b[0].elapsed_time(ev_b[1])
            tot_b[1] += ev_b[2].elapsed_time(ev_b[3])
    for (n, _), t in zip(phases[:nstep + (1 if fwd_persistent else 0)], tot):
        res[n] = round(t / a.iters, 3)
    if fwd_persistent:
        res["decoder_fwd_queued"] = round(tot_y / a.iters, 3)
    if bwd_persistent:
        res["backward_mid_chains"] = round(tot_b[0] / a.iters, 3)
        res["backward_mid_queued"] = round(tot_b[1] / a.iters, 3)
    res["total"] = round(sum(tot[:nstep]) / a.iters, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
