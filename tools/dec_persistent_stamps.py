"""Where a decoder step of dec_fwd_persistent spends its time: per-phase clock stamps.

Builds ``_C_stamps.so`` (the kernel library with csrc/kernels/decoder_persistent.hip compiled with
-DTSAMD_DEC_STAMPS; the other objects are those of the normal build), loads it instead of ``_C.so``,
runs the bench-shaped engine (as tools/phase_micro.py) and lets one decoder forward write its stamps:
wave 0 of every workgroup reads the 100 MHz wall clock at eight points of every step,

  0 g received | 1 cell done, [c, h] published | 2 [c, h] received | 3 s published | 4 s received |
  5 position loop done | 6 g published | 7 end of the step's stores.

Prints, in microseconds, the mean of every interval over all live (workgroup, step) pairs, the same
for the slowest team, and one JSON line.  ``--build-only`` stops after the build (object files do
not travel, so build where the normal build ran); ``--lib NAME`` uses another stamped library.

  python tools/dec_persistent_stamps.py [--batch B] [--enc T] [--build-only]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["wait_g", "cell", "wait_ch", "sproj", "wait_s", "attn_loop", "merge_pub_g", "tail_stores"]
TICK_US = 0.01  # wall_clock64: 100 MHz


def build_stamped(lib):
    from textsummarization_on_flink_amd import _build
    so = os.path.join(_build.PKG_DIR, lib)
    src = os.path.join(_build.CSRC, "kernels", "decoder_persistent.hip")
    _build.build_kernels()
    odir = _build.BUILD + "_stamps"
    os.makedirs(odir, exist_ok=True)
    obj = os.path.join(odir, "decoder_persistent.hip.o")
    _build._run([_build.HIPCC, *_build.kernel_flags(), "-DTSAMD_DEC_STAMPS", "-c", src, "-o", obj], False)
    objs = [os.path.join(_build.BUILD, f) for f in sorted(os.listdir(_build.BUILD))
            if f.endswith(".o") and f != "decoder_persistent.hip.o"]
    _build._run([_build.HIPCC, "-shared", "-fPIC", f"--offload-arch={_build.ARCH}", *objs, obj, "-o", so,
                 *_build._torch_flags()[1], "-lhipblaslt"], False)
    return so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--enc", type=int, default=400)
    ap.add_argument("--lib", default="_C_stamps.so")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    pkg = os.path.join(ROOT, "textsummarization_on_flink_amd")
    if a.build_only or not os.path.exists(os.path.join(pkg, a.lib)):
        print(build_stamped(a.lib), flush=True)
        if a.build_only:
            return
    os.environ["TSAMD_C_LIB"] = a.lib  # (read when the ops loader is imported)
    import torch
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.models.params import build_params
    from textsummarization_on_flink_amd.models.pointer_generator import HipPointerGenerator

    V, D = 50000, 100
    hps = HParams(batch_size=a.batch, max_enc_steps=a.enc, max_dec_steps=D, vocab_size=V, hidden_dim=a.hidden,
                  emb_dim=128, coverage=True, pointer_gen=True, enc_layers=1)
    corpus = SyntheticCorpus(vocab_size=V, seed=3)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=a.enc)[0]
    params = build_params(hps, vocab.size(), device="cuda").enable_grad().enable_adagrad(hps.adagrad_init_acc)
    eng = HipPointerGenerator(hps, vocab.size(), params, B=a.batch, T=a.enc)
    assert eng.dec_persistent, "the persistent decoder launch is not in use at this shape"
    eng.set_batch(batch)
    for _ in range(2):
        eng.train_step()
    torch.cuda.synchronize()
    grid = int(eng.k.dec_persistent_grid(a.batch))
    buf = torch.zeros(grid * D * 8, dtype=torch.int32, device="cuda")
    eng._encoder_forward()
    eng._decoder_forward()  # (warm)
    eng.k.dec_persistent_stamps(buf, a.batch, D)
    eng._encoder_forward()
    eng._decoder_forward()
    torch.cuda.synchronize()
    eng.k.dec_persistent_stamps(None, a.batch, D)
    st = buf.view(grid, D, 8).cpu().long() & 0xFFFFFFFF
    live = (st != 0).all(-1)                       # steps the workgroup's row was live for
    live[:, 1:] &= live[:, :-1].clone()
    prev_end = torch.cat([st[:, :1, 0], st[:, :-1, 7]], 1)   # step 0: no g to wait for
    edges = torch.cat([prev_end[..., None], st], -1)
    dur = ((edges[..., 1:] - edges[..., :-1]) & 0xFFFFFFFF).double() * TICK_US  # [grid][D][8]
    blk = torch.arange(grid)
    team = ((blk >> 3) // 16) * 8 + (blk & 7)
    res = {"batch": a.batch, "enc": a.enc, "lib": a.lib, "live_pairs": int(live.sum())}
    mean = (dur * live[..., None]).sum((0, 1)) / live.sum()
    step_by_team = []
    for tm in range(a.batch // 16):
        sel = live & (team == tm)[:, None]
        n = max(int(sel.sum()), 1)
        step_by_team.append((float((dur.sum(-1) * sel).sum() / n), tm, (dur * sel[..., None]).sum((0, 1)) / n))
    worst = max(step_by_team)
    print(f"{'interval':<14}{'mean us':>10}{'worst team us':>16}   (worst team: {worst[1]})")
    for i, n in enumerate(NAMES):
        print(f"{n:<14}{float(mean[i]):>10.2f}{float(worst[2][i]):>16.2f}")
        res[n] = round(float(mean[i]), 3)
        res[n + "_worst"] = round(float(worst[2][i]), 3)
    print(f"{'step':<14}{float(mean.sum()):>10.2f}{worst[0]:>16.2f}")
    res["step"], res["step_worst"], res["worst_team"] = round(float(mean.sum()), 3), round(worst[0], 3), worst[1]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
