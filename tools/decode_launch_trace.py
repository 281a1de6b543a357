"""What a device decoder queues: every op call of ``_encode``, ``_prologue`` and four ``_step``s (eager, the
tiny peaked model of the decode tests), as JSON lines ``[op, [argument, ...]]``, plus the ``zero_`` /
``fill_`` / ``copy_`` calls on the decoder's buffers ``dec.b``.  A tensor is logged as the name under which
the decoder or its engine holds it (matched by address) with shape and dtype, a scalar by value.  Two
trees that print the same lines for a configuration queue the same device work for it:

    python tools/decode_launch_trace.py --hps '{"beam_size": 8, "block_ngram_repeat": 3}' --kw '{"keep_attn": false}'

(engine switches such as TSAMD_FUSED_VOCAB are read from the environment as usual; ``"hidden_dim": 256,
"emb_dim": 128, "max_enc_steps": 64`` is a width at which the row attention and with it the fused step run).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hps", default="{}", help="JSON: HParams fields that differ from the test model's")
    ap.add_argument("--kw", default="{}", help="JSON: decoder keyword arguments (wide_beam, keep_attn)")
    args = ap.parse_args()
    import torch
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    from textsummarization_on_flink_amd.decode.device_beam import device_decoder
    from textsummarization_on_flink_amd.models.params import build_params

    hps = HParams(batch_size=8, max_enc_steps=48, max_dec_steps=20, min_dec_steps=3, beam_size=4, vocab_size=600,
                  emb_dim=64, hidden_dim=64, coverage=True, trunc_norm_init_std=0.5,
                  rand_unif_init_mag=0.3).replace(**json.loads(args.hps))
    V = hps.vocab_size
    corpus = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=2, art_mean=40, art_sd=10, sent_mean=4)
    vocab = corpus.vocab(V)
    batch = make_batches(hps, vocab, corpus, 1, pad_enc_to=hps.max_enc_steps)[0]
    dec = device_decoder(hps, vocab, build_params(hps, vocab.size(), device="cuda", seed=3),
                         n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=False, **json.loads(args.kw))
    log, names = [], {}

    def desc(x):
        if not torch.is_tensor(x):
            return x
        return [names.get(x.data_ptr(), "?"), list(x.shape), str(x.dtype)]

    class Logged(torch.Tensor):  # an entry of dec.b whose fills are logged (same storage: the ops take it as it is)
        __torch_function__ = torch._C._disabled_torch_function_impl

        def zero_(self):
            log.append(("zero_", [desc(self)]))
            return super().zero_()

        def fill_(self, v):
            log.append(("fill_", [desc(self), desc(v)]))
            return super().fill_(v)

        def copy_(self, src, non_blocking=False):
            log.append(("copy_", [desc(self), desc(src)]))
            return super().copy_(src, non_blocking)

    class Ops:  # dec.k with every call logged
        def __getattr__(self, op):
            def call(*a):
                log.append((op, [desc(x) for x in a]))
                return getattr(ops, op)(*a)
            return call

    ops, dec.k = dec.k, Ops()
    for n in dec.b:
        dec.b[n] = dec.b[n].as_subclass(Logged)
    for pre, d in [("p.", dict(dec.p.items())), ("eng.w.", dec.eng.w), ("eng.f32.", dec.eng.f32), ("eng.pk.", dec.eng.pk),
                   ("dec.", vars(dec)), ("st0.", dec.st[0]), ("st1.", dec.st[1]), ("b.", dec.b)]:
        for n, v in d.items():
            for i, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                if torch.is_tensor(t) and t.numel():
                    names[t.data_ptr()] = f"{pre}{n}" + (f"[{i}]" if isinstance(v, (list, tuple)) else "")
    dec._encode(batch)
    dec._prologue()
    for t in range(4):
        dec._step(t % 2)
    torch.cuda.synchronize()
    for rec in log:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
