"""The engine's per-batch inputs on the host (pure numpy; torch for dtype names only): what the
forked loader and stream-packer processes need of the engine, without its module or the ops."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

F32 = torch.float32


def host_inputs(batch, hps, D: int, sort_rows: bool = False, need_grad: bool = True,
                row_scale: Optional[np.ndarray] = None, cov_scale: Optional[np.ndarray] = None
                ) -> Dict[str, np.ndarray]:
    """The engine's per-batch inputs as host arrays (pure numpy: runs in loader worker
    processes too): token ids, lengths, the reversed-index map of the backward LSTM
    direction, extended-vocab ids, step-major decoder inputs / targets and the per-(step,
    row) loss weights of the reference's loss averaging (``model.py:252-268``).

    ``sort_rows``: the engine's rows are the batch's rows ordered by live decoder steps, longest
    first (stable), so the steps a row skips past its summary form a suffix of the rows at every
    decoder step and whole 16-row tiles of the decoder kernels go idle together.  The loss is a
    sum over rows; ``row_src[b]`` is the batch row of engine row b.

    ``need_grad`` False (decode / eval packs): the embedding-gradient id order is not computed
    (zeros; no backward reads it) -- the largest host cost of a serving batch.

    ``row_scale`` / ``cov_scale`` ([B] floats, batch row order; None = 1): per-row multipliers of the
    loss weights ``rowg`` and of the coverage-loss weights ``gcl``, applied after the normalisation
    above and before the row sort (train/scst.py weighs sample rows by their advantage with them; a
    weight may be negative).  A row whose weights are all 0 is skipped like a padded row."""
    T = batch.enc_batch.shape[1]
    lens = batch.enc_lens.astype(np.int64)
    if lens.min() < 1:
        raise ValueError("empty article in batch")
    t = np.arange(T)[None, :]
    rev = np.where(t < lens[:, None], lens[:, None] - 1 - t, t)
    valid = batch.valid.astype(np.float64)
    nvalid = valid.sum()
    if batch.dec_batch.shape[1] < D:
        raise ValueError(f"batch has {batch.dec_batch.shape[1]} decoder steps, engine needs {D}")
    dm = batch.dec_padding_mask[:, :D].astype(np.float64)
    dec_lens = dm.sum(1)
    if hps.pointer_gen:
        rowg = dm * (valid / (np.maximum(dec_lens, 1) * nvalid))[:, None]
    else:  # sequence_loss: sum(mask*CE)/sum(mask)
        wm = dm * valid[:, None]
        rowg = wm / wm.sum()
    gcl = hps.cov_loss_wt * dm * (valid / (np.maximum(dec_lens, 1) * nvalid))[:, None]
    if row_scale is not None:
        rowg = rowg * _row_scale(row_scale, len(valid), "row_scale")[:, None]
    if cov_scale is not None:
        gcl = gcl * _row_scale(cov_scale, len(valid), "cov_scale")[:, None]
    # live decoder steps per row: 1 + the last step with a nonzero loss weight (0: none).  Steps
    # past it reach only masked loss terms (model.py:252-268), so their forward values and
    # gradients need not be computed (EngineConfig.skip_pad_steps)
    live = (rowg != 0) | (gcl != 0)  # [B, D]
    dlen = np.where(live.any(1), D - np.argmax(live[:, ::-1], 1), 0)
    src = np.argsort(-dlen, kind="stable") if sort_rows else np.arange(len(dlen))
    enc_batch, ext, rev = batch.enc_batch[src], batch.enc_batch_extend_vocab[src], rev[src]
    enc_lens, rowg, gcl, dlen = batch.enc_lens[src], rowg[src], gcl[src], dlen[src]
    dec_t = np.ascontiguousarray(batch.dec_batch[src, :D].T).astype(np.int64)
    if need_grad:
        sid, perm = emb_sort(enc_batch, dec_t)
    else:
        sid = perm = np.zeros(enc_batch.size + dec_t.size, dtype=np.int32)
    # the fused vocab head's 32-row blocks of the t-major [D * B] rows that hold a live row, listed
    # first (vblk, vblk_n of them); vlive per block (the blocks pass 2 must keep zeroed)
    nb = (D * len(dlen) + 31) // 32
    lr = np.zeros(nb * 32, dtype=bool)
    lr[:D * len(dlen)] = (np.arange(D)[:, None] < dlen[None, :]).reshape(-1)
    vlive = lr.reshape(nb, 32).any(1)
    vblk = np.full(nb, nb, dtype=np.int32)  # past vblk_n: the dummy (all-zero) block nb of the compacted head
    live_ids = np.nonzero(vlive)[0]
    vblk[:len(live_ids)] = live_ids
    return {
        "enc_batch": enc_batch.astype(np.int64),
        "enc_lens": enc_lens.astype(np.int32),
        "rev_idx": rev.astype(np.int64),
        "ext": ext.astype(np.int32),
        "dec_batch_t": dec_t,
        "target_t": np.ascontiguousarray(batch.target_batch[src, :D].T).astype(np.int32),
        "rowg": np.ascontiguousarray(rowg.T).astype(np.float32),
        "gcl": np.ascontiguousarray(gcl.T).astype(np.float32),
        "emb_sid": sid,
        "emb_perm": perm,
        "dlen": dlen.astype(np.int32),
        "row_src": src.astype(np.int32),
        "vlive": vlive.astype(np.int32),
        "vblk": vblk,
        "vblk_n": np.array([len(live_ids)], dtype=np.int32),
    }


def _row_scale(x, B: int, name: str) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (B,) or not np.isfinite(x).all():
        raise ValueError(f"{name}: {B} finite per-row multipliers expected")
    return x


def emb_sort(enc_batch: np.ndarray, dec_t: np.ndarray):
    """Stable id order of the step's embedding-gradient rows: the encoder tokens (row b*T + t)
    then the decoder inputs (row B*T + t*B + b).  Returns (sorted ids, row permutation), int32.

    Computed on the host with the batch (a loader worker process when one is used) instead of
    a device sort inside the captured backward: torch.sort of more than ~1M keys (rocprim's
    onesweep radix sort) faulted the GPU on the second replay of the captured graph at config #5
    batch 2048 (memory-aperture violation at that kernel, three runs; the same step eager and
    kernel-serialised ran clean: profiles/r3/b2048_fault.md).  The stable order also makes the
    gradient's per-id summation order a function of the batch alone (deterministic mode)."""
    ids = np.concatenate([np.asarray(enc_batch).reshape(-1), np.asarray(dec_t).reshape(-1)])
    if ids.size and (ids.min() < 0 or ids.max() >= 2 ** 31):
        raise ValueError("token ids out of range")
    # numpy's stable sort is a radix sort for 16-bit keys: ~5 ms for 230k ids, 28 ms for 1.8M
    key = ids.astype(np.uint16) if ids.size == 0 or ids.max() < 65536 else ids.astype(np.int32)
    perm = np.argsort(key, kind="stable").astype(np.int32)
    return ids[perm].astype(np.int32), perm


_NP = {torch.long: np.int64, torch.int32: np.int32, F32: np.float32}


def input_layout(B: int, T: int, D: int):
    """Byte layout of the engine's input pack: [(name, offset, shape, torch dtype, nbytes)],
    total size (every array 256-byte aligned); the device copy is one buffer with views."""
    shapes = {"BT": (B, T), "B": (B,), "DB": (D, B), "R": (B * T + D * B,), "VB": ((D * B + 31) // 32,), "1": (1,)}
    layout, off = [], 0
    for name, sk, dt in (("enc_batch", "BT", torch.long), ("enc_lens", "B", torch.int32),
                         ("rev_idx", "BT", torch.long), ("ext", "BT", torch.int32),
                         ("dec_batch_t", "DB", torch.long), ("target_t", "DB", torch.int32),
                         ("rowg", "DB", F32), ("gcl", "DB", F32),
                         ("emb_sid", "R", torch.int32), ("emb_perm", "R", torch.int32), ("dlen", "B", torch.int32),
                         ("row_src", "B", torch.int32), ("vlive", "VB", torch.int32), ("vblk", "VB", torch.int32),
                         ("vblk_n", "1", torch.int32)):
        shp = shapes[sk]
        nb = int(np.prod(shp)) * np.dtype(_NP[dt]).itemsize
        layout.append((name, off, shp, dt, nb))
        off += (nb + 255) // 256 * 256
    return layout, off


def pack_host_inputs(host: Dict[str, np.ndarray], layout, out: Optional[np.ndarray] = None) -> np.ndarray:
    """host_inputs arrays -> one uint8 buffer in ``layout`` order (``out`` if given)."""
    if out is None:
        out = np.zeros(layout[-1][1] + (layout[-1][4] + 255) // 256 * 256, dtype=np.uint8)
    for name, o, shp, dt, nb in layout:
        a = np.ascontiguousarray(host[name], dtype=_NP[dt])
        if a.shape != tuple(shp):
            raise ValueError(f"input {name}: shape {a.shape} != {tuple(shp)}")
        out[o:o + nb] = a.reshape(-1).view(np.uint8)
    return out
