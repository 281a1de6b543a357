"""Execution choices of the HIP engine: ONE documented object instead of scattered
environment reads.

Every field has a measured-best default (``auto`` ones depend on the shape and are resolved by
the engine).  ``EngineConfig.from_env()`` reads the ``TSAMD_*`` variables below (once, when an
engine is built); code can also pass a config explicitly.

| Variable                  | Field              | Default / meaning |
|---------------------------|--------------------|-------------------|
| TSAMD_LSTM_PERSISTENT     | persistent_lstm    | 1: one persistent weight-resident launch per bi-LSTM pass; 0: per-step kernels |
| TSAMD_DEC_PERSISTENT      | dec_persistent     | 1: the decoder forward loop as one persistent launch with per-tile hand-offs when ``dec_persistent_eligible`` (hidden 256, emb 128, projected row attention, B % 16 == 0, the whole grid co-resident); 0 or not eligible: three launches per step and row group |
| TSAMD_DEC_BWD_PERSISTENT  | dec_bwd_persistent | 1: the decoder backward loop as one persistent launch with per-tile hand-offs when ``dec_bwd_persistent_eligible`` (the forward's shape and capacity rule, and no vocab-dW side stream beside the loop); 0 or not eligible: three launches per step and row group |
| TSAMD_ROW_ATTN            | row_attn           | auto (B >= 64): one workgroup per row; 0 / 1 force |
| TSAMD_SPLIT               | split              | auto (2 groups from B = 256, 4 from B = 1024): decoder row groups on parallel streams (forward loop: only when the persistent decoder launch is off or not eligible) |
| TSAMD_SPLIT_BWD           | split_bwd          | auto (= split): row groups of the decoder backward loop |
| TSAMD_FUSED_VOCAB_TRAIN   | fused_vocab_train  | 1: training vocab head with the logits only in MFMA accumulators; 0: library GEMM + ptr_loss |
| TSAMD_FUSED_VOCAB         | fused_vocab_decode | 1: decode vocab head + top-k fused; 0: GEMM + final_topk |
| TSAMD_PROJ_ATTN           | proj_attn          | 1: training row attention streams G = enc_out . W_in[E:] (emb_dim wide) instead of enc_out; 0: enc_out |
| TSAMD_SKIP_PAD_STEPS      | skip_pad_steps     | 1: the projected-context attention kernels skip (row, step) pairs past the row's last loss-weighted decoder step; 0: compute them |
| TSAMD_DEC_ROW_ATTN        | decode_row_attn    | 1: beam-decode attention through the row kernel; 0: score + softmax kernels |
| TSAMD_COMPACT_VOCAB_GRAD  | compact_vocab_grad | 1: with skip_pad_steps, the vocab-head dlogits of the live 32-row blocks are written compacted and the two gradient GEMMs run over those rows only (bucketed block counts); 0: every row |
| TSAMD_DEFER_WGRAD         | defer_wgrad        | 1: decoder-side weight gradients beside the encoder BPTT (B >= 256); 0: inline |
| TSAMD_DETERMINISTIC       | deterministic      | 0; 1: fixed-order reductions instead of fp32 atomics (bit-reproducible steps) |
| TSAMD_KERNEL_DEBUG        | (ops loader)       | 0; 1: the bounds-checked kernel library ``_C_debug.so`` |
"""
from __future__ import annotations

import os
from dataclasses import dataclass, fields, replace
from typing import Dict, Mapping, Optional, Tuple


def _flag(env: Mapping[str, str], name: str, default: bool) -> bool:
    v = env.get(name, "")
    return default if v == "" else v != "0"


def _tri(env: Mapping[str, str], name: str) -> Optional[bool]:
    v = env.get(name, "")
    return None if v == "" else v != "0"


@dataclass(frozen=True)
class EngineConfig:
    persistent_lstm: bool = True
    dec_persistent: bool = True
    dec_bwd_persistent: bool = True
    row_attn: Optional[bool] = None
    split: int = 0
    split_bwd: int = 0
    fused_vocab_train: bool = True
    fused_vocab_decode: bool = True
    proj_attn: bool = True
    skip_pad_steps: bool = True
    decode_row_attn: bool = True
    compact_vocab_grad: bool = True
    defer_wgrad: bool = True
    deterministic: bool = False

    @classmethod
    def from_env(cls, env: Optional[Mapping[str, str]] = None, **overrides) -> "EngineConfig":
        env = os.environ if env is None else env
        cfg = cls(
            persistent_lstm=_flag(env, "TSAMD_LSTM_PERSISTENT", True),
            dec_persistent=_flag(env, "TSAMD_DEC_PERSISTENT", True),
            dec_bwd_persistent=_flag(env, "TSAMD_DEC_BWD_PERSISTENT", True),
            row_attn=_tri(env, "TSAMD_ROW_ATTN"),
            split=int(env.get("TSAMD_SPLIT", "0") or 0),
            split_bwd=int(env.get("TSAMD_SPLIT_BWD", "0") or 0),
            fused_vocab_train=_flag(env, "TSAMD_FUSED_VOCAB_TRAIN", True),
            fused_vocab_decode=_flag(env, "TSAMD_FUSED_VOCAB", True),
            proj_attn=_flag(env, "TSAMD_PROJ_ATTN", True),
            skip_pad_steps=_flag(env, "TSAMD_SKIP_PAD_STEPS", True),
            decode_row_attn=_flag(env, "TSAMD_DEC_ROW_ATTN", True),
            compact_vocab_grad=_flag(env, "TSAMD_COMPACT_VOCAB_GRAD", True),
            defer_wgrad=_flag(env, "TSAMD_DEFER_WGRAD", True),
            deterministic=_flag(env, "TSAMD_DETERMINISTIC", False),
        )
        return replace(cfg, **overrides) if overrides else cfg

    def as_dict(self):
        return {f.name: getattr(self, f.name) for f in fields(self)}


# team scheme and shape rule of csrc/kernels/decoder_persistent.hip (tests/test_gpu_dec_persistent.py compares them)
DEC_PERSISTENT_TEAM = 16  # workgroups per 16-row tile
DEC_PERSISTENT_SHAPE = (256, 128, 512)  # (H, E, A)
DEC_PERSISTENT_MAX_T = 2048

# hand-off timeout codes (csrc/kernels/handoff.h, kErr*) -> (the kernel, its env switch, its EngineConfig field)
HANDOFF_CODES: Dict[int, Tuple[str, str, str]] = {
    1: ("persistent LSTM", "TSAMD_LSTM_PERSISTENT", "persistent_lstm"),
    2: ("persistent LSTM", "TSAMD_LSTM_PERSISTENT", "persistent_lstm"),
    3: ("persistent decoder forward", "TSAMD_DEC_PERSISTENT", "dec_persistent"),
    4: ("persistent decoder backward", "TSAMD_DEC_BWD_PERSISTENT", "dec_bwd_persistent"),
}


def handoff_error_message(code: int) -> Optional[str]:
    """The message for a hand-off error word: None for 0 (no timeout)."""
    if not code:
        return None
    if code not in HANDOFF_CODES:
        return f"a persistent kernel's hand-off timed out (unknown code {code}); results of that launch were discarded"
    what, env, field = HANDOFF_CODES[code]
    return (f"{what} hand-off timed out (code {code}: a workgroup was not co-resident); results of that launch "
            f"were discarded -- set {env}=0 (EngineConfig.{field})")


def fits_resident(grid: int, capacity: int, world: int, reserve_cus: int) -> bool:
    """Whether a grid whose workgroups wait for each other is co-resident: it fits ``capacity`` (the
    occupancy query's resident workgroup count, 0 without a device), less ``reserve_cus`` (the CUs
    an in-flight RCCL collective may hold) when there is more than one rank."""
    return 0 < grid <= capacity - (reserve_cus if world > 1 else 0)


def dec_persistent_grid(B: int) -> int:
    """Workgroups of the persistent decoder launch: teams of 16 dealt 8 at a time (one per XCD)."""
    if B < 16 or B % 16:
        return 0
    return 8 * DEC_PERSISTENT_TEAM * (-(-(B // 16) // 8))


def dec_persistent_eligible(H: int, E: int, A: int, B: int, T: int, proj_attn: bool, row_attn: bool,
                            world: int = 1, capacity: int = 0, reserve_cus: int = 0) -> bool:
    """Whether the decoder forward loop may run as ONE persistent launch (pure function of the
    shape, the attention path, the world size and the device's resident capacity).

    The kernel covers the headline family only (hidden 256, emb 128, A = 512, projected row
    attention, whole 16-row tiles) and its workgroups wait for each other (``fits_resident``).
    Not eligible means the three-kernel chains, never an error.

    Invariant behind ``capacity``: it is one workgroup per CU of the whole device, and at the
    headline batch of 256 the grid equals it with no margin.  That holds only while the launch has
    the device to itself: the decoder forward runs on the step's single stream with nothing beside
    it (the side streams of the step -- deferred weight gradients, the vocab dW -- all live in the
    backward; the input copy stream carries DMA copies only), and no CU mask is in force.  Anything that may hold CUs during the forward (a new
    side stream beside it, a CU mask, another process's kernels) must come off ``capacity`` here, as
    RCCL's CUs do, or workgroups wait for unscheduled peers until the hand-off timeout."""
    if not (proj_attn and row_attn):
        return False
    if (H, E, A) != DEC_PERSISTENT_SHAPE or not 1 <= T <= DEC_PERSISTENT_MAX_T:
        return False
    return fits_resident(dec_persistent_grid(B), capacity, world, reserve_cus)  # (grid 0: B is not whole tiles)


def dec_bwd_persistent_eligible(H: int, E: int, A: int, B: int, T: int, proj_attn: bool, row_attn: bool,
                                world: int = 1, capacity: int = 0, reserve_cus: int = 0,
                                dw_side: bool = False) -> bool:
    """Whether the decoder backward loop may run as ONE persistent launch
    (csrc/kernels/decoder_bwd_persistent.hip): the forward's shape and capacity rule, with
    ``capacity`` the occupancy query of the backward kernel, plus what may hold a CU beside the
    loop in the backward phase it runs in:

    * the vocab dW side stream (``dw_side``: the graph trainer's TSAMD_VOCAB_DW_SIDE) runs a GEMM
      beside the loop, so the launch is not eligible with it;
    * with more than one rank, bucket 0's all-reduce overlaps this phase, so ``reserve_cus`` comes
      off the capacity exactly as for the forward;
    * weight gradients that are not deferred run before the loop on the same stream, and the
      deferred ones start after it (they wait for the main stream), so neither holds a CU beside it.

    Not eligible means the three-kernel chains, never an error."""
    if dw_side:
        return False
    return dec_persistent_eligible(H, E, A, B, T, proj_attn, row_attn, world, capacity, reserve_cus)
