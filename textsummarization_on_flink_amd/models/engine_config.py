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
| TSAMD_VOCAB_PAD           | vocab_pad          | 1 (fused vocab head): dlogits rows and the bf16 output-projection weight padded to Vp = 128-aligned columns (the pad columns stay zero: allocated zeroed, never written), so the two vocab-gradient GEMMs run at an aligned K / N -- dX = dlogits . W^T on the split-K hand-written GEMM (headline: 566 -> 426 us) or the library (config #5: 7.88 -> 6.76 ms), dW = X^T . dlogits on the library into a [H][Vp] scratch (653 -> 502 us with the copy) (tools/vocab_grad_micro.py, profiles/r6/vocab_grad.md); 0: unpadded [N][V] |
| TSAMD_CTX_NATIVE          | ctx_native         | 1: the three batched attention-context GEMMs (ctx = a . enc_out, its gradients dA = dctx . enc_out^T and dE = a^T . dctx) on the hand-written ctx_bmm.hip kernels (step-major outputs, no tr01 pass); 0: torch.bmm + tr01 |
| TSAMD_DE_BF16             | de_bf16            | 1 (with the native context kernels and the persistent BPTT): the encoder-output gradient dE = a^T . dctx + dF . W_h^T kept in bf16 -- ctx_de writes a^T . dctx in bf16, the W_h GEMM adds into it (beta = 1, bf16 in and out), the top layer's BPTT reads it; 0: an fp32 [B][T][A] buffer written, re-read and rewritten, and read again (profiles/r6/de_bf16.md) |
| TSAMD_DX_MERGE            | dx_merge           | 1: the input gradients of an upper encoder layer as one hand-written GEMM per output direction over the concatenated [dz_fw, dz_bw], rows gathered through the reversed index, written straight into the lower layer's step frame (gemm_mfma.hip AMODE 2; needs ``gemm_dispatch.BLT`` and ``GEMM_BT`` != "0"); 0: two per-direction GEMMs + step_frame_hop.  Config #5 at batch 2048: same step time (391.8 vs 391.9 ms), 14 GB less memory (no per-direction dxs).  Layer 0 keeps the library GEMMs + from_step_frame: its merged GEMM (N = E = 128, one 128-column tile) measured 0.1 ms slower at batch 256 (profiles/r5/dx_merge.md) |
| TSAMD_LSTM_FX             | lstm_fx            | 1: encoder layer 0's input projection x.W_x inside the persistent recurrence (lstm_persistent.hip FX): the step-frame inputs (bf16, E = 128) are gathered once and each step's x MFMAs run in the shadow of the hand-off wait -- no gx GEMM, no gx buffer; 0: a GEMM writes gx (fp32 [2][T][B][4H]) before the recurrence |
| TSAMD_VOCAB_DW_SIDE       | vocab_dw_side      | 0; 1 (graph trainer): the vocab weight gradient dW = X^T . dlogits leaves the vocab-backward graph for a graph of its own, replayed on a side stream beside the decoder backward loop (train/trainer.py _Phase1).  Measured at the headline: phase 0 -0.4 ms, phase 1 +0.4 ms -- the loop's step kernels wait behind the GEMM's workgroups and share its HBM stream; CU-masked and low-priority side streams were slower still (profiles/r6/vocab_dw_side.md) |
| TSAMD_BLT_VOCAB_DW        | blt_vocab_dw       | 0: the vocab dW as a split-K batched GEMM; 1: through blt_mm (effective only with ``gemm_dispatch.BLT``) |
| (none)                    | vocab_dw_split_min | 1e12: K.M.N above which the padded vocab dW keeps the 4-way split-K batched GEMM (config #5: 8.2 ms against 9.5 ms for the library at the padded N) |
| TSAMD_KERNEL_DEBUG        | (ops loader)       | 0; 1: the bounds-checked kernel library ``_C_debug.so`` |

The process-wide GEMM switches (TSAMD_BLT, TSAMD_BLT_WGRAD, TSAMD_GEMM_BT, TSAMD_WGRAD_TT,
TSAMD_WGRAD_TT_MIN) are globals of ``gemm_dispatch``, read at its import.
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


def _on(env: Mapping[str, str], name: str) -> bool:
    """A switch that is off by default and on only at "1"."""
    return env.get(name, "0") == "1"


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
    vocab_pad: bool = True
    ctx_native: bool = True
    de_bf16: bool = True
    dx_merge: bool = True
    lstm_fx: bool = True
    vocab_dw_side: bool = False
    blt_vocab_dw: bool = False
    vocab_dw_split_min: float = 1e12

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
            vocab_pad=_flag(env, "TSAMD_VOCAB_PAD", True),
            ctx_native=_flag(env, "TSAMD_CTX_NATIVE", True),
            de_bf16=_flag(env, "TSAMD_DE_BF16", True),
            dx_merge=_flag(env, "TSAMD_DX_MERGE", True),
            lstm_fx=_flag(env, "TSAMD_LSTM_FX", True),
            vocab_dw_side=_on(env, "TSAMD_VOCAB_DW_SIDE"),
            blt_vocab_dw=_on(env, "TSAMD_BLT_VOCAB_DW"),
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
