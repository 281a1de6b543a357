"""GEMM dispatch of the HIP engine: each bf16 GEMM goes to hipBLASLt (``blt_mm``) or to a
hand-written gfx950 kernel (``gemm_bt``, ``wgrad_tt``).  The switches below are process-wide,
as the pick cache and the split-K workspace are: read from the environment at import, and set
in tests on THIS module (nothing re-exports them)."""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch

from ..ops import ops as _ops

BF = torch.bfloat16
F32 = torch.float32

# TSAMD_BLT=0: library GEMMs through torch.mm (hipBLASLt's first heuristic pick) instead of
# blt_mm (csrc/blt_gemm.cpp: hipBLASLt called directly, the fastest of its candidates per shape)
BLT = os.environ.get("TSAMD_BLT", "1") != "0"
# the long-K weight gradients (encoder, vocab dW) through blt_mm too (default: split-K batched GEMM;
# the vocab dW's switch is EngineConfig.blt_vocab_dw)
BLT_WGRAD = BLT and os.environ.get("TSAMD_BLT_WGRAD", "0") == "1"
# TSAMD_GEMM_BT: the hand-written MFMA GEMM (csrc/kernels/gemm_mfma.hip) for the activation GEMMs
# whose weight operand has a [N][K] twin.  "table" (default): a fixed per-shape rule from the
# recorded head-to-head timings (``_bt_rule``; profiles/r5/gemm_micro_v3.jsonl,
# profiles/r6/gemm_dispatch.md) -- the same pick on every run, box and rank; "auto" times it
# against blt_mm once per shape on the first eager call and keeps the faster (the round-5 default:
# picks could differ between runs); "1" always where eligible (deterministic mode too); "0" never
GEMM_BT = os.environ.get("TSAMD_GEMM_BT", "table")
_BT_PICK: Dict[tuple, bool] = {}
_BT_TIMES: Dict[tuple, tuple] = {}
# 2 log2(e): the attention features F = enc_out . W_h are stored multiplied by it (the kernels'
# tanh argument is 2^(K u); attn_common.h fadd_bf2)
K2LOG2E = 2.8853900817779268
# the step-frame gather path replaces to_step_frame + the GEMM: kept while the gather GEMM is at
# most this much slower than the library GEMM alone (the layout pass it saves costs ~25-40 % of it)
FRAME_SLACK = 1.25


def _aligned(t: torch.Tensor) -> bool:
    return t.stride(-1) == 1 and (t.dim() < 2 or t.stride(0) % 8 == 0) and t.data_ptr() % 16 == 0


def _bt_ok(out, sa, ta, Bt, beta, bias) -> bool:
    return (GEMM_BT != "0" and Bt is not None and not ta and Bt.dtype == BF and out.is_cuda and _aligned(sa)
            and _aligned(Bt) and _aligned(out) and beta in (0.0, 1.0) and not (beta and out.dtype == BF)
            and (bias is None or (bias.dtype == F32 and bias.is_contiguous()))
            and bool(_ops().gemm_bt_ok(out.shape[0], out.shape[1], Bt.shape[1])) and sa.shape[1] == Bt.shape[1])


def _deterministic() -> bool:
    return os.environ.get("TSAMD_DETERMINISTIC", "0") not in ("", "0")


def _time_us(fn, reps: int = 3) -> float:
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def _bt_timed(out, sa, Bt, beta, bias, sb, tb):
    """(gemm_bt us, blt_mm us) of this shape on a row subset (<= 131072 rows) into scratch."""
    key = (tuple(out.shape), out.dtype, sa.shape[1], beta != 0.0, bias is not None, sa.stride(0), Bt.stride(0))
    if key not in _BT_TIMES:
        m = min(out.shape[0], 131072)
        a, o = sa[:m], torch.empty(m, out.shape[1], dtype=out.dtype, device=out.device)
        k = _ops()
        t_bt = _time_us(lambda: k.gemm_bt(a, Bt, o, float(beta), bias, None, None, 0, 0, 0, None))
        t_blt = _time_us(lambda: k.blt_mm(a, sb, o, False, tb, float(beta), bias))
        _BT_TIMES[key] = (t_bt, t_blt)
    return _BT_TIMES[key]


def _bt_rule(K: int, out_bf16: bool, slack: float) -> bool:
    """The fixed dispatch (TSAMD_GEMM_BT=table), from the head-to-head records
    (profiles/r5/gemm_micro_v3.jsonl and the round-6 timed picks, profiles/r6/gemm_dispatch.md):
    the hand-written GEMM wins every K <= 256 shape (b256_gx 104 vs 112 us, c5_gx_l0 1340 vs 1443,
    25600 x 128 x 128 8.1 vs 16.2), the bf16-out shapes up to K = 1024 (25600 x 512 x 512 22.2 vs
    29.1, c5_F 1694 vs 1707; b256_F measured both ways across runs) and loses the fp32-out
    K >= 512 shapes (25600 x 256 x 512 28.1 vs 20.4, 102400 x 512 x 512 154 vs 117, c5_dx_l1 3380
    vs 3010) -- within FRAME_SLACK where it also saves the step-frame layout pass."""
    return slack > 1.0 or K <= 256 or (out_bf16 and K <= 1024)


def _use_bt(out, sa, ta, Bt, beta, bias, sb, tb, slack: float = 1.0) -> bool:
    if not _bt_ok(out, sa, ta, Bt, beta, bias):
        return False
    if GEMM_BT == "1" or _deterministic():
        return True
    key = (tuple(out.shape), out.dtype, sa.shape[1], beta != 0.0, bias is not None, sa.stride(0), Bt.stride(0), slack)
    if key not in _BT_PICK:
        if GEMM_BT != "auto":
            _BT_PICK[key] = _bt_rule(sa.shape[1], out.dtype == BF, slack)
        elif torch.cuda.is_current_stream_capturing():
            return False  # first seen inside a capture: no timing possible, keep the library GEMM
        else:
            t_bt, t_blt = _bt_timed(out, sa, Bt, beta, bias, sb, tb)
            _BT_PICK[key] = t_bt <= slack * t_blt
    return _BT_PICK[key]


def gemm_bt_stats() -> Dict[str, object]:
    """The hand-written-GEMM dispatch: mode, every shape seen (M x N x K, out dtype, frame
    gather) with the kernel it got, and (mode "auto") the timings behind the picks."""
    picks = {f"{k[0][0]}x{k[0][1]}x{k[2]}{'_bf16' if k[1] == BF else ''}{'_frame' if k[7] > 1.0 else ''}":
             ("gemm_bt" if v else "hipblaslt") for k, v in _BT_PICK.items()}
    return {"mode": "deterministic" if _deterministic() else GEMM_BT, "shapes": len(_BT_PICK),
            "gemm_bt": int(sum(_BT_PICK.values())), "picks": picks,
            "timed_us": {f"{k[0][0]}x{k[0][1]}x{k[2]}": [round(v[0], 1), round(v[1], 1)] for k, v in _BT_TIMES.items()}}


def _stored(x: torch.Tensor):
    """(row-contiguous tensor holding x's elements, whether x is its transpose)."""
    if x.stride(-1) == 1:
        return x, False
    if x.dim() == 2 and x.stride(0) == 1:
        return x.t(), True
    return x.contiguous(), False


def gemm(out: torch.Tensor, a: torch.Tensor, b: torch.Tensor, beta: float = 0.0,
         bias: Optional[torch.Tensor] = None, bt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = beta * out + a . b (+ bias[N]): bf16 operands, fp32 accumulate, fp32 or bf16 ``out``
    written in place (row slices of bigger buffers included).  Transposed views of stored
    operands are passed as (storage, transpose flag), never copied.  ``bt``: a row-major [N][K]
    twin of ``b`` (a packed weight layout) -- with it, or when ``b`` is itself the transpose of a
    row-major [N][K] matrix, the hand-written MFMA GEMM is eligible (TSAMD_GEMM_BT)."""
    if BLT and out.is_cuda and a.dtype == BF and b.dtype == BF:
        sa, ta = _stored(a)
        sb, tb = _stored(b)
        Bt = sb if tb else bt
        if _use_bt(out, sa, ta, Bt, beta, bias, sb, tb):
            _ops().gemm_bt(sa, Bt, out, float(beta), bias, None, None, 0, 0, 0, None)
            return out
        _ops().blt_mm(sa, sb, out, ta, tb, float(beta), bias)
        return out
    if beta != 0.0:
        assert bias is None
        if out.dtype == F32 and a.dtype == BF:
            return torch.addmm(out, a, b, out_dtype=F32, out=out)
        return out.addmm_(a, b, beta=beta)
    if out.dtype == F32 and a.dtype == BF:
        if bias is None:
            return torch.mm(a, b, out_dtype=F32, out=out)
        return torch.addmm(bias, a, b, out_dtype=F32, out=out)
    if bias is None:
        return torch.mm(a, b, out=out)
    return torch.addmm(bias.to(out.dtype), a, b, out=out)


def mm_into(out: torch.Tensor, a: torch.Tensor, b: torch.Tensor, bias: Optional[torch.Tensor] = None,
            bt: Optional[torch.Tensor] = None):
    """out = a . b (+ bias), fp32 accumulate, written straight into ``out`` (fp32 or bf16)
    -- no temporary, no separate bias pass (GEMM bias epilogue)."""
    return gemm(out, a, b, 0.0, bias, bt)


def wgrad_into(out: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    """out[M,N] = a[K,M]^T . b[K,N] for weight gradients: K (= rows: tokens or decoder steps
    x batch) is long and M x N is a handful of output tiles.  blt_mm picks among hipBLASLt's
    stream-K / split-K solutions per shape.  The torch path (TSAMD_BLT=0) splits K into S
    chunks as one batched GEMM (S x the tiles, fp32 partials) and sums the partials: 3-5x
    faster than torch.mm's pick for K = 25.6k-102k (tools/wgrad_micro.py)."""
    K = a.shape[0]
    if a.is_cuda and BLT_WGRAD and a.dtype == BF:
        return gemm(out, a.t(), b)
    if a.is_cuda:
        for S in ((32, 16, 8) if K >= 65536 else (16, 8)):
            if K % S == 0 and K // S >= 256:
                parts = torch.bmm(a.reshape(S, K // S, a.shape[1]).transpose(1, 2), b.reshape(S, K // S, b.shape[1]),
                                  out_dtype=F32)
                return torch.sum(parts, 0, out=out)
    return out.copy_(mmf(a.t(), b))


WGRAD_TT = os.environ.get("TSAMD_WGRAD_TT", "1") != "0"
WGRAD_TT_MIN = float(os.environ.get("TSAMD_WGRAD_TT_MIN", 1e11))
_WG_WS: Dict[object, torch.Tensor] = {}
_WG_WS_OLD: List[torch.Tensor] = []


def wgrad_enc_into(out: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    """Long-K weight gradients out = a^T . b: the encoder's x^T.dz / h^T.dz (K = T.B tokens:
    102k at the headline, 1.6M at config #5) and the inline decoder-side ones (K = D.B): the
    hand-written deterministic split-K GEMM (wgrad.hip ``wgrad_tt``: fp32 slabs summed in split
    order, no atomics, no torch.sum pass) where the shape fits it and is large, else
    ``wgrad_into``.  Its slab workspace is one buffer per device, grown outside graph capture
    (the trainer's eager warm-up) and reused by the captured graphs: these calls run one after
    another on the backward stream (model.py:290-297 / 89-93 gradients)."""
    # large shapes only (config #5: K.M.N >= 3e11); at the headline's K = 102k the split-K bmm is
    # as fast or faster (profiles/r6/wgrad_tt.md)
    if (WGRAD_TT and a.is_cuda and a.dtype == BF and b.dtype == BF and out.dtype == F32
            and a.shape[0] * a.shape[1] * b.shape[1] >= WGRAD_TT_MIN):
        k = _ops()
        n = int(k.wgrad_tt_ws(a.shape[1], b.shape[1], a.shape[0]))
        if n > 0:
            key = out.device
            ws = _WG_WS.get(key)
            if ws is None or ws.numel() < n:
                if torch.cuda.is_current_stream_capturing():
                    return wgrad_into(out, a, b)  # first seen inside a capture: no allocation there
                if ws is not None:  # graphs captured earlier may hold the old buffer: never freed
                    _WG_WS_OLD.append(ws)
                ws = _WG_WS[key] = torch.empty(n, device=out.device, dtype=F32)
            if k.wgrad_tt(a, b, out, ws, False):
                return out
    return wgrad_into(out, a, b)


def mmf(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """bf16 x bf16 -> fp32 GEMM (fp32 accumulate), hipBLASLt."""
    if BLT and a.is_cuda:
        return gemm(torch.empty(a.shape[0], b.shape[1], device=a.device, dtype=F32), a, b)
    if not a.is_cuda:  # (the out_dtype matmul is GPU-only)
        return a.float() @ b.float()
    return torch.mm(a, b, out_dtype=F32)
