"""The MFMA GEMM kernels (csrc/kernels/gemm_mfma.hip, wgrad.hip, ctx_bmm.hip) one by one against float64 torch:
gemm_bt (plain rows, step-frame gather with the xsf copy), gemm_bt_merge, gemm_bt_splitk, wgrad_tt (plain, swapped,
direct, narrow nv, both slab sums), wgrad_tn, ctx_fwd, ctx_da, ctx_de.  Every op is called through ops(); the
reference is a float64 matmul on the CPU of the bf16 operand values the kernel receives, upcast, with the gather /
merge index arithmetic written as plain loops; no reference goes through another kernel or an fp32 matmul.

Two kinds of input for every case.
  exact    operands integer-valued bf16 in [-8, 8] (att: multiples of 2^-6 in [0, 1]), bias / prefill integers.  Every
           product and partial sum is then an integer (a multiple of 2^-6) below 2^24 units (_assert_exact, on the
           reference), so the fp32 result is exact in ANY accumulation order: the output must equal the reference in
           every element (fp32), or the reference rounded once (bf16).
  general  randn operands scaled as in tests/test_gpu_gemm.py.  Per element, U = 2^-24:
               (K + 4) U sum_k |a_k b_k|                        a sum of K fp32 terms in any order
             + S U sum_k |a_k b_k|                              an S-way slab sum (wgrad_tn: S atomic adds onto the prefill,
                                                                so its magnitude is added; they are its acc add)
             + U (|running value| + bound so far)               one rounding per beta / acc / bias add, in kernel order
             + 2^-8 |ref + addends|                             a bf16 output
           sum_k |a_k b_k| is the float64 reference's.  A zero bound requires a zero error.  Nothing is measured.

Slack and sentinels.  Operands are views into larger NaN-filled allocations (columns K .. of every row, rows M .. of A,
the rows around a Bt row slice, table rows no id references, the workspaces); outputs are views into allocations
prefilled with NaN (stores) or 12288.0 (accumulates), a 4096-element block before and behind and, for ldc > N, columns
on both sides; every byte outside the output view must be bit-identical afterwards.  The deterministic paths are
bit-identical on a second run, wgrad_tn (atomics) on the exact inputs.

The runners below take the op table k (ops(), or the Emu class: fp32 torch in 64-wide K blocks with the gather, merge
and split logic in plain Python) and the device, so tests/test_gemm_ops_checks.py runs the same checks on the CPU with
the emulation and with one-line mistakes planted in it.  profiles/gemm_op_tests.md lists which launcher line each
shape exercises."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U24 = 2.0 ** -24
PAD = 4096
SENT = 12288.0  # exact in bf16
KINDS = ("exact", "general")


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _gen(*key):
    s = 0
    for v in key:
        s = (s * 1000003 + int(v) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _bits(t):
    return t.view({BF: torch.int16, F32: torch.int32}[t.dtype])


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ------------------------------------------------------------------ inputs
def _vals(g, shape, kind, scale=1.0):
    if kind == "exact":
        return torch.randint(-8, 9, tuple(shape), generator=g).float().bfloat16()
    return (torch.randn(tuple(shape), generator=g) * scale).bfloat16()


def _att(g, shape, kind):
    if kind == "exact":
        return (torch.randint(0, 65, tuple(shape), generator=g).float() / 64).bfloat16()
    return torch.rand(tuple(shape), generator=g).bfloat16()


def _addend(g, shape, kind, hi=8):
    """fp32 bias / prefill: integers (exact) or randn"""
    if kind == "exact":
        return torch.randint(-hi, hi + 1, tuple(shape), generator=g).float()
    return torch.randn(tuple(shape), generator=g)


def _in2d(vals, dev, ld_extra=8, before=0, after=2):
    """vals as rows before .. before + R of a NaN-filled [before + R + after][C + ld_extra] allocation"""
    R, C = vals.shape
    full = torch.full((before + R + after, C + ld_extra), NAN, dtype=vals.dtype)
    full[before:before + R, :C] = vals
    return full.to(dev)


def _inflat(vals, dev, pad=64):
    """a contiguous operand as a slice of a NaN-padded flat allocation"""
    flat = torch.full((2 * pad + vals.numel(),), NAN, dtype=vals.dtype)
    flat[pad:pad + vals.numel()] = vals.reshape(-1)
    return flat.to(dev)[pad:pad + vals.numel()].view(vals.shape)


class Out:
    """An [M][N] output view (row stride ldc, column offset c0, element shift) inside a sentinel-filled flat
    allocation with PAD elements before and behind."""

    def __init__(self, M, N, dtype, fill, dev, ldc=None, c0=0, shift=0, prefill=None):
        ldc = ldc or N
        n = 2 * PAD + shift + M * ldc
        body = slice(PAD + shift, PAD + shift + M * ldc)
        self.mask = torch.zeros(n, dtype=torch.bool)
        self.mask[body].view(M, ldc)[:, c0:c0 + N] = True
        self.flat = torch.full((n,), fill, dtype=dtype).to(dev)
        self.view = self.flat[body].view(M, ldc)[:, c0:c0 + N]
        if prefill is not None:
            self.view.copy_(prefill)
        self.before = _bits(self.flat).cpu().clone()

    def intact(self, tag, untouched=False):
        now = _bits(self.flat).cpu()
        bad = now != self.before
        if not untouched:
            bad &= ~self.mask
        assert not bool(bad.any()), f"{tag}: sentinel: {int(bad.sum())} elements outside the output changed, first at flat " \
                                    f"index {int(bad.nonzero()[0])} (output body starts at {PAD})"


def wide(N, on):
    """ldc > N with sentinel columns on both sides"""
    return dict(ldc=N + 24, c0=8) if on else {}


# ------------------------------------------------------------------ reference and checks
def _mmref(A, Bt):
    """A [M][K], Bt [N][K] -> the float64 product and sum_k |a_k b_k|"""
    A, Bt = A.double(), Bt.double()
    return A @ Bt.t(), A.abs() @ Bt.abs().t()


def _assert_exact(K, maxterm, unit, ref, mag, full):
    """every term a multiple of 1 / unit below maxterm units, K of them: every partial sum below 2^24 units"""
    assert K * maxterm < 2 ** 24
    assert float(mag.max()) * unit <= K * maxterm
    assert torch.equal((ref * unit).round(), ref * unit) and torch.equal((full * unit).round(), full * unit)
    assert float(full.abs().max()) * unit + float(mag.max()) * unit < 2 ** 24
    assert torch.equal(full.float().double(), full)


def _check(tag, got, ref, mag, K, kind, adds=(), slabs=0, slab_mag=None, out_bf16=False, unit=1, add_rounds=True):
    """got against ref + sum(adds) (adds in the kernel's order): exact inputs bit for bit, general inputs within the
    bound of the module docstring.  add_rounds=False: the adds are made by the slab sum's own roundings."""
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == (BF if out_bf16 else F32), (tag, got.shape, got.dtype)
    full = ref.clone()
    for a in adds:
        full = full + a.double()
    if kind == "exact":
        _assert_exact(K, 64 * (8 if unit == 64 else 1), unit, ref, mag, full)
        want = full.float().bfloat16() if out_bf16 else full.float()
        bad = ~(got == want)  # torch.equal, element by element; a NaN differs
        if bool(bad.any()):
            at = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{tag}: exact: {int(bad.sum())} of {bad.numel()} elements differ, first at {list(at)}: "
                                 f"got {float(got[at])}, want {float(want[at])}")
        return
    bound = (K + 4) * U24 * mag
    if slabs:
        bound = bound + slabs * U24 * (mag if slab_mag is None else slab_mag)
    run = ref
    for a in adds if add_rounds else ():
        run = run + a.double()
        bound = bound + U24 * (run.abs() + bound)
    if out_bf16:
        bound = bound + 2.0 ** -8 * full.abs()
    err = (got.double() - full).abs()
    ok = err <= bound  # a NaN fails; a zero bound requires a zero error
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).nan_to_num(nan=float("inf")).max()) if bool(pos.any()) else 0.0
    print(f"ERR/BOUND {tag} {ratio:.4f}")
    assert bool(ok.all()), f"{tag}: bound: {int((~ok).sum())} of {ok.numel()} elements outside the bound, largest err / " \
                           f"bound {ratio:.3g}, first at {(~ok).nonzero()[0].tolist()}"


def old_max_norm_error(got, full):
    """the measure of tests/test_gpu_gemm.py / test_gpu_ctx.py"""
    return float((got.detach().cpu().double() - full).abs().max() / full.abs().max().clamp_min(1e-30))


def _same_bits(tag, a, b):
    assert torch.equal(_bits(a.detach().cpu().contiguous()), _bits(b.detach().cpu().contiguous())), f"{tag}: rerun: not bit-identical"


# ------------------------------------------------------------------ host-side split rules (ports of the launchers')
def splits_bt(M, N, K):
    """gemm_bt_splits (gemm_mfma.hip)"""
    BN = 256 if N % 256 == 0 else 128
    tiles, steps = ((M + 255) // 256) * (N // BN), K // 64
    s = min(256 // tiles, steps // 16)
    if s < 2:
        return 1
    kc = (steps + s - 1) // s
    return (steps + kc - 1) // kc


def splits_tt(M, N, K):
    """wgrad_tt_splits (wgrad.hip)"""
    BN = 256 if N % 256 == 0 else 128
    tiles, steps = (M // 256) * (N // BN), K // 64
    s = max(1, min((256 + tiles - 1) // tiles, steps))
    kc = (steps + s - 1) // s
    return (steps + kc - 1) // kc


def splits_tn(M, N, K):
    """launch_wgrad_tn's number of K chunks"""
    tiles = (M // 128) * ((N + 127) // 128)
    s = max(1, min((512 + tiles - 1) // tiles, (K + 511) // 512))
    kchunk = ((K + s - 1) // s + 63) // 64 * 64
    return (K + kchunk - 1) // kchunk


def _tt_ok(M, N, K):
    return M % 256 == 0 and N % 128 == 0 and K % 64 == 0 and K >= 64


# ------------------------------------------------------------------ the emulation (CPU, fp32 torch)
class Emu:
    """The ops under test in fp32 torch on the CPU, products accumulated in 64-wide K blocks; mut plants one mistake."""

    def __init__(self, mut=None):
        self.mut = mut

    def _mm(self, A, Bt, k0=0, k1=None):
        A, Bt = A.float(), Bt.float()
        M, K = A.shape
        N = Bt.shape[0]
        k1 = K if k1 is None else min(k1, K)
        m0 = (M - 1) // 256 * 256  # the mistakes hit the last row tile, its first 128 columns, the last K block
        rows, cols, last = slice(m0, M), slice(0, min(N, 128)), k0 + (k1 - k0 - 1) // 64 * 64
        acc = torch.zeros(M, N)
        for kb in range(k0, k1, 64):
            a, b = A[:, kb:min(kb + 64, k1)], Bt[:, kb:min(kb + 64, k1)]
            if self.mut == "chunk_swap" and kb == last and a.shape[1] >= 16:
                a, r = a.clone(), slice(m0, min(m0 + 8, M))
                a[r, 0:8], a[r, 8:16] = A[r, kb + 8:kb + 16], A[r, kb:kb + 8]
            p = a @ b.t()
            if self.mut == "drop_block" and kb == last:
                p[rows, cols] = 0
            if self.mut == "double_block" and kb == last:
                p[rows, cols] *= 2
            acc += p
        if self.mut == "swap_rows" and M - m0 >= 2:
            acc[[m0, m0 + 1]] = acc[[m0 + 1, m0]]
        if self.mut == "one_elem_1e-3":
            flat = acc.view(-1)
            flat[int(flat.abs().argmin())] += 1e-3
        return acc

    def _store(self, out, v, acc, bias):
        M, N = out.shape
        if acc and self.mut != "acc_overwrite":
            v = v + out.float()
        if bias is not None:
            v = v + bias
        out.copy_(v)
        if self.mut == "row_past_M" and M % 256:  # the tile's next row, computed from the clamped row M - 1
            big = out.as_strided((M + 1, N), out.stride(), out.storage_offset())
            big[M] = big[M - 1]

    def gemm_bt(self, A, Bt, out, beta, bias, ids, rev, B, T, dirn, xsf):
        M, N = out.shape
        K = Bt.shape[1]
        if rev is not None:
            t = torch.arange(T)[:, None].expand(T, B)
            b = torch.arange(B)[None, :].expand(T, B)
            tt = t if dirn == 0 else rev.view(B, T)[b, t]
            src = (ids.view(B, T)[b, tt] if ids is not None else b * T + tt).reshape(-1)
            Ag = A[src, :K]
            if xsf is not None:  # each column-tile workgroup stores an interleaved 1 / ntn of a row tile
                ntn = N // (256 if N % 256 == 0 else 128)
                step = ntn + 1 if self.mut == "xsf_ntn" else ntn
                x = xsf.view(M, K)
                for m0 in range(0, M, 256):
                    for tn in range(ntn):
                        r = torch.arange(m0 + tn, min(m0 + 256, M), step)
                        x[r] = Ag[r]
        else:
            Ag = A[:M, :K]
        self._store(out, self._mm(Ag, Bt), beta != 0.0, bias)

    def gemm_bt_merge(self, dz, Bt, out, rev, B, T, mode):
        if self.mut == "rev_wrong_half":
            mode = (mode & 4) | ((mode & 1) << 1) | ((mode >> 1) & 1)
        Kh = dz.numel() // (2 * B * T)
        dz, rev = dz.view(2, T, B, Kh), rev.view(B, T)
        bb, tt = torch.arange(B)[:, None].expand(B, T), torch.arange(T)[None, :].expand(B, T)
        A = torch.cat([dz[0][rev if mode & 1 else tt, bb], dz[1][rev if mode & 2 else tt, bb]], -1)  # [B][T][2 Kh]
        if not mode & 4:
            A = A.transpose(0, 1)
        self._store(out, self._mm(A.reshape(B * T, 2 * Kh), Bt), False, None)

    def _slabs(self, A, Bt, S, K):
        kc = (K // 64 + S - 1) // S * 64
        return [self._mm(A, Bt, s * kc, (s + 1) * kc) for s in range(S)]

    def _slab_sum(self, parts):
        t = parts[0].clone()
        for p in parts[1:]:
            t += p
        if self.mut == "last_split_twice" and len(parts) > 1:
            t += parts[-1]
        return t

    def gemm_bt_splitk_ws(self, M, N, K):
        S = splits_bt(M, N, K)
        return S * M * N if S > 1 else 0

    def gemm_bt_splitk(self, A, Bt, out, ws, acc):
        M, N = out.shape
        K = Bt.shape[1]
        need = self.gemm_bt_splitk_ws(M, N, K)
        if need == 0 or ws.numel() < need:
            return False
        parts = self._slabs(A[:M], Bt, need // (M * N), K)
        ws[:need].view(len(parts), M, N).copy_(torch.stack(parts))
        self._store(out, self._slab_sum(parts), acc, None)
        return True

    def wgrad_tt_ws(self, M, N, K):
        if _tt_ok(M, N, K):
            S = splits_tt(M, N, K)
            return 1 if S == 1 else S * M * N
        return splits_tt(N, M, K) * M * N if _tt_ok(N, M, K) else 0

    def wgrad_tt(self, a, b, out, ws, acc):
        K, M = a.shape
        N, nv = b.shape[1], out.shape[1]
        plain = _tt_ok(M, N, K)
        swapped = not plain and _tt_ok(N, M, K)
        if not plain and not (swapped and nv == N):
            return False
        if nv != N and nv % 4:
            return False
        S = splits_tt(M, N, K) if plain else splits_tt(N, M, K)
        direct = plain and not acc and S == 1
        if ws.numel() < (0 if direct else S * M * N):
            assert acc
            return False
        if direct:
            out.copy_(self._mm(a.t(), b.t())[:, :nv])
            return True
        parts = self._slabs(a.t(), b.t(), S, K)
        slab = torch.stack(parts if plain else [p.t() for p in parts])
        ws[:slab.numel()].view(slab.shape).copy_(slab)
        self._store(out, self._slab_sum(parts)[:, :nv], acc, None)
        return True

    def wgrad_tn(self, a, b, out):
        self._store(out, self._mm(a.t(), b.t()), True, None)

    def ctx_fwd(self, att, enc, ctx, ctxb, B, T, D, A):
        att, enc, ctx, ctxb = att.view(D, B, T), enc.view(B, T, A), ctx.view(D, B, A), ctxb.view(D, B, A)
        for b in range(B):
            a_, e_ = att[:, b, :], enc[b].t()
            if self.mut == "ctx_tail" and T % 32:  # the clamped att chunk times the clamped enc row, not zeroed
                pad = 32 - T % 32
                a_ = torch.cat([a_, att[:, b, T - 8:].repeat(1, pad // 8)], 1)
                e_ = torch.cat([e_, enc[b, T - 1][:, None].expand(A, pad)], 1)
            v = self._mm(a_, e_)
            ctx[:, b, :] = v
            ctxb[:, b, :] = v

    def ctx_da(self, dctx, enc, da, B, T, D, A, acc):
        dctx, enc, da = dctx.view(D, B, A), enc.view(B, T, A), da.view(D, B, T)
        for b in range(B):
            self._store(da[:, b, :], self._mm(dctx[:, b, :], enc[b]), acc, None)

    def ctx_de(self, att, dctx, de, B, T, D, A):
        att, dctx, de = att.view(D, B, T), dctx.view(D, B, A), de.view(B, T, A)
        for b in range(B):
            de[b] = self._mm(att[:, b, :].t(), dctx[:, b, :].t())


# ------------------------------------------------------------------ runners: one case, one input kind
def run_plain(k, dev, kind, M, N, K, obf, bias, beta, ldw):
    g = _gen(1, M, N, K, obf, bias, beta, ldw, kind == "exact")
    A, Bt = _vals(g, (M, K), kind), _vals(g, (N, K), kind, K ** -0.5)
    bv = _addend(g, (N,), kind) if bias else None
    c0 = _addend(g, (M, N), kind, 64) if beta else None
    ref, mag = _mmref(A, Bt)
    Ad = _in2d(A, dev)  # [M + 2][K + 8]: rows M .. and columns K .. NaN, passed whole
    Btd = _in2d(Bt, dev, 16, 8, 8)[8:8 + N, :K]
    o = Out(M, N, BF if obf else F32, SENT if beta else NAN, dev, prefill=c0, **wide(N, ldw))
    k.gemm_bt(Ad, Btd, o.view, 1.0 if beta else 0.0, bv.to(dev) if bias else None, None, None, 0, 0, 0, None)
    _sync(dev)
    tag = f"gemm_bt/{'bf16' if obf else 'f32'}({M},{N},{K},bias={bias},beta={beta},ldw={ldw})"
    adds = ([c0] if beta else []) + ([bv[None, :].expand(M, N)] if bias else [])
    _check(tag, o.view, ref, mag, K, kind, adds, out_bf16=obf)
    o.intact(tag)


def _lens_rev(g, B, T):
    lens = [T, 1] + torch.randint(1, T + 1, (max(B - 2, 0),), generator=g).tolist()
    lens = lens[:B]
    return torch.tensor([[n - 1 - t if t < n else t for t in range(T)] for n in lens], dtype=torch.int64)


def run_frame(k, dev, kind, use_ids, dirn, B, T, N, K, obf, bias, beta, want_xsf, ldw):
    g = _gen(2, use_ids, dirn, B, T, N, K, obf, bias, beta, ldw, kind == "exact")
    M, V = B * T, 301
    rev = _lens_rev(g, B, T)
    if use_ids:
        src = _vals(g, (V, K), kind)
        ids = torch.randint(0, V, (B, T), generator=g)
        ids[0, 0], ids[B - 1, T - 1] = 0, V - 1
    else:
        src, ids = _vals(g, (M, K), kind), None
    rows = []  # step frame m = t * B + b
    for t in range(T):
        for b in range(B):
            tt = t if dirn == 0 else int(rev[b, t])
            rows.append(int(ids[b, tt]) if use_ids else b * T + tt)
    assert not use_ids or (0 in rows and V - 1 in rows)
    Ag = src[rows]
    W = _vals(g, (N, K), kind, K ** -0.5)
    bv = _addend(g, (N,), kind) if bias else None
    c0 = _addend(g, (M, N), kind, 64) if beta else None
    ref, mag = _mmref(Ag, W)
    table = src.clone()
    unused = torch.ones(table.shape[0], dtype=torch.bool)
    unused[rows] = False
    table[unused] = NAN  # rows no id references
    # ids: the V table rows of a taller allocation, so nsrc = V and the id V - 1 is the last row the binding accepts
    Ad = _in2d(table, dev, 8, 0, 0)[:, :K] if not use_ids else _in2d(table, dev, 8, 0, 2)[:V]
    Wd = _in2d(W, dev, 16, 8, 8)[8:8 + N, :K]
    o = Out(M, N, BF if obf else F32, SENT if beta else NAN, dev, prefill=c0, **wide(N, ldw))
    x = Out(1, M * K, BF, NAN, dev) if want_xsf else None
    k.gemm_bt(Ad, Wd, o.view, 1.0 if beta else 0.0, bv.to(dev) if bias else None, ids.to(dev) if use_ids else None,
              rev.to(dev), B, T, dirn, x.view if want_xsf else None)
    _sync(dev)
    tag = f"gemm_bt_frame/{'bf16' if obf else 'f32'}(ids={use_ids},dir={dirn},{B}x{T},{N},{K},bias={bias},beta={beta},ldw={ldw})"
    adds = ([c0] if beta else []) + ([bv[None, :].expand(M, N)] if bias else [])
    _check(tag, o.view, ref, mag, K, kind, adds, out_bf16=obf)
    o.intact(tag)
    if want_xsf:
        same = _bits(x.view.cpu().view(M, K)) == _bits(Ag)
        assert bool(same.all()), f"{tag}: xsf: {int((~same.all(1)).sum())} rows differ from the gathered rows"
        x.intact(tag + " xsf")


def run_merge(k, dev, kind, mode, B, T, Kh, N, half):
    g = _gen(3, mode, B, T, Kh, N, half, kind == "exact")
    M, K = B * T, 2 * Kh
    rev = _lens_rev(g, B, T)
    dz = _vals(g, (2, T, B, Kh), kind)
    Km = _vals(g, (N, K), kind, K ** -0.5)
    A = torch.empty(M, K, dtype=BF)
    for m in range(M):
        b, t = (m // T, m % T) if mode & 4 else (m % B, m // B)
        r = int(rev[b, t])
        A[m, :Kh], A[m, Kh:] = dz[0, r if mode & 1 else t, b], dz[1, r if mode & 2 else t, b]
    ref, mag = _mmref(A, Km)
    tall = _in2d(Km, dev, 16, N if half else 0, 0 if half else N)  # Km[:H] / Km[H:] of a [2 H] matrix, the other half NaN
    Btd = tall[half * N:(half + 1) * N, :K]
    o = Out(M, N, F32, NAN, dev)  # the binding takes a contiguous out only (row slices of taller buffers)
    k.gemm_bt_merge(_inflat(dz, dev), Btd, o.view, rev.to(dev), B, T, mode)
    _sync(dev)
    tag = f"gemm_bt_merge(mode={mode},{B}x{T},Kh={Kh},{N},half={half})"
    _check(tag, o.view, ref, mag, K, kind)
    o.intact(tag)


def run_splitk(k, dev, kind, M, N, K, acc, S):
    g = _gen(4, M, N, K, acc, kind == "exact")
    assert splits_bt(M, N, K) == S
    need = int(k.gemm_bt_splitk_ws(M, N, K))
    assert need == (S * M * N if S > 1 else 0), (need, S)
    A, Bt = _vals(g, (M, K), kind), _vals(g, (N, K), kind, K ** -0.5)
    c0 = _addend(g, (M, N), kind, 64) if acc else None
    Ad, Btd = _in2d(A, dev)[:, :K], _in2d(Bt, dev, 16, 8, 8)[8:8 + N, :K]
    o = Out(M, N, F32, SENT if acc else NAN, dev, prefill=c0, **wide(N, True))
    w = Out(1, max(need, 4), F32, NAN, dev)
    tag = f"gemm_bt_splitk({M},{N},{K},acc={acc},S={S})"
    done = k.gemm_bt_splitk(Ad, Btd, o.view, w.view[0], acc)
    _sync(dev)
    if S == 1:  # the boundary: no split, nothing launched
        assert not done, tag
        o.intact(tag, untouched=True)
        w.intact(tag, untouched=True)
        return
    assert done, tag
    ref, mag = _mmref(A, Bt)
    _check(tag, o.view, ref, mag, K, kind, [c0] if acc else [], slabs=S)
    o.intact(tag)
    w.intact(tag)
    o2 = Out(M, N, F32, SENT if acc else NAN, dev, prefill=c0, **wide(N, True))
    assert k.gemm_bt_splitk(Ad, Btd, o2.view, w.view[0], acc)
    _sync(dev)
    _same_bits(tag, o2.view, o.view)


def run_wgrad_tt(k, dev, kind, M, N, K, acc, nv=None, shift=0):
    g = _gen(5, M, N, K, acc, nv or 0, shift, kind == "exact")
    nv = nv or N
    plain = _tt_ok(M, N, K)
    S = splits_tt(M, N, K) if plain else splits_tt(N, M, K)
    a, b = _vals(g, (K, M), kind, 0.1), _vals(g, (K, N), kind, 0.1)
    c0 = _addend(g, (M, nv), kind, 64) if acc else None
    ad, bd = _in2d(a, dev)[:K, :M], _in2d(b, dev, 16)[:K, :N]
    ref, mag = _mmref(a.t(), b.t())
    ref, mag = ref[:, :nv], mag[:, :nv]
    tag = f"wgrad_tt/{'plain' if plain else 'swapped'}({M},{N},{K},acc={acc},nv={nv},shift={shift},S={S})"
    lay = dict(shift=shift) if shift else wide(nv, True)
    o = Out(M, nv, F32, SENT if acc else NAN, dev, prefill=c0, **lay)
    need = int(k.wgrad_tt_ws(M, N, K))
    assert need == (1 if plain and S == 1 else S * M * N), (tag, need)
    if acc and need == 1:  # documented: acc on a one-split shape needs the slab wgrad_tt_ws did not count
        w1 = Out(1, 4, F32, NAN, dev)
        assert k.wgrad_tt(ad, bd, o.view, w1.view[0][:1], True) is False, tag
        _sync(dev)
        o.intact(tag, untouched=True)
        w1.intact(tag, untouched=True)
    direct = plain and S == 1 and not acc
    w = Out(1, 4 if direct else S * M * N, F32, NAN, dev)
    assert k.wgrad_tt(ad, bd, o.view, w.view[0], acc), tag
    _sync(dev)
    _check(tag, o.view, ref, mag, K, kind, [c0] if acc else [], slabs=0 if direct else S)
    o.intact(tag)
    w.intact(tag, untouched=direct)
    o2 = Out(M, nv, F32, SENT if acc else NAN, dev, prefill=c0, **lay)
    assert k.wgrad_tt(ad, bd, o2.view, w.view[0], acc)
    _sync(dev)
    _same_bits(tag, o2.view, o.view)


def run_wgrad_tn(k, dev, kind, M, N, K, ldw):
    g = _gen(6, M, N, K, ldw, kind == "exact")
    a, b = _vals(g, (K, M), kind, 0.1), _vals(g, (K, N), kind, 0.1)
    c0 = _addend(g, (M, N), kind, 64)
    ad, bd = _in2d(a, dev)[:K, :M], _in2d(b, dev, 16)[:K, :N]
    ref, mag = _mmref(a.t(), b.t())
    S = splits_tn(M, N, K)
    tag = f"wgrad_tn({M},{N},{K},ldw={ldw},S={S})"
    o = Out(M, N, F32, SENT, dev, prefill=c0, **wide(N, ldw))
    k.wgrad_tn(ad, bd, o.view)
    _sync(dev)
    _check(tag, o.view, ref, mag, K, kind, [c0], slabs=S, slab_mag=mag + c0.double().abs(), add_rounds=False)
    o.intact(tag)
    if kind == "exact":
        o2 = Out(M, N, F32, SENT, dev, prefill=c0, **wide(N, ldw))
        k.wgrad_tn(ad, bd, o2.view)
        _sync(dev)
        _same_bits(tag, o2.view, o.view)


def _ctx_inputs(kind, B, T, D, A, salt):
    g = _gen(7, B, T, D, A, salt, kind == "exact")
    return _att(g, (D, B, T), kind), _vals(g, (B, T, A), kind), _vals(g, (D, B, A), kind), g


def run_ctx_fwd(k, dev, kind, B, T, D, A):
    att, enc, _, _ = _ctx_inputs(kind, B, T, D, A, 0)
    ref = torch.einsum("dbt,bta->dba", att.double(), enc.double())
    mag = torch.einsum("dbt,bta->dba", att.double(), enc.double().abs())
    o, ob = Out(1, D * B * A, F32, NAN, dev), Out(1, D * B * A, BF, NAN, dev)
    k.ctx_fwd(_inflat(att, dev), _inflat(enc, dev), o.view.view(D, B, A), ob.view.view(D, B, A), B, T, D, A)
    _sync(dev)
    tag = f"ctx_fwd({B},{T},{D},{A})"
    unit = 64 if kind == "exact" else 1
    _check(tag, o.view.view(D, B, A), ref, mag, T, kind, unit=unit)
    _check(tag.replace("ctx_fwd", "ctx_fwd/bf16"), ob.view.view(D, B, A), ref, mag, T, kind, out_bf16=True, unit=unit)
    assert torch.equal(_bits(ob.view.cpu()), _bits(o.view.cpu().bfloat16())), f"{tag}: ctxb: not ctx rounded once"
    o.intact(tag)
    ob.intact(tag + " ctxb")


def run_ctx_da(k, dev, kind, B, T, D, A, acc):
    _, enc, dctx, g = _ctx_inputs(kind, B, T, D, A, 1)
    c0 = _addend(g, (D, B, T), kind, 64) if acc else None
    ref = torch.einsum("dba,bta->dbt", dctx.double(), enc.double())
    mag = torch.einsum("dba,bta->dbt", dctx.double().abs(), enc.double().abs())
    o = Out(1, D * B * T, F32, SENT if acc else NAN, dev, prefill=c0.reshape(1, -1) if acc else None)
    k.ctx_da(_inflat(dctx, dev), _inflat(enc, dev), o.view.view(D, B, T), B, T, D, A, acc)
    _sync(dev)
    tag = f"ctx_da({B},{T},{D},{A},acc={acc})"
    _check(tag, o.view.view(D, B, T), ref, mag, A, kind, [c0] if acc else [])
    o.intact(tag)


def run_ctx_de(k, dev, kind, B, T, D, A, obf):
    att, _, dctx, _ = _ctx_inputs(kind, B, T, D, A, 2)
    ref = torch.einsum("dbt,dba->bta", att.double(), dctx.double())
    mag = torch.einsum("dbt,dba->bta", att.double(), dctx.double().abs())
    o = Out(1, B * T * A, BF if obf else F32, NAN, dev)
    k.ctx_de(_inflat(att, dev), _inflat(dctx, dev), o.view.view(B, T, A), B, T, D, A)
    _sync(dev)
    tag = f"ctx_de/{'bf16' if obf else 'f32'}({B},{T},{D},{A})"
    _check(tag, o.view.view(B, T, A), ref, mag, D, kind, out_bf16=obf, unit=64 if kind == "exact" else 1)
    o.intact(tag)


# ------------------------------------------------------------------ the cases (profiles/gemm_op_tests.md: which line each exercises)
# M, N, K, bf16 out, bias, beta, ldc > N
PLAIN = [(1, 128, 64, False, False, False, False), (1, 512, 128, False, True, True, False),
         (255, 256, 128, True, True, False, False), (255, 128, 64, False, True, True, False),
         (256, 384, 192, False, True, True, False), (256, 256, 64, False, False, False, False),
         (257, 512, 64, False, False, True, False), (257, 256, 192, True, True, False, False),
         (300, 384, 128, True, False, False, False), (300, 128, 192, False, True, False, False),
         (300, 512, 128, False, True, False, False), (770, 512, 64, False, False, False, False),
         (770, 384, 64, False, True, False, False), (300, 256, 128, False, True, True, True),
         (255, 128, 64, True, True, False, True), (300, 384, 192, False, False, True, True)]
# ids, dir, B, T, N, K, bf16 out, bias, beta, xsf, ldc > N
FRAME = [(True, 0, 3, 5, 128, 64, False, True, False, True, False), (True, 1, 40, 7, 384, 192, False, True, False, True, False),
         (False, 0, 40, 7, 512, 64, True, False, False, True, False), (False, 1, 3, 5, 256, 192, False, False, True, True, False),
         (True, 1, 40, 7, 512, 192, False, True, True, True, False), (False, 0, 40, 7, 128, 192, True, True, False, True, False),
         (False, 1, 40, 7, 384, 64, False, False, True, True, False), (True, 0, 3, 5, 256, 64, True, False, False, True, False),
         (True, 1, 3, 5, 384, 64, False, False, False, False, False), (False, 0, 40, 7, 256, 192, False, True, False, False, False),
         (True, 0, 40, 7, 256, 64, True, True, False, True, True), (False, 1, 40, 7, 384, 64, False, True, True, False, True)]
# mode, B, T, Kh, N, half
MERGE = [(0, 3, 5, 64, 128, 0), (1, 40, 7, 128, 256, 1), (2, 40, 7, 64, 384, 0), (3, 3, 5, 128, 256, 1),
         (4, 40, 7, 64, 128, 1), (5, 3, 5, 64, 384, 0), (6, 40, 7, 128, 128, 0), (7, 40, 7, 64, 256, 1)]
# M, N, K, acc, S
SPLITK = [(1, 128, 2048, False, 2), (257, 256, 2048, True, 2), (257, 128, 2112, False, 2), (1, 256, 2112, True, 2),
          (1, 128, 3072, True, 3), (257, 128, 1984, False, 1)]
# M, N, K, acc, nv, shift
WGRAD_TT = [(256, 128, 64, False, None, 0), (256, 128, 64, True, None, 0), (256, 256, 192, False, None, 0),
            (256, 256, 192, True, None, 0), (512, 384, 320, False, None, 0), (512, 384, 320, True, None, 0),
            (512, 384, 64, False, None, 0), (512, 384, 4160, False, None, 0), (128, 256, 64, False, None, 0),
            (128, 256, 192, True, None, 0), (128, 512, 320, False, None, 0), (128, 512, 64, True, None, 0),
            (256, 256, 192, False, None, 1), (256, 128, 64, False, None, 1), (128, 256, 192, True, None, 1),
            (256, 256, 192, False, 200, 0), (256, 256, 192, True, 200, 1), (256, 128, 64, False, 100, 0)]
# M, N, K, ldo > N
WGRAD_TN = [(128, 8, 1, False), (128, 120, 63, True), (256, 128, 64, False), (256, 136, 65, True), (128, 200, 130, False),
            (256, 200, 1100, True), (128, 128, 1100, False), (256, 8, 64, True),
            (256, 1160, 64, True)]
# B, T, D, A
CTX = [(1, 8, 1, 128), (3, 56, 15, 256), (9, 64, 16, 128), (3, 72, 17, 256), (1, 136, 100, 128), (3, 264, 128, 256),
       (9, 72, 100, 256), (9, 8, 128, 128)]


@pytest.mark.parametrize("case", PLAIN, ids=str)
def test_gemm_bt_plain(case):
    for kind in KINDS:
        run_plain(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", FRAME, ids=str)
def test_gemm_bt_step_frame(case):
    for kind in KINDS:
        run_frame(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", MERGE, ids=str)
def test_gemm_bt_merge(case):
    for kind in KINDS:
        run_merge(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", SPLITK, ids=str)
def test_gemm_bt_splitk(case):
    for kind in KINDS:
        run_splitk(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", WGRAD_TT, ids=str)
def test_wgrad_tt(case):
    for kind in KINDS:
        run_wgrad_tt(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", WGRAD_TN, ids=str)
def test_wgrad_tn(case):
    for kind in KINDS:
        run_wgrad_tn(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("case", CTX, ids=str)
def test_ctx_fwd(case):
    assert _ops().ctx_bmm_ok(*case)
    for kind in KINDS:
        run_ctx_fwd(_ops(), "cuda", kind, *case)


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("case", CTX, ids=str)
def test_ctx_da(case, acc):
    for kind in KINDS:
        run_ctx_da(_ops(), "cuda", kind, *case, acc)


@pytest.mark.parametrize("obf", [False, True])
@pytest.mark.parametrize("case", CTX, ids=str)
def test_ctx_de(case, obf):
    for kind in KINDS:
        run_ctx_de(_ops(), "cuda", kind, *case, obf)


CHILD_CASES = [((3, 136, 17, 128), False), ((3, 264, 100, 256), True)]


def _child_ctx_da():
    """in a fresh process started with TSAMD_CTX_DA_NW=4 (launch_ctx_da reads it once): the 4-wave ctx_da kernel"""
    assert os.environ.get("TSAMD_CTX_DA_NW") == "4"
    for case, acc in CHILD_CASES:
        for kind in KINDS:
            run_ctx_da(_ops(), "cuda", kind, *case, acc)


def test_ctx_da_four_wave_kernel_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_gemm_ops as m; m._child_ctx_da()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TSAMD_CTX_DA_NW="4"), capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
