"""The layout, column-sum and repack kernels one by one against float64 / integer torch on the CPU:
csrc/kernels/frames.hip (to_step_frame, from_step_frame, step_frame_hop, tr01, transpose_bta, cast_colsum, colsum),
csrc/kernels/pack.hip (pack_cast, with the host classifier pack_job_rows) and beam_gather (beam.hip).  Every op is
called through ops(); the reference writes the index arithmetic as plain gathers and never goes through another kernel.

Bit for bit.  The copies, transposes and gathers, the fp32 sums of two fp32 numbers (a float64 sum of two fp32 numbers
rounded once to fp32 is the fp32 sum), the scaled repack (a float64 product of two fp32 numbers is exact, so rounding it
to fp32 gives the fp32 product) and every bf16 output (torch's .bfloat16() of the fp32 value) are exactly determined:
every element must match.  The bf16 inputs include the halfway cases with an even and an odd kept mantissa, a carry
into the exponent, the largest finite fp32, +-inf, +-0, fp32 subnormals and one NaN (SPECIALS).

Column sums, two kinds of input as in tests/test_gpu_gemm_ops.py.
  exact    integers in [-8, 8], integer prefill: every partial sum is an integer below 2^24 (asserted on the
           reference), so the result is bit-equal in any order.
  general  randn.  Per column  d U sum_n |x_nc| + U |out|,  U = 2^-24, d the longest chain of additions of the
           kernel's reduction tree, computed from a Python mirror of the launcher's split rule (cast_colsum_depth,
           colsum_depth; derivation in profiles/layout_op_tests.md).  A zero bound requires a zero error.

Slack and sentinels.  Every operand is a view into a larger NaN-filled allocation (table rows and parent rows nothing
references are NaN too); every output is a view into an allocation prefilled with NaN (stores) or 12288.0
(accumulates) with a 4096-element block before and behind that must be bit-identical afterwards.  pack_cast reads one
NaN-padded fp32 arena and writes one bf16 and one fp32 arena filled with 12288.0; before every launch Arenas.validate
walks each job row as the kernel indexes it and asserts that every index falls inside its view and that no
destination element is written twice.

The runners take the op table k (ops(), or Emu: a torch emulation in the kernels' own index form) and the device, so
tests/test_layout_ops_checks.py runs the same checks on the CPU with the emulation and with mistakes planted in it."""
import math

import pytest
import torch

from test_gpu_gemm_ops import BF, F32, KINDS, NAN, SENT, U24, Out, _bits, _gen, _lens_rev, _same_bits, _sync

pytestmark = pytest.mark.gpu

I32 = torch.int32
K2LOG2E = 2.8853900817779268
GRID_CAP = 8192 * 256  # grid_for (frames.hip): threads of one grid-stride trip
# fp32 bit patterns for the bf16 roundings: halfway with the kept mantissa even / odd (both signs), the carry into the
# exponent, the largest finite, +-inf, +-0, subnormals (the smallest, one that is a bf16 subnormal, half the smallest
# bf16 subnormal), just above / below halfway, one NaN
SPECIALS = [0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f7fffff, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
            0x00000000, 0x80000000, 0x00000001, 0x00400000, 0x00008000, 0x00018000, 0x3f808001, 0x3f817fff, 0x7fc00000]


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _specials():
    return torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in SPECIALS], dtype=I32).view(F32)


def _with_specials(x):
    """x (fp32) with SPECIALS written over its first elements (as many as fit)"""
    s = _specials()
    n = min(x.numel(), s.numel())
    x.view(-1)[:n] = s[:n]
    return x


def _eq(tag, got, want, name="exact"):
    """bit for bit; a NaN matches a NaN"""
    got, want = got.detach().cpu().contiguous(), want.contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, got.dtype, want.shape, want.dtype)
    bad = (_bits(got) != _bits(want)) & ~(got.isnan() & want.isnan())
    if bool(bad.any()):
        at = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{tag}: {name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {list(at)}: "
                             f"got {float(got[at])}, want {float(want[at])}")


def _flat(vals, dev, shift=0):
    """a contiguous operand inside a NaN-padded (integers: -2^31) flat allocation, `shift` elements off the aligned start"""
    flat = torch.full((128 + shift + vals.numel(),), NAN if vals.is_floating_point() else -2 ** 31, dtype=vals.dtype)
    flat[64 + shift:64 + shift + vals.numel()] = vals.reshape(-1)
    return flat.to(dev)[64 + shift:64 + shift + vals.numel()].view(vals.shape)


def _out(shape, dtype, dev, fill=NAN, prefill=None, shift=0):
    n = math.prod(shape)
    o = Out(1, n, dtype, fill, dev, shift=shift, prefill=None if prefill is None else prefill.reshape(1, n))
    return o, o.view.view(shape)


def _refused(tag, fn):
    try:
        fn()
    except RuntimeError:
        return
    raise AssertionError(f"{tag}: refusal: the call was accepted")


def _aligned(t, nbytes):
    return (t.storage_offset() * t.element_size()) % nbytes == 0 and t.untyped_storage().data_ptr() % nbytes == 0


# ------------------------------------------------------------------ host-side split rules (ports of the launchers')
def cast_colsum_blocks(N, C):
    """cast_colsum_blocks (frames.hip)"""
    rpb = 256 // (C // 4)
    return min(max((N + rpb - 1) // rpb, 1), 256)


def cast_colsum_depth(N, C):
    """longest chain of additions behind one column of cast_colsum: a thread's rows (every G rpb-th), the block's rpb
    row groups, a finish lane's ceil(G / 16) partials, the 16 lanes"""
    rpb, G = 256 // (C // 4), cast_colsum_blocks(N, C)
    return -(-N // (G * rpb)) + (rpb - 1) + -(-G // 16) + 16


def colsum_det_chunks(N, C):
    """colsum_det_chunks (frames.hip)"""
    nct = (C + 255) // 256
    return max(1, min((2048 + nct - 1) // nct, max(1, N // 64)))


def colsum_rpc(N, C):
    G = colsum_det_chunks(N, C)
    return (N + G - 1) // G


def colsum_depth(N, C):
    """colsum: a wave's every 4th row of a chunk of rpc rows, the 3 adds of the other waves, a finish lane's
    ceil(G / GL) partials, the GL lanes (GL = 16 with 16 columns per block at C >= 64, 256 with one)"""
    G, GL = colsum_det_chunks(N, C), 16 if C >= 64 else 256
    return -(-colsum_rpc(N, C) // 4) + 3 + -(-G // GL) + GL


# ------------------------------------------------------------------ pack_cast: the job-row interpreter
def pack_walk(rows, total, mut=None):
    """Every workgroup of a pack_cast launch as the kernel indexes it (pack.hip): yields (job, source element offsets
    from the job's src pointer, destination element offsets from its dst pointer)."""
    nj = len(rows)
    start = [r[11] for r in rows] + [total]
    tid, a8 = torch.arange(256), torch.arange(8)
    for blk in range(total):
        lo, hi = 0, nj - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if start[mid] <= blk:
                lo = mid
            else:
                hi = mid - 1
        if mut == "search_job_before" and lo > 0 and blk == start[lo]:
            lo -= 1
        J = rows[lo]
        jb, kind, n = blk - start[lo], J[12], J[14]
        if kind == 1:
            e0 = jb * 2048 + tid * 8
            e = e0[:, None] + a8
            ok = (e0 < n)[:, None] & (e < n)
            if mut == "tail_8_past_n":
                ok = (e0 < n)[:, None].expand(256, 8)
            s = d = e[ok]
        elif kind == 2:
            R, C = J[3], J[4]
            tr = (R + 63) // 64
            i, c = (jb % tr) * 64 + torch.arange(64)[:, None], (jb // tr) * 64 + torch.arange(64)[None, :]
            ok = (i < R) & (c < C)
            s, d = (c * (C if mut == "k2_rowlen_C" else R) + i)[ok], (i * C + c)[ok]
        elif kind == 3:
            e0 = jb * 2048 + tid * 8
            ok = e0 < n
            r = e0 // J[4]
            c = e0 - r * J[4]
            s, d = ((r * J[6] + c)[:, None] + a8)[ok].reshape(-1), ((r * J[9] + c)[:, None] + a8)[ok].reshape(-1)
        else:
            li = jb * 256 + tid
            ok = li < n
            i2, r = li % J[4], li // J[4]
            i1, i0 = r % J[3], r // J[3]
            s, d = (i0 * J[5] + i1 * J[6] + i2 * J[7])[ok], (i0 * J[8] + i1 * J[9] + i2 * J[10])[ok]
        yield lo, s.reshape(-1), d.reshape(-1)


class Arenas:
    """One NaN-padded fp32 source arena, one bf16 and one fp32 destination arena filled with 12288.0.  Views are
    described by (offset, shape, strides) so the CPU reference and the device see the same geometry."""

    def __init__(self):
        self.specs, self.cur = [], {"s": 64, "b": 64, "f": 64}

    def _take(self, which, extent, shift):
        off = self.cur[which] + shift
        self.cur[which] = (off + extent + 63) // 64 * 64 + 64  # a gap of at least 64 elements, 64-element aligned
        return off

    def add(self, shape, sstr, dstr, f32o, scale, kind, sshift=0, dshift=0):
        ext = lambda st: 1 + sum((n - 1) * s for n, s in zip(shape, st))
        self.specs.append(dict(shape=tuple(shape), sstr=tuple(sstr), dstr=tuple(dstr), f32o=f32o, scale=scale, kind=kind,
                               soff=self._take("s", ext(sstr), sshift), doff=self._take("f" if f32o else "b", ext(dstr), dshift)))

    def build(self, g, dev):
        src = torch.full((self.cur["s"],), NAN)
        self.dst_cpu = {0: torch.full((self.cur["b"],), SENT, dtype=BF), 1: torch.full((self.cur["f"],), SENT)}
        self.mask = {i: torch.zeros(t.numel(), dtype=torch.bool) for i, t in self.dst_cpu.items()}
        self.smask = torch.zeros(src.numel(), dtype=torch.bool)
        for sp in self.specs:
            v = _with_specials(torch.randn(sp["shape"], generator=g))  # every job's first elements: the bf16 roundings
            sv = src.as_strided(sp["shape"], sp["sstr"], sp["soff"])
            assert bool(sv.isnan().all()), "source views overlap"
            sv.copy_(v)
            self.smask.as_strided(sp["shape"], sp["sstr"], sp["soff"]).fill_(True)
            m = self.mask[sp["f32o"]].as_strided(sp["shape"], sp["dstr"], sp["doff"])
            assert not bool(m.any()), "destination views overlap"
            m.fill_(True)
            # the reference: bf16(fp32(float64(x) * float64(sc)))
            want = (sv.double() * float(torch.tensor(sp["scale"] or 1.0, dtype=F32).double())).float()
            self.dst_cpu[sp["f32o"]].as_strided(sp["shape"], sp["dstr"], sp["doff"]).copy_(want)
        self.src = src.to(dev)
        self.dst = {i: torch.full((t.numel(),), SENT, dtype=t.dtype).to(dev) for i, t in self.dst_cpu.items()}
        for t in (self.src, self.dst[0], self.dst[1]):
            assert t.data_ptr() % 64 == 0
        return self

    def pairs(self):
        out = []
        for sp in self.specs:
            p = (self.dst[sp["f32o"]].as_strided(sp["shape"], sp["dstr"], sp["doff"]),
                 self.src.as_strided(sp["shape"], sp["sstr"], sp["soff"]))
            out.append(p + ((sp["scale"],) if sp["scale"] else ()))
        return out

    def offsets(self, rows, job, s, d):
        """element offsets into the arenas of a job's source / destination offsets; the pointers must be whole elements"""
        J = rows[job]
        sb, db = J[0] - self.src.data_ptr(), J[1] - self.dst[J[13]].data_ptr()
        es = 4 if J[13] else 2
        assert sb % 4 == 0 and db % es == 0, (sb, db)
        return s + sb // 4, d + db // es

    def validate(self, tag, rows, total):
        """walk every row as the kernel indexes it: sources inside a source view, destinations inside the arena,
        every destination element of every view written exactly once"""
        hit = {i: torch.zeros(t.numel(), dtype=torch.int32) for i, t in self.dst_cpu.items()}
        for job, s, d in pack_walk(rows, total):
            so, do = self.offsets(rows, job, s, d)
            if so.numel() == 0:
                continue
            f = rows[job][13]
            assert 0 <= int(so.min()) and int(so.max()) < self.src.numel(), f"{tag}: validator: job {job} reads outside the source arena"
            assert 0 <= int(do.min()) and int(do.max()) < hit[f].numel(), f"{tag}: validator: job {job} writes outside its arena"
            assert bool(self.smask[so].all()), f"{tag}: validator: job {job} reads outside its source view"
            hit[f].index_add_(0, do, torch.ones(do.numel(), dtype=torch.int32))
        for f in (0, 1):
            assert torch.equal(hit[f], self.mask[f].int()), f"{tag}: validator: destination elements written {int(hit[f].max())} times or missed"

    def check(self, tag):
        for f, name in ((0, "bf16"), (1, "f32")):
            got, want, m = self.dst[f].cpu(), self.dst_cpu[f], self.mask[f]
            _eq(f"{tag} {name}", got[m], want[m])
            _eq(f"{tag} {name}", got[~m], want[~m], "sentinel")


# ------------------------------------------------------------------ the emulation (CPU torch, the kernels' own index form)
class Emu:
    """The ops under test on the CPU: flat thread index -> element as the kernels decompose it, fp32 adds in the
    kernels' order for the column sums, the job-row interpreter for pack_cast.  mut plants one mistake."""

    def __init__(self, mut=None):
        self.mut, self.arenas = mut, None

    def _bf(self, x):
        if self.mut == "bf16_truncate":
            return (x.contiguous().view(I32) & -65536).view(F32).bfloat16()
        return x.bfloat16()

    @staticmethod
    def _need(ok, msg):
        if not ok:
            raise RuntimeError(msg)

    def to_step_frame(self, src, ids, rev, out, B, T, W, doff):
        es, S = src.element_size(), src.shape[-1]
        self._need(W * es % 16 == 0 and doff * es % 16 == 0 and doff + W <= S and S * es % 16 == 0, "row widths")
        self._need(_aligned(src, 16) and _aligned(out, 16), "alignment")
        ec, cpr = 16 // es, W * es // 16
        n = 2 * T * B * cpr
        if self.mut == "one_trip":
            n = min(n, GRID_CAP)
        i = torch.arange(n)
        c, rowo = i % cpr, i // cpr
        b, t, d = rowo % B, (rowo // B) % T, rowo // (B * T)
        rv = rev.reshape(-1)[b * T + t]
        tt = torch.where(d == 0, t, rv)
        if self.mut == "rev_on_fw":
            tt = torch.where(d == 0, rv, t)
        srow = ids.reshape(-1)[b * T + tt] if ids is not None else b * T + tt
        off = 0 if self.mut == "doff_dropped" else doff
        out.view(-1, ec)[i] = src.reshape(-1, S // ec, ec)[srow, d * off // ec + c]

    def from_step_frame(self, x, rev, out, B, T, W):
        self._need(W % 4 == 0, "W % 4")
        self._need(_aligned(x, 16) and _aligned(out, 16), "alignment")
        cpr = W // 4
        i = torch.arange(B * T * cpr)
        c, bt = i % cpr, i // cpr
        t, b = bt % T, bt // T
        rt = t if self.mut == "bw_at_t" else rev.reshape(-1)[b * T + t]
        x4 = x.reshape(-1, 4)
        out.view(-1, 4)[i] = x4[(t * B + b) * cpr + c] + x4[T * B * cpr + (rt * B + b) * cpr + c]

    def step_frame_hop(self, x, rev, out, B, T, H):
        self._need(H % 4 == 0, "H % 4")
        self._need(_aligned(x, 16) and _aligned(out, 16), "alignment")
        cpr = H // 4
        i = torch.arange(2 * T * B * cpr)
        c, row = i % cpr, i // cpr
        b, t, d = row % B, (row // B) % T, row // (B * T)
        rt = rev.reshape(-1)[b * T + t]
        t0, t1 = torch.where(d == 0, t, rt), torch.where(d == 0, rt, t)
        if self.mut == "hop_bw_not_reversed":
            t0 = t
        x4 = x.reshape(-1, 4)
        col = d * cpr + c
        out.view(-1, 4)[i] = x4[(t0 * B + b) * 2 * cpr + col] + x4[T * B * 2 * cpr + (t1 * B + b) * 2 * cpr + col]

    def tr01(self, x, out, outb, P, Q, R, acc):
        self._need(R % 4 == 0 and P >= 1 and Q >= 1, "R % 4")
        self._need(not acc or (out is not None and outb is None), "acc")
        self._need(_aligned(x, 16) and (out is None or _aligned(out, 16)) and (outb is None or _aligned(outb, 8)), "alignment")
        R4 = R // 4
        i = torch.arange(P * Q * R4)
        r, qp = i % R4, i // R4
        pp, q = qp % P, qp // P
        v = x.reshape(-1, 4)[(pp * Q + q) * R4 + r]
        if out is not None:
            o4 = out.view(-1, 4)
            o4[i] = v + o4[i] if acc and self.mut != "acc_overwrite" else v
        if outb is not None:
            outb.view(-1, 4)[i] = self._bf(v)

    def transpose_bta(self, x, out, B, T, A):
        self._need(A % 64 == 0, "A % 64")
        self._need(_aligned(x, 8) and (T % 4 != 0 or _aligned(out, 8)), "alignment")
        xv, ov = x.view(B, T, A), out.view(B, A, T)
        for t0 in range(0, T, 4):  # 4 positions per store; the scalar branch stops at T
            w = min(4, T - t0)
            ov[:, :, t0:t0 + w] = xv[:, t0:t0 + w, :].transpose(1, 2)
            if self.mut == "vec_store_past_T" and w < 4:  # the 8-byte store taken with t < T alone
                last = out.as_strided((4,), (1,), out.storage_offset() + (B * A - 1) * T + t0)
                last[w:] = 0

    def cast_colsum(self, x, xb, colsum, N, C):
        self._need(C % 4 == 0 and C // 4 <= 256 and 256 % (C // 4) == 0, "C")
        self._need(_aligned(x, 16) and _aligned(xb, 8), "alignment")
        x, rpb, G = x.view(N, C), 256 // (C // 4), cast_colsum_blocks(N, C)
        xb.view(N, C).copy_(self._bf(x))
        part = torch.zeros(G, C)
        for blk in range(G):
            ps = torch.zeros(rpb, C)
            for rg in range(rpb):
                first = blk * rpb + (0 if self.mut == "rowgroup_clamped" and blk * rpb + rg >= N else rg)
                for r in range(first, N, G * rpb):
                    ps[rg] += x[r]
            s = ps[0].clone()
            for g in range(1, rpb):
                s += ps[g]
            part[blk] = s
        red = torch.zeros(16, C)
        for gl in range(16):
            for g in range(gl, G, 16):
                red[gl] += part[g]
        t = torch.zeros(C)
        for i in range(16):
            t += red[i]
        colsum += t

    def colsum(self, x, out, N, C, acc):
        self._need(C % 4 != 0 or _aligned(x, 8 if x.dtype == BF else 16), "alignment")
        x = x.view(N, C).float()
        G, rpc, GL = colsum_det_chunks(N, C), colsum_rpc(N, C), 16 if C >= 64 else 256
        part = torch.zeros(G, C)
        for g in range(G):
            r0, r1 = g * rpc, min(N, g * rpc + rpc)
            if self.mut == "last_chunk_twice" and g == G - 1 and G > 1:
                r0 -= rpc
            ps = torch.zeros(4, C)
            for w in range(4):
                for r in range(r0 + w, r1, 4):
                    ps[w] += x[r]
            t = ps[0].clone()
            for w in range(1, 4):
                t += ps[w]
            part[g] = t
        red = torch.zeros(GL, C)
        for gl in range(GL):
            for g in range(gl, 1 if self.mut == "finish1_first_partial" and GL == 256 else G, GL):
                red[gl] += part[g]
        t = torch.zeros(C)
        for i in range(GL):
            t += red[i]
        out.copy_(out + t if acc else t)

    def beam_gather(self, gidx, latest, c_src, h_src, ctx_src, a_src, cov_src, XGtab, Xtab, c_out, h_out, ctx_out,
                    ctxb_out, cov_out, XG_out, x_out, R, H, A, T, E, V, unk, step):
        self._need(0 <= unk < V, "unk")
        self._need(cov_out is None or cov_src is not None, "cov_src")
        if step is not None:
            step += 1
        g = gidx.long()
        tok = latest.long()
        tok = tok % V if self.mut == "unk_modulo" else torch.where(tok < V, tok, torch.full_like(tok, unk))
        if self.mut == "parent_identity":
            g = torch.arange(R)
        c_out.view(R, H).copy_(c_src.view(R, H)[g])
        h_out.view(R, H).copy_(h_src.view(R, H)[g])
        ctx_out.view(R, A).copy_(ctx_src.view(R, A)[g])
        ctxb_out.view(R, A).copy_(self._bf(ctx_src.view(R, A)[g]))
        if cov_out is not None:
            cov_out.view(R, T).copy_(cov_src.view(R, T)[g] + a_src.view(R, T)[g])
        XG_out.view(R, 4 * H).copy_(XGtab.view(V, 4 * H)[tok])
        x_out.view(R, E).copy_(Xtab.view(V, E)[tok])

    def pack_max_jobs(self):
        return 64

    def pack_job_cols(self):
        return 16

    def bind_arenas(self, arenas):
        self.arenas = arenas

    def pack_cast(self, jobs, total):
        self._need(jobs.dim() == 2 and jobs.dtype == torch.long and jobs.shape[1] == 16 and 1 <= jobs.shape[0] <= 64, "jobs")
        rows, ar = jobs.tolist(), self.arenas
        for job, s, d in pack_walk(rows, int(total), self.mut):
            if s.numel() == 0:
                continue
            so, do = ar.offsets(rows, job, s, d)
            J = rows[job]
            sc = torch.tensor(J[15], dtype=I32).view(F32) if J[15] else torch.tensor(1.0)
            v = ar.src[so.clamp(0, ar.src.numel() - 1)]  # a planted mistake may index past the arena
            if J[13]:
                ar.dst[1][do] = v * sc
            elif self.mut == "scale_after_cast":
                ar.dst[0][do] = self._bf(v).float().mul(sc).bfloat16()
            else:
                ar.dst[0][do] = self._bf(v * sc)


# ------------------------------------------------------------------ runners: frames
def _frame_rows(ids, rev, B, T):
    """[2][T][B]: the source row of out[d][t][b]"""
    t, b = torch.arange(T)[:, None].expand(T, B), torch.arange(B)[None, :].expand(T, B)
    tt = torch.stack([t, rev[b, t]])
    return ids[b, tt] if ids is not None else b * T + tt


def _check_rev(rev, B, T):
    lens = [int((rev[b] != torch.arange(T)).sum()) for b in range(B)]  # rev is the identity past the length
    assert rev[0].tolist() == list(range(T - 1, -1, -1)) and rev[1].tolist() == list(range(T)), "lengths T and 1"
    assert bool((torch.gather(rev, 1, rev) == torch.arange(T)).all()), "rev is an involution"
    return lens


def run_to_step_frame(k, dev, bf, use_ids, B, T, W, doff):
    g = _gen(21, bf, use_ids, B, T, W, doff)
    rev = _lens_rev(g, B, T)
    _check_rev(rev, B, T)
    dt, S = BF if bf else F32, (W if use_ids else 2 * W)
    if use_ids:
        V = 53
        table = torch.randn(V, S, generator=g).to(dt)
        ids = torch.randint(0, V - 3, (B, T), generator=g)
        ids[0, 0], ids[0, 1], ids[B - 1, T - 1] = 0, 0, V - 1  # a repeat, the first and the last row
        used = torch.zeros(V, dtype=torch.bool)
        used[ids.reshape(-1)] = True
        assert not bool(used.all()) and ids.unique().numel() < ids.numel()
        table[~used] = NAN  # rows no id references
    else:
        table, ids = torch.randn(B * T, S, generator=g).to(dt), None
    rows = _frame_rows(ids, rev, B, T)
    want = torch.stack([table[rows[d], d * doff:d * doff + W] for d in range(2)])
    o, ov = _out((2, T, B, W), dt, dev)
    tag = f"to_step_frame/{'bf16' if bf else 'f32'}(ids={use_ids},{B}x{T},W={W},doff={doff})"
    src = _flat(table, dev)
    k.to_step_frame(src, ids.to(dev) if use_ids else None, rev.to(dev), ov, B, T, W, doff)
    _sync(dev)
    _eq(tag, ov, want)
    o.intact(tag)
    return 2 * T * B * (W * table.element_size() // 16)


def run_from_step_frame(k, dev, B, T, W):
    g = _gen(22, B, T, W)
    rev = _lens_rev(g, B, T)
    _check_rev(rev, B, T)
    x = torch.randn(2, T, B, W, generator=g)
    bw = torch.gather(x[1].permute(1, 0, 2), 1, rev[:, :, None].expand(B, T, W))  # [B][T][W]: in[1][rev[b][t]][b]
    want = (x[0].permute(1, 0, 2).double() + bw.double()).float()
    o, ov = _out((B, T, W), F32, dev)
    tag = f"from_step_frame({B}x{T},W={W})"
    k.from_step_frame(_flat(x, dev), rev.to(dev), ov, B, T, W)
    _sync(dev)
    _eq(tag, ov, want)
    o.intact(tag)
    return B * T * (W // 4)


def run_step_frame_hop(k, dev, B, T, H):
    """out[0][t][b] = in[0][t][b][0:H] + in[1][rev][b][0:H];  out[1][t][b] = in[0][rev][b][H:2H] + in[1][t][b][H:2H]"""
    g = _gen(23, B, T, H)
    rev = _lens_rev(g, B, T)
    _check_rev(rev, B, T)
    x = torch.randn(2, T, B, 2 * H, generator=g)
    r = rev.t()[:, :, None].expand(T, B, 2 * H)  # [T][B]: rev[b][t]
    at_rev = [torch.gather(x[p], 0, r) for p in range(2)]  # in[p][rev[b][t]][b]
    want = torch.stack([x[0][:, :, :H].double() + at_rev[1][:, :, :H].double(),
                        at_rev[0][:, :, H:].double() + x[1][:, :, H:].double()]).float()
    o, ov = _out((2, T, B, H), F32, dev)
    tag = f"step_frame_hop({B}x{T},H={H})"
    k.step_frame_hop(_flat(x, dev), rev.to(dev), ov, B, T, H)
    _sync(dev)
    _eq(tag, ov, want)
    o.intact(tag)
    return 2 * T * B * (H // 4)


def run_tr01(k, dev, P, Q, R, mode):
    g = _gen(24, P, Q, R, len(mode))
    x = _with_specials(torch.randn(P, Q, R, generator=g)) if "b" in mode else torch.randn(P, Q, R, generator=g)
    base = torch.randn(Q, P, R, generator=g) if mode == "acc" else None
    want = x.transpose(0, 1).contiguous()
    tag = f"tr01({P},{Q},{R},{mode})"
    o = ob = None
    if mode in ("out", "both", "acc"):
        o, ov = _out((Q, P, R), F32, dev, SENT if base is not None else NAN, base)
    if mode in ("outb", "both"):
        ob, obv = _out((Q, P, R), BF, dev)
    k.tr01(_flat(x, dev), ov if o else None, obv if ob else None, P, Q, R, mode == "acc")
    _sync(dev)
    if o:
        _eq(tag, ov, (want.double() + base.double()).float() if mode == "acc" else want)
        o.intact(tag)
    if ob:
        _eq(tag + " outb", obv, want.bfloat16(), "bf16")
        ob.intact(tag + " outb")


def run_tr01_refusals(k, dev):
    x = _flat(torch.zeros(2, 3, 8), dev)
    _, o = _out((3, 2, 8), F32, dev)
    _, ob = _out((3, 2, 8), BF, dev)
    _refused("tr01 R % 4", lambda: k.tr01(_flat(torch.zeros(2, 3, 6), dev), _out((3, 2, 6), F32, dev)[1], None, 2, 3, 6, False))
    _refused("tr01 acc with outb", lambda: k.tr01(x, o, ob, 2, 3, 8, True))
    _refused("tr01 acc without out", lambda: k.tr01(x, None, ob, 2, 3, 8, True))
    _refused("tr01 in offset", lambda: k.tr01(_flat(torch.zeros(2, 3, 8), dev, 1), o, None, 2, 3, 8, False))
    _refused("tr01 out offset", lambda: k.tr01(x, _out((3, 2, 8), F32, dev, shift=1)[1], None, 2, 3, 8, False))
    _refused("tr01 outb offset", lambda: k.tr01(x, None, _out((3, 2, 8), BF, dev, shift=1)[1], 2, 3, 8, False))
    _sync(dev)


def run_transpose_bta(k, dev, B, T, A):
    g = _gen(25, B, T, A)
    x = torch.randn(B, T, A, generator=g).bfloat16()
    want = torch.empty(B, A, T, dtype=BF)
    for b in range(B):
        for t in range(T):
            want[b, :, t] = x[b, t, :]
    o, ov = _out((B, A, T), BF, dev)
    tag = f"transpose_bta({B},{T},{A})"
    k.transpose_bta(_flat(x, dev), ov, B, T, A)
    _sync(dev)
    _eq(tag, ov, want)
    o.intact(tag)


def run_alignment_refusals(k, dev):
    """The frame and column-sum kernels use 16-byte (fp32) and 8-byte (bf16) vector accesses: a contiguous view one
    element off must be refused; colsum's and transpose_bta's element-by-element paths take any view."""
    z, B, T = torch.zeros, 2, 3
    rev = _lens_rev(_gen(26), B, T).to(dev)
    for sh_in, sh_out in ((1, 0), (0, 1)):
        tag = f"(in +{sh_in}, out +{sh_out})"
        _refused("to_step_frame " + tag, lambda: k.to_step_frame(_flat(z(B * T, 8, dtype=BF), dev, sh_in), None, rev,
                                                                 _out((2, T, B, 8), BF, dev, shift=sh_out)[1], B, T, 8, 0))
        _refused("from_step_frame " + tag, lambda: k.from_step_frame(_flat(z(2, T, B, 4), dev, sh_in), rev,
                                                                     _out((B, T, 4), F32, dev, shift=sh_out)[1], B, T, 4))
        _refused("step_frame_hop " + tag, lambda: k.step_frame_hop(_flat(z(2, T, B, 8), dev, sh_in), rev,
                                                                   _out((2, T, B, 4), F32, dev, shift=sh_out)[1], B, T, 4))
        _refused("transpose_bta " + tag, lambda: k.transpose_bta(_flat(z(2, 4, 64, dtype=BF), dev, sh_in),
                                                                 _out((2, 64, 4), BF, dev, shift=sh_out)[1], 2, 4, 64))
        _refused("cast_colsum " + tag, lambda: k.cast_colsum(_flat(z(3, 8), dev, sh_in), _out((3, 8), BF, dev, shift=sh_out)[1],
                                                             _out((8,), F32, dev, 0.0)[1], 3, 8))
    _refused("colsum f32", lambda: k.colsum(_flat(z(3, 8), dev, 1), _out((8,), F32, dev)[1], 3, 8, False))
    _refused("colsum bf16", lambda: k.colsum(_flat(z(3, 8, dtype=BF), dev, 1), _out((8,), F32, dev)[1], 3, 8, False))
    _sync(dev)


# ------------------------------------------------------------------ runners: beam_gather
def run_beam_gather(k, dev, H, A, T, E, cov, with_step):
    g = _gen(27, H, A, T, E, cov, with_step)
    R, V, unk = 12, 37, 3
    gidx = torch.tensor([5, 0, 0, 11, 7, 7, 7, 2, 1, 10, 5, 4], dtype=I32)  # repeats; parents 3, 6, 8, 9 unused
    latest = torch.tensor([0, V - 1, V, V + 1, 2 ** 31 - 2, 50000, 17, 17, 5, V, 1, 36], dtype=I32)  # below, at, far above V
    used_p = torch.zeros(R, dtype=torch.bool)
    used_p[gidx.long()] = True
    tok = [int(v) if int(v) < V else unk for v in latest]
    used_t = torch.zeros(V, dtype=torch.bool)
    used_t[tok] = True
    assert not bool(used_p.all()) and not bool(used_t.all()) and bool(used_t[unk])

    def rows(n, w, used, dt=F32):
        t = torch.randn(n, w, generator=g).to(dt)
        t[~used] = NAN
        return t

    c_src, h_src, ctx_src = rows(R, H, used_p), rows(R, H, used_p, BF), _with_specials(rows(R, A, used_p))
    ctx_src[~used_p] = NAN
    a_src, cov_src = rows(R, T, used_p), rows(R, T, used_p)
    XGtab, Xtab = rows(V, 4 * H, used_t), rows(V, E, used_t)
    want = {"c": torch.empty(R, H), "h": torch.empty(R, H, dtype=BF), "ctx": torch.empty(R, A), "cov": torch.empty(R, T),
            "XG": torch.empty(R, 4 * H), "x": torch.empty(R, E)}
    for r in range(R):
        p = int(gidx[r])
        want["c"][r], want["h"][r], want["ctx"][r] = c_src[p], h_src[p], ctx_src[p]
        want["cov"][r] = (cov_src[p].double() + a_src[p].double()).float()
        want["XG"][r], want["x"][r] = XGtab[tok[r]], Xtab[tok[r]]
    outs = {n: _out(s, dt, dev) for n, s, dt in (("c", (R, H), F32), ("h", (R, H), BF), ("ctx", (R, A), F32), ("ctxb", (R, A), BF),
                                                ("cov", (R, T), F32), ("XG", (R, 4 * H), F32), ("x", (R, E), F32))}
    stp = torch.full((9,), -7, dtype=I32)
    stp[4] = 41
    stp = stp.to(dev)
    f = lambda t: _flat(t, dev)
    tag = f"beam_gather(H={H},A={A},T={T},E={E},cov={cov},step={with_step})"
    k.beam_gather(f(gidx), f(latest), f(c_src), f(h_src), f(ctx_src), f(a_src), f(cov_src) if cov else None, f(XGtab), f(Xtab), outs["c"][1], outs["h"][1], outs["ctx"][1],
                  outs["ctxb"][1], outs["cov"][1] if cov else None, outs["XG"][1], outs["x"][1], R, H, A, T, E, V, unk,
                  stp[4:5] if with_step else None)
    _sync(dev)
    for n in ("c", "h", "ctx", "XG", "x") + (("cov",) if cov else ()):
        _eq(f"{tag} {n}", outs[n][1], want[n])
    _eq(f"{tag} ctxb", outs["ctxb"][1], want["ctx"].bfloat16(), "bf16")
    _eq(f"{tag} ctxb of ctx_out", outs["ctxb"][1], outs["ctx"][1].cpu().bfloat16(), "bf16")
    for n, (o, _) in outs.items():
        o.intact(f"{tag} {n}", untouched=(n == "cov" and not cov))
    assert stp.cpu().tolist() == [-7] * 4 + [42 if with_step else 41] + [-7] * 4, f"{tag}: step: {stp.cpu().tolist()}"


def run_beam_gather_refusals(k, dev):
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt).to(dev)
    a = lambda cov_src, cov_out, unk: k.beam_gather(z(2, dt=I32), z(2, dt=I32), z(2, 4), z(2, 4, dt=BF), z(2, 4), z(2, 3), cov_src,
                                                    z(5, 16), z(5, 4), z(2, 4), z(2, 4, dt=BF), z(2, 4), z(2, 4, dt=BF), cov_out,
                                                    z(2, 16), z(2, 4), 2, 4, 4, 3, 4, 5, unk, None)
    _refused("beam_gather cov_out without cov_src", lambda: a(None, z(2, 3), 0))
    _refused("beam_gather unk == V", lambda: a(None, None, 5))
    _sync(dev)


# ------------------------------------------------------------------ runners: column sums
def _cs_vals(g, shape, kind, bf=False):
    x = torch.randint(-8, 9, shape, generator=g).float() if kind == "exact" else torch.randn(shape, generator=g)
    return x.bfloat16() if bf else x


def _cs_check(tag, got, x, pre, d, kind):
    """got against pre + sum_n x (float64): exact inputs bit for bit, general within d U sum |x| + U |out|"""
    got = got.detach().cpu()
    xd = x.double()
    full, mag = xd.sum(0) + (0 if pre is None else pre.double()), xd.abs().sum(0)
    assert got.shape == full.shape and got.dtype == F32, (tag, got.shape, got.dtype)
    if kind == "exact":
        top = float(mag.max()) + (0 if pre is None else float(pre.abs().max()))
        assert top < 2 ** 24 and torch.equal(xd.round(), xd) and torch.equal(full.round(), full)  # every partial sum an integer below 2^24
        _eq(tag, got, full.float())
        return
    bound = d * U24 * mag + U24 * full.abs()
    err = (got.double() - full).abs()
    ok = err <= bound
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).nan_to_num(nan=float("inf")).max()) if bool(pos.any()) else 0.0
    print(f"ERR/BOUND {tag} d={d} {ratio:.4f}")
    assert bool(ok.all()), f"{tag}: bound: {int((~ok).sum())} of {ok.numel()} columns outside the bound, largest err / bound " \
                           f"{ratio:.3g}, first at {(~ok).nonzero()[0].tolist()}"


def run_cast_colsum(k, dev, kind, N, C):
    g = _gen(28, N, C, kind == "exact")
    x = _with_specials(torch.randn(N, C, generator=g)) if kind == "special" else _cs_vals(g, (N, C), kind)
    pre = torch.randint(-64, 65, (C,), generator=g).float() if kind == "exact" else torch.randn(C, generator=g)
    o, ov = _out((C,), F32, dev, SENT, pre)
    ob, obv = _out((N, C), BF, dev)
    tag = f"cast_colsum/{kind}({N},{C})"
    k.cast_colsum(_flat(x, dev), obv, ov, N, C)
    _sync(dev)
    _eq(tag + " xb", obv, x.bfloat16(), "bf16")
    if kind != "special":  # the specials (inf, NaN, 3.4e38) leave no column sum to judge
        _cs_check(tag, ov, x, pre, cast_colsum_depth(N, C), kind)
    o.intact(tag)
    ob.intact(tag + " xb")


def run_colsum(k, dev, kind, N, C, bf, acc):
    g = _gen(29, N, C, bf, acc, kind == "exact")
    x = _cs_vals(g, (N, C), kind, bf)
    pre = (torch.randint(-64, 65, (C,), generator=g).float() if kind == "exact" else torch.randn(C, generator=g)) if acc else None
    tag = f"colsum/{kind}/{'bf16' if bf else 'f32'}({N},{C},acc={acc})"
    xd = _flat(x, dev)
    o, ov = _out((C,), F32, dev, SENT if acc else NAN, pre)
    k.colsum(xd, ov, N, C, acc)
    _sync(dev)
    _cs_check(tag, ov, x, pre, colsum_depth(N, C), kind)
    o.intact(tag)
    o2, ov2 = _out((C,), F32, dev, SENT if acc else NAN, pre)
    k.colsum(xd, ov2, N, C, acc)
    _sync(dev)
    _same_bits(tag, ov2, ov)


# ------------------------------------------------------------------ runners: pack_cast
def _combos():
    return [(f, s) for f in (0, 1) for s in (None, K2LOG2E)]


def geom_k1(ar, n, f32o, scale):
    ar.add((n,), (1,), (1,), f32o, scale, (1, -(-n // 2048)))


def geom_tr(ar, R, C, f32o, scale):
    """dst [R][C] contiguous, src the transpose view of a contiguous [C][R]; a 1 x n or n x 1 pair is contiguous"""
    kind = (1, -(-R * C // 2048)) if R == 1 or C == 1 else (2, -(-R // 64) * -(-C // 64))
    ar.add((R, C), (1, R), (C, 1), f32o, scale, kind)


def geom_rows(ar, R, C, f32o, scale, spad=4, dpad=8):
    ar.add((R, C), (C + spad, 1), (C + dpad, 1), f32o, scale, (3, -(-R * C // 2048)))


def geom_gates(ar, din, H, which, f32o, scale):
    """the engine's gate permutations of a [din][4][H] block: (0, 2, 1) -> [din][H][4], (2, 1, 0) -> [H][4][din]"""
    if which == 0:
        ar.add((din, H, 4), (4 * H, 1, H), (4 * H, 4, 1), f32o, scale, (0, -(-din * 4 * H // 256)))
    else:
        ar.add((H, 4, din), (1, H, 4 * H), (4 * din, din, 1), f32o, scale, (0, -(-din * 4 * H // 256)))


def geom_colslice_t(ar, R, C, f32o, scale):
    """a column slice of a wider destination from a transposed source (WcT2[:, :A] = W.t()): generic"""
    ar.add((R, C), (1, R), (C + 16, 1), f32o, scale, (0, -(-R * C // 256)), dshift=8)


def geom_unaligned(ar, n, f32o, scale):
    """a contiguous pair whose source is only 4-byte aligned: falls back from kind 1 to the generic kind"""
    ar.add((n,), (1,), (1,), f32o, scale, (0, -(-n // 256)), sshift=1)


def run_pack(k, dev, name, build, expect_nj=None):
    """build(ar) adds the jobs; classify, validate on the host, launch once, compare both arenas whole"""
    from textsummarization_on_flink_amd.models.pointer_generator import pack_job_rows
    ar = Arenas()
    build(ar)
    ar.build(_gen(30, len(name), len(ar.specs), sum(map(ord, name))), dev)
    tag = f"pack_cast/{name}"
    rows, total = pack_job_rows(ar.pairs(), int(k.pack_max_jobs()))
    assert rows is not None and len(rows) == len(ar.specs) == (expect_nj or len(rows)) and len(rows[0]) == int(k.pack_job_cols())
    blk = 0
    for i, (row, sp) in enumerate(zip(rows, ar.specs)):
        kind, nblk = sp["kind"]
        assert (row[12], row[11]) == (kind, blk), f"{tag}: classifier: job {i} {sp['shape']} kind {row[12]} at workgroup {row[11]}, " \
                                                   f"want kind {kind} at {blk}"
        assert row[13] == sp["f32o"] and row[14] == math.prod(sp["shape"]) and bool(row[15]) == bool(sp["scale"])
        blk += nblk
    assert total == blk, f"{tag}: classifier: {total} workgroups, want {blk}"
    ar.validate(tag, rows, total)
    getattr(k, "bind_arenas", lambda a: None)(ar)
    k.pack_cast(torch.tensor(rows, dtype=torch.long).to(dev), total)
    _sync(dev)
    ar.check(tag)
    return rows, total


PACK_K1 = [1, 7, 8, 2047, 2048, 2049, 2055]
PACK_K2 = [(63, 65), (64, 64), (130, 70), (1, 200), (200, 1)]
PACK_K3 = [(3, 8), (5, 520), (300, 24)]
PACK_GATES = [(3, 5), (32, 20)]


def pack_cases():
    """name -> build(ar)"""
    cases = {}
    for n in PACK_K1:
        cases[f"k1 n={n}"] = lambda ar, n=n: [geom_k1(ar, n, f, s) for f, s in _combos()]
    for R, C in PACK_K2:
        cases[f"k2 {R}x{C}"] = lambda ar, R=R, C=C: [geom_tr(ar, R, C, f, s) for f, s in _combos()]
    for R, C in PACK_K3:
        cases[f"k3 {R}x{C}"] = lambda ar, R=R, C=C: [geom_rows(ar, R, C, f, s, 4 + 8 * i, 8) for i, (f, s) in enumerate(_combos())]
    for din, H in PACK_GATES:
        cases[f"k0 gates {din}x{H}"] = lambda ar, din=din, H=H: [geom_gates(ar, din, H, w, f, s) for w in (0, 1) for f, s in _combos()]
    cases["k0 column slice"] = lambda ar: [geom_colslice_t(ar, R, C, f, s) for R, C in ((5, 24), (70, 40)) for f, s in _combos()]
    cases["k0 unaligned source"] = lambda ar: [geom_unaligned(ar, n, f, s) for n in (8, 300) for f, s in _combos()]
    cases["one job"] = lambda ar: geom_k1(ar, 1, 0, None)

    def small64(ar):  # 64 one-workgroup jobs of mixed kinds
        for i in range(16):
            f, s = _combos()[i % 4]
            geom_k1(ar, 1 + 97 * i, f, s)
            geom_tr(ar, 3 + i, 5 + 2 * i, 1 - f, s)
            geom_rows(ar, 2 + i, 8 * (1 + i % 3), f, s)
            geom_gates(ar, 2, 3 + i, i % 2, 1 - f, s)
    cases["64 one-workgroup jobs"] = small64

    def mixed(ar):  # large jobs with one-workgroup neighbours on both sides
        geom_k1(ar, 7, 0, None)
        geom_k1(ar, 3 * 2048 + 1, 0, K2LOG2E)
        geom_rows(ar, 3, 8, 1, None)
        geom_tr(ar, 130, 70, 0, None)
        geom_unaligned(ar, 5, 0, K2LOG2E)
        geom_tr(ar, 2, 2, 1, K2LOG2E)
        geom_gates(ar, 32, 20, 1, 0, None)
        geom_k1(ar, 1, 1, None)
        geom_rows(ar, 300, 24, 0, K2LOG2E)
        geom_colslice_t(ar, 70, 40, 1, None)
        geom_k1(ar, 2055, 0, None)
    cases["large and one-workgroup jobs"] = mixed
    return cases


def run_pack_refusals(k, dev):
    from textsummarization_on_flink_amd.models.pointer_generator import pack_job_rows
    mj, cols = int(k.pack_max_jobs()), int(k.pack_job_cols())
    assert (mj, cols) == (64, 16)
    z = lambda r, c: torch.zeros(r, c, dtype=torch.long).to(dev)
    _refused("pack_cast 65 rows", lambda: k.pack_cast(z(mj + 1, cols), 1))
    _refused("pack_cast 0 rows", lambda: k.pack_cast(z(0, cols), 1))
    _refused("pack_cast row length", lambda: k.pack_cast(z(1, cols + 1), 1))
    _refused("pack_cast row length", lambda: k.pack_cast(z(1, cols - 1), 1))
    _sync(dev)
    ar = Arenas()
    for _ in range(mj + 1):
        geom_k1(ar, 8, 0, None)
    ar.build(_gen(32), "cpu")
    assert pack_job_rows(ar.pairs(), mj) == (None, 0), "beyond pack_max_jobs(): keep the torch path"
    rows, total = pack_job_rows(ar.pairs()[:mj], mj)
    assert len(rows) == mj and total == mj


# ------------------------------------------------------------------ the cases (profiles/layout_op_tests.md: which line each reaches)
# bf16, ids, B, T, W, doff
TO_FRAME = [(True, True, 3, 5, 8, 0), (True, True, 7, 9, 128, 0), (False, False, 3, 5, 4, 4), (False, False, 7, 9, 64, 64),
            (True, False, 3, 5, 8, 8), (False, True, 7, 9, 4, 0)]
TO_FRAME_BIG = (False, False, 48, 352, 256, 256)  # 2 T B (W es / 16) = 2162688 > 8192 * 256
FROM_FRAME = [(2, 1, 4), (3, 5, 4), (7, 9, 64), (5, 33, 132)]
FRAME_BIG_BT = (48, 352)  # B T = 16896 > 16384: a second trip at W = 512 / H = 256
HOP = [(2, 1, 4), (3, 5, 4), (7, 9, 64), (5, 33, 36)]
# P, Q, R
TR01 = [(1, 5, 12), (6, 1, 8), (1, 1, 4), (3, 7, 12), (5, 9, 100), (4, 16, 16)]
TR01_MODES = ("out", "outb", "both", "acc")
BTA = [(B, T, A) for T in (3, 64, 68, 101) for A in (64, 192) for B in (1, 3)]
# H, A, T, E
GATHER = [(64, 128, 7, 32), (320, 512, 300, 300), (64, 512, 300, 32), (320, 128, 7, 300)]
# N, C
CAST_COLSUM = [(3, 4), (257, 4), (1, 8), (129, 8), (5, 256), (1025, 256), (300, 1024), (1, 1024)]
COLSUM = [(N, C) for C in (1, 3, 63, 64, 130, 260, 514) for N in (1, 63, 130)] + [(4225, 4)]


@pytest.mark.parametrize("case", TO_FRAME, ids=str)
def test_to_step_frame(case):
    assert run_to_step_frame(_ops(), "cuda", *case) <= GRID_CAP


def test_to_step_frame_second_grid_stride_trip():
    assert run_to_step_frame(_ops(), "cuda", *TO_FRAME_BIG) > GRID_CAP


@pytest.mark.parametrize("case", FROM_FRAME, ids=str)
def test_from_step_frame(case):
    assert run_from_step_frame(_ops(), "cuda", *case) <= GRID_CAP


def test_from_step_frame_second_grid_stride_trip():
    assert run_from_step_frame(_ops(), "cuda", *FRAME_BIG_BT, 512) > GRID_CAP


@pytest.mark.parametrize("case", HOP, ids=str)
def test_step_frame_hop(case):
    assert run_step_frame_hop(_ops(), "cuda", *case) <= GRID_CAP


def test_step_frame_hop_second_grid_stride_trip():
    assert run_step_frame_hop(_ops(), "cuda", *FRAME_BIG_BT, 256) > GRID_CAP


@pytest.mark.parametrize("mode", TR01_MODES)
@pytest.mark.parametrize("case", TR01, ids=str)
def test_tr01(case, mode):
    run_tr01(_ops(), "cuda", *case, mode)


def test_tr01_refusals():
    run_tr01_refusals(_ops(), "cuda")


@pytest.mark.parametrize("case", BTA, ids=str)
def test_transpose_bta(case):
    run_transpose_bta(_ops(), "cuda", *case)


def test_transpose_bta_refuses_a_partial_feature_tile():
    _refused("transpose_bta A = 96", lambda: run_transpose_bta(_ops(), "cuda", 1, 3, 96))


def test_offset_views_are_refused_by_the_vector_kernels():
    run_alignment_refusals(_ops(), "cuda")


@pytest.mark.parametrize("with_step", [False, True])
@pytest.mark.parametrize("cov", [False, True])
@pytest.mark.parametrize("case", GATHER, ids=str)
def test_beam_gather(case, cov, with_step):
    run_beam_gather(_ops(), "cuda", *case, cov, with_step)


def test_beam_gather_refusals():
    run_beam_gather_refusals(_ops(), "cuda")


@pytest.mark.parametrize("case", CAST_COLSUM, ids=str)
def test_cast_colsum(case):
    for kind in KINDS + ("special",):
        run_cast_colsum(_ops(), "cuda", kind, *case)


def test_cast_colsum_refusals():
    for C in (12, 2048):
        _refused(f"cast_colsum C = {C}", lambda: run_cast_colsum(_ops(), "cuda", "exact", 3, C))


def test_the_split_rules_reach_the_lines_the_cases_are_meant_for():
    assert cast_colsum_blocks(3, 4) == 1  # 3 rows, 256 row groups
    assert [cast_colsum_blocks(N, C) for N, C in ((257, 4), (129, 8), (5, 256), (1025, 256))] == [2, 2, 2, 256]
    assert cast_colsum_blocks(300, 1024) == 256  # rows 256 .. 299: 44 workgroups on a second trip
    assert (colsum_det_chunks(4225, 4), colsum_rpc(4225, 4)) == (66, 65) and 65 * 65 == 4225  # chunk 65 is empty
    assert [colsum_det_chunks(N, 3) for N in (1, 63, 130)] == [1, 1, 2]  # finish<1> on two partials


@pytest.mark.parametrize("case", COLSUM, ids=str)
def test_colsum(case):
    N, C = case
    if case == (4225, 4):
        G, rpc = colsum_det_chunks(N, C), colsum_rpc(N, C)
        assert (G - 1) * rpc >= N, "the last row chunk must be empty"
    for kind in KINDS:
        for bf in (False, True):
            for acc in (False, True):
                run_colsum(_ops(), "cuda", kind, N, C, bf, acc)


@pytest.mark.parametrize("name", list(pack_cases()))
def test_pack_cast(name):
    run_pack(_ops(), "cuda", name, pack_cases()[name])


def test_pack_cast_refusals_and_the_job_cap():
    run_pack_refusals(_ops(), "cuda")
