// Persistent decoder forward loop (projected attention, hidden 256): ONE launch runs all D steps of
//   cell (dec_cell_fwd) -> s-projection (linear2) -> row attention (attn_fwd_rowp)
// instead of three dependent launches per step and row group.  No data of a decoder step crosses a
// 16-row batch tile, so there is no grid-wide dependency to pay for:
//   * a TEAM = 16 workgroups owns one 16-row tile; workgroup j of a team owns hidden units
//     [16j, 16j + 16) of the cell (all four gates), columns [32j, 32j + 32) of the s-projection and
//     batch row j of the tile in the attention; 16 waves, as attn_fwd_rowp_kernel<1, 16>;
//   * its 64 x 384 slice of the cell weights and its 32 x 512 slice of W_s live in LDS for the whole
//     launch; the cell state c of its units never leaves registers;
//   * three hand-offs per step stay inside the team (handoff.h: tagged 8-byte granules, members on
//     one XCD): g_{t-1} (16 x 128 bf16) into the cell, [c_t, h_t] (16 x 512 bf16) into the
//     s-projection, s_t (fp32, each workgroup reads its own row) into the attention;
//   * the hand-off buffers are double-buffered by step parity: a slot of step t is rewritten at
//     step t + 2, which a member reaches only after every member has consumed step t (each later
//     hand-off needs all 16 members' contributions);
//   * every wait is bounded (sweep): a timeout records code 3 in *err and the grid drains.
// Arithmetic and summation order are those of the per-step kernels (K split in four slices summed
// in slice order; the attention body is shared, attn_rowp_fwd.h), so the results are bit-identical
// and every buffer the backward reads (Cst, Cb, Hb, ACT, S, ATT, ATTb, COV, GV, GVb) is written
// where the per-step kernels write it.
// Dead steps (EngineConfig.skip_pad_steps): a row past dlen writes the zeros attn_fwd_rowp writes
// and still serves its column slices while any row of its tile is live; a tile whose rows are all
// dead leaves the loop and only writes the zeros of its remaining steps.
#include "attn_rowp_fwd.h"
#include "handoff.h"
#include "launchers.h"
#include <mutex>

using namespace attn_rowp;
using namespace handoff;

namespace {

constexpr int kH = 256, kE = 128, kA = 512, kNC = 16, kNW = 16, kNT = kNW * 64;
constexpr int kKc = kE + kH;                       // cell K: [g | h]
constexpr int kWcS = kKc + 8, kWsS = 2 * kH + 8;   // LDS row strides (bf16), +16 bytes against bank conflicts
constexpr int kChS = 2 * kH + 8, kGtS = kE + 8;
// granules of one team: g [2][16][64 pairs], [c, h] [2][16][256 units], s [2][16][512]
constexpr int kGg = 16 * (kE / 2), kGch = 16 * kH, kGs = 16 * kA;
constexpr int kTeamGranules = 2 * (kGg + kGch + kGs);
// dynamic LDS carve (bytes, every offset a multiple of 16)
constexpr int oWc = 0;
constexpr int oWs = oWc + 64 * kWcS * 2;
constexpr int oCh = oWs + 32 * kWsS * 2;
constexpr int oGt = oCh + 16 * kChS * 2;
constexpr int oEs = oGt + 16 * kGtS * 2;
constexpr int oPart = oEs + kRowMaxT * 4;          // attention partials; the K-split sums of the GEMMs alias it
constexpr int oSrow = oPart + kNW * 4 * kEG * 4;
constexpr int oMisc = oSrow + kA * 4;
constexpr int kLds = oMisc + 3 * kNW * 4;
static_assert(oWs % 16 == 0 && oCh % 16 == 0 && oGt % 16 == 0 && oEs % 16 == 0 && oPart % 16 == 0 && oSrow % 16 == 0 &&
              oMisc % 16 == 0, "LDS carve alignment");
static_assert(kLds <= 160 * 1024, "LDS of one CU");
static_assert(4 * 4 * 256 * 4 <= kNW * 4 * kEG * 4, "K-split partials fit the attention partial buffer");

}  // namespace

struct DecPersistentArgs {
  const float* XG;     // [D][B][4H]
  const bf16* KcT;     // [4H][E+H]
  const bf16* WsT;     // [A][2H]
  const float* bs;     // [A]
  float* Cst;          // [D+1][B][H]
  bf16* Cb;            // [D+1][B][H]
  bf16* Hb;            // [D+1][B][H]
  float* ACT;          // [D][B][4H]
  float* S;            // [D][B][A]
  const bf16* F;       // [B][T][A]
  const bf16* G;       // [B][T][E]
  const float* v;      // [A]
  const float* wc;     // [A] (nullable)
  float* COV;          // [D+1][B][T] (nullptr: no coverage)
  const int* lens;     // [B]
  float* ATT;          // [D][B][T]
  bf16* ATTb;          // [D][B][T]
  float* covloss;      // [D][B] (nullptr: no coverage)
  float* GV;           // [D][B][E]
  bf16* GVb;           // [D][B][E]
  const int* dlen;     // [B] (nullable)
  gu64* xbuf;          // [B/16][kTeamGranules], zeroed before the launch
  gu32* err;
  int B, T, D;
};

__global__ __launch_bounds__(kNT) void dec_fwd_persistent_kernel(DecPersistentArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* Wc = reinterpret_cast<bf16*>(smem + oWc);
  bf16* Ws = reinterpret_cast<bf16*>(smem + oWs);
  bf16* ch = reinterpret_cast<bf16*>(smem + oCh);
  bf16* gt = reinterpret_cast<bf16*>(smem + oGt);
  float* es = reinterpret_cast<float*>(smem + oEs);
  float(*part)[4][kEG] = reinterpret_cast<float(*)[4][kEG]>(smem + oPart);
  float* red = reinterpret_cast<float*>(smem + oPart);
  float* srow = reinterpret_cast<float*>(smem + oSrow);
  float* wm = reinterpret_cast<float*>(smem + oMisc);
  float* wl = wm + kNW;
  float* redw = wl + kNW;

  const int B = p.B, T = p.T, D = p.D;
  int team, j;
  if (!team_of(kNC, B / 16, team, j)) return;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int r0 = team * 16, b = r0 + j;
  const int l15 = lane & 15, kof = 8 * (lane >> 4);
  gu64* gbuf = p.xbuf + (size_t)team * kTeamGranules;
  gu64* chbuf = gbuf + 2 * kGg;
  gu64* sbuf = chbuf + 2 * kGch;

  // steps the tile / this workgroup's attention row are live for
  int tile_last = D, row_last = D;
  if (p.dlen) {
    tile_last = 0;
    for (int i = 0; i < 16; ++i) tile_last = max(tile_last, p.dlen[r0 + i]);
    tile_last = min(tile_last, D);
    row_last = p.dlen[b];
  }

  // weight slices and h_0 into LDS
  for (int i = tid; i < 64 * (kKc / 8); i += kNT) {
    const int row = i / (kKc / 8), c8 = i % (kKc / 8);
    const int grow = (row >> 4) * kH + 16 * j + (row & 15);  // gate-major rows of KcT
    *reinterpret_cast<bf16x8*>(Wc + row * kWcS + c8 * 8) = ld8(p.KcT + (size_t)grow * kKc + c8 * 8);
  }
  for (int i = tid; i < 32 * (2 * kH / 8); i += kNT) {
    const int row = i / (2 * kH / 8), c8 = i % (2 * kH / 8);
    *reinterpret_cast<bf16x8*>(Ws + row * kWsS + c8 * 8) = ld8(p.WsT + (size_t)(32 * j + row) * (2 * kH) + c8 * 8);
  }
  if (tid < 16 * (kH / 8)) {
    const int row = tid / (kH / 8), c8 = tid % (kH / 8);
    *reinterpret_cast<bf16x8*>(ch + row * kChS + kH + c8 * 8) = ld8(p.Hb + (size_t)(r0 + row) * kH + c8 * 8);
  }
  // the cell's (row, unit) of this thread (waves 0-3, the accumulator register wid of the MFMA tile)
  const int crow = (lane >> 4) * 4 + (wid & 3), cu = 16 * j + l15;
  const size_t cri = (size_t)(r0 + crow) * kH + cu;
  float cstate = wid < 4 ? p.Cst[cri] : 0.f;
  const size_t BH = (size_t)B * kH, BT = (size_t)B * T;
  bool dead = false;

  for (int t = 0; t < tile_last; ++t) {
    const unsigned tag = (unsigned)t + 1u;
    const int par = t & 1;
    // per-step copies of the attention's loop-invariant operands, opaque to the compiler: hoisted out
    // of the step loop, v / w_c and the row addresses would sit in registers (and spill) through the
    // cell and s-projection phases
    const bf16 *Fp = p.F, *Gp = p.G;
    const float *vp = p.v, *wcp = p.wc;
    asm volatile("" : "+s"(Fp), "+s"(Gp), "+s"(vp), "+s"(wcp));
    // ---- cell: z = XG_t + [g_{t-1}, h_{t-1}] . Wc^T
    float xg[4] = {0.f, 0.f, 0.f, 0.f};
    if (wid < 4) {
      const float* xr = p.XG + ((size_t)t * B + r0 + crow) * (4 * kH);
#pragma unroll
      for (int g = 0; g < 4; ++g) xg[g] = xr[g * kH + cu];
    }
    if (t > 0) {  // g_{t-1}: wave wid takes row wid (64 bf16 pairs)
      unsigned gv[1] = {0u};
      sweep<1>(gbuf + (par ^ 1) * kGg, wid * 64, tag - 1u, gv, dead, p.err, 3u, lane);
      *reinterpret_cast<unsigned*>(gt + wid * kGtS + 2 * lane) = gv[0];
    }
    __syncthreads();
    {
      // wave (gate, K slice): the four K slices of dec_cell_fwd's four waves (t == 0: h only)
      const int gate = wid & 3, ks = wid >> 2;
      const int ib = t > 0 ? 0 : kE / 32, nst = kKc / 32 - ib;
      const int i0 = ib + ks * nst / 4, i1 = ib + (ks + 1) * nst / 4;
      const bf16* wrow = Wc + (gate * 16 + l15) * kWcS + kof;
      const bf16* grow = gt + l15 * kGtS + kof;
      const bf16* hrow = ch + l15 * kChS + kH - kE + kof;  // indexed with k >= kE
      f32x4 acc = f32x4{0, 0, 0, 0};
      for (int i = i0; i < i1; ++i) {
        const int k = 32 * i;
        const bf16x8 a = k < kE ? ld8(grow + k) : ld8(hrow + k);
        acc = mfma16(a, ld8(wrow + k), acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((ks * 4 + gate) * 4 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wid < 4) {
      float z[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float s = 0.f;
#pragma unroll
        for (int src = 0; src < 4; ++src) s += red[((src * 4 + g) * 4 + wid) * 64 + lane];
        z[g] = s;
      }
      const float ig = fsigmoid(z[0] + xg[0]), jg = ftanh(z[1] + xg[1]);
      const float fg = fsigmoid(z[2] + xg[2] + 1.0f), og = fsigmoid(z[3] + xg[3]);
      const float c = fg * cstate + ig * jg;
      const float h = og * ftanh(c);
      cstate = c;
      store_granule(chbuf + par * kGch + crow * kH + cu, tag, pack_bf2(c, h));
      const size_t o = (size_t)(t + 1) * BH + cri;
      p.Cst[o] = c;
      p.Cb[o] = f2bf(c);
      p.Hb[o] = f2bf(h);
      float* a4 = p.ACT + ((size_t)t * B + r0 + crow) * (4 * kH);
      a4[cu] = ig; a4[kH + cu] = jg; a4[2 * kH + cu] = fg; a4[3 * kH + cu] = og;
    }
    // ---- [c_t, h_t] of the tile: wave wid takes row wid (256 {c, h} granules)
    {
      unsigned cv[4] = {0u, 0u, 0u, 0u};
      sweep<4>(chbuf + par * kGch, wid * kH, tag, cv, dead, p.err, 3u, lane);
      unsigned short* crw = reinterpret_cast<unsigned short*>(ch + wid * kChS);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        crw[q * 64 + lane] = (unsigned short)(cv[q] & 0xffffu);
        crw[kH + q * 64 + lane] = (unsigned short)(cv[q] >> 16);
      }
    }
    __syncthreads();
    // ---- s-projection: s = [c, h] . Ws^T + b, two 16-column tiles, linear2's four K slices
    if (wid < 8) {
      const int nt = wid & 1, ks = wid >> 1;
      const bf16* arow = ch + l15 * kChS + kof;
      const bf16* wrow = Ws + (nt * 16 + l15) * kWsS + kof;
      f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int i = 4 * ks; i < 4 * ks + 4; ++i) acc = mfma16(ld8(arow + 32 * i), ld8(wrow + 32 * i), acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((ks * 2 + nt) * 4 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wid < 8) {
      const int w = wid & 3, nt = wid >> 2;
      float o = 0.f;
#pragma unroll
      for (int src = 0; src < 4; ++src) o += red[((src * 2 + nt) * 4 + w) * 64 + lane];
      const int row = (lane >> 4) * 4 + w, n = 32 * j + nt * 16 + l15;
      const float sv = o + p.bs[n] + 0.f;
      store_granule(sbuf + par * kGs + row * kA + n, tag, __float_as_uint(sv));
      p.S[((size_t)t * B + r0 + row) * kA + n] = sv;
    }
    // ---- attention of row j
    if (t < row_last && wid < 8) {
      unsigned sv[1] = {0u};
      sweep<1>(sbuf + par * kGs + j * kA, wid * 64, tag, sv, dead, p.err, 3u, lane);
      srow[wid * 64 + lane] = __uint_as_float(sv[0]);
    }
    __syncthreads();
    gu64* gdst = gbuf + par * kGg + j * (kE / 2);
    attn_fwd_rowp_body<1, kNW>(
        Fp, Gp, srow, vp, wcp, (p.COV && t > 0) ? p.COV + (size_t)t * BT : nullptr, p.lens,
        p.ATT + (size_t)t * BT, p.COV ? p.COV + (size_t)(t + 1) * BT : nullptr,
        p.covloss ? p.covloss + (size_t)t * B : nullptr, p.GV + (size_t)t * B * kE, p.GVb + (size_t)t * B * kE, T,
        p.dlen, t, p.ATTb + (size_t)t * BT, b, es, part, wm, wl, redw, [&](int k, float g) {
          const float gn = __shfl_xor(g, 1, 64);  // (waves 0 and 1, all lanes)
          if (!(k & 1)) store_granule(gdst + (k >> 1), tag, pack_bf2(g, gn));
        });
  }
  // ---- the tile's dead steps: the zeros dec_cell_fwd and attn_fwd_rowp write (coverage carried)
  for (int t = tile_last; t < D; ++t) {
    if (wid < 4) {
      const size_t o = (size_t)(t + 1) * BH + cri;
      p.Cst[o] = 0.f;
      p.Cb[o] = f2bf(0.f);
      p.Hb[o] = f2bf(0.f);
      float* a4 = p.ACT + ((size_t)t * B + r0 + crow) * (4 * kH);
      a4[cu] = 0.f; a4[kH + cu] = 0.f; a4[2 * kH + cu] = 0.f; a4[3 * kH + cu] = 0.f;
    }
    __syncthreads();  // (the coverage written for step t by other threads of this workgroup)
    attn_fwd_rowp_body<1, kNW>(
        p.F, p.G, srow, p.v, p.wc, (p.COV && t > 0) ? p.COV + (size_t)t * BT : nullptr, p.lens,
        p.ATT + (size_t)t * BT, p.COV ? p.COV + (size_t)(t + 1) * BT : nullptr,
        p.covloss ? p.covloss + (size_t)t * B : nullptr, p.GV + (size_t)t * B * kE, p.GVb + (size_t)t * B * kE, T,
        p.dlen, t, p.ATTb + (size_t)t * BT, b, es, part, wm, wl, redw, [](int, float) {});
  }
}

// ------------------------------------------------------------------------------ host side
bool dec_persistent_shape_ok(int H, int E, int A, int B, int T) {
  return H == kH && E == kE && A == kA && B >= 16 && B % 16 == 0 && T >= 1 && T <= kRowMaxT;
}

// workgroups of a launch: teams are dealt 8 at a time (one per XCD), 16 members each
int dec_persistent_grid(int B) { return B >= 16 && B % 16 == 0 ? 8 * kNC * ((B / 16 + 7) / 8) : 0; }

size_t dec_persistent_xbuf_elems(int B) { return (size_t)(B / 16) * kTeamGranules; }

// workgroups the current device keeps resident at once (one per CU when the occupancy query admits
// the kernel with its LDS; 0 when it does not or there is no device).  The count assumes the launch
// has every CU of the device to itself: see dec_persistent_eligible (models/engine_config.py) for
// the invariant the engine keeps.
int dec_persistent_capacity() {
  static std::mutex mu;
  static int cache[64] = {};  // [device] -> capacity + 1 (guarded by mu)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (cache[dev]) return cache[dev] - 1;
  int cus = 0, occ = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
  bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(dec_fwd_persistent_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLds) == hipSuccess;
  ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, dec_fwd_persistent_kernel, kNT, kLds) == hipSuccess;
  const int cap = (ok && occ >= 1) ? cus : 0;
  cache[dev] = cap + 1;
  return cap;
}

void launch_dec_fwd_persistent(const float* XG, const bf16* KcT, const bf16* WsT, const float* bs, float* Cst, bf16* Cb,
                               bf16* Hb, float* ACT, float* S, const bf16* F, const bf16* G, const float* v,
                               const float* wc, float* COV, const int* lens, float* ATT, bf16* ATTb, float* covloss,
                               float* GV, bf16* GVb, const int* dlen, unsigned long long* xbuf, unsigned* err, int B,
                               int T, int D, hipStream_t st) {
  const int grid = dec_persistent_grid(B);
  if (grid <= 0 || grid > dec_persistent_capacity()) return;  // the binding checks both first
  DecPersistentArgs p{XG, KcT, WsT, bs, Cst, Cb, Hb, ACT, S, F, G, v, wc, COV, lens, ATT, ATTb, covloss, GV, GVb, dlen,
                      (gu64*)xbuf, (gu32*)err, B, T, D};
  hipLaunchKernelGGL(dec_fwd_persistent_kernel, dim3(grid), dim3(kNT), kLds, st, p);
}
