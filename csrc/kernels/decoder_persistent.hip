// Persistent decoder forward loop (projected attention, hidden 256): ONE launch runs all D steps of
//   cell (dec_cell_fwd) -> s-projection (linear2) -> row attention (attn_fwd_rowp)
// instead of three dependent launches per step and row group.  No data of a decoder step crosses a
// 16-row batch tile, so there is no grid-wide dependency to pay for:
//   * a TEAM = 16 workgroups owns one 16-row tile; workgroup j of a team owns hidden units
//     [16j, 16j + 16) of the cell (all four gates), columns [32j, 32j + 32) of the s-projection and
//     batch row j of the tile in the attention; 16 waves, as attn_fwd_rowp_kernel<1, 16>;
//   * its 64 x 384 slice of the cell weights and its 32 x 512 slice of W_s live in LDS for the whole
//     launch, and so do the attention's loop-invariant operands (v, w_c . 2 log2(e)) and the
//     coverage of its row; the cell state c of its units never leaves registers;
//   * three hand-offs per step stay inside the team (handoff.h: tagged 8-byte granules, members on
//     one XCD): g_{t-1} (16 x 128 bf16) into the cell, [c_t, h_t] (16 x 512 bf16) into the
//     s-projection, s_t (fp32, each workgroup reads its own row) into the attention;
//   * every wait is bounded (sweep): a timeout records kErrDecFwd in *err and the grid drains.
// Order of a step in one workgroup (P = publish, W = sweep, st = plain global stores):
//   W g_{t-1} | cell | P [c,h]_t | W [c,h]_t | s-projection | P s_t | W s_t (own row) |
//   first F / G loads | st Cst Cb Hb ACT S | position loop | P g_t | st ATT ATTb COV covloss
// gfx9 counts loads and stores in one in-order vmcnt, so a store in front of a sweep makes the sweep
// wait for that store's write acknowledgement.  The cell's and the s-projection's outputs are
// therefore held in registers (6 + 1) and stored behind the attention's first loads, where the
// position loop follows; nothing but the publish itself sits between a publish and the next sweep
// of the cell and the s-projection.  (The attention's T-position tail is the one store group that
// still precedes a sweep, the next step's g: its values exist only after the publish.)
// Double-buffering: the hand-off buffers have two slots, by step parity; a slot of step t is
// rewritten at step t + 2.  Only the order of publishes and sweeps matters for it, and that order is
// the one above for every member:
//   * g: a member publishes g_{t+2} after it received s_{t+2}, which needs every member's
//     [c,h]_{t+2}, which each computed after its sweep of g_{t+1}, i.e. after its sweep of g_t;
//   * [c,h]: a member publishes [c,h]_{t+2} after its sweep of g_{t+1}, which needs every member's
//     attention of step t + 1, hence its sweep of [c,h]_{t+1}, which follows its sweep of [c,h]_t;
//   * s: row j of the s slot is read by member j alone; the others rewrite it at step t + 2 after
//     sweeping [c,h]_{t+2}, which contains member j's part, published after j's attention of step
//     t + 1 and so after its sweep of s_t (a member whose row is dead never reads its s).
// Arithmetic and summation order are those of the per-step kernels (K split in four slices summed
// in slice order; the attention body is shared, attn_rowp_fwd.h), so the results are bit-identical
// and every buffer the backward reads (Cst, Cb, Hb, ACT, S, ATT, ATTb, COV, GV, GVb) is written
// where the per-step kernels write it.
// Dead steps (EngineConfig.skip_pad_steps): a row past dlen writes the zeros attn_fwd_rowp writes
// and still serves its column slices while any row of its tile is live; a tile whose rows are all
// dead leaves the loop and only writes the zeros of its remaining steps.
// Registers: the three phases of a step have disjoint live sets.  Each phase re-derives what it needs
// from the thread index and from the kernel arguments, both made opaque per phase (phase_tid,
// phase_args), so nothing of one phase is hoisted out of the step loop and kept live (spilled)
// through the others: 0 bytes of scratch at the 128 VGPRs 16 waves allow.
// -DTSAMD_DEC_STAMPS (never in the shipped library; tools/dec_persistent_stamps.py builds it):
// wave 0 of every workgroup records the 100 MHz clock at eight points of every step.
#include "attn_rowp_fwd.h"
#include "handoff.h"
#include "launchers.h"

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
// s_sleep between the passes of a sweep (handoff.h): three hand-offs per step and 16 teams here
constexpr int kSleep = 24;
constexpr int kStamps = 8;  // clock stamps per workgroup and step (TSAMD_DEC_STAMPS)
// dynamic LDS carve (bytes, every offset a multiple of 16)
constexpr int oWc = 0;
constexpr int oWs = oWc + 64 * kWcS * 2;
constexpr int oCh = oWs + 32 * kWsS * 2;
constexpr int oGt = oCh + 16 * kChS * 2;
constexpr int oEs = oGt + 16 * kGtS * 2;
constexpr int oPart = oEs + kRowMaxT * 4;          // attention partials; the K-split sums of the GEMMs alias it
constexpr int oSrow = oPart + kNW * 4 * kEG * 4;
constexpr int oMisc = oSrow + kA * 4;
constexpr int oV = oMisc + 3 * kNW * 4;            // v, w_c . 2 log2(e), the row's coverage so far
constexpr int oWk = oV + kA * 4;
constexpr int oCov = oWk + kA * 4;
constexpr int kLds = oCov + kRowMaxT * 4;
static_assert(oWs % 16 == 0 && oCh % 16 == 0 && oGt % 16 == 0 && oEs % 16 == 0 && oPart % 16 == 0 && oSrow % 16 == 0 &&
              oMisc % 16 == 0 && oV % 16 == 0 && oWk % 16 == 0 && oCov % 16 == 0, "LDS carve alignment");
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
  unsigned* stamps;    // [grid][D][kStamps] (TSAMD_DEC_STAMPS builds; nullptr: none)
  int B, T, D;
};

namespace {

typedef const DecPersistentArgs __attribute__((address_space(4))) KArgs;  // see phase_args (handoff.h)

// Src of the attention body (attn_rowp_fwd.h): the LDS-resident copies.
struct ResidentSrc {
  const float* vl;
  const float* wk;  // w_c . 2 log2(e) (zeros without coverage)
  float* covl;
  bool has_cov;
  __device__ __forceinline__ float2 v2(int k) const { return *reinterpret_cast<const float2*>(vl + k); }
  __device__ __forceinline__ f32x2 w2(int k) const {
    const float2 w = *reinterpret_cast<const float2*>(wk + k);
    return f32x2{w.x, w.y};
  }
  __device__ __forceinline__ float cov_at(size_t, int p) const { return has_cov ? covl[p] : 0.f; }
  __device__ __forceinline__ void cov_set(int i, float c) const { covl[i] = c; }
};

template <typename OnG, typename Early, typename Mark>
struct StepHooks {
  OnG on_g;
  Early early_;
  Mark mark_;
  __device__ __forceinline__ int tid() const { return phase_tid(); }
  __device__ __forceinline__ void early() const { early_(); }
  __device__ __forceinline__ void mark(int i) const { mark_(i); }
};
template <typename OnG, typename Early, typename Mark>
__device__ __forceinline__ StepHooks<OnG, Early, Mark> step_hooks(OnG g, Early e, Mark m) {
  return StepHooks<OnG, Early, Mark>{g, e, m};
}

#ifdef TSAMD_DEC_STAMPS
#define DEC_STAMP(i) (st[i] = (unsigned)wall_clock64())
#else
#define DEC_STAMP(i) ((void)0)
#endif

}  // namespace

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
  float* vl = reinterpret_cast<float*>(smem + oV);
  float* wk = reinterpret_cast<float*>(smem + oWk);
  float* covl = reinterpret_cast<float*>(smem + oCov);

  const int B = p.B, T = p.T, D = p.D;
  int team, j;
  if (!team_of(kNC, B / 16, team, j)) return;
  const int r0 = team * 16, b = r0 + j;
  const bool has_cov = p.COV != nullptr;
  int tile_last = D, row_last = D;  // steps the tile / this workgroup's attention row are live for
  float cstate = 0.f;               // the cell's (row, unit) of this thread (waves 0-3), see the cell phase
  {
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    if (p.dlen) {
      tile_last = 0;
      for (int i = 0; i < 16; ++i) tile_last = max(tile_last, p.dlen[r0 + i]);
      tile_last = min(tile_last, D);
      row_last = p.dlen[b];
    }
    // weight slices, h_0 and the attention's resident operands into LDS
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
    if (tid < kA) {
      vl[tid] = p.v[tid];
      wk[tid] = (p.wc ? p.wc[tid] : 0.f) * K2LOG2E;
    }
    for (int i = tid; i < kRowMaxT; i += kNT) covl[i] = 0.f;  // (the coverage before step 0)
    const int crow = (lane >> 4) * 4 + (wid & 3), cu = 16 * j + (lane & 15);
    if (wid < 4) cstate = p.Cst[(size_t)(r0 + crow) * kH + cu];
  }
  bool dead = false;
  const ResidentSrc src{vl, wk, covl, has_cov};

  for (int t = 0; t < tile_last; ++t) {
    const unsigned tag = (unsigned)t + 1u;
    const int par = t & 1;
#ifdef TSAMD_DEC_STAMPS
    unsigned st[kStamps] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#endif
    // values of this step stored behind the attention's first loads (waves 0-3: c, h, gates; 0-7: s)
    float dc = 0.f, dh = 0.f, dgate[4] = {0.f, 0.f, 0.f, 0.f}, ds = 0.f;
    // ---- cell: z = XG_t + [g_{t-1}, h_{t-1}] . Wc^T
    {
      KArgs* a = phase_args<DecPersistentArgs>();
      const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
      const int l15 = lane & 15, kof = 8 * (lane >> 4);
      const int crow = (lane >> 4) * 4 + (wid & 3), cu = 16 * j + l15;  // (the accumulator register wid of the MFMA tile)
      gu64* gbuf = a->xbuf + (size_t)team * kTeamGranules;
      if (t > 0) {  // g_{t-1}: wave wid takes row wid (64 bf16 pairs)
        unsigned gv[1] = {0u};
        sweep<1, kSleep>(gbuf + (par ^ 1) * kGg, wid * 64, tag - 1u, gv, dead, a->err, kErrDecFwd, lane);
        *reinterpret_cast<unsigned*>(gt + wid * kGtS + 2 * lane) = gv[0];
      }
      DEC_STAMP(0);
      float xg[4] = {0.f, 0.f, 0.f, 0.f};  // (behind the sweep: in flight through the GEMM)
      if (wid < 4) {
        const float* xr = a->XG + ((size_t)t * B + r0 + crow) * (4 * kH);
#pragma unroll
        for (int g = 0; g < 4; ++g) xg[g] = xr[g * kH + cu];
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
          const bf16x8 av = k < kE ? ld8(grow + k) : ld8(hrow + k);
          acc = mfma16(av, ld8(wrow + k), acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((ks * 4 + gate) * 4 + r) * 64 + lane] = acc[r];
      }
      __syncthreads();
      gu64* chbuf = gbuf + 2 * kGg;
      if (wid < 4) {
        float z[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float s = 0.f;
#pragma unroll
          for (int sl = 0; sl < 4; ++sl) s += red[((sl * 4 + g) * 4 + wid) * 64 + lane];
          z[g] = s;
        }
        const float ig = fsigmoid(z[0] + xg[0]), jg = ftanh(z[1] + xg[1]);
        const float fg = fsigmoid(z[2] + xg[2] + 1.0f), og = fsigmoid(z[3] + xg[3]);
        const float c = fg * cstate + ig * jg;
        const float h = og * ftanh(c);
        cstate = c;
        store_granule(chbuf + par * kGch + crow * kH + cu, tag, pack_bf2(c, h));
        dc = c; dh = h;
        dgate[0] = ig; dgate[1] = jg; dgate[2] = fg; dgate[3] = og;
      }
      DEC_STAMP(1);
      // ---- [c_t, h_t] of the tile: wave wid takes row wid (256 {c, h} granules)
      unsigned cv[4] = {0u, 0u, 0u, 0u};
      sweep<4, kSleep>(chbuf + par * kGch, wid * kH, tag, cv, dead, a->err, kErrDecFwd, lane);
      unsigned short* crw = reinterpret_cast<unsigned short*>(ch + wid * kChS);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        crw[q * 64 + lane] = (unsigned short)(cv[q] & 0xffffu);
        crw[kH + q * 64 + lane] = (unsigned short)(cv[q] >> 16);
      }
      DEC_STAMP(2);
    }
    __syncthreads();
    // ---- s-projection: s = [c, h] . Ws^T + b, two 16-column tiles, linear2's four K slices
    {
      KArgs* a = phase_args<DecPersistentArgs>();
      const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
      const int l15 = lane & 15, kof = 8 * (lane >> 4);
      const int w = wid & 3, nt2 = (wid >> 2) & 1;
      const int row = (lane >> 4) * 4 + w, n = 32 * j + nt2 * 16 + l15;  // the output of this thread (waves 0-7)
      const float bsn = a->bs[n];
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
      gu64* sbuf = a->xbuf + (size_t)team * kTeamGranules + 2 * kGg + 2 * kGch;
      if (wid < 8) {
        float o = 0.f;
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) o += red[((sl * 2 + nt2) * 4 + w) * 64 + lane];
        const float sv = o + bsn + 0.f;
        store_granule(sbuf + par * kGs + row * kA + n, tag, __float_as_uint(sv));
        ds = sv;
      }
      DEC_STAMP(3);
    }
    // ---- attention of row j
    {
      KArgs* a = phase_args<DecPersistentArgs>();
      const bf16 *Fp = a->F, *Gp = a->G;
      const int* lens = a->lens;
      const int* dlen = a->dlen;
      float *ATT = a->ATT, *COV = a->COV, *covloss = a->covloss, *GV = a->GV;
      bf16 *ATTb = a->ATTb, *GVb = a->GVb;
      gu64* gbuf = a->xbuf + (size_t)team * kTeamGranules;
      {
        const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
        if (t < row_last && wid < 8) {
          unsigned sv[1] = {0u};
          sweep<1, kSleep>(gbuf + 2 * kGg + 2 * kGch + par * kGs + j * kA, wid * 64, tag, sv, dead, a->err, kErrDecFwd, lane);
          srow[wid * 64 + lane] = __uint_as_float(sv[0]);
        }
      }
      DEC_STAMP(4);
      __syncthreads();
      const size_t BT = (size_t)B * T;
      gu64* gdst = gbuf + par * kGg + j * (kE / 2);
      attn_fwd_rowp_core<1, kNW>(
          Fp, Gp, srow, src, lens, ATT + (size_t)t * BT, has_cov ? COV + (size_t)(t + 1) * BT : nullptr,
          has_cov ? covloss + (size_t)t * B : nullptr, GV + (size_t)t * B * kE, GVb + (size_t)t * B * kE, T, dlen, t,
          ATTb + (size_t)t * BT, b, es, part, wm, wl, redw,
          step_hooks(
              [&](int k, float g) {
                const float gn = __shfl_xor(g, 1, 64);  // (waves 0 and 1, all lanes)
                if (!(k & 1)) store_granule(gdst + (k >> 1), tag, pack_bf2(g, gn));
              },
              [&]() {  // the cell's and the s-projection's stores of this step
                KArgs* a2 = phase_args<DecPersistentArgs>();
                const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
                const int l15 = lane & 15, w = wid & 3, rw = (lane >> 4) * 4 + w;
                if (wid < 4) {
                  const int cu = 16 * j + l15;
                  const size_t o = ((size_t)(t + 1) * B + r0 + rw) * kH + cu;
                  a2->Cst[o] = dc;
                  a2->Cb[o] = f2bf(dc);
                  a2->Hb[o] = f2bf(dh);
                  float* a4 = a2->ACT + ((size_t)t * B + r0 + rw) * (4 * kH);
                  a4[cu] = dgate[0]; a4[kH + cu] = dgate[1]; a4[2 * kH + cu] = dgate[2]; a4[3 * kH + cu] = dgate[3];
                }
                if (wid < 8) {
                  const int n = 32 * j + ((wid >> 2) & 1) * 16 + l15;
                  a2->S[((size_t)t * B + r0 + rw) * kA + n] = ds;
                }
              },
              [&](int i) {
                (void)i;
#ifdef TSAMD_DEC_STAMPS
                st[5 + i] = (unsigned)wall_clock64();
#endif
              }));
    }
    DEC_STAMP(7);
#ifdef TSAMD_DEC_STAMPS
    if (p.stamps && threadIdx.x == 0) {
      unsigned* o = p.stamps + ((size_t)blockIdx.x * D + t) * kStamps;
#pragma unroll
      for (int i = 0; i < kStamps; ++i) o[i] = st[i];
    }
#endif
  }
  // ---- the tile's dead steps: the zeros dec_cell_fwd and attn_fwd_rowp write (coverage carried)
  __syncthreads();  // (the resident coverage written in the last live step by other threads)
  for (int t = tile_last; t < D; ++t) {
    KArgs* a = phase_args<DecPersistentArgs>();
    const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
    if (wid < 4) {
      const int crow = (lane >> 4) * 4 + (wid & 3), cu = 16 * j + (lane & 15);
      const size_t o = ((size_t)(t + 1) * B + r0 + crow) * kH + cu;
      a->Cst[o] = 0.f;
      a->Cb[o] = f2bf(0.f);
      a->Hb[o] = f2bf(0.f);
      float* a4 = a->ACT + ((size_t)t * B + r0 + crow) * (4 * kH);
      a4[cu] = 0.f; a4[kH + cu] = 0.f; a4[2 * kH + cu] = 0.f; a4[3 * kH + cu] = 0.f;
    }
    const size_t BT = (size_t)B * T;
    attn_fwd_rowp_dead<kNW>(src, a->ATT + (size_t)t * BT, has_cov ? a->COV + (size_t)(t + 1) * BT : nullptr,
                            has_cov ? a->covloss + (size_t)t * B : nullptr, a->GV + (size_t)t * B * kE,
                            a->GVb + (size_t)t * B * kE, T, a->ATTb + (size_t)t * BT, b,
                            step_hooks([](int, float) {}, []() {}, [](int) {}));
  }
}

// ------------------------------------------------------------------------------ host side
bool dec_persistent_shape_ok(int H, int E, int A, int B, int T) {
  return H == kH && E == kE && A == kA && B >= 16 && B % 16 == 0 && T >= 1 && T <= kRowMaxT;
}

// workgroups of a launch: one team of 16 per 16-row tile
int dec_persistent_grid(int B) { return B >= 16 && B % 16 == 0 ? team_grid(kNC, B / 16) : 0; }

size_t dec_persistent_xbuf_elems(int B) { return (size_t)(B / 16) * kTeamGranules; }

// Clock stamps (-DTSAMD_DEC_STAMPS builds only): later launches write [grid][D][8] 100 MHz clock
// values into buf (nullptr: stop).  Returns the stamps per workgroup and step, 0 when the library
// was built without them.
namespace {
unsigned* g_stamps = nullptr;
}
int dec_persistent_stamps_into(unsigned* buf) {
#ifdef TSAMD_DEC_STAMPS
  g_stamps = buf;
  return kStamps;
#else
  (void)buf;
  return 0;
#endif
}

// resident workgroups on the current device (handoff.h; the engine's invariant: dec_persistent_eligible)
int dec_persistent_capacity() {
  static int cache[kMaxDevices] = {};
  return resident_capacity(cache, {{reinterpret_cast<const void*>(dec_fwd_persistent_kernel), kNT, kLds}});
}

void launch_dec_fwd_persistent(const float* XG, const bf16* KcT, const bf16* WsT, const float* bs, float* Cst, bf16* Cb,
                               bf16* Hb, float* ACT, float* S, const bf16* F, const bf16* G, const float* v,
                               const float* wc, float* COV, const int* lens, float* ATT, bf16* ATTb, float* covloss,
                               float* GV, bf16* GVb, const int* dlen, unsigned long long* xbuf, unsigned* err, int B,
                               int T, int D, hipStream_t st) {
  const int grid = dec_persistent_grid(B);
  if (grid <= 0 || grid > dec_persistent_capacity()) return;  // the binding checks both first
  DecPersistentArgs p{XG, KcT, WsT, bs, Cst, Cb, Hb, ACT, S, F, G, v, wc, COV, lens, ATT, ATTb, covloss, GV, GVb, dlen,
                      (gu64*)xbuf, (gu32*)err, g_stamps, B, T, D};
  hipLaunchKernelGGL(dec_fwd_persistent_kernel, dim3(grid), dim3(kNT), kLds, st, p);
}
