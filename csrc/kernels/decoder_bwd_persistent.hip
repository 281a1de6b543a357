// Persistent decoder backward loop (projected attention, hidden 256, emb 128, A = 512): ONE launch
// runs all D steps of the reverse chain
//   attention backward (attn_bwd_rowp) -> s-projection + cell backward (dec_bwd_cell) ->
//   [dx | dh] = dz . W_cell^T (dec_bwd_dz)
// instead of three dependent launches per step and row group.  The team scheme is the forward's
// (decoder_persistent.hip, handoff.h): a TEAM = 16 workgroups on one XCD owns one 16-row tile, and
// no data of a step crosses a tile.  Member j of a team owns
//   * batch row j of the tile in the attention backward (16 waves, as attn_bwd_rowp_kernel<1, 16>);
//   * hidden units [16j, 16j + 16) of the cell backward, all four gates;
//   * column tile j of dh = dz . W_cell[E:]^T and, for j < 8, column tile j of dx = dz . W_cell[:E]^T.
// dh_rec and dc_carry of a member's (row, unit) pairs never leave the member (LDS).  Its weight slices
// (2 x 16 rows of W_s, its 16 or 32 rows of W_cell over K = 4H) live in LDS for the whole launch,
// and so does the dcov of its row (consumed only by the next step of the same row, updated in place).
// Three hand-offs per step stay inside the team (tagged 8-byte granules, two slots by step
// parity, zeroed before every launch): ds_t (16 x 512 as bf16 pairs: dec_bwd_cell converts ds with
// f2bf anyway), dz_t (16 x 4H as bf16 pairs) and dx_t (16 x 128 fp32, row i read by member i alone).
// Every wait is bounded (sweep): a timeout records kErrDecBwd in *err and the grid drains.
// Order of step t (t from D - 1 down) in one workgroup (P = publish, W = sweep, st = plain stores):
//   W dx_{t+1} (own row) | first F / G loads | st DS DZ DX of step t + 1 | position loop (st DE_t) |
//   P ds_t | W ds_t | s-projection + cell backward | P dz_t | W dz_t | dh tile, dx tile | P dx_t
// gfx9 counts loads and stores in one in-order vmcnt, so a store in front of a sweep makes the sweep
// wait for that store's write acknowledgement.  The values of DS_t, DZ_t and DX_t are therefore
// held in registers (1 + 2 + 1) and stored behind the next step's first attention loads, where the
// position loop follows; nothing but the publish itself sits between a publish and the next
// sweep.  (DE_t is stored from inside the position loop, group by group, as the per-step kernel
// does: there is no LDS left to hold a row of de, and only the last group's store is young when ds_t
// is published.  The DE zeros of a row's dead steps in a live tile are written before the step loop.)
// Double-buffering: a slot of step t is rewritten at step t - 2.  Only the order of publishes and
// sweeps matters for it, and that order is the one above for every member of a live tile:
//   * ds: a member publishes ds_{t-2} after its whole step t - 1, hence after its sweep of
//     dz_{t-1}, which needs every member's dz_{t-1}, each published after that member's sweep of
//     ds_{t-1}, which follows its sweep of ds_t;
//   * dz: a member publishes dz_{t-2} after its sweep of ds_{t-2}, which needs every member's
//     ds_{t-2}, each published after that member's step t - 1, hence after its sweep of dz_{t-1},
//     which follows its sweep of dz_t;
//   * dx: row i of the dx slot is read by member i alone, at the start of step t - 1; the owners
//     rewrite it at step t - 2 after sweeping dz_{t-2}, which contains member i's part, published
//     after its attention of step t - 2 and so after its sweep of dx_t (a member whose row is dead
//     never reads its dx).
// Arithmetic and summation order are the per-step kernels' (the K split in four slices summed in
// slice order, the 16-wave merge of ds in wave order, block_sum for S; the products whose fusion
// -ffp-contract=fast may choose either way are written as the per-step kernels' assembly has
// them), so DE, DS, DZ, DX and the final dh_rec / dc_carry are bit-identical to the chains'.
// Dead steps (EngineConfig.skip_pad_steps): the loop runs downwards, so a tile starts dead and
// becomes live.  A tile whose rows are all dead writes what tile_dead makes the per-step kernels
// write (dz = 0, dx = 0, dh_rec = 0, and the zeros of attn_bwd_rowp) and waits for nobody; a dead row
// of a live tile publishes ds = 0 and still serves its column slices.
// Registers: the phases of a step re-derive what they need from the thread index and the kernel
// arguments, both made opaque per phase, as in the forward; the attention's per-feature parameters
// are re-read from LDS in every position group through a lane offset made opaque per group
// (profiles/attn_bwd_body.md).  tests/test_dec_bwd_persistent_resources.py holds the figures.
#include "attn_rowp_fwd.h"
#include "handoff.h"
#include "launchers.h"

using namespace attn_rowp;
using namespace handoff;

namespace {

constexpr int kH = 256, kE = 128, kA = 512, kNC = 16, kNW = 16, kNT = kNW * 64;
constexpr int kG4 = 4 * kH;                        // dz width
constexpr int kWsS = kA + 8, kWzS = kG4 + 8;       // LDS row strides (bf16), +16 bytes against bank conflicts
// granules of one team: ds [2][16][256 pairs], dz [2][16][2 gate pairs][256 units], dx [2][16][128]
constexpr int kGds = 16 * (kA / 2), kGdz = 16 * 2 * kH, kGdx = 16 * kE;
constexpr int oGds = 0, oGdz = 2 * kGds, oGdx = oGdz + 2 * kGdz;
constexpr int kTeamGranules = 2 * (kGds + kGdz + kGdx);
constexpr int kSleep = 24;
// dynamic LDS carve (bytes, every offset a multiple of 16)
constexpr int oWs = 0;                             // [32][kWsS]: W_s rows 16j.. (c part), H + 16j.. (h part)
constexpr int oWz = oWs + 32 * kWsS * 2;           // [32][kWzS]: W_cell rows E + 16j.. (dh tile), 16j.. (dx tile, j < 8)
constexpr int oPart = oWz + 32 * kWzS * 2;         // attention partials [16][512]; ds / dz of the tile alias it
constexpr int oPrm = oPart + kNW * kA * 4;
constexpr int oDxl = oPrm + 3 * 4 * 64 * 8;
constexpr int oRed16 = oDxl + 4 * 16 * 8;
constexpr int oKred = oRed16 + kNW * 4;            // K-split partials of the two GEMM phases
constexpr int oDcov = oKred + 4 * 2 * 256 * 4;     // dcov of the row [kRowMaxT], updated in place
constexpr int oState = oDcov + kRowMaxT * 4;       // dh_rec, dc_carry of the member's 16 rows x 16 units [2][256]
constexpr int kLds = oState + 2 * 256 * 4;
static_assert(oWz % 16 == 0 && oPart % 16 == 0 && oPrm % 16 == 0 && oDxl % 16 == 0 && oRed16 % 16 == 0 &&
              oKred % 16 == 0 && oDcov % 16 == 0 && oState % 16 == 0, "LDS carve alignment");
static_assert(kLds <= 160 * 1024, "LDS of one CU");
static_assert(16 * kWsS * 2 <= kNW * kA * 4, "ds of the tile fits the attention partial buffer");
static_assert(16 * kWzS * 2 <= oRed16 - oPart, "dz of the tile fits the attention's per-step LDS");

}  // namespace

struct DecBwdPersistentArgs {
  const bf16* G;        // [B][T][E]
  const bf16* F;        // [B][T][A]
  const float* S;       // [D][B][A]
  const float* v;       // [A]
  const float* wc;      // [A] (nullable)
  const float* COV;     // [D+1][B][T] (nullptr: no coverage); step t reads COV[t] for t > 0
  const float* ATT;     // [D][B][T]
  const float* GV;      // [D][B][E]
  const float* Ga;      // [D][B][T]
  const float* gcl;     // [D][B] (with COV)
  const int* lens;      // [B]
  float* DE;            // [D][B][T]
  float* DS;            // [D][B][A]
  const bf16* Ws;       // [2H][A]
  const float* dC_dir;  // [D][B][H] (nullable)
  const float* dH_dir;  // [D][B][H]
  float* dh_rec;        // [B][H], in: the loop's start values, out: after step 0
  float* dc_carry;      // [B][H]
  const float* ACT;     // [D][B][4H]
  const float* Cst;     // [D+1][B][H]
  bf16* DZ;             // [D][B][4H]
  const bf16* Kc;       // [E+H][4H]
  const float* dX_dir;  // [D][B][E] (nullable)
  float* DX;            // [D][B][E]
  const int* dlen;      // [B] (nullable)
  gu64* xbuf;           // [B/16][kTeamGranules], zeroed before the launch
  gu32* err;
  int B, T, D;
};

namespace {

typedef const DecBwdPersistentArgs __attribute__((address_space(4))) KArgs;  // see phase_args (handoff.h)

struct Scal {
  float a, r, c, dn;
};

}  // namespace

__global__ __launch_bounds__(kNT) void dec_bwd_persistent_kernel(DecBwdPersistentArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* Wsl = reinterpret_cast<bf16*>(smem + oWs);
  bf16* Wzl = reinterpret_cast<bf16*>(smem + oWz);
  float(*part)[kA] = reinterpret_cast<float(*)[kA]>(smem + oPart);
  bf16* dsl = reinterpret_cast<bf16*>(smem + oPart);
  bf16* dzl = reinterpret_cast<bf16*>(smem + oPart);
  f32x2* prm = reinterpret_cast<f32x2*>(smem + oPrm);
  f32x2* dxl = reinterpret_cast<f32x2*>(smem + oDxl);
  float* red16 = reinterpret_cast<float*>(smem + oRed16);
  float* red = reinterpret_cast<float*>(smem + oKred);
  float* dcl = reinterpret_cast<float*>(smem + oDcov);
  float* sdh = reinterpret_cast<float*>(smem + oState);  // dh_rec / dc_carry of thread tid < 256: its (row, unit)
  float* sdc = sdh + 256;

  const int B = p.B, T = p.T, D = p.D;
  int team, j;
  if (!team_of(kNC, B / 16, team, j)) return;
  const int r0 = team * 16, b = r0 + j;
  const bool has_cov = p.COV != nullptr;
  int tile_last = D, row_last = D;  // steps below these are live for the tile / this workgroup's attention row
  {
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    if (p.dlen) {
      tile_last = 0;
      for (int i = 0; i < 16; ++i) tile_last = max(tile_last, p.dlen[r0 + i]);
      tile_last = min(tile_last, D);
      row_last = p.dlen[b];
    }
    for (int i = tid; i < 32 * (kA / 8); i += kNT) {
      const int row = i / (kA / 8), c8 = i % (kA / 8);
      const int grow = (row >> 4) * kH + 16 * j + (row & 15);
      *reinterpret_cast<bf16x8*>(Wsl + row * kWsS + c8 * 8) = ld8(p.Ws + (size_t)grow * kA + c8 * 8);
    }
    const int nrows = j < 8 ? 32 : 16;
    for (int i = tid; i < nrows * (kG4 / 8); i += kNT) {
      const int row = i / (kG4 / 8), c8 = i % (kG4 / 8);
      const int grow = row < 16 ? kE + 16 * j + row : 16 * j + (row - 16);
      *reinterpret_cast<bf16x8*>(Wzl + row * kWzS + c8 * 8) = ld8(p.Kc + (size_t)grow * kG4 + c8 * 8);
    }
    for (int i = tid; i < kRowMaxT; i += kNT) dcl[i] = 0.f;  // (dcov_next of the first live step)
    if (wid < 4) {
      const size_t ri = (size_t)(r0 + (lane >> 4) * 4 + wid) * kH + 16 * j + (lane & 15);
      sdh[tid] = (tile_last < D) ? 0.f : p.dh_rec[ri];  // (a dead step of the tile leaves dh_rec = 0)
      sdc[tid] = p.dc_carry[ri];
    }
  }
  // ---- the tile's dead steps: the zeros of attn_bwd_rowp, dec_bwd_cell and dec_bwd_dz
  for (int t = D - 1; t >= tile_last; --t) {
    KArgs* a = phase_args<DecBwdPersistentArgs>();
    const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
    const int row = (lane >> 4) * 4 + (wid & 3), l15 = lane & 15;
    if (wid < 4) {
      bf16* dzr = a->DZ + ((size_t)t * B + r0 + row) * kG4 + 16 * j + l15;
      dzr[0] = f2bf(0.f); dzr[kH] = f2bf(0.f); dzr[2 * kH] = f2bf(0.f); dzr[3 * kH] = f2bf(0.f);
    } else if (wid < 8 && j < 8) {
      a->DX[((size_t)t * B + r0 + row) * kE + 16 * j + l15] = 0.f;
    }
    float* de = a->DE + ((size_t)t * B + b) * T;
    for (int i = tid; i < T; i += kNT) de[i] = 0.f;
    if (tid < kA) a->DS[((size_t)t * B + b) * kA + tid] = 0.f;
  }
  // the steps at which this row is dead in a live tile: its DE zeros are known now, and written here
  // they do not stand between a ds publish and the following sweep
  for (int t = min(tile_last, D) - 1; t >= max(row_last, 0); --t) {
    KArgs* a = phase_args<DecBwdPersistentArgs>();
    const int tid = phase_tid();
    float* de = a->DE + ((size_t)t * B + b) * T;
    for (int i = tid; i < T; i += kNT) de[i] = 0.f;
  }
  __syncthreads();
  bool dead = false;
  // values of the previous live step, stored behind this step's first attention loads
  int st_t = -1;
  float st_ds = 0.f, st_dx = 0.f;
  unsigned st_dz0 = 0u, st_dz1 = 0u;
  auto flush = [&]() {
    if (st_t < 0) return;
    KArgs* a = phase_args<DecBwdPersistentArgs>();
    const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
    const int row = (lane >> 4) * 4 + (wid & 3), l15 = lane & 15;
    if (tid < kA) a->DS[((size_t)st_t * B + b) * kA + tid] = st_ds;
    if (wid < 4) {
      unsigned short* dzr =
          reinterpret_cast<unsigned short*>(a->DZ) + ((size_t)st_t * B + r0 + row) * kG4 + 16 * j + l15;
      dzr[0] = (unsigned short)(st_dz0 & 0xffffu);
      dzr[kH] = (unsigned short)(st_dz0 >> 16);
      dzr[2 * kH] = (unsigned short)(st_dz1 & 0xffffu);
      dzr[3 * kH] = (unsigned short)(st_dz1 >> 16);
    } else if (wid < 8 && j < 8) {
      a->DX[((size_t)st_t * B + r0 + row) * kE + 16 * j + l15] = st_dx;
    }
  };

  for (int t = tile_last - 1; t >= 0; --t) {
    const unsigned tag = (unsigned)t + 1u;
    const int par = t & 1;
    float ds_val = 0.f;  // ds_t[b][tid], tid < 512
    // ---- attention backward of row j
    if (t < row_last) {
      KArgs* a = phase_args<DecBwdPersistentArgs>();
      const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
      gu64* tb = a->xbuf + (size_t)team * kTeamGranules;
      const bool has_dx = t < D - 1;
      float dxv = 0.f;  // dx_{t+1}[b][tid], tid < 128 (zeros where the tile was dead at t + 1)
      if (wid < 2) {
        if (has_dx && t + 1 < tile_last) {
          unsigned xv[1] = {0u};
          sweep<1, kSleep>(tb + oGdx + (par ^ 1) * kGdx + j * kE, wid * 64, tag + 1u, xv, dead, a->err, kErrDecBwd, lane);
          dxv = __uint_as_float(xv[0]);
        }
        // lane l of the position loop uses features (l & 15) * 8 .. + 8 as four pairs
        reinterpret_cast<float*>(dxl)[((((tid >> 1) & 3) * 16 + (tid >> 3)) << 1) + (tid & 1)] = dxv;
      }
      const Dot2Sel dsel = dot2_sel();
      const int len = (int)DCHECK_IDX(a->lens[b], 1, T + 1, CHK_ATTN_LEN);
      const size_t rb = ((size_t)t * B + b) * T;
      const float* att = a->ATT + rb;
      const float* Gar = a->Ga + rb;
      const float* covr = (has_cov && t > 0) ? a->COV + rb : nullptr;
      const float g = has_cov ? a->gcl[(size_t)t * B + b] : 0.f;
      // dcov of the row, in place: every read of position i (the S loop before the barriers, the
      // owning wave's load of its group) precedes that wave's write of i in the same step
      const float* dcn = dcl;
      float* dco = dcl;
      float* de_out = a->DE + rb;
      const bf16* Gb = a->G + (size_t)b * T * kEG + (lane & 15) * 8;
      const bf16* Fb = a->F + (size_t)b * T * kA;
      const int ngrp = (len + 3) >> 2;
      const int qm = lane >> 4;
      const int b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1;
      // (all zeroed: an undefined buffer would be carried, and spilled, around the step loop)
      Rows<1> fA{}, fB{};
      u32x4 gA = u32x4{0u, 0u, 0u, 0u}, gB = u32x4{0u, 0u, 0u, 0u};
      Scal xA{}, xB{};
      auto load = [&](int grp, Rows<1>& f, u32x4& gq, Scal& x) {
        load_rows<1>(f, Fb, 4 * grp, len, lane);
        const int pc = min(4 * grp + qm, len - 1);
        gq = __builtin_bit_cast(u32x4, ld8(Gb + (size_t)pc * kEG));
        x.a = att[pc];
        x.c = covr ? covr[pc] : 0.f;
        x.dn = has_cov ? dcn[pc] : 0.f;
        x.r = Gar[pc] + x.dn + ((has_cov && x.a <= x.c) ? g : 0.f);
      };
      if (wid < ngrp) load(wid, fA, gA, xA);
      flush();  // DS, DZ, DX of step t + 1
      f32x2 acc[4];
#pragma unroll
      for (int jp = 0; jp < 4; ++jp) {
        acc[jp] = f32x2{0.f, 0.f};
        if (wid != 0) continue;
        const int k0 = lane * 8;
        const float2 sv = *reinterpret_cast<const float2*>(a->S + ((size_t)t * B + b) * kA + k0 + 2 * jp);
        const float2 vv = *reinterpret_cast<const float2*>(a->v + k0 + 2 * jp);
        const float2 wv = a->wc ? *reinterpret_cast<const float2*>(a->wc + k0 + 2 * jp) : make_float2(0.f, 0.f);
        prm[(0 * 4 + jp) * 64 + lane] = f32x2{sv.x, sv.y} * K2LOG2E;
        prm[(1 * 4 + jp) * 64 + lane] = f32x2{wv.x, wv.y} * K2LOG2E;
        prm[(2 * 4 + jp) * 64 + lane] = f32x2{4.f * vv.x * wv.x, 4.f * vv.y * wv.y};
      }
      float S = 0.f;
      for (int i = tid; i < len; i += kNT) {
        const float ai = att[i];
        float r = Gar[i] + (has_cov ? dcn[i] : 0.f);
        if (has_cov && ai <= (covr ? covr[i] : 0.f)) r += g;
        S = __builtin_fmaf(ai, r, S);
      }
      if (has_dx && tid < kEG) S = __builtin_fmaf(dxv, a->GV[((size_t)t * B + b) * kEG + tid], S);
      {  // block_sum<kNT>
        S = wave_sum(S);
        __syncthreads();
        if (lane == 0) red16[wid] = S;
        __syncthreads();
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < kNW; ++i) r += red16[i];
        S = r;
      }
      auto compute = [&](int grp, const Rows<1>& f, const u32x4& gq, const Scal& x) {
        int pl = lane;  // LDS lane offset, opaque per group: the parameters are re-read, not kept in registers
        asm volatile("" : "+v"(pl));
        f32x2 d2 = f32x2{0.f, 0.f};
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) d2 = fma2(bf2pair(gq[jp]), dxl[jp * 16 + (pl & 15)], d2);
        const float dot = dpp_sum16(d2.x + d2.y);
        const int pp = 4 * grp + qm;
        const float de_q = pp < len ? x.a * (x.r + dot - S) : 0.f;
        float deq[4], cq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          deq[q] = rdlane(de_q, 16 * q);
          cq[q] = rdlane(x.c, 16 * q);
        }
        f32x2 dc2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dc2[q] = f32x2{0.f, 0.f};
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const f32x2 ps = prm[(0 * 4 + jp) * 64 + pl], pw = prm[(1 * 4 + jp) * 64 + pl], pv = prm[(2 * 4 + jp) * 64 + pl];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x2 y = fadd_bf2(f.x[0][q][jp], fma2(pw, splat2(cq[q]), ps), dsel);
            const f32x2 r = rsig2(y);
            const f32x2 qv = fma2(-r, r, r);
            acc[jp] = fma2(qv, splat2(deq[q]), acc[jp]);
            dc2[q] = fma2(qv, pv, dc2[q]);
          }
        }
        float dcv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dcv[q] = dc2[q].x + dc2[q].y;
        const float hc = bfly4(dcv, b5, b4);
        if ((lane & 15) == 0 && pp < T) {
          de_out[pp] = de_q;
          if (has_cov && pp < len) {  // (positions past len are never read back)
            float r = __builtin_fmaf(de_q, hc, x.dn);
            if (x.a > x.c) r += g;
            dco[pp] = r;
          }
        }
      };
      for (int gi = wid; gi < ngrp;) {
        const int g1 = gi + kNW;
        if (g1 < ngrp) load(g1, fB, gB, xB);
        compute(gi, fA, gA, xA);
        if (g1 >= ngrp) break;
        const int g2 = g1 + kNW;
        if (g2 < ngrp) load(g2, fA, gA, xA);
        compute(g1, fB, gB, xB);
        gi = g2;
      }
      for (int pp = 4 * ngrp + tid; pp < T; pp += kNT) de_out[pp] = 0.f;
#pragma unroll
      for (int jp = 0; jp < 4; ++jp)
        *reinterpret_cast<float2*>(&part[wid][lane * 8 + 2 * jp]) = make_float2(acc[jp].x, acc[jp].y);
      __syncthreads();
      if (tid < kA) {
        float x = 0.f;
#pragma unroll
        for (int w = 0; w < kNW; ++w) x += part[w][tid];
        ds_val = 4.f * a->v[tid] * x;
      }
    } else {  // dead row of a live tile: ds = 0 (its DE zeros were written before the loop, dcov stays zero)
      flush();
    }
    {  // P ds_t
      KArgs* a = phase_args<DecBwdPersistentArgs>();
      const int tid = phase_tid();
      if (tid < kA) {
        const float dn = __shfl_xor(ds_val, 1, 64);  // (waves 0-7, all lanes)
        if (!(tid & 1))
          store_granule(a->xbuf + (size_t)team * kTeamGranules + oGds + par * kGds + j * (kA / 2) + (tid >> 1), tag,
                        pack_bf2(ds_val, dn));
      }
    }
    __syncthreads();  // (the merge's reads of part, which the tile's ds overwrites)
    // ---- s-projection + cell backward of units [16j, 16j + 16)
    unsigned dz0 = 0u, dz1 = 0u;
    {
      KArgs* a = phase_args<DecBwdPersistentArgs>();
      const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
      const int l15 = lane & 15, kof = 8 * (lane >> 4);
      const int row = (lane >> 4) * 4 + (wid & 3), u = 16 * j + l15;  // this thread's (row, unit), waves 0-3
      gu64* tb = a->xbuf + (size_t)team * kTeamGranules;
      float dh0 = 0.f, dc0 = 0.f, dhr = 0.f, dcc = 0.f, a4[4] = {0.f, 0.f, 0.f, 0.f}, cn = 0.f, cpv = 0.f;
      if (wid < 4) {  // (in flight through the sweep)
        const size_t ri = ((size_t)t * B + r0 + row) * kH + u;
        dhr = sdh[tid];
        dcc = sdc[tid];
        dh0 = a->dH_dir[ri];
        dc0 = a->dC_dir ? a->dC_dir[ri] : 0.f;
        const float* ap = a->ACT + ((size_t)t * B + r0 + row) * kG4;
#pragma unroll
        for (int g = 0; g < 4; ++g) a4[g] = ap[g * kH + u];
        cn = a->Cst[ri + (size_t)B * kH];
        cpv = a->Cst[ri];
      }
      {  // W ds_t: wave wid takes row wid (256 bf16 pairs)
        unsigned dv[4] = {0u, 0u, 0u, 0u};
        sweep<4, kSleep>(tb + oGds + par * kGds, wid * (kA / 2), tag, dv, dead, a->err, kErrDecBwd, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<unsigned*>(dsl + wid * kWsS + 2 * (q * 64 + lane)) = dv[q];
      }
      __syncthreads();
      if (wid < 8) {  // wave (c / h part, K slice): the four K slices of dec_bwd_cell's four waves
        const int nb = wid >> 2, ks = wid & 3;
        const bf16* arow = dsl + l15 * kWsS + kof + (kA / 4) * ks;
        const bf16* wrow = Wsl + (nb * 16 + l15) * kWsS + kof + (kA / 4) * ks;
        f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kA / 4 / 32; ++i) acc = mfma16(ld8(arow + 32 * i), ld8(wrow + 32 * i), acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((ks * 2 + nb) * 4 + r) * 64 + lane] = acc[r];
      }
      __syncthreads();
      if (wid < 4) {
        float o[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          float s = 0.f;
#pragma unroll
          for (int sl = 0; sl < 4; ++sl) s += red[((sl * 2 + nb) * 4 + wid) * 64 + lane];
          o[nb] = s;
        }
        const float dh = (dhr + dh0) + o[1];
        float dc = (dcc + dc0) + o[0];
        const float ig = a4[0], jg = a4[1], fg = a4[2], og = a4[3];
        // ftanh(cn), and the products as dec_bwd_cell_kernel's assembly has them
        const float xc = fminf(fmaxf(cn, -15.0f), 15.0f);
        const float ex = __builtin_amdgcn_exp2f((xc + xc) * 1.4426950408889634f);
        const float tc = __builtin_fmaf(__builtin_amdgcn_rcpf(ex + 1.0f), -2.0f, 1.0f);
        const float dho = dh * og;
        dc = __builtin_fmaf(__builtin_fmaf(-tc, tc, 1.0f), dho, dc);
        const float t0 = dh * tc, t1 = t0 * og;
        const float dzo = t1 * (1.0f - og);
        const float t2 = dc * jg, t3 = t2 * ig;
        const float dzi = t3 * (1.0f - ig);
        const float t4 = dc * ig;
        const float dzj = t4 * __builtin_fmaf(-jg, jg, 1.0f);
        const float t5 = dc * cpv, t6 = t5 * fg;
        const float dzf = t6 * (1.0f - fg);
        sdc[tid] = dc * fg;
        dz0 = pack_bf2(dzi, dzj);
        dz1 = pack_bf2(dzf, dzo);
        gu64* zb = tb + oGdz + par * kGdz + row * (2 * kH) + u;
        store_granule(zb, tag, dz0);
        store_granule(zb + kH, tag, dz1);
      }
    }
    // ---- dh tile and (j < 8) dx tile of dz_t . W_cell^T
    float dxo = 0.f;
    {
      KArgs* a = phase_args<DecBwdPersistentArgs>();
      const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
      const int l15 = lane & 15, kof = 8 * (lane >> 4);
      const int w = wid & 3, row = (lane >> 4) * 4 + w;
      gu64* tb = a->xbuf + (size_t)team * kTeamGranules;
      const bool dxw = wid >= 4 && wid < 8 && j < 8;  // waves that own the dx tile's outputs
      float dxd = 0.f;
      if (dxw && a->dX_dir) dxd = a->dX_dir[((size_t)t * B + r0 + row) * kE + 16 * j + l15];
      {  // W dz_t: wave wid takes row wid (2 gate pairs x 256 units)
        unsigned zv[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        sweep<8, kSleep>(tb + oGdz + par * kGdz, wid * (2 * kH), tag, zv, dead, a->err, kErrDecBwd, lane);
        unsigned short* zr = reinterpret_cast<unsigned short*>(dzl + wid * kWzS);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int gp = q >> 2, ug = (q & 3) * 64 + lane;
          zr[(2 * gp) * kH + ug] = (unsigned short)(zv[q] & 0xffffu);
          zr[(2 * gp + 1) * kH + ug] = (unsigned short)(zv[q] >> 16);
        }
      }
      __syncthreads();
      if (wid < 4 || dxw) {  // wave (tile, K slice): the four K slices of dec_bwd_dz's four waves
        const int nb = wid >> 2;
        const bf16* arow = dzl + l15 * kWzS + kof + (kG4 / 4) * w;
        const bf16* wrow = Wzl + (nb * 16 + l15) * kWzS + kof + (kG4 / 4) * w;
        f32x4 acc = f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < kG4 / 4 / 32; ++i) acc = mfma16(ld8(arow + 32 * i), ld8(wrow + 32 * i), acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((w * 2 + nb) * 4 + r) * 64 + lane] = acc[r];
      }
      __syncthreads();
      if (wid < 4 || dxw) {
        const int nb = wid >> 2;
        float s = 0.f;
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) s += red[((sl * 2 + nb) * 4 + w) * 64 + lane];
        if (nb == 0) {
          sdh[tid] = s;
        } else {
          dxo = s + dxd;
          if (t > 0) store_granule(tb + oGdx + par * kGdx + row * kE + 16 * j + l15, tag, __float_as_uint(dxo));
        }
      }
    }
    st_t = t;
    st_ds = ds_val;
    st_dx = dxo;
    st_dz0 = dz0;
    st_dz1 = dz1;
  }
  flush();
  {
    KArgs* a = phase_args<DecBwdPersistentArgs>();
    const int tid = phase_tid(), wid = tid >> 6, lane = tid & 63;
    if (wid < 4) {
      const size_t ri = (size_t)(r0 + (lane >> 4) * 4 + wid) * kH + 16 * j + (lane & 15);
      a->dh_rec[ri] = sdh[tid];
      a->dc_carry[ri] = sdc[tid];
    }
  }
}

// ------------------------------------------------------------------------------ host side
// (shape rule and grid: dec_persistent_shape_ok / dec_persistent_grid of decoder_persistent.hip)
size_t dec_bwd_persistent_xbuf_elems(int B) { return (size_t)(B / 16) * kTeamGranules; }

// resident workgroups on the current device (handoff.h)
int dec_bwd_persistent_capacity() {
  static int cache[kMaxDevices] = {};
  return resident_capacity(cache, {{reinterpret_cast<const void*>(dec_bwd_persistent_kernel), kNT, kLds}});
}

void launch_dec_bwd_persistent(const bf16* G, const bf16* F, const float* S, const float* v, const float* wc,
                               const float* COV, const float* ATT, const float* GV, const float* Ga, const float* gcl,
                               const int* lens, float* DE, float* DS, const bf16* Ws, const float* dC_dir,
                               const float* dH_dir, float* dh_rec, float* dc_carry, const float* ACT, const float* Cst,
                               bf16* DZ, const bf16* Kc, const float* dX_dir, float* DX, const int* dlen,
                               unsigned long long* xbuf, unsigned* err, int B, int T, int D, hipStream_t st) {
  const int grid = dec_persistent_grid(B);
  if (grid <= 0 || grid > dec_bwd_persistent_capacity()) return;  // the binding checks both first
  DecBwdPersistentArgs p{G, F, S, v, wc, COV, ATT, GV, Ga, gcl, lens, DE, DS, Ws, dC_dir, dH_dir, dh_rec, dc_carry,
                         ACT, Cst, DZ, Kc, dX_dir, DX, dlen, (gu64*)xbuf, (gu32*)err, B, T, D};
  hipLaunchKernelGGL(dec_bwd_persistent_kernel, dim3(grid), dim3(kNT), kLds, st, p);
}
