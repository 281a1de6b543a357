// Forward body of the projected-context row attention (attention_row.hip, attn_fwd_rowp): one
// workgroup of NW waves computes one batch row of one decoder step.  Shared by the per-step kernel
// and the persistent decoder loop (decoder_persistent.hip), which runs it once per step on the
// query features it received from its team -- same arithmetic, same summation order.
// attn_fwd_rowp_core is the body; where the row's loop-invariant operands (v, w_c) and its coverage
// come from is a policy (Src): global memory for the per-step kernel (GlobalSrc), LDS-resident
// copies for the persistent loop.  Hooks are the persistent loop's points of interest inside a step.
#pragma once
#include "attn_common.h"

namespace attn_rowp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kRowMaxT = 2048;
constexpr int kEG = 128;

template <int NK>
struct Rows {
  u32x4 x[NK][4];  // 4 positions x NK 16-byte feature chunks of one tensor
};

template <int NK>
__device__ __forceinline__ void load_rows(Rows<NK>& r, const bf16* base, int p0, int len, int lane) {
  constexpr int A = 512 * NK;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = min(p0 + q, len - 1);
#pragma unroll
    for (int kb = 0; kb < NK; ++kb)
      r.x[kb][q] = __builtin_bit_cast(u32x4, ld8(base + (size_t)p * A + kb * 512 + lane * 8));
  }
}

// Src of the per-step kernel: v and w_c from global memory (w_c scaled here), the coverage so far
// from the previous step's global buffer (nullptr: zero).
struct GlobalSrc {
  const float* __restrict__ v;
  const float* __restrict__ wc;
  const float* cov;
  __device__ __forceinline__ float2 v2(int k) const { return *reinterpret_cast<const float2*>(v + k); }
  __device__ __forceinline__ f32x2 w2(int k) const {  // w_c . 2 log2(e)
    const float2 wv = wc ? *reinterpret_cast<const float2*>(wc + k) : make_float2(0.f, 0.f);
    return f32x2{wv.x, wv.y} * K2LOG2E;
  }
  __device__ __forceinline__ float cov_at(size_t rb, int p) const { return cov ? cov[rb + p] : 0.f; }
  __device__ __forceinline__ void cov_set(int, float) const {}
};

// Hooks of the per-step kernel: only on_g.
template <typename OnG>
struct OnGHooks {
  OnG on_g;
  __device__ __forceinline__ int tid() const { return threadIdx.x; }
  __device__ __forceinline__ void early() const {}   // every thread: the row's first loads are in flight
                                                     // (a dead row: on entry)
  __device__ __forceinline__ void mark(int) const {}  // 0: position loop done, 1: g published
};

// A step past the row's last loss-weighted decoder step: nothing it computes reaches the loss, so
// write zeros (a, g, coverage loss) and carry the coverage.
template <int NW, typename Src, typename Hooks>
__device__ __forceinline__ void attn_fwd_rowp_dead(const Src src, float* __restrict__ a_out, float* cov_out,
                                                   float* __restrict__ covloss, float* __restrict__ gx,
                                                   bf16* __restrict__ gx_bf, int T, bf16* __restrict__ a_bf, int b,
                                                   Hooks hk) {
  constexpr int NT = NW * 64;
  const int tid = hk.tid();
  const size_t rb = (size_t)b * T;
  for (int k = tid; k < kEG; k += NT) {
    gx[(size_t)b * kEG + k] = 0.f;
    gx_bf[(size_t)b * kEG + k] = f2bf(0.f);
    hk.on_g(k, 0.f);
  }
  hk.mark(1);
  for (int i = tid; i < T; i += NT) {
    a_out[rb + i] = 0.f;
    if (a_bf) a_bf[rb + i] = f2bf(0.f);
    if (cov_out) cov_out[rb + i] = src.cov_at(rb, i);
  }
  if (covloss && tid == 0) covloss[b] = 0.f;
}

// srow: the row's A query features s (global or LDS); b: the batch row; es / part / wm / wl / red:
// LDS scratch of kRowMaxT, NW * 4 * kEG, NW, NW, NW floats.  hk.on_g(k, g_k) is called by thread k
// (k < kEG: the first two waves, all lanes) with feature k of g right after it is stored.
template <int NK, int NW, typename Src, typename Hooks>
__device__ __forceinline__ void attn_fwd_rowp_core(
    const bf16* __restrict__ F, const bf16* __restrict__ G, const float* srow, const Src src,
    const int* __restrict__ lens, float* __restrict__ a_out, float* cov_out, float* __restrict__ covloss,
    float* __restrict__ gx, bf16* __restrict__ gx_bf, int T, const int* __restrict__ dlen, int step,
    bf16* __restrict__ a_bf, int b, float* es, float (*part)[4][kEG], float* wm, float* wl, float* red, Hooks hk) {
  const Dot2Sel dsel = dot2_sel();  // F pair selectors for fadd_bf2
  constexpr int A = 512 * NK, NT = NW * 64;
  const int tid = hk.tid(), wid = tid >> 6, lane = tid & 63;
  const int len = (int)DCHECK_IDX(lens[b], 1, T + 1, CHK_ATTN_LEN);
  const size_t rb = (size_t)b * T;
  if (dlen && step >= dlen[b]) {  // (block-uniform exit)
    hk.early();
    attn_fwd_rowp_dead<NW>(src, a_out, cov_out, covloss, gx, gx_bf, T, a_bf, b, hk);
    return;
  }
  const bf16* Fb = F + (size_t)b * T * A;
  const bf16* Gb = G + (size_t)b * T * kEG + (lane & 15) * 8;
  const int ngrp = (len + 3) >> 2;
  const int qm = lane >> 4;
  const int b5 = (lane >> 5) & 1, b4 = (lane >> 4) & 1;
  Rows<NK> fA, fB;
  u32x4 gA, gB;
  float cA = 0.f, cB = 0.f;
  auto load = [&](int grp, Rows<NK>& f, u32x4& gq, float& c) {
    load_rows<NK>(f, Fb, 4 * grp, len, lane);
    const int p = min(4 * grp + qm, len - 1);
    gq = __builtin_bit_cast(u32x4, ld8(Gb + (size_t)p * kEG));
    c = src.cov_at(rb, p);
  };
  if (wid < ngrp) load(wid, fA, gA, cA);
  hk.early();
  f32x2 s2[NK][4], w2[NK][4], v2[NK][4], acc[4];
  float vsum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NK; ++kb) {
    const int k0 = kb * 512 + lane * 8;
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
      const float2 sv = *reinterpret_cast<const float2*>(srow + k0 + 2 * jp);
      const float2 vv = src.v2(k0 + 2 * jp);
      s2[kb][jp] = f32x2{sv.x, sv.y} * K2LOG2E;
      w2[kb][jp] = src.w2(k0 + 2 * jp);
      v2[kb][jp] = f32x2{vv.x, vv.y};
      vsum += vv.x + vv.y;
    }
  }
#pragma unroll
  for (int jp = 0; jp < 4; ++jp) acc[jp] = f32x2{0.f, 0.f};
  // online softmax: m_w is wave-uniform, l_l is the lane's own position's share of the wave sum
  float m_w = -INFINITY, l_l = 0.f;
  auto compute = [&](int grp, const Rows<NK>& f, const u32x4& gq, float c_l) {
    float pd[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float c = rdlane(c_l, 16 * q);
      f32x2 d2 = f32x2{0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < NK; ++kb)
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const f32x2 y = fadd_bf2(f.x[kb][q][jp], fma2(w2[kb][jp], splat2(c), s2[kb][jp]), dsel);
          d2 = fma2(v2[kb][jp], rsig2(y), d2);
        }
      pd[q] = vsum - 2.0f * (d2.x + d2.y);
    }
    float eq = bfly4(pd, b5, b4);
    const int p = 4 * grp + qm;
    if (p >= len) eq = -INFINITY;
    if ((lane & 15) == 0 && p < len) es[p] = eq;
    const float e0 = rdlane(eq, 0), e1 = rdlane(eq, 16), e2 = rdlane(eq, 32), e3 = rdlane(eq, 48);
    const float mn = fmaxf(m_w, fmaxf(fmaxf(e0, e1), fmaxf(e2, e3)));  // e0 is always valid (p0 < len)
    const float sc = m_w == -INFINITY ? 0.f : fexp(m_w - mn);
    const float pq = fexp(eq - mn);
    l_l = fmaf(l_l, sc, pq);
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) acc[jp] = fma2(bf2pair(gq[jp]), splat2(pq), acc[jp] * sc);
    m_w = mn;
  };
  for (int g = wid; g < ngrp;) {
    const int g1 = g + NW;
    if (g1 < ngrp) load(g1, fB, gB, cB);
    compute(g, fA, gA, cA);
    if (g1 >= ngrp) break;
    const int g2 = g1 + NW;
    if (g2 < ngrp) load(g2, fA, gA, cA);
    compute(g1, fB, gB, cB);
    g = g2;
  }
  hk.mark(0);
  // merge: the 4 position quads of a wave hold the same features, then the waves
  const float lw = (rdlane(l_l, 0) + rdlane(l_l, 16)) + (rdlane(l_l, 32) + rdlane(l_l, 48));
  if (lane == 0) {
    wm[wid] = m_w;
    wl[wid] = lw;
  }
#pragma unroll
  for (int jp = 0; jp < 4; ++jp)
    *reinterpret_cast<float2*>(&part[wid][qm][(lane & 15) * 8 + 2 * jp]) = make_float2(acc[jp].x, acc[jp].y);
  __syncthreads();
  float m = -INFINITY;
#pragma unroll
  for (int w = 0; w < NW; ++w) m = fmaxf(m, wm[w]);
  // The sums over the waves are written as explicit FMAs: left to -ffp-contract, the compiler fused all
  // 16 terms of g in one translation unit and vectorised ten of them as packed multiply + add in the
  // other, and the persistent loop's g differed from the per-step kernel's by one ulp.
  float L = 0.f, wsc[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    wsc[w] = wm[w] == -INFINITY ? 0.f : fexp(wm[w] - m);
    L = __builtin_fmaf(wl[w], wsc[w], L);
  }
  const float invL = 1.0f / L;
  for (int k = tid; k < kEG; k += NT) {
    float c = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w)  // (explicit FMAs, see L above)
      c = __builtin_fmaf((part[w][0][k] + part[w][1][k]) + (part[w][2][k] + part[w][3][k]), wsc[w], c);
    c *= invL;
    gx[(size_t)b * kEG + k] = c;
    gx_bf[(size_t)b * kEG + k] = f2bf(c);
    hk.on_g(k, c);
  }
  hk.mark(1);
  float cl = 0.f;
  for (int i = tid; i < T; i += NT) {
    const float a = i < len ? fexp(es[i] - m) * invL : 0.f;
    a_out[rb + i] = a;
    if (a_bf) a_bf[rb + i] = f2bf(a);  // the bf16 operand of the post-loop ctx GEMM (no cast pass)
    if (cov_out) {
      const float c = src.cov_at(rb, i);
      cov_out[rb + i] = c + a;
      src.cov_set(i, c + a);
      cl += fminf(a, c);
    }
  }
  if (covloss) {
    cl = block_sum<NT>(cl, red);
    if (tid == 0) covloss[b] = cl;
  }
}

// The per-step kernel's entry: everything from global memory, on_g the only hook.
template <int NK, int NW, typename OnG>
__device__ __forceinline__ void attn_fwd_rowp_body(
    const bf16* __restrict__ F, const bf16* __restrict__ G, const float* srow, const float* __restrict__ v,
    const float* __restrict__ wc, const float* cov, const int* __restrict__ lens, float* __restrict__ a_out,
    float* cov_out, float* __restrict__ covloss, float* __restrict__ gx, bf16* __restrict__ gx_bf, int T,
    const int* __restrict__ dlen, int step, bf16* __restrict__ a_bf, int b, float* es, float (*part)[4][kEG],
    float* wm, float* wl, float* red, OnG on_g) {
  attn_fwd_rowp_core<NK, NW>(F, G, srow, GlobalSrc{v, wc, cov}, lens, a_out, cov_out,
                             covloss, gx, gx_bf, T, dlen, step, a_bf, b, es, part, wm, wl, red, OnGHooks<OnG>{on_g});
}

}  // namespace attn_rowp
