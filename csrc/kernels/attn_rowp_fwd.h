// Forward body of the projected-context row attention (attention_row.hip, attn_fwd_rowp): one
// workgroup of NW waves computes one batch row of one decoder step.  Shared by the per-step kernel
// and the persistent decoder loop (decoder_persistent.hip), which runs it once per step on the
// query features it received from its team -- same arithmetic, same summation order.
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

// srow: the row's A query features s (global or LDS); b: the batch row; es / part / wm / wl / red:
// LDS scratch of kRowMaxT, NW * 4 * kEG, NW, NW, NW floats.  on_g(k, g_k) is called by thread k
// (k < kEG: the first two waves, all lanes) with feature k of g right after it is stored.
template <int NK, int NW, typename OnG>
__device__ __forceinline__ void attn_fwd_rowp_body(
    const bf16* __restrict__ F, const bf16* __restrict__ G, const float* srow, const float* __restrict__ v,
    const float* __restrict__ wc, const float* cov, const int* __restrict__ lens, float* __restrict__ a_out,
    float* cov_out, float* __restrict__ covloss, float* __restrict__ gx, bf16* __restrict__ gx_bf, int T,
    const int* __restrict__ dlen, int step, bf16* __restrict__ a_bf, int b, float* es, float (*part)[4][kEG],
    float* wm, float* wl, float* red, OnG on_g) {
  const Dot2Sel dsel = dot2_sel();  // F pair selectors for fadd_bf2
  constexpr int A = 512 * NK, NT = NW * 64;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int len = (int)DCHECK_IDX(lens[b], 1, T + 1, CHK_ATTN_LEN);
  const size_t rb = (size_t)b * T;
  if (dlen && step >= dlen[b]) {
    // a step past the row's last loss-weighted decoder step (block-uniform exit): nothing it
    // computes reaches the loss, so write zeros (a, g, coverage loss) and carry the coverage
    for (int i = tid; i < T; i += NT) {
      a_out[rb + i] = 0.f;
      if (a_bf) a_bf[rb + i] = f2bf(0.f);
      if (cov_out) cov_out[rb + i] = cov ? cov[rb + i] : 0.f;
    }
    for (int k = tid; k < kEG; k += NT) {
      gx[(size_t)b * kEG + k] = 0.f;
      gx_bf[(size_t)b * kEG + k] = f2bf(0.f);
      on_g(k, 0.f);
    }
    if (covloss && tid == 0) covloss[b] = 0.f;
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
    c = cov ? cov[rb + p] : 0.f;
  };
  if (wid < ngrp) load(wid, fA, gA, cA);
  f32x2 s2[NK][4], w2[NK][4], v2[NK][4], acc[4];
  float vsum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NK; ++kb) {
    const int k0 = kb * 512 + lane * 8;
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
      const float2 sv = *reinterpret_cast<const float2*>(srow + k0 + 2 * jp);
      const float2 vv = *reinterpret_cast<const float2*>(v + k0 + 2 * jp);
      const float2 wv = wc ? *reinterpret_cast<const float2*>(wc + k0 + 2 * jp) : make_float2(0.f, 0.f);
      s2[kb][jp] = f32x2{sv.x, sv.y} * K2LOG2E;
      w2[kb][jp] = f32x2{wv.x, wv.y} * K2LOG2E;
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
  float L = 0.f, wsc[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    wsc[w] = wm[w] == -INFINITY ? 0.f : fexp(wm[w] - m);
    L += wl[w] * wsc[w];
  }
  const float invL = 1.0f / L;
  for (int k = tid; k < kEG; k += NT) {
    float c = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) c += ((part[w][0][k] + part[w][1][k]) + (part[w][2][k] + part[w][3][k])) * wsc[w];
    c *= invL;
    gx[(size_t)b * kEG + k] = c;
    gx_bf[(size_t)b * kEG + k] = f2bf(c);
    on_g(k, c);
  }
  float cl = 0.f;
  for (int i = tid; i < T; i += NT) {
    const float a = i < len ? fexp(es[i] - m) * invL : 0.f;
    a_out[rb + i] = a;
    if (a_bf) a_bf[rb + i] = f2bf(a);  // the bf16 operand of the post-loop ctx GEMM (no cast pass)
    if (cov_out) {
      const float c = cov ? cov[rb + i] : 0.f;
      cov_out[rb + i] = c + a;
      cl += fminf(a, c);
    }
  }
  if (covloss) {
    cl = block_sum<NT>(cl, red);
    if (tid == 0) covloss[b] = cl;
  }
}

}  // namespace attn_rowp
