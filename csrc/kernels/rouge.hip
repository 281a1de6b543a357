// ROUGE rewards on the device for self-critical fine-tuning (train/scst.py holds the rule:
// rouge_ids / rouge_f; this kernel follows it count for count).
//
//   rouge_reward   one wave per hypothesis row r (article a = r / rows) over the sampler's step-major
//                  token history tok_hist [D][R] / slen [R] and the references ref [Na][Lr] / ref_len [Na].
//                  Both sequences are cut before their first [STOP] and copied to LDS (<= 256 ids each).
//                  LCS: lane j of a 64-token reference word holds ref[j], so the ballot of
//                  (ref_j == h_i) is the match mask M of hypothesis token h_i; the bit-vector recurrence
//                  U = V & M; V = (V + U) | (V & ~M) runs over up to four 64-bit words with the carry of
//                  the sum passed from word to word, once per hypothesis token (wave-uniform values);
//                  the LCS length is the number of zero bits among the first n_ref.
//                  Clipped n-gram hits: lane i owns hypothesis n-gram i, counts the equal hypothesis
//                  n-grams before it and the equal reference n-grams; it is a hit when the first count
//                  is below the second (each distinct n-gram then has min(count_hyp, count_ref) hits);
//                  ballot + popcount sums them.
//                  counts [R][5] = hit1, hit2, lcs, n_hyp, n_ref; reward [R] = the F value(s) chosen by
//                  kind (0 rouge_l, 1 rouge_1, 2 rouge_2, 3 their mean), in fp32 in rouge_f's order.
//
// No atomics, no cross-workgroup traffic: a row's result does not depend on where the row sits.
#include "common.h"
#include "launchers.h"

#define RG_WORDS (ROUGE_MAX_LEN / 64)

// f = 2 p r / (p + r) with p = hit / n_hyp, r = hit / n_ref; exactly 0 without a hit (an empty side
// has none)
__device__ __forceinline__ float rouge_f_dev(int hit, int n_hyp, int n_ref) {
  if (hit <= 0) return 0.f;
  const float p = (float)hit / (float)n_hyp, r = (float)hit / (float)n_ref;
  return 2.f * p * r / (p + r);
}

__global__ __launch_bounds__(64) void rouge_reward_kernel(
    const int* __restrict__ tok_hist, const int* __restrict__ slen,  // [D][R], [R]
    const int* __restrict__ ref, const int* __restrict__ ref_len,    // [R / rows][Lr], [R / rows]
    int* __restrict__ counts, float* __restrict__ reward,            // [R][5], [R]
    int R, int D, int Lr, int rows, int stop_id, int kind) {
  __shared__ int sh[ROUGE_MAX_LEN];
  __shared__ int sr[ROUGE_MAX_LEN];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int a = r / rows;
  const int dmax = min(D, ROUGE_MAX_LEN), lmax = min(Lr, ROUGE_MAX_LEN);
  int nh = (int)DCHECK_IDX(slen[r], 0, dmax + 1, CHK_ROUGE_HYP_LEN);
  nh = min(max(nh, 0), dmax);
  int nr = (int)DCHECK_IDX(ref_len[a], 0, lmax + 1, CHK_ROUGE_REF_LEN);
  nr = min(max(nr, 0), lmax);
  // ---- both sequences into LDS, cut before their first [STOP] (words from the last down: the
  // lowest word that holds one decides)
  int cut_h = nh, cut_r = nr;
#pragma unroll
  for (int w = RG_WORDS - 1; w >= 0; --w) {
    const int i = w * 64 + lane;
    const int th = i < nh ? tok_hist[(size_t)i * R + r] : stop_id;
    const int tr = i < nr ? ref[(size_t)a * Lr + i] : stop_id;
    sh[i] = th;
    sr[i] = tr;
    const unsigned long long mh = __ballot(i < nh && th == stop_id);
    const unsigned long long mr = __ballot(i < nr && tr == stop_id);
    if (mh) cut_h = w * 64 + __ffsll((long long)mh) - 1;
    if (mr) cut_r = w * 64 + __ffsll((long long)mr) - 1;
  }
  nh = cut_h;
  nr = cut_r;
  __syncthreads();
  // ---- LCS length: the bit-vector recurrence over the reference words, one hypothesis token a turn
  const int nw = (nr + 63) >> 6;
  int rj[RG_WORDS];
  bool vj[RG_WORDS];
#pragma unroll
  for (int w = 0; w < RG_WORDS; ++w) {
    const int j = w * 64 + lane;
    vj[w] = j < nr;
    rj[w] = sr[j];
  }
  unsigned long long Vw[RG_WORDS];
#pragma unroll
  for (int w = 0; w < RG_WORDS; ++w) Vw[w] = ~0ull;
  for (int i = 0; i < nh; ++i) {
    const int hi = sh[i];
    unsigned long long carry = 0ull;
#pragma unroll
    for (int w = 0; w < RG_WORDS; ++w) {
      if (w < nw) {  // (wave-uniform)
        const unsigned long long M = __ballot(vj[w] && rj[w] == hi);
        const unsigned long long V = Vw[w], U = V & M;
        const unsigned long long s1 = V + U, s2 = s1 + carry;
        carry = (unsigned long long)((s1 < V) | (s2 < s1));
        Vw[w] = s2 | (V & ~M);
      }
    }
  }
  int lcs = 0;
#pragma unroll
  for (int w = 0; w < RG_WORDS; ++w) {
    if (w < nw) {
      const int bits = min(64, nr - w * 64);
      const unsigned long long mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1ull);
      lcs += __popcll(~Vw[w] & mask);
    }
  }
  // ---- clipped unigram / bigram hits: lane i owns hypothesis n-gram i
  int hit1 = 0, hit2 = 0;
  for (int w = 0; w * 64 < nh; ++w) {
    const int i = w * 64 + lane;
    const int jend = min(w * 64 + 64, nh);  // (hypothesis n-grams before i are all below it)
    bool h1 = false, h2 = false;
    if (i < nh) {
      const int x = sh[i];
      int c1 = 0, c2 = 0;
      for (int j = 0; j < jend; ++j) c1 += (j < i) & (sh[j] == x);
      for (int j = 0; j < nr; ++j) c2 += sr[j] == x;
      h1 = c1 < c2;
      if (i + 1 < nh) {
        const int y = sh[i + 1];
        c1 = 0;
        c2 = 0;
        for (int j = 0; j + 1 < jend; ++j) c1 += (j < i) & (sh[j] == x) & (sh[j + 1] == y);  // (i <= jend - 1)
        for (int j = 0; j + 1 < nr; ++j) c2 += (sr[j] == x) & (sr[j + 1] == y);
        h2 = c1 < c2;
      }
    }
    hit1 += __popcll(__ballot(h1));
    hit2 += __popcll(__ballot(h2));
  }
  if (lane == 0) {
    int* c = counts + (size_t)r * 5;
    c[0] = hit1;
    c[1] = hit2;
    c[2] = lcs;
    c[3] = nh;
    c[4] = nr;
    const float f1 = rouge_f_dev(hit1, nh, nr);
    const float f2 = rouge_f_dev(hit2, max(nh - 1, 0), max(nr - 1, 0));
    const float fl = rouge_f_dev(lcs, nh, nr);
    reward[r] = kind == 0 ? fl : kind == 1 ? f1 : kind == 2 ? f2 : (f1 + f2 + fl) / 3.f;
  }
}

void launch_rouge_reward(const int* tok_hist, const int* slen, const int* ref, const int* ref_len, int* counts,
                         float* reward, int R, int D, int Lr, int rows, int stop_id, int kind, hipStream_t st) {
  hipLaunchKernelGGL(rouge_reward_kernel, dim3(R), dim3(64), 0, st, tok_hist, slen, ref, ref_len, counts, reward, R,
                     D, Lr, rows, stop_id, kind);
}
