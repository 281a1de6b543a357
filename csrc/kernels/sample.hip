// Decode by sampling on the device (decode/sampling.py holds the rule; these kernels follow it).
//
//   sample_uniforms  probe: the device Philox4x32-10 uniform of every row's stream at the step the
//                    device counter holds (compared bit for bit with the host).
//   sample_topk      one wave per row over the step's candidate lists top_ids / top_lp [R][K]
//                    (K <= 32): the k + 1 best, [STOP] dropped before min_dec, the first k kept,
//                    weights exp((lp_j - lp_max) / temp), inverse CDF at u * sum.
//   sample_full      one workgroup per row over the fp32 logits [R][V]: ONE read of the row gives
//                    every 256-entry chunk's (max, sum of exponentials); the row max / sum, the
//                    chunk weights p_gen * softmax (vocabulary chunks) and (1 - p_gen) * a_i (article
//                    position chunks, after the vocabulary ones) and their scan follow in LDS; the
//                    chunk that holds the crossing is read once more and walked to the entry; the
//                    same workgroup then forms the chosen token's model log-prob (its softmax term
//                    plus the attention of every position that copies it).  The chunk order is
//                    fixed by (V, T): a row's result does not depend on where the row sits.  A row with
//                    nothing to draw from (all weights 0 or NaN) sets the optional error word.
//
// Both draw kernels end in the samples' bookkeeping (SampleBook): token / log-prob histories,
// log-prob sum, latest token, the per-row done flag and length, the attention / p_gen histories.
// Rows that are done, and steps past max_dec, are no-ops.  The step index t (and with it the
// Philox counter) is the device step counter minus one: beam_gather advanced it at the start of
// the decode step, so a captured graph replays with the right t.
#include "common.h"
#include "launchers.h"

// ------------------------------------------------------------------ Philox4x32-10
// key (seed lo, seed hi), counter (t, stream lo, stream hi, 0); the uniform is the top 24 bits of
// output word 0, exact in fp32, in [0, 1).
__device__ __forceinline__ unsigned philox_word0(unsigned long long seed, unsigned long long stream, unsigned t) {
  unsigned c0 = t, c1 = (unsigned)stream, c2 = (unsigned)(stream >> 32), c3 = 0u;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}
__device__ __forceinline__ float sample_u(unsigned long long seed, unsigned long long stream, int t) {
  return (float)(philox_word0(seed, stream, (unsigned)t) >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

__global__ __launch_bounds__(64) void sample_uniforms_kernel(unsigned long long seed,
                                                             const long long* __restrict__ streams,
                                                             const int* __restrict__ step, float* __restrict__ out,
                                                             int R) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r < R) out[r] = sample_u(seed, (unsigned long long)streams[r], *step);
}

void launch_sample_uniforms(unsigned long long seed, const long long* streams, const int* step, float* out, int R,
                            hipStream_t st) {
  hipLaunchKernelGGL(sample_uniforms_kernel, dim3((R + 63) / 64), dim3(64), 0, st, seed, streams, step, out, R);
}

// ------------------------------------------------------------------ bookkeeping
// One wave (lanes 0..63) of the row's workgroup, after the draw; the row was live and t < max_dec.
__device__ __forceinline__ void sample_book(const SampleBook& bk, int r, int R, int t, int tok, float lp, int stop_id,
                                            int T, int lane) {
  if (bk.att_hist) {
    float* dst = bk.att_hist + ((size_t)t * R + r) * T;
    const float* src = bk.att + (size_t)r * T;
    for (int i = lane; i < T; i += 64) dst[i] = src[i];
  }
  if (lane == 0) {
    bk.tok_hist[(size_t)t * R + r] = tok;
    bk.lp_hist[(size_t)t * R + r] = lp;
    bk.lp_sum[r] += lp;
    bk.latest[r] = tok;
    bk.slen[r] = t + 1;
    if (tok == stop_id) bk.done[r] = 1;
    if (bk.pg_hist) bk.pg_hist[(size_t)t * R + r] = bk.pg[r];
  }
}

// ------------------------------------------------------------------ top-k draw
__global__ __launch_bounds__(64) void sample_topk_kernel(
    const int* __restrict__ top_ids, const float* __restrict__ top_lp,  // [R][K]
    const long long* __restrict__ streams, const int* __restrict__ step, unsigned long long seed,
    int* __restrict__ out_tok, float* __restrict__ out_lp, int* __restrict__ out_pick,  // [R]
    int R, int K, int k, float temp, int stop_id, int min_dec, int max_dec, int T, SampleBook bk) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int t = *step - 1;
  if (t < 0 || t >= max_dec || (bk.done && bk.done[r])) return;  // (the whole wave)
  int id = -1;
  float lp = -INFINITY;
  if (lane < K) {
    id = top_ids[(size_t)r * K + lane];
    lp = top_lp[(size_t)r * K + lane];
  }
  // the k + 1 best, [STOP] dropped before min_dec, the first k of the rest
  const bool valid = lane <= k && lane < K && (t >= min_dec || id != stop_id);
  const unsigned long long vm = __ballot(valid);
  const int rank = __popcll(vm & ((1ull << lane) - 1ull));
  const bool keep = valid && rank < k;
  const unsigned long long km = __ballot(keep);
  int pick = 0;
  if (km) {
    const float m = wave_max(keep ? lp : -INFINITY);
    const float w = keep ? expf((lp - m) / temp) : 0.f;
    float c = w;  // inclusive prefix sums, lane order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float p = __shfl_up(c, o, 64);
      if (lane >= o) c += p;
    }
    const float W = __shfl(c, 63, 64);
    const float target = sample_u(seed, (unsigned long long)streams[r], t) * W;
    const unsigned long long cross = __ballot(keep && w > 0.f && c > target);
    // rounding may leave the target at or past the last sum: the last candidate of positive weight
    const unsigned long long pos = __ballot(keep && w > 0.f);
    pick = cross ? __ffsll((long long)cross) - 1 : (pos ? 63 - __clzll((long long)pos) : __ffsll((long long)km) - 1);
  }
  const int tok = __shfl(id, pick, 64);
  const float tlp = __shfl(lp, pick, 64);
  if (lane == 0) {
    out_tok[r] = tok;
    out_lp[r] = tlp;
    out_pick[r] = pick;
  }
  if (bk.tok_hist) sample_book(bk, r, R, t, tok, tlp, stop_id, T, lane);
}

void launch_sample_topk(const int* top_ids, const float* top_lp, const long long* streams, const int* step,
                        unsigned long long seed, int* out_tok, float* out_lp, int* out_pick, int R, int K, int k,
                        float temp, int stop_id, int min_dec, int max_dec, int T, const SampleBook& bk,
                        hipStream_t st) {
  hipLaunchKernelGGL(sample_topk_kernel, dim3(R), dim3(64), 0, st, top_ids, top_lp, streams, step, seed, out_tok,
                     out_lp, out_pick, R, K, k, temp, stop_id, min_dec, max_dec, T, bk);
}

// ------------------------------------------------------------------ full-distribution draw
#define SF_THREADS 256
#define SF_WAVES (SF_THREADS / 64)
#define SF_CHUNK 256  // entries per chunk: one wave, 4 per lane
int sample_full_max_chunks() { return SAMPLE_FULL_MAX_CHUNKS; }

// this lane's 4 entries of vocabulary chunk c: logit + bias, -inf past V
__device__ __forceinline__ void sf_load(const float* __restrict__ z, const float* __restrict__ bias, int V, int c,
                                        int lane, bool vec, float (&x)[4]) {
  const int v0 = c * SF_CHUNK + lane * 4;
  if (vec && v0 + 4 <= V) {
    const float4 a = *reinterpret_cast<const float4*>(z + v0), b = *reinterpret_cast<const float4*>(bias + v0);
    x[0] = a.x + b.x; x[1] = a.y + b.y; x[2] = a.z + b.z; x[3] = a.w + b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = v0 + j < V ? z[v0 + j] + bias[v0 + j] : -INFINITY;
  }
}

// inverse CDF inside one chunk by one wave: w[0..3] are this lane's weights (entry lane * 4 + j),
// rem the target minus the sum of the chunks before.  Returns the entry's index in the chunk: the
// first whose running sum exceeds rem, else (rounding) the last of positive weight, else -1.
__device__ __forceinline__ int sf_walk(const float (&w)[4], float rem, int lane) {
  float in[4];
  in[0] = w[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) in[j] = in[j - 1] + w[j];
  float c = in[3];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float p = __shfl_up(c, o, 64);
    if (lane >= o) c += p;
  }
  const float prev = __shfl_up(c, 1, 64);
  const float base = lane == 0 ? 0.f : prev;
  int first = -1, last = -1;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (w[j] > 0.f && base + in[j] > rem) first = j;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (w[j] > 0.f) last = j;
  }
  const unsigned long long fm = __ballot(first >= 0), lm = __ballot(last >= 0);
  if (fm) {
    const int l = __ffsll((long long)fm) - 1;
    return l * 4 + __shfl(first, l, 64);
  }
  if (lm) {
    const int l = 63 - __clzll((long long)lm);
    return l * 4 + __shfl(last, l, 64);
  }
  return -1;
}

__global__ __launch_bounds__(SF_THREADS) void sample_full_kernel(
    const float* __restrict__ logits, const float* __restrict__ bias,  // [R][V], [V]
    const float* __restrict__ pgen, const float* __restrict__ attn,    // [R], [R][T] (both or neither)
    const int* __restrict__ ext, const int* __restrict__ lens,         // [R / rows][T], [R / rows]
    const long long* __restrict__ streams, const int* __restrict__ step, unsigned long long seed,
    int* __restrict__ out_tok, float* __restrict__ out_lp, int* __restrict__ out_pick,  // [R]
    int R, int V, int T, int rows, int stop_id, int min_dec, int max_dec, int* __restrict__ err, SampleBook bk) {
  __shared__ float cm[SAMPLE_FULL_MAX_CHUNKS];  // chunk max (vocabulary chunks)
  __shared__ float cw[SAMPLE_FULL_MAX_CHUNKS];  // chunk sum of exponentials, then chunk weight
  __shared__ float seg[SF_THREADS];             // per-thread segment sums, then their exclusive scan
  __shared__ float red[SF_WAVES];
  __shared__ float s_tot;
  __shared__ int s_cross, s_lastpos, s_tok, s_entry;
  __shared__ float s_excl;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int t = *step - 1;
  if (t < 0 || t >= max_dec || (bk.done && bk.done[r])) return;  // (the whole workgroup)
  const int art = r / rows;
  const bool ptr = pgen != nullptr;
  const float pg = ptr ? pgen[r] : 1.f;
  int len = ptr ? (int)DCHECK_IDX(lens[art], 0, T + 1, CHK_LOSS_LEN) : 0;
  len = min(max(len, 0), T);
  const bool allow_stop = t >= min_dec;
  const int ncv = (V + SF_CHUNK - 1) / SF_CHUNK, ncp = (len + SF_CHUNK - 1) / SF_CHUNK, nch = ncv + ncp;
  const float* z = logits + (size_t)r * V;
  const float* a = ptr ? attn + (size_t)r * T : nullptr;
  const int* ex = ext + (size_t)art * T;
  const bool vec = (V & 3) == 0;
  const int stop_chunk = (!allow_stop && stop_id >= 0 && stop_id < V) ? stop_id / SF_CHUNK : -1;
  if (tid == 0) {
    s_cross = 0x7fffffff;
    s_lastpos = -1;
  }
  // ---- the one pass over the row: per-chunk (max, sum of exponentials); the [STOP] chunk keeps
  // the full sum for the softmax normaliser in cm / cw and its sum without [STOP] in s_excl
  for (int c = wv; c < ncv; c += SF_WAVES) {
    float x[4];
    sf_load(z, bias, V, c, lane, vec, x);
    const float m = wave_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = m > -INFINITY ? fexp(x[j] - m) : 0.f;  // (-inf past V: 0; a chunk of -inf: 0)
    const float s = wave_sum((e[0] + e[1]) + (e[2] + e[3]));
    if (c == stop_chunk) {
      const int sl = stop_id - c * SF_CHUNK;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lane * 4 + j == sl) e[j] = 0.f;
      const float se = wave_sum((e[0] + e[1]) + (e[2] + e[3]));
      if (lane == 0) s_excl = se;
    }
    if (lane == 0) {
      cm[c] = m;
      cw[c] = s;
    }
  }
  __syncthreads();
  // ---- row max and sum (thread q takes chunks q, q + 256, ..: fixed by the shape)
  float m_loc = -INFINITY;
  for (int c = tid; c < ncv; c += SF_THREADS) m_loc = fmaxf(m_loc, cm[c]);
  const float M = block_max<SF_THREADS>(m_loc, red);
  float s_loc = 0.f;
  for (int c = tid; c < ncv; c += SF_THREADS) s_loc += cw[c] * fexp(cm[c] - M);
  const float S = block_sum<SF_THREADS>(s_loc, red);
  const float scale = pg / S;
  const float excl = stop_chunk >= 0 ? s_excl : 0.f;
  __syncthreads();
  // ---- chunk weights: vocabulary chunks p_gen / S * (sum of exponentials) * exp(max - M) ...
  for (int c = tid; c < ncv; c += SF_THREADS) cw[c] = scale * (c == stop_chunk ? excl : cw[c]) * fexp(cm[c] - M);
  // ... and the article positions i < len, (1 - p_gen) * a_i, [STOP] copies dropped before min_dec
  for (int p = wv; p < ncp; p += SF_WAVES) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = p * SF_CHUNK + lane * 4 + j;
      if (i < len && (allow_stop || ex[i] != stop_id)) s += (1.f - pg) * a[i];
    }
    s = wave_sum(s);
    if (lane == 0) cw[ncv + p] = s;
  }
  __syncthreads();
  // ---- scan of the chunk weights: thread q owns chunks q * per .. (q + 1) * per - 1
  const int per = (nch + SF_THREADS - 1) / SF_THREADS;
  const int c_lo = min(tid * per, nch), c_hi = min(c_lo + per, nch);
  float sg = 0.f;
  for (int c = c_lo; c < c_hi; ++c) sg += cw[c];
  seg[tid] = sg;
  __syncthreads();
  if (wv == 0) {  // wave 0: exclusive scan of the 256 segment sums, 4 per lane
    float v[4], in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = seg[lane * 4 + j];
    in[0] = v[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) in[j] = in[j - 1] + v[j];
    float c = in[3];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float q = __shfl_up(c, o, 64);
      if (lane >= o) c += q;
    }
    const float prev = __shfl_up(c, 1, 64);
    const float base = lane == 0 ? 0.f : prev;
    seg[lane * 4] = base;
#pragma unroll
    for (int j = 1; j < 4; ++j) seg[lane * 4 + j] = base + in[j - 1];
    if (lane == 63) s_tot = c;
  }
  __syncthreads();
  const float W = s_tot;
  const float target = sample_u(seed, (unsigned long long)streams[r], t) * W;
  {
    float run = seg[tid];
    for (int c = c_lo; c < c_hi; ++c) {
      const float w = cw[c], nxt = run + w;
      if (w > 0.f) {
        atomicMax(&s_lastpos, c);
        // the first chunk whose running sum exceeds the target.  No lower test (run <= target): a
        // thread's run starts from the scanned segment base, summed in another order than the
        // thread before it sums, so the two may leave an ulp between them that no chunk would own
        if (nxt > target) atomicMin(&s_cross, c);
      }
      run = nxt;
    }
  }
  __syncthreads();
  // ---- the owning chunk walks to the crossing (wave 0); no crossing (rounding): the last chunk of
  // positive weight, target past its end, which sf_walk clamps to its last positive entry
  int cstar = s_cross;
  const bool clamped = cstar == 0x7fffffff;
  if (clamped) cstar = s_lastpos;
  if (wv == 0) {
    int entry = -1, tok = stop_id;
    if (cstar >= 0) {
      cstar = (int)DCHECK_IDX(cstar, 0, nch, CHK_SAMPLE_CHUNK);
      // the sum of the chunks before, in this thread layout's order
      const int own = cstar / per;
      float before = seg[own];
      for (int c = own * per; c < cstar; ++c) before += cw[c];
      const float rem = clamped ? INFINITY : target - before;
      float w[4];
      if (cstar < ncv) {
        float x[4];
        sf_load(z, bias, V, cstar, lane, vec, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int v = cstar * SF_CHUNK + lane * 4 + j;
          w[j] = (v < V && (allow_stop || v != stop_id)) ? scale * fexp(x[j] - M) : 0.f;
        }
        const int e = sf_walk(w, rem, lane);
        if (e >= 0) {
          entry = cstar * SF_CHUNK + e;
          tok = entry;
        }
      } else {
        const int p = cstar - ncv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = p * SF_CHUNK + lane * 4 + j;
          w[j] = (i < len && (allow_stop || ex[i] != stop_id)) ? (1.f - pg) * a[i] : 0.f;
        }
        const int e = sf_walk(w, rem, lane);
        if (e >= 0) {
          const int i = min(p * SF_CHUNK + e, T - 1);
          entry = V + i;
          tok = ex[i];
        }
      }
    }
    if (lane == 0) {
      s_tok = tok;
      s_entry = entry;
      // nothing to draw from (every weight 0, or NaN): the row ends with [STOP] and entry -1, and
      // the error word tells the host, which raises (the host rule raises ValueError here)
      if (entry < 0 && err) *err = 1;
    }
  }
  __syncthreads();
  // ---- the chosen token's model log-prob: its softmax term plus the attention of every copy
  const int tok = s_tok;
  float cp = 0.f;
  for (int i = tid; i < len; i += SF_THREADS)
    if (ex[i] == tok) cp += a[i];
  cp = block_sum<SF_THREADS>(cp, red);
  if (wv == 0) {
    const float pv = (tok >= 0 && tok < V) ? fexp(z[tok] + bias[tok] - M) / S : 0.f;
    const float lp = __logf(pg * pv + (1.f - pg) * cp);
    if (lane == 0) {
      out_tok[r] = tok;
      out_lp[r] = lp;
      out_pick[r] = s_entry;
    }
    if (bk.tok_hist) sample_book(bk, r, R, t, tok, lp, stop_id, T, lane);
  }
}

void launch_sample_full(const float* logits, const float* bias, const float* pgen, const float* attn, const int* ext,
                        const int* lens, const long long* streams, const int* step, unsigned long long seed,
                        int* out_tok, float* out_lp, int* out_pick, int R, int V, int T, int rows, int stop_id,
                        int min_dec, int max_dec, int* err, const SampleBook& bk, hipStream_t st) {
  hipLaunchKernelGGL(sample_full_kernel, dim3(R), dim3(SF_THREADS), 0, st, logits, bias, pgen, attn, ext, lens, streams,
                     step, seed, out_tok, out_lp, out_pick, R, V, T, rows, stop_id, min_dec, max_dec, err, bk);
}
