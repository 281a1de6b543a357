// Beam bookkeeping shared by beam_step_kernel (beam.hip) and the vocab select kernel's fused
// per-article tail (vocab_topk.hip): extend each live hypothesis with its top-K candidates,
// rank by total log-prob, collect finished (STOP) hypotheses after min_dec steps, keep the
// best ``beam`` live ones (reference beam_search.py:110-156).
#pragma once
#include <type_traits>
#include "common.h"
#include "launchers.h"

#define BEAM_CAND_MAX 16  // max beam (new hypotheses kept per step)
// candidates per article: beam * K <= 64 in the one-wave bookkeeping (beam_step_body), up to
// 16 * 32 in the workgroup-wide one (beam_step_wide_kernel, beam.hip)
#define BEAM_WIDE_CAND 512

// ------------------------------------------------------------------ n-gram blocking
// block_ngram_repeat = n (decode/beam_search.py ngram_blocked): candidate w of a hypothesis with
// tokens s[0..t] is blocked iff some e in [n - 1, t] has s[e] == w and s[e-n+1 .. e-1] equal to
// the hypothesis' last n - 1 tokens.  A blocked candidate's step log-prob becomes BLOCKED_LP: it
// ranks behind every unblocked one and is taken only when nothing else is left.
#define BLOCKED_LP (-1e20f)
// the kernels' optional trailing arguments: a pack of zero or one NgSeq, then zero or one BeamPen
template <typename T, typename... A>
constexpr bool pack_has = (std::is_same_v<T, A> || ...);
__device__ __forceinline__ NgSeq ng_of() { return NgSeq{}; }
__device__ __forceinline__ NgSeq ng_of(const NgSeq& x) { return x; }
__device__ __forceinline__ NgSeq ng_of(const BeamPen&) { return NgSeq{}; }
__device__ __forceinline__ NgSeq ng_of(const NgSeq& x, const BeamPen&) { return x; }
__device__ __forceinline__ BeamPen pen_of() { return BeamPen{}; }
__device__ __forceinline__ BeamPen pen_of(const NgSeq&) { return BeamPen{}; }
__device__ __forceinline__ BeamPen pen_of(const BeamPen& p) { return p; }
__device__ __forceinline__ BeamPen pen_of(const NgSeq&, const BeamPen& p) { return p; }

// The candidate-independent half of the test, once per article by the whole workgroup:
// ban[i * P + e] = s_i[e] where the n - 1 tokens before e match hypothesis i's suffix, else -1
// (also for e in (t, next multiple of 4), so the candidates scan whole int4s).  The sequences
// come from global memory (written by the previous step's launch; independent loads, L2).
__device__ __forceinline__ void ngram_ban_build(const int* __restrict__ seq_in, int* ban, int base, int beam, int P,
                                                int n, int t, int R) {
  const int t4 = (t + 4) & ~3;  // t + 1 tokens rounded up: <= P
  for (int idx = threadIdx.x; idx < beam * t4; idx += blockDim.x) {
    const int i = idx / t4, e = idx - i * t4;
    const int* s = seq_in + (size_t)DCHECK_IDX(base + i, 0, R, CHK_BEAM_SEQ) * P;
    DCHECK_IN(e, 0, P, CHK_BEAM_SEQ);
    int v = -1;
    if (e >= n - 1 && e <= t) {
      bool m = true;
      for (int k = 1; k < n; ++k) m &= s[e - k] == s[t + 1 - k];
      if (m) v = s[e];
    }
    ban[i * P + e] = v;
  }
}

// candidate (hypothesis i, token w >= 0): is w in the hypothesis' ban list?
__device__ __forceinline__ bool ngram_banned(const int* ban, int i, int P, int t, int w) {
  const int4* b = reinterpret_cast<const int4*>(ban + i * P);  // ban 16-byte aligned, P % 4 == 0
  bool hit = false;
  for (int q = 0; q <= (t >> 2); ++q) {
    const int4 v = b[q];
    hit |= (v.x == w) | (v.y == w) | (v.z == w) | (v.w == w);
  }
  return hit;
}

// seq_out[base + k] = seq_in[base + parent of k][0..t] ++ [token of k] for the new hypotheses
// (adv_par / adv_tok: LDS, written by beam_step_body), by the whole workgroup
__device__ __forceinline__ void ngram_seq_advance(const int* __restrict__ seq_in, int* __restrict__ seq_out,
                                                  const int* adv_par, const int* adv_tok, int base, int beam, int P,
                                                  int t, int R) {
  const int L1 = t + 2;  // <= max_dec + 1 <= P
  for (int idx = threadIdx.x; idx < beam * L1; idx += blockDim.x) {
    const int k = idx / L1, e = idx - k * L1;
    const int par = (int)DCHECK_IDX(adv_par[k], 0, beam, CHK_BEAM_SEQ);
    DCHECK_IN(e, 0, P, CHK_BEAM_SEQ);
    DCHECK_IN(base + k, 0, R, CHK_BEAM_SEQ);
    seq_out[(size_t)(base + k) * P + e] = e <= t ? seq_in[(size_t)(base + par) * P + e] : adv_tok[k];
  }
}

// ------------------------------------------------------------------ length / coverage penalties
// The rank key of a candidate with raw total tot of parent row ``row`` at step t (BeamPen,
// launchers.h).  Contraction is off here: each product and the difference is rounded on its own,
// so an fp32 mirror on the host reproduces every key bit for bit.
__device__ __forceinline__ float pen_key(const BeamPen& pen, float tot, int t, int row) {
#pragma clang fp contract(off)
  float key = tot * pen.inv_len[t + 2];
  if (pen.cpen) {
    const float p = pen.beta * pen.cpen[row];
    key = key - p;
  }
  return key;
}

// ------------------------------------------------------------------ beam bookkeeping
// PEN (pen, ckey: one more [64] LDS array): rank by pen_key instead of the raw total, which is
// still what lp_sum carries.
// NG: also leaves each new hypothesis' parent slot and token in adv_par / adv_tok (LDS, [beam])
// for ngram_seq_advance
template <bool NG = false, bool PEN = false>
__device__ __forceinline__ void beam_step_body(
    const int* __restrict__ top_ids, const float* __restrict__ top_lp, float* __restrict__ lp_sum,
    int* __restrict__ latest, int* __restrict__ gidx, int* __restrict__ tok_hist, int* __restrict__ par_hist,
    int* __restrict__ done, int* __restrict__ res_count, float* __restrict__ res_score, int* __restrict__ res_len,
    int* __restrict__ res_step, int* __restrict__ res_par, float* cval, int* cid, int* srt, int a, int lane, int t,
    int base, int beam, int K, int stop_id, int min_dec, float tot, int tid_cand, int nres0, int Na,
    int* adv_par = nullptr, int* adv_tok = nullptr, const BeamPen& pen = BeamPen{}, float* ckey = nullptr) {
  // tot / tid_cand / nres0: this lane's candidate and the result count, loaded by the caller
  // in the same memory round trip as the step counter and the done flag
  const int norig = t == 0 ? 1 : beam;
  const int ncand = norig * K;
  if (lane >= ncand) tot = -INFINITY;
  float key = tot;  // what the candidates are ranked by
  if constexpr (PEN) {
    // (lanes past ncand hold a row of the article -- rows >= 1 at t == 0 -- or lane / K >= beam)
    key = lane < ncand ? pen_key(pen, tot, t, base + lane / K) : -INFINITY;
  }
  // stable rank: descending total, ties keep candidate order (readlane: a uniform lane index,
  // no LDS permute per candidate)
  int rank = 0;
  for (int q = 0; q < ncand; ++q) {
    const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(key), q));
    if (v > key || (v == key && q < lane)) ++rank;
  }
  if (lane < ncand) {  // rank-ordered candidate table: value, token, parent
    cval[rank] = tot;
    if constexpr (PEN) ckey[rank] = key;
    cid[rank] = tid_cand;
    srt[rank] = lane / K;
  }
  __shared__ float nlp[BEAM_CAND_MAX];
  __shared__ int ntok[BEAM_CAND_MAX], npar[BEAM_CAND_MAX];
  __shared__ int nh_s, nres_s;
  __shared__ float nkey[PEN ? BEAM_CAND_MAX : 1];
  __syncthreads();
  // The reference walks the ranked candidates in order: a STOP (from step min_dec on) becomes a
  // result, any other token a new hypothesis, until beam of either (beam_search.py:120-150).
  // Here every rank position decides at once: with the exclusive counts of results / hypotheses
  // ranked before it (ballot + popcount), position q is reached iff both counts are still below
  // beam, and its slot is that count.
  if (lane < 64) {
    const bool act = lane < ncand;
    const int tok = act ? cid[lane] : 0;
    const bool is_res = act && tok == stop_id && t >= min_dec;
    const bool is_hyp = act && tok != stop_id;
    const unsigned long long below = (1ull << lane) - 1ull;  // lanes < this one (lane <= 63)
    const unsigned long long mres = __ballot(is_res), mhyp = __ballot(is_hyp);
    const int ns = __popcll(mres & below), nn = __popcll(mhyp & below);
    const bool reached = act && nn < beam && nres0 + ns < beam;
    const float v = act ? cval[lane] : 0.f;
    const int par = act ? srt[lane] : 0;
    if (reached && is_res) {
      const int slot = a * beam + nres0 + ns;
      if constexpr (PEN) {
        res_score[slot] = ckey[lane];
        pen.res_lp[slot] = v;
      } else {
        res_score[slot] = v / (float)(t + 2);
      }
      res_len[slot] = t + 2;
      res_step[slot] = t;
      res_par[slot] = par;
    }
    if (reached && is_hyp) {
      nlp[nn] = v;
      if constexpr (PEN) nkey[nn] = ckey[lane];
      ntok[nn] = tok;
      npar[nn] = par;
    }
    const unsigned long long mreach = __ballot(reached);
    if (lane == 0) {
      const int nres = nres0 + __popcll(mres & mreach);
      nh_s = __popcll(mhyp & mreach);
      nres_s = nres;
      res_count[a] = nres;
      if (nres >= beam) done[a] = 1;
    }
  }
  __syncthreads();
  if (lane < beam) {
    const int nh = nh_s, k = lane;
    const int kk = k < nh ? k : (nh > 0 ? nh - 1 : 0);
    const int par = nh > 0 ? npar[kk] : 0;
    lp_sum[base + k] = nh > 0 ? nlp[kk] : -INFINITY;
    if constexpr (PEN) pen.key_sum[base + k] = nh > 0 ? nkey[kk] : -INFINITY;
    latest[base + k] = nh > 0 ? ntok[kk] : stop_id;
    gidx[base + k] = base + par;
    tok_hist[(size_t)t * Na * beam + base + k] = nh > 0 ? ntok[kk] : stop_id;
    par_hist[(size_t)t * Na * beam + base + k] = par;
    if constexpr (NG) {
      adv_par[k] = par;
      adv_tok[k] = nh > 0 ? ntok[kk] : stop_id;
    }
  }
  (void)nres_s;
}


// Beam bookkeeping of article a run by the LAST of its rows' workgroups in the vocab select
// kernel (vocab_topk.hip, BeamTail): the same steps as beam_step_kernel for one article, with
// t = *step - 1 (the step counter was advanced at the start of this decode step).  The rows'
// candidates arrive as tagged 64-bit granules {tag = step (15 bits) | id (17 bits), log-prob}
// written with relaxed agent-scope atomic stores by the rows' workgroups (possibly on other
// XCDs): the tail polls them until every tag is this step's -- no device-scope fence (on this
// GPU a release fence writes back the whole L2).  Every thread of the workgroup calls it (it
// contains block barriers); lanes < 64 do the work.  err: set when a poll times out.
// NG (n-gram blocking): the whole workgroup builds the article's ban table (ban: >= beam * ng.P
// ints of LDS, 16-byte aligned) before the poll and advances the sequences after the bookkeeping
// (adv: 2 * BEAM_CAND_MAX ints of LDS).
// PEN (length / coverage penalties): only the bookkeeping after the poll differs (beam_step_body).
template <bool NG = false, bool PEN = false>
__device__ __forceinline__ void beam_article_tail(const BeamTail& bt, int a, float* cval, int* cid, int* srt,
                                                  const NgSeq& ng = NgSeq{}, int* ban = nullptr, int* adv = nullptr,
                                                  const BeamPen& pen = BeamPen{}, float* ckey = nullptr) {
  const int lane = threadIdx.x, beam = bt.beam, K = bt.K, base = a * beam;
  const size_t R = (size_t)bt.Na * beam;
  const int t = *bt.step - 1;
  const unsigned tag = (unsigned)(*bt.step) & 0x7fffu;
  const int is_done = bt.done[a], nres0 = bt.res_count[a];
  if constexpr (NG) {
    if (!(is_done || t >= bt.max_dec)) ngram_ban_build(ng.seq[t & 1], ban, base, beam, ng.P, ng.n, t, (int)R);
  }
  float tot = -INFINITY;
  int tid_cand = 0;
  if (lane < beam * K) {
    const int i = lane / K, j = lane % K;
    const unsigned long long* g = bt.gran + (size_t)(base + i) * K + j;
    unsigned long long x = 0;
    for (unsigned spins = 0;; ++spins) {
      x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)(x >> 49) == tag) break;
      if (spins > (1u << 20)) {  // bounded: results garbage, error recorded, the grid drains
        __hip_atomic_store(bt.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    tid_cand = (int)((x >> 32) & 0x1ffffu);
    tot = bt.lp_sum[base + i] + __uint_as_float((unsigned)x);
  }
  if (bt.att_hist) {
    const size_t th = (size_t)min(t, bt.max_dec - 1);
    // (att was written by the previous launch; each row workgroup stores its own pg_hist entry)
    for (int i = lane; i < beam * bt.T; i += blockDim.x)
      bt.att_hist[(th * R + base) * bt.T + i] = bt.att[(size_t)base * bt.T + i];
  }
  if (is_done || t >= bt.max_dec) {
    if (lane < beam) bt.gidx[base + lane] = base + lane;
  } else if constexpr (NG) {
    __syncthreads();  // the ban table is complete
    if (lane < beam * K && ngram_banned(ban, lane / K, ng.P, t, tid_cand))
      tot = bt.lp_sum[base + lane / K] + BLOCKED_LP;
    beam_step_body<true, PEN>(nullptr, nullptr, bt.lp_sum, bt.latest, bt.gidx, bt.tok_hist, bt.par_hist, bt.done,
                              bt.res_count, bt.res_score, bt.res_len, bt.res_step, bt.res_par, cval, cid, srt, a, lane,
                              t, base, beam, K, bt.stop_id, bt.min_dec, tot, tid_cand, nres0, bt.Na, adv,
                              adv + BEAM_CAND_MAX, pen, ckey);
    __syncthreads();  // the new hypotheses' parents / tokens written by lanes < beam
    ngram_seq_advance(ng.seq[t & 1], ng.seq[(t + 1) & 1], adv, adv + BEAM_CAND_MAX, base, beam, ng.P, t, (int)R);
  } else {
    beam_step_body<false, PEN>(nullptr, nullptr, bt.lp_sum, bt.latest, bt.gidx, bt.tok_hist, bt.par_hist, bt.done,
                               bt.res_count, bt.res_score, bt.res_len, bt.res_step, bt.res_par, cval, cid, srt, a, lane,
                               t, base, beam, K, bt.stop_id, bt.min_dec, tot, tid_cand, nres0, bt.Na, nullptr, nullptr,
                               pen, ckey);
  }
}
