// In-launch hand-offs between the workgroups of a persistent kernel (lstm_persistent.hip,
// decoder_persistent.hip, decoder_bwd_persistent.hip): the data is the flag.  A payload travels as
// 8-byte {tag, value} granules, each written with ONE agent-scope store and polled with agent-scope
// loads until the tag matches (tags = step index + 1; the granule buffer is zeroed before every
// launch).  Team members are placed on one XCD (team_of), so a hand-off stays in that XCD's L2.
// Every spin is bounded: on timeout the wave records its family's code (the enum below; messages:
// HANDOFF_CODES in models/engine_config.py) in *err and stops waiting (results are then garbage,
// but the grid always drains).  The host side is here too: team_grid and resident_capacity.
#pragma once
#include "common.h"
#include <initializer_list>
#include <mutex>

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

namespace handoff {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;
// a sweep gives up after kSpinLimit / 4 passes with s_sleep(SLEEP) between them: ~0.1-1 s at 24
constexpr unsigned kSpinLimit = 1u << 21;
enum : unsigned { kErrLstmFwd = 1, kErrLstmBwd = 2, kErrDecFwd = 3, kErrDecBwd = 4 };

__device__ __forceinline__ unsigned pack_bf2(float lo, float hi) {
  const unsigned a = __builtin_bit_cast(unsigned short, f2bf(lo));
  const unsigned b = __builtin_bit_cast(unsigned short, f2bf(hi));
  return a | (b << 16);
}

__device__ __forceinline__ void store_granule(gu64* g, unsigned tag, unsigned v) {
  __hip_atomic_store(g, ((unsigned long long)tag << 32) | v, RLX_AGENT);
}

// One wave reads NPL granules per lane (indices first + j*64 + lane) until every tag
// matches; a pass re-reads only the granules that were not ready yet.  SLEEP: the s_sleep argument
// between passes (64 clocks each), a per-kernel choice.
template <int NPL, int SLEEP = 24>
__device__ __forceinline__ void sweep(const gu64* g, int first, unsigned tag, unsigned (&v)[NPL], bool& dead,
                                      gu32* err, unsigned code, int lane) {
  static_assert(NPL <= 32, "ready mask is 32 bits");
  constexpr unsigned all = NPL == 32 ? 0xffffffffu : ((1u << NPL) - 1);
  unsigned ready = 0;
  unsigned long long x[NPL];
  for (unsigned spins = 0;;) {
    // issue every outstanding load first (one round trip per pass), then check them
#pragma unroll
    for (int j = 0; j < NPL; ++j)
      if (!((ready >> j) & 1)) x[j] = __hip_atomic_load(g + first + j * 64 + lane, RLX_AGENT);
#pragma unroll
    for (int j = 0; j < NPL; ++j)
      if (!((ready >> j) & 1) && (unsigned)(x[j] >> 32) == tag) {
        v[j] = (unsigned)x[j];
        ready |= 1u << j;
      }
    if (__all(ready == all) || dead) return;
    if (++spins > kSpinLimit / 4) {
      if (lane == 0) __hip_atomic_store(err, code, RLX_AGENT);
      dead = true;
      return;
    }
    // The LSTM's s_sleep(24) (~1500 clocks) between passes: the polls of 32 teams are a large share of
    // the L2 traffic, and fewer of them lower every team's hand-off latency (tools/lstm_micro.py,
    // per step: H = 512, B = 256: 6.82 us with s_sleep(1), 6.65 with 8, 6.28 with 24, 6.27 with
    // 48; H = 256, B = 256: 3.01 / 2.97 / 2.97 / 3.46).  Spinning on one granule per lane first
    // and sweeping once it is ready costs one more L2 round trip: 6.8 -> 8.3 us.
    __builtin_amdgcn_s_sleep(SLEEP);
  }
}

// block -> (team, slice): team members share blockIdx % 8 (same XCD under round-robin dealing)
__device__ __forceinline__ bool team_of(int NC, int nteams, int& team, int& c) {
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  team = (q / NC) * 8 + xcd;
  c = q % NC;
  return team < nteams;
}

// The kernel's arguments (one struct), read from the kernarg segment where they are used.  The segment
// pointer is made opaque once per phase: a phase loads the few pointers it needs into SGPRs and drops
// them at its end, instead of all of them staying live (and spilling) through the whole step loop.
template <class Args>
__device__ __forceinline__ const Args __attribute__((address_space(4)))* phase_args() {
  typedef const Args __attribute__((address_space(4))) KArgs;
  KArgs* a = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return a;
}
// The thread index, opaque per phase, so that a phase's per-thread addresses are re-derived in it.
__device__ __forceinline__ int phase_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// ------------------------------------------------------------------------------ host side
// workgroups of a launch: nteams teams of NC workgroups, dealt 8 at a time (one per XCD, see team_of)
constexpr int team_grid(int NC, int nteams) { return 8 * NC * ((nteams + 7) / 8); }

struct Probe {  // one kernel variant of a persistent family, as it is launched
  const void* kernel;
  int threads, dyn_lds;
};
constexpr int kMaxDevices = 64;
// Workgroups the current device keeps resident at once: the CU count the runtime reports (not an
// assumed 256: a partitioned or smaller device shrinks the admissible grid instead of spinning into
// the timeout) when the occupancy query admits every probe, else 0, as without a device.  It also
// sets MaxDynamicSharedMemorySize, so launchers call it first.  What may hold CUs beside the launch
// comes off it in fits_resident (models/engine_config.py).  cache: one per probe list, capacity + 1.
inline int resident_capacity(int (&cache)[kMaxDevices], std::initializer_list<Probe> probes) {
  static std::mutex mu;  // guards every cache
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (cache[dev]) return cache[dev] - 1;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
  bool ok = true;
  for (const Probe& p : probes) {
    int occ = 0;
    if (p.dyn_lds > 0)
      ok = ok && hipFuncSetAttribute(p.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, p.dyn_lds) == hipSuccess;
    ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, p.kernel, p.threads, p.dyn_lds) == hipSuccess &&
         occ >= 1;
  }
  const int cap = ok ? cus : 0;
  cache[dev] = cap + 1;
  return cap;
}

}  // namespace handoff
