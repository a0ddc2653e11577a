// Host-only plumbing of the one-launch engines whose workgroups hand off to one another through the `partials` records (mi_ode_persist.h):
// the workgroups spin, so the whole grid has to be co-resident.  Used by the adaptive adjoints (mi_ode_adjoint.hip, mi_ode_linadj.hip) and,
// through mi_ode_discrete_host.h, by the four discrete sweeps.  `what` is the engine's name in front of every error message.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_persist.h"

namespace mi {

struct HandoffHost {           // embedded in each handle
  int grid, block;
  size_t lds;
  double* partials;            // hand-off records (2 parities)
  unsigned seq;                // sequence numbers already used on this handle
  int spin_limit, spin_first;
};

// A device, its CU count to *cus, the dynamic LDS attribute on every kernel of fns, the occupancy of the first.
inline int handoff_device(const void* const* fns, int n_fns, int block, size_t lds, int* cus, const char* what) {
  int ndev = 0, dev = 0, per_cu = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) { mi_set_error("%s: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  for (int i = 0; i < n_fns; ++i)
    if (hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fns[0], block, lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    mi_set_error("%s kernel does not fit a compute unit (LDS %zu bytes, %d threads)", what, lds, block);
    return MI_ODE_E_HIP;
  }
  return 0;
}

// every workgroup co-resident (the hand-offs spin): at most one per CU
inline int handoff_cap_grid(long long g, int cus, int max_grid = kPersistMaxGrid) {
  if (g > cus) g = cus;
  if (g > max_grid) g = max_grid;
  return (int)g;
}

// The hand-off records, after the engine's own allocations (e: their outcome, passed on), and the spin bounds.  spin_limit: the skew a
// hand-off of this engine absorbs - a bound, not a time-out to hit; spin_first: the residency check of the first hand-off of a launch.
inline hipError_t handoff_alloc(HandoffHost& c, hipError_t e, int spin_limit) {
  const size_t rec_bytes = (size_t)kMaxBlocks * kRec * sizeof(double);
  if (e == hipSuccess) e = hipMalloc((void**)&c.partials, rec_bytes);
  if (e == hipSuccess) e = hipMemset(c.partials, 0, rec_bytes);
  c.seq = 0;
  c.spin_limit = spin_limit;
  c.spin_first = 1 << 14;
  if (const char* e3 = getenv("MI_ODE_PERSIST_SPIN_FIRST")) c.spin_first = atoi(e3);
  if (const char* e2 = getenv("MI_ODE_PERSIST_SPIN_LIMIT")) c.spin_limit = atoi(e2);
  return e;
}

// The hand-off fields of a single-rank launch.
inline void handoff_fill(PersistArgs& p, const HandoffHost& c) {
  p.s.partials = c.partials;
  p.world = 1;
  p.seq_base = c.seq;
  p.spin_limit = c.spin_limit;
  p.spin_first = c.spin_first < c.spin_limit ? c.spin_first : c.spin_limit;
  p.sleep_first = c.grid <= 32 ? 16 : 32; p.sleep_poll = 2;
}

// The next launch stamps its records past the `used` sequence numbers of this one.
inline void handoff_advance(HandoffHost& c, unsigned used) {
  c.seq += used;
  if (c.seq >= 0xE0000000u) c.seq = 0;
}

// The result record of an adaptive dopri5 segment (AdjResult, LinAdjResult) as mi_ode_stats; reversed: the kernel integrated -t.
template <class Result>
inline void handoff_stats(mi_ode_stats* stats, const Result& r, bool reversed) {
  memset(stats, 0, sizeof(*stats));
  stats->n_attempts = r.n_attempt; stats->n_accepted = r.n_accept; stats->n_rejected = r.n_attempt - r.n_accept;
  stats->nfe = 2 + 6 * r.n_attempt;
  stats->t = reversed ? -r.t1 : r.t1; stats->dt = r.dt; stats->last_ratio = r.ratio; stats->status = r.status;
  stats->n_polls = 1; stats->n_launches = 1;
}

}  // namespace mi
