// Host-only plumbing shared by the one-launch discrete sweeps whose argument block travels through device memory: mi_ode_discrete.hip,
// mi_ode_discrete64.hip, mi_ode_discrete_linear.hip and mi_ode_discrete_linear_grid.hip.  Device check, grid cap, hand-off records and
// spin bounds are those of every hand-off engine (mi_ode_handoff_host.h); what is here is the sweeps' own.  `what` is the engine's name in
// front of every error message.  Each sweep is disc_begin, the fill of its argument block, disc_run: hipStreamSynchronize, hipMemcpyAsync,
// (float64: the two pack launches,) hipLaunchKernel, hipStreamSynchronize.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "mi_ode_handoff_host.h"
#include "mi_ode_discrete.h"

namespace mi {

struct DiscHost : HandoffHost {   // embedded in each handle
  int S;                       // stages
  DiscResult* res;             // pinned host
  void* args_host;             // pinned staging of the kernel's argument block ...
  void* args_dev;              // ... and its device copy (the kernel and its non-inlined passes read it with scalar loads)
  size_t args_bytes;
  double prof_us[3];
};

// a tableau of n_stages rows has n_stages + 1 stages; c_sol carries b
inline int disc_check_tableau(const mi_ode_tableau& tb, const char* what) {
  if (tb.n_stages >= 0 && tb.n_stages + 1 <= kDiscMaxStages) return 0;
  mi_set_error("%s: explicit Runge-Kutta tableaus of at most %d stages", what, kDiscMaxStages);
  return MI_ODE_E_INVALID;
}

inline int disc_check_points(int n_points, const char* what) {
  if (n_points >= 2 && n_points - 1 <= kDiscMaxSteps) return 0;
  mi_set_error("%s: 2 <= n_points <= %d", what, kDiscMaxSteps + 1);
  return MI_ODE_E_INVALID;
}

// The grid of the linear sweeps' 16-row tiles of width D: a workgroup per tile, and at least one per 1024 entries of the final fold - a small
// batch still spreads the fold of D * D + D entries; the extra workgroups own no tile and contribute zeros.
inline int disc_linear_grid(long long batch, int D, int cus) {
  const long long ntiles = (batch + 15) / 16, fold = ((long long)D * D + D + 1023) / 1024;
  return handoff_cap_grid(ntiles < fold ? fold : ntiles, cus);
}

// The common block's memory, after the engine's own allocations (e: their outcome), and the spin bounds.
inline int disc_alloc(DiscHost& c, hipError_t e, size_t args_bytes, const char* what) {
  c.args_bytes = args_bytes;
  e = handoff_alloc(c, e, 1 << 22);              // the final hand-off absorbs the skew of a whole sweep (tiles are dealt round-robin: at most one
                                                 // tile of every step); the first comes right after the weights or slices are staged
  if (e == hipSuccess) e = hipHostMalloc((void**)&c.res, sizeof(DiscResult), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc(&c.args_host, args_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc(&c.args_dev, args_bytes);
  if (e != hipSuccess) { mi_set_error("%s workspace: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  memset(c.res, 0, sizeof(DiscResult));
  return 0;
}

inline void disc_free(DiscHost& c) {
  if (c.partials) (void)hipFree(c.partials);
  if (c.res) (void)hipHostFree(c.res);
  if (c.args_host) (void)hipHostFree(c.args_host);
  if (c.args_dev) (void)hipFree(c.args_dev);
}

// First act of a sweep: the pinned argument block may still be in flight from a previous call; then it is all zero.
inline int disc_begin(DiscHost& c, hipStream_t st) {
  MI_HIP(hipStreamSynchronize(st));
  memset(c.args_host, 0, c.args_bytes);
  return 0;
}

// Shape and hand-off plumbing of a single-rank sweep (the weights in p.s.rhs are the engine's to fill).
inline void disc_fill_persist(PersistArgs& p, const DiscHost& c, long long batch, int dim) {
  StepArgs& s = p.s;
  s.batch = batch; s.dim = dim; s.n_plane = batch * (long long)dim;
  s.rhs.sign = 1.0;
  s.cp.n_local = s.n_plane;
  handoff_fill(p, c);
}

// a_ij and b_i into the block's ha / hb, in T
template <typename T>
inline void disc_fill_tableau(T (*ha)[kDiscMaxStages], T* hb, const mi_ode_tableau& tb, int S) {
  for (int i = 1; i < S; ++i)
    for (int j = 0; j < i; ++j) ha[i][j] = (T)tb.beta[i - 1][j];
  for (int i = 0; i < S; ++i) hb[i] = (T)tb.c_sol[i];
}

// alpha as the quotient the forward step functions divide by: 1/3 -> h 1 / 3, 2/3 -> h 2 / 3, 1/2 -> h 1 / 2, 1 -> h 1 / 1 (exact);
// any other alpha: h alpha / 1 (documented in mi_ode.h: the tableaus of the four supported methods take the branches above)
template <typename T>
inline void stage_quotient(double alpha, T* num, T* den) {
  for (int dn = 1; dn <= 3; ++dn) {
    const double v = alpha * dn;
    if (fabs(v - nearbyint(v)) < 1e-12) { *num = (T)nearbyint(v); *den = (T)dn; return; }
  }
  *num = (T)alpha; *den = (T)1;
}

// stage i is evaluated at t[n] + (h tn[i]) / tdn[i] (stage 0 at t[n])
template <typename T>
inline void disc_fill_stage_times(T* tn, T* tdn, const mi_ode_tableau& tb, int S) {
  tn[0] = (T)0; tdn[0] = (T)1;
  for (int i = 1; i < S; ++i) stage_quotient(tb.alpha[i - 1], &tn[i], &tdn[i]);
}

inline int disc_no_pre() { return 0; }

// The argument block to the device, `pre` (launches that go between the copy and the sweep; non-zero: its return code ends the call), the
// sweep kernel, the synchronise - the kernel's last act was the zero-copy store of its result record - and the record to *r.
template <class Pre = int (*)()>
inline int disc_run(DiscHost& c, const void* fn, hipStream_t st, const char* what, DiscResult* r, Pre pre = disc_no_pre) {
  MI_HIP(hipMemcpyAsync(c.args_dev, c.args_host, c.args_bytes, hipMemcpyHostToDevice, st));
  const int prc = pre();
  if (prc != 0) return prc;
  const void* dev_args = c.args_dev;
  void* args[] = {(void*)&dev_args};
  hipError_t e = hipLaunchKernel(fn, dim3((unsigned)c.grid), dim3((unsigned)c.block), args, c.lds, st);
  if (e != hipSuccess) { mi_set_error("%s kernel launch failed: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  MI_HIP(hipStreamSynchronize(st));
  *r = *c.res;
  handoff_advance(c, (unsigned)r->handoffs + 16u);
  for (int i = 0; i < 3; ++i) c.prof_us[i] = 0.01 * (double)r->prof[i];
  return 0;
}

inline void disc_stats(mi_ode_stats* stats, int n_steps, int64_t nfe, double t0, unsigned status) {
  if (stats == nullptr) return;
  memset(stats, 0, sizeof(*stats));
  stats->n_attempts = stats->n_accepted = n_steps;
  stats->nfe = nfe;
  stats->t = t0; stats->status = status;
  stats->n_polls = 1; stats->n_launches = 1;
}

}  // namespace mi
