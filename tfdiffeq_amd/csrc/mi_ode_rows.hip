// Host side of per-trajectory step control (include/mi_ode.h: mi_ode_integrate_rows; csrc/mi_ode_rows.h) and the float64
// instantiations of k_rows_rowlocal for the catalogue families.  One launch per call, no co-residency requirement.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_rows.h"

using namespace mi;

const void* mi_rows_fn_f64(int family, int S, int ts_dense, int fsal) {
  switch (family) {
    case FAM_CUBIC2: return RowsKernels<double, RhsCubic2<double>>::fn(S, ts_dense, fsal);
    case FAM_LINEAR2: return RowsKernels<double, RhsLinear2<double>>::fn(S, ts_dense, fsal);
    case FAM_LV: return RowsKernels<double, RhsLotkaVolterra<double>>::fn(S, ts_dense, fsal);
    case FAM_LORENZ: return RowsKernels<double, RhsLorenz<double>>::fn(S, ts_dense, fsal);
    default: return nullptr;
  }
}

// the output times beyond those that travel as kernel arguments: the handle's device / pinned staging arrays, grown on demand
int mi_rows_ensure_t_out(mi_ode_solver* h, int n) {
  if (n > h->t_out_cap) {
    if (h->t_out_dev) (void)hipFree(h->t_out_dev);
    h->t_out_dev = nullptr; h->t_out_cap = 0;
    const int cap = n < 64 ? 64 : n;
    MI_HIP(hipMalloc((void**)&h->t_out_dev, (size_t)cap * sizeof(double)));
    h->t_out_cap = cap;
  }
  if (n > h->t_out_host_cap) {
    if (h->t_out_host) (void)hipHostFree(h->t_out_host);
    h->t_out_host = nullptr; h->t_out_host_cap = 0;
    const int cap = n < 64 ? 64 : n;
    MI_HIP(hipHostMalloc((void**)&h->t_out_host, (size_t)cap * sizeof(double), hipHostMallocDefault));
    h->t_out_host_cap = cap;
  }
  return 0;
}

// tableau, right-hand side and controller parameters of the handle, as the shared kernels get them
void mi_rows_step_args(mi_ode_solver* h, StepArgs& A) {
  memset(&A, 0, sizeof(A));
  A.ctl = h->ctl; A.planes = h->planes; A.stride = h->stride; A.batch = h->d.batch; A.dim = (int)h->d.dim;
  A.interp = h->d.interp; A.out = h->cur_out; A.t_out = h->t_out_dev; A.n_plane = h->n;
  fill_tableau(A, h->d.tableau, h->S);
  A.partials = h->partials; A.rhs = h->rhs;
  A.ticket = nullptr;
  A.cp = h->cp;
}

namespace {

bool rows_family(const mi_ode_solver* h) {
  return h->family == FAM_CUBIC2 || h->family == FAM_LINEAR2 || h->family == FAM_LV || h->family == FAM_LORENZ || h->family == FAM_PLUGIN;
}

}  // namespace

extern "C" int mi_ode_integrate_rows(mi_ode_handle h, const void* rows_plugin, const void* y0_dev, const double* t_host, int32_t T,
                                     void* out_dev, int64_t* row_stats_dev, mi_ode_stats* stats, void* stream) {
  if (h == nullptr || y0_dev == nullptr || t_host == nullptr || out_dev == nullptr || row_stats_dev == nullptr || T < 1) {
    mi_set_error("bad argument");
    return MI_ODE_E_INVALID;
  }
  if (!h->d.adaptive || h->d.multistep != 0) { mi_set_error("per-trajectory step control: an adaptive Runge-Kutta handle is needed"); return MI_ODE_E_INVALID; }
  if (!rows_family(h)) {
    mi_set_error("per-trajectory step control: the right-hand side of this handle is not trajectory-per-thread (matrix-core and cooperative "
                 "families evaluate f with the threads of a workgroup together)");
    return MI_ODE_E_INVALID;
  }
  if (h->nseg > 1 || h->d.world_size > 1 || h->d.allgather != nullptr || h->nccl_comm != nullptr) {
    mi_set_error("per-trajectory step control: one state tensor on one rank");
    return MI_ODE_E_INVALID;
  }
  const int fsal = h->d.tableau.fsal ? 1 : 0;
  const void* fn = nullptr;
  if (h->family == FAM_PLUGIN) {
    const mi_ode_rows_plugin* pl = (const mi_ode_rows_plugin*)rows_plugin;
    if (pl == nullptr) { mi_set_error("per-trajectory step control: a plugin right-hand side needs its rows plugin (mi_ode_rows_plugin_get)"); return MI_ODE_E_INVALID; }
    if (pl->abi != MI_ODE_ROWS_PLUGIN_ABI || pl->rows_fn == nullptr) { mi_set_error("rows plugin was built against different headers (abi %d vs %d): rebuild it", pl->abi, MI_ODE_ROWS_PLUGIN_ABI); return MI_ODE_E_INVALID; }
    if (pl->dtype != h->d.dtype || pl->dim != (int)h->d.dim) { mi_set_error("rows plugin is for dtype %d dim %d, the state is dtype %d dim %d", pl->dtype, pl->dim, h->d.dtype, (int)h->d.dim); return MI_ODE_E_INVALID; }
    fn = pl->rows_fn(h->S, h->ts_dense, fsal);
  } else {
    fn = h->is_f32 ? mi_rows_fn_f32((int)h->family, h->S, h->ts_dense, fsal) : mi_rows_fn_f64((int)h->family, h->S, h->ts_dense, fsal);
  }
  if (fn == nullptr) { mi_set_error("per-trajectory step control: no kernel for a %d-row tableau with this dense output", h->S); return MI_ODE_E_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  for (int i = 1; i < T; ++i)
    if (!(t_host[i] > t_host[i - 1])) {
      if (stats) { memset(stats, 0, sizeof(*stats)); stats->status = MI_ODE_ST_BAD_T; }
      return MI_ODE_ST_BAD_T;                  // _assert_increasing (misc.py:158-159)
    }
  const int n_out = T - 1;
  if (n_out > kPersistTSmall) {
    MI_HIP(hipStreamSynchronize(st));          // the pinned staging buffer may still be in flight from a previous call
    const int rc = mi_rows_ensure_t_out(h, n_out);
    if (rc != 0) return rc;
    memcpy(h->t_out_host, t_host + 1, (size_t)n_out * sizeof(double));
    MI_HIP(hipMemcpyAsync(h->t_out_dev, h->t_out_host, (size_t)n_out * sizeof(double), hipMemcpyHostToDevice, st));
  }
  h->n_launches = 0; h->n_polls = 0; h->enq_attempts = 0; h->prof_done = 0;
  h->cp.t_out = h->t_out_dev;
  h->cur_out = (char*)out_dev + (size_t)h->n * h->elt;
  RowsArgs R;
  memset(&R, 0, sizeof(R));
  PersistArgs& A = R.p;
  mi_rows_step_args(h, A.s);
  A.y0 = y0_dev; A.out0 = out_dev; A.n_out = n_out;
  A.t0 = t_host[0];
  A.first_dt = h->cp.auto_first_step ? 0.0 : h->d.first_step;
  for (int i = 0; i < n_out && i < kPersistTSmall; ++i) A.t_small[i] = t_host[1 + i];
  A.world = 1; A.nseg = h->nseg;
  R.row_stats = (long long*)row_stats_dev;
  R.agg = h->ctl;
  MI_HIP(hipMemsetAsync(h->ctl, 0, sizeof(Ctl), st));
  const long long g = (h->d.batch + 255) / 256;
  void* args[] = {(void*)&R};
  hipError_t e = hipLaunchKernel(fn, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), args, 0, st);
  if (e != hipSuccess) { mi_set_error("per-trajectory kernel launch failed: %s", hipGetErrorString(e)); return MI_ODE_E_HIP; }
  h->n_launches += 1;
  MI_HIP(hipMemcpyAsync(h->ctl_host, h->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
  MI_HIP(hipStreamSynchronize(st));            // the status check: the one synchronisation of the call
  h->n_polls += 1;
  h->begun = 1;
  const Ctl* c = h->ctl_host;
  h->last_call_attempts = c->n_attempt;
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_attempts = c->n_attempt; stats->n_accepted = c->n_accept; stats->n_rejected = c->n_reject; stats->nfe = c->nfe;
    stats->t = t_host[T - 1];
    stats->status = c->status;
    stats->n_polls = h->n_polls; stats->n_launches = h->n_launches;
  }
  return (int)c->status;
}
