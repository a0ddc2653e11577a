// Host side of per-trajectory step control with per-row times, lengths and tolerances (include/mi_ode.h: mi_ode_integrate_rows_t;
// csrc/mi_ode_rows_t.h) and the float64 instantiations of k_rows_rowlocal_t for the catalogue families.  One launch and one
// synchronisation per call, no co-residency requirement; the times stay on the device (nothing of them is read here).
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_rows_t.h"

using namespace mi;

const void* mi_rows_t_fn_f64(int family, int S, int ts_dense, int fsal) {
  switch (family) {
    case FAM_CUBIC2: return RowsTKernels<double, RhsCubic2<double>>::fn(S, ts_dense, fsal);
    case FAM_LINEAR2: return RowsTKernels<double, RhsLinear2<double>>::fn(S, ts_dense, fsal);
    case FAM_LV: return RowsTKernels<double, RhsLotkaVolterra<double>>::fn(S, ts_dense, fsal);
    case FAM_LORENZ: return RowsTKernels<double, RhsLorenz<double>>::fn(S, ts_dense, fsal);
    default: return nullptr;
  }
}

namespace {

// tableau, right-hand side and controller parameters of the handle, as mi_ode_integrate_rows hands them to its kernel
void rows_t_step_args(mi_ode_solver* h, StepArgs& A) {
  memset(&A, 0, sizeof(A));
  A.ctl = h->ctl; A.planes = h->planes; A.stride = h->stride; A.batch = h->d.batch; A.dim = (int)h->d.dim;
  A.interp = h->d.interp; A.out = h->cur_out; A.t_out = nullptr; A.n_plane = h->n;
  fill_tableau(A, h->d.tableau, h->S);
  A.partials = h->partials; A.rhs = h->rhs;
  A.ticket = nullptr;
  A.cp = h->cp;
}

bool rows_t_family(const mi_ode_solver* h) {
  return h->family == FAM_CUBIC2 || h->family == FAM_LINEAR2 || h->family == FAM_LV || h->family == FAM_LORENZ || h->family == FAM_PLUGIN;
}

}  // namespace

extern "C" int mi_ode_integrate_rows_t(mi_ode_handle h, const void* rows_t_plugin, const void* y0_dev, const double* t_dev, int32_t T,
                                       const int32_t* len_dev, const double* rtol_dev, const double* atol_dev, void* out_dev,
                                       int64_t* row_stats_dev, mi_ode_stats* stats, void* stream) {
  if (h == nullptr || y0_dev == nullptr || t_dev == nullptr || out_dev == nullptr || row_stats_dev == nullptr || T < 1) {
    mi_set_error("bad argument");
    return MI_ODE_E_INVALID;
  }
  if (!h->d.adaptive || h->d.multistep != 0) { mi_set_error("per-trajectory step control: an adaptive Runge-Kutta handle is needed"); return MI_ODE_E_INVALID; }
  if (!rows_t_family(h)) {
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
    const mi_ode_rows_t_plugin* pl = (const mi_ode_rows_t_plugin*)rows_t_plugin;
    if (pl == nullptr) { mi_set_error("per-trajectory step control: a plugin right-hand side needs its rows-t plugin (mi_ode_rows_t_plugin_get)"); return MI_ODE_E_INVALID; }
    if (pl->abi != MI_ODE_ROWS_T_PLUGIN_ABI || pl->rows_t_fn == nullptr) { mi_set_error("rows-t plugin was built against different headers (abi %d vs %d): rebuild it", pl->abi, MI_ODE_ROWS_T_PLUGIN_ABI); return MI_ODE_E_INVALID; }
    if (pl->dtype != h->d.dtype || pl->dim != (int)h->d.dim) { mi_set_error("rows-t plugin is for dtype %d dim %d, the state is dtype %d dim %d", pl->dtype, pl->dim, h->d.dtype, (int)h->d.dim); return MI_ODE_E_INVALID; }
    fn = pl->rows_t_fn(h->S, h->ts_dense, fsal);
  } else {
    fn = h->is_f32 ? mi_rows_t_fn_f32((int)h->family, h->S, h->ts_dense, fsal) : mi_rows_t_fn_f64((int)h->family, h->S, h->ts_dense, fsal);
  }
  if (fn == nullptr) { mi_set_error("per-trajectory step control: no kernel for a %d-row tableau with this dense output", h->S); return MI_ODE_E_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  h->n_launches = 0; h->n_polls = 0; h->enq_attempts = 0; h->prof_done = 0;
  h->cur_out = (char*)out_dev + (size_t)h->n * h->elt;
  RowsTArgs R;
  memset(&R, 0, sizeof(R));
  PersistArgs& A = R.r.p;
  rows_t_step_args(h, A.s);
  A.s.cp.t_out = nullptr;                      // (every lane points it into its own row of t_dev)
  A.y0 = y0_dev; A.out0 = out_dev; A.n_out = T - 1;
  A.t0 = 0.0;
  A.first_dt = h->cp.auto_first_step ? 0.0 : h->d.first_step;
  A.world = 1; A.nseg = h->nseg;
  R.r.row_stats = (long long*)row_stats_dev;
  R.r.agg = h->ctl;
  R.t = t_dev; R.len = (const int*)len_dev; R.rtol = rtol_dev; R.atol = atol_dev; R.T = T;
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
    stats->status = c->status;                 // (stats->t stays 0: every row ends at a time of its own)
    stats->n_polls = h->n_polls; stats->n_launches = h->n_launches;
  }
  return (int)c->status;
}
