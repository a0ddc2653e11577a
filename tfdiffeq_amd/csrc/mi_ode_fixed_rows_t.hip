// Host side of fixed-grid solves with per-row times and lengths (include/mi_ode.h: mi_ode_integrate_fixed_rows_t;
// csrc/mi_ode_fixed_rows_t.h) and the float64 instantiations of k_fixed_rowlocal_t for the catalogue families.  One launch and one
// synchronisation per call, no co-residency requirement; the times stay on the device (nothing of them is read here).
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_fixed_rows_t.h"

using namespace mi;

const void* mi_fixed_rows_t_fn_f64(int family) {
  switch (family) {
    case FAM_CUBIC2: return (const void*)k_fixed_rowlocal_t<double, RhsCubic2<double>>;
    case FAM_LINEAR2: return (const void*)k_fixed_rowlocal_t<double, RhsLinear2<double>>;
    case FAM_LV: return (const void*)k_fixed_rowlocal_t<double, RhsLotkaVolterra<double>>;
    case FAM_LORENZ: return (const void*)k_fixed_rowlocal_t<double, RhsLorenz<double>>;
    default: return nullptr;
  }
}

extern "C" int mi_ode_integrate_fixed_rows_t(mi_ode_handle h, const void* fixed_rows_t_plugin, const void* y0_dev, const double* t_dev, int32_t T,
                                             const int32_t* len_dev, void* out_dev, mi_ode_stats* stats, void* stream) {
  if (h == nullptr || y0_dev == nullptr || t_dev == nullptr || out_dev == nullptr || T < 1) {
    mi_set_error("bad argument");
    return MI_ODE_E_INVALID;
  }
  if (h->d.adaptive || h->d.multistep != 0 || (h->S != 0 && h->S != 3)) {
    mi_set_error("fixed grid with per-row times: a fixed-grid handle with the euler (0 rows) or rk4 3/8 (3 rows) tableau is needed");
    return MI_ODE_E_INVALID;
  }
  if (!(h->family == FAM_CUBIC2 || h->family == FAM_LINEAR2 || h->family == FAM_LV || h->family == FAM_LORENZ || h->family == FAM_PLUGIN)) {
    mi_set_error("fixed grid with per-row times: the right-hand side of this handle is not trajectory-per-thread (matrix-core and cooperative "
                 "families evaluate f with the threads of a workgroup together)");
    return MI_ODE_E_INVALID;
  }
  if (h->nseg > 1 || h->d.world_size > 1 || h->d.allgather != nullptr || h->nccl_comm != nullptr) {
    mi_set_error("fixed grid with per-row times: one state tensor on one rank");
    return MI_ODE_E_INVALID;
  }
  const void* fn = nullptr;
  if (h->family == FAM_PLUGIN) {
    const mi_ode_fixed_rows_t_plugin* pl = (const mi_ode_fixed_rows_t_plugin*)fixed_rows_t_plugin;
    if (pl == nullptr) { mi_set_error("fixed grid with per-row times: a plugin right-hand side needs its fixed-rows-t plugin (mi_ode_fixed_rows_t_plugin_get)"); return MI_ODE_E_INVALID; }
    if (pl->abi != MI_ODE_FIXED_ROWS_T_PLUGIN_ABI || pl->fixed_rows_t_fn == nullptr) { mi_set_error("fixed-rows-t plugin was built against different headers (abi %d vs %d): rebuild it", pl->abi, MI_ODE_FIXED_ROWS_T_PLUGIN_ABI); return MI_ODE_E_INVALID; }
    if (pl->dtype != h->d.dtype || pl->dim != (int)h->d.dim) { mi_set_error("fixed-rows-t plugin is for dtype %d dim %d, the state is dtype %d dim %d", pl->dtype, pl->dim, h->d.dtype, (int)h->d.dim); return MI_ODE_E_INVALID; }
    fn = pl->fixed_rows_t_fn;
  } else {
    fn = h->is_f32 ? mi_fixed_rows_t_fn_f32((int)h->family) : mi_fixed_rows_t_fn_f64((int)h->family);
  }
  if (fn == nullptr) { mi_set_error("fixed grid with per-row times: no kernel for this right-hand side"); return MI_ODE_E_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  h->n_launches = 0; h->n_polls = 0;
  FixedRowsTArgs A;
  memset(&A, 0, sizeof(A));
  A.y0 = y0_dev; A.out = out_dev; A.t = t_dev; A.len = (const int*)len_dev; A.batch = h->d.batch; A.T = T; A.rk4 = h->S == 0 ? 0 : 1; A.rhs = h->rhs;
  long long g = (h->d.batch + 255) / 256;
  if (g < 1) g = 1;
  if (g > (1 << 20)) g = 1 << 20;                            // (the kernel strides over the rows)
  void* args[] = {(void*)&A};
  hipError_t e = hipLaunchKernel(fn, dim3((unsigned)g), dim3(256), args, 0, st);
  if (e != hipSuccess) { mi_set_error("fixed-grid per-row kernel launch failed: %s", hipGetErrorString(e)); return MI_ODE_E_HIP; }
  h->n_launches += 1;
  MI_HIP(hipStreamSynchronize(st));                          // the one synchronisation of the call
  h->n_polls += 1;
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->nfe = (long long)(h->S == 0 ? 1 : 4) * (T - 1);   // of the longest row
    stats->n_attempts = stats->n_accepted = T - 1;
    stats->n_launches = h->n_launches; stats->n_polls = h->n_polls;
  }
  return 0;
}
