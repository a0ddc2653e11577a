// Host side of the lowered discrete sweep over per-row times and lengths (include/mi_ode.h: mi_ode_discrete_row_sweep_t;
// csrc/mi_ode_discrete_row_t.h): validates the descriptor and calls the kernel through the discrete-t plugin's table - the kernel itself
// is instantiated in the plugin, for its generated functor.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_discrete_row_t.h"

using namespace mi;

extern "C" int64_t mi_ode_discrete_row_t_sizeof(void) { return (int64_t)sizeof(mi_ode_discrete_row_t_desc); }

extern "C" int mi_ode_discrete_row_sweep_t(const mi_ode_discrete_row_t_desc* desc, const mi_ode_rhs* rhs, const void* ys_dev, const void* grad_ys_dev,
                                           void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats, void* stream) {
  if (desc == nullptr || rhs == nullptr || ys_dev == nullptr || grad_ys_dev == nullptr || grad_y0_out_dev == nullptr) {
    mi_set_error("null argument");
    return MI_ODE_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  const mi_ode_discrete_row_t_desc& d = *desc;
  if (d.dtype != MI_ODE_F32 && d.dtype != MI_ODE_F64) { mi_set_error("lowered discrete sweep (per-row times): bad dtype"); return MI_ODE_E_INVALID; }
  if (d.batch < 1 || d.dim < 1 || d.n_times < 1) { mi_set_error("lowered discrete sweep (per-row times): needs batch >= 1, dim >= 1 and T >= 1"); return MI_ODE_E_INVALID; }
  if (d.n_params < 0 || d.n_params > kDiscreteRowMaxParams) {
    mi_set_error("lowered discrete sweep (per-row times): %d trainable elements (the wavefront partials in LDS take up to %d)", d.n_params, kDiscreteRowMaxParams);
    return MI_ODE_E_INVALID;
  }
  if (d.n_params > 0 && grad_theta_out_dev == nullptr) { mi_set_error("lowered discrete sweep (per-row times): null grad_theta_out"); return MI_ODE_E_INVALID; }
  const long long groups = (d.batch + kDiscreteRowThreads - 1) / kDiscreteRowThreads;
  if (d.grid < 1 || d.grid > kDiscreteRowMaxGrid || d.grid > groups) {
    mi_set_error("lowered discrete sweep (per-row times): grid %d outside 1 .. min(%d, %lld groups of %d rows)", d.grid, kDiscreteRowMaxGrid, groups, kDiscreteRowThreads);
    return MI_ODE_E_INVALID;
  }
  if (d.t_dev == nullptr || d.partials_dev == nullptr || d.ticket_dev == nullptr) { mi_set_error("lowered discrete sweep (per-row times): null t / partials / ticket"); return MI_ODE_E_INVALID; }
  const mi_ode_tableau& tb = d.tableau;
  const int S = tb.n_stages + 1;                               // a tableau of n_stages rows has n_stages + 1 stages; c_sol carries b
  if (tb.n_stages < 0 || (S != 1 && S != 4)) {
    mi_set_error("lowered discrete sweep (per-row times): tableaus of 1 or 4 stages (euler, rk4), got %d", S);
    return MI_ODE_E_INVALID;
  }
  const mi_ode_discrete_row_t_plugin* pl = rhs->kind == MI_ODE_RHS_PLUGIN ? (const mi_ode_discrete_row_t_plugin*)rhs->plugin : nullptr;
  if (pl == nullptr || pl->abi != MI_ODE_DISCRETE_T_PLUGIN_ABI) {
    mi_set_error("lowered discrete sweep (per-row times): mi_ode_rhs.plugin must be a discrete-t plugin table (mi_ode_discrete_t_plugin_get, abi %#x)", MI_ODE_DISCRETE_T_PLUGIN_ABI);
    return MI_ODE_E_INVALID;
  }
  if (pl->dtype != d.dtype || pl->dim != d.dim || pl->n_params != d.n_params || pl->launch_sweep == nullptr) {
    mi_set_error("discrete-t plugin is for dtype %d dim %d with %d trainable elements, the call has dtype %d dim %d and %d", pl->dtype, pl->dim,
                 pl->n_params, d.dtype, d.dim, d.n_params);
    return MI_ODE_E_INVALID;
  }
  DiscreteRowTArgs R;
  memset(&R, 0, sizeof(R));
  DiscreteRowArgs& A = R.r;
  A.ys = ys_dev; A.gys = grad_ys_dev; A.gy0 = grad_y0_out_dev; A.gtheta = grad_theta_out_dev;
  A.partials = d.partials_dev; A.ticket = (unsigned*)d.ticket_dev; A.t = nullptr;
  A.batch = d.batch; A.n_points = d.n_times; A.n_params = d.n_params; A.stages = S;
  for (int i = 1; i < S; ++i) {
    A.tb.c[i] = tb.alpha[i - 1];
    for (int j = 0; j < i; ++j) A.tb.a[i][j] = tb.beta[i - 1][j];
  }
  for (int i = 0; i < S; ++i) A.tb.b[i] = tb.c_sol[i];
  fill_rhs(A.rhs, *rhs);
  A.rhs.sign = 1.0;
  R.t = d.t_dev; R.len = (const int*)d.len_dev;
  const int rc = pl->launch_sweep(&R, d.grid, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (rc != 0 || e != hipSuccess) {
    mi_set_error("lowered discrete sweep (per-row times) launch failed: %s", e != hipSuccess ? hipGetErrorString(e) : "launcher refused the arguments");
    return rc != 0 ? rc : MI_ODE_E_HIP;
  }
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_launches = 1;
    stats->n_accepted = stats->n_attempts = d.n_times - 1;     // of the longest row
    stats->nfe = (int64_t)(d.n_times - 1) * S;
  }
  return 0;
}
