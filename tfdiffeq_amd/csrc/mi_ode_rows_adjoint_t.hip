// Host side of the per-trajectory adjoint with per-row times, lengths and tolerances (include/mi_ode.h: mi_ode_adjoint_rows_t;
// csrc/mi_ode_rows_adjoint_t.h): validates the descriptor and calls the kernel through the rows-adjoint-t plugin's table - the kernel
// itself is instantiated in the plugin, for its generated functor.  One launch for the whole backward; nothing is allocated, nothing of
// the times is read and nothing is waited for here.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_rows_adjoint_t.h"

using namespace mi;

extern "C" int64_t mi_ode_adjoint_rows_t_sizeof(void) { return (int64_t)sizeof(mi_ode_adjoint_rows_t_desc); }

extern "C" int mi_ode_adjoint_rows_t(const mi_ode_adjoint_rows_t_desc* desc, const mi_ode_rhs* rhs, const void* ans_dev, const void* grad_ans_dev,
                                     void* grad_y0_out_dev, void* grad_params_out_dev, mi_ode_stats* stats, void* stream) {
  if (desc == nullptr || rhs == nullptr || ans_dev == nullptr || grad_ans_dev == nullptr || grad_y0_out_dev == nullptr ||
      grad_params_out_dev == nullptr) {
    mi_set_error("null argument");
    return MI_ODE_E_INVALID;
  }
  const mi_ode_adjoint_rows_t_desc& d = *desc;
  if (d.dtype != MI_ODE_F32 && d.dtype != MI_ODE_F64) { mi_set_error("per-trajectory adjoint: bad dtype"); return MI_ODE_E_INVALID; }
  if (d.batch < 1 || d.dim < 1 || d.n_times < 1 || d.n_params < 0) {
    mi_set_error("per-trajectory adjoint: needs batch >= 1, dim >= 1, at least one output time and n_params >= 0");
    return MI_ODE_E_INVALID;
  }
  const int n_aug = 2 * d.dim + 1 + (d.n_params > 0 ? d.n_params : 1);
  if (n_aug > kRowsAdjMaxAug) {
    mi_set_error("per-trajectory adjoint: an augmented state of %d elements per row (2 dim + 1 + n_params <= %d)", n_aug, kRowsAdjMaxAug);
    return MI_ODE_E_INVALID;
  }
  if (d.neg_t_dev == nullptr || d.partials_dev == nullptr || d.ticket_dev == nullptr || d.row_params_dev == nullptr || d.row_time_vjps_dev == nullptr ||
      d.row_counts_dev == nullptr || d.row_status_dev == nullptr) {
    mi_set_error("per-trajectory adjoint: null neg_t / partials / ticket / per-row output");
    return MI_ODE_E_INVALID;
  }
  const mi_ode_tableau& tb = d.tableau;
  const int S = tb.n_stages;
  if (!tb.fsal || (S != 6 && S != 3)) {
    mi_set_error("per-trajectory adjoint: the FSAL shaped 6-row (dopri5) and 3-row (bosh3) tableaus, got %d rows", S);
    return MI_ODE_E_INVALID;
  }
  if (!(d.rtol >= 0.0) || !(d.atol >= 0.0) || !(d.safety > 0.0) || !(d.ifactor > 0.0) || !(d.dfactor > 0.0)) {
    mi_set_error("per-trajectory adjoint: bad controller parameters");
    return MI_ODE_E_INVALID;
  }
  const mi_ode_rows_adjoint_t_plugin* pl = rhs->kind == MI_ODE_RHS_PLUGIN ? (const mi_ode_rows_adjoint_t_plugin*)rhs->plugin : nullptr;
  if (pl == nullptr || pl->abi != MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI) {
    mi_set_error("per-trajectory adjoint: mi_ode_rhs.plugin must be a rows-adjoint-t plugin table (mi_ode_rows_adjoint_t_plugin_get, abi %#x)",
                 MI_ODE_ROWS_ADJOINT_T_PLUGIN_ABI);
    return MI_ODE_E_INVALID;
  }
  if (pl->dtype != d.dtype || pl->dim != d.dim || pl->n_params != d.n_params || pl->launch == nullptr) {
    mi_set_error("rows-adjoint-t plugin is for dtype %d dim %d with %d trainable elements, the call has dtype %d dim %d and %d", pl->dtype, pl->dim,
                 pl->n_params, d.dtype, d.dim, d.n_params);
    return MI_ODE_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  const long long groups = (d.batch + kRowsAdjThreads - 1) / kRowsAdjThreads;
  if (groups > 2147483647LL) { mi_set_error("per-trajectory adjoint: batch too large"); return MI_ODE_E_INVALID; }
  RowsAdjTArgs R;
  memset(&R, 0, sizeof(R));
  RowsAdjArgs& A = R.a;
  StepArgs& s = A.s;
  s.batch = d.batch; s.dim = d.dim; s.n_plane = d.batch * d.dim; s.interp = MI_ODE_INTERP_QUARTIC_MID;
  fill_tableau(s, tb, S);
  fill_rhs(s.rhs, *rhs);
  s.rhs.sign = 1.0;                                          // (the kernel reverses time itself)
  fill_ctrl(s.cp, d, d.dim, d.dtype == MI_ODE_F32 ? 1 : 0, S);   // (cp.t_out stays null: set per interval, by the row)
  A.ans = ans_dev; A.g = grad_ans_dev; A.grad_y0 = grad_y0_out_dev;
  A.row_params = d.row_params_dev; A.row_tvjp = d.row_time_vjps_dev; A.row_counts = (long long*)d.row_counts_dev;
  A.row_status = (long long*)d.row_status_dev;
  A.grad_params = grad_params_out_dev; A.grad_t = nullptr;   // (the time gradient is the rows' own: row_time_vjps_dev)
  A.partials = d.partials_dev; A.ticket = (unsigned*)d.ticket_dev; A.neg_t = d.neg_t_dev;
  A.batch = d.batch; A.n_t = d.n_times;
  R.len = (const int*)d.len_dev; R.rtol = d.rtol_dev; R.atol = d.atol_dev;
  const int rc = pl->launch(&R, S, (int)groups, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (rc != 0 || e != hipSuccess) {
    mi_set_error("per-trajectory adjoint launch failed: %s", e != hipSuccess ? hipGetErrorString(e) : "launcher refused the arguments");
    return rc != 0 ? rc : MI_ODE_E_HIP;
  }
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_launches = 1;
  }
  return 0;
}
