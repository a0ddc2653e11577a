// Host side and instantiations of per-trajectory step control for the ODEFunc MLP (include/mi_ode.h: mi_ode_integrate_rows_mlp;
// csrc/mi_ode_rows_mlp.h): k_rows_mlp per padded width, tableau and hidden activation - a translation unit of its own so that these
// large kernels compile in parallel with the others.  One launch per call, no co-residency requirement.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_rows_mlp.h"

using namespace mi;

namespace {

template <int DP, int HP, int ACT>
const void* rows_mlp_fn_act(const mi_ode_solver* h) {
  if (h->S == 6) return h->ts_dense ? (const void*)k_rows_mlp<DP, HP, ACT, 6, true> : (const void*)k_rows_mlp<DP, HP, ACT, 6, false>;
  if (h->S == 3 && !h->ts_dense) return (const void*)k_rows_mlp<DP, HP, ACT, 3, false>;
  return nullptr;
}
template <int DP, int HP>
const void* rows_mlp_fn(const mi_ode_solver* h, size_t* lds, int* block) {
  *lds = MlpGeom<DP, HP>::lds_bytes(); *block = 64 * MlpGeom<DP, HP>::NW;
  switch ((int)h->rhs.s[0]) {                                 // mi_ode_rhs.scalars[0]: 0 tanh, 1 relu, 2 softplus
    case MLP_ACT_TANH: return rows_mlp_fn_act<DP, HP, MLP_ACT_TANH>(h);
    case MLP_ACT_RELU: return rows_mlp_fn_act<DP, HP, MLP_ACT_RELU>(h);
    case MLP_ACT_SOFTPLUS: return rows_mlp_fn_act<DP, HP, MLP_ACT_SOFTPLUS>(h);
    default: return nullptr;
  }
}
const void* rows_mlp_fn_any(const mi_ode_solver* h, size_t* lds, int* block) {
  if (h->mlp_dp == 16 && h->mlp_hp == 16) return rows_mlp_fn<16, 16>(h, lds, block);
  if (h->mlp_dp == 16 && h->mlp_hp == 128) return rows_mlp_fn<16, 128>(h, lds, block);
  if (h->mlp_dp == 64 && h->mlp_hp == 16) return rows_mlp_fn<64, 16>(h, lds, block);
  if (h->mlp_dp == 64 && h->mlp_hp == 128) return rows_mlp_fn<64, 128>(h, lds, block);
  return nullptr;
}

}  // namespace

extern "C" int64_t mi_ode_rows_mlp_sizeof(void) { return (int64_t)sizeof(mi_ode_rows_mlp_desc); }

extern "C" int mi_ode_integrate_rows_mlp(mi_ode_handle h, const mi_ode_rows_mlp_desc* desc, const void* y0_dev, const double* t_host, int32_t T,
                                         void* out_dev, int64_t* row_stats_dev, mi_ode_stats* stats, void* stream) {
  if (h == nullptr || desc == nullptr || y0_dev == nullptr || t_host == nullptr || out_dev == nullptr || row_stats_dev == nullptr || T < 1) {
    mi_set_error("bad argument");
    return MI_ODE_E_INVALID;
  }
  if (desc->grid < 0 || desc->reserved != 0) { mi_set_error("per-trajectory MLP: grid >= 0 and reserved = 0 are needed"); return MI_ODE_E_INVALID; }
  if (!h->d.adaptive || h->d.multistep != 0) { mi_set_error("per-trajectory step control: an adaptive Runge-Kutta handle is needed"); return MI_ODE_E_INVALID; }
  if (h->family != FAM_MLP || !h->is_f32) {
    mi_set_error("per-trajectory MLP: a float32 handle of the ODEFunc network inside the tile kernels' box (dim <= 64, hidden <= 128) is needed");
    return MI_ODE_E_INVALID;
  }
  if (h->nseg > 1 || h->d.world_size > 1 || h->d.allgather != nullptr || h->nccl_comm != nullptr) {
    mi_set_error("per-trajectory step control: one state tensor on one rank");
    return MI_ODE_E_INVALID;
  }
  size_t lds = 0; int block = 0;
  const void* fn = h->d.tableau.fsal ? rows_mlp_fn_any(h, &lds, &block) : nullptr;
  if (fn == nullptr) {
    mi_set_error("per-trajectory MLP: no kernel for a %d-row tableau with this dense output (it is instantiated for dopri5, tsit5 and bosh3)", h->S);
    return MI_ODE_E_INVALID;
  }
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
  // a tile per workgroup; more tiles than a few waves of workgroups per CU: the tile loop (no co-residency is needed, the cap only
  // spares launching workgroups that would queue anyway).  desc->grid > 0 clamps it.
  const long long ntiles = (h->d.batch + 31) / 32;
  long long g = ntiles;
  const long long cap = (long long)(h->num_cus > 0 ? h->num_cus : 256) * 8;
  if (g > cap) g = cap;
  if (desc->grid > 0 && g > desc->grid) g = desc->grid;
  if (g < 1) g = 1;
  void* args[] = {(void*)&R};
  hipError_t e = hipLaunchKernel(fn, dim3((unsigned)g), dim3((unsigned)block), args, lds, st);
  if (e != hipSuccess) { mi_set_error("per-trajectory MLP kernel launch failed: %s", hipGetErrorString(e)); return MI_ODE_E_HIP; }
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
