// Host side of the fused reverse sweep of a fixed-grid solve (include/mi_ode.h section A'''', csrc/mi_ode_discrete.h).
#include <stdio.h>
#include "mi_ode_discrete_host.h"

using namespace mi;

static const char kWhat[] = "fused discrete sweep";

struct mi_ode_discrete {
  mi_ode_discrete_desc d;
  DiscHost c;
  int dp, hp;                  // padded widths of the kernel instantiation
  int td;                      // 1: time-dependent first layer - theta starts with w_t [hidden]
  int P, Ppad, SL;
  int chunk;
  const void* fn[3];           // the kernel for each hidden activation (mi_ode_rhs.scalars[0])
  long long ntiles;
  float *act, *wpart;
};

namespace {
template <int DP, int HP>
const void* disc_fn(int act, size_t* lds, int* block) {
  *lds = DiscLds<DP, HP>::lds_bytes();
  *block = 64 * AdjGeom<DP, HP>::NW;
  switch (act) {
    case MLP_ACT_TANH: return (const void*)k_discrete_mlp<DP, HP, MLP_ACT_TANH>;
    case MLP_ACT_RELU: return (const void*)k_discrete_mlp<DP, HP, MLP_ACT_RELU>;
    case MLP_ACT_SOFTPLUS: return (const void*)k_discrete_mlp<DP, HP, MLP_ACT_SOFTPLUS>;
    default: return nullptr;
  }
}
const void* disc_fn_dims(int dp, int hp, int act, size_t* lds, int* block) {
  if (dp == 16 && hp == 16) return disc_fn<16, 16>(act, lds, block);
  if (dp == 16 && hp == 128) return disc_fn<16, 128>(act, lds, block);
  if (dp == 64 && hp == 16) return disc_fn<64, 16>(act, lds, block);
  return disc_fn<64, 128>(act, lds, block);
}
int pad16(int v, int lo, int hi) { return v <= lo ? lo : hi; }
}  // namespace

extern "C" int mi_ode_discrete_destroy(mi_ode_discrete_handle h) {
  if (h == nullptr) return 0;
  if (h->act) (void)hipFree(h->act);
  if (h->wpart) (void)hipFree(h->wpart);
  disc_free(h->c);
  delete h;
  return 0;
}

extern "C" int64_t mi_ode_discrete_num_params(mi_ode_discrete_handle h) { return h ? (int64_t)h->P : -1; }

extern "C" int mi_ode_discrete_create(const mi_ode_discrete_desc* desc, mi_ode_discrete_handle* out) {
  return mi_ode_discrete_create_td(desc, 0, out);
}

extern "C" int mi_ode_discrete_create_td(const mi_ode_discrete_desc* desc, int32_t time_dependent, mi_ode_discrete_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  if (time_dependent != 0 && time_dependent != 1) { mi_set_error("fused discrete sweep: time_dependent must be 0 or 1"); return MI_ODE_E_INVALID; }
  const mi_ode_tableau& tb = desc->tableau;
  if (desc->batch < 1 || desc->dim < 1 || desc->dim > 64 || desc->hidden < 1 || desc->hidden > 128) {
    mi_set_error("fused discrete sweep: batch >= 1, 1 <= dim <= 64, 1 <= hidden <= 128"); return MI_ODE_E_INVALID;
  }
  int rc = disc_check_tableau(tb, kWhat);
  if (rc == 0) rc = disc_check_points(desc->n_points, kWhat);
  if (rc != 0) return rc;
  mi_ode_discrete* h = new mi_ode_discrete();
  memset(h, 0, sizeof(*h));
  DiscHost& c = h->c;
  h->d = *desc;
  c.S = tb.n_stages + 1;
  h->td = time_dependent;
  h->dp = pad16(desc->dim, 16, 64);
  h->hp = pad16(desc->hidden, 16, 128);
  for (int act = 0; act < 3; ++act) h->fn[act] = disc_fn_dims(h->dp, h->hp, act, &c.lds, &c.block);
  const int d = desc->dim, hd = desc->hidden;
  h->P = h->td * hd + d * hd + hd + hd * hd + hd + hd * d + d;
  h->Ppad = (h->P + 63) / 64 * 64;
  h->ntiles = (desc->batch + 31) / 32;
  int cus = 0;
  rc = handoff_device(h->fn, 3, c.block, c.lds, &cus, kWhat);
  if (rc != 0) { mi_ode_discrete_destroy(h); return rc; }
  c.grid = handoff_cap_grid(h->ntiles, cus);
  h->SL = (h->P + c.grid - 1) / c.grid;
  const long long per_wg = (h->ntiles + c.grid - 1) / c.grid;
  const size_t slot_floats = (size_t)32 * (2 * (size_t)h->dp + 4 * (size_t)h->hp);
  // chunk_tiles == 0: all of a workgroup's tiles per weight-gradient pass (the fastest schedule measured), as far as 1 GiB of activation
  // scratch goes (4 slots per tile: 320 KB at 64 x 128, i.e. 12 tiles per workgroup on 256 CUs - every batch up to 98304 rows)
  long long chunk = desc->chunk_tiles > 0 ? desc->chunk_tiles : per_wg;
  if (desc->chunk_tiles <= 0) {
    const long long fit = (long long)(((size_t)1 << 30) / ((size_t)c.grid * 4 * slot_floats * sizeof(float)));
    if (chunk > fit) chunk = fit < 1 ? 1 : fit;
  }
  if (chunk > per_wg) chunk = per_wg;
  h->chunk = (int)chunk;
  hipError_t e = hipMalloc((void**)&h->act, (size_t)c.grid * (size_t)h->chunk * 4 * slot_floats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wpart, (size_t)c.grid * 3 * (size_t)h->Ppad * sizeof(float));
  rc = disc_alloc(c, e, sizeof(DiscArgs), kWhat);
  if (rc != 0) { mi_ode_discrete_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int mi_ode_discrete_sweep(mi_ode_discrete_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                                     const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats,
                                     void* stream) {
  if (h == nullptr || t_host == nullptr || ys_dev == nullptr || grad_ys_dev == nullptr || grad_y0_out_dev == nullptr ||
      grad_theta_out_dev == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (rhs == nullptr || rhs->kind != MI_ODE_RHS_MLP_TANH || rhs->hidden != h->d.hidden || rhs->w[0] == nullptr || rhs->w[1] == nullptr ||
      rhs->w[2] == nullptr) {
    mi_set_error("fused discrete sweep: rhs must be the MLP descriptor the handle was created for"); return MI_ODE_E_INVALID;
  }
  if ((rhs->scalars[1] != 0.0) != (h->td != 0)) {
    mi_set_error("fused discrete sweep: the handle was created for a time-%s network, rhs->scalars[1] says time-%s",
                 h->td ? "dependent" : "independent", h->td ? "independent" : "dependent");
    return MI_ODE_E_INVALID;
  }
  const int act = (int)rhs->scalars[0];
  if (act < 0 || act > 2) { mi_set_error("fused discrete sweep: unknown activation code %d", act); return MI_ODE_E_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  DiscHost& c = h->c;
  int rc = disc_begin(c, st);
  if (rc != 0) return rc;
  DiscArgs& D = *(DiscArgs*)c.args_host;
  AdjArgs& A = D.a;
  StepArgs& S = A.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  disc_fill_persist(A.p, c, h->d.batch, h->d.dim);
  fill_rhs(S.rhs, *rhs);
  A.act = h->act; A.wpart = h->wpart;
  A.P = h->P; A.Ppad = h->Ppad; A.SL = h->SL; A.td = h->td;
  D.ys = (const float*)ys_dev; D.gys = (const float*)grad_ys_dev; D.lam = (float*)grad_y0_out_dev; D.th_out = (float*)grad_theta_out_dev;
  D.res = c.res;
  D.N = h->d.n_points; D.S = c.S; D.chunk = h->chunk;
  disc_fill_tableau(D.ha, D.hb, tb, c.S);
  disc_fill_stage_times(D.tn, D.tdn, tb, c.S);
  for (int n = 0; n + 1 < D.N; ++n) {                      // solvers.py:84: the grid in the state dtype
    D.t0[n] = (float)t_host[n];
    D.h[n] = (float)t_host[n + 1] - (float)t_host[n];
  }
  DiscResult r;
  rc = disc_run(c, h->fn[act], st, kWhat, &r);
  if (rc != 0) return rc;
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete prof] steps %d  grid %d  chunk %d  us: tile passes %.1f  weight-gradient passes %.1f  hand-off + fold %.1f\n",
            D.N - 1, c.grid, h->chunk, c.prof_us[0], c.prof_us[1], c.prof_us[2]);
  disc_stats(stats, D.N - 1, (int64_t)(D.N - 1) * c.S, t_host[0], r.status);
  return (int)r.status;
}
