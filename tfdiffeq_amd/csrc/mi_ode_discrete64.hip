// Host side of the float64 fused reverse sweep of a fixed-grid solve (include/mi_ode.h section A''''-64, csrc/mi_ode_discrete64.h).
#include <stdio.h>
#include "mi_ode_discrete_host.h"
#include "mi_ode_discrete64.h"

using namespace mi;

static const char kWhat[] = "fused float64 discrete sweep";

struct mi_ode_discrete64 {
  mi_ode_discrete_desc d;
  DiscHost c;
  int dp, hp;                  // padded widths of the kernel instantiation: (16, 16) or (64, 128)
  int td;                      // 1: time-dependent first layer - theta starts with w_t [hidden]
  int P, SL, PP;               // parameters, slice of the fold per workgroup, doubles of a partial block
  int pack_doubles;
  int chunk;
  const void* fn[3];           // the kernel for each hidden activation (mi_ode_rhs.scalars[0])
  long long ntiles;
  double *act, *wpart, *pack, *pack_t;
};

namespace {
template <int DP, int HP>
const void* disc64_fn(int act) {
  switch (act) {
    case MLP_ACT_TANH: return (const void*)k_discrete_mlp64<DP, HP, MLP_ACT_TANH>;
    case MLP_ACT_RELU: return (const void*)k_discrete_mlp64<DP, HP, MLP_ACT_RELU>;
    case MLP_ACT_SOFTPLUS: return (const void*)k_discrete_mlp64<DP, HP, MLP_ACT_SOFTPLUS>;
    default: return nullptr;
  }
}
template <int DP, int HP>
void disc64_geom(mi_ode_discrete64* h) {
  h->c.lds = DiscGeom64<DP, HP>::lds_bytes();
  h->c.block = 64 * MlpGeom64<DP, HP>::NW;
  h->PP = DiscGeom64<DP, HP>::PP;
  h->pack_doubles = MlpGeom64<DP, HP>::PACK;
  for (int act = 0; act < 3; ++act) h->fn[act] = disc64_fn<DP, HP>(act);
}
template <int DP, int HP>
int disc64_pack(const mi_ode_discrete64* h, const RhsParams& rhs, hipStream_t st) {
  const dim3 grid((MlpGeom64<DP, HP>::PACK + 255) / 256), block(256);
  hipLaunchKernelGGL((k_mlp64_pack<DP, HP>), grid, block, 0, st, rhs, (int)h->d.dim, h->pack);
  hipLaunchKernelGGL((k_mlp64_pack_t<DP, HP>), grid, block, 0, st, rhs, (int)h->d.dim, h->pack_t);
  if (hipGetLastError() == hipSuccess) return 0;
  mi_set_error("%s: the weight pack launches failed", kWhat);
  return MI_ODE_E_HIP;
}
}  // namespace

extern "C" int mi_ode_discrete64_destroy(mi_ode_discrete64_handle h) {
  if (h == nullptr) return 0;
  if (h->act) (void)hipFree(h->act);
  if (h->wpart) (void)hipFree(h->wpart);
  if (h->pack) (void)hipFree(h->pack);
  if (h->pack_t) (void)hipFree(h->pack_t);
  disc_free(h->c);
  delete h;
  return 0;
}

extern "C" int64_t mi_ode_discrete64_num_params(mi_ode_discrete64_handle h) { return h ? (int64_t)h->P : -1; }

extern "C" int mi_ode_discrete64_create(const mi_ode_discrete_desc* desc, int32_t time_dependent, mi_ode_discrete64_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  if (time_dependent != 0 && time_dependent != 1) { mi_set_error("fused float64 discrete sweep: time_dependent must be 0 or 1"); return MI_ODE_E_INVALID; }
  const mi_ode_tableau& tb = desc->tableau;
  if (desc->batch < 1 || desc->dim < 1 || desc->dim > 64 || desc->hidden < 1 || desc->hidden > 128) {
    mi_set_error("fused float64 discrete sweep: batch >= 1, 1 <= dim <= 64, 1 <= hidden <= 128"); return MI_ODE_E_INVALID;
  }
  int rc = disc_check_tableau(tb, kWhat);
  if (rc == 0) rc = disc_check_points(desc->n_points, kWhat);
  if (rc != 0) return rc;
  mi_ode_discrete64* h = new mi_ode_discrete64();
  memset(h, 0, sizeof(*h));
  DiscHost& c = h->c;
  h->d = *desc;
  c.S = tb.n_stages + 1;
  h->td = time_dependent;
  // the two geometries of the float64 forward (mi_ode_launch_mlp64.hip)
  if (desc->dim <= 16 && desc->hidden <= 16) { h->dp = 16; h->hp = 16; disc64_geom<16, 16>(h); }
  else { h->dp = 64; h->hp = 128; disc64_geom<64, 128>(h); }
  const int d = desc->dim, hd = desc->hidden;
  h->P = h->td * hd + d * hd + hd + hd * hd + hd + hd * d + d;
  h->ntiles = (desc->batch + 31) / 32;
  int cus = 0;
  rc = handoff_device(h->fn, 3, c.block, c.lds, &cus, kWhat);
  if (rc != 0) { mi_ode_discrete64_destroy(h); return rc; }
  c.grid = handoff_cap_grid(h->ntiles, cus);
  h->SL = (h->P + c.grid - 1) / c.grid;
  const long long per_wg = (h->ntiles + c.grid - 1) / c.grid;
  const size_t slot_doubles = (size_t)32 * (2 * (size_t)h->dp + 4 * (size_t)h->hp);
  // chunk_tiles == 0: all of a workgroup's tiles per weight-gradient pass, as far as 1 GiB of activation scratch goes (4 slots per
  // tile: 640 KB at 64 x 128, i.e. 6 tiles per workgroup on 256 CUs), chunks of that size beyond - the rule of the float32 sweep
  long long chunk = desc->chunk_tiles > 0 ? desc->chunk_tiles : per_wg;
  if (desc->chunk_tiles <= 0) {
    const long long fit = (long long)(((size_t)1 << 30) / ((size_t)c.grid * kDiscMaxStages * slot_doubles * sizeof(double)));
    if (chunk > fit) chunk = fit < 1 ? 1 : fit;
  }
  if (chunk > per_wg) chunk = per_wg;
  h->chunk = (int)chunk;
  hipError_t e = hipMalloc((void**)&h->act, (size_t)c.grid * (size_t)h->chunk * kDiscMaxStages * slot_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wpart, (size_t)c.grid * (size_t)h->PP * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->pack, (size_t)h->pack_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->pack_t, (size_t)h->pack_doubles * sizeof(double));
  rc = disc_alloc(c, e, sizeof(Disc64Args), kWhat);
  if (rc != 0) { mi_ode_discrete64_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" int mi_ode_discrete64_sweep(mi_ode_discrete64_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                                       const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats,
                                       void* stream) {
  if (h == nullptr || t_host == nullptr || ys_dev == nullptr || grad_ys_dev == nullptr || grad_y0_out_dev == nullptr ||
      grad_theta_out_dev == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (rhs == nullptr || rhs->kind != MI_ODE_RHS_MLP_TANH || rhs->hidden != h->d.hidden || rhs->w[0] == nullptr || rhs->w[1] == nullptr ||
      rhs->w[2] == nullptr) {
    mi_set_error("fused float64 discrete sweep: rhs must be the MLP descriptor the handle was created for"); return MI_ODE_E_INVALID;
  }
  if ((rhs->scalars[1] != 0.0) != (h->td != 0)) {
    mi_set_error("fused float64 discrete sweep: the handle was created for a time-%s network, rhs->scalars[1] says time-%s",
                 h->td ? "dependent" : "independent", h->td ? "independent" : "dependent");
    return MI_ODE_E_INVALID;
  }
  const int act = (int)rhs->scalars[0];
  if (act < 0 || act > 2) { mi_set_error("fused float64 discrete sweep: unknown activation code %d", act); return MI_ODE_E_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  DiscHost& c = h->c;
  int rc = disc_begin(c, st);
  if (rc != 0) return rc;
  Disc64Args& D = *(Disc64Args*)c.args_host;
  StepArgs& S = D.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  disc_fill_persist(D.p, c, h->d.batch, h->d.dim);
  fill_rhs(S.rhs, *rhs);
  D.ys = (const double*)ys_dev; D.gys = (const double*)grad_ys_dev; D.lam = (double*)grad_y0_out_dev; D.th_out = (double*)grad_theta_out_dev;
  D.pack = h->pack; D.pack_t = h->pack_t; D.act = h->act; D.wpart = h->wpart;
  D.res = c.res;
  D.N = h->d.n_points; D.S = c.S; D.chunk = h->chunk; D.td = h->td;
  D.P = h->P; D.SL = h->SL;
  disc_fill_tableau(D.ha, D.hb, tb, c.S);
  disc_fill_stage_times(D.tn, D.tdn, tb, c.S);
  for (int n = 0; n + 1 < D.N; ++n) {                      // solvers.py:84: the grid in the state dtype
    D.t0[n] = t_host[n];
    D.h[n] = t_host[n + 1] - t_host[n];
  }
  DiscResult r;
  // this call's weights -> the two packs, on the stream in front of the sweep (as the float64 forward does)
  rc = disc_run(c, h->fn[act], st, kWhat, &r,
                [&] { return h->dp == 16 ? disc64_pack<16, 16>(h, S.rhs, st) : disc64_pack<64, 128>(h, S.rhs, st); });
  if (rc != 0) return rc;
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete64 prof] steps %d  grid %d  chunk %d  us: tile passes %.1f  weight-gradient passes %.1f  hand-off + fold %.1f\n",
            D.N - 1, c.grid, h->chunk, c.prof_us[0], c.prof_us[1], c.prof_us[2]);
  // n_launches 1: the sweep kernel; the two pack launches in front of it are not counted (float64 forward family)
  disc_stats(stats, D.N - 1, (int64_t)(D.N - 1) * c.S, t_host[0], r.status);
  return (int)r.status;
}

extern "C" int mi_ode_discrete64_profile(mi_ode_discrete64_handle h, double* out3) {
  if (h == nullptr || out3 == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  for (int i = 0; i < 3; ++i) out3[i] = h->c.prof_us[i];
  return 0;
}
