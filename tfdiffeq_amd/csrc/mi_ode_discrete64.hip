// Host side of the float64 fused reverse sweep of a fixed-grid solve (include/mi_ode.h section A''''-64, csrc/mi_ode_discrete64.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_discrete64.h"

using namespace mi;

struct mi_ode_discrete64 {
  mi_ode_discrete_desc d;
  int dp, hp;                  // padded widths of the kernel instantiation: (16, 16) or (64, 128)
  int S;                       // stages
  int td;                      // 1: time-dependent first layer - theta starts with w_t [hidden]
  int P, SL, PP;               // parameters, slice of the fold per workgroup, doubles of a partial block
  int pack_doubles;
  int grid, block, chunk;
  size_t lds;
  const void* fn[3];           // the kernel for each hidden activation (mi_ode_rhs.scalars[0])
  long long ntiles;
  double *act, *wpart, *pack, *pack_t;
  double* partials;            // hand-off records (2 parities)
  DiscResult* res;             // pinned host
  Disc64Args* args_host;       // pinned staging of the kernel's argument block ...
  Disc64Args* args_dev;        // ... and its device copy
  unsigned seq;
  int spin_limit, spin_first;
  double prof_us[3];
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
  h->lds = DiscGeom64<DP, HP>::lds_bytes();
  h->block = 64 * MlpGeom64<DP, HP>::NW;
  h->PP = DiscGeom64<DP, HP>::PP;
  h->pack_doubles = MlpGeom64<DP, HP>::PACK;
  for (int act = 0; act < 3; ++act) h->fn[act] = disc64_fn<DP, HP>(act);
}
template <int DP, int HP>
int disc64_pack(const mi_ode_discrete64* h, const RhsParams& rhs, hipStream_t st) {
  const dim3 grid((MlpGeom64<DP, HP>::PACK + 255) / 256), block(256);
  hipLaunchKernelGGL((k_mlp64_pack<DP, HP>), grid, block, 0, st, rhs, (int)h->d.dim, h->pack);
  hipLaunchKernelGGL((k_mlp64_pack_t<DP, HP>), grid, block, 0, st, rhs, (int)h->d.dim, h->pack_t);
  return hipGetLastError() == hipSuccess ? 0 : MI_ODE_E_HIP;
}
// alpha as the quotient the forward step functions divide by (stage_quotient of the float32 sweep, in double)
void stage_quotient64(double alpha, double* num, double* den) {
  for (int dn = 1; dn <= 3; ++dn) {
    const double v = alpha * dn;
    if (fabs(v - nearbyint(v)) < 1e-12) { *num = nearbyint(v); *den = (double)dn; return; }
  }
  *num = alpha; *den = 1.0;
}
}  // namespace

extern "C" int mi_ode_discrete64_destroy(mi_ode_discrete64_handle h) {
  if (h == nullptr) return 0;
  if (h->act) (void)hipFree(h->act);
  if (h->wpart) (void)hipFree(h->wpart);
  if (h->pack) (void)hipFree(h->pack);
  if (h->pack_t) (void)hipFree(h->pack_t);
  if (h->partials) (void)hipFree(h->partials);
  if (h->res) (void)hipHostFree(h->res);
  if (h->args_host) (void)hipHostFree(h->args_host);
  if (h->args_dev) (void)hipFree(h->args_dev);
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
  // a tableau of n_stages rows has n_stages + 1 stages; c_sol carries b
  if (tb.n_stages < 0 || tb.n_stages + 1 > kDiscMaxStages) {
    mi_set_error("fused float64 discrete sweep: explicit Runge-Kutta tableaus of at most %d stages", kDiscMaxStages); return MI_ODE_E_INVALID;
  }
  if (desc->n_points < 2 || desc->n_points - 1 > kDiscMaxSteps) {
    mi_set_error("fused float64 discrete sweep: 2 <= n_points <= %d", kDiscMaxSteps + 1); return MI_ODE_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  mi_ode_discrete64* h = new mi_ode_discrete64();
  memset(h, 0, sizeof(*h));
  h->d = *desc;
  h->S = tb.n_stages + 1;
  h->td = time_dependent;
  // the two geometries of the float64 forward (mi_ode_launch_mlp64.hip)
  if (desc->dim <= 16 && desc->hidden <= 16) { h->dp = 16; h->hp = 16; disc64_geom<16, 16>(h); }
  else { h->dp = 64; h->hp = 128; disc64_geom<64, 128>(h); }
  const int d = desc->dim, hd = desc->hidden;
  h->P = h->td * hd + d * hd + hd + hd * hd + hd + hd * d + d;
  h->ntiles = (desc->batch + 31) / 32;
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e0 = hipGetDevice(&dev);
  if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e0 != hipSuccess) {
    mi_set_error("fused float64 discrete sweep: %s", hipGetErrorString(e0));
    (void)hipGetLastError();
    mi_ode_discrete64_destroy(h);
    return MI_ODE_E_HIP;
  }
  for (int act = 0; act < 3; ++act)
    if (hipFuncSetAttribute(h->fn[act], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) (void)hipGetLastError();
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->fn[0], h->block, h->lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    mi_set_error("fused float64 discrete sweep kernel does not fit a compute unit (LDS %zu bytes, %d threads)", h->lds, h->block);
    mi_ode_discrete64_destroy(h); return MI_ODE_E_HIP;
  }
  long long g = h->ntiles;                       // every workgroup co-resident (the final hand-off spins): at most one per CU
  if (g > cus) g = cus;
  if (g > kPersistMaxGrid) g = kPersistMaxGrid;
  h->grid = (int)g;
  h->SL = (h->P + h->grid - 1) / h->grid;
  const long long per_wg = (h->ntiles + h->grid - 1) / h->grid;
  const size_t slot_doubles = (size_t)32 * (2 * (size_t)h->dp + 4 * (size_t)h->hp);
  // chunk_tiles == 0: all of a workgroup's tiles per weight-gradient pass, as far as 1 GiB of activation scratch goes (4 slots per
  // tile: 640 KB at 64 x 128, i.e. 6 tiles per workgroup on 256 CUs), chunks of that size beyond - the rule of the float32 sweep
  long long chunk = desc->chunk_tiles > 0 ? desc->chunk_tiles : per_wg;
  if (desc->chunk_tiles <= 0) {
    const long long fit = (long long)(((size_t)1 << 30) / ((size_t)h->grid * kDiscMaxStages * slot_doubles * sizeof(double)));
    if (chunk > fit) chunk = fit < 1 ? 1 : fit;
  }
  if (chunk > per_wg) chunk = per_wg;
  h->chunk = (int)chunk;
  hipError_t e = hipMalloc((void**)&h->act, (size_t)h->grid * (size_t)h->chunk * kDiscMaxStages * slot_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wpart, (size_t)h->grid * (size_t)h->PP * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->pack, (size_t)h->pack_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->pack_t, (size_t)h->pack_doubles * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->partials, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->res, sizeof(DiscResult), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->args_host, sizeof(Disc64Args), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&h->args_dev, sizeof(Disc64Args));
  if (e == hipSuccess) e = hipMemset(h->partials, 0, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e != hipSuccess) {
    mi_set_error("fused float64 discrete sweep workspace: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    mi_ode_discrete64_destroy(h);
    return MI_ODE_E_HIP;
  }
  memset(h->res, 0, sizeof(DiscResult));
  h->seq = 0;
  h->spin_limit = 1 << 22;                       // the final hand-off absorbs the skew of a whole sweep: a bound, not a time-out to hit
  h->spin_first = 1 << 14;                       // residency check (the first hand-off is the kernel's first act)
  if (const char* e3 = getenv("MI_ODE_PERSIST_SPIN_FIRST")) h->spin_first = atoi(e3);
  if (const char* e2 = getenv("MI_ODE_PERSIST_SPIN_LIMIT")) h->spin_limit = atoi(e2);
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
  MI_HIP(hipStreamSynchronize(st));              // the pinned argument block may still be in flight from a previous call
  Disc64Args& D = *h->args_host;
  memset(&D, 0, sizeof(D));
  StepArgs& S = D.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  S.batch = h->d.batch; S.dim = h->d.dim; S.n_plane = h->d.batch * (long long)h->d.dim;
  S.partials = h->partials;
  for (int i = 0; i < 8; ++i) S.rhs.s[i] = rhs->scalars[i];
  for (int i = 0; i < 3; ++i) { S.rhs.w[i] = rhs->w[i]; S.rhs.b[i] = rhs->b[i]; }
  S.rhs.sign = 1.0;
  S.rhs.hidden = rhs->hidden;
  S.cp.n_local = S.n_plane;
  D.p.world = 1;
  D.p.seq_base = h->seq;
  D.p.spin_limit = h->spin_limit;
  D.p.spin_first = h->spin_first < h->spin_limit ? h->spin_first : h->spin_limit;
  D.p.sleep_first = h->grid <= 32 ? 16 : 32; D.p.sleep_poll = 2;
  D.ys = (const double*)ys_dev; D.gys = (const double*)grad_ys_dev; D.lam = (double*)grad_y0_out_dev; D.th_out = (double*)grad_theta_out_dev;
  D.pack = h->pack; D.pack_t = h->pack_t; D.act = h->act; D.wpart = h->wpart;
  D.res = h->res;
  D.N = h->d.n_points; D.S = h->S; D.chunk = h->chunk; D.td = h->td;
  D.P = h->P; D.SL = h->SL;
  for (int i = 1; i < h->S; ++i)
    for (int j = 0; j < i; ++j) D.ha[i][j] = tb.beta[i - 1][j];
  for (int i = 0; i < h->S; ++i) D.hb[i] = tb.c_sol[i];
  D.tn[0] = 0.0; D.tdn[0] = 1.0;
  for (int i = 1; i < h->S; ++i) stage_quotient64(tb.alpha[i - 1], &D.tn[i], &D.tdn[i]);
  for (int n = 0; n + 1 < D.N; ++n) {                      // solvers.py:84: the grid in the state dtype
    D.t0[n] = t_host[n];
    D.h[n] = t_host[n + 1] - t_host[n];
  }
  MI_HIP(hipMemcpyAsync(h->args_dev, h->args_host, sizeof(Disc64Args), hipMemcpyHostToDevice, st));
  // this call's weights -> the two packs, on the stream in front of the sweep (as the float64 forward does)
  const int prc = h->dp == 16 ? disc64_pack<16, 16>(h, S.rhs, st) : disc64_pack<64, 128>(h, S.rhs, st);
  if (prc != 0) { mi_set_error("fused float64 discrete sweep: the weight pack launches failed"); return prc; }
  const Disc64Args* dev_args = h->args_dev;
  void* args[] = {(void*)&dev_args};
  hipError_t e = hipLaunchKernel(h->fn[act], dim3((unsigned)h->grid), dim3((unsigned)h->block), args, h->lds, st);
  if (e != hipSuccess) { mi_set_error("fused float64 discrete sweep kernel launch failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  MI_HIP(hipStreamSynchronize(st));              // the kernel's last act was the zero-copy store of its result record
  const DiscResult r = *h->res;
  h->seq += (unsigned)r.handoffs + 16u;
  if (h->seq >= 0xE0000000u) h->seq = 0;
  for (int i = 0; i < 3; ++i) h->prof_us[i] = 0.01 * (double)r.prof[i];
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete64 prof] steps %d  grid %d  chunk %d  us: tile passes %.1f  weight-gradient passes %.1f  hand-off + fold %.1f\n",
            D.N - 1, h->grid, h->chunk, h->prof_us[0], h->prof_us[1], h->prof_us[2]);
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_attempts = stats->n_accepted = D.N - 1;
    stats->nfe = (int64_t)(D.N - 1) * h->S;
    stats->t = t_host[0]; stats->status = r.status;
    stats->n_polls = 1; stats->n_launches = 1;   // the sweep kernel; the two pack launches in front of it are not counted (float64 forward family)
  }
  return (int)r.status;
}

extern "C" int mi_ode_discrete64_profile(mi_ode_discrete64_handle h, double* out3) {
  if (h == nullptr || out3 == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  for (int i = 0; i < 3; ++i) out3[i] = h->prof_us[i];
  return 0;
}
