// Host side of the fused reverse sweep of a fixed-grid solve (include/mi_ode.h section A'''', csrc/mi_ode_discrete.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_discrete.h"

using namespace mi;

struct mi_ode_discrete {
  mi_ode_discrete_desc d;
  int dp, hp;                  // padded widths of the kernel instantiation
  int S;                       // stages
  int td;                      // 1: time-dependent first layer - theta starts with w_t [hidden]
  int P, Ppad, SL;
  int grid, block, chunk;
  size_t lds;
  const void* fn[3];           // the kernel for each hidden activation (mi_ode_rhs.scalars[0])
  long long ntiles;
  float *act, *wpart;
  double* partials;            // hand-off records (2 parities)
  DiscResult* res;             // pinned host
  DiscArgs* args_host;         // pinned staging of the kernel's argument block ...
  DiscArgs* args_dev;          // ... and its device copy (the kernel and its non-inlined passes read it with scalar loads)
  unsigned seq;
  int spin_limit, spin_first;
  double prof_us[3];
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
// alpha as the quotient the forward step functions divide by: 1/3 -> h 1 / 3, 2/3 -> h 2 / 3, 1/2 -> h 1 / 2, 1 -> h 1 / 1 (exact);
// any other alpha: h alpha / 1 (documented in mi_ode.h: the tableaus of the four supported methods take the branches above)
void stage_quotient(double alpha, float* num, float* den) {
  for (int dn = 1; dn <= 3; ++dn) {
    const double v = alpha * dn;
    if (fabs(v - nearbyint(v)) < 1e-12) { *num = (float)nearbyint(v); *den = (float)dn; return; }
  }
  *num = (float)alpha; *den = 1.f;
}
}  // namespace

extern "C" int mi_ode_discrete_destroy(mi_ode_discrete_handle h) {
  if (h == nullptr) return 0;
  if (h->act) (void)hipFree(h->act);
  if (h->wpart) (void)hipFree(h->wpart);
  if (h->partials) (void)hipFree(h->partials);
  if (h->res) (void)hipHostFree(h->res);
  if (h->args_host) (void)hipHostFree(h->args_host);
  if (h->args_dev) (void)hipFree(h->args_dev);
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
  // a tableau of n_stages rows has n_stages + 1 stages; c_sol carries b
  if (tb.n_stages < 0 || tb.n_stages + 1 > kDiscMaxStages) {
    mi_set_error("fused discrete sweep: explicit Runge-Kutta tableaus of at most %d stages", kDiscMaxStages); return MI_ODE_E_INVALID;
  }
  if (desc->n_points < 2 || desc->n_points - 1 > kDiscMaxSteps) {
    mi_set_error("fused discrete sweep: 2 <= n_points <= %d", kDiscMaxSteps + 1); return MI_ODE_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  mi_ode_discrete* h = new mi_ode_discrete();
  memset(h, 0, sizeof(*h));
  h->d = *desc;
  h->S = tb.n_stages + 1;
  h->td = time_dependent;
  h->dp = pad16(desc->dim, 16, 64);
  h->hp = pad16(desc->hidden, 16, 128);
  for (int act = 0; act < 3; ++act) h->fn[act] = disc_fn_dims(h->dp, h->hp, act, &h->lds, &h->block);
  const int d = desc->dim, hd = desc->hidden;
  h->P = h->td * hd + d * hd + hd + hd * hd + hd + hd * d + d;
  h->Ppad = (h->P + 63) / 64 * 64;
  h->ntiles = (desc->batch + 31) / 32;
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e0 = hipGetDevice(&dev);
  if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e0 != hipSuccess) {
    mi_set_error("fused discrete sweep: %s", hipGetErrorString(e0));
    (void)hipGetLastError();
    mi_ode_discrete_destroy(h);
    return MI_ODE_E_HIP;
  }
  for (int act = 0; act < 3; ++act)
    if (hipFuncSetAttribute(h->fn[act], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) (void)hipGetLastError();
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->fn[0], h->block, h->lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    mi_set_error("fused discrete sweep kernel does not fit a compute unit (LDS %zu bytes, %d threads)", h->lds, h->block);
    mi_ode_discrete_destroy(h); return MI_ODE_E_HIP;
  }
  long long g = h->ntiles;                       // every workgroup co-resident (the final hand-off spins): at most one per CU
  if (g > cus) g = cus;
  if (g > kPersistMaxGrid) g = kPersistMaxGrid;
  h->grid = (int)g;
  h->SL = (h->P + h->grid - 1) / h->grid;
  const long long per_wg = (h->ntiles + h->grid - 1) / h->grid;
  const size_t slot_floats = (size_t)32 * (2 * (size_t)h->dp + 4 * (size_t)h->hp);
  // chunk_tiles == 0: all of a workgroup's tiles per weight-gradient pass (the fastest schedule measured), as far as 1 GiB of activation
  // scratch goes (4 slots per tile: 320 KB at 64 x 128, i.e. 12 tiles per workgroup on 256 CUs - every batch up to 98304 rows)
  long long chunk = desc->chunk_tiles > 0 ? desc->chunk_tiles : per_wg;
  if (desc->chunk_tiles <= 0) {
    const long long fit = (long long)(((size_t)1 << 30) / ((size_t)h->grid * 4 * slot_floats * sizeof(float)));
    if (chunk > fit) chunk = fit < 1 ? 1 : fit;
  }
  if (chunk > per_wg) chunk = per_wg;
  h->chunk = (int)chunk;
  hipError_t e = hipMalloc((void**)&h->act, (size_t)h->grid * (size_t)h->chunk * 4 * slot_floats * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wpart, (size_t)h->grid * 3 * (size_t)h->Ppad * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->partials, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->res, sizeof(DiscResult), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->args_host, sizeof(DiscArgs), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&h->args_dev, sizeof(DiscArgs));
  if (e == hipSuccess) e = hipMemset(h->partials, 0, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e != hipSuccess) {
    mi_set_error("fused discrete sweep workspace: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    mi_ode_discrete_destroy(h);
    return MI_ODE_E_HIP;
  }
  memset(h->res, 0, sizeof(DiscResult));
  h->seq = 0;
  h->spin_limit = 1 << 22;                       // the final hand-off absorbs the skew of a whole sweep (tiles are dealt round-robin: at most one
                                                 // tile of every step): a bound, not a time-out to hit
  h->spin_first = 1 << 14;                       // residency check (the first hand-off comes right after the weights are staged)
  if (const char* e3 = getenv("MI_ODE_PERSIST_SPIN_FIRST")) h->spin_first = atoi(e3);
  if (const char* e2 = getenv("MI_ODE_PERSIST_SPIN_LIMIT")) h->spin_limit = atoi(e2);
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
  MI_HIP(hipStreamSynchronize(st));              // the pinned argument block may still be in flight from a previous call
  DiscArgs& D = *h->args_host;
  memset(&D, 0, sizeof(D));
  AdjArgs& A = D.a;
  StepArgs& S = A.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  S.batch = h->d.batch; S.dim = h->d.dim; S.n_plane = h->d.batch * (long long)h->d.dim;
  S.partials = h->partials;
  for (int i = 0; i < 8; ++i) S.rhs.s[i] = rhs->scalars[i];
  for (int i = 0; i < 3; ++i) { S.rhs.w[i] = rhs->w[i]; S.rhs.b[i] = rhs->b[i]; }
  S.rhs.sign = 1.0;
  S.rhs.hidden = rhs->hidden;
  S.cp.n_local = S.n_plane;
  A.p.world = 1;
  A.p.seq_base = h->seq;
  A.p.spin_limit = h->spin_limit;
  A.p.spin_first = h->spin_first < h->spin_limit ? h->spin_first : h->spin_limit;
  A.p.sleep_first = h->grid <= 32 ? 16 : 32; A.p.sleep_poll = 2;
  A.act = h->act; A.wpart = h->wpart;
  A.P = h->P; A.Ppad = h->Ppad; A.SL = h->SL; A.td = h->td;
  D.ys = (const float*)ys_dev; D.gys = (const float*)grad_ys_dev; D.lam = (float*)grad_y0_out_dev; D.th_out = (float*)grad_theta_out_dev;
  D.res = h->res;
  D.N = h->d.n_points; D.S = h->S; D.chunk = h->chunk;
  for (int i = 1; i < h->S; ++i)
    for (int j = 0; j < i; ++j) D.ha[i][j] = (float)tb.beta[i - 1][j];
  for (int i = 0; i < h->S; ++i) D.hb[i] = (float)tb.c_sol[i];
  D.tn[0] = 0.f; D.tdn[0] = 1.f;
  for (int i = 1; i < h->S; ++i) stage_quotient(tb.alpha[i - 1], &D.tn[i], &D.tdn[i]);
  for (int n = 0; n + 1 < D.N; ++n) {                      // solvers.py:84: the grid in the state dtype
    D.t0[n] = (float)t_host[n];
    D.h[n] = (float)t_host[n + 1] - (float)t_host[n];
  }
  MI_HIP(hipMemcpyAsync(h->args_dev, h->args_host, sizeof(DiscArgs), hipMemcpyHostToDevice, st));
  const DiscArgs* dev_args = h->args_dev;
  void* args[] = {(void*)&dev_args};
  hipError_t e = hipLaunchKernel(h->fn[act], dim3((unsigned)h->grid), dim3((unsigned)h->block), args, h->lds, st);
  if (e != hipSuccess) { mi_set_error("fused discrete sweep kernel launch failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  MI_HIP(hipStreamSynchronize(st));              // the kernel's last act was the zero-copy store of its result record
  const DiscResult r = *h->res;
  h->seq += (unsigned)r.handoffs + 16u;
  if (h->seq >= 0xE0000000u) h->seq = 0;
  for (int i = 0; i < 3; ++i) h->prof_us[i] = 0.01 * (double)r.prof[i];
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete prof] steps %d  grid %d  chunk %d  us: tile passes %.1f  weight-gradient passes %.1f  hand-off + fold %.1f\n",
            D.N - 1, h->grid, h->chunk, h->prof_us[0], h->prof_us[1], h->prof_us[2]);
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_attempts = stats->n_accepted = D.N - 1;
    stats->nfe = (int64_t)(D.N - 1) * h->S;
    stats->t = t_host[0]; stats->status = r.status;
    stats->n_polls = 1; stats->n_launches = 1;
  }
  return (int)r.status;
}
