// Host side of the fused reverse sweep of a fixed-grid solve of the linear system (include/mi_ode.h section A'''''', csrc/mi_ode_discrete_linear.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_discrete_linear.h"

using namespace mi;

struct mi_ode_discrete_linear {
  mi_ode_discrete_linear_desc d;
  int D;                       // width of the kernel instantiation
  int S;                       // stages
  int grid, block;
  size_t lds, esz;
  const void* fn;
  void* gpart;                 // [grid][D * D + D] partial blocks
  double* partials;            // hand-off records (2 parities)
  DiscResult* res;             // pinned host
  DiscLinArgs* args_host;      // pinned staging of the kernel's argument block ...
  DiscLinArgs* args_dev;       // ... and its device copy
  unsigned seq;
  int spin_limit, spin_first;
  double prof_us[3];
};

namespace {
template <typename T>
const void* dl_fn(int D, size_t* lds) {
  switch (D) {
    case 16: *lds = discrete_linear_lds_bytes<T, 16>(); return (const void*)k_discrete_linear<T, 16>;
    case 32: *lds = discrete_linear_lds_bytes<T, 32>(); return (const void*)k_discrete_linear<T, 32>;
    case 64: *lds = discrete_linear_lds_bytes<T, 64>(); return (const void*)k_discrete_linear<T, 64>;
    default: *lds = discrete_linear_lds_bytes<T, 128>(); return (const void*)k_discrete_linear<T, 128>;
  }
}
}  // namespace

extern "C" int mi_ode_discrete_linear_destroy(mi_ode_discrete_linear_handle h) {
  if (h == nullptr) return 0;
  if (h->gpart) (void)hipFree(h->gpart);
  if (h->partials) (void)hipFree(h->partials);
  if (h->res) (void)hipHostFree(h->res);
  if (h->args_host) (void)hipHostFree(h->args_host);
  if (h->args_dev) (void)hipFree(h->args_dev);
  delete h;
  return 0;
}

extern "C" int mi_ode_discrete_linear_profile(mi_ode_discrete_linear_handle h, double* out3) {
  if (h == nullptr || out3 == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  for (int i = 0; i < 3; ++i) out3[i] = h->prof_us[i];
  return h->grid;
}

extern "C" int mi_ode_discrete_linear_create(const mi_ode_discrete_linear_desc* desc, mi_ode_discrete_linear_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  const mi_ode_tableau& tb = desc->tableau;
  if (desc->dtype != MI_ODE_F32 && desc->dtype != MI_ODE_F64) { mi_set_error("fused linear sweep: dtype must be MI_ODE_F32 or MI_ODE_F64"); return MI_ODE_E_INVALID; }
  if (desc->batch < 1 || desc->dim < 1 || desc->dim > 128) {
    mi_set_error("fused linear sweep: batch >= 1, 1 <= dim <= 128"); return MI_ODE_E_INVALID;
  }
  // a tableau of n_stages rows has n_stages + 1 stages; c_sol carries b
  if (tb.n_stages < 0 || tb.n_stages + 1 > kDiscMaxStages) {
    mi_set_error("fused linear sweep: explicit Runge-Kutta tableaus of at most %d stages", kDiscMaxStages); return MI_ODE_E_INVALID;
  }
  if (desc->n_points < 2 || desc->n_points - 1 > kDiscMaxSteps) {
    mi_set_error("fused linear sweep: 2 <= n_points <= %d", kDiscMaxSteps + 1); return MI_ODE_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  mi_ode_discrete_linear* h = new mi_ode_discrete_linear();
  memset(h, 0, sizeof(*h));
  h->d = *desc;
  h->S = tb.n_stages + 1;
  h->D = desc->dim <= 16 ? 16 : desc->dim <= 32 ? 32 : desc->dim <= 64 ? 64 : 128;
  h->block = 4 * h->D;
  h->esz = desc->dtype == MI_ODE_F64 ? 8 : 4;
  h->fn = desc->dtype == MI_ODE_F64 ? dl_fn<double>(h->D, &h->lds) : dl_fn<float>(h->D, &h->lds);
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e0 = hipGetDevice(&dev);
  if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e0 != hipSuccess) {
    mi_set_error("fused linear sweep: %s", hipGetErrorString(e0));
    (void)hipGetLastError();
    mi_ode_discrete_linear_destroy(h);
    return MI_ODE_E_HIP;
  }
  if (hipFuncSetAttribute(h->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) (void)hipGetLastError();
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->fn, h->block, h->lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    mi_set_error("fused linear sweep kernel does not fit a compute unit (LDS %zu bytes, %d threads)", h->lds, h->block);
    mi_ode_discrete_linear_destroy(h); return MI_ODE_E_HIP;
  }
  // Every workgroup co-resident (the hand-offs spin): at most one per CU.  A workgroup per tile, and at least one per 1024 entries of the
  // final fold - a small batch still spreads the fold of dim * dim + dim entries; the extra workgroups own no tile and contribute zeros.
  const long long ntiles = (desc->batch + 15) / 16;
  const long long E = (long long)h->D * h->D + h->D;
  long long g = ntiles;
  if (g < (E + 1023) / 1024) g = (E + 1023) / 1024;
  if (g > cus) g = cus;
  if (g > kPersistMaxGrid) g = kPersistMaxGrid;
  h->grid = (int)g;
  hipError_t e = hipMalloc((void**)&h->gpart, (size_t)h->grid * (size_t)E * h->esz);
  if (e == hipSuccess) e = hipMalloc((void**)&h->partials, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->res, sizeof(DiscResult), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->args_host, sizeof(DiscLinArgs), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&h->args_dev, sizeof(DiscLinArgs));
  if (e == hipSuccess) e = hipMemset(h->partials, 0, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e != hipSuccess) {
    mi_set_error("fused linear sweep workspace: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    mi_ode_discrete_linear_destroy(h);
    return MI_ODE_E_HIP;
  }
  memset(h->res, 0, sizeof(DiscResult));
  h->seq = 0;
  h->spin_limit = 1 << 22;                       // the final hand-off absorbs the skew of a whole sweep: a bound, not a time-out to hit
  h->spin_first = 1 << 14;                       // residency check (the first hand-off comes right after the slices are loaded)
  if (const char* e3 = getenv("MI_ODE_PERSIST_SPIN_FIRST")) h->spin_first = atoi(e3);
  if (const char* e2 = getenv("MI_ODE_PERSIST_SPIN_LIMIT")) h->spin_limit = atoi(e2);
  *out = h;
  return 0;
}

extern "C" int mi_ode_discrete_linear_sweep(mi_ode_discrete_linear_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                                            const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_W_out_dev, void* grad_b_out_dev,
                                            mi_ode_stats* stats, void* stream) {
  if (h == nullptr || t_host == nullptr || ys_dev == nullptr || grad_ys_dev == nullptr || grad_y0_out_dev == nullptr ||
      grad_W_out_dev == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (rhs == nullptr || rhs->kind != MI_ODE_RHS_LINEAR || rhs->w[0] == nullptr) {
    mi_set_error("fused linear sweep: rhs must be the MI_ODE_RHS_LINEAR descriptor (w[0] = W [dim, dim], b[0] = bias or null)"); return MI_ODE_E_INVALID;
  }
  if ((h->d.has_bias != 0) != (rhs->b[0] != nullptr)) {
    mi_set_error("fused linear sweep: the handle was created %s a bias, the descriptor comes %s one", h->d.has_bias ? "with" : "without",
                 rhs->b[0] != nullptr ? "with" : "without");
    return MI_ODE_E_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  MI_HIP(hipStreamSynchronize(st));              // the pinned argument block may still be in flight from a previous call
  DiscLinArgs& A = *h->args_host;
  memset(&A, 0, sizeof(A));
  StepArgs& S = A.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  S.batch = h->d.batch; S.dim = h->d.dim; S.n_plane = h->d.batch * (long long)h->d.dim;
  S.partials = h->partials;
  S.rhs.w[0] = rhs->w[0]; S.rhs.b[0] = rhs->b[0];
  S.rhs.sign = 1.0;
  S.cp.n_local = S.n_plane;
  A.p.world = 1;
  A.p.seq_base = h->seq;
  A.p.spin_limit = h->spin_limit;
  A.p.spin_first = h->spin_first < h->spin_limit ? h->spin_first : h->spin_limit;
  A.p.sleep_first = h->grid <= 32 ? 16 : 32; A.p.sleep_poll = 2;
  A.ys = ys_dev; A.gys = grad_ys_dev; A.lam = grad_y0_out_dev; A.gw = grad_W_out_dev; A.gb = h->d.has_bias ? grad_b_out_dev : nullptr;
  A.gpart = h->gpart; A.res = h->res;
  A.N = h->d.n_points; A.S = h->S; A.has_bias = h->d.has_bias ? 1 : 0;
  for (int i = 1; i < h->S; ++i)
    for (int j = 0; j < i; ++j) A.ha[i][j] = tb.beta[i - 1][j];
  for (int i = 0; i < h->S; ++i) A.hb[i] = tb.c_sol[i];
  const bool f64 = h->d.dtype == MI_ODE_F64;
  for (int n = 0; n + 1 < A.N; ++n)               // solvers.py:84: the grid in the state dtype
    A.h[n] = f64 ? t_host[n + 1] - t_host[n] : (double)((float)t_host[n + 1] - (float)t_host[n]);
  MI_HIP(hipMemcpyAsync(h->args_dev, h->args_host, sizeof(DiscLinArgs), hipMemcpyHostToDevice, st));
  const DiscLinArgs* dev_args = h->args_dev;
  void* args[] = {(void*)&dev_args};
  hipError_t e = hipLaunchKernel(h->fn, dim3((unsigned)h->grid), dim3((unsigned)h->block), args, h->lds, st);
  if (e != hipSuccess) { mi_set_error("fused linear sweep kernel launch failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  MI_HIP(hipStreamSynchronize(st));              // the kernel's last act was the zero-copy store of its result record
  const DiscResult r = *h->res;
  h->seq += (unsigned)r.handoffs + 16u;
  if (h->seq >= 0xE0000000u) h->seq = 0;
  for (int i = 0; i < 3; ++i) h->prof_us[i] = 0.01 * (double)r.prof[i];
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete linear prof] steps %d  grid %d  us: tile sweep %.1f  partial store %.1f  hand-off + fold %.1f\n",
            A.N - 1, h->grid, h->prof_us[0], h->prof_us[1], h->prof_us[2]);
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_attempts = stats->n_accepted = A.N - 1;
    stats->nfe = (int64_t)(A.N - 1) * h->S;
    stats->t = t_host[0]; stats->status = r.status;
    stats->n_polls = 1; stats->n_launches = 1;
  }
  return (int)r.status;
}
