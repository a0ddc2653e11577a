// Host side of the fused reverse sweep of a fixed-grid solve of the linear system on a grid of its own (options['step_size']), without a
// stored trajectory (include/mi_ode.h section A''''''', the GRID = true instantiations of csrc/mi_ode_discrete_linear.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_discrete_linear.h"

using namespace mi;

struct mi_ode_discrete_linear_grid {
  mi_ode_discrete_linear_grid_desc d;
  int D;                       // width of the kernel instantiation
  int S;                       // stages
  int grid, block;
  size_t lds, esz;
  size_t scratch_bytes;        // grid * n_steps * 16 * D elements
  const void* fn;
  void* gpart;                 // [grid][D * D + D] partial blocks
  void* scratch;               // [grid][n_steps][16][D] checkpoints
  double* partials;            // hand-off records (2 parities)
  DiscResult* res;             // pinned host
  DiscLinGridArgs* args_host;  // pinned staging of the kernel's argument block ...
  DiscLinGridArgs* args_dev;   // ... and its device copy
  unsigned seq;
  int spin_limit, spin_first;
  double prof_us[3];
};

namespace {
constexpr size_t kScratchMax = (size_t)1 << 30;

template <typename T>
const void* dlg_fn(int D, size_t* lds) {
  switch (D) {
    case 16: *lds = discrete_linear_lds_bytes<T, 16>(); return (const void*)k_discrete_linear<T, 16, true>;
    case 32: *lds = discrete_linear_lds_bytes<T, 32>(); return (const void*)k_discrete_linear<T, 32, true>;
    case 64: *lds = discrete_linear_lds_bytes<T, 64>(); return (const void*)k_discrete_linear<T, 64, true>;
    default: *lds = discrete_linear_lds_bytes<T, 128>(); return (const void*)k_discrete_linear<T, 128, true>;
  }
}
}  // namespace

// Everything that can be said without a device: the descriptor, and - where given - the grid and the assignment of the outputs.
extern "C" int mi_ode_discrete_linear_grid_validate(const mi_ode_discrete_linear_grid_desc* desc, const double* grid_host,
                                                    const int32_t* out_step, const double* out_w) {
  if (desc == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  const mi_ode_tableau& tb = desc->tableau;
  if (desc->dtype != MI_ODE_F32 && desc->dtype != MI_ODE_F64) { mi_set_error("fused linear sweep (own grid): dtype must be MI_ODE_F32 or MI_ODE_F64"); return MI_ODE_E_INVALID; }
  if (desc->batch < 1 || desc->dim < 1 || desc->dim > 128) {
    mi_set_error("fused linear sweep (own grid): batch >= 1, 1 <= dim <= 128"); return MI_ODE_E_INVALID;
  }
  if (tb.n_stages < 0 || tb.n_stages + 1 > kDiscMaxStages) {
    mi_set_error("fused linear sweep (own grid): explicit Runge-Kutta tableaus of at most %d stages", kDiscMaxStages); return MI_ODE_E_INVALID;
  }
  if (desc->n_steps < 1 || desc->n_steps > kDiscMaxSteps) {
    mi_set_error("fused linear sweep (own grid): 1 <= n_steps <= %d", kDiscMaxSteps); return MI_ODE_E_INVALID;
  }
  if (desc->n_out < 2 || desc->n_out > kDiscMaxSteps + 1) {
    mi_set_error("fused linear sweep (own grid): 2 <= n_out <= %d", kDiscMaxSteps + 1); return MI_ODE_E_INVALID;
  }
  if (grid_host != nullptr)
    for (int n = 0; n < desc->n_steps; ++n)
      if (!(grid_host[n + 1] > grid_host[n])) { mi_set_error("fused linear sweep (own grid): the grid must increase strictly"); return MI_ODE_E_INVALID; }
  if (out_step != nullptr) {
    if (out_step[0] != -1) { mi_set_error("fused linear sweep (own grid): out_step[0] must be -1 (output 0 is y0)"); return MI_ODE_E_INVALID; }
    for (int j = 1; j < desc->n_out; ++j) {
      if (out_step[j] < 0 || out_step[j] >= desc->n_steps || out_step[j] < out_step[j - 1]) {
        mi_set_error("fused linear sweep (own grid): out_step[%d] = %d is outside [0, n_steps) or decreases", j, (int)out_step[j]); return MI_ODE_E_INVALID;
      }
    }
  }
  if (out_w != nullptr)
    for (int j = 1; j < desc->n_out; ++j)
      if (!(out_w[j] >= 0.0 && out_w[j] <= 1.0)) { mi_set_error("fused linear sweep (own grid): out_w[%d] = %g is outside [0, 1]", j, out_w[j]); return MI_ODE_E_INVALID; }
  return 0;
}

extern "C" int mi_ode_discrete_linear_grid_destroy(mi_ode_discrete_linear_grid_handle h) {
  if (h == nullptr) return 0;
  if (h->gpart) (void)hipFree(h->gpart);
  if (h->scratch) (void)hipFree(h->scratch);
  if (h->partials) (void)hipFree(h->partials);
  if (h->res) (void)hipHostFree(h->res);
  if (h->args_host) (void)hipHostFree(h->args_host);
  if (h->args_dev) (void)hipFree(h->args_dev);
  delete h;
  return 0;
}

extern "C" int64_t mi_ode_discrete_linear_grid_profile(mi_ode_discrete_linear_grid_handle h, double* out3, int64_t* scratch_bytes) {
  if (h == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (out3 != nullptr)
    for (int i = 0; i < 3; ++i) out3[i] = h->prof_us[i];
  if (scratch_bytes != nullptr) *scratch_bytes = (int64_t)h->scratch_bytes;
  return h->grid;
}

extern "C" int mi_ode_discrete_linear_grid_create(const mi_ode_discrete_linear_grid_desc* desc, mi_ode_discrete_linear_grid_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  const int rc = mi_ode_discrete_linear_grid_validate(desc, nullptr, nullptr, nullptr);
  if (rc != 0) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  mi_ode_discrete_linear_grid* h = new mi_ode_discrete_linear_grid();
  memset(h, 0, sizeof(*h));
  h->d = *desc;
  h->S = desc->tableau.n_stages + 1;
  h->D = desc->dim <= 16 ? 16 : desc->dim <= 32 ? 32 : desc->dim <= 64 ? 64 : 128;
  h->block = 4 * h->D;
  h->esz = desc->dtype == MI_ODE_F64 ? 8 : 4;
  h->fn = desc->dtype == MI_ODE_F64 ? dlg_fn<double>(h->D, &h->lds) : dlg_fn<float>(h->D, &h->lds);
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e0 = hipGetDevice(&dev);
  if (e0 == hipSuccess) e0 = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e0 != hipSuccess) {
    mi_set_error("fused linear sweep (own grid): %s", hipGetErrorString(e0));
    (void)hipGetLastError();
    mi_ode_discrete_linear_grid_destroy(h);
    return MI_ODE_E_HIP;
  }
  if (hipFuncSetAttribute(h->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds) != hipSuccess) (void)hipGetLastError();
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->fn, h->block, h->lds) != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    mi_set_error("fused linear sweep (own grid) kernel does not fit a compute unit (LDS %zu bytes, %d threads)", h->lds, h->block);
    mi_ode_discrete_linear_grid_destroy(h); return MI_ODE_E_HIP;
  }
  // the grid of mi_ode_discrete_linear_create: a workgroup per tile, at least one per 1024 entries of the fold, at most one per CU
  const long long ntiles = (desc->batch + 15) / 16;
  const long long E = (long long)h->D * h->D + h->D;
  long long g = ntiles;
  if (g < (E + 1023) / 1024) g = (E + 1023) / 1024;
  if (g > cus) g = cus;
  if (g > kPersistMaxGrid) g = kPersistMaxGrid;
  h->grid = (int)g;
  h->scratch_bytes = (size_t)h->grid * (size_t)desc->n_steps * 16u * (size_t)h->D * h->esz;
  if (h->scratch_bytes > kScratchMax) {
    mi_set_error("fused linear sweep (own grid): %zu bytes of checkpoint scratch (%d workgroups x %d steps x 16 x %d) are above the bound of %zu",
                 h->scratch_bytes, h->grid, (int)desc->n_steps, h->D, kScratchMax);
    mi_ode_discrete_linear_grid_destroy(h);
    return MI_ODE_E_INVALID;
  }
  hipError_t e = hipMalloc((void**)&h->gpart, (size_t)h->grid * (size_t)E * h->esz);
  if (e == hipSuccess) e = hipMalloc((void**)&h->scratch, h->scratch_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->partials, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->res, sizeof(DiscResult), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->args_host, sizeof(DiscLinGridArgs), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&h->args_dev, sizeof(DiscLinGridArgs));
  if (e == hipSuccess) e = hipMemset(h->partials, 0, (size_t)kMaxBlocks * kRec * sizeof(double));
  if (e != hipSuccess) {
    mi_set_error("fused linear sweep (own grid) workspace: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    mi_ode_discrete_linear_grid_destroy(h);
    return MI_ODE_E_HIP;
  }
  memset(h->res, 0, sizeof(DiscResult));
  h->seq = 0;
  h->spin_limit = 1 << 22;                       // (the values of mi_ode_discrete_linear_create)
  h->spin_first = 1 << 14;
  if (const char* e3 = getenv("MI_ODE_PERSIST_SPIN_FIRST")) h->spin_first = atoi(e3);
  if (const char* e2 = getenv("MI_ODE_PERSIST_SPIN_LIMIT")) h->spin_limit = atoi(e2);
  *out = h;
  return 0;
}

extern "C" int mi_ode_discrete_linear_grid_sweep(mi_ode_discrete_linear_grid_handle h, const mi_ode_rhs* rhs, const double* grid_host,
                                                 const int32_t* out_step, const double* out_w, const void* y0_dev, const void* grad_out_dev,
                                                 void* grad_y0_out_dev, void* grad_W_out_dev, void* grad_b_out_dev, mi_ode_stats* stats,
                                                 void* stream) {
  if (h == nullptr || grid_host == nullptr || out_step == nullptr || out_w == nullptr || y0_dev == nullptr || grad_out_dev == nullptr ||
      grad_y0_out_dev == nullptr || grad_W_out_dev == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (rhs == nullptr || rhs->kind != MI_ODE_RHS_LINEAR || rhs->w[0] == nullptr) {
    mi_set_error("fused linear sweep (own grid): rhs must be the MI_ODE_RHS_LINEAR descriptor (w[0] = W [dim, dim], b[0] = bias or null)"); return MI_ODE_E_INVALID;
  }
  if ((h->d.has_bias != 0) != (rhs->b[0] != nullptr)) {
    mi_set_error("fused linear sweep (own grid): the handle was created %s a bias, the descriptor comes %s one", h->d.has_bias ? "with" : "without",
                 rhs->b[0] != nullptr ? "with" : "without");
    return MI_ODE_E_INVALID;
  }
  if (h->d.has_bias && grad_b_out_dev == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  const int rcv = mi_ode_discrete_linear_grid_validate(&h->d, grid_host, out_step, out_w);
  if (rcv != 0) return rcv;
  hipStream_t st = (hipStream_t)stream;
  MI_HIP(hipStreamSynchronize(st));              // the pinned argument block may still be in flight from a previous call
  DiscLinGridArgs& G = *h->args_host;
  memset(&G, 0, sizeof(G));
  DiscLinArgs& A = G.a;
  StepArgs& S = A.p.s;
  const mi_ode_tableau& tb = h->d.tableau;
  const int M = h->d.n_steps, n_out = h->d.n_out;
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
  A.ys = nullptr; A.gys = nullptr; A.lam = grad_y0_out_dev; A.gw = grad_W_out_dev; A.gb = h->d.has_bias ? grad_b_out_dev : nullptr;
  A.gpart = h->gpart; A.res = h->res;
  A.N = M + 1; A.S = h->S; A.has_bias = h->d.has_bias ? 1 : 0;
  for (int i = 1; i < h->S; ++i)
    for (int j = 0; j < i; ++j) A.ha[i][j] = tb.beta[i - 1][j];
  for (int i = 0; i < h->S; ++i) A.hb[i] = tb.c_sol[i];
  const bool f64 = h->d.dtype == MI_ODE_F64;
  for (int n = 0; n < M; ++n)                    // solvers.py:84: the grid in the state dtype
    A.h[n] = f64 ? grid_host[n + 1] - grid_host[n] : (double)((float)grid_host[n + 1] - (float)grid_host[n]);
  G.y0 = y0_dev; G.gout = grad_out_dev; G.scratch = h->scratch; G.M = M; G.n_out = n_out;
  {
    int j = 1;                                   // out_step is non-decreasing: the outputs of step n are a run of j
    for (int n = 0; n < M; ++n) {
      G.obeg[n] = j;
      while (j < n_out && out_step[j] == n) ++j;
    }
    G.obeg[M] = j;                               // (== n_out: validated above)
  }
  for (int j = 0; j < n_out; ++j) G.ow[j] = f64 ? out_w[j] : (double)(float)out_w[j];
  MI_HIP(hipMemcpyAsync(h->args_dev, h->args_host, sizeof(DiscLinGridArgs), hipMemcpyHostToDevice, st));
  const DiscLinGridArgs* dev_args = h->args_dev;
  void* args[] = {(void*)&dev_args};
  hipError_t e = hipLaunchKernel(h->fn, dim3((unsigned)h->grid), dim3((unsigned)h->block), args, h->lds, st);
  if (e != hipSuccess) { mi_set_error("fused linear sweep (own grid) kernel launch failed: %s", hipGetErrorString(e)); (void)hipGetLastError(); return MI_ODE_E_HIP; }
  MI_HIP(hipStreamSynchronize(st));              // the kernel's last act was the zero-copy store of its result record
  const DiscResult r = *h->res;
  h->seq += (unsigned)r.handoffs + 16u;
  if (h->seq >= 0xE0000000u) h->seq = 0;
  for (int i = 0; i < 3; ++i) h->prof_us[i] = 0.01 * (double)r.prof[i];
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete linear (own grid) prof] steps %d  grid %d  us: tile sweep %.1f  partial store %.1f  hand-off + fold %.1f\n",
            M, h->grid, h->prof_us[0], h->prof_us[1], h->prof_us[2]);
  if (stats != nullptr) {
    memset(stats, 0, sizeof(*stats));
    stats->n_attempts = stats->n_accepted = M;
    stats->nfe = (int64_t)(M - 1) * h->S + (int64_t)M * h->S;      // phase A: S evaluations for each of M - 1 steps; phase B as the default-grid sweep counts
    stats->t = grid_host[0]; stats->status = r.status;
    stats->n_polls = 1; stats->n_launches = 1;
  }
  return (int)r.status;
}
