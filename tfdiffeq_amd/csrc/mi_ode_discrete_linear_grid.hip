// Host side of the fused reverse sweep of a fixed-grid solve of the linear system on a grid of its own (options['step_size']), without a
// stored trajectory (include/mi_ode.h section A''''''', the GRID = true instantiations of csrc/mi_ode_discrete_linear.h).
#include <stdio.h>
#include "mi_ode_discrete_host.h"
#include "mi_ode_discrete_linear.h"

using namespace mi;

static const char kWhat[] = "fused linear sweep (own grid)";

struct mi_ode_discrete_linear_grid {
  mi_ode_discrete_linear_grid_desc d;
  DiscHost c;
  int D;                       // width of the kernel instantiation
  size_t esz;
  size_t scratch_bytes;        // grid * n_steps * 16 * D elements
  const void* fn;
  void* gpart;                 // [grid][D * D + D] partial blocks
  void* scratch;               // [grid][n_steps][16][D] checkpoints
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
  const int rct = disc_check_tableau(tb, kWhat);
  if (rct != 0) return rct;
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
  disc_free(h->c);
  delete h;
  return 0;
}

extern "C" int64_t mi_ode_discrete_linear_grid_profile(mi_ode_discrete_linear_grid_handle h, double* out3, int64_t* scratch_bytes) {
  if (h == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  if (out3 != nullptr)
    for (int i = 0; i < 3; ++i) out3[i] = h->c.prof_us[i];
  if (scratch_bytes != nullptr) *scratch_bytes = (int64_t)h->scratch_bytes;
  return h->c.grid;
}

extern "C" int mi_ode_discrete_linear_grid_create(const mi_ode_discrete_linear_grid_desc* desc, mi_ode_discrete_linear_grid_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  int rc = mi_ode_discrete_linear_grid_validate(desc, nullptr, nullptr, nullptr);
  if (rc != 0) return rc;
  mi_ode_discrete_linear_grid* h = new mi_ode_discrete_linear_grid();
  memset(h, 0, sizeof(*h));
  DiscHost& c = h->c;
  h->d = *desc;
  c.S = desc->tableau.n_stages + 1;
  h->D = desc->dim <= 16 ? 16 : desc->dim <= 32 ? 32 : desc->dim <= 64 ? 64 : 128;
  c.block = 4 * h->D;
  h->esz = desc->dtype == MI_ODE_F64 ? 8 : 4;
  h->fn = desc->dtype == MI_ODE_F64 ? dlg_fn<double>(h->D, &c.lds) : dlg_fn<float>(h->D, &c.lds);
  int cus = 0;
  rc = handoff_device(&h->fn, 1, c.block, c.lds, &cus, kWhat);
  if (rc != 0) { mi_ode_discrete_linear_grid_destroy(h); return rc; }
  c.grid = disc_linear_grid(desc->batch, h->D, cus);
  h->scratch_bytes = (size_t)c.grid * (size_t)desc->n_steps * 16u * (size_t)h->D * h->esz;
  if (h->scratch_bytes > kScratchMax) {
    mi_set_error("fused linear sweep (own grid): %zu bytes of checkpoint scratch (%d workgroups x %d steps x 16 x %d) are above the bound of %zu",
                 h->scratch_bytes, c.grid, (int)desc->n_steps, h->D, kScratchMax);
    mi_ode_discrete_linear_grid_destroy(h);
    return MI_ODE_E_INVALID;
  }
  hipError_t e = hipMalloc((void**)&h->gpart, (size_t)c.grid * ((size_t)h->D * h->D + h->D) * h->esz);
  if (e == hipSuccess) e = hipMalloc((void**)&h->scratch, h->scratch_bytes);
  rc = disc_alloc(c, e, sizeof(DiscLinGridArgs), kWhat);
  if (rc != 0) { mi_ode_discrete_linear_grid_destroy(h); return rc; }
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
  DiscHost& c = h->c;
  int rc = disc_begin(c, st);
  if (rc != 0) return rc;
  DiscLinGridArgs& G = *(DiscLinGridArgs*)c.args_host;
  DiscLinArgs& A = G.a;
  StepArgs& S = A.p.s;
  const int M = h->d.n_steps, n_out = h->d.n_out;
  disc_fill_persist(A.p, c, h->d.batch, h->d.dim);
  S.rhs.w[0] = rhs->w[0]; S.rhs.b[0] = rhs->b[0];
  A.ys = nullptr; A.gys = nullptr; A.lam = grad_y0_out_dev; A.gw = grad_W_out_dev; A.gb = h->d.has_bias ? grad_b_out_dev : nullptr;
  A.gpart = h->gpart; A.res = c.res;
  A.N = M + 1; A.S = c.S; A.has_bias = h->d.has_bias ? 1 : 0;
  disc_fill_tableau(A.ha, A.hb, h->d.tableau, c.S);
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
  DiscResult r;
  rc = disc_run(c, h->fn, st, kWhat, &r);
  if (rc != 0) return rc;
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete linear (own grid) prof] steps %d  grid %d  us: tile sweep %.1f  partial store %.1f  hand-off + fold %.1f\n",
            M, c.grid, c.prof_us[0], c.prof_us[1], c.prof_us[2]);
  // nfe, phase A: S evaluations for each of M - 1 steps; phase B as the default-grid sweep counts
  disc_stats(stats, M, (int64_t)(M - 1) * c.S + (int64_t)M * c.S, grid_host[0], r.status);
  return (int)r.status;
}
