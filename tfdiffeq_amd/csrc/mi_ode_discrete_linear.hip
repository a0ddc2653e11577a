// Host side of the fused reverse sweep of a fixed-grid solve of the linear system (include/mi_ode.h section A'''''', csrc/mi_ode_discrete_linear.h).
#include <stdio.h>
#include "mi_ode_discrete_host.h"
#include "mi_ode_discrete_linear.h"

using namespace mi;

static const char kWhat[] = "fused linear sweep";

struct mi_ode_discrete_linear {
  mi_ode_discrete_linear_desc d;
  DiscHost c;
  int D;                       // width of the kernel instantiation
  size_t esz;
  const void* fn;
  void* gpart;                 // [grid][D * D + D] partial blocks
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
  disc_free(h->c);
  delete h;
  return 0;
}

extern "C" int mi_ode_discrete_linear_profile(mi_ode_discrete_linear_handle h, double* out3) {
  if (h == nullptr || out3 == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  for (int i = 0; i < 3; ++i) out3[i] = h->c.prof_us[i];
  return h->c.grid;
}

extern "C" int mi_ode_discrete_linear_create(const mi_ode_discrete_linear_desc* desc, mi_ode_discrete_linear_handle* out) {
  if (desc == nullptr || out == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  *out = nullptr;
  const mi_ode_tableau& tb = desc->tableau;
  if (desc->dtype != MI_ODE_F32 && desc->dtype != MI_ODE_F64) { mi_set_error("fused linear sweep: dtype must be MI_ODE_F32 or MI_ODE_F64"); return MI_ODE_E_INVALID; }
  if (desc->batch < 1 || desc->dim < 1 || desc->dim > 128) {
    mi_set_error("fused linear sweep: batch >= 1, 1 <= dim <= 128"); return MI_ODE_E_INVALID;
  }
  int rc = disc_check_tableau(tb, kWhat);
  if (rc == 0) rc = disc_check_points(desc->n_points, kWhat);
  if (rc != 0) return rc;
  mi_ode_discrete_linear* h = new mi_ode_discrete_linear();
  memset(h, 0, sizeof(*h));
  DiscHost& c = h->c;
  h->d = *desc;
  c.S = tb.n_stages + 1;
  h->D = desc->dim <= 16 ? 16 : desc->dim <= 32 ? 32 : desc->dim <= 64 ? 64 : 128;
  c.block = 4 * h->D;
  h->esz = desc->dtype == MI_ODE_F64 ? 8 : 4;
  h->fn = desc->dtype == MI_ODE_F64 ? dl_fn<double>(h->D, &c.lds) : dl_fn<float>(h->D, &c.lds);
  int cus = 0;
  rc = handoff_device(&h->fn, 1, c.block, c.lds, &cus, kWhat);
  if (rc != 0) { mi_ode_discrete_linear_destroy(h); return rc; }
  c.grid = disc_linear_grid(desc->batch, h->D, cus);
  hipError_t e = hipMalloc((void**)&h->gpart, (size_t)c.grid * ((size_t)h->D * h->D + h->D) * h->esz);
  rc = disc_alloc(c, e, sizeof(DiscLinArgs), kWhat);
  if (rc != 0) { mi_ode_discrete_linear_destroy(h); return rc; }
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
  DiscHost& c = h->c;
  int rc = disc_begin(c, st);
  if (rc != 0) return rc;
  DiscLinArgs& A = *(DiscLinArgs*)c.args_host;
  StepArgs& S = A.p.s;
  disc_fill_persist(A.p, c, h->d.batch, h->d.dim);
  S.rhs.w[0] = rhs->w[0]; S.rhs.b[0] = rhs->b[0];
  A.ys = ys_dev; A.gys = grad_ys_dev; A.lam = grad_y0_out_dev; A.gw = grad_W_out_dev; A.gb = h->d.has_bias ? grad_b_out_dev : nullptr;
  A.gpart = h->gpart; A.res = c.res;
  A.N = h->d.n_points; A.S = c.S; A.has_bias = h->d.has_bias ? 1 : 0;
  disc_fill_tableau(A.ha, A.hb, h->d.tableau, c.S);
  const bool f64 = h->d.dtype == MI_ODE_F64;
  for (int n = 0; n + 1 < A.N; ++n)               // solvers.py:84: the grid in the state dtype
    A.h[n] = f64 ? t_host[n + 1] - t_host[n] : (double)((float)t_host[n + 1] - (float)t_host[n]);
  DiscResult r;
  rc = disc_run(c, h->fn, st, kWhat, &r);
  if (rc != 0) return rc;
  if (getenv("MI_ODE_DISCRETE_PROF") != nullptr)
    fprintf(stderr, "[discrete linear prof] steps %d  grid %d  us: tile sweep %.1f  partial store %.1f  hand-off + fold %.1f\n",
            A.N - 1, c.grid, c.prof_us[0], c.prof_us[1], c.prof_us[2]);
  disc_stats(stats, A.N - 1, (int64_t)(A.N - 1) * c.S, t_host[0], r.status);
  return (int)r.status;
}
