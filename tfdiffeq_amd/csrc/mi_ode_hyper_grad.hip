// Host side of the hypersolver gradient (include/mi_ode.h section D', csrc/mi_ode_hyper_grad.h): validates the descriptor, lays out
// g's images, the partial rows and the LDS tiles, packs the images to the workspace when they do not fit in LDS, and calls the kernel
// through the hyper-grad plugin's table - the kernel itself is instantiated in the plugin, for its generated functor.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_hyper_grad.h"

using namespace mi;

namespace {

// the part of the descriptor the layout depends on; 0 or a negative MI_ODE_E_*
int fill_layers(const mi_ode_hyper_grad& d, HyperGradArgs& A) {
  memset(&A, 0, sizeof(A));
  if (d.dtype != MI_ODE_F32 && d.dtype != MI_ODE_F64) { mi_set_error("hypersolver gradient: bad dtype"); return MI_ODE_E_INVALID; }
  if (d.dim < 1 || 2 * d.dim + 1 > kHypMaxWidth) { mi_set_error("hypersolver gradient: g's input 2 dim + 1 must be <= %d", kHypMaxWidth); return MI_ODE_E_INVALID; }
  if (d.n_layers < 2 || d.n_layers > kHypMaxLayers) { mi_set_error("hypersolver gradient: g needs 2 .. %d Linear layers (got %d)", kHypMaxLayers, d.n_layers); return MI_ODE_E_INVALID; }
  const int D = (int)d.dim;
  A.n_layers = d.n_layers;
  A.dim = D;
  for (int l = 0; l < d.n_layers; ++l) {
    const mi_ode_hyper_layer& L = d.layers[l];
    const int want_in = l == 0 ? 2 * D + 1 : d.layers[l - 1].out;
    if (L.in != want_in || L.out < 1 || L.out > kHypMaxWidth || (l == d.n_layers - 1 && L.out != D)) {
      mi_set_error("hypersolver gradient: layer %d is Linear(%d, %d); expected in = %d, out <= %d%s", l, L.in, L.out, want_in, kHypMaxWidth,
                   l == d.n_layers - 1 ? " and out = dim" : "");
      return MI_ODE_E_INVALID;
    }
    if (L.act < MI_ODE_HYPER_ACT_NONE || L.act > MI_ODE_HYPER_ACT_SOFTPLUS || (L.act == MI_ODE_HYPER_ACT_PRELU && L.n_alpha != 1 && L.n_alpha != L.out)) {
      mi_set_error("hypersolver gradient: layer %d: unknown activation %d or PReLU without 1 / out weights", l, L.act);
      return MI_ODE_E_INVALID;
    }
    A.in[l] = L.in; A.out_[l] = L.out; A.act[l] = L.act; A.n_alpha[l] = L.n_alpha; A.slope[l] = L.slope;
    A.w[l] = L.w; A.b[l] = L.b; A.alpha[l] = L.alpha;
    A.gw[l] = d.grad_w[l]; A.gb[l] = d.grad_b[l]; A.ga[l] = L.act == MI_ODE_HYPER_ACT_PRELU ? d.grad_alpha[l] : nullptr;
  }
  hyper_grad_layout(A);
  return 0;
}

size_t elt_of(const mi_ode_hyper_grad& d) { return d.dtype == MI_ODE_F64 ? sizeof(double) : sizeof(float); }

}  // namespace

extern "C" int mi_ode_hyper_grad_sizeof(void) { return (int)sizeof(mi_ode_hyper_grad); }

extern "C" int64_t mi_ode_hyper_grad_tile_bytes(const mi_ode_hyper_grad* desc) {
  if (desc == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  HyperGradArgs A;
  const int rc = fill_layers(*desc, A);
  if (rc != 0) return rc;
  return (int64_t)((size_t)A.act_elems * elt_of(*desc) + 16);
}

extern "C" int64_t mi_ode_hyper_grad_workspace_bytes(const mi_ode_hyper_grad* desc) {
  if (desc == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  HyperGradArgs A;
  const int rc = fill_layers(*desc, A);
  if (rc != 0) return rc;
  if (desc->grid < 1 || desc->grid > kHgMaxGrid) { mi_set_error("hypersolver gradient: grid %d outside 1 .. %d", desc->grid, kHgMaxGrid); return MI_ODE_E_INVALID; }
  return (int64_t)(((size_t)desc->grid * A.pack_elems + A.image_elems) * elt_of(*desc));
}

extern "C" int mi_ode_hyper_grad_run(const mi_ode_hyper_grad* desc, void* stream) {
  if (desc == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  const mi_ode_hyper_grad& d = *desc;
  HyperGradArgs A;
  int rc = fill_layers(d, A);
  if (rc != 0) return rc;
  if (d.method < MI_ODE_HYPER_EULER || d.method > MI_ODE_HYPER_HEUN) { mi_set_error("hypersolver gradient: bad method %d", d.method); return MI_ODE_E_INVALID; }
  if (d.mode != MI_ODE_HYPER_TRAJECTORY && d.mode != MI_ODE_HYPER_G_RESIDUALS) { mi_set_error("hypersolver gradient: mode %d has no parameters to differentiate", d.mode); return MI_ODE_E_INVALID; }
  if (d.batch < 1 || d.T < 2) { mi_set_error("hypersolver gradient: needs batch >= 1 and T >= 2"); return MI_ODE_E_INVALID; }
  if (d.t == nullptr || d.ys == nullptr || d.grad_out == nullptr || d.workspace == nullptr || d.ticket == nullptr) {
    mi_set_error("hypersolver gradient: null t / ys / grad_out / workspace / ticket");
    return MI_ODE_E_INVALID;
  }
  for (int l = 0; l < d.n_layers; ++l) {
    if (d.layers[l].w == nullptr || (d.layers[l].act == MI_ODE_HYPER_ACT_PRELU && d.layers[l].alpha == nullptr)) {
      mi_set_error("hypersolver gradient: layer %d: null weight or PReLU weight", l);
      return MI_ODE_E_INVALID;
    }
    if (A.gw[l] != nullptr || A.gb[l] != nullptr || A.ga[l] != nullptr) A.want_params = 1;
    if (A.gb[l] != nullptr && A.b[l] == nullptr) { mi_set_error("hypersolver gradient: layer %d has no bias to differentiate", l); return MI_ODE_E_INVALID; }
  }
  A.t = d.t; A.ys = d.ys; A.gout = d.grad_out; A.gy = d.mode == MI_ODE_HYPER_TRAJECTORY ? d.grad_y : nullptr;
  A.batch = d.batch; A.T = d.T; A.method = d.method; A.mode = d.mode;
  A.rows = (long long)d.T * d.batch;
  const long long work = d.mode == MI_ODE_HYPER_TRAJECTORY ? d.batch : A.rows;
  const long long tiles = (work + kHypRows - 1) / kHypRows;
  if (d.grid < 1 || d.grid > kHgMaxGrid || d.grid > tiles) {
    mi_set_error("hypersolver gradient: grid %d outside 1 .. min(%d, %lld tiles of %d rows)", d.grid, kHgMaxGrid, tiles, kHypRows);
    return MI_ODE_E_INVALID;
  }
  const size_t elt = elt_of(d);
  const size_t tile_bytes = (size_t)A.act_elems * elt + 16;
  if (tile_bytes > kHgLdsBudget) {
    mi_set_error("hypersolver gradient: g's activation tiles take %zu bytes of LDS (limit %zu)", tile_bytes, kHgLdsBudget);
    return MI_ODE_E_INVALID;
  }
  A.lds_w = tile_bytes + (size_t)A.image_elems * elt <= kHgLdsBudget ? 1 : 0;
  A.partials = d.workspace;
  A.ticket = (unsigned*)d.ticket;

  const mi_ode_rhs& r = d.rhs;
  fill_rhs(A.rhs, r);
  A.rhs.sign = 1.0;
  const mi_ode_hyper_grad_plugin* pl = r.kind == MI_ODE_RHS_PLUGIN ? (const mi_ode_hyper_grad_plugin*)r.plugin : nullptr;
  if (pl == nullptr || pl->abi != MI_ODE_HYPER_GRAD_PLUGIN_ABI || (r.sign != 0.0 && r.sign != 1.0)) {
    mi_set_error("hypersolver gradient: mi_ode_rhs.plugin must be a hyper-grad plugin table (mi_ode_hyper_grad_plugin_get, abi %#x), sign +1", MI_ODE_HYPER_GRAD_PLUGIN_ABI);
    return MI_ODE_E_INVALID;
  }
  if (pl->dtype != d.dtype || pl->dim != d.dim || pl->launch == nullptr) {
    mi_set_error("hyper-grad plugin is for dtype %d dim %d, the state is dtype %d dim %d", pl->dtype, pl->dim, d.dtype, (int)d.dim);
    return MI_ODE_E_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  int n_launch = 1;
  if (!A.lds_w) {
    A.pack = (const char*)d.workspace + (size_t)d.grid * A.pack_elems * elt;
    const int g = (A.image_elems + kHypThreads - 1) / kHypThreads;
    if (d.dtype == MI_ODE_F64) hipLaunchKernelGGL((k_hyper_grad_pack<double>), dim3(g < 256 ? g : 256), dim3(kHypThreads), 0, st, A);
    else hipLaunchKernelGGL((k_hyper_grad_pack<float>), dim3(g < 256 ? g : 256), dim3(kHypThreads), 0, st, A);
    n_launch = 2;
  }
  rc = pl->launch(&A, d.grid, st);
  const hipError_t e = hipGetLastError();
  if (rc != 0 || e != hipSuccess) {
    mi_set_error("hypersolver gradient launch failed: %s", e != hipSuccess ? hipGetErrorString(e) : "launcher refused the arguments");
    return rc != 0 ? rc : MI_ODE_E_HIP;
  }
  return n_launch;
}
