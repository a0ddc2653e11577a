// Host side of the hypersolvers (include/mi_ode.h section D, csrc/mi_ode_hyper.h): validates the descriptor, lays out g's pack,
// and launches the catalogue systems' kernels (instantiated here for the three methods and both dtypes) or a hyper plugin's.
#include <hip/hip_runtime.h>
#include <string.h>
#include "mi_ode_host.h"
#include "mi_ode_hyper.h"
#include "mi_ode_stage_rowlocal.h"

using namespace mi;

namespace {

template <typename T>
int launch_builtin(int kind, bool cube, const HyperArgs& A, hipStream_t st) {
  const bool traj = A.mode == MI_ODE_HYPER_TRAJECTORY;
  switch (kind) {
    case MI_ODE_RHS_LORENZ: return traj ? HyperLaunch<T, RhsLorenz<T>>::traj(&A, st) : HyperLaunch<T, RhsLorenz<T>>::resid(&A, st);
    case MI_ODE_RHS_LOTKA_VOLTERRA:
      return traj ? HyperLaunch<T, RhsLotkaVolterra<T>>::traj(&A, st) : HyperLaunch<T, RhsLotkaVolterra<T>>::resid(&A, st);
    default:
      if (cube) return traj ? HyperLaunch<T, RhsCubic2<T>>::traj(&A, st) : HyperLaunch<T, RhsCubic2<T>>::resid(&A, st);
      return traj ? HyperLaunch<T, RhsLinear2<T>>::traj(&A, st) : HyperLaunch<T, RhsLinear2<T>>::resid(&A, st);
  }
}

int round16(int n) { return (n + 15) / 16 * 16; }

}  // namespace

extern "C" int mi_ode_hyper_run(const mi_ode_hyper* desc, void* stream) {
  if (desc == nullptr) { mi_set_error("null argument"); return MI_ODE_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); mi_set_error("no HIP device"); return MI_ODE_E_NODEVICE; }
  const mi_ode_hyper& d = *desc;
  if (d.dtype != MI_ODE_F32 && d.dtype != MI_ODE_F64) { mi_set_error("hypersolver: bad dtype"); return MI_ODE_E_INVALID; }
  if (d.method < MI_ODE_HYPER_EULER || d.method > MI_ODE_HYPER_HEUN) { mi_set_error("hypersolver: bad method %d", d.method); return MI_ODE_E_INVALID; }
  if (d.mode < MI_ODE_HYPER_TRAJECTORY || d.mode > MI_ODE_HYPER_G_RESIDUALS) { mi_set_error("hypersolver: bad mode %d", d.mode); return MI_ODE_E_INVALID; }
  if (d.mode == MI_ODE_HYPER_RESIDUAL && d.method != MI_ODE_HYPER_EULER) {
    mi_set_error("hypersolver: residual_trajectory exists for HyperEuler only (the reference raises NotImplementedError)");
    return MI_ODE_E_INVALID;
  }
  if (d.batch < 1 || d.dim < 1 || d.T < 2) { mi_set_error("hypersolver: needs batch >= 1, dim >= 1 and T >= 2 (dt = t[1] - t[0])"); return MI_ODE_E_INVALID; }
  if (d.t == nullptr || d.y == nullptr || d.out == nullptr) { mi_set_error("hypersolver: null t / y / out"); return MI_ODE_E_INVALID; }
  const int D = (int)d.dim;
  if (2 * D + 1 > kHypMaxWidth) { mi_set_error("hypersolver: g's input 2 dim + 1 must be <= %d (dim %d)", kHypMaxWidth, D); return MI_ODE_E_INVALID; }
  const bool network = d.mode != MI_ODE_HYPER_RESIDUAL;        // (residual_trajectory does not evaluate g)
  if (network && (d.n_layers < 2 || d.n_layers > kHypMaxLayers)) { mi_set_error("hypersolver: g needs 2 .. %d Linear layers (got %d)", kHypMaxLayers, d.n_layers); return MI_ODE_E_INVALID; }

  HyperArgs A;
  memset(&A, 0, sizeof(A));
  A.t = d.t; A.y = d.y; A.out = d.out; A.batch = d.batch; A.T = d.T; A.dim = D; A.method = d.method; A.mode = d.mode;
  A.n_layers = network ? d.n_layers : 0;
  A.rows = d.mode == MI_ODE_HYPER_RESIDUAL ? (long long)(d.T - 1) * d.batch : (long long)d.T * d.batch;
  int off = 0;
  for (int l = 0; l < A.n_layers; ++l) {
    const mi_ode_hyper_layer& L = d.layers[l];
    const int want_in = l == 0 ? 2 * D + 1 : d.layers[l - 1].out;
    if (L.in != want_in || L.out < 1 || L.out > kHypMaxWidth || (l == d.n_layers - 1 && L.out != D)) {
      mi_set_error("hypersolver: layer %d is Linear(%d, %d); expected in = %d, out <= %d%s", l, L.in, L.out, want_in, kHypMaxWidth,
                   l == d.n_layers - 1 ? " and out = dim" : "");
      return MI_ODE_E_INVALID;
    }
    if (L.w == nullptr || L.act < MI_ODE_HYPER_ACT_NONE || L.act > MI_ODE_HYPER_ACT_SOFTPLUS ||
        (L.act == MI_ODE_HYPER_ACT_PRELU && (L.alpha == nullptr || (L.n_alpha != 1 && L.n_alpha != L.out)))) {
      mi_set_error("hypersolver: layer %d: null weight, unknown activation %d or PReLU without 1 / out weights", l, L.act);
      return MI_ODE_E_INVALID;
    }
    A.in[l] = L.in; A.out_[l] = L.out; A.kp[l] = round16(L.in); A.np[l] = round16(L.out); A.act[l] = L.act;
    A.n_alpha[l] = L.n_alpha; A.slope[l] = L.slope; A.w[l] = L.w; A.b[l] = L.b; A.alpha[l] = L.alpha;
    A.off_w[l] = off; off += A.kp[l] * A.np[l];
    A.off_b[l] = off; off += A.np[l];
    A.off_a[l] = off; off += A.np[l];
  }
  A.pack_elems = off;
  const size_t elt = d.dtype == MI_ODE_F64 ? sizeof(double) : sizeof(float);

  // f
  const mi_ode_rhs& r = d.rhs;
  fill_rhs(A.rhs, r);
  A.rhs.sign = r.sign == 0.0 ? 1.0 : r.sign;
  const mi_ode_hyper_plugin* pl = nullptr;
  switch (r.kind) {
    case MI_ODE_RHS_LORENZ:
      if (D != 3) { mi_set_error("lorenz needs dim 3"); return MI_ODE_E_INVALID; }
      break;
    case MI_ODE_RHS_LOTKA_VOLTERRA:
    case MI_ODE_RHS_LINEAR:
    case MI_ODE_RHS_CUBIC_LINEAR:
      if (D != 2 || (r.kind != MI_ODE_RHS_LOTKA_VOLTERRA && r.b[0] != nullptr)) {
        mi_set_error("hypersolver: the catalogue systems are lorenz (dim 3), lotka_volterra and the bias-free 2 x 2 linear / cubic (dim 2)");
        return MI_ODE_E_INVALID;
      }
      break;
    case MI_ODE_RHS_PLUGIN:
      pl = (const mi_ode_hyper_plugin*)r.plugin;
      if (pl == nullptr || pl->abi != MI_ODE_HYPER_PLUGIN_ABI) {
        mi_set_error("hypersolver: mi_ode_rhs.plugin must be a hyper plugin table (mi_ode_hyper_plugin_get, abi %#x)", MI_ODE_HYPER_PLUGIN_ABI);
        return MI_ODE_E_INVALID;
      }
      if (pl->dtype != d.dtype || pl->dim != D || pl->launch_traj == nullptr || pl->launch_resid == nullptr) {
        mi_set_error("hypersolver plugin is for dtype %d dim %d, the state is dtype %d dim %d", pl->dtype, pl->dim, d.dtype, D);
        return MI_ODE_E_INVALID;
      }
      break;
    default:
      mi_set_error("hypersolver: RHS kind %d is not row-local (no fused hypersolver kernel)", r.kind);
      return MI_ODE_E_INVALID;
  }

  // g's weights: in LDS next to the two activation tiles when they fit, else packed to the workspace first
  int n_launch = 1;
  A.lds_w = (size_t)(2 * kHypRows * kHypLd + off) * elt <= kHypLdsBudget ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (network && !A.lds_w) {
    if ((size_t)off * elt > (size_t)MI_ODE_HYPER_WORKSPACE_BYTES || d.workspace == nullptr) {
      mi_set_error("hypersolver: g's pack (%zu bytes) needs the %d-byte workspace", (size_t)off * elt, MI_ODE_HYPER_WORKSPACE_BYTES);
      return MI_ODE_E_INVALID;
    }
    A.pack = d.workspace;
    const int g = (off + kHypThreads - 1) / kHypThreads;
    if (d.dtype == MI_ODE_F64) hipLaunchKernelGGL((k_hyper_pack<double>), dim3(g < 256 ? g : 256), dim3(kHypThreads), 0, st, A);
    else hipLaunchKernelGGL((k_hyper_pack<float>), dim3(g < 256 ? g : 256), dim3(kHypThreads), 0, st, A);
    n_launch = 2;
  }
  int rc;
  if (pl != nullptr) rc = d.mode == MI_ODE_HYPER_TRAJECTORY ? pl->launch_traj(&A, st) : pl->launch_resid(&A, st);
  else if (d.dtype == MI_ODE_F64) rc = launch_builtin<double>(r.kind, r.kind == MI_ODE_RHS_CUBIC_LINEAR, A, st);
  else rc = launch_builtin<float>(r.kind, r.kind == MI_ODE_RHS_CUBIC_LINEAR, A, st);
  const hipError_t e = hipGetLastError();
  if (rc != 0 || e != hipSuccess) {
    mi_set_error("hypersolver launch failed: %s", e != hipSuccess ? hipGetErrorString(e) : "launcher refused the arguments");
    return rc != 0 ? rc : MI_ODE_E_HIP;
  }
  return n_launch;
}
