// Host side of the convolutional ODE stage (include/mi_ode.h section E, csrc/mi_ode_conv.h): validates the descriptor and launches
// k_conv_stage, instantiated for dtype x activation x time dependence (the stage width n_k is a run-time argument).
#include <hip/hip_runtime.h>
#include <string.h>
#include <mutex>
#include <set>
#include <utility>
#include "mi_ode_host.h"
#include "mi_ode_conv.h"

using namespace mi;

namespace {

template <typename T, int ACT>
const void* conv_kernel(bool td) {
  return td ? (const void*)k_conv_stage<T, ACT, true> : (const void*)k_conv_stage<T, ACT, false>;
}

template <typename T>
const void* conv_kernel(int act, bool td) {
  switch (act) {
    case MI_ODE_CONV_ACT_RELU: return conv_kernel<T, MI_ODE_CONV_ACT_RELU>(td);
    case MI_ODE_CONV_ACT_SOFTPLUS: return conv_kernel<T, MI_ODE_CONV_ACT_SOFTPLUS>(td);
    case MI_ODE_CONV_ACT_TANH: return conv_kernel<T, MI_ODE_CONV_ACT_TANH>(td);
    default: return nullptr;
  }
}

// The dynamic-LDS limit above 64 KB (float64 with F > 64), raised once per kernel and device to the most any call can ask for - not
// on every launch (nor inside a stream capture after the first eager call).
int allow_conv_lds(const void* fn, size_t max_lds) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({fn, dev})) return 0;
  MI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds));
  done.insert({fn, dev});
  return 0;
}

}  // namespace

extern "C" int mi_ode_conv_stage(const mi_ode_conv_desc* desc, const void* y0, const void* const* ks, int32_t n_k, const double* beta_row,
                                 const double* dt_dev, const void* t_dev, void* k_out, void* y_out, void* stream) {
  if (desc == nullptr || y0 == nullptr || k_out == nullptr) { mi_set_error("conv_stage: null descriptor / y0 / k_out"); return MI_ODE_E_INVALID; }
  const mi_ode_conv_desc& d = *desc;
  if (d.dtype != MI_ODE_F32 && d.dtype != MI_ODE_F64) { mi_set_error("conv_stage: bad dtype"); return MI_ODE_E_INVALID; }
  if (d.channels < 1 || d.channels > MI_ODE_CONV_MAX_C || d.filters < 1 || d.filters > MI_ODE_CONV_MAX_F) {
    mi_set_error("conv_stage: needs 1 <= channels <= %d and 1 <= filters <= %d (got %d, %d)", MI_ODE_CONV_MAX_C, MI_ODE_CONV_MAX_F,
                 d.channels, d.filters);
    return MI_ODE_E_INVALID;
  }
  if (d.batch < 1 || d.height < 1 || d.width < 1) { mi_set_error("conv_stage: empty batch / image"); return MI_ODE_E_INVALID; }
  if (n_k < 0 || n_k > MI_ODE_MAX_K || (n_k > 0 && (ks == nullptr || beta_row == nullptr || dt_dev == nullptr))) {
    mi_set_error("conv_stage: bad stage combination (n_k %d)", n_k);
    return MI_ODE_E_INVALID;
  }
  if (d.w1 == nullptr || d.b1 == nullptr || d.w2 == nullptr || d.b2 == nullptr || d.w3 == nullptr || d.b3 == nullptr ||
      (d.time_dependent && (d.w2t == nullptr || t_dev == nullptr))) {
    mi_set_error("conv_stage: null weight / bias / time pointer");
    return MI_ODE_E_INVALID;
  }
  const void* fn = d.dtype == MI_ODE_F64 ? conv_kernel<double>(d.activation, d.time_dependent != 0)
                                         : conv_kernel<float>(d.activation, d.time_dependent != 0);
  if (fn == nullptr) { mi_set_error("conv_stage: bad activation %d", d.activation); return MI_ODE_E_INVALID; }

  ConvArgs A;
  memset(&A, 0, sizeof(A));
  A.y0 = y0;
  A.n_k = n_k;
  for (int j = 0; j < n_k; ++j) {
    if (ks[j] == nullptr) { mi_set_error("conv_stage: null k[%d]", j); return MI_ODE_E_INVALID; }
    A.ks[j] = ks[j];
    A.beta[j] = beta_row[j];
  }
  A.dt = dt_dev; A.t = t_dev; A.k_out = k_out; A.y_out = y_out;
  A.w1 = d.w1; A.b1 = d.b1; A.w2 = d.w2; A.w2t = d.w2t; A.b2 = d.b2; A.w3 = d.w3; A.b3 = d.b3;
  A.sign = d.sign;
  A.C = d.channels; A.H = d.height; A.W = d.width; A.F = d.filters; A.Fp = (d.filters + 15) / 16 * 16;
  A.tiles_x = (d.width + kConvTile - 1) / kConvTile;
  A.n_tiles = A.tiles_x * ((d.height + kConvTile - 1) / kConvTile);
  const long long grid = (long long)A.n_tiles * d.batch;
  if (grid > 0x7fffffffLL) { mi_set_error("conv_stage: batch x tiles exceeds the grid"); return MI_ODE_E_INVALID; }
  const size_t elem = d.dtype == MI_ODE_F64 ? sizeof(double) : sizeof(float);
  const size_t lds = conv_lds_bytes(A.Fp, elem);
  if (lds > 64 * 1024) {
    const int rc = allow_conv_lds(fn, conv_lds_bytes(MI_ODE_CONV_MAX_F, elem));
    if (rc < 0) return rc;
  }
  void* args[] = {(void*)&A};
  MI_HIP(hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kConvThreads), args, lds, (hipStream_t)stream));
  return 0;
}
