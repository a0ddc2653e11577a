// Hypersolvers (tfdiffeq/hyper_solvers/euler.py of the reference): a fixed step of Euler / midpoint / Heun plus a learned correction
// dt^(p+1) * g(cat([y, f(t, y), dt])), g a small dense network.  A trajectory never interacts with another one and there is no
// controller, so a whole `trajectory` call is ONE launch:
//
//   workgroup = 256 threads (4 wavefronts) owning a tile of 16 trajectories; per step
//     lanes 0..15 of wavefront 0   one trajectory each: f through the row-local functor (the RHS type k_fixed_rowlocal takes), the
//                                  row [y, dy, dt, 0 ..] of the tile's input in LDS, the update, the output row
//     all 4 wavefronts             g's layers: a layer's output columns in blocks of 16 spread over the wavefronts, each block a
//                                  chain of v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 over the layer's input (zero padded to a
//                                  multiple of 16), bias + activation + zero padding in the epilogue, written to the other LDS buffer
//   weights    each workgroup copies g's LIVE parameters (torch's [out, in] layout) into LDS once, transposed and zero padded to
//              [Kp][Np], when they fit next to the two activation buffers (the notebook's 7-64-64-64-3 in float64: 82 KB); otherwise
//              k_hyper_pack writes the same image to a device workspace in front of the launch and the chains read it through L2.
//              Either way the parameters are read on every call: an optimizer step between two calls is seen.
//
// k_hyper_resid covers residual_trajectory (HyperEuler: (base[i+1] - base[i] - dt f(t_i, base[i])) / dt^2, no network) and
// _hypersolver_residuals (g at every row of a given trajectory: T * batch independent rows, the tiles of k_hyper_traj).
//
// The update formulas are euler.py's literally (its operation order, no FMA contraction), including its quirks: dt = t[1] - t[0] for
// every step, g sees dt as its time input, row i of the output is the state BEFORE step i, midpoint / Heun scale the second
// correction by dt^3.  g's products are k-ordered fma chains (the matrix cores' own rounding), not numpy's summation order.
// Bound at batch 1: the latency of the dependent MFMA chains and the barriers between layers; at large batches: the matrix pipe.
#pragma once
#include "mi_ode_dev.h"

namespace mi {

constexpr int kHypRows = 16;                   // trajectories per workgroup tile (one 16-row MFMA block)
constexpr int kHypThreads = 256;
constexpr int kHypMaxLayers = MI_ODE_HYPER_MAX_LAYERS;
constexpr int kHypMaxWidth = 128;              // widest layer (input and output), padded
constexpr int kHypLd = kHypMaxWidth + 1;       // LDS row stride of an activation tile: odd, the 16 rows of a column fall in distinct banks
constexpr int kHypMaxGrid = 2048;
constexpr size_t kHypLdsBudget = 160 * 1024;   // LDS per CU on gfx950

struct HyperArgs {
  const void* t;                 // [T], state dtype
  const void* y;                 // trajectory: y0 [batch, dim]; residual modes: the base trajectory [T, batch, dim]
  void* out;                     // trajectory [T, batch, dim]; residual_trajectory [T - 1, batch, dim]; g residuals [T, batch, dim]
  const void* pack;              // the packed weights in global memory (lds_w == 0), else null
  long long batch;
  long long rows;                // rows of the residual modes: (T - 1) * batch or T * batch
  int T, dim, method, mode, n_layers, lds_w;
  int in[kHypMaxLayers], out_[kHypMaxLayers], kp[kHypMaxLayers], np[kHypMaxLayers], act[kHypMaxLayers], n_alpha[kHypMaxLayers];
  double slope[kHypMaxLayers];
  const void* w[kHypMaxLayers];
  const void* b[kHypMaxLayers];
  const void* alpha[kHypMaxLayers];
  int off_w[kHypMaxLayers], off_b[kHypMaxLayers], off_a[kHypMaxLayers];
  int pack_elems;
  RhsParams rhs;
};

// g's parameters -> [Kp][Np] W^T | b [Np] | a [Np] per layer (a: the PReLU weights expanded per channel, or the LeakyReLU slope);
// every padded entry 0.  dst: LDS (the workgroup's copy) or the global workspace (k_hyper_pack).
template <typename T>
__device__ void hyper_pack(const HyperArgs& A, T* dst, int tid, int nt) {
  for (int l = 0; l < A.n_layers; ++l) {
    const T* W = (const T*)A.w[l];
    const T* B = (const T*)A.b[l];
    const T* Al = (const T*)A.alpha[l];
    const int in = A.in[l], out = A.out_[l], np = A.np[l], kp = A.kp[l];
    for (int e = tid; e < kp * np; e += nt) {
      const int k = e / np, c = e - k * np;
      dst[A.off_w[l] + e] = (k < in && c < out) ? W[(long long)c * in + k] : (T)0;
    }
    for (int c = tid; c < np; c += nt) {
      dst[A.off_b[l] + c] = (B != nullptr && c < out) ? B[c] : (T)0;
      T a = (T)0;
      if (A.act[l] == MI_ODE_HYPER_ACT_PRELU && c < out) a = Al[A.n_alpha[l] == 1 ? 0 : c];
      else if (A.act[l] == MI_ODE_HYPER_ACT_LEAKY_RELU) a = (T)A.slope[l];
      dst[A.off_a[l] + c] = a;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_hyper_pack(HyperArgs A) {
  hyper_pack<T>(A, (T*)A.pack, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}

// activations of nn.ReLU / LeakyReLU / PReLU / Tanh / Softplus(beta 1, threshold 20), torch's formulas
template <typename T>
__device__ __forceinline__ T hyper_act(int act, T x, T a) {
  switch (act) {
    case MI_ODE_HYPER_ACT_RELU: return x > (T)0 ? x : (x != x ? x : (T)0);
    case MI_ODE_HYPER_ACT_LEAKY_RELU:
    case MI_ODE_HYPER_ACT_PRELU: return x > (T)0 ? x : a * x;
    case MI_ODE_HYPER_ACT_TANH: return tanh(x);
    case MI_ODE_HYPER_ACT_SOFTPLUS: return x > (T)20 ? x : log1p(exp(x));
    default: return x;
  }
}

template <typename T>
struct HypMfma;
template <>
struct HypMfma<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t step(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }        // f64 C / D layout
};
template <>
struct HypMfma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t step(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};

// g on the tile whose input rows are in `src` (every thread of the workgroup calls it; it ends behind a barrier).  Returns the buffer that
// holds g's output, [16][kHypLd], columns 0 .. dim - 1.  wb: the packed weights (LDS or global).
template <typename T>
__device__ __forceinline__ const T* hyper_g(const HyperArgs& A, const T* wb, T* src, T* dst) {
  using M = HypMfma<T>;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int kr = lane >> 4, cl = lane & 15;
  for (int l = 0; l < A.n_layers; ++l) {
    const int np = A.np[l], ks = A.kp[l] / 4, out = A.out_[l], act = A.act[l];
    const T* W = wb + A.off_w[l];
    for (int cb = wave; cb < np / 16; cb += kHypThreads / 64) {
      typename M::acc_t acc = {(T)0, (T)0, (T)0, (T)0};
      const T* ap = src + cl * kHypLd + kr;                    // A[row cl][k = 4 s + kr]
      const T* bp = W + kr * np + 16 * cb + cl;                // B[k = 4 s + kr][column 16 cb + cl]
      for (int s = 0; s < ks; ++s) acc = M::step(ap[4 * s], bp[(long long)4 * s * np], acc);
      const int col = 16 * cb + cl;
      const T bias = wb[A.off_b[l] + col], a = wb[A.off_a[l] + col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T v = hyper_act<T>(act, acc[r] + bias, a);
        // (the select is redundant for finite rows: the next layer's weight rows out .. Kp - 1 are zero in the pack, so whatever a padded
        // column holds - act(0), e.g. log 2 under Softplus - is multiplied by 0; only a non-finite row's padded columns differ, and its live columns are non-finite already)
        dst[M::row(lane, r) * kHypLd + col] = col < out ? v : (T)0;
      }
    }
    __syncthreads();
    T* tmp = src;
    src = dst;
    dst = tmp;
  }
  return src;
}

// lanes 0..15: the input row [y, dy, dt, 0 ..] of trajectory `r` of the tile
template <typename T, int D>
__device__ __forceinline__ void hyper_put_row(T* x, int kp0, const T* y, const T* dy, T dt) {
#pragma unroll
  for (int d = 0; d < D; ++d) { x[d] = y[d]; x[D + d] = dy[d]; }
  x[2 * D] = dt;
  for (int c = 2 * D + 1; c < kp0; ++c) x[c] = (T)0;
}

template <typename T, class RHS>
__device__ __forceinline__ void hyper_f(const RHS& rhs, T sign, T t, const T* y, T* k) {
  rhs(sign * t, y, k);
#pragma unroll
  for (int d = 0; d < RHS::D; ++d) k[d] = sign * k[d];
}

template <typename T, class RHS, int METHOD>
__device__ void hyper_traj_body(const HyperArgs& A, const T* wb, T* s_a, T* s_b) {
  constexpr int D = RHS::D;
  const RHS rhs(A.rhs);
  const T sign = (T)A.rhs.sign;
  const T* tp = (const T*)A.t;
  const T* y0 = (const T*)A.y;
  T* out = (T*)A.out;
  const T dt = tp[1] - tp[0];                                  // euler.py: dt = t_span[1] - t_span[0] for every step
  const T dt2 = dt * dt, dt3 = dt * dt * dt;
  const int tid = (int)threadIdx.x;
  const long long n = A.batch * D;
  const long long ntiles = (A.batch + kHypRows - 1) / kHypRows;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row = tile * kHypRows + tid;
    const bool owner = tid < kHypRows, live = owner && row < A.batch;
    T* x = s_a + tid * kHypLd;                                 // (owners only)
    T y[D], dy[D], y2[D], dy2[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { y[d] = live ? y0[row * D + d] : (T)0; dy[d] = (T)0; y2[d] = (T)0; dy2[d] = (T)0; }
    for (int i = 0; i < A.T; ++i) {
      if (live) {
#pragma unroll
        for (int d = 0; d < D; ++d) out[(long long)i * n + row * D + d] = y[d];      // row i: the state before step i
      }
      if (i == A.T - 1) break;                                 // (the reference's last update is never written)
      const T t = tp[i];
      if (owner) {
        if (live) hyper_f<T, RHS>(rhs, sign, t, y, dy);
        hyper_put_row<T, D>(x, A.kp[0], y, dy, dt);
      }
      __syncthreads();
      const T* g = hyper_g<T>(A, wb, s_a, s_b) + tid * kHypLd;
      if constexpr (METHOD == MI_ODE_HYPER_EULER) {
        if (owner) {
#pragma unroll
          for (int d = 0; d < D; ++d) y[d] = y[d] + dy[d] * dt + dt2 * g[d];              // euler.py:16
        }
      } else {
        if (owner) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            if constexpr (METHOD == MI_ODE_HYPER_MIDPOINT) y2[d] = y[d] + dy[d] * dt / (T)2 + dt2 * g[d];   // euler.py:46
            else y2[d] = y[d] + dy[d] * dt + dt2 * g[d];                                                     // euler.py:71
          }
          if (live) hyper_f<T, RHS>(rhs, sign, METHOD == MI_ODE_HYPER_MIDPOINT ? t + dt / (T)2 : t + dt, y2, dy2);
          hyper_put_row<T, D>(x, A.kp[0], y2, dy2, dt);
        }
        __syncthreads();
        const T* g2 = hyper_g<T>(A, wb, s_a, s_b) + tid * kHypLd;
        if (owner) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            if constexpr (METHOD == MI_ODE_HYPER_MIDPOINT) y[d] = y[d] + dt * dy2[d] + dt3 * g2[d];                  // euler.py:48
            else y[d] = y[d] + dt / (T)2 * (dy[d] + dy2[d]) + dt3 * g2[d];                                           // euler.py:73
          }
        }
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ T* hyper_smem() {
  extern __shared__ __align__(16) unsigned char hyp_smem[];
  return (T*)hyp_smem;
}

template <typename T, class RHS, int METHOD>
__global__ __launch_bounds__(256) void k_hyper_traj(HyperArgs A) {
  T* s_a = hyper_smem<T>();
  T* s_b = s_a + kHypRows * kHypLd;
  if (A.lds_w) {
    T* s_w = s_b + kHypRows * kHypLd;
    hyper_pack<T>(A, s_w, (int)threadIdx.x, kHypThreads);
    __syncthreads();
    hyper_traj_body<T, RHS, METHOD>(A, s_w, s_a, s_b);
  } else {
    hyper_traj_body<T, RHS, METHOD>(A, (const T*)A.pack, s_a, s_b);
  }
}

// MODE 1 (residual_trajectory, HyperEuler): a thread per row, no network.  MODE 2 (_hypersolver_residuals): the tiles of k_hyper_traj
// over the T * batch rows of the base trajectory.
template <typename T, class RHS, int MODE>
__device__ void hyper_resid_body(const HyperArgs& A, const T* wb, T* s_a, T* s_b) {
  constexpr int D = RHS::D;
  const RHS rhs(A.rhs);
  const T sign = (T)A.rhs.sign;
  const T* tp = (const T*)A.t;
  const T* base = (const T*)A.y;
  T* out = (T*)A.out;
  const T dt = tp[1] - tp[0];
  if constexpr (MODE == MI_ODE_HYPER_RESIDUAL) {
    const T dt2 = dt * dt;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < A.rows; r += (long long)gridDim.x * blockDim.x) {
      const int i = (int)(r / A.batch);
      T y[D], k[D];
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = base[r * D + d];
      hyper_f<T, RHS>(rhs, sign, tp[i], y, k);
#pragma unroll
      for (int d = 0; d < D; ++d) out[r * D + d] = (base[(r + A.batch) * D + d] - y[d] - dt * k[d]) / dt2;   // euler.py:29
    }
  } else {
    const int tid = (int)threadIdx.x;
    const long long ntiles = (A.rows + kHypRows - 1) / kHypRows;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const long long r = tile * kHypRows + tid;
      const bool owner = tid < kHypRows, live = owner && r < A.rows;
      if (owner) {
        T y[D], dy[D];
#pragma unroll
        for (int d = 0; d < D; ++d) { y[d] = live ? base[r * D + d] : (T)0; dy[d] = (T)0; }
        if (live) hyper_f<T, RHS>(rhs, sign, tp[r / A.batch], y, dy);
        hyper_put_row<T, D>(s_a + tid * kHypLd, A.kp[0], y, dy, dt);
      }
      __syncthreads();
      const T* g = hyper_g<T>(A, wb, s_a, s_b) + tid * kHypLd;
      if (live) {
#pragma unroll
        for (int d = 0; d < D; ++d) out[r * D + d] = g[d];
      }
      __syncthreads();                                         // (the owners' next rows overwrite the buffer g was read from)
    }
  }
}

template <typename T, class RHS, int MODE>
__global__ __launch_bounds__(256) void k_hyper_resid(HyperArgs A) {
  if constexpr (MODE == MI_ODE_HYPER_RESIDUAL) {
    hyper_resid_body<T, RHS, MODE>(A, nullptr, nullptr, nullptr);
  } else {
    T* s_a = hyper_smem<T>();
    T* s_b = s_a + kHypRows * kHypLd;
    if (A.lds_w) {
      T* s_w = s_b + kHypRows * kHypLd;
      hyper_pack<T>(A, s_w, (int)threadIdx.x, kHypThreads);
      __syncthreads();
      hyper_resid_body<T, RHS, MODE>(A, s_w, s_a, s_b);
    } else {
      hyper_resid_body<T, RHS, MODE>(A, (const T*)A.pack, s_a, s_b);
    }
  }
}

// dynamic LDS of the network kernels: two activation tiles, plus the weights when they live there
template <typename T>
__host__ __device__ inline size_t hyper_lds_bytes(const HyperArgs& A) {
  return (size_t)(2 * kHypRows * kHypLd + (A.lds_w ? A.pack_elems : 0)) * sizeof(T);
}

template <typename T>
static int hyper_launch_kernel(const void* fn, bool network, long long work, const HyperArgs& A, hipStream_t st) {
  const size_t lds = network ? hyper_lds_bytes<T>(A) : 0;
  if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MI_ODE_E_HIP;
  long long g = network ? (work + kHypRows - 1) / kHypRows : (work + kHypThreads - 1) / kHypThreads;
  if (g < 1) g = 1;
  if (g > kHypMaxGrid) g = kHypMaxGrid;
  void* args[] = {(void*)&A};
  if (hipLaunchKernel(fn, dim3((unsigned)g), dim3(kHypThreads), args, lds, st) != hipSuccess) return MI_ODE_E_HIP;
  return 0;
}

// the launchers the library (catalogue systems) and every hyper plugin (csrc/mi_ode_hyper_plugin.h) instantiate for their functor
template <typename T, class RHS>
struct HyperLaunch {
  static int traj(const HyperArgs* A, hipStream_t st) {
    const void* fn = A->method == MI_ODE_HYPER_EULER ? (const void*)k_hyper_traj<T, RHS, MI_ODE_HYPER_EULER>
                   : A->method == MI_ODE_HYPER_MIDPOINT ? (const void*)k_hyper_traj<T, RHS, MI_ODE_HYPER_MIDPOINT>
                   : A->method == MI_ODE_HYPER_HEUN ? (const void*)k_hyper_traj<T, RHS, MI_ODE_HYPER_HEUN> : nullptr;
    if (fn == nullptr) return MI_ODE_E_INVALID;
    return hyper_launch_kernel<T>(fn, true, A->batch, *A, st);
  }
  static int resid(const HyperArgs* A, hipStream_t st) {
    if (A->mode == MI_ODE_HYPER_RESIDUAL) return hyper_launch_kernel<T>((const void*)k_hyper_resid<T, RHS, MI_ODE_HYPER_RESIDUAL>, false, A->rows, *A, st);
    if (A->mode == MI_ODE_HYPER_G_RESIDUALS) return hyper_launch_kernel<T>((const void*)k_hyper_resid<T, RHS, MI_ODE_HYPER_G_RESIDUALS>, true, A->rows, *A, st);
    return MI_ODE_E_INVALID;
  }
};

}  // namespace mi

// What a hyper plugin's mi_ode_hyper_plugin_get(dtype) returns (a table of its own: the row-local plugin table stays as it is).
#define MI_ODE_HYPER_PLUGIN_ABI 0x48590001
struct mi_ode_hyper_plugin {
  int abi;                       // MI_ODE_HYPER_PLUGIN_ABI (also tells it apart from a mi_ode_rowlocal_plugin in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int (*launch_traj)(const mi::HyperArgs* A, hipStream_t st);
  int (*launch_resid)(const mi::HyperArgs* A, hipStream_t st);
};
