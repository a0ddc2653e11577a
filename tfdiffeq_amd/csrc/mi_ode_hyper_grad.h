// The gradient of a hypersolver call (csrc/mi_ode_hyper.h is the forward): all steps and all rows of the reverse sweep of a
// `trajectory`, or the parameter gradient of a `_hypersolver_residuals` call, in ONE launch.
//
//   hyper_grad_step     one step of one trajectory backwards, host/device, no HIP construct: takes f (operator() + vjp, what
//                       tfdiffeq_amd/lower.py generates) and a "g with vjp" object (eval keeps the activations of ONE evaluation, vjp
//                       applies J_g^T to it and adds that evaluation's parameter contributions).  The kernel passes the MFMA-backed g
//                       below, the CPU tests a plain-loop dense g compiled by g++.
//   k_hyper_grad_traj   the forward's decomposition: 256 threads own a tile of 16 trajectories, lanes 0..15 of wavefront 0 run f and its
//                       vjp, all four wavefronts run g's layers and their transposes as 16x16x4 MFMA chains.  lambda = G[T-1]; for
//                       i = T-2 .. 0 the step is redone from the stored state out[i] (no checkpoints) and lambda <- ybar + G[i].
//   k_hyper_grad_resid  no recursion: row r of the base trajectory contributes the parameter gradient of g([y_r, f(t_i, y_r), dt]) under G[r].
//
// g backwards, per evaluation: the forward keeps every layer's input X_l and pre-activation Z_l in LDS (row strides follow the layer
// widths); then for l = L-1 .. 0: Z_l <- delta (.) act'(Z_l) in place (a thread per column, which also sums the column for db and the
// PReLU rule), delta_prev = Z_l . W_l (B operand: a second weight image in torch's own [out][in] orientation, so that no read is
// transposed), dW_l += X_l^T . Z_l (M = input block, N = output block, K = the tile's 16 rows).
//
// Where dW accumulates: in the workgroup's OWN row of a [grid, P] buffer in global memory (P: the padded pack layout), read and written
// only by that workgroup, every element always by the same lane - write-through stores and L1-bypassing loads, no barrier needed between
// steps; the first evaluation of a workgroup stores instead of adding, so the buffer needs no zeroing.  It costs one L2 round trip of P
// elements per evaluation and bounds nothing: the box is bounded by the activations (X_l, Z_l of one evaluation must fit in LDS).
// The fold is k_discrete_rowlocal's: the stores drain, the workgroup takes a ticket, the LAST arrival sums the rows in workgroup order
// straight into the gradient tensors (torch layout).  No floating-point atomics, no workgroup waits for another: reruns agree in every bit.
#pragma once

#ifndef MI_ODE_HG_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_ODE_HG_HD __host__ __device__ __forceinline__
#else
#define MI_ODE_HG_HD inline
#endif
#endif

namespace mi {

constexpr int kHgEuler = 0, kHgMidpoint = 1, kHgHeun = 2;      // enum mi_ode_hyper_method

struct HyperGradNoAcc {                                        // f has no trainable tensor (P = 0): its vjp never calls add
  template <typename T>
  MI_ODE_HG_HD void add(int, T) {}
};

// One step of one trajectory backwards: ybar = (d step / d y)^T lam, g's parameter contributions through g.vjp.  x = [y, k, dt]; the
// cotangent of the dt column is dropped.  dt is t_span[1] - t_span[0] for every step (the reference's quirk).
template <typename T, int METHOD, int D, class F, class G>
MI_ODE_HG_HD void hyper_grad_step(const F& f, G& g, T t, T dt, const T* y, const T* lam, T* ybar) {
  HyperGradNoAcc na;
  const T dt2 = dt * dt, dt3 = dt * dt * dt;
  T k1[D], gv[D], gb[D], xy[D], xk[D], kb[D], fy[D];
  f(t, y, k1);
  if constexpr (METHOD == kHgEuler) {
    g.eval(y, k1, dt, gv);                                     // y+ = y + k1 dt + dt^2 g(x1)
#pragma unroll
    for (int d = 0; d < D; ++d) gb[d] = dt2 * lam[d];
    g.vjp(gb, xy, xk);
#pragma unroll
    for (int d = 0; d < D; ++d) kb[d] = dt * lam[d] + xk[d];
    f.vjp(t, y, kb, fy, na);
#pragma unroll
    for (int d = 0; d < D; ++d) ybar[d] = lam[d] + xy[d] + fy[d];
  } else {
    constexpr bool mid = METHOD == kHgMidpoint;
    T y2[D], k2[D], yb2[D];
    g.eval(y, k1, dt, gv);
#pragma unroll
    for (int d = 0; d < D; ++d) y2[d] = mid ? y[d] + k1[d] * dt / (T)2 + dt2 * gv[d] : y[d] + k1[d] * dt + dt2 * gv[d];
    const T t2 = mid ? t + dt / (T)2 : t + dt;
    f(t2, y2, k2);
    g.eval(y2, k2, dt, gv);                                    // the second evaluation's backward comes first
#pragma unroll
    for (int d = 0; d < D; ++d) gb[d] = dt3 * lam[d];
    g.vjp(gb, xy, xk);
#pragma unroll
    for (int d = 0; d < D; ++d) kb[d] = (mid ? dt : dt / (T)2) * lam[d] + xk[d];
    f.vjp(t2, y2, kb, fy, na);
#pragma unroll
    for (int d = 0; d < D; ++d) yb2[d] = xy[d] + fy[d];
    g.eval(y, k1, dt, gv);                                     // the first evaluation again: g keeps one set of activations
#pragma unroll
    for (int d = 0; d < D; ++d) gb[d] = dt2 * yb2[d];
    g.vjp(gb, xy, xk);
#pragma unroll
    for (int d = 0; d < D; ++d) kb[d] = (mid ? dt / (T)2 * yb2[d] : dt / (T)2 * lam[d] + dt * yb2[d]) + xk[d];
    f.vjp(t, y, kb, fy, na);
#pragma unroll
    for (int d = 0; d < D; ++d) ybar[d] = lam[d] + yb2[d] + xy[d] + fy[d];
  }
}

}  // namespace mi

#if defined(__HIPCC__)
#include "mi_ode_hyper.h"

namespace mi {

static_assert(kHgEuler == MI_ODE_HYPER_EULER && kHgMidpoint == MI_ODE_HYPER_MIDPOINT && kHgHeun == MI_ODE_HYPER_HEUN, "method codes");

constexpr int kHgMaxGrid = MI_ODE_HYPER_GRAD_MAX_GRID;
constexpr size_t kHgLdsBudget = 160 * 1024;

struct HyperGradArgs {
  const void* t;                 // [T], state dtype
  const void* ys;                // trajectory: the forward's output [T, batch, dim]; residuals: the base trajectory [T, batch, dim]
  const void* gout;              // [T, batch, dim] the gradient of the loss with respect to the call's result
  void* gy;                      // [batch, dim] or null (trajectory only)
  void* partials;                // [grid, pack_elems] workspace
  unsigned* ticket;              // device word, zero between launches
  const void* pack;              // both weight images in global memory (lds_w == 0), else null
  long long batch, rows;
  int T, dim, method, mode, n_layers, lds_w, want_params;
  int in[kHypMaxLayers], out_[kHypMaxLayers], kp[kHypMaxLayers], np[kHypMaxLayers], act[kHypMaxLayers], n_alpha[kHypMaxLayers];
  double slope[kHypMaxLayers];
  const void* w[kHypMaxLayers];
  const void* b[kHypMaxLayers];
  const void* alpha[kHypMaxLayers];
  void* gw[kHypMaxLayers];       // gradient tensors, torch layout, null: not wanted
  void* gb[kHypMaxLayers];
  void* ga[kHypMaxLayers];
  int off_w[kHypMaxLayers], off_b[kHypMaxLayers], off_a[kHypMaxLayers];   // forward image / partial row: W^T [Kp][Np] | b [Np] | a [Np]
  int off_wb[kHypMaxLayers];     // backward image (behind the forward one): W [Np][Kp]
  int off_x[kHypMaxLayers], off_z[kHypMaxLayers], off_d, ld_d;             // LDS: X_l [16][Kp + 1], Z_l [16][Np + 1], delta [16][ld_d]
  int pack_elems, image_elems, act_elems;                                   // image_elems: both images; act_elems: all tiles
  RhsParams rhs;
};

// the layout every party uses (host launcher, pack kernel, Python through mi_ode_hyper_grad_workspace_bytes)
inline void hyper_grad_layout(HyperGradArgs& A) {
  int off = 0, maxw = 16;
  for (int l = 0; l < A.n_layers; ++l) {
    A.kp[l] = (A.in[l] + 15) / 16 * 16;
    A.np[l] = (A.out_[l] + 15) / 16 * 16;
    A.off_w[l] = off; off += A.kp[l] * A.np[l];
    A.off_b[l] = off; off += A.np[l];
    A.off_a[l] = off; off += A.np[l];
    if (A.kp[l] > maxw) maxw = A.kp[l];
    if (A.np[l] > maxw) maxw = A.np[l];
  }
  A.pack_elems = off;
  for (int l = 0; l < A.n_layers; ++l) { A.off_wb[l] = off; off += A.np[l] * A.kp[l]; }
  A.image_elems = off;
  int lo = 0;
  for (int l = 0; l < A.n_layers; ++l) {
    A.off_x[l] = lo; lo += kHypRows * (A.kp[l] + 1);
    A.off_z[l] = lo; lo += kHypRows * (A.np[l] + 1);
  }
  A.off_d = lo; A.ld_d = maxw + 1; lo += kHypRows * A.ld_d;
  A.act_elems = (lo + 1) / 2 * 2;                              // (even: what follows stays 16-byte aligned in float64, 8 in float32)
}

// dynamic LDS: the tiles, the two images when they live there, one flag word in a 16-byte slot (no static LDS: the dynamic base stays aligned)
template <typename T>
inline size_t hyper_grad_lds_bytes(const HyperGradArgs& A, bool lds_w) {
  return (size_t)(A.act_elems + (lds_w ? A.image_elems : 0)) * sizeof(T) + 16;
}

template <typename T>
__device__ void hyper_grad_pack(const HyperGradArgs& A, T* dst, int tid, int nt) {
  for (int l = 0; l < A.n_layers; ++l) {
    const T* W = (const T*)A.w[l];
    const T* B = (const T*)A.b[l];
    const T* Al = (const T*)A.alpha[l];
    const int in = A.in[l], out = A.out_[l], np = A.np[l], kp = A.kp[l];
    for (int e = tid; e < kp * np; e += nt) {
      const int k = e / np, c = e - k * np;
      dst[A.off_w[l] + e] = (k < in && c < out) ? W[(long long)c * in + k] : (T)0;
    }
    for (int e = tid; e < kp * np; e += nt) {
      const int c = e / kp, k = e - c * kp;
      dst[A.off_wb[l] + e] = (k < in && c < out) ? W[(long long)c * in + k] : (T)0;
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
__global__ __launch_bounds__(256) void k_hyper_grad_pack(HyperGradArgs A) {
  hyper_grad_pack<T>(A, (T*)A.pack, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}

// act'(z), torch's backward formulas (Softplus: beta 1, threshold 20)
template <typename T>
__device__ __forceinline__ T hyper_act_grad(int act, T z, T a) {
  switch (act) {
    case MI_ODE_HYPER_ACT_RELU: return z > (T)0 ? (T)1 : (T)0;
    case MI_ODE_HYPER_ACT_LEAKY_RELU:
    case MI_ODE_HYPER_ACT_PRELU: return z > (T)0 ? (T)1 : a;
    case MI_ODE_HYPER_ACT_TANH: { const T th = tanh(z); return (T)1 - th * th; }
    case MI_ODE_HYPER_ACT_SOFTPLUS: { if (z > (T)20) return (T)1; const T e = exp(z); return e / (e + (T)1); }
    default: return (T)1;
  }
}

__device__ __forceinline__ void hg_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void hg_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float hg_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double hg_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// g on the workgroup's tile, with its vjp.  EVERY thread of the workgroup calls eval / vjp (they hold barriers); lanes 0..15 of
// wavefront 0 (`owner`) carry one trajectory each, the other threads pass and receive nothing.
template <typename T, int D>
struct HyperGradG {
  using M = HypMfma<T>;
  const HyperGradArgs& A;
  const T* wi;                   // the images (LDS or global)
  T* lds;                        // the tiles
  T* part;                       // this workgroup's row of the partials
  bool first;                    // no evaluation has been added to `part` yet
  bool owner;
  int tid;

  __device__ __forceinline__ void eval(const T* y, const T* k, T dt, T* out) {
    const int L = A.n_layers;
    if (owner) {
      T* x = lds + A.off_x[0] + tid * (A.kp[0] + 1);
#pragma unroll
      for (int d = 0; d < D; ++d) { x[d] = y[d]; x[D + d] = k[d]; }
      x[2 * D] = dt;
      for (int c = 2 * D + 1; c < A.kp[0]; ++c) x[c] = (T)0;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, kr = lane >> 4, cl = lane & 15;
    for (int l = 0; l < L; ++l) {
      const int np = A.np[l], kp = A.kp[l], ks = kp / 4, outw = A.out_[l], act = A.act[l];
      const int ldx = kp + 1, ldz = np + 1;
      const T* X = lds + A.off_x[l];
      T* Z = lds + A.off_z[l];
      T* nxt = l + 1 < L ? lds + A.off_x[l + 1] : lds + A.off_d;
      const int ldn = l + 1 < L ? A.kp[l + 1] + 1 : A.ld_d;
      const T* W = wi + A.off_w[l];
      for (int cb = wave; cb < np / 16; cb += kHypThreads / 64) {
        typename M::acc_t acc = {(T)0, (T)0, (T)0, (T)0};
        const T* ap = X + cl * ldx + kr;
        const T* bp = W + kr * np + 16 * cb + cl;
        for (int s = 0; s < ks; ++s) acc = M::step(ap[4 * s], bp[4 * s * np], acc);
        const int col = 16 * cb + cl;
        const T bias = wi[A.off_b[l] + col], a = wi[A.off_a[l] + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = M::row(lane, r);
          const T z = acc[r] + bias;
          Z[row * ldz + col] = col < outw ? z : (T)0;
          nxt[row * ldn + col] = col < outw ? hyper_act<T>(act, z, a) : (T)0;
        }
      }
      __syncthreads();
    }
    const T* o = lds + A.off_d + tid * A.ld_d;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = owner ? o[d] : (T)0;
  }

  __device__ __forceinline__ void vjp(const T* gbar, T* xy, T* xk) {
    const int L = A.n_layers;
    T* Dl = lds + A.off_d;
    const int ldd = A.ld_d;
    if (owner) {
      for (int c = 0; c < A.np[L - 1]; ++c) Dl[tid * ldd + c] = (T)0;
#pragma unroll
      for (int d = 0; d < D; ++d) Dl[tid * ldd + d] = gbar[d];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, kr = lane >> 4, cl = lane & 15;
    for (int l = L - 1; l >= 0; --l) {
      const int np = A.np[l], kp = A.kp[l], act = A.act[l];
      const int ldx = kp + 1, ldz = np + 1;
      const T* X = lds + A.off_x[l];
      T* Z = lds + A.off_z[l];
      if (tid < np) {                                          // delta_pre = delta (.) act'(z), in place; the column sums
        const T a = wi[A.off_a[l] + tid];
        T db = (T)0, da = (T)0;
        for (int r = 0; r < kHypRows; ++r) {
          const T z = Z[r * ldz + tid], dl = Dl[r * ldd + tid];
          const T dp = dl * hyper_act_grad<T>(act, z, a);
          Z[r * ldz + tid] = dp;
          db += dp;
          da += z > (T)0 ? (T)0 : dl * z;                      // d prelu / d weight = z where z <= 0
        }
        if (A.want_params) {
          T* pb = part + A.off_b[l] + tid;
          T* pa = part + A.off_a[l] + tid;
          hg_store(pb, first ? db : hg_load(pb) + db);
          if (act == MI_ODE_HYPER_ACT_PRELU) hg_store(pa, first ? da : hg_load(pa) + da);
        }
      }
      __syncthreads();
      const T* Wb = wi + A.off_wb[l];
      for (int cb = wave; cb < kp / 16; cb += kHypThreads / 64) {              // delta_prev = delta_pre . W
        typename M::acc_t acc = {(T)0, (T)0, (T)0, (T)0};
        const T* ap = Z + cl * ldz + kr;
        const T* bp = Wb + kr * kp + 16 * cb + cl;
        for (int s = 0; s < np / 4; ++s) acc = M::step(ap[4 * s], bp[4 * s * kp], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) Dl[M::row(lane, r) * ldd + 16 * cb + cl] = acc[r];
      }
      if (A.want_params) {                                     // dW += X^T . delta_pre, the block's accumulator in this workgroup's row
        const int nob = np / 16, nblk = (kp / 16) * nob;
        for (int blk = wave; blk < nblk; blk += kHypThreads / 64) {
          const int ib = blk / nob, ob = blk - ib * nob;
          T* pw = part + A.off_w[l] + (16 * ib) * np + 16 * ob + cl;
          typename M::acc_t acc = {(T)0, (T)0, (T)0, (T)0};
          if (!first) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = hg_load(pw + M::row(lane, r) * np);
          }
          const T* ap = X + kr * ldx + 16 * ib + cl;             // A[m = input 16 ib + cl][k = row 4 s + kr]
          const T* bp = Z + kr * ldz + 16 * ob + cl;             // B[k = row 4 s + kr][n = output 16 ob + cl]
#pragma unroll
          for (int s = 0; s < kHypRows / 4; ++s) acc = M::step(ap[4 * s * ldx], bp[4 * s * ldz], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) hg_store(pw + M::row(lane, r) * np, acc[r]);
        }
      }
      __syncthreads();
    }
    first = false;
#pragma unroll
    for (int d = 0; d < D; ++d) { xy[d] = owner ? Dl[tid * ldd + d] : (T)0; xk[d] = owner ? Dl[tid * ldd + D + d] : (T)0; }
  }
};

// f behind a switch: a thread without a trajectory evaluates nothing
template <typename T, class RHS>
struct HyperGradF {
  const RHS& rhs;
  bool on;
  __device__ __forceinline__ void operator()(T t, const T* y, T* k) const {
    if (on) rhs(t, y, k);
    else {
#pragma unroll
      for (int d = 0; d < RHS::D; ++d) k[d] = (T)0;
    }
  }
  template <class ACC>
  __device__ __forceinline__ void vjp(T t, const T* y, const T* kbar, T* ybar, ACC& acc) const {
    if (on) rhs.vjp(t, y, kbar, ybar, acc);
    else {
#pragma unroll
      for (int d = 0; d < RHS::D; ++d) ybar[d] = (T)0;
    }
  }
};

// the workgroup's row is complete: drain, take a ticket; the last workgroup folds the rows in workgroup order into the gradient tensors
template <typename T>
__device__ void hyper_grad_fold(const HyperGradArgs& A, T* lds, int* s_last) {
  const int tid = (int)threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this thread's stores have landed before the workgroup's ticket says so
  __syncthreads();
  if (tid == 0) {
    const unsigned tk = __hip_atomic_fetch_add(A.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (tk == gridDim.x - 1);
  }
  __syncthreads();
  if (!*s_last) return;
  const T* all = (const T*)A.partials;
  const long long PE = A.pack_elems;
  const unsigned G = gridDim.x;
  for (int l = 0; l < A.n_layers; ++l) {
    const int in = A.in[l], out = A.out_[l], np = A.np[l];
    T* gw = (T*)A.gw[l];
    T* gb = (T*)A.gb[l];
    T* ga = (T*)A.ga[l];
    if (gw != nullptr) {
      for (int e = tid; e < in * out; e += kHypThreads) {
        const int c = e / in, k = e - c * in;
        T s = (T)0;
        for (unsigned b = 0; b < G; ++b) s += hg_load(all + b * PE + A.off_w[l] + k * np + c);
        gw[e] = s;
      }
    }
    if (gb != nullptr) {
      for (int c = tid; c < out; c += kHypThreads) {
        T s = (T)0;
        for (unsigned b = 0; b < G; ++b) s += hg_load(all + b * PE + A.off_b[l] + c);
        gb[c] = s;
      }
    }
    if (ga != nullptr && A.act[l] == MI_ODE_HYPER_ACT_PRELU) {
      T s = (T)0;
      if (tid < out) {
        for (unsigned b = 0; b < G; ++b) s += hg_load(all + b * PE + A.off_a[l] + tid);
      }
      if (A.n_alpha[l] != 1) {
        if (tid < out) ga[tid] = s;
      } else {                                                 // one shared weight: the channels in channel order
        __syncthreads();
        if (tid < out) lds[tid] = s;
        __syncthreads();
        if (tid == 0) {
          T tot = (T)0;
          for (int c = 0; c < out; ++c) tot += lds[c];
          ga[0] = tot;
        }
      }
    }
  }
  if (tid == 0) __hip_atomic_store(A.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
__device__ __forceinline__ T* hyper_grad_smem() {
  extern __shared__ __align__(16) unsigned char hg_smem[];
  return (T*)hg_smem;
}

template <typename T, class RHS, int METHOD>
__global__ __launch_bounds__(256) void k_hyper_grad_traj(HyperGradArgs A) {
  constexpr int D = RHS::D;
  T* lds = hyper_grad_smem<T>();
  T* s_w = lds + A.act_elems;
  int* s_last = (int*)(s_w + (A.lds_w ? A.image_elems : 0));
  const int tid = (int)threadIdx.x;
  if (A.lds_w) {
    hyper_grad_pack<T>(A, s_w, tid, kHypThreads);
    __syncthreads();
  }
  const RHS rhs(A.rhs);
  const T* tp = (const T*)A.t;
  const T* ys = (const T*)A.ys;
  const T* go = (const T*)A.gout;
  T* gy = (T*)A.gy;
  const T dt = tp[1] - tp[0];
  const long long n = A.batch * D;
  const long long ntiles = (A.batch + kHypRows - 1) / kHypRows;
  HyperGradG<T, D> g{A, A.lds_w ? s_w : (const T*)A.pack, lds, (T*)A.partials + (long long)blockIdx.x * A.pack_elems, true, tid < kHypRows, tid};
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row = tile * kHypRows + tid;
    const bool live = tid < kHypRows && row < A.batch;
    const HyperGradF<T, RHS> f{rhs, live};
    T lam[D], y[D], yb[D];
#pragma unroll
    for (int d = 0; d < D; ++d) lam[d] = live ? go[(long long)(A.T - 1) * n + row * D + d] : (T)0;
    for (int i = A.T - 2; i >= 0; --i) {
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = live ? ys[(long long)i * n + row * D + d] : (T)0;
      hyper_grad_step<T, METHOD, D>(f, g, tp[i], dt, y, lam, yb);
#pragma unroll
      for (int d = 0; d < D; ++d) lam[d] = live ? yb[d] + go[(long long)i * n + row * D + d] : (T)0;
    }
    if (live && gy != nullptr) {
#pragma unroll
      for (int d = 0; d < D; ++d) gy[row * D + d] = lam[d];
    }
  }
  if (A.want_params) hyper_grad_fold<T>(A, lds, s_last);
}

template <typename T, class RHS>
__global__ __launch_bounds__(256) void k_hyper_grad_resid(HyperGradArgs A) {
  constexpr int D = RHS::D;
  T* lds = hyper_grad_smem<T>();
  T* s_w = lds + A.act_elems;
  int* s_last = (int*)(s_w + (A.lds_w ? A.image_elems : 0));
  const int tid = (int)threadIdx.x;
  if (A.lds_w) {
    hyper_grad_pack<T>(A, s_w, tid, kHypThreads);
    __syncthreads();
  }
  const RHS rhs(A.rhs);
  const T* tp = (const T*)A.t;
  const T* ys = (const T*)A.ys;
  const T* go = (const T*)A.gout;
  const T dt = tp[1] - tp[0];
  const long long ntiles = (A.rows + kHypRows - 1) / kHypRows;
  HyperGradG<T, D> g{A, A.lds_w ? s_w : (const T*)A.pack, lds, (T*)A.partials + (long long)blockIdx.x * A.pack_elems, true, tid < kHypRows, tid};
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long r = tile * kHypRows + tid;
    const bool live = tid < kHypRows && r < A.rows;
    const HyperGradF<T, RHS> f{rhs, live};
    T y[D], k[D], gv[D], gb[D], xy[D], xk[D];
#pragma unroll
    for (int d = 0; d < D; ++d) { y[d] = live ? ys[r * D + d] : (T)0; gb[d] = live ? go[r * D + d] : (T)0; }
    f(live ? tp[r / A.batch] : (T)0, y, k);
    g.eval(y, k, dt, gv);
    g.vjp(gb, xy, xk);
  }
  if (A.want_params) hyper_grad_fold<T>(A, lds, s_last);
}

// what a hyper-grad plugin (csrc/mi_ode_hyper_grad_plugin.h) instantiates for its functor
template <typename T, class RHS>
struct HyperGradLaunch {
  static int run(const HyperGradArgs* A, int grid, hipStream_t st) {
    static_assert(RHS::P == 0, "f of a fused hypersolver gradient has no trainable tensor");
    const void* fn = A->mode == MI_ODE_HYPER_G_RESIDUALS ? (const void*)k_hyper_grad_resid<T, RHS>
                   : A->mode != MI_ODE_HYPER_TRAJECTORY ? nullptr
                   : A->method == MI_ODE_HYPER_EULER ? (const void*)k_hyper_grad_traj<T, RHS, MI_ODE_HYPER_EULER>
                   : A->method == MI_ODE_HYPER_MIDPOINT ? (const void*)k_hyper_grad_traj<T, RHS, MI_ODE_HYPER_MIDPOINT>
                   : A->method == MI_ODE_HYPER_HEUN ? (const void*)k_hyper_grad_traj<T, RHS, MI_ODE_HYPER_HEUN> : nullptr;
    const size_t lds = hyper_grad_lds_bytes<T>(*A, A->lds_w != 0);
    if (fn == nullptr || grid < 1 || grid > kHgMaxGrid || A->dim != RHS::D || lds > kHgLdsBudget) return MI_ODE_E_INVALID;
    if (lds > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MI_ODE_E_HIP;
    void* args[] = {(void*)A};
    if (hipLaunchKernel(fn, dim3((unsigned)grid), dim3(kHypThreads), args, lds, st) != hipSuccess) return MI_ODE_E_HIP;
    return 0;
  }
};

}  // namespace mi

#define MI_ODE_HYPER_GRAD_PLUGIN_ABI 0x48470001
struct mi_ode_hyper_grad_plugin {
  int abi;                       // MI_ODE_HYPER_GRAD_PLUGIN_ABI (tells it apart from the other tables that travel in mi_ode_rhs.plugin)
  int dtype;                     // MI_ODE_F32 / MI_ODE_F64
  int dim;
  int (*launch)(const mi::HyperGradArgs* A, int grid, hipStream_t st);
};
#endif  // __HIPCC__
