// One Runge-Kutta stage of the convolutional ODE function (tfdiffeq/models/conv_odenet.py: Conv2dODEFunc) as ONE launch:
//
//   y_s = y0 + sum_j (dt * beta_j) * k_j        mi_ode_lincomb_dev's operation order (k_lincomb, mi_ode_plane.h): bit-identical y_s
//   h1  = act(conv1(y_s))                       1x1, C -> F
//   h2  = act(conv2(h1))                        3x3, zero-padded "same", F -> F
//   k   = sign * conv3(h2)                      1x1, F -> C
//
// Workgroup = 256 threads (4 wavefronts) owning an 8 x 8 pixel tile of one image (tiles clip at the image border):
//   y_s   formed on the tile plus a one-pixel halo (10 x 10) straight from y0 / k_j in HBM, into LDS [100][C]; the tile's own pixels
//         optionally stored (y_out: the last stage of an FSAL tableau is y1)
//   h1    on the 10 x 10 halo, into LDS [100][Fp + 1] (F zero padded to the MFMA granule of 16, one pad column against bank
//         conflicts); halo pixels outside the image hold 0 - conv2 zero-pads h1, not act(b1)
//   h2    implicit GEMM M = 64 pixels, N = Fp, K = 9 Fp on the matrix cores: wavefront w owns pixels 16 w .. 16 w + 15 and every
//         16-column block of N (<= 8 accumulators); A = h1 rows of the tap's shifted pixels read from LDS, B = the packed
//         [tap][in][out] weights read through L2 (590 KB at F = 128 in float32: too large for LDS next to h1).
//         v_mfma_f32_16x16x4_f32 (exact float32 products - gfx950 has no xf32) / v_mfma_f64_16x16x4_f64.
//         Epilogue: + b2 + t * (sum of the time channel's weights over the taps that land INSIDE the image - the time channel is
//         zero padded like every other channel), act, into LDS over h1 (after a barrier)
//   k     conv3 for the tile's own pixels, scalar dot products over F, stored to k_out (NCHW)
// Time enters 1x1 convs as the uniform bias t * w_t; t is read from the device stage-time buffer (graph replays see new times).
// sign = -1 (reversed time axis): k = -f(-t, y), the sign folded into the kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mi_ode.h"

namespace mi {

constexpr int kConvThreads = 256;
constexpr int kConvTile = 8;                             // tile edge (pixels)
constexpr int kConvHalo = kConvTile + 2;                 // 10: tile plus the 3x3 halo
constexpr int kConvHaloPix = kConvHalo * kConvHalo;      // 100
constexpr int kConvTilePix = kConvTile * kConvTile;      // 64 = M of the conv2 GEMM: 4 wavefronts x 16 rows

struct ConvArgs {
  const void* y0;
  const void* ks[MI_ODE_MAX_K];
  double beta[MI_ODE_MAX_K];
  int n_k;
  const double* dt;
  const void* t;
  void* k_out;
  void* y_out;
  const void *w1, *b1, *w2, *w2t, *b2, *w3, *b3;
  double sign;
  int C, H, W, F, Fp, tiles_x, n_tiles;
};

template <typename T>
struct ConvMfma;
template <>
struct ConvMfma<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t step(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }        // f64 C / D layout
};
template <>
struct ConvMfma<float> {
  typedef float acc_t __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t step(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};

// nn.ReLU (NaN stays NaN), nn.Softplus (beta 1, threshold 20), nn.Tanh - torch's formulas, ocml's exp / log1p / tanh
template <typename T, int ACT>
__device__ __forceinline__ T conv_act(T x) {
  if constexpr (ACT == MI_ODE_CONV_ACT_RELU) return x > (T)0 ? x : (x != x ? x : (T)0);
  else if constexpr (ACT == MI_ODE_CONV_ACT_SOFTPLUS) return x > (T)20 ? x : log1p(exp(x));
  else return tanh(x);
}

__host__ __device__ inline size_t conv_lds_bytes(int Fp, size_t elem) {
  return (size_t)(kConvHaloPix * MI_ODE_CONV_MAX_C + kConvHaloPix * (Fp + 1)) * elem;
}

template <typename T, int ACT, bool TD>
__global__ __launch_bounds__(kConvThreads) void k_conv_stage(ConvArgs A) {
  using M = ConvMfma<T>;
  extern __shared__ __align__(16) unsigned char conv_smem[];
  T* s_y = (T*)conv_smem;                                  // [100][C]
  T* s_h = s_y + kConvHaloPix * MI_ODE_CONV_MAX_C;         // h1 [100][Ld], later h2 [64][Ld]
  const int C = A.C, H = A.H, W = A.W, F = A.F, Fp = A.Fp, Ld = Fp + 1;
  const int tid = (int)threadIdx.x;
  const long long b = (long long)blockIdx.x / A.n_tiles;
  const int tile = (int)((long long)blockIdx.x - b * A.n_tiles);
  const int ty0 = (tile / A.tiles_x) * kConvTile, tx0 = (tile % A.tiles_x) * kConvTile;
  const long long HW = (long long)H * W;
  const long long img = b * C * HW;
  const bool neg = A.sign < 0.0;
  T tt = (T)0;
  if constexpr (TD) tt = neg ? -*(const T*)A.t : *(const T*)A.t;
  const T scale = A.n_k > 0 ? (T)*A.dt : (T)0;

  // ---- y_s on tile + halo (k_lincomb's arithmetic, element for element) --------------------------------------------------------
  for (int i = tid; i < C * kConvHaloPix; i += kConvThreads) {
    const int c = i / kConvHaloPix, p = i - c * kConvHaloPix;
    const int py = p / kConvHalo, px = p - py * kConvHalo;
    const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
    T v = (T)0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const long long idx = img + c * HW + (long long)gy * W + gx;
      v = ((const T*)A.y0)[idx];
      if (A.n_k > 0) {
        T acc = (scale * (T)A.beta[0]) * ((const T*)A.ks[0])[idx];
        for (int j = 1; j < A.n_k; ++j) acc = acc + (scale * (T)A.beta[j]) * ((const T*)A.ks[j])[idx];
        v = v + acc;
      }
      if (A.y_out != nullptr && py >= 1 && py <= kConvTile && px >= 1 && px <= kConvTile) ((T*)A.y_out)[idx] = v;
    }
    s_y[p * MI_ODE_CONV_MAX_C + c] = v;
  }
  __syncthreads();

  // ---- h1 = act(conv1(y_s)) on tile + halo; 0 outside the image and in the padding columns ------------------------------------
  {
    const T* w1 = (const T*)A.w1;
    const T* b1 = (const T*)A.b1;
    const int cin = C + (TD ? 1 : 0);
    for (int i = tid; i < kConvHaloPix * Fp; i += kConvThreads) {
      const int p = i / Fp, f = i - p * Fp;
      const int py = p / kConvHalo, px = p - py * kConvHalo;
      const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
      T h = (T)0;
      if (f < F && gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const T* wr = w1 + (long long)f * cin;
        T z = b1[f];
        if constexpr (TD) z = z + wr[0] * tt;
        const T* yr = s_y + p * MI_ODE_CONV_MAX_C;
        for (int c = 0; c < C; ++c) z = z + wr[(TD ? 1 : 0) + c] * yr[c];
        h = conv_act<T, ACT>(z);
      }
      s_h[p * Ld + f] = h;
    }
  }
  __syncthreads();

  // ---- h2 = conv2(h1): implicit GEMM on the matrix cores ---------------------------------------------------------------------------
  const int wave = tid >> 6, lane = tid & 63, kr = lane >> 4, cl = lane & 15;
  const int NB = Fp / 16, KS = Fp / 4;
  typename M::acc_t acc[MI_ODE_CONV_MAX_F / 16];
#pragma unroll
  for (int nb = 0; nb < MI_ODE_CONV_MAX_F / 16; ++nb) acc[nb] = (typename M::acc_t){(T)0, (T)0, (T)0, (T)0};
  {
    const int m = 16 * wave + cl;                            // the A row this lane supplies: tile pixel m
    const int my = m / kConvTile, mx = m - my * kConvTile;
    const T* w2 = (const T*)A.w2;
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - dy * 3;
      const T* ap = s_h + ((my + dy) * kConvHalo + mx + dx) * Ld + kr;             // A[pixel m][k = 4 s + kr] (in channel)
      const T* bp = w2 + (long long)tap * Fp * Fp + (long long)kr * Fp + cl;       // B[k = 4 s + kr][out 16 nb + cl]
      for (int s = 0; s < KS; ++s) {
        const T a = ap[4 * s];
        const T* bs = bp + (long long)4 * s * Fp;
#pragma unroll
        for (int nb = 0; nb < MI_ODE_CONV_MAX_F / 16; ++nb)
          if (nb < NB) acc[nb] = M::step(a, bs[16 * nb], acc[nb]);
      }
    }
  }
  __syncthreads();                                           // every wavefront is done reading h1: h2 goes over it
  {
    const T* b2 = (const T*)A.b2;
    const T* w2t = (const T*)A.w2t;
#pragma unroll
    for (int nb = 0; nb < MI_ODE_CONV_MAX_F / 16; ++nb) {
      if (nb >= NB) break;
      const int f = 16 * nb + cl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * wave + M::row(lane, r);
        T h = (T)0;
        if (f < F) {
          T z = acc[nb][r] + b2[f];
          if constexpr (TD) {
            const int gy = ty0 + m / kConvTile, gx = tx0 + m % kConvTile;
            T ws = (T)0;                                     // the time channel's taps that land inside the image
            for (int tap = 0; tap < 9; ++tap) {
              const int sy = gy + tap / 3 - 1, sx = gx + tap % 3 - 1;
              if (sy >= 0 && sy < H && sx >= 0 && sx < W) ws = ws + w2t[tap * F + f];
            }
            z = z + ws * tt;
          }
          h = conv_act<T, ACT>(z);
        }
        s_h[m * Ld + f] = h;
      }
    }
  }
  __syncthreads();

  // ---- k = sign * conv3(h2) for the tile's own pixels ---------------------------------------------------------------------------
  {
    const T* w3 = (const T*)A.w3;
    const T* b3 = (const T*)A.b3;
    const int fin = F + (TD ? 1 : 0);
    for (int i = tid; i < C * kConvTilePix; i += kConvThreads) {
      const int c = i / kConvTilePix, m = i - c * kConvTilePix;
      const int gy = ty0 + m / kConvTile, gx = tx0 + m % kConvTile;
      if (gy >= H || gx >= W) continue;
      const T* wr = w3 + (long long)c * fin;
      T z = b3[c];
      if constexpr (TD) z = z + wr[0] * tt;
      const T* hr = s_h + m * Ld;
      for (int f = 0; f < F; ++f) z = z + wr[(TD ? 1 : 0) + f] * hr[f];
      ((T*)A.k_out)[img + c * HW + (long long)gy * W + gx] = neg ? -z : z;
    }
  }
}

}  // namespace mi
