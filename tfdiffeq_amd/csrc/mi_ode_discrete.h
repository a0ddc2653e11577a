// The exact gradient of a fixed-grid Runge-Kutta solve of the ODEFunc MLP (csrc/mi_ode_adjoint.h: same network, same operand layouts),
// fp32, time dependent or not: the TRANSPOSE of the discrete map the forward kernel computed, all steps in ONE launch.
//
// Forward step n (fixed_grid.py / rk_common.py:73-81):  Y_i = y_n + h sum_{j<i} a_ij k_j,  k_i = f(t_i, Y_i),  y_{n+1} = y_n + h sum_i b_i k_i.
// With lambda_{n+1} = dL/dy_{n+1} the reverse sweep runs, for i = s .. 1,
//     kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j,     Ybar_i = (df/dy at Y_i)^T kbar_i,     theta_bar += (df/dtheta at Y_i)^T kbar_i
// and lambda_n = lambda_{n+1} + sum_i Ybar_i + gbar_n (gbar_n: the caller's gradient of the output at grid point n).
//
// Rows are independent trajectories and a workgroup owns its 32-row tiles for the whole sweep (the persistent grid of k_adjoint_mlp), so
// nothing crosses workgroups per step - no controller, no norms.  Per step and tile:
//   1. forward tile pass: the <= 4 stages from the checkpoint y_n (the forward solution on the default grid holds every y_n), the layer
//      activations X = Y_i, H1, H2 of each stage to scratch slot i ([column][32 rows], the layout adj_wgrad_pass reads);
//   2. backward-data passes in reverse stage order through the three transposed layers: A = kbar_i, G2, G1 to the same slot; kbar_i and
//      Ybar_i stay in registers;
//   3. after `chunk` tiles: ONE weight-gradient pass X^T Delta over those tiles and all stages (adj_wgrad_pass, SWEEP instantiation:
//      coefficient 1, K = 32 rows x stages x chunk), accumulators in registers, added to this workgroup's own partial block.
// lambda lives in the caller's grad_y0 buffer between steps (a thread reads back what it wrote itself).  Schedule: `chunk` tiles form the
// inner unit - chunk = all tiles of the workgroup is "steps outer" (largest K per pass, scratch for every tile), chunk = 1 "tiles outer"
// (smallest scratch).  At the end ONE grid hand-off, then every workgroup folds its 1/G slice of theta_bar over the workgroups in a fixed
// order (adj_slice): no atomics, two runs give identical bits.  (A first hand-off right after the weights are staged is the residency
// check of every persistent kernel here.)
// Time-dependent network (a.td, dense_odenet.py:79-84): stage i of step n sees t_i = t_n + (h tn_i) / td_i in the state dtype - t_n + h / 2,
// t_n + h, t_n + h / 3, t_n + h 2 / 3: what fixed_grid.py and k_fixed_mlp form - as the bias shift t_i w_t of the first layer.  w_t does
// not multiply y, so the backward-data passes are what they were; its gradient is sum t_i (column sum of G1), which adj_wgrad_pass carries
// in st[] from the stage times of its pass list.  The stage times are formed once per step (disc_prepare), for the pass list and for the
// tile pass, so the weight applied to a column sum is the time its stage was evaluated at.  The tile pass has no register to spare (248
// VGPRs, 102 SGPRs before this): the bias shifts t_i w_t of the step's stages sit behind the dynamic LDS segment of AdjGeom (DiscLds:
// 4 x HP floats, zero for the time-independent network) and layer 1 reads its column's where it adds the bias - one transient register.
// theta_bar then starts with w_t [hidden].
#pragma once
#include "mi_ode_adjoint.h"

namespace mi {

constexpr int kDiscMaxStages = 4;
constexpr int kDiscMaxSteps = 1024;                          // step sizes travel in the argument block

struct DiscResult {            // pinned host record, written by the kernel's last act
  unsigned status;
  int handoffs;
  long long prof[3];           // workgroup 0, 10 ns ticks: tile passes, weight-gradient passes, final hand-off + fold
};

struct DiscArgs {
  AdjArgs a;                   // what adj_wgrad_pass / adj_slice / AdjCtx read: shape, weights (a.p.s.rhs), act, wpart, P, Ppad, SL, hand-off plumbing
  const float* ys;             // [N, batch, dim] the forward solution
  const float* gys;            // [N, batch, dim] gradient of the loss with respect to it
  float* lam;                  // [batch, dim] lambda; on return grad_y0
  float* th_out;               // [P] canonical order
  DiscResult* res;
  int N;                       // grid points
  int S;                       // stages
  int chunk;                   // tiles per weight-gradient pass
  float ha[kDiscMaxStages][kDiscMaxStages];   // a_ij (row i, j < i)
  float hb[kDiscMaxStages];
  float tn[kDiscMaxStages], tdn[kDiscMaxStages];   // stage i is evaluated at t[n] + (h tn[i]) / tdn[i] (stage 0 at t[n])
  float h[kDiscMaxSteps];      // t[n + 1] - t[n] in the state dtype
  float t0[kDiscMaxSteps];     // t[n] in the state dtype (time-dependent network)
};

// What the discrete kernel keeps behind AdjGeom's dynamic LDS segment: tw[stage][HP] = t_stage w_t[column] of the current step (zero in
// the padding, all zero for the time-independent network).
template <int DP, int HP>
struct DiscLds {
  static constexpr int OFF_TW = (int)(AdjGeom<DP, HP>::lds_bytes() / sizeof(float));
  static constexpr size_t lds_bytes() { return (size_t)(OFF_TW + kDiscMaxStages * HP) * sizeof(float); }
};

// The times the network sees at the stages of step n, to ts[0 .. S - 1]: the forward kernels' expressions (mi_ode_mlp.h k_fixed_mlp:
// te + dt / 3.0f, te + dt * 2.0f / 3.0f, te + dt; fixed_grid.py:16-32: t + dt / 2, t + dt).  Zeros for the time-independent network, whose
// first layer then adds 0 w_t = 0 whatever the grid holds.
template <class DA>
__device__ __forceinline__ void disc_stage_times(const DA& D, int n, float* ts) {
  const float t0 = D.t0[n], hn = D.h[n];
#pragma unroll
  for (int q = 0; q < kDiscMaxStages; ++q) ts[q] = (!D.a.td || q >= D.S) ? 0.f : q == 0 ? t0 : t0 + (hn * D.tn[q]) / D.tdn[q];
}

template <int DP, int HP, int ACT>
struct DiscCtx : AdjCtx<DP, HP, ACT> {
  using B = AdjCtx<DP, HP, ACT>;
  using G = AdjGeom<DP, HP>;

  // f4 = f(t_s, xs) for the tile whose stage inputs are xs (4 elements per owner thread); X, H1, H2 go to the slot `act`.
  // s: the stage - its time shifts the first layer's bias by t_s w_t, as in AdjCtx::eval (the product from DiscLds; 0 for the
  // time-independent network).  Every thread of the workgroup must call it.
  __device__ __forceinline__ void fwd(const float* xs, float* f4, g_float* act, int s) {
    constexpr int KS1 = G::KS1, KS2 = G::KS2;
    using DL = DiscLds<DP, HP>;
    if (B::wave < G::NW3) {
#pragma unroll
      for (int i = 0; i < 4; ++i) B::s_x[(B::rbase + i) * G::LDX + B::col] = xs[i];
      *(g_f4*)(act + (unsigned)(G::OFF_X + B::col * G::R + B::rbase)) = adj_f4{xs[0], xs[1], xs[2], xs[3]};
    }
    __syncthreads();
    if (B::wave < G::NW12) {                                // layer 1
      adj_f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS1 / 4; ++m) {
        const int k0 = adj_k<G::CH1>(B::lg, 4 * m);
        const adj_f4 a0 = *(const lds_f4*)(B::s_x + B::li * G::LDX + k0), a1 = *(const lds_f4*)(B::s_x + (16 + B::li) * G::LDX + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float b = B::s_w1[(k0 + v) * G::LW1 + B::col12];
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], b, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], b, c1, 0, 0, 0);
        }
      }
      const float b1e = B::b1v + B::s_w1[DL::OFF_TW + s * HP + B::col12];     // (read here: no register is held across the products)
      float h[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        h[i] = mlp_act<ACT>(c0[i] + b1e);
        h[4 + i] = mlp_act<ACT>(c1[i] + b1e);
        B::s_hA[(4 * B::lg + i) * G::LDH + B::col12] = h[i];
        B::s_hA[(16 + 4 * B::lg + i) * G::LDH + B::col12] = h[4 + i];
      }
      *(g_f4*)(act + (unsigned)(G::OFF_H1 + B::col12 * G::R + 4 * B::lg)) = adj_f4{h[0], h[1], h[2], h[3]};
      *(g_f4*)(act + (unsigned)(G::OFF_H1 + B::col12 * G::R + 16 + 4 * B::lg)) = adj_f4{h[4], h[5], h[6], h[7]};
    }
    __syncthreads();
    if (B::wave < G::NW12) {                                // layer 2
      adj_f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS2 / 4; ++m) {
        const int k0 = adj_k<G::CH2>(B::lg, 4 * m);
        const adj_f4 a0 = *(const lds_f4*)(B::s_hA + B::li * G::LDH + k0), a1 = *(const lds_f4*)(B::s_hA + (16 + B::li) * G::LDH + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], B::w2f[4 * m + v], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], B::w2f[4 * m + v], c1, 0, 0, 0);
        }
      }
      float h[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        h[i] = mlp_act<ACT>(c0[i] + B::b2v);
        h[4 + i] = mlp_act<ACT>(c1[i] + B::b2v);
        B::s_hB[(4 * B::lg + i) * G::LDH + B::col12] = h[i];
        B::s_hB[(16 + 4 * B::lg + i) * G::LDH + B::col12] = h[4 + i];
      }
      *(g_f4*)(act + (unsigned)(G::OFF_H2 + B::col12 * G::R + 4 * B::lg)) = adj_f4{h[0], h[1], h[2], h[3]};
      *(g_f4*)(act + (unsigned)(G::OFF_H2 + B::col12 * G::R + 16 + 4 * B::lg)) = adj_f4{h[4], h[5], h[6], h[7]};
    }
    __syncthreads();
    if (B::wave < G::NW3) {                                 // layer 3
      const int rb = B::wave / G::CB;
      adj_f4 c = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS2 / 4; ++m) {
        const int k0 = adj_k<G::CH2>(B::lg, 4 * m);
        const adj_f4 a = *(const lds_f4*)(B::s_hB + (16 * rb + B::li) * G::LDH + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[v], B::s_w3[(k0 + v) * G::LW3 + B::col], c, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) f4[i] = c[i] + B::b3v;
    }
  }

  // v4 = as^T df/dy at the stage whose activations fwd() left in the slot `act`; A = as, G2, G1 go to the same slot.
  // Every thread of the workgroup must call it.
  __device__ __forceinline__ void bwd(const float* as, float* v4, g_float* act) {
    constexpr int KS1 = G::KS1, KS2 = G::KS2;
    float h1k[8], h2k[8];
    if (B::wave < G::NW3) {
#pragma unroll
      for (int i = 0; i < 4; ++i) B::s_a[(B::rbase + i) * G::LDX + B::col] = as[i];
      *(g_f4*)(act + (unsigned)(G::OFF_A + B::col * G::R + B::rbase)) = adj_f4{as[0], as[1], as[2], as[3]};
    }
    if (B::wave < G::NW12) {                                // this lane's own activations of the stage (it wrote them itself)
      const adj_f4 p0 = *(const g_f4*)(act + (unsigned)(G::OFF_H1 + B::col12 * G::R + 4 * B::lg));
      const adj_f4 p1 = *(const g_f4*)(act + (unsigned)(G::OFF_H1 + B::col12 * G::R + 16 + 4 * B::lg));
      const adj_f4 q0 = *(const g_f4*)(act + (unsigned)(G::OFF_H2 + B::col12 * G::R + 4 * B::lg));
      const adj_f4 q1 = *(const g_f4*)(act + (unsigned)(G::OFF_H2 + B::col12 * G::R + 16 + 4 * B::lg));
#pragma unroll
      for (int i = 0; i < 4; ++i) { h1k[i] = p0[i]; h1k[4 + i] = p1[i]; h2k[i] = q0[i]; h2k[4 + i] = q1[i]; }
    }
    __syncthreads();
    if (B::wave < G::NW12) {                                // layer 3 transposed: g2 = (a @ W3^T) * act'(h2)
      adj_f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS1 / 4; ++m) {
        const int k0 = adj_k<G::CH1>(B::lg, 4 * m);
        const adj_f4 a0 = *(const lds_f4*)(B::s_a + B::li * G::LDX + k0), a1 = *(const lds_f4*)(B::s_a + (16 + B::li) * G::LDX + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float b = B::s_w3[B::col12 * G::LW3 + k0 + v];
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], b, c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], b, c1, 0, 0, 0);
        }
      }
      float g[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[i] = c0[i] * mlp_act_deriv<ACT>(h2k[i]);
        g[4 + i] = c1[i] * mlp_act_deriv<ACT>(h2k[4 + i]);
        B::s_hA[(4 * B::lg + i) * G::LDH + B::col12] = g[i];
        B::s_hA[(16 + 4 * B::lg + i) * G::LDH + B::col12] = g[4 + i];
      }
      *(g_f4*)(act + (unsigned)(G::OFF_G2 + B::col12 * G::R + 4 * B::lg)) = adj_f4{g[0], g[1], g[2], g[3]};
      *(g_f4*)(act + (unsigned)(G::OFF_G2 + B::col12 * G::R + 16 + 4 * B::lg)) = adj_f4{g[4], g[5], g[6], g[7]};
    }
    __syncthreads();
    if (B::wave < G::NW12) {                                // layer 2 transposed: g1 = (g2 @ W2^T) * act'(h1)
      adj_f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS2 / 4; ++m) {
        const int k0 = adj_k<G::CH2>(B::lg, 4 * m);
        const adj_f4 a0 = *(const lds_f4*)(B::s_hA + B::li * G::LDH + k0), a1 = *(const lds_f4*)(B::s_hA + (16 + B::li) * G::LDH + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], B::w2t[4 * m + v], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], B::w2t[4 * m + v], c1, 0, 0, 0);
        }
      }
      float g[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g[i] = c0[i] * mlp_act_deriv<ACT>(h1k[i]);
        g[4 + i] = c1[i] * mlp_act_deriv<ACT>(h1k[4 + i]);
        B::s_hB[(4 * B::lg + i) * G::LDH + B::col12] = g[i];
        B::s_hB[(16 + 4 * B::lg + i) * G::LDH + B::col12] = g[4 + i];
      }
      *(g_f4*)(act + (unsigned)(G::OFF_G1 + B::col12 * G::R + 4 * B::lg)) = adj_f4{g[0], g[1], g[2], g[3]};
      *(g_f4*)(act + (unsigned)(G::OFF_G1 + B::col12 * G::R + 16 + 4 * B::lg)) = adj_f4{g[4], g[5], g[6], g[7]};
    }
    __syncthreads();
    if (B::wave < G::NW3) {                                 // layer 1 transposed: v = g1 @ W1^T
      const int rb = B::wave / G::CB;
      adj_f4 c = {0, 0, 0, 0};
#pragma unroll
      for (int m = 0; m < KS2 / 4; ++m) {
        const int k0 = adj_k<G::CH2>(B::lg, 4 * m);
        const adj_f4 a = *(const lds_f4*)(B::s_hB + (16 * rb + B::li) * G::LDH + k0);
#pragma unroll
        for (int v = 0; v < 4; ++v) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[v], B::s_w1[B::col * G::LW1 + k0 + v], c, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) v4[i] = c[i];
    }
  }
};

// Step n of the reverse sweep for the workgroup's tiles k0 .. k0 + cnt - 1 (counted in ITS tiles): lambda_{n+1} -> lambda_n in D.lam, the
// activations of every stage at scratch item blockIdx.x * chunk + (k - k0).  The bias shifts of the stages are those disc_prepare left
// in DiscLds.
template <int DP, int HP, int ACT>
__device__ __attribute__((noinline)) void disc_tile_pass(const DiscArgs* D_, unsigned smem, int n, int k0, int cnt) {
  using G = AdjGeom<DP, HP>;
  constexpr int MS = kDiscMaxStages;
  const MI_CONST DiscArgs& D = *(const MI_CONST DiscArgs*)uniform_p(D_);     // scalar loads
  smem = (unsigned)__builtin_amdgcn_readfirstlane((int)smem);
  n = __builtin_amdgcn_readfirstlane(n); k0 = __builtin_amdgcn_readfirstlane(k0); cnt = __builtin_amdgcn_readfirstlane(cnt);
  const MI_CONST StepArgs& SA = D.a.p.s;
  DiscCtx<DP, HP, ACT> cx;
  cx.bind(SA.rhs, SA.dim, smem);
  cx.load_w2(SA.rhs);
  const int d = cx.d, col = cx.col, rbase = cx.rbase, S = D.S;
  const bool owner = cx.owner;
  const long long npl = SA.batch * (long long)d;
  const g_float* const yn = (const g_float*)D.ys + (long long)n * npl;
  const g_float* const gn = (const g_float*)D.gys + (long long)n * npl;
  const g_float* const glast = (const g_float*)D.gys + (long long)(D.N - 1) * npl;
  g_float* const lam = (g_float*)D.lam;
  g_float* const act_base = (g_float*)D.a.act;
  const bool first = n == D.N - 2;                          // lambda_{N-1} is the output gradient at the last grid point
  float hs = D.h[n];
  asm volatile("" : "+v"(hs));
  for (int k = k0; k < k0 + cnt; ++k) {
    const long long tile_i = blockIdx.x + (long long)k * gridDim.x;
    const long long row0 = tile_i * G::R;
    g_float* const act_tile = act_base + ((long long)blockIdx.x * D.chunk + (k - k0)) * (long long)(4 * G::SLOT);
    const long long ebase = row0 * d;
    unsigned eo[4];
    bool ok[4];
    float y0e[4], lm[4], ky[MS][4] = {}, yb[MS][4] = {};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      eo[i] = (unsigned)((rbase + i) * d + col);
      ok[i] = owner && row0 + rbase + i < SA.batch;
      y0e[i] = ok[i] ? (yn + ebase)[eo[i]] : 0.f;
      lm[i] = ok[i] ? (first ? (glast + ebase)[eo[i]] : (lam + ebase)[eo[i]]) : 0.f;
    }
#pragma unroll
    for (int s = 0; s < MS; ++s) {                          // forward: the stages from the checkpoint (rk_common.py:50-51 order of operations)
      if (s < S) {
        float xs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < s; ++j) acc = j == 0 ? (hs * D.ha[s][0]) * ky[0][i] : acc + (hs * D.ha[s][j]) * ky[j][i];
          xs[i] = s == 0 ? y0e[i] : y0e[i] + acc;
        }
        cx.fwd(xs, ky[s], act_tile + (long long)s * G::SLOT, s);
      }
    }
#pragma unroll
    for (int s = MS - 1; s >= 0; --s) {                     // backward: kbar_s from lambda_{n+1} and the later stages' Ybar
      if (s < S) {
        float kb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float acc = (hs * D.hb[s]) * lm[i];
#pragma unroll
          for (int j = s + 1; j < MS; ++j)
            if (j < S) acc = acc + (hs * D.ha[j][s]) * yb[j][i];
          kb[i] = acc;
        }
        cx.bwd(kb, yb[s], act_tile + (long long)s * G::SLOT);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ok[i]) {
        float v = lm[i];
#pragma unroll
        for (int s = 0; s < MS; ++s)
          if (s < S) v = v + yb[s][i];
        (lam + ebase)[eo[i]] = v + (gn + ebase)[eo[i]];
      }
    }
    __syncthreads();                                        // the LDS tiles are the weight-gradient pass's staging area
  }
}

// Before the passes of step n: the pass list of the weight-gradient pass (ntile tiles, every stage with coefficient 1 and its time) and
// the bias shifts of the tile pass.  Every thread of the workgroup must call it; ends with a barrier.
template <int DP, int HP>
__device__ __attribute__((noinline)) void disc_prepare(const DiscArgs* D_, unsigned smem, unsigned ash_off, int n, int cnt, int accum) {
  const MI_CONST DiscArgs& D = *(const MI_CONST DiscArgs*)uniform_p(D_);     // scalar loads
  lds_AdjShared* const ash = (lds_AdjShared*)(size_t)__builtin_amdgcn_readfirstlane((int)ash_off);
  lds_float* const s_tw = (lds_float*)(size_t)__builtin_amdgcn_readfirstlane((int)smem) + DiscLds<DP, HP>::OFF_TW;
  n = __builtin_amdgcn_readfirstlane(n); cnt = __builtin_amdgcn_readfirstlane(cnt); accum = __builtin_amdgcn_readfirstlane(accum);
  const int S = D.S, hd = D.a.p.s.rhs.hidden;
  float ts[kDiscMaxStages];
  disc_stage_times(D, n, ts);
  if (threadIdx.x == 0) {
    MI_LDS AdjWList& L = ash->wl[0];
    L.n = S;
#pragma unroll
    for (int q = 0; q < kDiscMaxStages; ++q)
      if (q < S) { L.slot[q] = q; L.c[0][q] = 1.f; L.c[1][q] = 0.f; L.ts[q] = ts[q]; }
    L.ntile = cnt; L.cap = D.chunk; L.accum = accum;
  }
  if (D.a.td) {
    const g_float* const wt = (const g_float*)D.a.p.s.rhs.w[0];            // row 0 of the time-dependent W1
    for (int c = threadIdx.x; c < HP; c += blockDim.x) {
      const float w = c < hd ? wt[c] : 0.f;
#pragma unroll
      for (int q = 0; q < kDiscMaxStages; ++q)
        if (q < S) s_tw[q * HP + c] = ts[q] * w;
    }
  }
  __syncthreads();
}

template <int DP, int HP, int ACT>
__global__ __launch_bounds__((64 * AdjGeom<DP, HP>::NW)) void k_discrete_mlp(const DiscArgs* __restrict__ Dp) {
  using G = AdjGeom<DP, HP>;
  using SH = PersistSharedT<kPersistMaxGrid, 8>;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ SH sh;
  __shared__ AdjShared ash_;
  const DiscArgs& D = *Dp;
  const AdjArgs& A = D.a;
  const AdjArgs* const Ap = &Dp->a;
  const unsigned smem = (unsigned)(size_t)(MI_LDS char*)smem_raw;
  const unsigned ash_off = (unsigned)(size_t)(MI_LDS AdjShared*)&ash_;
  const StepArgs& SA = A.p.s;
  {
    AdjCtx<DP, HP, ACT> cx;
    cx.bind(SA.rhs, SA.dim, smem);
    cx.stage_weights(SA.rhs);
  }
  lds_float* const slice_scratch = (lds_float*)(size_t)smem + (DP * G::LW1 + HP * G::LW3);
  for (int i = threadIdx.x; i < kDiscMaxStages * HP; i += blockDim.x) ((lds_float*)(size_t)smem)[DiscLds<DP, HP>::OFF_TW + i] = 0.f;
  if (threadIdx.x == 0) sh.ok = 1;
  __syncthreads();
  unsigned gen = 0;
  double r[5];
  Acc none;
  bool ok = grid_reduce_rank(A.p, none, sh, gen++, r);      // residency check: every workgroup of the grid runs
  long long prof[3] = {0, 0, 0};
  if (ok) {
    const long long ntiles = (SA.batch + G::R - 1) / G::R;
    const int my_tiles = (long long)blockIdx.x < ntiles ? (int)((ntiles - 1 - blockIdx.x) / gridDim.x + 1) : 0;
    bool accum = false;
    for (int k0 = 0; k0 < my_tiles; k0 += D.chunk) {
      const int cnt = my_tiles - k0 < D.chunk ? my_tiles - k0 : D.chunk;
      for (int n = D.N - 2; n >= 0; --n) {
        disc_prepare<DP, HP>(Dp, smem, ash_off, n, cnt, accum ? 1 : 0);
        const long long tk0 = (long long)wall_clock64();
        disc_tile_pass<DP, HP, ACT>(Dp, smem, n, k0, cnt);
        const long long tk1 = (long long)wall_clock64();
        adj_wgrad_pass<DP, HP, 1, true>(Ap, smem, ash_off, 0, 0);
        prof[0] += tk1 - tk0; prof[1] += (long long)wall_clock64() - tk1;
        accum = true;
      }
    }
    const long long tk2 = (long long)wall_clock64();
    ok = grid_reduce_rank(A.p, none, sh, gen++, r);         // every workgroup's partial block is complete (written through before its record)
    if (ok) adj_slice<1>(A, slice_scratch, [&](int p, const float* s) { D.th_out[p] = s[0]; });
    prof[2] = (long long)wall_clock64() - tk2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    DiscResult res;
    res.status = ok ? 0u : (unsigned)MI_ODE_ST_SYNC_TIMEOUT; res.handoffs = (int)gen;
    for (int i = 0; i < 3; ++i) res.prof[i] = prof[i];
    const long long* src = (const long long*)&res;
    long long* dst = (long long*)D.res;
    for (int i = 0; i < (int)(sizeof(DiscResult) / sizeof(long long)); ++i)
      __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace mi
