// The exact gradient of a fixed-grid Runge-Kutta solve of the ODEFunc MLP in FLOAT64, time dependent or not: the float64 twin of
// k_discrete_mlp (csrc/mi_ode_discrete.h - same recursion, same per-step schedule, same determinism), all steps in ONE launch.
//
//     kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j,     Ybar_i = (df/dy at Y_i)^T kbar_i,     theta_bar += (df/dtheta at Y_i)^T kbar_i
//     lambda_n = lambda_{n+1} + sum_i Ybar_i + gbar_n
//
// The operand plan is that of the float64 forward (csrc/mi_ode_mlp64.h), not that of the float32 adjoint core: a 32-row tile per
// workgroup, ONE physical wavefront per SIMD playing V virtual wavefronts (all 512 registers), the layers as chains of
// v_mfma_f64_16x16x4_f64, activations through LDS (x, a, hA, hB tiles: 100 KB at 64 x 128) - and the weights are NOT resident: 64-128-128-64
// in float64 is 264 KB, so they are streamed from packed copies in global memory, in BOTH orientations: the forward pack of k_mlp64_pack
// and a transposed pack with the same slot function and the roles of K and N swapped (W3^T as [DP -> HP], W2^T, W1^T as [HP -> DP]:
// k_mlp64_pack_t).  Both are refreshed in front of every launch (weights change between training steps).  A slice's first chunk is
// requested before the barrier its layer waits at; inside a chain the next chunk is in flight under the current one.
//
// Per step and tile (a workgroup owns its tiles for the whole sweep, lambda lives in the caller's grad_y0 buffer between steps):
//   1. the <= 4 stages are recomputed from the checkpoint y_n (rk_common's order of operations, the stage times formed in double by the
//      forward's own expressions); X = Y_i, H1, H2 of each stage go to scratch slot i, [column][32 rows];
//   2. the transposed passes run in reverse stage order; kbar_i and Ybar_i stay in registers, A = kbar_i, G2, G1 go to the same slot.  The
//      activation derivative is taken from the activation output (softplus' = -expm1(-h): no cancellation at small h);
//   3. after `chunk` tiles ONE weight-gradient pass X^T Delta on the f64 MFMA (K = 32 rows x stages x chunk), the three products one
//      after another (32 accumulator doubles per lane at most), accumulators added to this workgroup's own partial block.
// Within a slot the 32 rows of a column are stored in accumulator order - row 16 rb + lg + 4 i at position 16 rb + 4 lg + i - so that a
// lane writes its four values with one 32-byte store; every plane uses the same permutation and the weight-gradient products sum over
// rows, so the order only has to be the same on both operands.
// The bias gradients are column sums of G1, G2 and A, the w_t gradient sum t_i colsum(G1): a lane sums its own rows, two lane exchanges
// complete the column, and the running sums stay in registers for the whole sweep (carried from chunk to chunk like the others).
// At the end ONE grid hand-off (grid_reduce_rank, bounded spin, MI_ODE_ST_SYNC_TIMEOUT), then every workgroup folds its 1 / G slice of
// theta_bar over the workgroups in a fixed order (adj_slice's structure in double): no atomics, two runs give identical bits.
#pragma once
#include "mi_ode_discrete.h"
#include "mi_ode_mlp64.h"

namespace mi {

#ifndef MI_D64_CHUNK
#define MI_D64_CHUNK 4
#endif
constexpr int kD64Chunk = MI_D64_CHUNK;                      // k-pairs of a weight slice per request

struct Disc64Args {
  PersistArgs p;               // hand-off plumbing (p.s.partials, sequence numbers, spin bounds), shape (p.s.batch, p.s.dim, p.s.rhs.hidden)
  const double* ys;            // [N, batch, dim] the forward solution
  const double* gys;           // [N, batch, dim] gradient of the loss with respect to it
  double* lam;                 // [batch, dim] lambda; on return grad_y0
  double* th_out;              // [P] canonical order
  const double* pack;          // MlpGeom64 pack of this call's weights (k_mlp64_pack)
  const double* pack_t;        // ... and of their transposes (k_mlp64_pack_t)
  double* act;                 // [grid][chunk][4][SLOT] activation scratch
  double* wpart;               // [grid][PP] weight-gradient partials, padded layout (DiscGeom64)
  DiscResult* res;
  int N, S, chunk, td;         // grid points, stages, tiles per weight-gradient pass, time-dependent first layer
  int P, SL;                   // parameters, slice of the fold per workgroup
  double ha[kDiscMaxStages][kDiscMaxStages];   // a_ij (row i, j < i)
  double hb[kDiscMaxStages];
  double tn[kDiscMaxStages], tdn[kDiscMaxStages];   // stage i is evaluated at t[n] + (h tn[i]) / tdn[i] (stage 0 at t[n])
  double h[kDiscMaxSteps];     // t[n + 1] - t[n]
  double t0[kDiscMaxSteps];    // t[n]
};

template <int DP, int HP>
struct DiscGeom64 {
  using G = MlpGeom64<DP, HP>;
  static constexpr int R = 32;
  // a scratch slot: six planes [column][32 rows]
  static constexpr int OFF_X = 0, OFF_H1 = R * DP, OFF_H2 = OFF_H1 + R * HP, OFF_A = OFF_H2 + R * HP, OFF_G2 = OFF_A + R * DP,
                       OFF_G1 = OFF_G2 + R * HP;
  static constexpr int SLOT = R * (2 * DP + 4 * HP);
  // a workgroup's partial block: W1 [DP][HP] | W2 [HP][HP] | W3 [HP][DP] | w_t [HP] | b1 [HP] | b2 [HP] | b3 [2 row blocks][DP]
  static constexpr int PW1 = 0, PW2 = DP * HP, PW3 = PW2 + HP * HP, PWT = PW3 + HP * DP, PB1 = PWT + HP, PB2 = PB1 + HP, PB3 = PB2 + HP;
  static constexpr int PP = PB3 + 2 * DP;
  static constexpr size_t lds_bytes() { return (size_t)R * (2 * G::LDX + 2 * G::LDH) * sizeof(double); }
};

// The transposed weights of this call -> a pack with k_mlp64_pack's slot function (element (block, s, lane): k = lg * KS + s,
// column = 16 * block + li): W3^T where the forward pack keeps W1 ([DP -> HP]), W2^T where it keeps W2, W1^T (without the row of t)
// where it keeps W3 ([HP -> DP]).  The w_t row, the biases and the padding are zero.
template <int DP, int HP>
__global__ __launch_bounds__(256) void k_mlp64_pack_t(RhsParams rhs, int d, double* pack) {
  using G = MlpGeom64<DP, HP>;
  const int hd = rhs.hidden;
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x), nt = (int)(gridDim.x * blockDim.x);
  const double* W1 = (const double*)rhs.w[0];
  const double* W2 = (const double*)rhs.w[1];
  const double* W3 = (const double*)rhs.w[2];
  const int td = rhs.s[1] != 0.0 ? 1 : 0;
  auto slot = [](int blk, int KS, int s, int lane) { return ((blk * (KS / 2) + (s >> 1)) * 64 + lane) * 2 + (s & 1); };
  for (int e = tid; e < G::NW12 * G::KS1 * 64; e += nt) {
    const int lane = e & 63, s = (e >> 6) % G::KS1, w = (e >> 6) / G::KS1;
    const int k = (lane >> 4) * G::KS1 + s, c = 16 * w + (lane & 15);
    pack[G::OFF_W1 + slot(w, G::KS1, s, lane)] = (k < d && c < hd) ? W3[(long long)c * d + k] : 0.0;
  }
  for (int e = tid; e < G::NW12 * G::KS2 * 64; e += nt) {
    const int lane = e & 63, s = (e >> 6) % G::KS2, w = (e >> 6) / G::KS2;
    const int k = (lane >> 4) * G::KS2 + s, c = 16 * w + (lane & 15);
    pack[G::OFF_W2 + slot(w, G::KS2, s, lane)] = (k < hd && c < hd) ? W2[(long long)c * hd + k] : 0.0;
  }
  for (int e = tid; e < G::CB3 * G::KS2 * 64; e += nt) {
    const int lane = e & 63, s = (e >> 6) % G::KS2, cb = (e >> 6) / G::KS2;
    const int k = (lane >> 4) * G::KS2 + s, c = 16 * cb + (lane & 15);
    pack[G::OFF_W3 + slot(cb, G::KS2, s, lane)] = (k < hd && c < d) ? W1[(long long)(c + td) * hd + k] : 0.0;
  }
  for (int c = tid; c < HP; c += nt) { pack[G::OFF_WT + c] = 0.0; pack[G::OFF_B1 + c] = 0.0; pack[G::OFF_B2 + c] = 0.0; }
  for (int c = tid; c < DP; c += nt) pack[G::OFF_B3 + c] = 0.0;
}

// d act / d z from the activation's OUTPUT h (mlp_act_deriv in double): tanh' = 1 - h^2, relu' = [h > 0], softplus' = 1 - e^{-h}.
template <int ACT>
__device__ __forceinline__ double mlp64_act_deriv(double h) {
  if constexpr (ACT == MLP_ACT_TANH) return 1.0 - h * h;
  else if constexpr (ACT == MLP_ACT_RELU) return h > 0.0 ? 1.0 : 0.0;
  else return -expm1(-h);
}

// The times the network sees at the stages of step n (disc_stage_times in double): k_fixed_mlp64's te + dt / 3.0, te + dt * 2.0 / 3.0,
// te + dt; fixed_grid.py's t + dt / 2.  Zeros for the time-independent network.
__device__ __forceinline__ void disc64_stage_times(const Disc64Args& D, int n, double* ts) {
  const double t0 = D.t0[n], hn = D.h[n];
#pragma unroll
  for (int q = 0; q < kDiscMaxStages; ++q) ts[q] = (!D.td || q >= D.S) ? 0.0 : q == 0 ? t0 : t0 + (hn * D.tn[q]) / D.tdn[q];
}

// The partials cross workgroups (and XCDs) inside the kernel: agent-scope stores and loads, the recipe of the float32 sweep.
__device__ __forceinline__ void d64_store_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double d64_load_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// NC chunks of CH k-pairs of one slice: chunk h + 1 is requested before the chain of chunk h runs.  w0 holds chunk 0 (requested by the caller).
template <int CH, int NC, bool TWO>
__device__ __forceinline__ void d64_run(const double* a0p, const double* a1p, const mlp_d2* wp, mlp_d2* w0, mlp_d4& c0, mlp_d4& c1) {
  mlp_d2 w1[CH];
#pragma unroll
  for (int h = 0; h < NC; ++h) {
    if (h + 1 < NC) mlp64_load<CH>(wp + (h + 1) * CH * 64, (h & 1) ? w0 : w1);
    mlp64_chain<CH, TWO>(a0p + 2 * CH * h, a1p + 2 * CH * h, (h & 1) ? w1 : w0, c0, c1);
  }
}

__device__ __forceinline__ double d64_sum4(const mlp_d4& c) { return (c[0] + c[1]) + (c[2] + c[3]); }
// the sum over the four lane groups of a column (every lane of the column ends with the same bits)
__device__ __forceinline__ double d64_colsum(double t) {
  t += __shfl_xor(t, 16, 64);
  t += __shfl_xor(t, 32, 64);
  return t;
}

// One product X^T Delta of the weight-gradient pass over `cnt` tiles x S stages: X the plane at xoff (its row blocks IB0 .. IB0 + NIB - 1,
// 16 columns each), Delta the plane at doff (16 NOB columns).  A wavefront owns the output column blocks wave, wave + NW, .. and the NIB
// row blocks; its accumulators are added to the matrix at `part` of this workgroup's partial block (row stride ldp; accum: it holds
// earlier passes).
template <int DP, int HP, int NIB, int NOB, int IB0>
__device__ __forceinline__ void d64_wgrad_product(const double* act_wg, int xoff, int doff, int cnt, int S, double* part, int ldp, bool accum) {
  using DG = DiscGeom64<DP, HP>;
  constexpr int NW = MlpGeom64<DP, HP>::NW;
  constexpr int NOBW = NOB >= NW ? NOB / NW : 1;
  static_assert(NOB < NW || NOB % NW == 0, "column blocks are dealt evenly");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lg = lane >> 4;
  if (NOB < NW && wave >= NOB) return;
  mlp_d4 acc[NIB][NOBW];
#pragma unroll
  for (int a = 0; a < NIB; ++a)
#pragma unroll
    for (int b = 0; b < NOBW; ++b) acc[a][b] = mlp_d4{0, 0, 0, 0};
  for (int k = 0; k < cnt; ++k) {
    for (int s = 0; s < S; ++s) {
      const double* slot = act_wg + ((long long)k * kDiscMaxStages + s) * DG::SLOT;
      const double* xp = slot + xoff + (16 * IB0 + li) * 32 + lg * 8;
      const double* dp = slot + doff + (16 * wave + li) * 32 + lg * 8;
#pragma unroll
      for (int q = 0; q < 4; ++q) {                          // k-pairs of the tile: lane group lg holds positions 8 lg .. 8 lg + 7
        mlp_d2 xa[NIB], db[NOBW];
#pragma unroll
        for (int a = 0; a < NIB; ++a) xa[a] = *(const mlp_d2*)(xp + a * 16 * 32 + 2 * q);
#pragma unroll
        for (int b = 0; b < NOBW; ++b) db[b] = *(const mlp_d2*)(dp + b * NW * 16 * 32 + 2 * q);
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int a = 0; a < NIB; ++a)
#pragma unroll
            for (int b = 0; b < NOBW; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[a][e], db[b][e], acc[a][b], 0, 0, 0);
      }
    }
  }
  // accumulator element i of block (a, b): row 16 (IB0 + a) + lg + 4 i (input unit), column 16 (wave + NW b) + li (output unit)
#pragma unroll
  for (int a = 0; a < NIB; ++a)
#pragma unroll
    for (int b = 0; b < NOBW; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double* p = part + (16 * (IB0 + a) + lg + 4 * i) * ldp + 16 * (wave + NW * b) + li;
        d64_store_agent(p, accum ? d64_load_agent(p) + acc[a][b][i] : acc[a][b][i]);
      }
}

// The weight-gradient pass of a chunk: the three products one after another, W2's in two halves (at most 32 accumulator doubles per
// lane).  A function of its own - one register allocation, apart from the tile pass's.  Every thread of the workgroup must call it.
template <int DP, int HP>
__device__ __attribute__((noinline)) void disc64_wgrad_pass(const double* act_wg, int cnt, int S, double* part, int accum_) {
  using DG = DiscGeom64<DP, HP>;
  constexpr int HB = HP / 16, CB = DP / 16, H2 = HB > 1 ? HB / 2 : 1;
  act_wg = uniform_p(act_wg); part = uniform_p(part);
  cnt = __builtin_amdgcn_readfirstlane(cnt); S = __builtin_amdgcn_readfirstlane(S);
  const bool accum = __builtin_amdgcn_readfirstlane(accum_) != 0;
  d64_wgrad_product<DP, HP, H2, HB, 0>(act_wg, DG::OFF_H1, DG::OFF_G2, cnt, S, part + DG::PW2, HP, accum);
  if constexpr (HB > 1) d64_wgrad_product<DP, HP, H2, HB, H2>(act_wg, DG::OFF_H1, DG::OFF_G2, cnt, S, part + DG::PW2, HP, accum);
  d64_wgrad_product<DP, HP, CB, HB, 0>(act_wg, DG::OFF_X, DG::OFF_G1, cnt, S, part + DG::PW1, HP, accum);
  d64_wgrad_product<DP, HP, HB, CB, 0>(act_wg, DG::OFF_H2, DG::OFF_A, cnt, S, part + DG::PW3, DP, accum);
}

template <int DP, int HP, int ACT>
struct Disc64Ctx {
  using G = MlpGeom64<DP, HP>;
  using DG = DiscGeom64<DP, HP>;
  static constexpr int V = G::V, NW = G::NW, KS1 = G::KS1, KS2 = G::KS2;
  double *s_x, *s_a, *s_hA, *s_hB;
  const double *pack, *pack_t;
  int lane, wave, li, lg, d;
  // running column sums (bias and w_t gradients), per virtual wavefront: this lane's hidden column 16 vw + li / state column col(v)
  double sb1[V], sb2[V], swt[V], sb3[V];

  __device__ __forceinline__ int vw(int v) const { return wave + v * NW; }
  __device__ __forceinline__ int col(int v) const { return 16 * (vw(v) % G::CB3) + li; }
  __device__ __forceinline__ int rb(int v) const { return vw(v) / G::CB3; }
  __device__ __forceinline__ int row_of(int v, int i) const { return 16 * rb(v) + lg + 4 * i; }
  __device__ __forceinline__ bool owner(int v) const { return vw(v) < G::NW3 && col(v) < d; }

  __device__ __forceinline__ void init(const Disc64Args& D, char* smem) {
    s_x = (double*)smem;
    s_a = s_x + G::R * G::LDX;
    s_hA = s_a + G::R * G::LDX;
    s_hB = s_hA + G::R * G::LDH;
    lane = threadIdx.x & 63; wave = threadIdx.x >> 6; li = lane & 15; lg = lane >> 4;
    d = D.p.s.dim;
    pack = D.pack; pack_t = D.pack_t;
#pragma unroll
    for (int v = 0; v < V; ++v) sb1[v] = sb2[v] = swt[v] = sb3[v] = 0.0;
  }

  // [32 x 4 KS] rows of src times the slices of a layer with HP outputs: virtual wavefront vw < NW12 owns 16 columns and both row blocks.
  // epi(v, column, c0, c1).  The barrier in front of the chains is the one src is complete at.
  template <int KS, class Epi>
  __device__ __forceinline__ void wide(const double* src, int ld, const double* wl, Epi&& epi) {
    constexpr int P = KS / 2, CH = P >= kD64Chunk ? kD64Chunk : P, NC = P / CH;
    mlp_d2 wf[V][CH];
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (vw(v) < G::NW12) mlp64_load<CH>((const mlp_d2*)wl + (vw(v) * P) * 64 + lane, wf[v]);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW12) {
        mlp_d4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
        d64_run<CH, NC, true>(src + li * ld + lg * KS, src + (16 + li) * ld + lg * KS, (const mlp_d2*)wl + (vw(v) * P) * 64 + lane, wf[v], c0, c1);
        epi(v, 16 * vw(v) + li, c0, c1);
      }
    }
  }
  // ... of a layer with DP outputs (input rows in s_hB): virtual wavefront vw < NW3 owns one 16-row block x 16 columns.  epi(v, c).
  template <class Epi>
  __device__ __forceinline__ void narrow(const double* wl, Epi&& epi) {
    constexpr int P = KS2 / 2, CH = P >= kD64Chunk ? kD64Chunk : P, NC = P / CH;
    mlp_d2 wf[V][CH];
#pragma unroll
    for (int v = 0; v < V; ++v)
      if (vw(v) < G::NW3) mlp64_load<CH>((const mlp_d2*)wl + ((vw(v) % G::CB3) * P) * 64 + lane, wf[v]);
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW3) {
        mlp_d4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
        const double* ap = s_hB + (16 * rb(v) + li) * G::LDH + lg * KS2;
        d64_run<CH, NC, false>(ap, ap, (const mlp_d2*)wl + ((vw(v) % G::CB3) * P) * 64 + lane, wf[v], c0, c1);
        epi(v, c0);
      }
    }
  }
  // the owners' values of a [32 x DP] tile -> LDS rows (zero in the padding columns) and the plane `plane` of the slot
  __device__ __forceinline__ void put(double* s_t, const double (*v4)[4], double* plane) {
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW3) {
        mlp_d4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = col(v) < d ? v4[v][i] : 0.0;
          s_t[row_of(v, i) * G::LDX + col(v)] = o[i];
        }
        *(mlp_d4*)(plane + col(v) * 32 + 16 * rb(v) + 4 * lg) = o;
      }
    }
  }
  // both row blocks of hidden column cc -> LDS and the plane
  __device__ __forceinline__ void put_hidden(double* s_t, double* plane, int cc, const mlp_d4& h0, const mlp_d4& h1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s_t[(lg + 4 * i) * G::LDH + cc] = h0[i];
      s_t[(16 + lg + 4 * i) * G::LDH + cc] = h1[i];
    }
    *(mlp_d4*)(plane + cc * 32 + 4 * lg) = h0;
    *(mlp_d4*)(plane + cc * 32 + 16 + 4 * lg) = h1;
  }

  // f = f(ts, xs) for the tile whose stage inputs are xs; X, H1, H2 go to `slot`.  Every thread of the workgroup must call it.
  __device__ __forceinline__ void fwd(const double (*xs)[4], double (*f)[4], double* slot, double ts) {
    put(s_x, xs, slot + DG::OFF_X);
    wide<KS1>(s_x, G::LDX, pack + G::OFF_W1, [&](int, int cc, const mlp_d4& c0, const mlp_d4& c1) {
      const double b = pack[G::OFF_B1 + cc] + ts * pack[G::OFF_WT + cc];
      mlp_d4 h0, h1;
#pragma unroll
      for (int i = 0; i < 4; ++i) { h0[i] = mlp64_act<ACT>(c0[i] + b); h1[i] = mlp64_act<ACT>(c1[i] + b); }
      put_hidden(s_hA, slot + DG::OFF_H1, cc, h0, h1);
    });
    wide<KS2>(s_hA, G::LDH, pack + G::OFF_W2, [&](int, int cc, const mlp_d4& c0, const mlp_d4& c1) {
      const double b = pack[G::OFF_B2 + cc];
      mlp_d4 h0, h1;
#pragma unroll
      for (int i = 0; i < 4; ++i) { h0[i] = mlp64_act<ACT>(c0[i] + b); h1[i] = mlp64_act<ACT>(c1[i] + b); }
      put_hidden(s_hB, slot + DG::OFF_H2, cc, h0, h1);
    });
    narrow(pack + G::OFF_W3, [&](int v, const mlp_d4& c) {
      const double b = pack[G::OFF_B3 + col(v)];
#pragma unroll
      for (int i = 0; i < 4; ++i) f[v][i] = c[i] + b;
    });
  }

  // yb = as^T df/dy at the stage whose activations fwd() left in `slot`; A = as, G2, G1 go to the same slot, their column sums to the
  // running bias sums (ts: the stage's time, the weight of colsum(G1) in the w_t gradient).  Every thread of the workgroup must call it.
  __device__ __forceinline__ void bwd(const double (*as)[4], double (*yb)[4], double* slot, double ts) {
    mlp_d4 h1k[V][2], h2k[V][2];                             // this lane's own activations of the stage (it wrote them itself)
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW12) {
        const int cc = 16 * vw(v) + li;
        h1k[v][0] = *(const mlp_d4*)(slot + DG::OFF_H1 + cc * 32 + 4 * lg); h1k[v][1] = *(const mlp_d4*)(slot + DG::OFF_H1 + cc * 32 + 16 + 4 * lg);
        h2k[v][0] = *(const mlp_d4*)(slot + DG::OFF_H2 + cc * 32 + 4 * lg); h2k[v][1] = *(const mlp_d4*)(slot + DG::OFF_H2 + cc * 32 + 16 + 4 * lg);
      }
    }
    put(s_a, as, slot + DG::OFF_A);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW3) {
        const double t = col(v) < d ? (as[v][0] + as[v][1]) + (as[v][2] + as[v][3]) : 0.0;
        sb3[v] += d64_colsum(t);
      }
    }
    wide<KS1>(s_a, G::LDX, pack_t + G::OFF_W1, [&](int v, int cc, const mlp_d4& c0, const mlp_d4& c1) {     // g2 = (a @ W3^T) * act'(h2)
      mlp_d4 g0, g1;
#pragma unroll
      for (int i = 0; i < 4; ++i) { g0[i] = c0[i] * mlp64_act_deriv<ACT>(h2k[v][0][i]); g1[i] = c1[i] * mlp64_act_deriv<ACT>(h2k[v][1][i]); }
      put_hidden(s_hA, slot + DG::OFF_G2, cc, g0, g1);
      sb2[v] += d64_colsum(d64_sum4(g0) + d64_sum4(g1));
    });
    wide<KS2>(s_hA, G::LDH, pack_t + G::OFF_W2, [&](int v, int cc, const mlp_d4& c0, const mlp_d4& c1) {     // g1 = (g2 @ W2^T) * act'(h1)
      mlp_d4 g0, g1;
#pragma unroll
      for (int i = 0; i < 4; ++i) { g0[i] = c0[i] * mlp64_act_deriv<ACT>(h1k[v][0][i]); g1[i] = c1[i] * mlp64_act_deriv<ACT>(h1k[v][1][i]); }
      put_hidden(s_hB, slot + DG::OFF_G1, cc, g0, g1);
      const double t = d64_colsum(d64_sum4(g0) + d64_sum4(g1));
      sb1[v] += t;
      swt[v] += ts * t;
    });
    narrow(pack_t + G::OFF_W3, [&](int v, const mlp_d4& c) {                                                 // Ybar = g1 @ W1^T
#pragma unroll
      for (int i = 0; i < 4; ++i) yb[v][i] = c[i];
    });
  }

  // the running column sums -> this workgroup's partial block (once, after its last step)
  __device__ __forceinline__ void store_sums(double* part) {
    if (lg != 0) return;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (vw(v) < G::NW12) {
        const int cc = 16 * vw(v) + li;
        d64_store_agent(part + DG::PWT + cc, swt[v]);
        d64_store_agent(part + DG::PB1 + cc, sb1[v]);
        d64_store_agent(part + DG::PB2 + cc, sb2[v]);
      }
      if (vw(v) < G::NW3) d64_store_agent(part + DG::PB3 + rb(v) * DP + col(v), sb3[v]);
    }
  }
};

// canonical parameter p (w_t when time dependent, W1 [dim][hidden], b1, W2, b2, W3, b3) -> its place in a partial block; two: the
// entry is the sum of two places DP apart (b3: one per row block)
template <int DP, int HP>
__device__ __forceinline__ int disc64_place(int p, int d, int hd, int td, bool& two) {
  using DG = DiscGeom64<DP, HP>;
  two = false;
  int q = p;
  if (td) { if (q < hd) return DG::PWT + q; q -= hd; }
  if (q < d * hd) return DG::PW1 + (q / hd) * HP + q % hd;
  q -= d * hd;
  if (q < hd) return DG::PB1 + q;
  q -= hd;
  if (q < hd * hd) return DG::PW2 + (q / hd) * HP + q % hd;
  q -= hd * hd;
  if (q < hd) return DG::PB2 + q;
  q -= hd;
  if (q < hd * d) return DG::PW3 + (q / d) * DP + q % d;
  q -= hd * d;
  two = true;
  return DG::PB3 + q;
}

// this workgroup's slice of theta_bar: the partials of all workgroups summed in a fixed order (adj_slice in double): 128 entries at a
// time, thread group q (of blockDim / 128) sums workgroups q, q + groups, .., the groups' sums are folded in order through LDS.
template <int DP, int HP>
__device__ __forceinline__ void disc64_slice(const Disc64Args& D, double* scratch) {
  using DG = DiscGeom64<DP, HP>;
  const int G_ = (int)gridDim.x;
  const int ngroups = (int)blockDim.x / 128, grp = (int)threadIdx.x / 128, el = (int)threadIdx.x % 128;
  const int d = D.p.s.dim, hd = D.p.s.rhs.hidden;
  for (int e0 = 0; e0 < D.SL; e0 += 128) {
    const int e = e0 + el, p = (int)blockIdx.x * D.SL + e;
    const bool live = e < D.SL && p < D.P;
    double s = 0.0;
    if (live) {
      bool two;
      const int at = disc64_place<DP, HP>(p, d, hd, D.td, two);
      const double* wp = D.wpart + at;
      int g = grp;
      for (; g + 7 * ngroups < G_; g += 8 * ngroups) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const double* q = wp + (long long)(g + u * ngroups) * DG::PP;
          v[u] = two ? d64_load_agent(q) + d64_load_agent(q + DP) : d64_load_agent(q);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
      }
      for (; g < G_; g += ngroups) {
        const double* q = wp + (long long)g * DG::PP;
        s += two ? d64_load_agent(q) + d64_load_agent(q + DP) : d64_load_agent(q);
      }
    }
    __syncthreads();                                        // (scratch may still be read by the previous chunk)
    scratch[grp * 128 + el] = s;
    __syncthreads();
    if (grp == 0 && live) {
      double t = 0.0;
      for (int q = 0; q < ngroups; ++q) t += scratch[q * 128 + el];
      D.th_out[p] = t;
    }
  }
}

template <int DP, int HP, int ACT>
__global__ __launch_bounds__((64 * MlpGeom64<DP, HP>::NW)) void k_discrete_mlp64(const Disc64Args* __restrict__ Dp) {
  using G = MlpGeom64<DP, HP>;
  using DG = DiscGeom64<DP, HP>;
  using SH = PersistSharedT<kPersistMaxGrid, 8>;
  constexpr int V = G::V, MS = kDiscMaxStages;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ SH sh;
  const Disc64Args& D = *Dp;
  const StepArgs& SA = D.p.s;
  Disc64Ctx<DP, HP, ACT> cx;
  cx.init(D, smem_raw);
  if (threadIdx.x == 0) sh.ok = 1;
  __syncthreads();
  unsigned gen = 0;
  double r[5];
  Acc none;
  bool ok = grid_reduce_rank(D.p, none, sh, gen++, r);      // residency check: every workgroup of the grid runs
  long long prof[3] = {0, 0, 0};
  if (ok) {
    const int d = cx.d, S = D.S;
    const long long ntiles = (SA.batch + G::R - 1) / G::R;
    const int my_tiles = (long long)blockIdx.x < ntiles ? (int)((ntiles - 1 - blockIdx.x) / gridDim.x + 1) : 0;
    const long long npl = SA.batch * (long long)d;
    const double* const glast = D.gys + (long long)(D.N - 1) * npl;
    double* const act_wg = D.act + (long long)blockIdx.x * D.chunk * (long long)(MS * DG::SLOT);
    double* const part = D.wpart + (long long)blockIdx.x * DG::PP;
    bool accum = false;
    for (int k0 = 0; k0 < my_tiles; k0 += D.chunk) {
      const int cnt = my_tiles - k0 < D.chunk ? my_tiles - k0 : D.chunk;
      for (int n = D.N - 2; n >= 0; --n) {
        const long long tk0 = (long long)wall_clock64();
        double ts[MS];
        disc64_stage_times(D, n, ts);
        const double* const yn = D.ys + (long long)n * npl;
        const double* const gn = D.gys + (long long)n * npl;
        const bool first = n == D.N - 2;                    // lambda_{N-1} is the output gradient at the last grid point
        double hs = D.h[n];
        asm volatile("" : "+v"(hs));
        for (int k = k0; k < k0 + cnt; ++k) {
          const long long tile_i = blockIdx.x + (long long)k * gridDim.x;
          const long long row0 = tile_i * G::R;
          double* const act_tile = act_wg + (long long)(k - k0) * (MS * DG::SLOT);
          const long long ebase = row0 * d;
          unsigned eo[V][4];
          bool okr[V][4];
          double y0e[V][4], lm[V][4], ky[MS][V][4], yb[MS][V][4];
#pragma unroll
          for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              eo[v][i] = (unsigned)(cx.row_of(v, i) * d + cx.col(v));
              okr[v][i] = cx.owner(v) && row0 + cx.row_of(v, i) < SA.batch;
              y0e[v][i] = okr[v][i] ? (yn + ebase)[eo[v][i]] : 0.0;
              lm[v][i] = okr[v][i] ? (first ? (glast + ebase)[eo[v][i]] : (D.lam + ebase)[eo[v][i]]) : 0.0;
#pragma unroll
              for (int s = 0; s < MS; ++s) { ky[s][v][i] = 0.0; yb[s][v][i] = 0.0; }
            }
          }
#pragma unroll
          for (int s = 0; s < MS; ++s) {                    // forward: the stages from the checkpoint (rk_common.py:50-51 order of operations)
            if (s < S) {
              double xs[V][4];
#pragma unroll
              for (int v = 0; v < V; ++v) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  double acc = 0.0;
#pragma unroll
                  for (int j = 0; j < s; ++j) acc = j == 0 ? (hs * D.ha[s][0]) * ky[0][v][i] : acc + (hs * D.ha[s][j]) * ky[j][v][i];
                  xs[v][i] = s == 0 ? y0e[v][i] : y0e[v][i] + acc;
                }
              }
              cx.fwd(xs, ky[s], act_tile + (long long)s * DG::SLOT, ts[s]);
            }
          }
#pragma unroll
          for (int s = MS - 1; s >= 0; --s) {               // backward: kbar_s from lambda_{n+1} and the later stages' Ybar
            if (s < S) {
              double kb[V][4];
#pragma unroll
              for (int v = 0; v < V; ++v) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  double acc = (hs * D.hb[s]) * lm[v][i];
#pragma unroll
                  for (int j = s + 1; j < MS; ++j)
                    if (j < S) acc = acc + (hs * D.ha[j][s]) * yb[j][v][i];
                  kb[v][i] = acc;
                }
              }
              cx.bwd(kb, yb[s], act_tile + (long long)s * DG::SLOT, ts[s]);
            }
          }
#pragma unroll
          for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (okr[v][i]) {
                double vv = lm[v][i];
#pragma unroll
                for (int s = 0; s < MS; ++s)
                  if (s < S) vv = vv + yb[s][v][i];
                (D.lam + ebase)[eo[v][i]] = vv + (gn + ebase)[eo[v][i]];
              }
            }
          }
        }
        __syncthreads();                                    // every wavefront's planes of the chunk are written
        const long long tk1 = (long long)wall_clock64();
        disc64_wgrad_pass<DP, HP>(act_wg, cnt, S, part, accum ? 1 : 0);
        __syncthreads();                                    // the slots are free for the next step
        prof[0] += tk1 - tk0; prof[1] += (long long)wall_clock64() - tk1;
        accum = true;
      }
    }
    const long long tk2 = (long long)wall_clock64();
    cx.store_sums(part);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the partials are written through before this workgroup's record says so
    __syncthreads();
    ok = grid_reduce_rank(D.p, none, sh, gen++, r);         // every workgroup's partial block is complete
    if (ok) disc64_slice<DP, HP>(D, (double*)smem_raw);
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
