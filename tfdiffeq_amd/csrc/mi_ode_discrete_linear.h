// The exact gradient of a fixed-grid Runge-Kutta solve of the linear system f(y) = y W (+ b) (models.LinearODEFunc, rhs.Linear, the lowered
// `y @ W`): the TRANSPOSE of the discrete map k_fixed_linear_mfma computed, all steps in ONE launch, float32 and float64.
//
// Forward step n:  Y_1 = y_n,  Y_i = y_n + h sum_{j<i} a_ij k_j,  k_j = Y_j W + b,  y_{n+1} = y_n + h sum_i b_i k_i.  With lambda_{n+1} = dL/dy_{n+1}
// the reverse step runs, for i = S .. 1,
//     kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j,     Ybar_i = kbar_i W^T,     Wbar += Y_i^T kbar_i,     bbar += sum_rows kbar_i
// and lambda_n = lambda_{n+1} + sum_i Ybar_i + gbar_n - the recursion of csrc/mi_ode_discrete.h with df/dy = W^T and df/dW = Y_i^T (.).
//
// Schedule (every instantiation): BOTH slices resident.  A wavefront owns the 16 columns LinCtx gives it, holds its slice of W (forward
// evaluations) and of W^T (transposed ones) in registers, and accumulates its dim x 16 block of Wbar (D / 16 accumulator tiles of 16 x 16)
// plus one accumulator tile for bbar in registers over all of the workgroup's tiles and steps.  Rows are independent, so a workgroup
// walks each of its 16-row tiles through ALL steps (tile = blockIdx.x, + gridDim.x, ...): lambda of the tile stays in registers from the
// last grid point to the first and grad_y0 is written once; per step the tile costs the loads of y_n and gbar_n (prefetched a step ahead).
// Per step and tile:
//   1. S - 1 forward evaluations (rhs_eval of the W context): stage tile Y_i -> LDS tile i - 1 -> k_i; Y_S is written to its tile directly;
//   2. for i = S .. 1: rhs_eval of the W^T context: kbar_i -> one of two alternating LDS tiles -> Ybar_i; then the weight-gradient MFMAs
//      straight from the two LDS tiles: K = the 16 rows (4 MFMA steps), M = 16 rows of Wbar per accumulator tile (operand Y_i[row][16 m + lane]),
//      N = the wavefront's columns (operand kbar_i[row][col]); bbar: the same B operand against a constant 1;
//   3. one LDS barrier (the next step rewrites tile 0, which the last weight-gradient product read).
// LDS: kDiscMaxStages + 2 = 6 tiles of 16 x (D + VEC).  Rows >= batch of a ragged tile load y, lambda and gbar as zero: their k_j are
// not zero when there is a bias, but their kbar_i are, which keeps them out of Wbar and bbar.  Columns >= dim are zero in both slices.
// At the end: each workgroup stores its partial block [D * D + D] (the layout of k_linadj's gpart) write-through, ONE grid hand-off, then
// every workgroup folds its 1 / G share of the entries over the workgroups in index order: no atomics, two calls give identical bits.  A
// workgroup without tiles stores zeros and takes part in both hand-offs (the first one, right after the slices are loaded, is the residency
// check of every persistent kernel here).
//
// GRID = true (mi_ode_discrete_linear_grid_*): the same sweep for a solve on a grid of its own (options['step_size']) whose outputs were
// interpolated linearly inside the step that reaches them - WITHOUT a stored trajectory.  Per tile, phase A walks forward from y0 over steps
// 0 .. M - 2 (S forward evaluations each: k_S is needed here) and stores y_1 .. y_{M-1} into the workgroup's scratch block [M][16][D]; phase B
// is the reverse loop above with y_n read back from the scratch (y0 for n = 0), and the output gradients placed on the grid as it goes:
// before the stages of step n  lambda += sum_{j: n_j = n} w_j g_j,  after them  lambda_n += sum (1 - w_j) g_j  of the same outputs (in the
// order of j; at n = 0 also g_0).  Ownership: a lane stores element i of a row block at row_of(i) * D + col, where row_of(i) = acc_row(lane, i)
// and col = 16 wave + (lane & 15) are functions of the thread alone (LinCtx::off_of is the same pair with the state's row length) - in
// phase B the SAME thread reads exactly the addresses it wrote, so program order is all the ordering the scratch needs: no fence, no
// hand-off, and the next tile of the workgroup reuses the block.  The scratch does not depend on the batch: grid x M x 16 x D elements.
#pragma once
#include <type_traits>
#include "mi_ode_persist.h"
#include "mi_ode_discrete.h"

namespace mi {

struct DiscLinArgs {
  PersistArgs p;               // hand-off plumbing (p.s.partials, seq_base, spin limits), shape (p.s.batch, p.s.dim), weights (p.s.rhs.w[0], b[0])
  const void* ys;              // [N, batch, dim] the forward solution
  const void* gys;             // [N, batch, dim] gradient of the loss with respect to it
  void* lam;                   // [batch, dim] grad_y0
  void* gw;                    // [dim, dim] in [in, out] layout
  void* gb;                    // [dim] or null
  void* gpart;                 // [G][D * D + D] partial blocks, state dtype
  DiscResult* res;
  int N;                       // grid points
  int S;                       // stages
  int has_bias;
  double ha[kDiscMaxStages][kDiscMaxStages];   // a_ij (row i, j < i)
  double hb[kDiscMaxStages];
  double h[kDiscMaxSteps];     // t[n + 1] - t[n], formed in the state dtype
};

struct DiscLinGridArgs {       // GRID = true: the argument block of the default-grid kernel (ys, gys, N unused: N = M + 1), then the grid's own
  DiscLinArgs a;
  const void* y0;              // [batch, dim]
  const void* gout;            // [n_out, batch, dim] gradient of the loss with respect to the outputs
  void* scratch;               // [G][M][16][D] checkpoints of the workgroup's current tile (slot 0 unused: y_0 is y0)
  int M;                       // grid steps
  int n_out;
  int obeg[kDiscMaxSteps + 1]; // outputs j >= 1 assigned to step n: obeg[n] <= j < obeg[n + 1] (non-decreasing assignment)
  double ow[kDiscMaxSteps + 1];// w_j (state dtype), indexed by output
};

__device__ __forceinline__ const DiscLinArgs& dl_base(const DiscLinArgs* p) { return *p; }
__device__ __forceinline__ const DiscLinArgs& dl_base(const DiscLinGridArgs* p) { return p->a; }

__device__ __forceinline__ void dl_store_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dl_store_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float dl_load_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double dl_load_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, int D>
constexpr size_t discrete_linear_lds_bytes() { return (size_t)(kDiscMaxStages + 2) * LinCtx<T, D>::TILE * sizeof(T); }

template <typename T, int D, bool GRID = false>
__global__ __launch_bounds__(D * 4) void k_discrete_linear(const typename std::conditional<GRID, DiscLinGridArgs, DiscLinArgs>::type* __restrict__ Ap) {
  using CX = LinCtx<T, D>;
  using TR = MfmaTraits<T>;
  using acc_t = typename TR::acc_t;
  using SH = PersistSharedT<kPersistMaxGrid, 8>;
  constexpr int MS = kDiscMaxStages, R_ = CX::R_, LD = CX::LD, TILE = CX::TILE, NB = D / 16, E = D * D + D;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ SH sh;
  const DiscLinArgs& A = dl_base(Ap);
  T* const tiles = (T*)smem_raw;                              // [MS + 2][R_][LD]: Y_1 .. Y_S, then the two kbar tiles
  const int dim = A.p.s.dim, S = A.S, N = A.N;
  const long long batch = A.p.s.batch;
  const bool has_bias = A.has_bias != 0;
  CX fw, bw;
  fw.init_matrix((const T*)A.p.s.rhs.w[0], has_bias ? (const T*)A.p.s.rhs.b[0] : nullptr, 1.0, false, tiles, dim);
  bw.init_matrix((const T*)A.p.s.rhs.w[0], nullptr, 1.0, true, tiles, dim);
  const int lane = fw.lane, li = fw.li, lg = fw.lg, col = fw.col;
  if (threadIdx.x == 0) sh.ok = 1;
  __syncthreads();
  unsigned gen = 0;
  double r[5];
  Acc none;
  bool ok = grid_reduce_rank(A.p, none, sh, gen++, r);        // residency check: every workgroup of the grid runs
  long long prof[3] = {0, 0, 0};
  if (ok) {
    const long long tk0 = (long long)wall_clock64();
    acc_t wg[NB], bg = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < NB; ++m) wg[m] = acc_t{0, 0, 0, 0};
    T ca[MS][MS], cb[MS];                                     // the tableau in the state dtype (uniform: scalar registers)
#pragma unroll
    for (int i = 0; i < MS; ++i) {
      cb[i] = (T)A.hb[i];
#pragma unroll
      for (int j = 0; j < MS; ++j) ca[i][j] = (T)A.ha[i][j];
    }
    const long long ntiles = (batch + R_ - 1) / R_;
    const long long npl = batch * (long long)dim;             // elements of one grid point
    const T* const ys = (const T*)A.ys;
    const T* const gys = (const T*)A.gys;
    T* const lam = (T*)A.lam;
    for (long long tile_i = blockIdx.x; tile_i < ntiles; tile_i += gridDim.x) {
      const long long ebase = tile_i * R_ * dim;
      const int nr = fw.rows_here(tile_i, batch);
      unsigned eo[4];
      bool live[4];
      T lm[4], yn[4], gn[4];
      [[maybe_unused]] unsigned so[4];                        // GRID: this thread's elements inside a slot of the scratch block
      [[maybe_unused]] T* scr = nullptr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        eo[i] = fw.off_of(i);
        live[i] = fw.colok && fw.row_of(i) < nr;
      }
      if constexpr (GRID) {
        // phase A: the checkpoints y_1 .. y_{M-1} of this tile, forward from y0 (evaluations alternate between tiles 0 and 1: one barrier each)
        const T* const y0p = (const T*)Ap->y0 + ebase;
        scr = (T*)Ap->scratch + (long long)blockIdx.x * (long long)(N - 1) * (R_ * D);
        T yc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          so[i] = (unsigned)(fw.row_of(i) * D + col);
          yc[i] = live[i] ? y0p[eo[i]] : (T)0;
        }
        fw.s_ys = tiles; fw.cur = 0;
        for (int n = 0; n + 2 < N; ++n) {
          const T hs = (T)A.h[n];
          T kf[MS][4] = {};
#pragma unroll
          for (int s = 0; s < MS; ++s) {
            if (s < S) {
              T xs[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                T a_ = (T)0;
#pragma unroll
                for (int j = 0; j < s; ++j) a_ = j == 0 ? (hs * ca[s][0]) * kf[0][i] : a_ + (hs * ca[s][j]) * kf[j][i];
                xs[i] = s == 0 ? yc[i] : yc[i] + a_;
              }
              fw.rhs_eval(xs, kf[s]);
            }
          }
          T* const sp = scr + (long long)(n + 1) * (R_ * D);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            T a_ = (hs * cb[0]) * kf[0][i];
#pragma unroll
            for (int s = 1; s < MS; ++s)
              if (s < S) a_ = a_ + (hs * cb[s]) * kf[s][i];
            yc[i] = yc[i] + a_;
            sp[so[i]] = yc[i];                                // (rows / columns beyond the state stay inside the padded slot; phase B never reads them)
          }
        }
        lds_barrier();                                        // phase B rewrites tiles 0 / 1, which the last chains above read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lm[i] = (T)0;                                       // lambda_M is formed from the outputs of the last step, below
          gn[i] = (T)0;
          yn[i] = !live[i] ? (T)0 : N - 2 > 0 ? (scr + (long long)(N - 2) * (R_ * D))[so[i]] : y0p[eo[i]];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lm[i] = live[i] ? (gys + (long long)(N - 1) * npl + ebase)[eo[i]] : (T)0;     // lambda_{N-1}: the output gradient at the last grid point
          yn[i] = live[i] ? (ys + (long long)(N - 2) * npl + ebase)[eo[i]] : (T)0;
          gn[i] = live[i] ? (gys + (long long)(N - 2) * npl + ebase)[eo[i]] : (T)0;
        }
      }
      for (int n = N - 2; n >= 0; --n) {
        const T hs = (T)A.h[n];
        T y0e[4], g0e[4], k[MS - 1][4] = {}, yb[MS][4] = {};
#pragma unroll
        for (int i = 0; i < 4; ++i) { y0e[i] = yn[i]; g0e[i] = gn[i]; }
        if constexpr (GRID) {
          if (n > 0) {                                        // the next step's checkpoint travels under this step's chains
            const T* const yp = n - 1 > 0 ? scr + (long long)(n - 1) * (R_ * D) : (const T*)Ap->y0 + ebase;
#pragma unroll
            for (int i = 0; i < 4; ++i) yn[i] = live[i] ? yp[n - 1 > 0 ? so[i] : eo[i]] : (T)0;
          }
          // the outputs interpolated inside step n, in the order of j: w_j g_j joins lambda_{n+1}, (1 - w_j) g_j (g0e) lambda_n
          const T* const go = (const T*)Ap->gout + ebase;
#pragma unroll
          for (int i = 0; i < 4; ++i) g0e[i] = (n == 0 && live[i]) ? go[eo[i]] : (T)0;
          for (int j = Ap->obeg[n]; j < Ap->obeg[n + 1]; ++j) {
            const T w = (T)Ap->ow[j];
            const T* const gj = go + (long long)j * npl;
            if (w != (T)1) {
              const T w1 = (T)1 - w;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const T g_ = live[i] ? gj[eo[i]] : (T)0;
                lm[i] = lm[i] + w * g_;
                g0e[i] = g0e[i] + w1 * g_;
              }
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i) lm[i] = lm[i] + (live[i] ? gj[eo[i]] : (T)0);
            }
          }
        } else if (n > 0) {                                   // the next step's checkpoint and output gradient travel under this step's chains
          const T* const yp = ys + (long long)(n - 1) * npl + ebase;
          const T* const gp = gys + (long long)(n - 1) * npl + ebase;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            yn[i] = live[i] ? yp[eo[i]] : (T)0;
            gn[i] = live[i] ? gp[eo[i]] : (T)0;
          }
        }
#pragma unroll
        for (int s = 0; s < MS; ++s) {                        // forward: the stage states from the checkpoint; S - 1 evaluations
          if (s < S) {
            T xs[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              T a_ = (T)0;
#pragma unroll
              for (int j = 0; j < s; ++j) a_ = j == 0 ? (hs * ca[s][0]) * k[0][i] : a_ + (hs * ca[s][j]) * k[j][i];
              xs[i] = s == 0 ? y0e[i] : y0e[i] + a_;
            }
            if (s + 1 < S) {
              fw.s_ys = tiles + s * TILE; fw.cur = 0;         // (rhs_eval writes tile `cur` of s_ys: stage s goes to tile s)
              fw.rhs_eval(xs, k[s < MS - 1 ? s : 0]);
            } else {                                          // Y_S is only an operand of the weight gradient (the first barrier of the reverse stages publishes it)
              T* const yt = tiles + s * TILE;
#pragma unroll
              for (int i = 0; i < 4; ++i) yt[fw.row_of(i) * LD + col] = xs[i];
            }
          }
        }
#pragma unroll
        for (int s = MS - 1; s >= 0; --s) {                   // backward: kbar_s from lambda_{n+1} and the later stages' Ybar
          if (s < S) {
            T kb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              T a_ = (hs * cb[s]) * lm[i];
#pragma unroll
              for (int j = s + 1; j < MS; ++j)
                if (j < S) a_ = a_ + (hs * ca[j][s]) * yb[j][i];
              kb[i] = a_;
            }
            T* const kt = tiles + (MS + (s & 1)) * TILE;
            const T* const yt = tiles + s * TILE;
            bw.s_ys = kt; bw.cur = 0;
            bw.rhs_eval(kb, yb[s]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {                     // Wbar += Y_s^T kbar_s, bbar += 1^T kbar_s: K = rows 4 q + lg
              const T b_ = kt[(4 * q + lg) * LD + col];
#pragma unroll
              for (int m = 0; m < NB; ++m) wg[m] = TR::mfma(yt[(4 * q + lg) * LD + 16 * m + li], b_, wg[m]);
              if (has_bias) bg = TR::mfma((T)1, b_, bg);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          T v = lm[i];
#pragma unroll
          for (int s = 0; s < MS; ++s)
            if (s < S) v = v + yb[s][i];
          lm[i] = v + g0e[i];
        }
        lds_barrier();                                        // tile 0 is rewritten by the next step; the last product above read it
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (live[i]) (lam + ebase)[eo[i]] = lm[i];
    }
    const long long tk1 = (long long)wall_clock64();
    // this workgroup's partial block, written through before its hand-off record says so
    T* const mine = (T*)A.gpart + (long long)blockIdx.x * E;
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) dl_store_agent(mine + (16 * m + TR::acc_row(lane, i)) * D + col, wg[m][i]);
    if (lg == 0) dl_store_agent(mine + D * D + col, bg[0]);   // (every row of the bias tile holds the column sums)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const long long tk2 = (long long)wall_clock64();
    ok = grid_reduce_rank(A.p, none, sh, gen++, r);           // every workgroup's partial block is complete
    if (ok) {
      const int G = (int)gridDim.x;
      const int EPW = (E + G - 1) / G;                        // entries per workgroup: a contiguous run
      const int e_lo = (int)blockIdx.x * EPW, e_hi = e_lo + EPW < E ? e_lo + EPW : E;
      const T* const part = (const T*)A.gpart;
      T* const gw = (T*)A.gw;
      T* const gb = (T*)A.gb;
      for (int e = e_lo + (int)threadIdx.x; e < e_hi; e += (int)blockDim.x) {
        const int a = e / D, c = e % D;
        const bool is_w = e < D * D;
        if (is_w ? !(a < dim && c < dim) : !(gb != nullptr && c < dim)) continue;
        T s_ = (T)0;
        int g = 0;
        for (; g + 8 <= G; g += 8) {                          // workgroup order, eight loads in flight
          T v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = dl_load_agent(part + (long long)(g + u) * E + e);
#pragma unroll
          for (int u = 0; u < 8; ++u) s_ = s_ + v[u];
        }
        for (; g < G; ++g) s_ = s_ + dl_load_agent(part + (long long)g * E + e);
        if (is_w) gw[a * dim + c] = s_;
        else gb[c] = s_;
      }
    }
    prof[0] = tk1 - tk0; prof[1] = tk2 - tk1; prof[2] = (long long)wall_clock64() - tk2;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    DiscResult res;
    res.status = ok ? 0u : (unsigned)MI_ODE_ST_SYNC_TIMEOUT; res.handoffs = (int)gen;
    for (int i = 0; i < 3; ++i) res.prof[i] = prof[i];
    const long long* src = (const long long*)&res;
    long long* dst = (long long*)A.res;
    for (int i = 0; i < (int)(sizeof(DiscResult) / sizeof(long long)); ++i)
      __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace mi
