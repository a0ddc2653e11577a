// Per-trajectory step control for the ODEFunc MLP on the matrix cores: options={'per_trajectory': True} / mi_ode_integrate_rows_mlp.
//
// k_rows_rowlocal (mi_ode_rows.h) gives every LANE an integration of its own - impossible where f is evaluated by the threads of a
// workgroup together, as the MLP tile kernels do (a barrier under per-lane control flow hangs).  Here the control flow stays
// workgroup-uniform and only the DATA is per row: a 32-row tile (MlpGeom, weight slices resident as in MlpCtx::init) runs through the
// whole call with y and the stage derivatives in registers, as k_fixed_mlp does, and every row of it has its own step size, stage time,
// error record, controller state, output cursor and done flag in LDS.  The tile loops until its last row is done.  Output row r of an
// MFMA product depends on input row r only, so a row's numbers cannot depend on its tile-mates: row i of the result is what the call
// on y0[i:i+1] computes, whatever batch it travels in.
//   * per attempt: S evaluations (3 barriers each, as mlp_eval), one barrier between the rows' error partials and the controller, one
//     after the controller's write-back: 3 S + 2;
//   * the controller is attempt_core / controller_apply of mi_ode_ctrl_dev.h, one lane per row (32 lanes of the last wavefront), on the
//     row's own record: max |y0|, max |y1|, sum err^2 reduced over the 16 lanes of a column block with the __shfl_down tree of wave_sum
//     and over the CB3 column blocks in order - the order in which the shared kernels fold a one-row batch (block_reduce_thread0);
//   * a row that is done, failed or padding takes no further part: no stores, registers frozen, its step 0 so that its stage times stay
//     finite.  A failing row sets ITS status bits; the others run to the end;
//   * dense output per row, speculative as in mlp_pass: the outputs the row's attempt would cross are written before the controller
//     decides and overwritten by the accepted step that covers them (the row's cursor only advances on accept);
//   * the grid is a loop over tiles: no co-residency, no mailbox, no ticket; a tile costs what its slowest row costs.
// fp32 only.  HBM traffic: y0 in, solution rows out, [batch, 4] int64 of per-row results, the final y / f planes.
#pragma once
#include "mi_ode_mlp.h"
#include "mi_ode_rows.h"

namespace mi {

constexpr int kRowsMlpTout = 512;       // output times cached in LDS (more: read from the uploaded array)

// what the rows of a tile keep between attempts.  Written by the controller lanes (lane r: row r), read by everyone behind a barrier.
struct RowsMlpShared {
  AttemptState st[32];                  // the rows' scalar state rests here between attempts
  double tout[kRowsMlpTout];
  double part[3][4][32];                // [max a | sum a, max b | sum b, sum err^2 | flag][column block][row]
  double t_start[32], dt64[32];         // the attempt interval in float64 (dense output)
  float hs[32], t0[32];                 // step and start time in the state dtype (rk_common.py:45-46); hs = 0: the row takes no part
  float ts[32];                         // the time the network sees in this evaluation, per row (direction sign included)
  int j_lo[32], j_hi[32];               // outputs the row's attempt would cross
  int live[32], accepted[32];
  int any_live;                         // the loop condition: one word
};

// every thread: the output times into LDS when they fit - rows_stage_tout with this kernel's smaller cache (the few that travel as kernel
// arguments are read at constant indices: an argument array indexed by the thread number costs a private copy of ALL arguments)
__device__ __forceinline__ const double* rows_mlp_stage_tout(const PersistArgs& A, double* lds_tout) {
  if (A.n_out <= kPersistTSmall) {
#pragma unroll
    for (int i = 0; i < kPersistTSmall; ++i)
      if ((int)threadIdx.x == i && i < A.n_out) lds_tout[i] = A.t_small[i];
    return lds_tout;
  }
  if (A.n_out <= kRowsMlpTout) {
    for (int i = threadIdx.x; i < A.n_out; i += blockDim.x) lds_tout[i] = A.s.t_out[i];
    return lds_tout;
  }
  return A.s.t_out;
}

// mlp_eval with a first-layer bias per ROW: stage time is t_row + alpha * dt_row, so the shift ts * w_t of a time-dependent net differs
// between the rows 4 lg + i and 16 + 4 lg + i a thread holds.  Everything else is mlp_eval's, operation for operation (the existing
// instantiations stay what they are: this is a sibling, not a flag).
template <int ACT>
__device__ __forceinline__ void mlp_act_pair_rows(float a, float b, float bias_a, float bias_b, float& oa, float& ob) {
  if constexpr (ACT == MLP_ACT_TANH) {
    mlp_f2 x = {a, b};
    const mlp_f2 bias = {bias_a, bias_b};
    x = x + bias;
    const mlp_f2 y = mlp_tanh2(x);
    oa = y.x; ob = y.y;
  } else {
    oa = mlp_act<ACT>(a + bias_a); ob = mlp_act<ACT>(b + bias_b);
  }
}

template <int DP, int HP, int ACT>
__device__ __forceinline__ void mlp_eval_rows(float* s_x, float* s_h1, float* s_h2, const float* w1f, const float* w2f, const float* w3f,
                                              float b1v, float wtv, const float* s_ts, float b2v, float b3v, float* out4) {
  using G = MlpGeom<DP, HP>;
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  constexpr int KS1 = DP / 4, KS2 = HP / 4;
  __syncthreads();                                          // s_x and s_ts are complete
  if (wave < G::NW12) {                                     // layer 1: [32 x DP] @ [DP x 16]
    f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
    const float* a0p = s_x + li * G::LDX + lg * KS1;
    const float* a1p = s_x + (16 + li) * G::LDX + lg * KS1;
#pragma unroll
    for (int m = 0; m < KS1 / 4; ++m) {
      const f4 a0 = *(const f4*)(a0p + 4 * m), a1 = *(const f4*)(a1p + 4 * m);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], w1f[4 * m + v], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], w1f[4 * m + v], c1, 0, 0, 0);
      }
    }
    const int col = 16 * wave + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float h0, h1;
      mlp_act_pair_rows<ACT>(c0[i], c1[i], b1v + s_ts[4 * lg + i] * wtv, b1v + s_ts[16 + 4 * lg + i] * wtv, h0, h1);
      s_h1[(4 * lg + i) * G::LDH + col] = h0;
      s_h1[(16 + 4 * lg + i) * G::LDH + col] = h1;
    }
  }
  __syncthreads();
  if (wave < G::NW12) {                                     // layer 2: [32 x HP] @ [HP x 16]
    f4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
    const float* a0p = s_h1 + li * G::LDH + lg * KS2;
    const float* a1p = s_h1 + (16 + li) * G::LDH + lg * KS2;
#pragma unroll
    for (int m = 0; m < KS2 / 4; ++m) {
      const f4 a0 = *(const f4*)(a0p + 4 * m), a1 = *(const f4*)(a1p + 4 * m);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[v], w2f[4 * m + v], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[v], w2f[4 * m + v], c1, 0, 0, 0);
      }
    }
    const int col = 16 * wave + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float h0, h1;
      mlp_act_pair<ACT>(c0[i], c1[i], b2v, h0, h1);
      s_h2[(4 * lg + i) * G::LDH + col] = h0;
      s_h2[(16 + 4 * lg + i) * G::LDH + col] = h1;
    }
  }
  __syncthreads();
  if (wave < G::NW3) {                                      // layer 3: one 16-row block x 16 output columns per wave
    const int rb = wave / G::CB3;
    f4 c = {0, 0, 0, 0};
    const float* ap = s_h2 + (16 * rb + li) * G::LDH + lg * KS2;
#pragma unroll
    for (int m = 0; m < KS2 / 4; ++m) {
      const f4 a = *(const f4*)(ap + 4 * m);
#pragma unroll
      for (int v = 0; v < 4; ++v) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[v], w3f[4 * m + v], c, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out4[i] = c[i] + b3v;
  }
}

// a row's reduction over the 16 lanes of its column block: the offsets 8, 4, 2, 1 of wave_sum / wave_max (the larger ones fold exact
// zeros into a one-row batch), valid in the lane with li == 0
__device__ __forceinline__ double rows_sum16(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_down(v, off, 16);
  return v;
}
__device__ __forceinline__ double rows_max16(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 16));
  return v;
}

template <int DP, int HP, int ACT, int S, bool TS>
__global__ __launch_bounds__((64 * MlpGeom<DP, HP>::NW)) void k_rows_mlp(RowsArgs R) {
  using G = MlpGeom<DP, HP>;
  static_assert(G::R == 32 && G::CB3 <= 4, "RowsMlpShared is laid out for 32-row tiles of at most 4 column blocks");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ RowsMlpShared sh;
  const PersistArgs& A = R.p;
  const StepArgs& SA = A.s;
  MlpCtx<DP, HP, ACT> cx;
  cx.init(SA.rhs, SA.dim, smem_raw);
  CtrlParams cp = SA.cp;
  cp.t_out = rows_mlp_stage_tout(A, sh.tout);
  const double* t_out = cp.t_out;
  const int d = cx.d, col = cx.col;
  const float sign = cx.sign;
  const bool own_wave = cx.wave < G::NW3;                     // this wavefront holds state elements (layer 3)
  const int rbase = own_wave ? cx.rbase : 0;                  // (the other wavefronts read no per-row data)
  const int cb = cx.wave % G::CB3;
  const bool ctrl = cx.wave == G::NW - 1 && cx.lane < 32;     // the controller lanes: lane r is row r of the tile
  const int r = cx.lane & 31;
  const float t_first = (float)A.t0;
  float* const y_fin = (float*)SA.planes;                     // the final state: planes 0 / 2 (mi_ode_get_state), as k_rows_rowlocal
  float* const f_fin = (float*)(SA.planes + 2 * SA.stride);
  const long long ntiles = (SA.batch + G::R - 1) / G::R;

  auto eval = [&](float* out4) {
    mlp_eval_rows<DP, HP, ACT>(cx.s_x, cx.s_h1, cx.s_h2, cx.w1f, cx.w2f, cx.w3f, cx.b1v, cx.wtv, sh.ts, cx.b2v, cx.b3v, out4);
  };
  // controller lane r: what the next attempt of its row needs; returns whether the row goes on
  auto publish = [&](const AttemptState& st, bool exists) -> bool {
    const bool live = exists && !st.done;
    sh.live[r] = live ? 1 : 0;
    sh.hs[r] = live ? (float)st.dt : 0.f;                     // rk_common.py:46
    sh.t0[r] = (float)st.t1;                                  // rk_common.py:45
    sh.t_start[r] = st.t1; sh.dt64[r] = st.dt;
    int j = live ? st.next_out : 0;
    const int lo = j;
    const double t_new = st.t1 + st.dt;
    if (live)
      while (j < st.n_out && !(t_out[j] > t_new)) ++j;        // same test as the controller's output cursor
    sh.j_lo[r] = lo; sh.j_hi[r] = j;
    return live;
  };
  // all 32 controller lanes, converged: the loop condition
  auto publish_any = [&](bool live) {
    const unsigned long long any = __ballot(live);
    if (cx.lane == 0) sh.any_live = any != 0ull ? 1 : 0;
  };
  // the row's record from the column blocks' partials, folded in order from zero as block_reduce_thread0 folds wavefronts
  auto record = [&](double (&rec)[kRec], bool maxes) {
    double v0 = 0, v1 = 0, v2 = 0;
    for (int c = 0; c < G::CB3; ++c) {
      if (maxes) { v0 = fmax(v0, sh.part[0][c][r]); v1 = fmax(v1, sh.part[1][c][r]); v2 += sh.part[2][c][r]; }
      else { v0 += sh.part[0][c][r]; v1 += sh.part[1][c][r]; v2 = fmax(v2, sh.part[2][c][r]); }
    }
    if (maxes) { rec[R_MAXA] = v0; rec[R_MAXB] = v1; rec[R_SUMA] = v2; rec[R_SUMB] = 0; rec[R_FLAG] = 0; }
    else { rec[R_MAXA] = 0; rec[R_MAXB] = 0; rec[R_SUMA] = v0; rec[R_SUMB] = v1; rec[R_FLAG] = v2; }
    rec[R_N] = (double)d; rec[6] = 0; rec[7] = 0;
  };

  __syncthreads();                                            // the staged output times
  for (long long tile_i = blockIdx.x; tile_i < ntiles; tile_i += gridDim.x) {
    const long long row0 = tile_i * G::R;
    const long long left = SA.batch - row0;
    const int nr = left < G::R ? (int)left : G::R;            // rows of this tile that exist
    const long long tb = row0 * d;
    const unsigned e0 = (unsigned)(rbase * d + col);          // element i of this thread: tb + e0 + i * d
    float y0e[4], k[S + 1][4], ys[4], kn[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ok[i] = cx.owner && rbase + i < nr;
      const unsigned eo = e0 + (unsigned)(i * d);
      y0e[i] = ok[i] ? ((const float*)A.y0 + tb)[eo] : 0.f;
      if (ok[i]) ((float*)A.out0 + tb)[eo] = y0e[i];          // solution[0] = y0 (solvers.py:30)
    }
    // ---- before_integrate: f0 and the norms of misc._select_initial_step, per row (MLP_F0 of mlp_pass) ----
    if (threadIdx.x < 32) sh.ts[threadIdx.x] = sign * t_first;
    cx.put_x(y0e);
    eval(kn);
    if (own_wave) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float f0 = sign * kn[i];
        k[0][i] = f0;
        double qa = 0.0, qb = 0.0, fl = 0.0;
        if (ok[i]) {
          const float sc = (float)cp.atol + fabsf(y0e[i]) * (float)cp.rtol;      // misc.py:225
          const double q0 = (double)(y0e[i] / sc), q1 = (double)(f0 / sc);
          qa = q0 * q0; qb = q1 * q1;
          if (!finite_(y0e[i])) fl = 1.0;
        }
        qa = rows_sum16(qa); qb = rows_sum16(qb); fl = rows_max16(fl);
        if (cx.li == 0) { sh.part[0][cb][rbase + i] = qa; sh.part[1][cb][rbase + i] = qb; sh.part[2][cb][rbase + i] = fl; }
      }
    }
    __syncthreads();
    Ctl c = Ctl();
    double rec[kRec];
    if (ctrl) {
      c.t0 = c.t1 = A.t0;
      c.dt = cp.auto_first_step ? 0.0 : A.first_dt;
      if (r < nr) { record(rec, false); controller_apply(&c, rec, PH_F0, cp); }
      sh.hs[r] = (r < nr && cp.auto_first_step) ? (float)c.h0 : 0.f;
    }
    if (cp.auto_first_step) {                                 // misc.py:235-245 (MLP_INITB of mlp_pass)
      __syncthreads();
      if (own_wave) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ys[i] = y0e[i] + sh.hs[rbase + i] * k[0][i];         // misc.py:235
      }
      if (threadIdx.x < 32) sh.ts[threadIdx.x] = sign * (t_first + sh.hs[threadIdx.x]);
      cx.put_x(ys);
      eval(kn);
      if (own_wave) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double qa = 0.0;
          if (ok[i]) {
            const float sc = (float)cp.atol + fabsf(y0e[i]) * (float)cp.rtol;
            const double q = (double)((sign * kn[i] - k[0][i]) / sc);            // misc.py:237
            qa = q * q;
          }
          qa = rows_sum16(qa);
          if (cx.li == 0) { sh.part[0][cb][rbase + i] = qa; sh.part[1][cb][rbase + i] = 0.0; sh.part[2][cb][rbase + i] = 0.0; }
        }
      }
      __syncthreads();
      if (ctrl && r < nr) { record(rec, false); controller_apply(&c, rec, PH_INITB, cp); }
    }
    if (ctrl) {
      if (r < nr) rows_set_outputs(c, A.n_out);
      else c.done = 1;
      AttemptState st;
      st.load(c);
      st.accepted = 0;
      const bool live = publish(st, r < nr);
      sh.accepted[r] = 0;
      sh.st[r] = st;
      publish_any(live);
    }
    __syncthreads();

    // ---- the adaptive loop (dopri5.py:82-121): workgroup-uniform, while any row of the tile is not done ----
    while (uniform_i(sh.any_live)) {
      auto stage = [&](auto sg_c) {
        constexpr int SG = decltype(sg_c)::value;
        if (own_wave) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float kk[SG];
#pragma unroll
            for (int j = 0; j < SG; ++j) kk[j] = k[j][i];
            ys[i] = mlp_combine<SG>(y0e[i], kk, sh.hs[rbase + i], SA);           // the row's own step
          }
        }
        if (threadIdx.x < 32)                                                    // rk_common.py:50, in the state dtype, per row
          sh.ts[threadIdx.x] = sign * (sh.t0[threadIdx.x] + (float)SA.alpha[SG - 1] * sh.hs[threadIdx.x]);
        cx.put_x(ys);
        eval(kn);
#pragma unroll
        for (int i = 0; i < 4; ++i) k[SG][i] = sign * kn[i];
      };
      for_stages<1, S>(stage);
      if (own_wave) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = rbase + i;
          const float hs = sh.hs[row];
          float kk[S + 1];
#pragma unroll
          for (int j = 0; j <= S; ++j) kk[j] = k[j][i];
          const float err = mlp_error<S>(kk, hs, SA);
          double ma = 0.0, mb = 0.0, se = 0.0;
          if (ok[i]) {
            ma = fmax(ma, (double)fabsf(y0e[i]));
            mb = fmax(mb, (double)fabsf(ys[i]));
            se = (double)err * (double)err;
            if (sh.live[row] && sh.j_hi[row] > sh.j_lo[row]) {                   // speculative dense output of the row's own attempt
              StepPlanes<float, S> P;
              P.j_lo = sh.j_lo[row]; P.j_hi = sh.j_hi[row];
              P.t_start = sh.t_start[row]; P.dt64 = sh.dt64[row]; P.t_new = P.t_start + P.dt64;
              float err_unused, ymid = y0e[i];
              if constexpr (!TS) step_finish<float, S>(y0e[i], kk, hs, SA, err_unused, ymid, true);
              step_emit<float, S, TS>(SA, P, y0e[i], ys[i], kk, ymid, tb + e0 + (unsigned)(i * d), t_out);
            }
          }
          ma = rows_max16(ma); mb = rows_max16(mb); se = rows_sum16(se);
          if (cx.li == 0) { sh.part[0][cb][row] = ma; sh.part[1][cb][row] = mb; sh.part[2][cb][row] = se; }
        }
      }
      __syncthreads();
      if (ctrl) {
        int acc = 0;
        bool live = false;
        if (sh.live[r]) {                                      // (a row that is done keeps its state and its published zeros)
          AttemptState st = sh.st[r];
          record(rec, true);
          attempt_core(st, rec, cp);
          acc = st.accepted;
          live = publish(st, true);
          sh.st[r] = st;
        }
        sh.accepted[r] = acc;
        publish_any(live);
      }
      __syncthreads();
      if (own_wave) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (sh.accepted[rbase + i]) { y0e[i] = ys[i]; k[0][i] = k[S][i]; }     // FSAL (rk_common.py:58); a row that is done stays frozen
      }
    }

    // ---- the tile's results ----
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ok[i]) {
        const unsigned eo = e0 + (unsigned)(i * d);
        (y_fin + tb)[eo] = y0e[i];
        (f_fin + tb)[eo] = k[0][i];
      }
    }
    if (cx.wave == G::NW - 1) {                                // every lane of the controller wavefront: one set of atomics per tile
      RowResult res;
      res.n_attempt = res.n_accept = res.nfe = 0; res.status = 0;
      if (ctrl && r < nr) {
        const AttemptState& st = sh.st[r];
        res.n_attempt = st.n_attempt; res.n_accept = st.n_accept; res.nfe = st.nfe; res.status = st.status;
        long long* o = R.row_stats + (row0 + r) * 4;
        o[0] = res.n_attempt; o[1] = res.n_accept; o[2] = res.nfe; o[3] = (long long)res.status;
      }
      const long long m_att = rows_wave_max(res.n_attempt), m_acc = rows_wave_max(res.n_accept);
      const long long m_rej = rows_wave_max(res.n_attempt - res.n_accept), m_nfe = rows_wave_max(res.nfe);
      unsigned bits = res.status;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) bits |= (unsigned)__shfl_down((int)bits, off, 64);
      if (cx.lane == 0) {
        __hip_atomic_fetch_max(&R.agg->n_attempt, m_att, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&R.agg->n_accept, m_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&R.agg->n_reject, m_rej, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(&R.agg->nfe, m_nfe, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bits != 0u) __hip_atomic_fetch_or(&R.agg->status, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // (the next tile's first writes to the per-row arrays follow the barriers of its first evaluation)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {                  // (fields no atomic above touches)
    Ctl* g = R.agg;
    g->idx_y0 = 0; g->idx_y1 = 1;
    for (int j = 0; j < kMaxK; ++j) g->idx_k[j] = 2 + j;
    g->t0 = g->t1 = A.n_out > 0 ? t_out[A.n_out - 1] : A.t0;
    g->done = 1;
  }
}

}  // namespace mi
