// Per-trajectory step control: ONE trajectory's whole adaptive integration as a plain function.
//
// rows_integrate is AdaptiveStepsizeODESolver.integrate (solvers.py:27-35, dopri5.py:70-121) for a single row of a batch: its own
// _select_initial_step, its own error ratio over its D elements, its own accept / reject sequence, output cursor, dense output,
// max_num_steps and dt-underflow checks.  It is what thread 0 of k_persist_rowlocal does for a batch of one trajectory, operation for
// operation: the same device functions (step_combine, step_finish, step_y1_general, step_emit, controller_apply, attempt_core) in the
// same order, fed a record that is the row's own - max a / max b / sum a accumulated over d = 0 .. D-1 as the shared kernel's thread
// accumulates them, R_N = D.  (A one-row block reduction only folds the thread's values with exact zeros.)
//
// No HIP construct in here: the kernel (mi_ode_rows.h) calls it from every live lane, the CPU tests compile it with g++.  The includer
// declares, in namespace mi, before this header: Ctl, CtrlParams, Acc, AttemptState, kRec, R_*, PH_*, finite_, controller_apply,
// attempt_core (mi_ode_dev.h, mi_ode_ctrl_dev.h) and StepArgs, StepPlanes, for_stages, step_combine, step_finish, step_y1_general,
// step_emit (mi_ode_step_fused.h).
#pragma once

#ifndef MI_ODE_ROWS_FN
#if defined(__HIPCC__)
#define MI_ODE_ROWS_FN __device__ __forceinline__
#else
#define MI_ODE_ROWS_FN inline
#endif
#endif

namespace mi {

struct RowResult {            // what a row reports: [batch, 4] int64 on the device
  long long n_attempt, n_accept, nfe;
  unsigned status;            // MI_ODE_ST_* of THIS row
};

// the row's own record: a thread's running reductions are the whole reduction
MI_ODE_ROWS_FN void rows_record(double (&rec)[kRec], const Acc& acc, int n) {
  rec[R_MAXA] = acc.maxa; rec[R_MAXB] = acc.maxb; rec[R_SUMA] = acc.suma; rec[R_SUMB] = acc.sumb; rec[R_FLAG] = (double)acc.flag;
  rec[R_N] = (double)n; rec[6] = 0; rec[7] = 0;
}

// the output cursor and the entry assertions (solvers.py:33-34, dopri5.py:98-100), as set_outputs_apply arms them for the shared kernel
MI_ODE_ROWS_FN void rows_set_outputs(Ctl& c, int n_out) {
  c.next_out = 0; c.n_out = n_out; c.n_steps_out = 0; c.emit_lo = c.emit_hi = 0;
  c.done = 0;
  if (n_out <= 0) { c.done = 1; return; }
  if (c.y0_nonfinite && c.n_attempt == 0) { c.status |= MI_ODE_ST_NONFINITE; c.done = 1; return; }
  if (!(c.t1 + c.dt > c.t1)) { c.status |= MI_ODE_ST_DT_UNDERFLOW; c.done = 1; }
}

// y: the row's state (in: y0, out: the state at the last accepted step); f: f at that state (out); e0: the row's first element in a
// solution plane; cp.t_out: the n_out requested times after t_start.  The only exits of the loop are attempt_tail's: all outputs
// produced, max_num_steps attempts inside one output interval, t + dt == t.
template <typename T, int S, bool TS, bool FSAL, class RHS>
MI_ODE_ROWS_FN void rows_integrate(const RHS& rhs, const StepArgs& sa, const CtrlParams& cp, T sign, double t_start, double first_dt,
                                   int n_out, T (&y)[RHS::D], T (&f)[RHS::D], long long e0, RowResult& res) {
  constexpr int D = RHS::D;
  const double* t_out = cp.t_out;
  // The scalar state lives in a Ctl only for the two phases of before_integrate (controller_apply works on one); the loop keeps an
  // AttemptState.  Everything is inlined: the fields nobody reads never exist.
  Ctl c = Ctl();
  c.t0 = c.t1 = t_start;
  c.dt = cp.auto_first_step ? 0.0 : first_dt;
  const T t_first = (T)c.t1;
  double rec[kRec];

  // ---- before_integrate: f0 and the norms of misc._select_initial_step ----
  T f0[D];
  {
    Acc acc;
    T ys[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ys[d] = y[d];
    rhs(sign * t_first, ys, f0);
#pragma unroll
    for (int d = 0; d < D; ++d) f0[d] = sign * f0[d];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const T sc = (T)cp.atol + fabs(y[d]) * (T)cp.rtol;     // misc.py:225
      const double q0 = (double)(y[d] / sc);
      acc.suma += q0 * q0;
      if (!finite_(y[d])) acc.flag = 1;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const T sc = (T)cp.atol + fabs(y[d]) * (T)cp.rtol;
      const double q1 = (double)(f0[d] / sc);
      acc.sumb += q1 * q1;                                   // misc.py:228
    }
    rows_record(rec, acc, D);
    controller_apply(&c, rec, PH_F0, cp);
  }
  if (cp.auto_first_step) {                                  // misc.py:235-245
    Acc acc;
    const T h0 = (T)c.h0;
    T ys[D], f1[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ys[d] = y[d] + h0 * f0[d];
    rhs(sign * (t_first + (T)1.0 * h0), ys, f1);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const T kn = sign * f1[d];
      const T sc = (T)cp.atol + fabs(y[d]) * (T)cp.rtol;
      const double q = (double)((kn - f0[d]) / sc);          // misc.py:237
      acc.suma += q * q;
    }
    rows_record(rec, acc, D);
    controller_apply(&c, rec, PH_INITB, cp);
  }
  rows_set_outputs(c, n_out);
  AttemptState st;
  st.load(c);

  // ---- the adaptive loop (dopri5.py:82-121) ----
  T k[S + 1][D];
#pragma unroll
  for (int d = 0; d < D; ++d) k[0][d] = f0[d];
  while (!st.done) {
    const T hs = (T)st.dt;                                   // rk_common.py:46
    const T t0 = (T)st.t1;                                   // rk_common.py:45
    T ys[D];
    auto stage = [&](auto sg_c) {
      constexpr int SG = decltype(sg_c)::value;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        T kk[SG];
#pragma unroll
        for (int j = 0; j < SG; ++j) kk[j] = k[j][d];
        ys[d] = step_combine<T, SG>(y[d], kk, hs, sa);
      }
      T kn[D];
      rhs(sign * (t0 + (T)sa.alpha[SG - 1] * hs), ys, kn);
#pragma unroll
      for (int d = 0; d < D; ++d) k[SG][d] = sign * kn[d];
    };
    for_stages<1, S>(stage);
    Acc acc;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      T kk[S + 1];
#pragma unroll
      for (int j = 0; j <= S; ++j) kk[j] = k[j][d];
      T err, unused_mid;
      step_finish<T, S>(y[d], kk, hs, sa, err, unused_mid, false);       // y_mid only if an output falls into the step (below)
      if constexpr (!FSAL) ys[d] = step_y1_general<T, S>(y[d], kk, hs, sa);   // rk_common.py:55-56
      acc.maxa = fmax(acc.maxa, (double)fabs(y[d]));
      acc.maxb = fmax(acc.maxb, (double)fabs(ys[d]));
      acc.suma += (double)err * (double)err;
    }
    rows_record(rec, acc, D);
    attempt_core(st, rec, cp);
    if (st.accepted) {
      if (st.emit_hi > st.emit_lo) {
        StepPlanes<T, S> P;
        P.j_lo = st.emit_lo; P.j_hi = st.emit_hi;
        P.t_start = st.emit_t0; P.t_new = st.emit_t1; P.dt64 = st.emit_dt;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          T kk[S + 1];
#pragma unroll
          for (int j = 0; j <= S; ++j) kk[j] = k[j][d];
          T err_unused, ymid = y[d];
          if constexpr (!TS) step_finish<T, S>(y[d], kk, hs, sa, err_unused, ymid, true);
          step_emit<T, S, TS>(sa, P, y[d], ys[d], kk, ymid, e0 + d, t_out);
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) { y[d] = ys[d]; k[0][d] = k[S][d]; }       // FSAL (rk_common.py:58)
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) f[d] = k[0][d];
  res.n_attempt = st.n_attempt; res.n_accept = st.n_accept; res.nfe = st.nfe; res.status = st.status;
}

}  // namespace mi
