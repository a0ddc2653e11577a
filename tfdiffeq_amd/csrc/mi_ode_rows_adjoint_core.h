// The adjoint of a per-trajectory solve: ONE trajectory's whole backward pass as a plain function.
//
// rows_adjoint_row is adjoint.py:117-178 (tfdiffeq_amd/adjoint.py::_generic_backward) applied to a single row of a batch: for
// k = T-1 .. 1 the time gradient of the measurement point (dLd_cur_t = f(t_k, y_k) . g_k, adj_t -= dLd_cur_t), the adaptive integration of
// the four-component tuple state (y [1, D], adj_y [1, D], adj_t [], adj_params [P]) from t_k to t_{k-1} with the dynamics
// (f, -a^T df/dy, -a^T df/dt, -a^T df/dtheta), and the jump adj_y += g_{k-1}.  Every interval is an odeint call of its own, as in the
// reference: its own _select_initial_step (python max over the component norms), one error ratio and one scalar tolerance per component,
// accepted only if all ratios are <= 1, the step from the first maximal ratio (controller_apply_seg / attempt_core_seg,
// mi_ode_ctrl_dev.h), the value at t_{k-1} from the dense output of the overshooting last step.  Time runs backwards: sign = -1, the
// solver sees s = -t (misc.py:318-321), as rows_integrate allows.
//
// The row owns its adj_params: nothing is reduced inside the loop.  The stage derivatives k[S + 1][NA], NA = 2 D + 1 + max(P, 1), are
// thread-private and indexed by compile-time constants only (S and NA are template parameters; every loop over them is unrolled).
//
// No HIP construct in here: the kernel (mi_ode_rows_adjoint.h) calls it from every live lane, the CPU tests compile it with g++.  The
// includer declares, in namespace mi, before this header: what mi_ode_rows_core.h needs, SegState, controller_apply_seg, attempt_core_seg
// (mi_ode_ctrl_dev.h), quartic_from_mid, quartic_eval, interp_x (mi_ode_dense.h), and mi_ode_rows_core.h itself (rows_record,
// rows_set_outputs, RowResult).
//
// RHS: a generated functor (tfdiffeq_amd/lower.py: adjoint_source) with D, P, operator()(t, y, k) and
// vjp_t(t, y, kbar, ybar, tbar, acc): ybar = (df/dy)^T kbar, tbar = (df/dt)^T kbar, acc.add(i, (df/dtheta_i)^T kbar).
#pragma once

namespace mi {

template <class RHS>
struct AdjLayout {
  static constexpr int D = RHS::D;
  static constexpr int P = RHS::P;
  static constexpr int PP = P > 0 ? P : 1;          // without parameters adj_params is one zero scalar (adjoint.py:124)
  static constexpr int NA = 2 * D + 1 + PP;
  static constexpr int kSeg = 4;
  static constexpr int seg(int e) { return e < D ? 0 : e < 2 * D ? 1 : e == 2 * D ? 2 : 3; }
  static constexpr int count(int s) { return s < 2 ? D : s == 2 ? 1 : PP; }
};

// the sink of the generated vjp: the row's own -a^T df/dtheta, thread-private
template <typename T>
struct AdjPrivateSink {
  T* g;
  MI_ODE_ROWS_FN void add(int i, T v) { g[i] += v; }
};

// the augmented dynamics (adjoint.py:69-105) at (t, z): dz = (f, vjp_y, vjp_t, vjp_params) with grad_outputs -adj_y
template <typename T, class RHS>
MI_ODE_ROWS_FN void adj_dynamics(const RHS& rhs, T t, const T* z, T* dz) {
  using L = AdjLayout<RHS>;
  T kbar[L::D];
#pragma unroll
  for (int d = 0; d < L::D; ++d) kbar[d] = -z[L::D + d];
  rhs(t, z, dz);
#pragma unroll
  for (int p = 0; p < L::PP; ++p) dz[2 * L::D + 1 + p] = (T)0;
  AdjPrivateSink<T> sink{dz + 2 * L::D + 1};
  T tbar = (T)0;
  rhs.vjp_t(t, z, kbar, dz + L::D, tbar, sink);
  dz[2 * L::D] = tbar;
}

template <class L>
MI_ODE_ROWS_FN void adj_records(double (&rec)[L::kSeg][kRec], const Acc (&acc)[L::kSeg]) {
#pragma unroll
  for (int s = 0; s < L::kSeg; ++s) rows_record(rec[s], acc[s], L::count(s));
}

// One interval: odeint(augmented_dynamics, z, [t_start, t_out[0]]) in the solver's (negated) time; z: in the state at t_start, out the
// dense output at cp.t_out[0] (unchanged contents are meaningless when res.status != 0).  The only exits of the loop are attempt_tail's.
template <typename T, int S, class RHS>
MI_ODE_ROWS_FN void adj_interval(const RHS& rhs, const StepArgs& sa, const CtrlParams& cp, double t_start, T (&z)[AdjLayout<RHS>::NA], RowResult& res) {
  using L = AdjLayout<RHS>;
  constexpr int NA = L::NA;
  const T sign = (T)-1;
  Ctl c = Ctl();
  c.t0 = c.t1 = t_start;
  c.dt = 0.0;
  const T t_first = (T)c.t1;
  double rec[L::kSeg][kRec];
  SegState ss;

  // ---- before_integrate: f0 and the norms of misc._select_initial_step, per component ----
  T k[S + 1][NA];
  {
    Acc acc[L::kSeg];
    T f0[NA];
    adj_dynamics<T, RHS>(rhs, sign * t_first, z, f0);
#pragma unroll
    for (int e = 0; e < NA; ++e) k[0][e] = sign * f0[e];
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const T sc = (T)cp.atol + fabs(z[e]) * (T)cp.rtol;     // misc.py:225
      const double q0 = (double)(z[e] / sc);
      const double q1 = (double)(k[0][e] / sc);
      acc[L::seg(e)].suma += q0 * q0;                        // misc.py:227
      acc[L::seg(e)].sumb += q1 * q1;                        // misc.py:228
      if (!finite_(z[e])) acc[L::seg(e)].flag = 1;
    }
    adj_records<L>(rec, acc);
    controller_apply_seg(&c, &ss, rec, L::kSeg, PH_F0, cp);
  }
  {                                                          // misc.py:235-245
    Acc acc[L::kSeg];
    const T h0 = (T)c.h0;
    T zs[NA], f1[NA];
#pragma unroll
    for (int e = 0; e < NA; ++e) zs[e] = z[e] + h0 * k[0][e];
    adj_dynamics<T, RHS>(rhs, sign * (t_first + (T)1.0 * h0), zs, f1);
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      const T kn = sign * f1[e];
      const T sc = (T)cp.atol + fabs(z[e]) * (T)cp.rtol;
      const double q = (double)((kn - k[0][e]) / sc);        // misc.py:237
      acc[L::seg(e)].suma += q * q;
    }
    adj_records<L>(rec, acc);
    controller_apply_seg(&c, &ss, rec, L::kSeg, PH_INITB, cp);
  }
  rows_set_outputs(c, 1);
  AttemptState st;
  st.load(c);

  // ---- the adaptive loop (dopri5.py:82-121) over the tuple state ----
  while (!st.done) {
    const T hs = (T)st.dt;                                   // rk_common.py:46
    const T t0 = (T)st.t1;                                   // rk_common.py:45
    T zs[NA];
    auto stage = [&](auto sg_c) {
      constexpr int SG = decltype(sg_c)::value;
#pragma unroll
      for (int e = 0; e < NA; ++e) {
        T kk[SG];
#pragma unroll
        for (int j = 0; j < SG; ++j) kk[j] = k[j][e];
        zs[e] = step_combine<T, SG>(z[e], kk, hs, sa);
      }
      T kn[NA];
      adj_dynamics<T, RHS>(rhs, sign * (t0 + (T)sa.alpha[SG - 1] * hs), zs, kn);
#pragma unroll
      for (int e = 0; e < NA; ++e) k[SG][e] = sign * kn[e];
    };
    for_stages<1, S>(stage);
    Acc acc[L::kSeg];
#pragma unroll
    for (int e = 0; e < NA; ++e) {
      T kk[S + 1];
#pragma unroll
      for (int j = 0; j <= S; ++j) kk[j] = k[j][e];
      T err, unused_mid;
      step_finish<T, S>(z[e], kk, hs, sa, err, unused_mid, false);
      Acc& a = acc[L::seg(e)];
      a.maxa = fmax(a.maxa, (double)fabs(z[e]));
      a.maxb = fmax(a.maxb, (double)fabs(zs[e]));            // FSAL shaped: y1 = y_S (rk_common.py:58)
      a.suma += (double)err * (double)err;
    }
    adj_records<L>(rec, acc);
    attempt_core_seg(st, rec, L::kSeg, cp, nullptr, nullptr);
    if (st.accepted) {
      if (st.emit_hi > st.emit_lo) {
        // the one requested time falls into this step: its dense output, in registers (what step_emit writes to a solution plane)
        const T x = interp_x<T>(st.emit_t0, st.emit_t1, cp.t_out[0]);
#pragma unroll
        for (int e = 0; e < NA; ++e) {
          T kk[S + 1];
#pragma unroll
          for (int j = 0; j <= S; ++j) kk[j] = k[j][e];
          T err_unused, zmid;
          step_finish<T, S>(z[e], kk, hs, sa, err_unused, zmid, true);
          T co[5];
          quartic_from_mid<T>(z[e], zs[e], zmid, kk[0], kk[S], (T)st.emit_dt, co);
          z[e] = quartic_eval<T>(co, x);
        }
      } else {
#pragma unroll
        for (int e = 0; e < NA; ++e) { z[e] = zs[e]; k[0][e] = k[S][e]; }       // FSAL (rk_common.py:58)
      }
    }
  }
  res.n_attempt = st.n_attempt; res.n_accept = st.n_accept; res.nfe = st.nfe; res.status = st.status;
}

// What one row reads and writes.  ans / g: this row's first element of output time 0, `plane` elements between output times.
template <typename T>
struct AdjRowIO {
  const T* ans;
  const T* g;
  long long plane;
  T* grad_y0;                  // [D]
  T* grad_params;              // [max(P, 1)]
  T* time_vjps;                // [n_t]
  long long* counts;           // [3][n_t - 1]: attempts, accepted steps, function evaluations of interval k -> k - 1 at index k - 1
};

// neg_t: the n_t output times, negated (the solver's time).  Returns the row's status bits; an interval that ends with one ends the row.
template <typename T, int S, class RHS>
MI_ODE_ROWS_FN unsigned rows_adjoint_row(const RHS& rhs, const StepArgs& sa, CtrlParams cp, const double* neg_t, int n_t, const AdjRowIO<T>& io) {
  using L = AdjLayout<RHS>;
  constexpr int D = L::D, PP = L::PP, NA = L::NA;
  T z[NA];
#pragma unroll
  for (int e = 0; e < NA; ++e) z[e] = (T)0;
#pragma unroll
  for (int d = 0; d < D; ++d) z[D + d] = io.g[(long long)(n_t - 1) * io.plane + d];        // adj_y = grad_output[-1]
  for (int i = 0; i < n_t - 1; ++i) io.counts[i] = io.counts[(n_t - 1) + i] = io.counts[2 * (n_t - 1) + i] = 0;
  for (int i = 0; i < n_t; ++i) io.time_vjps[i] = (T)0;
  unsigned status = 0;
  for (int k = n_t - 1; k >= 1; --k) {
    T f[D];
#pragma unroll
    for (int d = 0; d < D; ++d) z[d] = io.ans[(long long)k * io.plane + d];
    rhs((T)(-neg_t[k]), z, f);
    T dl = f[0] * io.g[(long long)k * io.plane];             // adjoint.py:134-140
#pragma unroll
    for (int d = 1; d < D; ++d) dl = dl + f[d] * io.g[(long long)k * io.plane + d];
    z[2 * D] = z[2 * D] - dl;
    io.time_vjps[k] = dl;
    cp.t_out = neg_t + (k - 1);
    RowResult res;
    adj_interval<T, S, RHS>(rhs, sa, cp, neg_t[k], z, res);
    io.counts[k - 1] = res.n_attempt; io.counts[(n_t - 1) + k - 1] = res.n_accept; io.counts[2 * (n_t - 1) + k - 1] = res.nfe;
    if (res.status != 0u) { status = res.status; break; }
#pragma unroll
    for (int d = 0; d < D; ++d) z[D + d] = z[D + d] + io.g[(long long)(k - 1) * io.plane + d];
  }
  io.time_vjps[0] = z[2 * D];
#pragma unroll
  for (int d = 0; d < D; ++d) io.grad_y0[d] = z[D + d];
#pragma unroll
  for (int p = 0; p < PP; ++p) io.grad_params[p] = z[2 * D + 1 + p];
  return status;
}

}  // namespace mi
