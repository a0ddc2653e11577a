"""Systems, inputs and generated sources of the tests of per-row output times, lengths and tolerances under options={'per_trajectory': True}
(a 2-D `t`, options['t_lengths'], [batch] rtol / atol; csrc/mi_ode_rows_t.h) - shared by the CPU tests, the GPU tests and
`__graft_entry__.build()`, which compiles the rows-t plugins here so that the GPU box does not run hipcc.  The systems are those of
tests/per_trajectory_cases.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import per_trajectory_cases as PC                          # noqa: E402

DTYPES = PC.DTYPES
BATCH = 70                                                  # PC.base_y0(): one full wavefront, one with 6 live lanes, a dead remainder


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def horizon_t(batch=BATCH, T=5, lo=0.5, span=1.0):
    """t[i] = linspace(0, lo + span * i / (batch - 1), T): every row its own horizon."""
    ends = lo + span * np.arange(batch) / max(batch - 1, 1)
    return np.linspace(0., 1., T)[None, :] * ends[:, None]


def ragged(batch=BATCH, T=12, end=1.0):
    """(t [batch, T] with NaN in the padding, lengths cycling through 1 .. T): row i has len_i times linspace(0, end_i, len_i)[: len_i],
    end_i spread over [end / 2, end]."""
    lengths = 1 + np.arange(batch) % T
    t = np.full((batch, T), np.nan)
    for i, n in enumerate(lengths):
        t[i, :n] = np.linspace(0., end * (0.5 + 0.5 * i / max(batch - 1, 1)), n) if n > 1 else 0.
    return t, lengths.astype(np.int32)


def spread_rtol(batch=BATCH):
    """rtol from 1e-3 to 1e-8 over the rows, atol two decades below."""
    r = 10.0 ** np.linspace(-3, -8, batch)
    return r, r * 1e-2


def blow_up_y0(n=9):
    """y' = y^2 rows with their poles at 1 / y0 = 8 / (8 + i)."""
    return 1.0 + np.arange(n)[:, None] / 8.0


# ---- the per-row integration with per-row times as host code ------------------------------------------------------------------------
HOST_T_ENTRY = r"""
// what a lane of k_rows_rowlocal_t does, row after row: t: [batch][T]; len: [batch]; rtol / atol: [batch]; out: [T - 1][batch * D]
template <int S, bool TS, bool FSAL>
static void run_t(const double* tab, const double* ctrl, const double* rhs_scalars, long long batch, const double* y0, const double* t, int T,
                  const int* len, const double* rtol, const double* atol, double* out, long long* stats) {
  constexpr int D = %d;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  const double* p = tab;
  for (int i = 0; i < 13; ++i) sa.alpha[i] = *p++;
  for (int i = 0; i < 13; ++i) for (int j = 0; j < 13; ++j) sa.beta[i][j] = *p++;
  for (int j = 0; j < 14; ++j) sa.csol[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.e[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.cmid[j] = *p++;
  for (int i = 0; i < 8; ++i) sa.rhs.s[i] = rhs_scalars[i];
  sa.rhs.sign = 1.0;
  sa.batch = batch; sa.dim = D; sa.n_plane = batch * D; sa.out = out; sa.interp = (int)ctrl[10];
  CtrlParams base;
  memset(&base, 0, sizeof(base));
  base.safety = ctrl[2]; base.ifactor = ctrl[3]; base.dfactor = ctrl[4];
  base.inv_ifactor = 1.0 / base.ifactor; base.inv_dfactor = 1.0 / base.dfactor;
  base.auto_first_step = 1;
  base.max_num_steps = (long long)ctrl[6]; base.order = (int)ctrl[7]; base.init_order = (int)ctrl[8]; base.controller = (int)ctrl[9];
  base.is_f32 = 0; base.n_stages = S; base.n_local = D;
  sa.cp = base;
  const Rhs<double> rhs(sa.rhs);
  for (long long row = 0; row < batch; ++row) {
    const double* tr = t + row * T;
    CtrlParams cp = base;
    cp.t_out = tr + 1; cp.rtol = rtol[row]; cp.atol = atol[row];
    double y[D], f[D];
    for (int d = 0; d < D; ++d) y[d] = y0[row * D + d];
    RowResult res;
    rows_integrate<double, S, TS, FSAL, Rhs<double>>(rhs, sa, cp, 1.0, tr[0], 0.0, len[row] - 1, y, f, row * D, res);
    stats[row * 4 + 0] = res.n_attempt; stats[row * 4 + 1] = res.n_accept; stats[row * 4 + 2] = res.nfe; stats[row * 4 + 3] = (long long)res.status;
  }
}
extern "C" int rows_run_t(int S, int ts, int fsal, const double* tab, const double* ctrl, const double* rhs_scalars, long long batch, const double* y0,
                          const double* t, int T, const int* len, const double* rtol, const double* atol, double* out, long long* stats) {
  if (S == 6 && fsal && !ts) run_t<6, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, len, rtol, atol, out, stats);
  else if (S == 6 && fsal && ts) run_t<6, true, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, len, rtol, atol, out, stats);
  else if (S == 3 && fsal) run_t<3, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, len, rtol, atol, out, stats);
  else if (S == 13 && fsal) run_t<13, false, true>(tab, ctrl, rhs_scalars, batch, y0, t, T, len, rtol, atol, out, stats);
  else if (S == 1 && !fsal) run_t<1, false, false>(tab, ctrl, rhs_scalars, batch, y0, t, T, len, rtol, atol, out, stats);
  else return -1;
  return 0;
}
"""


def host_source_t(functor, dim):
    """PC.host_source's g++ translation unit (the project's device headers behind host stand-ins, csrc/mi_ode_rows_core.h) with a
    `rows_run_t` entry point that gives every row its own times, length and tolerances, as a lane of k_rows_rowlocal_t does."""
    return PC.host_source(functor, dim) + HOST_T_ENTRY % dim


# ---- one row's whole backward with per-row times as host code -------------------------------------------------------------------------
HOST_ADJ_T_ENTRY = r"""
// what a lane of k_rows_adjoint_t does, row after row: t: [batch][T]; len, rtol, atol: [batch]; counts: [batch][3][T - 1], a row's own
// packed as rows_adjoint_row leaves them ([3][len - 1]) - the caller unpacks
template <int S>
static void run_t(const double* tab, const double* ctrl, const double* ps, const double* cw, long long batch, int T, const double* t, const int* len,
                  const double* rtol, const double* atol, const double* ans, const double* g, double* gy0, double* rowp, double* rowt,
                  long long* counts, long long* status) {
  using R = RhsUser<double>;
  using L = AdjLayout<R>;
  StepArgs sa;
  memset(&sa, 0, sizeof(sa));
  const double* p = tab;
  for (int i = 0; i < 13; ++i) sa.alpha[i] = *p++;
  for (int i = 0; i < 13; ++i) for (int j = 0; j < 13; ++j) sa.beta[i][j] = *p++;
  for (int j = 0; j < 14; ++j) sa.csol[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.e[j] = *p++;
  for (int j = 0; j < 14; ++j) sa.cmid[j] = *p++;
  sa.batch = batch; sa.dim = L::D; sa.n_plane = batch * L::D; sa.interp = MI_ODE_INTERP_QUARTIC_MID;
  CtrlParams base;
  memset(&base, 0, sizeof(base));
  base.safety = ctrl[2]; base.ifactor = ctrl[3]; base.dfactor = ctrl[4];
  base.inv_ifactor = 1.0 / base.ifactor; base.inv_dfactor = 1.0 / base.dfactor;
  base.auto_first_step = 1;
  base.max_num_steps = (long long)ctrl[5]; base.order = (int)ctrl[6]; base.init_order = (int)ctrl[7]; base.controller = MI_ODE_CTRL_MISC;
  base.is_f32 = 0; base.n_stages = S; base.n_local = L::D;
  const R rhs(ps, cw);
  for (long long row = 0; row < batch; ++row) {
    double neg_t[64];
    for (int i = 0; i < len[row]; ++i) neg_t[i] = -t[row * T + i];
    CtrlParams cp = base;
    cp.rtol = rtol[row]; cp.atol = atol[row];
    AdjRowIO<double> io;
    io.ans = ans + row * L::D; io.g = g + row * L::D; io.plane = batch * L::D;
    io.grad_y0 = gy0 + row * L::D; io.grad_params = rowp + row * L::PP; io.time_vjps = rowt + row * T;
    io.counts = counts + row * 3 * (T - 1);
    status[row] = (long long)rows_adjoint_row<double, S, R>(rhs, sa, cp, neg_t, len[row], io);
  }
}
extern "C" int adj_rows_run_t(int S, const double* tab, const double* ctrl, const double* ps, const double* cw, long long batch, int T, const double* t,
                              const int* len, const double* rtol, const double* atol, const double* ans, const double* g, double* gy0, double* rowp,
                              double* rowt, long long* counts, long long* status) {
  if (T > 64) return -1;
  if (S == 6) run_t<6>(tab, ctrl, ps, cw, batch, T, t, len, rtol, atol, ans, g, gy0, rowp, rowt, counts, status);
  else if (S == 3) run_t<3>(tab, ctrl, ps, cw, batch, T, t, len, rtol, atol, ans, g, gy0, rowp, rowt, counts, status);
  else return -1;
  return 0;
}
"""


def host_adjoint_source_t(tr):
    """per_trajectory_adjoint_cases.host_source's g++ translation unit with an `adj_rows_run_t` entry point that gives every row its own
    negated times, length and tolerances, as a lane of k_rows_adjoint_t does."""
    import per_trajectory_adjoint_cases as AC
    return AC.host_source(tr) + HOST_ADJ_T_ENTRY


def ragged_adjoint_t(name, batch, T=5):
    """(t [batch, T] with NaN in the padding, lengths cycling T, 1, 2, .. T - 1) on the interval of the system's own shared times
    (per_trajectory_adjoint_cases.SYSTEMS): row i has len_i times from t_0 to an end of its own."""
    import per_trajectory_adjoint_cases as AC
    base = np.asarray(AC.SYSTEMS[name][5], dtype=np.float64)
    lengths = np.array([T if i % T == 0 else i % T for i in range(batch)], dtype=np.int32)
    t = np.full((batch, T), np.nan)
    for i, n in enumerate(lengths):
        end = base[0] + (base[-1] - base[0]) * (0.5 + 0.5 * i / max(batch - 1, 1))
        t[i, :n] = np.linspace(base[0], end, n) if n > 1 else base[0]
    return t, lengths


# ---- sources build() compiles ---------------------------------------------------------------------------------------------------------
def sources(device='cpu'):
    """The row-local AND the rows-t plugin of every plugin system the tests use (a rows-t call creates its handle from the row-local one,
    and the batch-of-one calls the rows are held to run on it); for the modules of the gradient tests the rows-t plugin of the forward
    and the rows-adjoint-t plugin of the backward (their row-local, rows and rows-adjoint plugins: per_trajectory_adjoint_cases)."""
    import per_trajectory_adjoint_cases as AC
    from tfdiffeq_amd import lower, rhs
    out = []
    for dt in DTYPES:
        for system in (PC.van_der_pol(), PC.blow_up()):
            out += [system.source(dt), system.rows_t_source(dt)]
        for src in lower.sources_for(PC.time_callable, torch.zeros(2, PC.TIME_DIM, dtype=dt, device=device)):
            out += [src, rhs.rows_t_source_of(src)]
    for mod, y0 in AC.modules(device):
        out += [rhs.rows_t_source_of(src) for src in lower.sources_for(mod, y0)]
        out.append(rhs.rows_adjoint_t_source_of(lower.adjoint_source(lower.trace(mod, y0))))
    return out
