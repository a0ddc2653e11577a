/*
 * mi_ode.h - C ABI of the MI355X-native explicit Runge-Kutta ODE engine.
 *
 * This is the drop-in boundary underneath the reference's three Python
 * contracts; the reference itself has no FFI, so each
 * entry point cites the reference interface it replaces (paths relative to
 * /root/reference/tfdiffeq/).  Plain C: integer status returns, raw device
 * pointers + sizes, no exceptions, no torch types.  All work is enqueued on the
 * caller's hipStream_t (passed as void*).  The caller owns every state / output
 * buffer; a handle owns only its workspace (stage planes, block partials, the
 * device-resident controller record).  One handle per host thread; no globals.
 *
 * Two families of entry points:
 *
 *  (A) fused engine  - the RHS f(t, y) is one of the device catalogue kinds and
 *      is evaluated INSIDE each stage kernel (y_sigma is never materialised),
 *      the step-size controller runs on the device, dense output is emitted by
 *      a kernel.  Replaces, for a single [batch, dim] state tensor:
 *        Dopri5Solver / Tsit5Solver / Bosh3Solver .before_integrate + .advance
 *          (dopri5.py:70-121, tsit5.py:91-151, bosh3.py:53-99)
 *        _runge_kutta_step                      (rk_common.py:22-61)
 *        _compute_error_ratio / _optimal_step_size / _select_initial_step
 *                                               (misc.py:183-287, tsit5.py:53-62)
 *        _interp_fit / _interp_evaluate         (interp.py:6-67, tsit5.py:33-50)
 *        FixedGridODESolver.integrate + Euler/RK4.step_func
 *                                               (solvers.py:82-104, fixed_grid.py:4-46)
 *
 *  (B) stateless plane kernels - for an arbitrary Python callable f (evaluated
 *      by the caller between launches) and tuple states.  They are the fused
 *      equivalents of the reference's eager-op sequences:
 *        mi_ode_lincomb        <- misc._scaled_dot_product (misc.py:118-121)
 *        mi_ode_error_norms    <- misc._compute_error_ratio reductions (misc.py:256-263)
 *        mi_ode_scaled_sumsq   <- misc._norm(x / scale)   (misc.py:170-175, 225-237)
 *        mi_ode_interp_eval    <- interp._interp_fit + _interp_evaluate / tsit5._interp_eval_tsit5
 *
 *  (C) opaque right-hand side, controller on the device (mi_ode_opq_*) - f is still
 *      evaluated by the caller between launches, but an attempt contains no host
 *      decision, so the caller can record it once as a hipGraph and replay it:
 *        mi_ode_opq_finish     <- rk_common.py:60 (error estimate) + misc._compute_error_ratio +
 *                                 the accept test + misc._optimal_step_size (dopri5.py:103-121)
 *        mi_ode_opq_commit     <- the accepted branch of _adaptive_dopri5_step (dopri5.py:113-121)
 *                                 + Dopri5Solver.advance's _interp_evaluate (dopri5.py:87)
 */
#ifndef MI_ODE_H
#define MI_ODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: mi_ode_desc.multistep (fixed-grid Adams family).  10: multistep = 3 + ms_gamma_star (variable-order Adams), the four
 * mi_ode_adams_* plane entry points.  11: family (C) mi_ode_opq_* (opaque right-hand side, device-resident controller: what a
 * captured hipGraph of an attempt needs), mi_ode_stats.clock_mhz.
 * 13: (A''') mi_ode_linadj_* - the backward segment of odeint_adjoint for the linear right-hand side in one launch. */
#define MI_ODE_ABI_VERSION 13
#define MI_ODE_MAX_STAGES 13         /* rows of the tableau (dopri8 = 13, dopri5 / tsit5 = 6, bosh3 = 3, rk4 = 3, adaptive_heun = 1) */
#define MI_ODE_MAX_K (MI_ODE_MAX_STAGES + 1)
#define MI_ODE_MAX_LINCOMB 14        /* stateless lincomb: up to 14 planes (dopri8: f0 + 13 stages) */
#define MI_ODE_MAX_SEGMENTS 8        /* components of a tuple state packed into one buffer (mi_ode_desc.n_segments) */

/* ---- status bits (also the bits of mi_ode_stats.status) --------------------------------- */
#define MI_ODE_OK 0
#define MI_ODE_ST_DT_UNDERFLOW 0x1u    /* assert t0 + dt > t0            (dopri5.py:98)      */
#define MI_ODE_ST_NONFINITE 0x2u       /* assert _is_finite(abs(y0))     (dopri5.py:99-100)  */
#define MI_ODE_ST_MAX_STEPS 0x4u       /* assert n_steps < max_num_steps (dopri5.py:85-86)   */
#define MI_ODE_ST_SYNC_TIMEOUT 0x10u   /* engine: the in-kernel grid hand-off of the whole-integration kernel timed out */
#define MI_ODE_ST_BAD_T 0x8u           /* _assert_increasing / interpolation range (misc.py:158, interp.py:59) */
/* negative returns: API errors */
#define MI_ODE_E_INVALID (-1)          /* bad argument / unsupported combination */
#define MI_ODE_E_HIP (-2)              /* a HIP runtime call failed (see mi_ode_last_error) */
#define MI_ODE_E_NODEVICE (-3)
#define MI_ODE_E_EXCHANGE (-4)         /* the multi-rank exchange callback failed */

enum mi_ode_dtype { MI_ODE_F32 = 0, MI_ODE_F64 = 1 };

/* Device RHS catalogue.  All are trajectory(row)-local on a [batch, dim] row-major state.      */
enum mi_ode_rhs_kind {
  MI_ODE_RHS_LINEAR = 1,         /* f = y @ W (+ b)            W [dim,dim] row-major  (config 4: W = A^T)
                                    3 <= dim <= 128: MFMA tile kernels, W slices resident in registers (every schedule);
                                    129 <= dim <= 256 (round 6): 256-wide MFMA tile kernels, W streamed from a copy in
                                    consumption order - three- / six-row FSAL tableaus and the fixed grid, whole call /
                                    per attempt; anything else up to dim 256: vector-ALU stage kernels               */
  MI_ODE_RHS_CUBIC_LINEAR = 2,   /* f = (y**3) @ W             examples/ode_demo.py:33-35 (spiral)          */
  MI_ODE_RHS_LOTKA_VOLTERRA = 3, /* dim 2: [a u - b u v, -c v + d u v]   scalars = {a,b,c,d}                */
  MI_ODE_RHS_LORENZ = 4,         /* dim 3: examples/lorenz_attractor.py:20-37, scalars = {sigma,beta,rho}   */
  MI_ODE_RHS_MLP_TANH = 5,       /* dim->hidden->hidden->dim MLP of models/dense_odenet.py:41-92; hidden activation =
                                    scalars[0]: 0 tanh, 1 relu (the reference's default, :14), 2 softplus;
                                    scalars[1] != 0: time dependent (:79-84, fc1 sees concat([t, x])): w[0] is
                                    [dim + 1, hidden] and its row 0 multiplies the stage time.  float32, dim <= 64,
                                    hidden <= 128: MFMA tile kernels (every Runge-Kutta schedule).  Otherwise (float32 /
                                    float64, dim, hidden <= 256; round 5): a cooperative kernel, a thread per state element -
                                    adaptive 3- / 6-row tableaus as ONE launch per call (fusion 0 / 4, one rank, co-resident
                                    grid, T > 1: else MI_ODE_E_INVALID) and multistep != 0 (the Adams family in one launch) */
  MI_ODE_RHS_PLUGIN = 6          /* user device code for a trajectory-local system: mi_ode_rhs.plugin (csrc/mi_ode_plugin.h) -
                                    a trajectory per thread (dim <= 32) or, with mi_ode_rowlocal_plugin.cooperative = 1, a
                                    state element per thread (dim <= 256; adaptive methods as one launch per call, euler /
                                    rk4, the Adams family); scalars[0..7] and w[]/b[] are passed through to it          */
};

enum mi_ode_controller {
  MI_ODE_CTRL_MISC = 0,          /* misc._optimal_step_size: sqrt + float32-rounded exponent (misc.py:267-287) */
  MI_ODE_CTRL_TSIT5 = 1          /* tsit5._optimal_step_size: no sqrt, float64 exponent     (tsit5.py:53-62)  */
};

enum mi_ode_interp {
  MI_ODE_INTERP_QUARTIC_MID = 0, /* interp._interp_fit/_interp_evaluate with y_mid from c_mid (dopri5, bosh3) */
  MI_ODE_INTERP_TSIT5 = 1,       /* tsit5 seven-weight dense output from y0 (corrected)                       */
  MI_ODE_INTERP_TSIT5_REF = 2    /* tsit5 dense output from k[0] = f0, exactly as tsit5.py:45-50 (defect F6b) */
};

/* _ButcherTableau(alpha, beta, c_sol, c_error) (rk_common.py:5) + the dense-output mid-point weights. */
typedef struct mi_ode_tableau {
  int32_t n_stages;                                   /* S = len(alpha) */
  int32_t fsal;                                       /* 1 iff c_sol[-1]==0 and c_sol[:-1]==beta[-1] (rk_common.py:54) */
  double alpha[MI_ODE_MAX_STAGES];
  double beta[MI_ODE_MAX_STAGES][MI_ODE_MAX_STAGES];  /* row sigma uses entries [0..sigma] */
  double c_sol[MI_ODE_MAX_K];
  double c_error[MI_ODE_MAX_K];
  double c_mid[MI_ODE_MAX_K];                         /* DPS_C_MID / BS_C_MID; unused for tsit5 */
} mi_ode_tableau;

typedef struct mi_ode_rhs {
  int32_t kind;               /* enum mi_ode_rhs_kind */
  int32_t hidden;             /* MLP hidden width (else 0) */
  double sign;                /* +1, or -1 for a reversed time axis: f <- -f(-t, y) (misc.py:318-321) */
  double scalars[8];          /* kind specific scalars */
  const void* w[3];           /* device pointers, state dtype: LINEAR/CUBIC {W}; MLP {W1,W2,W3} ([in,out] row-major) */
  const void* b[3];           /* device pointers (nullable): biases */
  const void* plugin;         /* MI_ODE_RHS_PLUGIN: what the plugin's mi_ode_plugin_get(dtype) returned */
} mi_ode_rhs;

/* Exchange hook for batch-sharded runs: all-gather `count` doubles per rank.
 * sendbuf/recvbuf are DEVICE pointers; the hook must enqueue the collective so that it is ordered
 * after prior work on `stream` and before later work on it (RCCL via torch.distributed in the
 * Python shim).  recvbuf holds world_size * count doubles in rank order.  Return 0 on success. */
typedef int (*mi_ode_allgather_fn)(void* user, const void* sendbuf, void* recvbuf, int32_t count, void* stream);

typedef struct mi_ode_desc {
  int32_t dtype;              /* enum mi_ode_dtype: state dtype (time is always double in adaptive solvers) */
  int32_t adaptive;           /* 1: adaptive tableau solver; 0: fixed grid (tableau = the RK scheme, c_error unused) */
  int64_t batch;              /* rows held by THIS rank */
  int64_t dim;                /* state width */
  mi_ode_tableau tableau;
  mi_ode_rhs rhs;
  int32_t controller;         /* enum mi_ode_controller */
  int32_t interp;             /* enum mi_ode_interp */
  int32_t order;              /* controller order: 5 (dopri5, tsit5), 3 (bosh3)      (dopri5.py:68, bosh3.py:93) */
  int32_t init_order;         /* order passed to _select_initial_step: 4 / 2         (dopri5.py:74, bosh3.py:56) */
  double rtol, atol;          /* rtol[0], atol[0] of the reference's per-component lists */
  double safety, ifactor, dfactor;   /* pass the float32-rounded values the reference ends up with (misc.py:137-144) */
  double first_step;          /* NaN: select automatically (misc.py:183-247) */
  int64_t max_num_steps;      /* per output time, rejected attempts included (dopri5.py:83-88) */
  /* batch sharding (world_size 1: leave zero / NULL) */
  int32_t world_size, rank;
  mi_ode_allgather_fn allgather;
  void* allgather_user;
  double* exchange_send_dev;  /* optional caller-owned device buffers (8 doubles / world_size*8 doubles) that the */
  double* exchange_recv_dev;  /* hook gathers from / into; NULL: the handle allocates its own */
  /* tuning knobs (0 = default) */
  int32_t linear_variant;     /* 0 auto, 1 force VALU fallback, 2 force MFMA tile kernel */
  int32_t chunk_attempts;     /* attempts enqueued between host polls (0 = adaptive) */
  int32_t reserved0;          /* (was a hipGraph knob: the attempt chain is GPU-latency-bound, not launch-bound - DESIGN.md) */
  int32_t profile;            /* 1: bracket the stage kernels of every attempt with HIP events (mi_ode_get_profile) */
  int32_t fusion;             /* 0 auto, 1 one kernel per RK stage (34 planes/attempt), 2 whole attempt in one kernel
                                 (4 planes/attempt; row-local RHS keep k_2..k_S on chip; single rank: the controller
                                 runs in the kernel's last workgroup), 3 as 2 but with the controller as its own launch,
                                 4 whole integration in ONE launch (tiny row-local systems, single rank; auto picks it
                                 when every workgroup can be co-resident; mi_ode_integrate only) */
  int32_t reserved;
  /* Optional cross-rank hand-off memory for the whole-call kernels (world_size > 1): a HOST memory segment shared by
   * all ranks of the node (e.g. a /dev/shm mapping), at least mi_ode_xrank_bytes(world_size) bytes, zero-filled before the
   * first use.  The handle registers it with HIP; its kernels then exchange their per-attempt records through it
   * (system-scope stores / loads over PCIe or xGMI, no host involvement, no collective launch), so a sharded run keeps
   * the one-launch-per-call schedule.  The allgather hook stays the fallback (mi_ode_xrank_enable). */
  void* xrank_host;
  int64_t xrank_bytes;
  /* Tuple states (odeint.py:28-81: y0 may be a tuple of tensors; the RHS is applied to every component).  The components -
   * each [rows_k, dim] - travel in ONE buffer with a segment table: component k starts at a multiple of MI_ODE_SEGMENT_ALIGN
   * rows (the caller pads; padding rows are never read or written) and has seg_rows[k] rows; `batch` = the padded total.  The
   * scalar decisions run per component exactly as in the reference: one error ratio each (misc.py:250-264), accepted if all
   * are <= 1 (dopri5.py:108), python max() of them for the next step (misc.py:270) and over the per-component norms of the
   * initial step (misc.py:227-245); with the tsit5 controller ONE ratio pooled over all components (tsit5.py:126-138).
   * n_segments <= 1: a single tensor.  Row-local right-hand sides (catalogue and plugins), adaptive tableaus, one rank,
   * whole-call schedule. */
  int32_t n_segments;
  int32_t seg_tolerances;     /* 1: seg_rtol / seg_atol hold one pair per component (dopri5.py:60-61 accepts lists); 0: rtol / atol for all */
  int64_t seg_rows[MI_ODE_MAX_SEGMENTS];
  double seg_rtol[MI_ODE_MAX_SEGMENTS], seg_atol[MI_ODE_MAX_SEGMENTS];   /* (the initial step uses rtol / atol = the first pair, dopri5.py:74) */
  /* Fixed-grid multistep solvers (adaptive = 0; the tableau is ignored): the reference's AdamsBashforth / AdamsBashforthMoulton
   * (fixed_adams.py:152-212) as ONE launch per mi_ode_fixed_grid_integrate[_on] call, for the row-local catalogue systems.
   * ms_ab / ms_am / ms_am0 are HOST arrays, copied at create, holding the coefficients as the reference forms them in Python
   * floats: ms_ab[o * 12 + j] = (1 / DIVISOR[o]) * BASHFORTH[o][j], ms_am[o * 12 + j] = (1 / DIVISOR[o + 1]) * MOULTON[o + 1][j + 1],
   * ms_am0[o] = MOULTON[o + 1][0] / DIVISOR[o + 1], o = 0 .. 12 (rows of unused orders: zeros).  rtol / atol: the corrector's
   * convergence test (misc.py:129-134; odeint passes ITS rtol / atol).  stats.n_rejected = steps whose corrector did not converge
   * (the reference prints a warning for each and drops its oldest history entry, fixed_adams.py:197-200). */
  int32_t multistep;          /* 0: none, 1: Adams-Bashforth ('explicit_adams'), 2: Adams-Bashforth-Moulton ('fixed_adams'),
                               * 3: the variable-step, variable-order Adams solver ('adams', adams.py:66-211; ABI 10): adaptive = 1, the whole
                               * mi_ode_integrate call is ONE launch for the row-local catalogue systems (csrc/mi_ode_adams_vc.h); uses
                               * rtol / atol / safety / ifactor / dfactor, ms_max_order (<= 12) and ms_gamma_star; the tableau is ignored */
  int32_t ms_max_order;       /* <= 12 (fixed_adams.py:89) */
  int32_t ms_max_iters;       /* corrector iterations (fixed_adams.py:90: 4) */
  int32_t ms_min_order;       /* below it the start-up RK4 3/8 step runs (fixed_adams.py:88: 4) */
  const double* ms_ab;
  const double* ms_am;
  const double* ms_am0;
  const double* ms_gamma_star; /* multistep = 3: HOST array of 13 doubles (adams.py:15-18), copied at create */
} mi_ode_desc;
#define MI_ODE_SEGMENT_ALIGN 256

typedef struct mi_ode_stats {
  int64_t n_attempts, n_accepted, n_rejected, nfe;
  double t, dt;               /* rk_state.t1 and the next step size */
  double last_ratio;          /* last mean_sq_error_ratio */
  uint32_t status;            /* MI_ODE_ST_* bits */
  int32_t n_polls;            /* host synchronisations taken */
  int64_t n_launches;         /* kernels enqueued */
  double clock_mhz;           /* shader clock the one-launch kernels of the call ran at (their own cycle counter against the
                                 100 MHz constant clock); 0 where not measured */
  double handoff_us;          /* ABI 13: time workgroup 0 of the whole-call linear tile kernel spent in the call's grid hand-offs (the
                                 cross-rank exchange of a sharded run included); 0 where not measured */
} mi_ode_stats;

typedef struct mi_ode_solver* mi_ode_handle;

/* ---- library ------------------------------------------------------------------------------ */
int mi_ode_abi_version(void);
const char* mi_ode_status_string(uint32_t status_bits);   /* reference assertion text for the first set bit */
const char* mi_ode_last_error(void);                      /* thread-local text of the last negative return */
int64_t mi_ode_reduce_workspace_bytes(void);              /* scratch the stateless reductions need */
int64_t mi_ode_sizeof(int32_t which);                     /* 0: mi_ode_desc, 1: mi_ode_stats, 2: mi_ode_tableau, 3: mi_ode_rhs,
                                                             5: mi_ode_ctrl_params, 6: mi_ode_adjoint_desc, 7: mi_ode_opq_desc, 8: mi_ode_linadj_desc,
                                                             9: mi_ode_discrete_desc, 10: mi_ode_discrete_row_desc, 11: mi_ode_discrete_linear_desc,
                                                             12: mi_ode_discrete_linear_grid_desc
                                                             (lets a foreign-language binding verify its struct layout) */

/* ---- (A) fused engine ---------------------------------------------------------------------- */
int mi_ode_create(const mi_ode_desc* desc, mi_ode_handle* out);
int mi_ode_destroy(mi_ode_handle h);

/* Solver.before_integrate(t): load y0, evaluate f0, pick the first step (dopri5.py:70-79). */
int mi_ode_begin(mi_ode_handle h, const void* y0_dev, double t0, void* stream);
/* Solver.advance(next_t) for n_out strictly increasing times (dopri5.py:81-89); out_dev: [n_out, batch*dim].
 * Blocks until the outputs are produced or a status bit is raised; returns status bits (>=0) or an error (<0). */
int mi_ode_advance(mi_ode_handle h, const double* t_out_host, int32_t n_out, void* out_dev, void* stream);
/* AdaptiveStepsizeODESolver.integrate(t) (solvers.py:27-35): out_dev [T, batch*dim], out[0] = y0. */
int mi_ode_integrate(mi_ode_handle h, const void* y0_dev, const double* t_host, int32_t T, void* out_dev,
                     mi_ode_stats* stats, void* stream);
/* Per-trajectory step control (csrc/mi_ode_rows.h): the same call for a batch of INDEPENDENT systems.  Row i of out_dev is what
 * mi_ode_integrate returns for y0[i] alone, bit for bit: every row has its own initial step, error ratio over its dim elements,
 * accept / reject sequence, output cursor and dense output, max_num_steps and dt-underflow checks; t, rtol, atol and the other
 * options of the handle are shared.  One launch for any batch size, no co-residency requirement.
 *   h             an adaptive handle created for a trajectory-per-thread right-hand side (lotka_volterra, lorenz, 2 x 2 linear /
 *                 cubic-linear without bias, a row-local plugin), one state tensor, one rank - anything else: MI_ODE_E_INVALID
 *   rows_plugin   the table mi_ode_rows_plugin_get(dtype) of the plugin's rows shared object returned (csrc/mi_ode_rows_plugin.h)
 *                 when the handle's right-hand side is a row-local plugin; NULL for the catalogue systems
 *   row_stats_dev device [batch, 4] int64: attempts, accepted steps, function evaluations, status bits (MI_ODE_ST_*) of every row
 *   stats         (nullable) n_attempts / n_accepted / n_rejected / nfe: the MAXIMUM over the rows; status: the OR over the rows
 * A row that fails sets its own status and stops; the other rows are integrated to the end.  Returns the OR of the rows' status
 * bits (>= 0) or an error (< 0). */
int mi_ode_integrate_rows(mi_ode_handle h, const void* rows_plugin, const void* y0_dev, const double* t_host, int32_t T,
                          void* out_dev, int64_t* row_stats_dev, mi_ode_stats* stats, void* stream);
/* The same with output times, lengths and tolerances of every row's own (csrc/mi_ode_rows_t.h).  Row i of out_dev is what
 * mi_ode_integrate returns for y0[i] alone with the times t_dev[i][0 .. len_i - 1] on a handle whose rtol / atol are rtol_dev[i] /
 * atol_dev[i], bit for bit; out_dev[k][i] for k >= len_i is exactly 0 and t_dev[i][len_i ..] is never read.
 *   h, row_stats_dev, stats, the return value: as for mi_ode_integrate_rows (stats->t is 0: every row ends at a time of its own)
 *   rows_t_plugin the table mi_ode_rows_t_plugin_get(dtype) of the plugin's rows-t shared object returned
 *                 (csrc/mi_ode_rows_t_plugin.h) when the handle's right-hand side is a row-local plugin; NULL for the catalogue systems
 *   t_dev         DEVICE [batch][T] float64, every row strictly increasing over its own length (the caller checks that: nothing of
 *                 it is read on the host; times that are not can give wrong numbers or a status bit, never an unbounded loop)
 *   len_dev       DEVICE [batch] int32 with values in 1 .. T (clamped to that range by the kernel), or NULL: every row has T times
 *   rtol_dev, atol_dev   DEVICE [batch] float64 each, or NULL: the handle's value for every row
 * One launch and one synchronisation, as there. */
int mi_ode_integrate_rows_t(mi_ode_handle h, const void* rows_t_plugin, const void* y0_dev, const double* t_dev, int32_t T,
                            const int32_t* len_dev, const double* rtol_dev, const double* atol_dev, void* out_dev,
                            int64_t* row_stats_dev, mi_ode_stats* stats, void* stream);
/* Per-trajectory step control for the ODEFunc network on the matrix cores (csrc/mi_ode_rows_mlp.h): the same call for a handle of the
 * fp32 MLP tile family.  A 32-row tile runs through the whole call with the weights resident; the control flow is workgroup-uniform and
 * every row of the tile has its own initial step, error ratio over its dim elements, accept / reject sequence, output cursor and dense
 * output, max_num_steps and dt-underflow checks.  A row's numbers do not depend on the rows it shares a tile with: out_dev[:, i] is what
 * the call computes for y0[i] alone, bit for bit, however the batch is sliced or ordered.  One launch for any batch size, no
 * co-residency requirement.
 *   h             an adaptive float32 handle created for an MI_ODE_RHS_MLP right-hand side inside the tile kernels' box (dim <= 64,
 *                 hidden <= 128; relu, softplus or tanh; with or without the time input), the FSAL shaped 6-row (dopri5, tsit5) or 3-row
 *                 (bosh3) tableau, one state tensor, one rank - anything else: MI_ODE_E_INVALID
 *   desc          launch options (below); sizeof(mi_ode_rows_mlp_desc) = mi_ode_rows_mlp_sizeof()
 *   row_stats_dev, stats, the return value: as for mi_ode_integrate_rows */
typedef struct mi_ode_rows_mlp_desc {
  int32_t grid;               /* 0: the library chooses (a workgroup per 32-row tile, capped); > 0: at most this many workgroups - they
                                 loop over the tiles (results do not depend on it) */
  int32_t reserved;           /* 0 */
} mi_ode_rows_mlp_desc;
int mi_ode_integrate_rows_mlp(mi_ode_handle h, const mi_ode_rows_mlp_desc* desc, const void* y0_dev, const double* t_host, int32_t T,
                              void* out_dev, int64_t* row_stats_dev, mi_ode_stats* stats, void* stream);
int64_t mi_ode_rows_mlp_sizeof(void);                     /* sizeof(mi_ode_rows_mlp_desc), for a binding's layout check */
/* A fixed-grid solve (euler / rk4 on the default grid) with output times and a length of every row's own (csrc/mi_ode_fixed_rows_t.h).
 * Row i of out_dev is what mi_ode_fixed_grid_integrate returns for y0[i] alone with the times t_dev[i][0 .. len_i - 1], bit for bit;
 * out_dev[k][i] for k >= len_i is exactly 0 and t_dev[i][len_i ..] is never read.
 *   h             a fixed-grid handle (adaptive 0, no multistep; the euler or the rk4 3/8 tableau) of a trajectory-per-thread right-hand
 *                 side, one state tensor on one rank
 *   fixed_rows_t_plugin   the table mi_ode_fixed_rows_t_plugin_get(dtype) of the plugin's fixed-rows-t shared object returned
 *                 (csrc/mi_ode_fixed_rows_t_plugin.h) when the handle's right-hand side is a row-local plugin; NULL for the catalogue systems
 *   t_dev         DEVICE [batch][T] float64, every row strictly increasing over its own length, values already rounded to the state
 *                 dtype (the caller checks that: nothing of it is read on the host; times that are not give wrong numbers, never an
 *                 access outside the row)
 *   len_dev       DEVICE [batch] int32 with values in 1 .. T (clamped to that range by the kernel), or NULL: every row has T times
 *   out_dev       [T, batch, dim]
 * One launch and one synchronisation; returns 0 or a negative MI_ODE_E_* (MI_ODE_E_INVALID for null arguments or another handle). */
int mi_ode_integrate_fixed_rows_t(mi_ode_handle h, const void* fixed_rows_t_plugin, const void* y0_dev, const double* t_dev, int32_t T,
                                  const int32_t* len_dev, void* out_dev, mi_ode_stats* stats, void* stream);
/* FixedGridODESolver.integrate(t) with grid = t (solvers.py:82-104); no host synchronisation inside. */
int mi_ode_fixed_grid_integrate(mi_ode_handle h, const void* y0_dev, const double* t_host, int32_t T,
                                void* out_dev, mi_ode_stats* stats, void* stream);
/* The same on a time grid of its own (FixedGridODESolver(step_size=... | grid_constructor=..., eps=...), solvers.py:41-56, 86-100):
 * steps are taken on grid_host[0..G-1] (grid[0] == t[0], grid[G-1] == t[T-1]); a requested time that is not a grid point is
 * linearly interpolated inside the step that reaches it (_linear_interp, solvers.py:106-115); `eps` is added to the time the
 * step function evaluates f at (fixed_grid.py:7, 42).  One launch; row-local and MFMA-linear RHS families. */
int mi_ode_fixed_grid_integrate_on(mi_ode_handle h, const void* y0_dev, const double* grid_host, int32_t G,
                                   const double* t_host, int32_t T, double eps, void* out_dev, mi_ode_stats* stats, void* stream);
/* One attempt with a given dt - the parity surface mirroring _runge_kutta_step (rk_common.py:22-61):
 * y1/f1/err_norms outputs are device pointers (nullable); err_norms = {max|y0|, max|y1|, sum err^2, nonfinite}.
 * k_out (nullable): [S+1, batch*dim] stage derivatives. */
int mi_ode_rk_step_fused(mi_ode_handle h, const void* y0_dev, const void* f0_dev, double t0, double dt,
                         void* y1_dev, void* f1_dev, double* err_norms_host, void* k_out_dev, void* stream);
/* f(t, y) through the fused kernels (y0 -> f0), e.g. to seed mi_ode_rk_step_fused. */
int mi_ode_eval_rhs(mi_ode_handle h, const void* y_dev, double t, void* f_dev, void* stream);
int mi_ode_get_stats(mi_ode_handle h, mi_ode_stats* stats, void* stream);
/* Kernel timing collected with hipEvents on the launch stream when desc.profile = 1 (real attempts only):
 * out[0] = sum of last-stage (stage+error kernel) durations [ms], out[1] = number of those launches,
 * out[2] = sum over attempts of the span first-stage-start .. last-stage-end [ms], out[3] = attempts counted. */
int mi_ode_get_profile(mi_ode_handle h, double* out4);
/* current rk_state: y1, f1 (device, nullable). */
int mi_ode_get_state(mi_ode_handle h, void* y_dev, void* f_dev, void* stream);

/* Cross-rank hand-off (mi_ode_desc.xrank_host).  mi_ode_xrank_selftest: every rank of the group calls it at the same
 * point; a few hand-off rounds run through the shared segment with a bounded wait; returns 0 when this rank saw every
 * peer's records intact.  The caller combines the verdicts (e.g. all-reduce MIN) and calls mi_ode_xrank_enable(h, 1) on
 * every rank only if all passed; otherwise the allgather hook keeps being used. */
int64_t mi_ode_xrank_bytes(int32_t world_size);
int mi_ode_xrank_selftest(mi_ode_handle h, void* stream);
int mi_ode_xrank_enable(mi_ode_handle h, int32_t on);

/* The same hand-off through PEER DEVICE MEMORY - the transport for the GPUs of one xGMI node (the only
 * cross-rank traffic of the path is one 6-double record per rank per step attempt; no reference counterpart, the
 * reference is single-device).  Every rank owns a mailbox in its own HBM:
 *   mi_ode_xpeer_prepare  allocates it (uncached device memory, mi_ode_xrank_bytes(world_size) bytes, zeroed) and returns
 *                         its hipIpcMemHandle_t (MI_ODE_IPC_HANDLE_BYTES bytes) for the caller to all-gather over any
 *                         channel it has (torch.distributed in the Python shim, MPI, a file ...);
 *   mi_ode_xpeer_connect  takes the handles of ALL ranks in rank order, maps the peers' mailboxes into this process
 *                         (hipIpcOpenMemHandle; entry `rank` is this rank's own allocation) and hands the pointer table
 *                         to the kernels.  From then on mi_ode_xrank_selftest / mi_ode_xrank_enable use this transport
 *                         (it takes precedence over xrank_host): each rank's gateway lane q stores the rank record
 *                         into rank q's mailbox over the link to q and polls only its own, local mailbox.
 * Both return 0 or a negative error; a failure leaves the handle on its previous transport. */
#define MI_ODE_IPC_HANDLE_BYTES 64
int mi_ode_xpeer_prepare(mi_ode_handle h, void* ipc_handle_out);
int mi_ode_xpeer_connect(mi_ode_handle h, const void* all_ipc_handles, int32_t world_size);

/* RCCL from inside the library, for the launch-per-attempt schedule (ranks on several nodes, or no usable mailbox):
 * the per-attempt record exchange becomes ncclAllGather(send, recv, 8, ncclDouble, comm, stream) enqueued by
 * libmi_ode itself between the attempt kernel and the controller kernel - no callback into the host language.
 * librccl is taken from the process if it is already loaded (PyTorch-ROCm ships one), else dlopen'ed.
 *   mi_ode_rccl_unique_id   ncclGetUniqueId into id_out (MI_ODE_RCCL_ID_BYTES bytes); rank 0 calls it and broadcasts the bytes;
 *   mi_ode_rccl_connect     ncclCommInitRank(world_size, id, rank) (collective over the ranks); the communicator belongs to the
 *                           handle and is destroyed with it.  Takes precedence over mi_ode_desc.allgather.  id == NULL: drop the
 *                           communicator again (when some rank could not join, every rank has to fall back together). */
#define MI_ODE_RCCL_ID_BYTES 128
int mi_ode_rccl_unique_id(void* id_out);
int mi_ode_rccl_connect(mi_ode_handle h, const void* id, int32_t world_size, int32_t rank);

/* ---- (A') fused backward segment of odeint_adjoint --------------------------------------------------------------- */
/* tfdiffeq/adjoint.py:57-178: the reference's backward pass calls odeint on the augmented tuple state
 *     (y, adj_y, adj_t, adj_params)   with dynamics   (f, -adj_y^T df/dy, -adj_y^T df/dt, -adj_y^T df/dparams)
 * over [t_i, t_{i-1}] (adjoint.py:148-153), once per output interval.  This entry point is that call for the ODEFunc MLP
 * (MI_ODE_RHS_MLP_TANH, fp32, state [batch, dim]) in ONE launch: dopri5 over all four components, per-component error
 * ratios and their max (misc.py:250-287), initial step over all components (misc.py:183-247), dense output at t_end
 * (interp.py:6-67).  adj_params is one flat vector in CANONICAL order W1 [dim,hidden], b1, W2 [hidden,hidden], b2,
 * W3 [hidden,dim], b3 (weights [in, out] row-major as in mi_ode_rhs.w); mi_ode_adjoint_num_params() entries. */
typedef struct mi_ode_adjoint_desc {
  int64_t batch;
  int32_t dim, hidden;
  mi_ode_tableau tableau;     /* dopri5: 6 rows, FSAL shaped, c_mid filled, c_sol[1] = c_error[1] = c_mid[1] = 0 */
  double rtol, atol;          /* scalars: adjoint.py passes them through to every component (dopri5.py:60-61) */
  double safety, ifactor, dfactor;
  int32_t order, init_order;
  int64_t max_num_steps;
  int32_t time_dependent;     /* 1: the network of dense_odenet.py:79-84 with time_dependent=True - fc1 sees concat([t, x]): mi_ode_rhs.w[0]
                               * is [dim + 1, hidden] (row 0 = w_t multiplies t, mi_ode_rhs.scalars[1] != 0), adj_t has the derivative
                               * -adj_y^T df/dt, and adj_params starts with the `hidden` entries of w_t (canonical order
                               * w_t, W1 [dim,hidden], b1, W2, b2, W3, b3) */
  int32_t reserved;
} mi_ode_adjoint_desc;
typedef struct mi_ode_adjoint* mi_ode_adjoint_handle;
int mi_ode_adjoint_create(const mi_ode_adjoint_desc* desc, mi_ode_adjoint_handle* out);
int mi_ode_adjoint_destroy(mi_ode_adjoint_handle h);
int64_t mi_ode_adjoint_num_params(mi_ode_adjoint_handle h);
/* One backward interval t_start -> t_end (either direction; decreasing time is handled as misc._check_inputs does,
 * misc.py:311-321).  All state pointers are DEVICE memory, fp32; adj_t is a device scalar.  rhs: the weights (sign is ignored).
 * y_out is nullable (the reference discards it, adjoint.py:155-160).  Blocks until done; returns status bits or an error. */
int mi_ode_adjoint_segment(mi_ode_adjoint_handle h, const mi_ode_rhs* rhs, const void* y_dev, const void* adj_y_dev,
                           const void* adj_t_dev, const void* adj_params_dev, double t_start, double t_end, void* y_out_dev,
                           void* adj_y_out_dev, void* adj_t_out_dev, void* adj_params_out_dev, mi_ode_stats* stats, void* stream);
/* One evaluation of the augmented dynamics (adjoint.py:69-105), the function-level parity surface of the kernel:
 * f_out = f(y), vjp_y_out = -adj_y^T df/dy, vjp_params_out = -adj_y^T df/dparams (canonical order). */
int mi_ode_adjoint_dynamics(mi_ode_adjoint_handle h, const mi_ode_rhs* rhs, const void* y_dev, const void* adj_y_dev,
                            void* f_out_dev, void* vjp_y_out_dev, void* vjp_params_out_dev, void* stream);
/* ... at time t (the time-dependent network; mi_ode_adjoint_dynamics evaluates at t = 0).  -adj_y^T df/dt is not a separate output:
 * it is dot(w_t, b1 slice of vjp_params_out) (the identity the segment kernel integrates adj_t with). */
int mi_ode_adjoint_dynamics_at(mi_ode_adjoint_handle h, const mi_ode_rhs* rhs, double t, const void* y_dev, const void* adj_y_dev,
                               void* f_out_dev, void* vjp_y_out_dev, void* vjp_params_out_dev, void* stream);

/* ---- (A'') the linear right-hand side under odeint_adjoint -------------------------------------------------------- */
/* tfdiffeq/adjoint.py:69-105 for f(t, y) = y W + b: the augmented dynamics are (y W + b, -adj_y W^T, 0, -(y^T adj_y), -sum_rows adj_y).
 * The first two are the linear right-hand side itself (mi_ode_eval_rhs of a handle created with W, and of one created with -W^T);
 * the parameter part is a GEMM with M = N = dim and K = batch - the shape vendor BLAS serves worst (0.3 TFLOP/s fp64 in rocBLAS at
 * 65536 x 128, 7.0 ms against 63 us here) - and this entry point:
 *     out_w[dim, dim] = scale * (y^T a)   (weights [in, out], the layout of mi_ode_rhs.w)      out_b[dim] = scale * column sums of a
 * over two [batch, dim] device planes, dim <= 128, fp32 or fp64 (MFMA); out_b nullable.  Deterministic (slab partials folded in
 * slab order).  workspace_dev: mi_ode_outer_workspace_bytes(dtype, batch, dim) bytes of device scratch.  Enqueues two kernels on
 * `stream` and returns: no synchronisation, capturable in a hipGraph. */
int64_t mi_ode_outer_workspace_bytes(int32_t dtype, int64_t batch, int32_t dim);
int mi_ode_outer_reduce(int32_t dtype, int64_t batch, int32_t dim, const void* y_dev, const void* a_dev, double scale,
                        void* out_w_dev, void* out_b_dev, void* workspace_dev, void* stream);

/* ---- (A''') the backward segment of odeint_adjoint for the linear right-hand side, ONE launch (ABI 13) ------------- */
/* tfdiffeq/adjoint.py:148-160: odeint(augmented_dynamics, (y, adj_y, adj_t, adj_params), [t_i, t_{i-1}]) for f(t, y) = y W + b,
 * dopri5 over the four components with the reference's per-component error ratios, python max() of them, the initial step over all
 * components (misc.py:183-287) and dense output at t_end (interp.py:6-67).  y and adj_y run on config 4's tile kernels (W and W^T
 * resident in registers); adj_params needs ONE product over the batch per INTERVAL - y0^T a0, carried from step to step through the
 * stage polynomials of the two linear systems (csrc/mi_ode_linadj.h, docs/KERNELS.md 4e).  State dtype
 * float32 or float64, 1 <= dim <= 128.  adj_params is one flat vector: W's gradient [dim, dim] in W's own [in, out] layout, then
 * (with a bias) the dim entries of b's. */
typedef struct mi_ode_linadj_desc {
  int64_t batch;
  int32_t dim;
  int32_t dtype;              /* enum mi_ode_dtype */
  mi_ode_tableau tableau;     /* dopri5: 6 rows, FSAL shaped, c_mid filled */
  double rtol, atol;          /* scalars: adjoint.py passes them through to every component (dopri5.py:60-61) */
  double safety, ifactor, dfactor;
  int32_t order, init_order;
  int64_t max_num_steps;
} mi_ode_linadj_desc;
typedef struct mi_ode_linadj* mi_ode_linadj_handle;
int mi_ode_linadj_create(const mi_ode_linadj_desc* desc, mi_ode_linadj_handle* out);
int mi_ode_linadj_destroy(mi_ode_linadj_handle h);
/* One backward interval t_start -> t_end (either direction; decreasing time as misc._check_inputs handles it, misc.py:311-321).
 * All pointers are DEVICE memory in the state dtype; w_dev [dim, dim] row-major ([in, out]: f = y W), b_dev nullable; adj_t is a
 * device scalar.  grad_out_dev (nullable): grad_output at t_start, [batch, dim] - the segment then starts from
 * adj_t - f(t_start, y) . grad_out (the time gradient of the measurement point, adjoint.py:134-140; f(t_start, y) is the kernel's own first
 * evaluation) and stores that dot product in dldt_out_dev (nullable device scalar).  host_scalars (nullable): {the dot product,
 * adj_t(t_end)} as doubles, for a caller that assembles the time gradients on the host.  y(t_end) is not produced (the reference
 * discards it, adjoint.py:155-160).  Blocks until done; returns status bits (>= 0) or an error (< 0).  stats->n_launches == 1. */
int mi_ode_linadj_segment(mi_ode_linadj_handle h, const void* w_dev, const void* b_dev, const void* y_dev, const void* adj_y_dev,
                          const void* adj_t_dev, const void* adj_params_dev, const void* grad_out_dev, double t_start, double t_end,
                          void* adj_y_out_dev, void* adj_t_out_dev, void* adj_params_out_dev, void* dldt_out_dev, double* host_scalars,
                          mi_ode_stats* stats, void* stream);
/* where the time of the last segment went, microseconds of workgroup 0: {tile passes, adj_params combinations, hand-offs of the
 * attempts, slab passes, folds + small products with their hand-offs, prologue, epilogue, hand-offs (count)} */
int mi_ode_linadj_profile(mi_ode_linadj_handle h, double* out8);

/* ---- (A'''') exact gradient of a fixed-grid solve: the reverse sweep of the discrete map, ONE launch --------------------- */
/* The reference trains by back-propagating through the solver's own ops (tfdiffeq/fixed_grid.py under the caller's tape); what that
 * returns is the gradient of the discrete map y_{n+1} = y_n + h sum_i b_i f(Y_i), not the continuous adjoint's.  This entry point is that
 * gradient for the ODEFunc MLP (MI_ODE_RHS_MLP_TANH, fp32, state [batch, dim]; time independent, or time dependent - the first layer
 * sees concat([t, x]), mi_ode_discrete_create_td) on the default grid (the output times
 * are the grid; a solve on the grid of options['step_size'] hands it the recomputed grid states and the output gradients placed on
 * that grid - section A''''''' does both inside the launch for the linear system): with lambda_{n+1} the gradient at y_{n+1}, for i = s .. 1
 *     kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j,   Ybar_i = (df/dy at Y_i)^T kbar_i,   theta_bar += (df/dtheta at Y_i)^T kbar_i,
 * lambda_n = lambda_{n+1} + sum_i Ybar_i + (the output gradient at grid point n).  The stages are recomputed from the stored y_n, the
 * time-dependent network's at the times the forward step functions form in the state dtype (t_n, t_n + h / 2, t_n + h, t_n + h / 3,
 * t_n + h 2 / 3): the actual, decreasing times on a decreasing grid. */
typedef struct mi_ode_discrete_desc {
  int64_t batch;
  int32_t dim, hidden;
  mi_ode_tableau tableau;     /* explicit, at most 3 rows (4 stages): beta = a_ij, c_sol = b (euler: no rows; midpoint, heun: one; rk4: three) */
  int32_t n_points;           /* grid points N (N - 1 steps), 2 <= N <= 1025 */
  int32_t chunk_tiles;        /* 32-row tiles of a workgroup that share one weight-gradient pass; 0: all of them */
} mi_ode_discrete_desc;
typedef struct mi_ode_discrete* mi_ode_discrete_handle;
int mi_ode_discrete_create(const mi_ode_discrete_desc* desc, mi_ode_discrete_handle* out);      /* the time-independent network */
/* time_dependent: 0 - as mi_ode_discrete_create; 1 - the handle is sized for the time-dependent network (rhs->scalars[1] != 0, W1 is
 * [1 + dim, hidden] with the row of t first): `hidden` more parameters.  The sizes are fixed at creation, hence the flag here.
 * Stage i is evaluated at t_n + (h p) / q with alpha_i = p / q, q the smallest of 1, 2, 3 that makes p an integer - the divisions the
 * forward step functions perform for euler, midpoint, heun and the 3/8 rule (h / 2, h / 3, (h 2) / 3), so the recomputed stage is the
 * stage the forward ran.  Any other alpha is taken as t_n + h alpha (rounded to the state dtype once): exact to rounding, not bitwise
 * the time of a forward that divides differently. */
int mi_ode_discrete_create_td(const mi_ode_discrete_desc* desc, int32_t time_dependent, mi_ode_discrete_handle* out);
int mi_ode_discrete_destroy(mi_ode_discrete_handle h);
int64_t mi_ode_discrete_num_params(mi_ode_discrete_handle h);
/* t_host: the N grid times (host): their differences in the state dtype are the step sizes, and the times themselves are what the
 * time-dependent network is evaluated at.  ys_dev: the forward solution [N, batch, dim]; grad_ys_dev: the gradient of the loss with
 * respect to it, same shape; grad_y0_out_dev [batch, dim]; grad_theta_out_dev: mi_ode_discrete_num_params() entries in the canonical
 * order of (A'): (w_t [hidden] when time dependent - row 0 of W1,) W1 [dim][hidden], b1, W2, b2, W3, b3, weights [in, out].  All device
 * memory, fp32.  rhs: the weights (sign is ignored); MI_ODE_E_INVALID when rhs->scalars[1] disagrees with the handle's flag.
 * Deterministic: two calls give identical bits.  Blocks until done; returns status bits (>= 0) or an error (< 0).
 * stats->n_launches == 1. */
int mi_ode_discrete_sweep(mi_ode_discrete_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                          const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats, void* stream);

/* ---- (A''''-64) the same reverse sweep for the ODEFunc MLP in fp64, ONE launch ---------------------------------------------------- */
/* The float64 twin of section A'''' (csrc/mi_ode_discrete64.h): same recursion, same schedule, same determinism, the operand plan of the
 * float64 forward kernels - weights streamed from packed copies, in both orientations, refreshed in front of every sweep.  The descriptor
 * is mi_ode_discrete_desc (same box: dim <= 64, hidden <= 128, at most 4 stages, 2 <= n_points <= 1025; chunk_tiles as there, a scratch
 * slot is 32 (2 DP + 4 HP) doubles); time_dependent as in mi_ode_discrete_create_td, the stage times are formed in double.
 * mi_ode_discrete64_sweep: every device buffer is fp64, grad_theta_out_dev in the canonical order of (A') - w_t first when time
 * dependent.  MI_ODE_E_INVALID when rhs->scalars[1] disagrees with the handle's flag or the activation code is unknown.  Deterministic:
 * two calls give identical bits.  Blocks until done; returns status bits (>= 0) or an error (< 0).  stats->n_launches == 1: it counts the
 * sweep kernel, as the float64 forward family counts its kernels - the two small pack launches enqueued in front of it are not counted. */
typedef struct mi_ode_discrete64* mi_ode_discrete64_handle;
int mi_ode_discrete64_create(const mi_ode_discrete_desc* desc, int32_t time_dependent, mi_ode_discrete64_handle* out);
int mi_ode_discrete64_destroy(mi_ode_discrete64_handle h);
int64_t mi_ode_discrete64_num_params(mi_ode_discrete64_handle h);
int mi_ode_discrete64_sweep(mi_ode_discrete64_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                            const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats, void* stream);
/* where the time of the last sweep went, microseconds of workgroup 0: {tile passes, weight-gradient passes, final hand-off + fold} */
int mi_ode_discrete64_profile(mi_ode_discrete64_handle h, double* out3);

/* ---- (A''''') the same reverse sweep for a row-local f with a generated vjp (tfdiffeq_amd/lower.py), ONE launch ------------------------ */
/* rhs: MI_ODE_RHS_PLUGIN with `plugin` = what a discrete plugin's mi_ode_discrete_plugin_get(dtype) returned (csrc/mi_ode_discrete_plugin.h);
 * scalars and w[0] as for the row-local plugin of the same callable.  A trajectory per lane; the parameter gradient is reduced in a fixed
 * order (lanes, wavefronts, workgroups - the last workgroup to arrive folds): two calls give identical bits, no workgroup waits for another.
 * fp32 or fp64.  The caller owns the small device buffers (nothing is allocated here). */
typedef struct mi_ode_discrete_row_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t n_points;           /* grid points N (N - 1 steps), N >= 2 */
  int64_t batch;
  int32_t dim;                /* <= 32, the plugin's */
  int32_t n_params;           /* P <= 1024: trainable elements, the plugin's */
  int32_t grid;               /* workgroups, 1 .. min(1024, ceil(batch / 256)) */
  int32_t reserved;
  mi_ode_tableau tableau;     /* explicit, 0, 1 or 3 rows (1, 2 or 4 stages): beta = a_ij, c_sol = b */
  const double* t_dev;        /* device: the N grid times, float64 (values already rounded to the state dtype) */
  void* partials_dev;         /* device workspace: grid * P elements of the state dtype */
  void* ticket_dev;           /* device: one zeroed 32-bit word (left zero again) */
} mi_ode_discrete_row_desc;
/* ys_dev: the forward solution [N, batch, dim]; grad_ys_dev: the gradient of the loss with respect to it; grad_y0_out_dev [batch, dim];
 * grad_theta_out_dev [P] in the compact order of the generated vjp.  Enqueues one launch on `stream`; returns 0 or a negative MI_ODE_E_*
 * (MI_ODE_E_INVALID for a null / inconsistent descriptor or another table in rhs->plugin, MI_ODE_E_NODEVICE without a device). */
int mi_ode_discrete_row_sweep(const mi_ode_discrete_row_desc* desc, const mi_ode_rhs* rhs, const void* ys_dev, const void* grad_ys_dev,
                              void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats, void* stream);

/* The same for a solve with times and a length of every row's own (mi_ode_integrate_fixed_rows_t; csrc/mi_ode_discrete_row_t.h): the exact
 * gradient of every row's own discrete map, all rows and all steps in ONE launch.  grad y0 of row i is what mi_ode_discrete_row_sweep
 * returns for row i alone with the times t[i][0 .. len_i - 1], bit for bit; grad theta is the sum over the rows in the fixed order of
 * mi_ode_discrete_row_sweep.  rhs: MI_ODE_RHS_PLUGIN with `plugin` = what a discrete-t plugin's mi_ode_discrete_t_plugin_get(dtype)
 * returned (csrc/mi_ode_discrete_t_plugin.h).  euler and rk4 (tableaus of 0 and 3 rows). */
typedef struct mi_ode_discrete_row_t_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t n_times;            /* T >= 1: the second axis of the times, the longest row */
  int64_t batch;
  int32_t dim;                /* <= 32, the plugin's */
  int32_t n_params;           /* P <= 1024: trainable elements, the plugin's */
  int32_t grid;               /* workgroups, 1 .. min(1024, ceil(batch / 256)) */
  int32_t reserved;
  mi_ode_tableau tableau;     /* explicit, 0 or 3 rows (1 or 4 stages): beta = a_ij, c_sol = b */
  const double* t_dev;        /* device [batch][T] float64 (values already rounded to the state dtype); row i is read up to len_i - 1 only */
  const int32_t* len_dev;     /* device [batch] with values in 1 .. T (clamped to that range by the kernel), or NULL: every row has T times */
  void* partials_dev;         /* device workspace: grid * P elements of the state dtype */
  void* ticket_dev;           /* device: one zeroed 32-bit word (left zero again) */
} mi_ode_discrete_row_t_desc;
/* ys_dev / grad_ys_dev [T, batch, dim]: grad_ys_dev[k][i] for k >= len_i is never read; grad_y0_out_dev [batch, dim]; grad_theta_out_dev
 * [P].  Enqueues one launch on `stream`; returns 0 or a negative MI_ODE_E_* as mi_ode_discrete_row_sweep does. */
int mi_ode_discrete_row_sweep_t(const mi_ode_discrete_row_t_desc* desc, const mi_ode_rhs* rhs, const void* ys_dev, const void* grad_ys_dev,
                                void* grad_y0_out_dev, void* grad_theta_out_dev, mi_ode_stats* stats, void* stream);
int64_t mi_ode_discrete_row_t_sizeof(void);               /* sizeof(mi_ode_discrete_row_t_desc), for a binding's layout check */

/* ---- (A-rows-adjoint) gradients of a per-trajectory solve (mi_ode_integrate_rows) for a row-local f with a generated vjp, ONE launch ---- */
/* The reference's adjoint algorithm (adjoint.py:117-178) applied to every row of the batch ALONE (csrc/mi_ode_rows_adjoint.h): for
 * k = T-1 .. 1 the row's dLd_cur_t = f(t_k, y_k) . g_k, then the adaptive integration of ITS tuple state (y [1, dim], adj_y [1, dim],
 * adj_t [], adj_params [P]) from t_k to t_{k-1} with the reference's per-component control (one error ratio and one scalar tolerance per
 * component, accepted if all ratios are <= 1), then adj_y += g_{k-1}.  A trajectory per lane; rows never interact inside the loops.
 * rhs: MI_ODE_RHS_PLUGIN with `plugin` = what a rows-adjoint plugin's mi_ode_rows_adjoint_plugin_get(dtype) returned
 * (csrc/mi_ode_rows_adjoint_plugin.h); scalars and w[0] as for the row-local plugin of the same callable.  fp32 or fp64,
 * 2 dim + 1 + max(n_params, 1) <= 32, the FSAL shaped 6-row (dopri5) and 3-row (bosh3) tableaus.  The caller owns every buffer. */
typedef struct mi_ode_adjoint_rows_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t n_times;            /* T >= 1 output times */
  int64_t batch;
  int32_t dim;                /* the plugin's */
  int32_t n_params;           /* P: trainable elements, the plugin's */
  int32_t order, init_order;  /* dopri5: 5, 4; bosh3: 3, 2 */
  double rtol, atol;          /* adjoint_rtol / adjoint_atol: one scalar pair for the four components */
  double safety, ifactor, dfactor;
  int64_t max_num_steps;      /* <= 0: 2^31 - 1 */
  mi_ode_tableau tableau;
  const double* neg_t_dev;    /* device: the T output times, NEGATED (the backward solves run in the solver's time s = -t, misc.py:318-321) */
  void* row_params_dev;       /* out [batch, max(P, 1)]: every row's own adj_params */
  void* row_time_vjps_dev;    /* out [batch, T]: every row's own time vjps */
  int64_t* row_counts_dev;    /* out [batch, 3, T - 1]: attempts, accepted steps, function evaluations of the interval t_k -> t_{k-1} at k - 1 */
  int64_t* row_status_dev;    /* out [batch]: MI_ODE_ST_* bits of the row (an interval that ends with one ends the row) */
  void* partials_dev;         /* workspace: ceil(batch / 256) * (max(P, 1) + T) elements of the state dtype */
  void* ticket_dev;           /* one zeroed 32-bit word (left zero again) */
} mi_ode_adjoint_rows_desc;
/* ans_dev: the forward solution [T, batch, dim]; grad_ans_dev: the gradient of the loss with respect to it; grad_y0_out_dev [batch, dim];
 * grad_params_out_dev [max(P, 1)] and grad_t_out_dev [T]: the rows summed in a fixed order (rows of a workgroup in row order, workgroups in
 * order, by the last workgroup to arrive) - two calls give identical bits.  Enqueues one launch on `stream` and returns 0 without waiting,
 * or a negative MI_ODE_E_* (MI_ODE_E_INVALID for a null / inconsistent argument or another table in rhs->plugin, MI_ODE_E_NODEVICE
 * without a device); a failing row is reported in row_status_dev, not here. */
int mi_ode_adjoint_rows(const mi_ode_adjoint_rows_desc* desc, const mi_ode_rhs* rhs, const void* ans_dev, const void* grad_ans_dev,
                        void* grad_y0_out_dev, void* grad_params_out_dev, void* grad_t_out_dev, mi_ode_stats* stats, void* stream);
int64_t mi_ode_adjoint_rows_sizeof(void);                 /* sizeof(mi_ode_adjoint_rows_desc), for a binding's layout check */

/* The same for a solve with output times, lengths and tolerances of every row's own (mi_ode_integrate_rows_t;
 * csrc/mi_ode_rows_adjoint_t.h).  Row i is what mi_ode_adjoint_rows returns for row i alone with the times t[i][0 .. len_i - 1] at
 * rtol_dev[i] / atol_dev[i], bit for bit.  rhs: MI_ODE_RHS_PLUGIN with `plugin` = what a rows-adjoint-t plugin's
 * mi_ode_rows_adjoint_t_plugin_get(dtype) returned (csrc/mi_ode_rows_adjoint_t_plugin.h).  Limits as there. */
typedef struct mi_ode_adjoint_rows_t_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t n_times;            /* T >= 1: the second axis of the times, the longest row */
  int64_t batch;
  int32_t dim;                /* the plugin's */
  int32_t n_params;           /* P: trainable elements, the plugin's */
  int32_t order, init_order;  /* dopri5: 5, 4; bosh3: 3, 2 */
  double rtol, atol;          /* adjoint_rtol / adjoint_atol of every row without a value of its own (rtol_dev / atol_dev NULL) */
  double safety, ifactor, dfactor;
  int64_t max_num_steps;      /* <= 0: 2^31 - 1 */
  mi_ode_tableau tableau;
  const double* neg_t_dev;    /* device [batch][T]: every row's output times, NEGATED; row i is read up to len_i - 1 only */
  const int32_t* len_dev;     /* device [batch] with values in 1 .. T (clamped to that range by the kernel), or NULL: every row has T times */
  const double* rtol_dev;     /* device [batch] float64, or NULL */
  const double* atol_dev;     /* device [batch] float64, or NULL */
  void* row_params_dev;       /* out [batch, max(P, 1)]: every row's own adj_params */
  void* row_time_vjps_dev;    /* out [batch, T]: every row's own time vjps, exact zeros from len_i on - the gradient of `t`, not summed */
  int64_t* row_counts_dev;    /* out [batch, 3, T - 1]: as mi_ode_adjoint_rows_desc; zeros for the intervals beyond len_i - 1 */
  int64_t* row_status_dev;    /* out [batch]: MI_ODE_ST_* bits of the row */
  void* partials_dev;         /* workspace: ceil(batch / 256) * max(P, 1) elements of the state dtype */
  void* ticket_dev;           /* one zeroed 32-bit word (left zero again) */
} mi_ode_adjoint_rows_t_desc;
/* ans_dev / grad_ans_dev [T, batch, dim]: grad_ans_dev[k][i] for k >= len_i is never read; grad_y0_out_dev [batch, dim];
 * grad_params_out_dev [max(P, 1)]: the rows summed in the fixed order of mi_ode_adjoint_rows - two calls give identical bits.  Enqueues
 * one launch on `stream` and returns 0 without waiting, or a negative MI_ODE_E_* as mi_ode_adjoint_rows does; a failing row is reported
 * in row_status_dev. */
int mi_ode_adjoint_rows_t(const mi_ode_adjoint_rows_t_desc* desc, const mi_ode_rhs* rhs, const void* ans_dev, const void* grad_ans_dev,
                          void* grad_y0_out_dev, void* grad_params_out_dev, mi_ode_stats* stats, void* stream);
int64_t mi_ode_adjoint_rows_t_sizeof(void);               /* sizeof(mi_ode_adjoint_rows_t_desc), for a binding's layout check */

/* ---- (A'''''') the same reverse sweep for the linear system f(y) = y W (+ b) on the matrix cores, ONE launch ------------------------ */
/* The transpose of the fixed-grid map of MI_ODE_RHS_LINEAR (csrc/mi_ode_discrete_linear.h): Ybar_i = kbar_i W^T, Wbar += Y_i^T kbar_i,
 * bbar += sum_rows kbar_i.  fp32 or fp64, dim <= 128 (smaller dims run zero padded on the 16 / 32 / 64 / 128 wide instantiations), at most
 * 4 stages and 1024 steps, on the default grid (every grid point an output; a grid of its own: the next section).  A persistent grid of
 * at most one workgroup per CU; the parameter gradient is reduced in a fixed order. */
typedef struct mi_ode_discrete_linear_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t dim;                /* 1 .. 128 */
  int64_t batch;
  int32_t has_bias;           /* 0 / 1: must agree with rhs->b[0] of every sweep */
  int32_t n_points;           /* grid points N (N - 1 steps), 2 <= N <= 1025 */
  mi_ode_tableau tableau;     /* explicit, at most 3 rows (4 stages): beta = a_ij, c_sol = b */
} mi_ode_discrete_linear_desc;
typedef struct mi_ode_discrete_linear* mi_ode_discrete_linear_handle;
/* MI_ODE_E_INVALID for dim < 1 or > 128, n_points < 2 or > 1025, more than 4 stages, a dtype other than fp32 / fp64. */
int mi_ode_discrete_linear_create(const mi_ode_discrete_linear_desc* desc, mi_ode_discrete_linear_handle* out);
int mi_ode_discrete_linear_destroy(mi_ode_discrete_linear_handle h);
/* t_host: the N grid times (host).  ys_dev / grad_ys_dev [N, batch, dim]; grad_y0_out_dev [batch, dim]; grad_W_out_dev [dim, dim] in the
 * [in, out] layout of W; grad_b_out_dev [dim] or NULL.  All device memory in the state dtype.  rhs: the MI_ODE_RHS_LINEAR descriptor
 * (w[0] = W, b[0] = bias or NULL; sign is ignored); the weights are read at every call.  Deterministic: two calls give identical bits.
 * Blocks until done; returns status bits (>= 0; MI_ODE_ST_SYNC_TIMEOUT when a grid hand-off timed out: nothing was committed) or an error
 * (< 0).  stats->n_launches == 1. */
int mi_ode_discrete_linear_sweep(mi_ode_discrete_linear_handle h, const mi_ode_rhs* rhs, const double* t_host, const void* ys_dev,
                                 const void* grad_ys_dev, void* grad_y0_out_dev, void* grad_W_out_dev, void* grad_b_out_dev,
                                 mi_ode_stats* stats, void* stream);
/* Workgroup 0's clock of the last sweep, microseconds: out3 = {tile sweep (all steps, weight-gradient products included), partial-block
 * store, final hand-off + fold}.  Returns the grid size, or MI_ODE_E_INVALID. */
int mi_ode_discrete_linear_profile(mi_ode_discrete_linear_handle h, double* out3);

/* ---- (A''''''') the linear reverse sweep for a solve on a grid of its own (options['step_size']), ONE launch, no stored trajectory --- */
/* The solver walked a grid of n_steps steps and interpolated the n_out requested times linearly inside the step that reaches them
 * (solvers.py:86-115).  The kernel recomputes the checkpoints of each 16-row tile forward from y0 into a scratch block of its workgroup
 * (grid x n_steps x 16 x D elements of the state dtype, D the instantiation's width: it does not depend on the batch; at most 1 GiB) and
 * then runs the reverse sweep of section A'''''' over them, placing the output gradients on the grid as it goes:
 * gbar_{n_j + 1} += w_j g_j, gbar_{n_j} += (1 - w_j) g_j (the latter only when w_j != 1), output 0 is y0. */
typedef struct mi_ode_discrete_linear_grid_desc {
  int32_t dtype;              /* MI_ODE_F32 / MI_ODE_F64 */
  int32_t dim;                /* 1 .. 128 */
  int64_t batch;
  mi_ode_tableau tableau;     /* explicit, at most 3 rows (4 stages): beta = a_ij, c_sol = b */
  int32_t n_steps;            /* grid steps M, 1 .. 1024 */
  int32_t n_out;              /* requested times, 2 .. 1025 (the first one is the start of the grid) */
  int32_t has_bias;           /* 0 / 1: must agree with rhs->b[0] of every sweep */
  int32_t reserved;
} mi_ode_discrete_linear_grid_desc;
typedef struct mi_ode_discrete_linear_grid* mi_ode_discrete_linear_grid_handle;
/* What can be checked without a device, MI_ODE_E_INVALID or 0: the descriptor (dim < 1 or > 128, n_steps < 1 or > 1024, n_out < 2 or > 1025,
 * more than 4 stages, a dtype other than fp32 / fp64) and, where the pointers are not NULL, a grid that does not increase, out_step[0] != -1,
 * an out_step[j >= 1] outside [0, n_steps) or decreasing, a weight outside [0, 1].  create and sweep run it first. */
int mi_ode_discrete_linear_grid_validate(const mi_ode_discrete_linear_grid_desc* desc, const double* grid_host, const int32_t* out_step,
                                         const double* out_w);
/* MI_ODE_E_INVALID also when the checkpoint scratch would exceed 1 GiB (mi_ode_last_error says so). */
int mi_ode_discrete_linear_grid_create(const mi_ode_discrete_linear_grid_desc* desc, mi_ode_discrete_linear_grid_handle* out);
int mi_ode_discrete_linear_grid_destroy(mi_ode_discrete_linear_grid_handle h);
/* grid_host [n_steps + 1]: the solver's grid; out_step [n_out]: the grid step each output was interpolated in (out_step[0] = -1,
 * non-decreasing); out_w [n_out]: its weight (t_j - t0) / (t1 - t0) in the state dtype, 1 for an exact hit of t1 - all host memory.
 * y0_dev [batch, dim]; grad_out_dev [n_out, batch, dim]; grad_y0_out_dev [batch, dim]; grad_W_out_dev [dim, dim] in the [in, out] layout
 * of W; grad_b_out_dev [dim] or NULL.  Step sizes are formed in the state dtype.  Deterministic: the outputs of a step are summed in the
 * order of j, the parameter gradient in workgroup order.  Blocks until done; returns status bits (>= 0; MI_ODE_ST_SYNC_TIMEOUT: nothing was
 * committed) or an error (< 0).  stats->n_launches == 1; stats->nfe counts the recomputation and the transposed evaluations. */
int mi_ode_discrete_linear_grid_sweep(mi_ode_discrete_linear_grid_handle h, const mi_ode_rhs* rhs, const double* grid_host,
                                      const int32_t* out_step, const double* out_w, const void* y0_dev, const void* grad_out_dev,
                                      void* grad_y0_out_dev, void* grad_W_out_dev, void* grad_b_out_dev, mi_ode_stats* stats, void* stream);
/* out3 (may be NULL): as mi_ode_discrete_linear_profile; *scratch_bytes (may be NULL): the checkpoint scratch the handle owns.  Returns
 * the grid size, or MI_ODE_E_INVALID. */
int64_t mi_ode_discrete_linear_grid_profile(mi_ode_discrete_linear_grid_handle h, double* out3, int64_t* scratch_bytes);

/* ---- function-level parity surface of the step controller ----------------------------------- */
/* The scalar tail of one step attempt exactly as the kernels run it (csrc/mi_ode_ctrl_dev.h, ONE device thread per case):
 *   phase 2 (attempt): misc._compute_error_ratio's scalar part + accept test + misc._optimal_step_size / tsit5._optimal_step_size
 *                      (misc.py:256-287, tsit5.py:53-62, dopri5.py:103-121)
 *   phase 0 / 1      : the two halves of misc._select_initial_step (misc.py:227-245)
 * on caller-supplied numbers, so that the DEVICE arithmetic can be driven with the reference's own vectors.
 * in[c]  (8 doubles per case): {max|y0|, max|y1|, sum_a, sum_b, nonfinite flag, N (elements behind the sums), -, -}
 * st[c]  (4 doubles per case): {t1, dt, h0, d1}   (rk_state.t1 / rk_state.dt; h0, d1: what phase 0 produced, for phase 1)
 * out[c] (8 doubles per case): {ratio, accepted, dt_next, t1_next, t0_next, status bits, h0, d0 (phase 0) | d1 in out[c][6..7]}
 *          phase 0 writes {-, -, -, -, -, -, h0, d0} and d1 into out[c][2]; phase 1 writes the first step size into out[c][2].
 * All pointers are HOST memory; the call is synchronous. */
typedef struct mi_ode_ctrl_params {
  double rtol, atol, safety, ifactor, dfactor;   /* safety / ifactor / dfactor: the float32-rounded values (misc.py:137-144) */
  int32_t order, init_order;                     /* dopri5.py:68,74 */
  int32_t controller;                            /* enum mi_ode_controller */
  int32_t dtype;                                 /* enum mi_ode_dtype of the STATE: float32 states take the float32 detours */
} mi_ode_ctrl_params;
int mi_ode_controller_update(const mi_ode_ctrl_params* p, int32_t phase, int32_t n_cases, const double* in_host,
                             const double* st_host, double* out_host, void* stream);
/* y_sigma = y0 + add_n((dt * beta_j) * k_j)  - one stage combination of rk_common._runge_kutta_step (rk_common.py:51);
 * the same kernel as mi_ode_lincomb, under the name SURVEY.md 8(b) gives it */
int mi_ode_rk_stage_combine(int32_t dtype, int64_t n, const void* y0_dev, const void* const* k_dev, const double* beta_row,
                            int32_t n_k, double dt, void* out_dev, void* stream);
/* {max|y0|, max|y1|, sum err^2, nonfinite} of one attempt (misc.py:256-263): mi_ode_error_norms under its 8(b) name */
int mi_ode_rk_error_reduce(int32_t dtype, int64_t n, const void* err_dev, const void* y0_dev, const void* y1_dev,
                           double* result_dev, void* workspace_dev, void* stream);

/* ---- (C) opaque right-hand side, device-resident controller ------------------------------------------------ */
/* The reference's own call shape - odeint(func, y0, t) with a Python callable (tests/odeint_tests.py:30-77,
 * examples/ode_demo.py:39,169) - costs one host decision per attempt when the controller runs on the host
 * (dopri5.py:103-121 reads the error ratio back).  Here the scalar state of the solver (rk_state.t0 / t1 / dt, the output
 * cursor, the counters, the reference's assertions as status bits) lives in a device record; the caller evaluates f between
 * our launches, the stage combinations are mi_ode_lincomb_dev with scale_dev = mi_ode_opq_dt_dev(h), and f receives its time
 * argument as a 0-d view of the stage-time array - so one attempt
 *     for sigma = 1..S:  y_sigma = lincomb_dev(y0, k_1..k_sigma, beta_sigma);  k_{sigma+1} = f(ts[sigma-1], y_sigma)
 *     [not FSAL shaped: y1 = lincomb_dev(y0, k, c_sol)]                          (rk_common.py:49-56)
 *     mi_ode_opq_finish(y0, y1, k);  mi_ode_opq_commit(y0, f0, y1, k)
 * contains no host value and can be captured as a hipGraph and replayed.  A tuple state has n_comp components (all pointer
 * arrays are [n_comp], k is [n_comp][S + 1] flattened, k[c][0] = f0 of component c); ratios are per component, accepted if all
 * are <= 1, python max() of them drives the step size (misc.py:250-287); the tsit5 controller pools them (tsit5.py:126-138).
 * Every kernel is a no-op once the record says `done` (all outputs produced, or a status bit), and mi_ode_opq_commit is a
 * no-op after a rejected attempt: a host that replays attempts blindly in chunks and polls once per chunk is correct. */
typedef struct mi_ode_opq_desc {
  int32_t dtype;              /* enum mi_ode_dtype of every component */
  int32_t n_comp;             /* 1 .. MI_ODE_MAX_SEGMENTS */
  int64_t n[MI_ODE_MAX_SEGMENTS];                 /* elements per component */
  mi_ode_tableau tableau;     /* 1, 3, 6 or 13 rows (dense output is instantiated for S + 1 = 2, 4, 7, 14 stage derivatives) */
  int32_t controller, interp, order, init_order;  /* as mi_ode_desc */
  double rtol[MI_ODE_MAX_SEGMENTS], atol[MI_ODE_MAX_SEGMENTS];   /* one pair per component (dopri5.py:60-61); tsit5: pair 0 */
  double safety, ifactor, dfactor;                /* the float32-rounded values (misc.py:137-144) */
  int64_t max_num_steps;
} mi_ode_opq_desc;
typedef struct mi_ode_opq* mi_ode_opq_handle;
int mi_ode_opq_create(const mi_ode_opq_desc* desc, mi_ode_opq_handle* out);
int mi_ode_opq_destroy(mi_ode_opq_handle h);
/* device address of rk_state.dt (float64): the scale_dev of the attempt's mi_ode_lincomb_dev calls */
const double* mi_ode_opq_dt_dev(mi_ode_opq_handle h);
/* Arms an integration: rk_state = (t0, t0, first_dt) (dopri5.py:79), the output cursor over t_out_host[0 .. n_out-1]
 * (strictly increasing, all > t0; solvers.py:31-35), out_dev[c] = the [n_out, n[c]] solution rows of component c, and the
 * first attempt's stage times into stage_times_dev ([S] elements of the state dtype; rewritten after every attempt).
 * A recorded attempt (finish + commit captured in a hipGraph) stays valid across opq_begin calls: the kernels read the solution
 * rows' addresses and the output times from tables inside the handle when they run - as long as n_out never exceeds what the
 * handle has held before (1024 at creation; a larger n_out moves the output-time table, and the attempt must be recorded again). */
int mi_ode_opq_begin(mi_ode_opq_handle h, double t0, double first_dt, const double* t_out_host, int32_t n_out,
                     void* const* out_dev, void* stage_times_dev, void* stream);
int mi_ode_opq_finish(mi_ode_opq_handle h, const void* const* y0_dev, const void* const* y1_dev, const void* const* k_dev,
                      void* stream);
int mi_ode_opq_commit(mi_ode_opq_handle h, void* const* y0_dev, void* const* f0_dev, const void* const* y1_dev,
                      const void* const* k_dev, void* stream);
/* Reads the scalar state back (one stream synchronisation): *done, the counters, status bits (also the return value). */
int mi_ode_opq_poll(mi_ode_opq_handle h, mi_ode_stats* stats, int32_t* done, void* stream);

/* ---- (B) stateless plane kernels (arbitrary Python f, tuple states) ------------------------- */
/* out[i] = (base ? base[i] : 0) + sum_j (scale * coef[j]) * xs[j][i]       (misc.py:118-121; zeros not skipped) */
int mi_ode_lincomb(int32_t dtype, int64_t n, const void* base_dev, const void* const* xs_dev, const double* coef,
                   int32_t nx, double scale, void* out_dev, void* stream);
/* same with the scale (dt) read from device memory at execution time: what a captured hipGraph of an RK attempt needs
 * (the graph is replayed with a new dt without re-recording) */
int mi_ode_lincomb_dev(int32_t dtype, int64_t n, const void* base_dev, const void* const* xs_dev, const double* coef,
                       int32_t nx, const double* scale_dev, void* out_dev, void* stream);
/* result_dev[4] (double) = {max|y0|, max|y1|, sum err^2, nonfinite(y0)}            (misc.py:256-263) */
int mi_ode_error_norms(int32_t dtype, int64_t n, const void* err_dev, const void* y0_dev, const void* y1_dev,
                       double* result_dev, void* workspace_dev, void* stream);
/* result_dev[1] (double) = sum_i ((x[i] - (xsub ? xsub[i] : 0)) / (atol + |y0[i]| * rtol))^2   (misc.py:225-237) */
int mi_ode_scaled_sumsq(int32_t dtype, int64_t n, const void* x_dev, const void* xsub_dev, const void* y0_dev,
                        double rtol, double atol, double* result_dev, void* workspace_dev, void* stream);
/* The variable-order Adams solver's host loop (tfdiffeq/adams.py:134-210, any callable f) on four plane kernels instead of one linear
 * combination at a time.  phi: the implicit-phi planes, newest first (`order` of them); g: the values of the float32 g vector,
 * g[0..order]; beta[0..order-1] (beta[0] unused); all planes hold n elements of `dtype`.
 *   predict     p = y + dt * sum_{j < max(1, order-1)} g_j explicit_phi_j,  explicit_phi_0 = phi_0, explicit_phi_j = beta_j phi_j
 *   correct     ip_0 = f_p, ip_j = ip_{j-1} - explicit_phi_{j-1};  y_next = p + dt g_{order-1} ip_{order-1};  also returns the planes
 *               ip_order, ip_{order-1}, ip_{order-2} (nullable) and result[4] = {max|y|, max|y_next|, sum local_error^2, nonfinite(y)}
 *   error_sums  result[2] = sums of ((dt * coef) x / tol)^2 for one or two planes (xb nullable): the error ratios times n
 *   update_phi  new_0 = f_new, new_j = new_{j-1} - explicit_phi_{j-1}, j <= order  (order + 1 output planes) */
int mi_ode_adams_predict(int32_t dtype, int64_t n, const void* y_dev, const void* const* phi_dev, int32_t order, const double* g,
                         const double* beta, double dt, void* p_out_dev, void* stream);
int mi_ode_adams_correct(int32_t dtype, int64_t n, const void* y_dev, const void* p_dev, const void* f_p_dev, const void* const* phi_dev,
                         int32_t order, const double* g, const double* beta, double dt, void* y_next_out_dev, void* ip_k_out_dev,
                         void* ip_k1_out_dev, void* ip_k2_out_dev, double* result_dev, void* workspace_dev, void* stream);
int mi_ode_adams_error_sums(int32_t dtype, int64_t n, const void* xa_dev, double coef_a, const void* xb_dev, double coef_b, double dt,
                            double tol, double* result_dev, void* workspace_dev, void* stream);
int mi_ode_adams_update_phi(int32_t dtype, int64_t n, const void* f_new_dev, const void* const* phi_dev, int32_t order,
                            const double* beta, void* const* new_phi_out_dev, void* stream);
/* result_dev[1] (double) = 1.0 if ANY element violates |a - b| < atol + rtol * max(|a|, |b|), else 0.0
 * (misc._has_converged, misc.py:129-134: the corrector iteration test of fixed_adams.py:196) */
int mi_ode_not_converged(int32_t dtype, int64_t n, const void* a_dev, const void* b_dev, double rtol, double atol,
                         double* result_dev, void* workspace_dev, void* stream);
/* dense output at one time t in [t0, t1] from the accepted step's (y0, y1, k[0..nk-1]):
 * interp = QUARTIC_MID: interp.py:6-67 with y_mid = y0 + dt*sum c_mid[j] k[j] (dt = the step size the step was
 * taken with, dopri5.py:41); TSIT5 / TSIT5_REF: tsit5.py:33-50 */
int mi_ode_interp_eval(int32_t dtype, int32_t interp, int64_t n, const void* y0_dev, const void* y1_dev,
                       const void* const* ks_dev, int32_t nk, const double* c_mid, double dt, double t0, double t1,
                       double t, void* out_dev, void* stream);

/* ---- (D) hypersolvers (tfdiffeq/hyper_solvers/: HyperEuler, HyperMidpoint, HyperHeun) ------------------------------------
 * A fixed step of the base method plus dt^(p+1) * g(cat([y, f(t, y), dt])), g a dense network given as a layer table; euler.py's
 * formulas literally (dt = t[1] - t[0] for every step, row i of a trajectory = the state before step i).  One call = the whole
 * trajectory / residual computation: csrc/mi_ode_hyper.h.  f: a row-local catalogue system (LORENZ, LOTKA_VOLTERRA, the dim-2
 * LINEAR / CUBIC_LINEAR with W by value in scalars[0..3]) or MI_ODE_RHS_PLUGIN with `plugin` = what a hyper plugin's
 * mi_ode_hyper_plugin_get(dtype) returned (csrc/mi_ode_hyper_plugin.h). */
#define MI_ODE_HYPER_MAX_LAYERS 6
#define MI_ODE_HYPER_WORKSPACE_BYTES (1 << 20)    /* device workspace a call may use for g's packed weights */
enum mi_ode_hyper_method { MI_ODE_HYPER_EULER = 0, MI_ODE_HYPER_MIDPOINT = 1, MI_ODE_HYPER_HEUN = 2 };
enum mi_ode_hyper_mode {
  MI_ODE_HYPER_TRAJECTORY = 0,   /* trajectory(t_span, y): out [T, batch, dim] from y [batch, dim]                          */
  MI_ODE_HYPER_RESIDUAL = 1,     /* residual_trajectory(t_span, base) of HyperEuler: out [T - 1, batch, dim] from y [T, batch, dim] */
  MI_ODE_HYPER_G_RESIDUALS = 2   /* _hypersolver_residuals(t_span, base): out [T, batch, dim] from y [T, batch, dim]           */
};
enum mi_ode_hyper_act {
  MI_ODE_HYPER_ACT_NONE = 0, MI_ODE_HYPER_ACT_RELU = 1, MI_ODE_HYPER_ACT_LEAKY_RELU = 2, MI_ODE_HYPER_ACT_PRELU = 3,
  MI_ODE_HYPER_ACT_TANH = 4, MI_ODE_HYPER_ACT_SOFTPLUS = 5     /* softplus: beta 1, threshold 20 */
};
typedef struct mi_ode_hyper_layer {
  int32_t in, out;            /* nn.Linear(in, out); widths <= 128 */
  int32_t act;                /* enum mi_ode_hyper_act: the activation that follows the layer */
  int32_t n_alpha;            /* PReLU: 1 (shared) or out (per channel) */
  double slope;               /* LeakyReLU negative slope */
  const void* w;              /* device, state dtype: [out, in] row-major (nn.Linear.weight) */
  const void* b;              /* device, nullable: [out] */
  const void* alpha;          /* device, PReLU only: [n_alpha] */
} mi_ode_hyper_layer;
typedef struct mi_ode_hyper {
  int32_t dtype;              /* enum mi_ode_dtype */
  int32_t method;             /* enum mi_ode_hyper_method */
  int32_t mode;               /* enum mi_ode_hyper_mode */
  int32_t n_layers;           /* 2 .. MI_ODE_HYPER_MAX_LAYERS; layers[0].in = 2 dim + 1, layers[n - 1].out = dim */
  int64_t batch, dim;
  int32_t T;                  /* time points, >= 2 */
  int32_t reserved;
  const void* t;              /* device [T], state dtype */
  const void* y;              /* device: y0 [batch, dim] (TRAJECTORY) or the base trajectory [T, batch, dim] */
  void* out;                  /* device, see enum mi_ode_hyper_mode */
  void* workspace;            /* device, MI_ODE_HYPER_WORKSPACE_BYTES: g's packed weights when they do not fit in LDS */
  mi_ode_rhs rhs;             /* f */
  mi_ode_hyper_layer layers[MI_ODE_HYPER_MAX_LAYERS];
} mi_ode_hyper;
/* Enqueues the call on `stream`.  Returns the number of kernel launches it enqueued (1, or 2 when g's weights are packed to the
 * workspace first), or a negative MI_ODE_E_*. */
int mi_ode_hyper_run(const mi_ode_hyper* desc, void* stream);

/* ---- (D') the gradient of a hypersolver call, one launch (csrc/mi_ode_hyper_grad.h) ------------------------------------------
 * TRAJECTORY: from the forward's output ys [T, batch, dim] and the gradient grad_out [T, batch, dim] of the loss with respect to it,
 * the reverse sweep over all steps and rows: grad_y [batch, dim] (nullable) and the gradient of every parameter of g whose
 * grad_w / grad_b / grad_alpha pointer is not null (torch's layouts: [out, in], [out], [n_alpha]).  G_RESIDUALS: ys is the base
 * trajectory, parameter gradients only.  f: MI_ODE_RHS_PLUGIN with `plugin` = what a hyper-grad plugin's
 * mi_ode_hyper_grad_plugin_get(dtype) returned (csrc/mi_ode_hyper_grad_plugin.h: f with a generated vjp), sign +1.
 * workspace: mi_ode_hyper_grad_workspace_bytes(desc) bytes, contents arbitrary (the per-workgroup parameter partials [grid, P] and,
 * when g's two weight images do not fit in LDS beside the activation tiles, the images); ticket: a 4-byte word that is zero. */
#define MI_ODE_HYPER_GRAD_MAX_GRID 256
typedef struct mi_ode_hyper_grad {
  int32_t dtype;              /* enum mi_ode_dtype */
  int32_t method;             /* enum mi_ode_hyper_method */
  int32_t mode;               /* MI_ODE_HYPER_TRAJECTORY or MI_ODE_HYPER_G_RESIDUALS */
  int32_t n_layers;
  int64_t batch, dim;
  int32_t T;                  /* time points, >= 2 */
  int32_t grid;               /* workgroups: 1 .. min(tiles of 16 rows, MI_ODE_HYPER_GRAD_MAX_GRID) */
  const void* t;              /* device [T], state dtype */
  const void* ys;             /* device [T, batch, dim] */
  const void* grad_out;       /* device [T, batch, dim] */
  void* grad_y;               /* device [batch, dim], nullable */
  void* workspace;
  void* ticket;
  mi_ode_rhs rhs;             /* f */
  mi_ode_hyper_layer layers[MI_ODE_HYPER_MAX_LAYERS];
  void* grad_w[MI_ODE_HYPER_MAX_LAYERS];
  void* grad_b[MI_ODE_HYPER_MAX_LAYERS];
  void* grad_alpha[MI_ODE_HYPER_MAX_LAYERS];
} mi_ode_hyper_grad;
/* Enqueues the call on `stream`.  Returns the number of kernel launches it enqueued (1, or 2 when the weight images are packed to
 * the workspace first), or a negative MI_ODE_E_*. */
int mi_ode_hyper_grad_run(const mi_ode_hyper_grad* desc, void* stream);
/* Bytes of `workspace` for this descriptor (dtype, grid, n_layers and the layers' widths are read), or a negative MI_ODE_E_*. */
int64_t mi_ode_hyper_grad_workspace_bytes(const mi_ode_hyper_grad* desc);
/* Bytes of LDS the gradient kernel needs for g's activation tiles alone (the size limit of the fused gradient), or negative. */
int64_t mi_ode_hyper_grad_tile_bytes(const mi_ode_hyper_grad* desc);
int mi_ode_hyper_grad_sizeof(void);

/* ---- (E) convolutional ODE function (tfdiffeq/models/conv_odenet.py: Conv2dODEFunc) -----------------------------------------
 * f(t, y) = conv3(act(conv2(act(conv1(y))))) on NCHW images: conv1 1x1 C -> F, conv2 3x3 zero-padded "same" F -> F, conv3 1x1
 * F -> C, all with biases; time dependent: every conv sees concat([t, x]) along the channels (time is input channel 0, zero padded
 * in conv2 like every other channel).  One call = one Runge-Kutta stage: y_s = y0 + sum_j (dt * beta_row[j]) * ks[j] (the operation
 * order of mi_ode_lincomb_dev; n_k = 0: y_s = y0) and k_out = sign * f(sign * t, y_s), as ONE kernel launch (csrc/mi_ode_conv.h).
 * Box: 1 <= channels <= MI_ODE_CONV_MAX_C, 1 <= filters <= MI_ODE_CONV_MAX_F, any height / width / batch.  Weights, device, in
 * the state dtype (Fp = filters rounded up to 16; td = 1 when time dependent, else 0):
 *   w1  [filters][td + channels]     conv1.weight as torch holds it (column 0: time)
 *   w2  [9][Fp][Fp]                  conv2.weight[:, td:] as [tap = 3 ky + kx][in][out], zero padded to Fp
 *   w2t [9][filters]                 conv2.weight[:, 0] as [tap][out] (time dependent only; else nullable)
 *   w3  [channels][td + filters]     conv3.weight as torch holds it (column 0: time)
 *   b1, b2 [filters], b3 [channels] */
#define MI_ODE_CONV_MAX_C 16
#define MI_ODE_CONV_MAX_F 128
enum mi_ode_conv_act { MI_ODE_CONV_ACT_RELU = 0, MI_ODE_CONV_ACT_SOFTPLUS = 1, MI_ODE_CONV_ACT_TANH = 2 };   /* softplus: beta 1, threshold 20 */
typedef struct mi_ode_conv_desc {
  int32_t dtype;              /* enum mi_ode_dtype */
  int32_t activation;         /* enum mi_ode_conv_act */
  int32_t time_dependent;     /* 0 / 1 */
  int32_t reserved;
  double sign;                /* +1, or -1 on a reversed time axis: k = -f(-t, y) */
  int64_t batch;
  int32_t channels, height, width, filters;
  const void *w1, *b1, *w2, *w2t, *b2, *w3, *b3;
} mi_ode_conv_desc;
/* y0, ks[j], k_out, y_out: device [batch, channels, height, width] contiguous; beta_row: host [n_k] (0 <= n_k <= 14); dt_dev: device
 * float64 step size (read when the kernel runs; unused when n_k = 0); t_dev: device stage time in the state dtype; y_out: nullable,
 * receives y_s.  Enqueues one launch on `stream`; returns 0 or a negative MI_ODE_E_*. */
int mi_ode_conv_stage(const mi_ode_conv_desc* desc, const void* y0, const void* const* ks, int32_t n_k, const double* beta_row,
                      const double* dt_dev, const void* t_dev, void* k_out, void* y_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_ODE_H */
