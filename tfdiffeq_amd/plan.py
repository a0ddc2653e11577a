"""`odeint.plan(func, y0, t, ...)`: which engine a call will take and the predicate that chose it - BEFORE running it, with or without a GPU.

The decision is not made here: `plan` constructs the solver `odeint` would construct and formats `solver.route()` (tfdiffeq_amd/dispatch.py, what
`integrate` itself consumes).  This module adds the name of the C++ kernel instantiation per route kind and family (csrc `pick_family` stays the
authority for C-ABI callers) and the launch count.  Co-residency is decided later, inside `mi_ode_create`: `plan` reports the rule and
`dispatch.after(route)` rather than the device's answer.

    >>> odeint.plan(lambda t, y: torch.matmul(y, W), y0, t, method='dopri5')
    {'engine': 'fused', 'family': 'linear', 'kernel': 'k_persist_linear_mfma<double, 128, 6>', 'launches': 'one per call', ...}
"""
import torch

from . import dispatch as D
from . import rhs as R
from .fixed_adams import AdamsBashforthMoulton
from .misc import _TupleFunc
from .solvers import FixedGridODESolver, _AdaptiveRKSolver

TNAME = {torch.float32: 'float', torch.float64: 'double'}
ENGINE = {'callable': 'callable', 'planes': 'plane kernels'}          # (every other route kind: 'fused')
FAMILY = {'rowlocal': 'row-local (a trajectory per thread)', 'coop': 'generated / user code, a thread per state element'}     # as displayed
# what a 'callable' route, and a 'planes' route of each solver family, runs on: (kernel, launches)
HOST = {'callable': ('k_opq_norms + k_opq_commit around torch kernels (graph_step.DeviceControlledRK)',
                     'one hipGraph replay per attempt once recorded (options graph=%r), eager before'),
        _AdaptiveRKSolver: ('mi_ode_lincomb / mi_ode_error_norms / mi_ode_interp_eval between evaluations of f', 'several per stage, the controller on the host'),
        AdamsBashforthMoulton: ('mi_ode_lincomb', 'several per step'),
        FixedGridODESolver: ('step_func over mi_ode_lincomb, one evaluation of forward() per stage', 'several per grid interval'),
        object: ('k_adams_predict / _correct / _error_sums / _update_phi', 'four per attempt')}
# the 'fused' route of an adaptive Runge-Kutta call on a family with ONE kernel: (kernel, launches, why); formatted with T, S, A, M
ADAPTIVE = {'rowlocal': ('k_persist_rowlocal<{T}, {S}, ..> (k_persist_rowlocal_planes beyond 131072 trajectories)', 'one per call',
                         'row_local right-hand side: state and stage derivatives thread-private'),
            'coop': ('k_persist_rowlocal<{T}, {S}, .., RhsUserCoop> (planes variant beyond a co-resident batch)', 'one per call',
                     'cooperative plugin: a thread per state element, dim <= 256'),
            'mlp': ('k_persist_mlp{M}<DP, HP, {A}, {S}> (dim / hidden padded; k_mlp per attempt when the tile grid is not co-resident)', 'one per call',
                    'rhs.MLP.supports: dim <= 64, hidden <= 128 - the MFMA tile kernels (float32: weights resident in registers; '
                    'float64: weights streamed from a packed copy)'),
            # (y ** 3) @ W beyond 2 x 2: csrc pick_family keeps the cube on the vector-ALU stage kernels
            'cubic_linear': ('k_stage_linear_valu', 'one per stage', '(y ** 3) @ W: the tile kernels have no cube in front of the product (measured in round 6: '
                             'a run-time switch for it costs the linear system 1.4 % at config 4) - the vector-ALU stage kernels, dim <= 256')}


def _host(solver, route, opts, why=None):
    """A 'callable' / 'planes' route, formatted."""
    key = 'callable' if route.kind == 'callable' else next(k for k in HOST if isinstance(k, type) and isinstance(solver, k))
    return {'engine': ENGINE[route.kind], 'kernel': HOST[key][0], 'launches': HOST[key][1].replace('%r', repr(opts.get('graph', 'auto'))),
            'why': route.why if why is None else why}


def plan_conv(rhs, y, solver, route, opts):
    """rhs.Conv2dODE: the fused stage kernel (csrc/mi_ode_conv.h) inside its box, the torch module on the callable engine outside."""
    why, rk = rhs.in_box(y), isinstance(solver, _AdaptiveRKSolver)
    if why:
        d = _host(solver, route, opts, 'rhs.Conv2dODE outside the fused kernel\'s box (%s): the torch module runs' % why)
    elif route.kind == 'callable':
        d = _host(solver, route, opts, 'rhs.Conv2dODE: each Runge-Kutta stage (stage state + three convolutions) is one launch')
        d['kernel'] = 'k_conv_stage<%s> per stage + k_opq_norms + k_opq_commit (graph_step.DeviceControlledRK)' % TNAME[y.dtype]
    else:                                                # (graph='host', force_plane_kernels, process_group: the host loop calls f per stage)
        d = _host(solver, route, opts, 'rhs.Conv2dODE on the host-controlled loop (the options ask for it): one fused evaluation per stage'
                  if rk else 'rhs.Conv2dODE on a fixed-grid / multistep method')
        d['kernel'] = 'k_conv_stage<%s> per evaluation of f, plane kernels between' % TNAME[y.dtype]
        d['launches'] = d['launches'] if rk else 'one per evaluation of f plus the solver\'s state arithmetic'
    d.update(family='conv2d', fused_stage=not why,
             box='NCHW float32 / float64, C <= %d, F <= %d, relu / softplus / tanh, any H, W, batch' % (rhs.MAX_C, rhs.MAX_F))
    if not why:
        d['odeblock'] = ('fused stage kernel' if rhs.faster_than_torch(y) else
                         'torch module: %.3g GFLOP of conv2 per evaluation > %.3g, where the fused kernel measured slower than torch'
                         % (rhs.conv2_flop(y) / 1e9, rhs.FUSED_MAX_CONV2_FLOP / 1e9))
    return d


def _linear_kernel(dim, T, S, fusion):
    """(kernel, launches, why) of rhs.Linear on the 'fused' route of an adaptive Runge-Kutta call: the tier csrc `pick_family` picks."""
    per = {D.STAGE: 'stage', D.STEP: 'attempt'}.get(fusion)
    if 3 <= dim <= 128 or (128 < dim <= 256 and S in (3, 6) and fusion != D.STAGE):
        tile = 256 if dim > 128 else max(16, 1 << (dim - 1).bit_length())
        kernel = 'k_%s_linear_mfma<%s, %d, %d> (one kernel per %s)' % ('step' if per == 'attempt' else 'stage', T, tile, S, per) if per else \
            'k_persist_linear_mfma<%s, %d, %d> (co-resident batch; k_step_linear_mfma per attempt otherwise)' % (T, tile, S)
        return kernel, 'per %s' % per if per else 'one per call', (
            '3 <= dim <= 128: the MFMA tile kernels (W slice resident in registers)' if dim <= 128 else
            '128 < dim <= 256, three- or six-row tableau: the 256-wide MFMA tile kernels (W streamed from a copy in consumption order, '
            'csrc/mi_ode_step_fused.h LinCtx::STREAM)')
    return ('k_stage_linear_valu', 'one per stage',
            'dim %d outside 3 .. 128 (and not a dopri5 / tsit5 / bosh3 call at dim <= 256): the vector-ALU fallback (dim <= 256)' % dim)


def plan_rhs(rhs, y, solver, route, opts):
    """A DeviceRHS and ONE state tensor: the solver's route, formatted (shape / dtype are read, nothing else)."""
    T, fam, kind = TNAME[y.dtype], D.family(rhs), route.kind
    d = {'engine': ENGINE.get(kind, 'fused'), 'launches': 'one per call', 'why': route.why}
    if kind in ENGINE:
        d = _host(solver, route, opts)
    elif kind == 'fused_multistep':
        d['kernel'] = '%s<%s, ..>' % ('k_fixed_adams_rowlocal' if isinstance(solver, FixedGridODESolver) else 'k_adams_vc_rowlocal', T)
        d['launches'] = 'one per call (co-resident batch; %s otherwise)' % ENGINE[D.after(route).kind]
    elif isinstance(solver, FixedGridODESolver):
        k = 'k_fixed_rowlocal' if (fam in ('rowlocal', 'coop') or kind == 'fused_coop') else \
            ('k_fixed_mlp' if fam == 'mlp' else 'k_fixed_linear_mfma' if (fam == 'linear' and 3 <= rhs.dim <= 256) else 'FX_* stage kernels (vector ALU)')
        d['kernel'] = '%s<%s, ..>' % (k, T)
    elif kind == 'fused_coop':
        d['kernel'] = 'k_persist_rowlocal<%s, %d, .., RhsMlpCoop> (planes variant beyond a co-resident batch)' % (T, len(solver.tableau.alpha))
    else:                                               # the family's own sentence says which of its kernels, and why
        S = len(solver.tableau.alpha)
        k = _linear_kernel(int(rhs.dim), T, S, solver._fusion) if fam == 'linear' else ADAPTIVE.get(fam, ('catalogue kernels of ' + fam, 'one per call', route.why))
        fmt = dict(T=T, S=S, M='' if y.dtype == torch.float32 else '64', A=R.MLP.ACTIVATIONS.get(getattr(rhs, 'activation', None)))
        d.update(kernel=k[0].format(**fmt) if fam != 'linear' else k[0], launches=k[1], why=k[2])
    d.update(family=FAMILY.get(fam, fam), state='%d x %d %s' % (y.numel() // max(int(rhs.dim or 1), 1), rhs.dim, str(y.dtype).replace('torch.', '')))
    return d


def plan_rows(func, y0, rtol, atol, method, opts, t=None):
    """options['per_trajectory']: the per-trajectory kernel (csrc/mi_ode_rows.h) - or the reason the call is refused with (a ValueError
    at the call: shared control is never substituted).  t: with a 2-D `t`, options['t_lengths'] or [batch] tolerances the kernel is
    k_rows_rowlocal_t (csrc/mi_ode_rows_t.h); decided from shapes alone, as the call refuses them (values are checked by the call)."""
    from . import rows_times
    from .odeint import SOLVERS, _per_trajectory_target
    per_row_t = False
    try:
        per_row_t, why = rows_times.shapes(y0, t, rtol, atol, opts)
        if why:
            raise ValueError("options['per_trajectory'] refused: " + why)
        if per_row_t:
            opts = {k: v for k, v in opts.items() if k != 't_lengths'}
            rtol, atol = (D.ROWS_T_RTOL0 if D._shape_of(rtol) else rtol), (D.ROWS_T_ATOL0 if D._shape_of(atol) else atol)      # (the handle's: rows_times.prepare)
        low, run_opts = _per_trajectory_target(func, y0, method, opts)
        f, state = (func, y0) if low is None else (low.rhs, (y0[0] if isinstance(y0, (tuple, list)) else y0).reshape(low.state_shape))
        run_opts.pop('lower', None)
        ys = (state,) if isinstance(state, torch.Tensor) else tuple(state)
        solver = SOLVERS[method](_TupleFunc(f), ys, rtol=rtol, atol=atol, **run_opts)
        route = solver.route()
    except ValueError as e:
        return {'engine': 'refused', 'kernel': None, 'launches': None, 'per_trajectory': True, 'why': str(e), 'lower': None}
    y, rhs, S = ys[0], route.rhs, len(solver.tableau.alpha)
    fam = D.family(rhs)
    lower = None if low is None else {'lowered': True, 'kind': low.kind, 'dim': low.dim, 'batch_axes': low.trace.nb}
    if route.kind == 'fused_rows_mlp':
        if per_row_t:
            return {'engine': 'refused', 'kernel': None, 'launches': None, 'per_trajectory': True,
                    'why': "options['per_trajectory'] refused: " + D.ROWS_MLP_T_REFUSAL, 'lower': None}
        dp, hp = (16 if rhs.dim <= 16 else 64), (16 if rhs.hidden <= 16 else 128)
        return {'engine': 'fused', 'kernel': 'k_rows_mlp<%d, %d, %s, %d, ..> (a 32-row tile per workgroup with the weights resident, every row its own '
                                             'control, a loop over tiles: any batch size, no grid hand-off)' % (dp, hp, rhs.activation, S),
                'launches': 'one per call', 'why': D.ROWS_MLP_WHY, 'per_trajectory': True, 'family': FAMILY.get(fam, fam),
                'state': '%d x %d %s' % (y.numel() // max(int(rhs.dim or 1), 1), rhs.dim, str(y.dtype).replace('torch.', '')), 'lower': lower}
    kernel, why = ('k_rows_rowlocal_t<%s, %d, ..> (a trajectory per thread with its own times, length and tolerances, any batch size, no grid hand-off)',
                   D.ROWS_T_WHY) if per_row_t else ('k_rows_rowlocal<%s, %d, ..> (a trajectory per thread, any batch size, no grid hand-off)', D.ROWS_WHY)
    return {'engine': 'fused', 'kernel': kernel % (TNAME[y.dtype], S),
            'launches': 'one per call', 'why': why, 'per_trajectory': True, 'family': FAMILY.get(fam, fam),
            'state': '%d x %d %s' % (y.numel() // max(int(rhs.dim or 1), 1), rhs.dim, str(y.dtype).replace('torch.', '')),
            'lower': None if low is None else {'lowered': True, 'kind': low.kind, 'dim': low.dim, 'batch_axes': low.trace.nb}}


def plan(func, y0, t=None, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint=False):
    """What `odeint(func, y0, t, rtol, atol, method, options)` will run on.  A dict: engine ('fused' | 'callable' | 'plane kernels'),
    kernel, launches, why (the predicate that decided), family / state, and `lower` (how a Python callable was lowered, or why not).
    adjoint=True (with options['per_trajectory']): what `odeint_adjoint` runs for the same arguments - the per-trajectory adjoint kernel, or
    engine 'refused' with the reason (`odeint_adjoint.plan`, which also takes the adjoint_* arguments)."""
    if adjoint:
        from . import rows_adjoint
        return rows_adjoint.plan(func, y0, t, rtol=rtol, atol=atol, method=method, options=options)
    from . import lower as L
    from .odeint import LOWER_DEFAULT, SOLVERS       # (the submodule: the package exports the function under its name)
    method = method or 'dopri5'
    opts = dict(options or {})
    opts, per_row = D.per_trajectory_option(opts)
    if per_row:
        return plan_rows(func, y0, rtol, atol, method, opts, t)
    from . import fixed_rows
    if fixed_rows.wanted(method, t, opts):
        return fixed_rows.plan(func, y0, t, method, opts)
    mode = opts.pop('lower', LOWER_DEFAULT)
    tensor_input = isinstance(y0, torch.Tensor)
    ys = (y0,) if tensor_input else tuple(y0)

    def routed(f, state, lift=tensor_input):
        """The solver `odeint` constructs for this call (misc._check_inputs, odeint.py) and the route it takes."""
        solver = SOLVERS[method](_TupleFunc(f) if lift else f, state, rtol=rtol, atol=atol, **opts)
        return solver, solver.route()
    why_not = None
    if getattr(func, 'stage_rhs', None) is not None and len(ys) == 1:
        return dict(plan_conv(func.stage_rhs, ys[0], *routed(func, ys), opts), lower=None)
    if getattr(func, 'kind', 0) and len(ys) == 1:
        return dict(plan_rhs(func, ys[0], *routed(func, ys), opts), lower=None)
    if getattr(func, 'per_component', False):
        solver, route = routed(func, ys)
        d = _host(solver, route, opts) if route.kind != 'fused_tuple' else {
            'engine': 'fused', 'launches': 'one per call', 'why': route.why,
            'kernel': 'k_fixed_rowlocal over the concatenated components' if isinstance(solver, FixedGridODESolver) else 'k_persist_rowlocal over one segmented buffer'}
        fam = D.family(func.device_rhs)
        return dict(d, family='tuple of ' + FAMILY.get(fam, fam), lower=None)
    if len(ys) == 1 and not getattr(func, 'kind', 0):
        why_not, lowered = D.not_traced(opts, mode), None
        # (a one-component tuple: `odeint` lowers the tensor form of the same system and re-enters with a tensor state, odeint.py `_try_lower`)
        f1 = func if tensor_input else (lambda t_, y_: func(t_, (y_,))[0])
        try:
            if not why_not:
                tr = L.trace(f1, ys[0])
                prog = L.program_for(tr, generic=method in L.GENERIC_ONLY_METHODS)
                lowered = prog.bind(tr, ys[0].device) if prog.kind in ('linear', 'cubic', 'mlp') else prog.rhs
        except L.TraceError as e:
            why_not = str(e)
        except Exception as e:
            why_not = 'tracing failed: %s: %s' % (type(e).__name__, e)
        if lowered is not None:
            shaped = ys[0].reshape(tr.batch_shape + (prog.dim,))
            return dict(plan_rhs(lowered, shaped, *routed(lowered, (shaped,), True), opts),
                        lower={'lowered': True, 'kind': prog.kind, 'dim': prog.dim, 'batch_axes': tr.nb})
    solver, route = routed(func, ys)
    return dict(_host(solver, route, opts, route.why + (' (%s)' % why_not if why_not else '')), lower={'lowered': False, 'why': why_not} if why_not else None)
