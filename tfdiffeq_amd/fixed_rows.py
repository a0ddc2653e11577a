"""Fixed-grid solves on every row's own time grid: `odeint(func, y0, t, method='euler' | 'rk4')` with `t` of shape
[batch, T] and, optionally, options['t_lengths'] (int [batch], 1 .. T).  Row i of the result [T, batch, dim] is bit for bit what
odeint(func, y0[i:i+1], t[i, :len_i], method=...) returns on the one-launch kernel; solution[len_i:, i] is exactly 0 and t[i, len_i:] is
never read.  One launch for any batch (csrc/mi_ode_fixed_rows_t.h).  What the kernel cannot take is a ValueError with the reason, decided
from `func`, shapes, dtypes and options before any launch; `odeint.plan` reports the same reason.  The options key 'per_trajectory' is
not needed - it is about step control, a fixed grid has none, and with a fixed-grid method it stays refused."""
import torch

from . import dispatch as D
from . import rows_times

REFUSED = D.FIXED_ROWS_T_REFUSED


def wanted(method, t, options):
    """True when the call is the fixed-grid route with per-row times: a method that is not adaptive Runge-Kutta, with a 2-D `t` or
    options['t_lengths'].  A 1-D `t` without lengths is the call as it was."""
    from .odeint import SOLVERS
    if method is None or method not in SOLVERS or D.rows_method_refusal(SOLVERS[method]) == '':
        return False
    if 't_lengths' in (options or {}):
        return True
    shape = D._shape_of(t)
    if shape is None and isinstance(t, (list, tuple)) and len(t) > 0 and (isinstance(t[0], (list, tuple)) or (D._shape_of(t[0]) or ()) != ()):     # (times as nested lists)
        return True
    return shape is not None and len(shape) >= 2


def target(func, y0, t, method, options):
    """(device right-hand side, state [batch, dim], lowered callable | None, solver options) of a call `wanted` - or ValueError with the
    reason.  No device is touched."""
    from .odeint import _descriptor, _wants_grad

    def refuse(why):
        raise ValueError(REFUSED + why)
    opts = {k: v for k, v in (options or {}).items() if k not in ('t_lengths', 'lower')}
    ys = tuple(y0) if isinstance(y0, (tuple, list)) else (y0,)
    descriptor = _descriptor(func)
    if getattr(func, 'stage_rhs', None) is not None and method in D.FIXED_ROWS_T_METHODS:      # (rhs.Conv2dODE: its state is not [batch, dim] either)
        refuse(D.rows_family_why(type(func).__name__, getattr(func, 'dim', None)))
    why = D.fixed_rows_t_refusal(method, None, ys, options, check_rhs=False)             # (method, options, state: before anything is traced)
    if why:
        refuse(why)
    y = ys[0]
    _wanted, why_t = rows_times.shapes(y, t, None, None, {'t_lengths': options['t_lengths']} if 't_lengths' in (options or {}) else {})
    if why_t:
        refuse(why_t)
    if getattr(func, 'stage_rhs', None) is not None:
        refuse(D.rows_family_why(type(func).__name__, getattr(func, 'dim', None)))
    if descriptor:
        why = D.fixed_rows_t_refusal(method, func, ys, options)
        if why:
            refuse(why)
        return func, y, None, opts
    if not callable(func):
        refuse('`func` is neither a DeviceRHS nor a callable')
    if torch.is_grad_enabled() and (y.requires_grad or _wants_grad(func, y0)):
        refuse('inputs that require grad: plain odeint has no gradient route over per-row grids - call odeint_discrete (the exact gradient of '
               'every row\'s own discrete map, one launch)')
    # (odeint.LOWER_DEFAULT / TFDIFFEQ_AMD_LOWER=0 choose between the tracer and the callable engines where both exist; here there is no
    # callable engine to fall back to, so - as for options['per_trajectory'] - asking for the route IS asking for the tracer, and only the
    # option itself declines)
    mode = (options or {}).get('lower', 'auto')
    if mode is False or mode == 'off':
        refuse("options['lower'] is False: a Python callable reaches the fixed-grid kernel with per-row times only as a lowered row program")
    from . import lower as _lower
    wrapped = func
    if y is not y0:                                          # a one-component tuple: the tensor form of the same system
        def wrapped(t_, y_, _f=func):
            return _f(t_, (y_,))[0]
    try:
        low = _lower.lower(wrapped, y.detach(), method=method)
    except _lower.TraceError as e:
        refuse('the tracer refuses this callable (%s), and a Python callable has no kernel that walks per-row grids' % e)
    except Exception as e:
        refuse('tracing this callable failed (%s: %s), and a Python callable has no kernel that walks per-row grids' % (type(e).__name__, e))
    why = D.fixed_rows_t_refusal(method, low.rhs, ys, options, lowered=(low.kind, low.dim))
    if why:
        refuse(why)
    if tuple(low.state_shape) != tuple(y.shape):
        refuse('the callable lowers to a program over a state of shape %s, not the [batch, dim] = %s of the call: row i of `t` must belong '
               'to row i of the program' % (tuple(low.state_shape), tuple(y.shape)))
    return low.rhs, y, low, opts


def times(y, t, options):
    """rows_times.prepare on the times rounded to the state dtype (solvers.py:84: a fixed-grid solver casts `t` to it)."""
    t = torch.as_tensor(t)
    if torch.is_floating_point(t):
        t = t.detach().to(y.dtype).to(torch.float64)
    lengths = {'t_lengths': options['t_lengths']} if 't_lengths' in (options or {}) else {}
    return rows_times.prepare(y, t, None, None, lengths, prefix=REFUSED)[0]


def solve(func, y0, t, method, options, prepared=None):
    """The call.  prepared: (target(...), times(...)) of a caller that has planned it already (odeint_discrete), so that `t` is validated
    and the callable resolved once."""
    from .graph_step import _credit_nfe
    from .misc import _check_inputs
    from .odeint import SOLVERS, odeint
    (rhs, y, low, opts), rt = prepared if prepared is not None else (target(func, y0, t, method, options), None)
    if rt is None:
        rt = times(y, t, options)
    state = y.detach().contiguous()
    # misc._check_inputs on a stand-in for the direction the rows share: the sign goes to the right-hand side as for a 1-D t
    _tensor_input, f, st, _ = _check_inputs(rhs, state, [0., -1.] if rt.decreasing else [0., 1.])
    solver = SOLVERS[method](f, st, **opts)
    sol = solver.integrate_rows_t(rt)[0]
    stats = getattr(solver, 'stats', {})
    if low is not None:
        info = low.describe()
        info['lowered'] = True
        stats['lower'] = info
        _credit_nfe(func, int(stats.get('nfe', 0)) - low.py_calls)
    odeint.last_stats = stats
    return (sol,) if isinstance(y0, (tuple, list)) else sol


def plan(func, y0, t, method, options):
    """odeint.plan for a call `wanted`: the kernel, or engine 'refused' with the reason the call raises."""
    from .plan import FAMILY, TNAME
    try:
        rhs, y, low, _opts = target(func, y0, t, method, options)
    except ValueError as e:
        return {'engine': 'refused', 'kernel': None, 'launches': None, 'why': str(e), 'lower': None}
    fam = D.family(rhs)
    return {'engine': 'fused', 'kernel': 'k_fixed_rowlocal_t<%s, %s> (a trajectory per thread on its own time grid, any batch size)' % (TNAME[y.dtype], method),
            'launches': 'one per call', 'why': D.FIXED_ROWS_T_WHY, 'family': FAMILY.get(fam, fam),
            'state': '%d x %d %s' % (int(y.shape[0]), int(y.shape[1]), str(y.dtype).replace('torch.', '')),
            'lower': None if low is None else {'lowered': True, 'kind': low.kind, 'dim': low.dim, 'batch_axes': low.trace.nb}}
