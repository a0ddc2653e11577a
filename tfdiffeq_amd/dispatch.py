"""Which engine an `odeint` call runs on: the one decision the solvers (solvers.py, adams.py), `odeint.plan`, `odeint`'s tracer gate and
`models.ODEBlock` share.  Pure functions of the descriptor behind `func` (`device_rhs`, `per_component`), the state's shapes and dtypes, the
tableau's shape or the multistep kind, and the normalised options: no engine, no library, no device (the solvers refuse host tensors BEFORE
they ask).  What only `mi_ode_create` or a run can know - co-residency, a grid hand-off that timed out - is the solvers' fallback to `after`."""
import collections

import torch

from . import _native as N
from . import rhs as R

# options['fusion']: the schedule of the fused engine, by name or by the code include/mi_ode.h gives it; normalised where the option is popped
FUSION = {'auto': 0, 'stage': 1, 'step': 2, 'step_split': 3, 'whole': 4}
AUTO, STAGE, STEP, WHOLE = (FUSION[k] for k in ('auto', 'stage', 'step', 'whole'))

# kind:  fused            one state tensor on the catalogue / tile / row-local kernels
#        fused_coop       the cooperative whole-call kernel (a network outside the tile kernels' box, or a tableau they are not instantiated for)
#        fused_tuple      rhs.PerComponent over one segmented (adaptive) or concatenated (fixed grid) buffer
#        fused_multistep  the one-launch fixed-order / variable-order Adams kernels
#        fused_rows       options['per_trajectory']: every row an integration of its own on k_rows_rowlocal (no fallback: refused or run)
#        fused_rows_mlp   options['per_trajectory'] for the float32 ODEFunc network: a 32-row tile per workgroup on k_rows_mlp, every row its own control
#        callable         graph_step.DeviceControlledRK: f as a callable, the controller on the device
#        planes           the host loop over plane kernels
# rhs: the DeviceRHS a fused engine is built from.  why: the predicate that decided.  told: a descriptor whose family has no kernel for
# this problem and says so once (`warn_limits`).
Route = collections.namedtuple('Route', 'kind rhs why told', defaults=(None,))

_TUPLE_WHY = 'rhs.PerComponent of a row-local right-hand side: tuple components share one buffer'
_PYTHON = {True: 'a Python callable', False: 'a tuple state of a Python callable'}        # by len(y0) == 1


def after(route, device_controlled=False):
    """The order, stated once: fused* -> callable (an adaptive Runge-Kutta call `device_controlled(...)` takes) -> planes."""
    kind = 'callable' if device_controlled and route.kind.startswith('fused') else 'planes'
    return Route(kind, None, 'no one-launch kernel for this batch: its workgroups are not co-resident, or the grid hand-off timed out')


def _single(rhs, y0, multistep=False):
    """`rhs` if its fused kernels (multistep: the one-launch Adams kernels, with limits of their own) take the ONE state tensor, else None."""
    y = y0[0]
    if rhs is None or len(y0) != 1 or not (isinstance(y, torch.Tensor) and y.dim() >= 1 and y.numel() > 0):
        return None
    return rhs if (rhs.supports_multistep if multistep else rhs.supports)(y) else None


def _coop(rhs, y0, any_box=False):
    """`rhs` if the cooperative one-launch kernel is its route for the ONE state tensor (rhs.MLP.supports_coop), else None."""
    if rhs is None or len(y0) != 1 or not hasattr(rhs, 'supports_coop') or not isinstance(y0[0], torch.Tensor) or y0[0].numel() == 0:
        return None
    return rhs if rhs.supports_coop(y0[0], any_box=any_box) else None


def _tuple(func, y0):
    """The row-local DeviceRHS behind a `rhs.PerComponent` lift if this tuple state can travel as one buffer, else None."""
    rhs, y = getattr(func, 'device_rhs', None), y0[0]
    if rhs is None or not getattr(func, 'per_component', False) or not getattr(rhs, 'row_local', False) or not 2 <= len(y0) <= N.MAX_SEGMENTS:
        return None
    ok = all(isinstance(c, torch.Tensor) and c.dim() >= 1 and c.numel() > 0 and c.dtype == y.dtype and c.device == y.device and rhs.supports(c) for c in y0)
    return rhs if ok else None


def family(rhs):
    """The kernel family of a descriptor, as csrc `pick_family` sees it: 'rowlocal', 'coop', 'mlp', 'cubic_linear', 'linear' or its class name."""
    if getattr(rhs, 'row_local', False):
        return 'rowlocal'
    if getattr(rhs, 'coop', False) or isinstance(rhs, R.CustomCoop):
        return 'coop'
    for cls, name in ((R.MLP, 'mlp'), (R.CubicLinear, 'cubic_linear'), (R.Linear, 'linear')):
        if isinstance(rhs, cls):
            return name
    return type(rhs).__name__


def has_kernel(rhs, y):
    """True when a Runge-Kutta kernel of the descriptor's family takes this state tensor: its own box or the cooperative kernel's."""
    return _single(rhs, (y,)) is not None or _coop(rhs, (y,)) is not None


def device_controlled(y0, rows, *, quartic, force_planes, group, graph):
    """True where graph_step.DeviceControlledRK takes a callable; False: the loop with the controller on the host."""
    like = y0[0]
    if graph == 'host' or force_planes or group or not 1 <= len(y0) <= N.MAX_SEGMENTS or rows + 1 not in (2, 4, 7, 14):
        return False
    if like.dtype not in (torch.float32, torch.float64) or any(y.dtype != like.dtype or y.device != like.device or y.numel() == 0 for y in y0):
        return False
    return quartic or rows == 6


ROWS_WHY = 'per-trajectory step control, one launch'
ROWS_TABLEAUS = 'dopri5, tsit5, bosh3, dopri8 and adaptive_heun'


def per_trajectory_option(options):
    """(options without the key, True | False) for options['per_trajectory']; anything but True / False is a ValueError."""
    opts = dict(options or {})
    value = opts.pop('per_trajectory', False)
    if value is not True and value is not False:
        raise ValueError("options['per_trajectory'] must be True or False (got %r)" % (value,))
    return (opts if options is not None else None), value


def rows_method_refusal(solver_cls):
    """'' when `solver_cls` is an adaptive Runge-Kutta solver, else why options['per_trajectory'] refuses it."""
    from .solvers import _AdaptiveRKSolver                # (solvers imports this module)
    if isinstance(solver_cls, type) and issubclass(solver_cls, _AdaptiveRKSolver):
        return ''
    return ('a fixed-grid or Adams method (%s): every row already takes the same steps on a fixed grid, and the Adams kernels have shared '
            'control only - per-trajectory step control exists for %s' % (getattr(solver_cls, '__name__', solver_cls), ROWS_TABLEAUS))


ROWS_MLP_WHY = 'per-trajectory step control on the MLP tile kernel: a 32-row tile per workgroup, every row its own control, one launch'
ROWS_MLP_TABLEAUS = 'dopri5, tsit5 and bosh3'
ROWS_MLP_BOX = ('the float32 ODEFunc network (rhs.MLP, rhs.from_sequential, models.ODEFunc, a lowered Linear / activation / Linear / activation / '
                'Linear) with dim <= %d and hidden <= %d on %s' % (R.MLP.MAX_DIM, R.MLP.MAX_HIDDEN, ROWS_MLP_TABLEAUS))
ROWS_MLP_T_REFUSAL = ('per-row times, lengths or tolerances (a 2-D `t`, options[\'t_lengths\'], `rtol` / `atol` tensors) with the ODEFunc network: '
                      'k_rows_mlp reads one `t` and one tolerance pair for all rows - pass a 1-D `t` and scalar tolerances')


def rows_family_why(name, dim, also=''):
    """also: what the caller's route takes beyond the trajectory-per-thread right-hand sides (the adaptive route: ROWS_MLP_BOX)."""
    return ('a right-hand side on the matrix-core or cooperative kernels (%s, dim %s): f is evaluated by the threads of a workgroup '
            'together there, and a barrier under per-lane control flow cannot be - per-trajectory control takes rhs.Lorenz, '
            'rhs.LotkaVolterra, 2 x 2 rhs.Linear / rhs.CubicLinear, rhs.CustomRowLocal and lowered callables of at most 32 elements%s'
            % (name, dim, (', and ' + also) if also else ''))


def rows_mlp_refusal(dev, y, rows, fsal, quartic=True):
    """'' when k_rows_mlp (csrc/mi_ode_rows_mlp.h) takes an options['per_trajectory'] call of the rhs.MLP `dev`, else the reason.  Pure."""
    name = type(dev).__name__
    if not (isinstance(y, torch.Tensor) and y.dim() >= 1 and y.numel() > 0 and y.shape[-1] == dev.dim):
        return rows_family_why(name, dev.dim, ROWS_MLP_BOX) + ': the state must be a non-empty [batch, %d] tensor' % dev.dim
    if y.dtype != torch.float32:
        return rows_family_why(name, dev.dim, ROWS_MLP_BOX) + (': this state is %s (the float64 tile kernel has no registers left for a '
                                                               'row\'s own step, time and record)' % str(y.dtype).replace('torch.', ''))
    if dev.dim > R.MLP.MAX_DIM or dev.hidden > R.MLP.MAX_HIDDEN:
        return rows_family_why(name, dev.dim, ROWS_MLP_BOX) + ': this network is %d -> %d (outside the tile kernels\' box)' % (dev.dim, dev.hidden)
    if not ((fsal and rows == 3 and quartic) or (fsal and rows == 6)):
        named = {13: 'dopri8', 1: 'adaptive_heun'}.get(rows, 'this method')
        return ('a %d-row tableau (%s) the per-trajectory MLP tile kernel is not instantiated for: it is for %s (a tile keeps k_1 .. k_S of '
                'its rows in registers next to the resident weights)' % (rows, named, ROWS_MLP_TABLEAUS))
    return ''


def rows_refusal(func, y0, rows, fsal, *, quartic=True, force_planes=False, group=False):
    """'' when k_rows_rowlocal (csrc/mi_ode_rows.h) - for an rhs.MLP: k_rows_mlp - takes this call, else the reason options['per_trajectory'] is refused with.  Pure: reads
    the descriptor behind `func`, shapes and dtypes - never the device."""
    dev = getattr(func, 'device_rhs', None)
    if getattr(func, 'per_component', False) or len(y0) != 1:
        return ('a tuple state of several components / rhs.PerComponent: the components of a tuple share one step size by definition '
                '(misc.py:250-287) - pass one [batch, dim] tensor')
    if group:
        return 'a sharded run (process_group): rows never communicate, so shard the batch yourself and call once per rank'
    if force_planes:
        return "options['force_plane_kernels'] asks for the host loop, which has shared control only"
    if dev is None:
        return ('a Python callable that was not lowered: only a right-hand side that runs on the trajectory-per-thread kernels can have '
                'per-trajectory control')
    y = y0[0]
    if isinstance(dev, R.MLP):
        return rows_mlp_refusal(dev, y, rows, fsal, quartic)
    if not getattr(dev, 'row_local', False) or not (isinstance(y, torch.Tensor) and y.dim() >= 1 and y.numel() > 0 and dev.supports(y)):
        return rows_family_why(type(dev).__name__, getattr(dev, 'dim', None), ROWS_MLP_BOX)
    one_row = rows == 1 and not fsal
    if not ((fsal and rows in (3, 13) and quartic) or (fsal and rows == 6) or (one_row and quartic)):
        return 'a %d-row tableau the per-trajectory kernel is not instantiated for (it is for %s)' % (rows, ROWS_TABLEAUS)
    return ''


ROWS_T_WHY = 'per-trajectory step control with per-row times, lengths or tolerances, one launch'
# what a handle or descriptor is created with where every row brings a tolerance of its own (the kernels read the row's, never these)
ROWS_T_RTOL0, ROWS_T_ATOL0 = 1e-6, 1e-9


def _shape_of(x):
    """The shape of a tensor or numpy array, None for anything else (a Python scalar; a tuple of tolerances keeps the reference's meaning:
    one per component of a tuple state)."""
    if isinstance(x, torch.Tensor) or type(x).__name__ == 'ndarray':
        return tuple(x.shape)
    return None


def rows_t_wanted(t_shape, rtol_shape, atol_shape, has_lengths):
    """True when an options['per_trajectory'] call goes to k_rows_rowlocal_t (csrc/mi_ode_rows_t.h): a 2-D `t`, or rtol / atol that are
    not scalars.  A 1-D `t` with scalar tolerances is the shared-t call, as it was - with options['t_lengths'] a ValueError.  Pure: shapes only
    (a scalar's is None or ())."""
    if has_lengths and (t_shape is None or len(t_shape) != 2):
        raise ValueError("options['t_lengths'] needs a 2-D `t` of shape [batch, T]: the lengths say how many of a row's own times count")
    return (t_shape is not None and len(t_shape) >= 2) or any(s is not None and len(s) >= 1 for s in (rtol_shape, atol_shape))


def rows_t_refusal(y_shape, t_shape, lengths_shape=None, lengths_is_int=True, rtol_shape=None, atol_shape=None,
                   names=('rtol', 'atol')):
    """'' when the per-row inputs of an options['per_trajectory'] call fit its state, else the reason the call is refused with.  Pure:
    shapes and one dtype flag.  (Values - lengths in 1 .. T, monotone rows - are checked on the tensors: rows_times.prepare.)"""
    if len(y_shape) != 2:
        return ('per-row times, lengths or tolerances with a state of shape %s: row i of `t`, `rtol`, `atol` belongs to row i of a '
                '[batch, dim] state' % (tuple(y_shape),))
    batch = int(y_shape[0])
    if len(t_shape) not in (1, 2) or (len(t_shape) == 2 and (int(t_shape[0]) != batch or int(t_shape[1]) < 1)):
        return ('`t` of shape %s for a state of %d rows: a 2-D `t` is [batch, T] with T >= 1, row i the output times of row i'
                % (tuple(t_shape), batch))
    if lengths_shape is not None:
        if not lengths_is_int:
            return "options['t_lengths'] must be an integer tensor of shape [batch] (values in 1 .. T)"
        if tuple(lengths_shape) != (batch,):
            return "options['t_lengths'] of shape %s for a state of %d rows: one length per row, shape [batch]" % (tuple(lengths_shape), batch)
    for name, shape in zip(names, (rtol_shape, atol_shape)):
        if shape is not None and len(shape) >= 1 and tuple(shape) != (batch,):
            return '`%s` of shape %s for a state of %d rows: a scalar, or one value per row, shape [batch]' % (name, tuple(shape), batch)
    return ''


FIXED_ROWS_T_WHY = 'euler / rk4 on every row\'s own time grid (per-row times and lengths), one launch'
FIXED_ROWS_T_REFUSED = 'a 2-D `t` / options[\'t_lengths\'] with a fixed-grid or Adams method refused: '
FIXED_ROWS_T_METHODS = ('euler', 'rk4')


def fixed_rows_t_refusal(method, dev, y0, options, lowered=None, check_rhs=True):
    """'' when k_fixed_rowlocal_t (csrc/mi_ode_fixed_rows_t.h) takes a fixed-grid call with a 2-D `t`, else the reason the call is refused
    with.  Pure: the method's name, the descriptor `dev` behind func (None: a Python callable that was not lowered), the state tuple and
    the option keys - never the device.  lowered: (kind, dim) of a lowered callable's program; check_rhs False: method, options and state only."""
    if method not in FIXED_ROWS_T_METHODS:
        return ('method %r has no one-launch forward kernel a row\'s own time grid could be defined against (bit for bit the batch-of-one '
                'call): per-row times exist for %s' % (method, ' and '.join(FIXED_ROWS_T_METHODS)))
    opts = options or {}
    for key in ('step_size', 'grid_constructor'):
        if opts.get(key) is not None:
            return ('options[%r] gives the solver a grid of its own, and per-row grids with interpolated outputs are not built: with a 2-D `t` '
                    'every row steps on its own times' % key)
    if float(opts.get('eps', 0.0) or 0.0) != 0.0:
        return "options['eps'] != 0 shifts the evaluation times off the rows' own grids, which is not built for a 2-D `t`"
    if opts.get('process_group') is not None:
        return 'a sharded run (process_group): rows never communicate, so shard the batch yourself and call once per rank'
    if len(y0) != 1 or not isinstance(y0[0], torch.Tensor):
        return 'a tuple state: row i of `t` belongs to row i of ONE [batch, dim] state tensor'
    y = y0[0]
    if y.dim() != 2 or y.numel() == 0 or y.dtype not in (torch.float32, torch.float64):
        return 'a state of shape %s, dtype %s: row i of `t` belongs to row i of a non-empty float32 / float64 [batch, dim] state' % (tuple(y.shape), y.dtype)
    if not check_rhs:
        return ''
    if dev is None:
        return ('a Python callable that was not lowered: only a right-hand side on the trajectory-per-thread kernels can walk every row '
                'over its own times')
    if lowered is not None and lowered[0] != 'rowlocal':
        return rows_family_why("a lowered '%s' program" % lowered[0], lowered[1])
    if not getattr(dev, 'row_local', False) or not dev.supports(y):
        return rows_family_why(type(dev).__name__, getattr(dev, 'dim', None))
    return ''


def fixed_rows_t(func, y0, method, options=None):
    """The fixed-grid solvers with per-row times: k_fixed_rowlocal_t or a ValueError - there is no other schedule."""
    dev = getattr(func, 'device_rhs', None)
    why = fixed_rows_t_refusal(method, dev, y0, options)
    if why:
        raise ValueError(FIXED_ROWS_T_REFUSED + why)
    return Route('fused_rows_t', dev, 'k_fixed_rowlocal_t: ' + FIXED_ROWS_T_WHY)


ROWS_ADJOINT_WHY = 'per-trajectory adjoint: every row its own augmented solve with per-component control, one launch'
ROWS_ADJOINT_T_WHY = 'per-trajectory adjoint over per-row times, lengths or tolerances: every row its own augmented solve, one launch'
ROWS_ADJOINT_METHODS = ('dopri5', 'bosh3')


def rows_adjoint_refusal(dim, n_params, adjoint_method, adjoint_rtol, adjoint_atol, adjoint_options):
    """'' when k_rows_adjoint (csrc/mi_ode_rows_adjoint.h) takes the backward of an options['per_trajectory'] call whose forward
    k_rows_rowlocal takes, else the reason odeint_adjoint refuses it with.  Pure: sizes, names and option keys only."""
    n_aug = 2 * int(dim) + 1 + max(int(n_params), 1)
    if n_aug > N.ROWS_ADJOINT_MAX_AUG:
        return ('an augmented state of N_aug = 2 * %d + 1 + %d = %d elements per row: (y, adj_y, adj_t, adj_params) and its stage derivatives are '
                'thread-private, the limit is %d' % (dim, max(int(n_params), 1), n_aug, N.ROWS_ADJOINT_MAX_AUG))
    if adjoint_method not in ROWS_ADJOINT_METHODS:
        return 'adjoint_method %r: the per-trajectory adjoint kernel is instantiated for %s' % (adjoint_method, ' and '.join(ROWS_ADJOINT_METHODS))
    if isinstance(adjoint_rtol, (tuple, list)) or isinstance(adjoint_atol, (tuple, list)):
        return 'tuple adjoint_rtol / adjoint_atol: the kernel takes one scalar pair for the four components'
    extra = sorted(k for k in (adjoint_options or {}) if k != 'max_num_steps')
    if extra:
        return 'adjoint_options %s: the kernel\'s controller takes max_num_steps only (pass adjoint_options explicitly)' % extra
    return ''


def adaptive_rk(func, y0, rows, fsal, *, quartic=True, force_planes=False, group=False, fusion=AUTO, graph='auto', per_trajectory=False):
    """The adaptive Runge-Kutta solvers.  rows, fsal: the tableau's shape; quartic: the dense output is the quartic through the midpoint.
    per_trajectory: every row of the batch is an integration of its own (k_rows_rowlocal, k_rows_mlp) - or a ValueError: never shared control."""
    if per_trajectory:
        why = rows_refusal(func, y0, rows, fsal, quartic=quartic, force_planes=force_planes, group=group)
        if why:
            raise ValueError("options['per_trajectory'] refused: " + why)
        if isinstance(func.device_rhs, R.MLP):
            return Route('fused_rows_mlp', func.device_rhs, ROWS_MLP_WHY)
        return Route('fused_rows', func.device_rhs, ROWS_WHY)

    def host(why, told=None):
        ok = device_controlled(y0, rows, quartic=quartic, force_planes=force_planes, group=group, graph=graph)
        return Route('callable' if ok else 'planes', None, why, told)
    dev = getattr(func, 'device_rhs', None)
    if dev is None:
        return host(_PYTHON[len(y0) == 1])
    if force_planes:
        return host("options['force_plane_kernels']")
    one_row = rows == 1 and not fsal
    whole = not group and fusion in (AUTO, WHOLE)
    rhs = boxed = _single(dev, y0)
    if rhs is not None and one_row and hasattr(rhs, 'supports_coop'):
        rhs = None                                   # adaptive_heun: the MLP tile kernels have no 1-row tableau - the cooperative kernel does
    if rhs is None and whole:
        if _tuple(func, y0) is not None:             # tuple state of a row-local RHS: one segmented buffer
            return Route('fused_tuple', dev, _TUPLE_WHY)
        if _coop(dev, y0, any_box=one_row) is not None:
            # a network outside the tile kernels' box (float64, wide): the cooperative whole-call kernel (it exists for every adaptive tableau)
            return Route('fused_coop', dev, 'rhs.MLP.supports_coop: outside the tile kernels\' box (dim <= 64, hidden <= 128), inside the '
                         'cooperative kernel\'s (<= 256 wide) and under COOP_MAX_FMA multiply-adds per evaluation')
    # dopri8 (13 rows) and adaptive_heun (1 row, not FSAL shaped): row-local kernels only, no per-stage schedule
    wide_ok = ((fsal and rows == 13) or one_row) and fusion != STAGE and (
        getattr(rhs, 'row_local', False) or getattr(rhs, 'wide_tableaus', False) or (rows == 13 and getattr(rhs, 'tile_dopri8', False)))
    if rhs is not None and (wide_ok or (fsal and rows in (3, 6))):
        return Route('fused', rhs, 'supports(y0)')
    if boxed is not None:
        why = 'the %d-row tableau exists for row-local / cooperative right-hand sides%s only' % (rows, ' and the tile kernels' if rows == 13 else '')
    elif getattr(func, 'per_component', False):
        why = 'rhs.PerComponent shares one buffer on the whole-call schedule only (2 .. %d components, row-local, no process group)' % N.MAX_SEGMENTS
    else:
        why = '%s.supports(y0) is False (dim %s, dtype %s)' % (type(dev).__name__, dev.dim, getattr(y0[0], 'dtype', None))
    # (e.g. hidden > 256: no kernel of the family takes it - the descriptor says so once)
    told = rhs is None and whole and len(y0) == 1 and hasattr(dev, 'warn_limits') and isinstance(y0[0], torch.Tensor) and not dev.coop_in_box(y0[0])
    return host(why, dev if told else None)


def multistep(func, y0, refused=''):
    """The Adams solvers: one launch (csrc/mi_ode_adams.h, mi_ode_adams_vc.h) or the per-step loop.  refused: the option that rules it out."""
    dev = getattr(func, 'device_rhs', None)
    rhs = None if refused else _single(dev, y0, multistep=True)
    if rhs is not None and getattr(rhs, 'multistep_fused', False):
        return Route('fused_multistep', rhs, 'multistep_fused: row-local systems, matrix right-hand sides and networks up to 256 wide')
    return Route('planes', None, _PYTHON[len(y0) == 1] if dev is None else refused or 'no one-launch multistep kernel for this right-hand side')


def fixed_grid(func, y0, name, *, one_launch, default_grid=True, eps=0.0, fusion=AUTO):
    """The fixed-grid Runge-Kutta solvers.  one_launch: the method has a fused kernel (euler, rk4); default_grid: the steps are on `t` itself."""
    dev = getattr(func, 'device_rhs', None)
    own_grid = not (default_grid and eps == 0.0)
    kind, rhs = 'fused', _single(dev, y0) if one_launch else None
    if rhs is None and one_launch:
        # a network outside the tile kernels' box (float64, wide): euler / rk4 on the cooperative one-launch kernel
        kind, rhs = 'fused_coop', _coop(dev, y0)
    if rhs is None and one_launch and not own_grid and getattr(_tuple(func, y0), 'fixed_grid_fused', False):
        # a tuple state of a row-local RHS: a fixed grid has no norms, so the components simply share one buffer and the one-launch kernel
        return Route('fused_tuple', dev, _TUPLE_WHY)
    if rhs is not None and rhs.fixed_grid_fused and not (own_grid and fusion == STAGE):
        return Route(kind, rhs, 'euler / rk4 have one-launch fixed-grid kernels for every fused family')
    if dev is None:
        return Route('planes', None, _PYTHON[len(y0) == 1])
    if not one_launch:
        return Route('planes', None, '%s has no fused kernel (euler / rk4 do)' % name)
    return Route('planes', None, 'a grid of its own (step_size / grid_constructor / eps) on the per-stage schedule: the grid-walking kernel '
                 'is whole-call' if rhs is not None and rhs.fixed_grid_fused else 'no fixed-grid kernel takes this state')


def not_traced(opts, mode):
    """'' when the options leave a Python callable to the tracer (lower.py), else why they do not.  mode: options['lower']."""
    if mode is False or mode == 'off':
        return "options['lower'] is False"
    asks = ('process_group', 'force_plane_kernels', 'grid_constructor')
    if any(k in opts for k in asks) or (opts.get('graph', 'auto') != 'auto' and mode is not True):
        return 'an option asks for one of the callable engines (%s)' % sorted(k for k in opts if k in asks + ('graph',))
    return ''
