"""`odeint_discrete`: the gradient of the DISCRETE map a fixed-grid solver computed - what the reference's taped solver returns.

The reference trains by back-propagating through the solver's own ops (both branches of its ODEBlock call plain `odeint` under the
caller's tape; its MNIST example uses one Euler step over [0, 1]).  On a fixed grid that is NOT what the continuous adjoint yields: with
one Euler step the tape evaluates df/dtheta at y0, the adjoint solve at y1 - O(h) apart.  `odeint_adjoint` stays what it is;
this module adds the other gradient, opt-in.

For a step  y_{n+1} = y_n + h sum_i b_i k_i,  k_i = f(t_n + c_i h, Y_i),  Y_i = y_n + h sum_{j<i} a_ij k_j  and the incoming
lambda_{n+1} = dL/dy_{n+1}, for i = s .. 1:

    kbar_i = h b_i lambda_{n+1} + h sum_{j>i} a_ji Ybar_j       Ybar_i = (df/dy at Y_i)^T kbar_i       theta_bar += (df/dtheta at Y_i)^T kbar_i

and lambda_n = lambda_{n+1} + sum_i Ybar_i + gbar_n (gbar_n: the output gradient at grid point n).  The forward solution on the default
grid holds every y_n, so the checkpoints are free and each step is recomputed from its own.

Five engines:
  * fused linear sweep - opt-in (`linear='auto'` / True, module default LINEAR): f(t, y) = y W (+ b) - models.LinearODEFunc, or a callable the
    tracer puts in the 'linear' family (`y @ W`, `y @ W + b`, torch.nn.Linear(d, d)) - float32 and float64, dim <= 128: the whole backward,
    all steps, is ONE launch on the matrix cores (csrc/mi_ode_discrete_linear.h);
  * fused row-local sweep - opt-in (`lower='auto'` / True, module default LOWER): a plain Python callable the tracer lowers to a row-local
    program (lower.py, state of up to 32 elements per trajectory) gets the vjp of its trace as generated device code, and the whole
    backward, all steps, is ONE launch with a trajectory per lane (csrc/mi_ode_discrete_row.h), float32 and float64;
  * fused mlp sweep - models.ODEFunc / rhs.MLP (relu, softplus, tanh), float32, time dependent or not, dim <= 64, hidden <= 128, any
    subset of the six parameters trainable, up to 1024 steps per segment: the whole backward, all steps, is ONE launch
    (csrc/mi_ode_discrete.h); a float64 network stays on the generic sweep unless the next engine is switched on;
  * fused mlp sweep (float64) - opt-in (`mlp64='auto'` / True, module default MLP64): the same network, box and step limit in float64, all
    six parameters in float64: the whole backward, all steps, is ONE launch on the f64 matrix cores, weights streamed from packed copies
    in both orientations (csrc/mi_ode_discrete64.h);
  * generic sweep   - any `func`, any dtype, tuple states: per step one taped re-evaluation in torch ops and one torch.autograd.grad call.

Scope: euler, midpoint, heun / huen and rk4 (the 3/8 rule) with eps == 0, on the default grid (`t` itself) and - opt-in, `own_grid=True` /
module default OWN_GRID - on the grid of options['step_size'], whose outputs the solver interpolates linearly inside the step that reaches
them (solvers.py:86-115).  There the backward recomputes the grid states from y0 (one default-grid solve, cut into segments beyond
GRID_BYTES), places the output gradients on the grid (_grid_plan) and runs the engines above; the linear system has a kernel mode that
does all of it in ONE launch without a stored trajectory ('fused linear sweep (own grid)', GRID_KERNEL).  Adaptive solves over a recorded
step sequence, the multistep family, grid_constructor and eps != 0 are not covered: they raise ValueError and name `odeint_adjoint`.

Layout: the engines that own a native handle (_FusedDiscreteEngine / ...64, _FusedLinearEngine, _FusedLinearGridEngine) share engine._SweepEngine
(create, close, the status of a sweep) and the size-4 cache rule of engine._cached, as the adjoint engines do.  `odeint_discrete` plans a call ONCE, in the order own-grid
linear kernel, linear sweep, row-local sweep, float64 mlp check - each for the trajectory length the backward will sweep - and hands the
outcome to _OdeintDiscretePlanned as one _Plans record; with every switch off it calls plain _OdeintDiscrete.
"""
import collections
import ctypes as C

import torch

from . import _native as N
from .engine import HandoffTimeout, _SweepEngine, _cached
from .fixed_grid import Euler, RK4
from .odeint import _graph_leaves, odeint
from .rk_common import _ButcherTableau

# the tableaus the forward kernels use (fixed_grid.py), plus midpoint and heun (fixed_grid.py:16-18, 28-32) written as two-stage tableaus
TABLEAUS = {
    'euler': Euler._fused_tableau,
    'midpoint': _ButcherTableau(alpha=[1 / 2], beta=[[1 / 2]], c_sol=[0., 1.], c_error=[0., 0.]),
    'heun': _ButcherTableau(alpha=[1.], beta=[[1.]], c_sol=[1 / 2, 1 / 2], c_error=[0., 0.]),
    'rk4': RK4._fused_tableau,
}
TABLEAUS['huen'] = TABLEAUS['heun']
FUSED = True                  # False: every call takes the generic sweep
CHUNK_TILES = 0               # 32-row tiles of a workgroup that share one weight-gradient pass of the fused kernel; 0: all of them,
                              # as far as 1 GiB of activation scratch goes
LOWER = False                 # default of odeint_discrete(lower=...): False - today's routes; 'auto' - the fused row-local sweep where it applies;
                              # True - raise ValueError where it does not
LINEAR = False                # default of odeint_discrete(linear=...): False - today's routes; 'auto' - the fused linear sweep where it applies; True -
                              # raise ValueError where it does not
OWN_GRID = False              # default of odeint_discrete(own_grid=...): False - options['step_size'] raises as before; True - it is accepted
GRID_BYTES = 1 << 30          # own grid: bound on the recomputed grid states plus their gradients; beyond it the grid is swept in segments
GRID_KERNEL = True            # own grid, linear system: the one-launch kernel that recomputes its checkpoints (csrc/mi_ode_discrete_linear.h,
                              # GRID = true); False: the recompute on the grid and the default-grid linear sweep
MLP64 = False                 # default of odeint_discrete(mlp64=...): False - a float64 network takes the generic sweep, as before; 'auto' - the fused
                              # float64 mlp sweep where it applies; True - raise ValueError where it does not
ROW_GRID = 0                  # workgroups of the fused row-local sweep; 0: one per 256 trajectories, up to 1024
_ENGINES = {}
_ENGINES64 = {}
_LINEAR_ENGINES = {}


def check_supported(method, options=None, t=None, own_grid=False):
    """ValueError for everything outside the scope of the discrete gradient, naming the reason and the alternative.  own_grid: True
    accepts options['step_size']."""
    alt = '; use odeint_adjoint (the continuous adjoint) for this call'
    if method not in TABLEAUS:
        raise ValueError('odeint_discrete: method %r is not a fixed-grid Runge-Kutta method (%s): adaptive and multistep solves have no '
                         'fixed discrete map to transpose here%s' % (method, ', '.join(sorted(TABLEAUS)), alt))
    opts = options or {}
    for key in ('step_size', 'grid_constructor'):
        if opts.get(key) is not None and not (own_grid and key == 'step_size'):
            raise ValueError('odeint_discrete: options[%r] gives the solver a grid of its own and the outputs are interpolated; only the '
                             'default grid (`t` itself) is covered%s' % (key, alt))
    if float(opts.get('eps', 0.0) or 0.0) != 0.0:
        raise ValueError("odeint_discrete: options['eps'] != 0 shifts the evaluation times off the default grid; only eps == 0 is covered" + alt)
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise ValueError('odeint_discrete: `t` requires grad, and the discrete gradient is taken with respect to y0 and the parameters only' + alt)


def taped_step(func, tableau, t0, h, y):
    """One step of the tableau in plain torch ops (autograd sees every one): y is a tuple, func maps (t, tuple) -> tuple; t0, h are 0-d
    tensors in the state dtype.  The solvers' own step_func runs untaped plane kernels, hence this restatement for the backward."""
    ks = [func(t0, y)]
    for alpha_i, beta_i in zip(tableau.alpha, tableau.beta):
        yi = tuple(y_ + sum((h * float(b)) * k[c] for b, k in zip(beta_i, ks) if b != 0.0) for c, y_ in enumerate(y))
        ks.append(func(t0 + float(alpha_i) * h, yi))
    return tuple(y_ + sum((h * float(b)) * k[c] for b, k in zip(tableau.c_sol, ks) if b != 0.0) for c, y_ in enumerate(y))


GridPlan = collections.namedtuple('GridPlan', 'grid out_step out_w')


def _grid_plan(t, step_size, dtype):
    """Where a solve with options['step_size'] put its outputs: GridPlan(grid, out_step, out_w).  grid: the solver's own grid, [M + 1] in
    the state dtype (FixedGridODESolver._grid_constructor_from_step_size on `t` in that dtype); out_step[j]: the grid step n_j whose end
    is the first t1 >= t[j] (solvers.py:93-100; out_step[0] = -1: output 0 is y0); out_w[j] = (t[j] - t0) / (t1 - t0), formed in the state
    dtype, exactly 1 where t[j] == t1 (_linear_interp returns y1 itself) and for j = 0.  The output gradients map onto the grid as
    gbar[n_j + 1] += w_j g_j and gbar[n_j] += (1 - w_j) g_j, the latter only when w_j != 1."""
    from .solvers import FixedGridODESolver
    tt = torch.as_tensor(t).detach().cpu().to(dtype)
    grid = FixedGridODESolver._grid_constructor_from_step_size(None, step_size)(None, None, tt)
    if not (bool(grid[0] == tt[0]) and bool(grid[-1] == tt[-1])):                         # solvers.py:87
        raise ValueError('odeint_discrete: the grid of step_size %r does not span t' % (step_size,))
    out_step, out_w = [-1], [torch.ones((), dtype=dtype)]
    j, n_out = 1, int(tt.shape[0])
    for n in range(int(grid.shape[0]) - 1):
        t0, t1 = grid[n], grid[n + 1]
        while j < n_out and bool(t1 >= tt[j]):
            out_step.append(n)
            out_w.append(torch.ones((), dtype=dtype) if bool(tt[j] == t1) else (tt[j] - t0) / (t1 - t0))
            j += 1
    assert j == n_out, 'the grid ends at t[-1]: every output lies inside a step'
    return GridPlan(grid, out_step, torch.stack(out_w))


def _segments(n_steps, point_bytes):
    """[0, K, 2 K, .., n_steps]: the grid cut so that K + 1 states and as many gradients fit GRID_BYTES (at most 1024 steps each: the
    fused sweeps take no more).  One segment is the common case."""
    k = max(1, min(int(n_steps), int(GRID_BYTES) // max(2 * int(point_bytes), 1) - 1, N.DISCRETE_MAX_STEPS))
    return list(range(0, int(n_steps), k)) + [int(n_steps)]


def _segment_points(bounds):
    """The distinct numbers of grid points of the segments of _segments(), the first segment's first."""
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a + 1 not in out:
            out.append(b - a + 1)
    return tuple(out)


def generic_sweep(func, params, ys, t, grad_ys, method):
    """The reverse sweep in torch ops, device-agnostic.  func: (t, tuple) -> tuple; params: the tensors to differentiate with respect to;
    ys / grad_ys: tuples of [N, ...] tensors (the forward solution and the gradient of the loss with respect to it); t: the N grid times.
    Returns (tuple of gradients at y0, list of parameter gradients - None where no step reached the tensor)."""
    tableau = TABLEAUS[method]
    like = ys[0]
    n_pts = like.shape[0]
    tt = torch.as_tensor(t).detach().to(device=like.device, dtype=like.dtype)
    params = tuple(params)
    lam = tuple(g[n_pts - 1] for g in grad_ys)
    gp = [None] * len(params)
    for n in range(n_pts - 2, -1, -1):
        with torch.enable_grad():
            y = tuple(c[n].detach().requires_grad_(True) for c in ys)
            y1 = taped_step(func, tableau, tt[n], tt[n + 1] - tt[n], y)
            grads = torch.autograd.grad(y1, y + params, lam, allow_unused=True)
        lam = tuple((l_ if g is None else g) + gy[n] for g, l_, gy in zip(grads[:len(y)], lam, grad_ys))
        for i, g in enumerate(grads[len(y):]):
            if g is not None:
                gp[i] = g if gp[i] is None else gp[i] + g
    return lam, gp


class _FusedDiscreteEngine(_SweepEngine):
    """Owns one mi_ode_discrete handle: the reverse sweep of `n_points - 1` steps of `method` for a [batch, dim] state in `dtype` and the
    dim -> hidden -> hidden -> dim MLP (time_dependent: (1 + dim) -> hidden, the first layer sees concat([t, x])), one launch."""
    dtype = torch.float32
    _create, _destroy, _num_params, _sweep = 'mi_ode_discrete_create_td', 'mi_ode_discrete_destroy', 'mi_ode_discrete_num_params', 'mi_ode_discrete_sweep'

    def __init__(self, batch, dim, hidden, method, n_points, device, chunk_tiles=0, time_dependent=False):
        d = N.DiscreteDesc()
        d.batch, d.dim, d.hidden = int(batch), int(dim), int(hidden)
        d.n_points, d.chunk_tiles = int(n_points), int(chunk_tiles)
        self._open(device, d, TABLEAUS[method], None, 1 if time_dependent else 0)
        self.batch, self.dim, self.n_points, self.time_dependent = int(batch), int(dim), int(n_points), bool(time_dependent)
        self.n_params = int(getattr(self.lib, self._num_params)(self.h))

    def sweep(self, mlp, t, ys, grad_ys):
        """(grad_y0 [batch, dim], grad_theta [P] in canonical order) from the forward solution and its gradient, both [N, batch, dim]."""
        r = N.Rhs()
        keep = mlp.fill(r, self.dtype, self.device)          # (the tensors the descriptor points into live to the end of the call)
        ys, grad_ys = ys.contiguous(), grad_ys.contiguous()
        g_y0 = torch.empty(self.batch, self.dim, dtype=self.dtype, device=self.device)
        g_th = torch.empty(self.n_params, dtype=self.dtype, device=self.device)
        tt = (C.c_double * self.n_points)(*[float(v) for v in t])
        out = self._run(self._sweep, (C.byref(r), tt, ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_th.data_ptr()), (g_y0, g_th))
        del keep
        return out


def _cached_engine(batch, dim, hidden, method, n_points, device, chunk_tiles=0, time_dependent=False):
    """The float32 MLP engine (shape first in the key, the chunk last).  Eviction closes: the plan is formed in backward, around its sweep."""
    key = (batch, dim, hidden, method, n_points, device, bool(time_dependent), chunk_tiles)
    return _cached(_ENGINES, key, lambda: _FusedDiscreteEngine(batch, dim, hidden, method, n_points, device, chunk_tiles, time_dependent), True)


class _FusedDiscreteEngine64(_FusedDiscreteEngine):
    """Owns one mi_ode_discrete64 handle: _FusedDiscreteEngine for a float64 state and float64 parameters (csrc/mi_ode_discrete64.h)."""
    dtype = torch.float64
    _create, _destroy, _num_params, _sweep = ('mi_ode_discrete64_create', 'mi_ode_discrete64_destroy', 'mi_ode_discrete64_num_params',
                                              'mi_ode_discrete64_sweep')

    def profile(self):
        """Where the time of the last sweep went, microseconds of workgroup 0: (tile passes, weight-gradient passes, hand-off + fold)."""
        out = (C.c_double * 3)()
        N.check(self.lib.mi_ode_discrete64_profile(self.h, out), 'mi_ode_discrete64_profile')
        return tuple(float(v) for v in out)


def _cached_engine64(batch, dim, hidden, method, n_points, device, chunk_tiles=0, time_dependent=False):
    """_cached_engine for the float64 kernel: a cache of its own, the dtype in the key."""
    key = (batch, dim, hidden, method, n_points, device, 'float64', bool(time_dependent), chunk_tiles)
    return _cached(_ENGINES64, key, lambda: _FusedDiscreteEngine64(batch, dim, hidden, method, n_points, device, chunk_tiles, time_dependent), True)


def clear_engines():
    """Empties the engine caches.  The MLP engines (float32 and float64) are closed here.  A linear engine is only dropped: a call that has run forward and not
    yet backward still holds it, so its device memory is released when the last such graph is gone, which need not be now."""
    while _ENGINES:
        _ENGINES.pop(next(iter(_ENGINES))).close()
    while _ENGINES64:
        _ENGINES64.pop(next(iter(_ENGINES64))).close()
    _LINEAR_ENGINES.clear()                              # (dropped, not closed: see _cached_linear_engine)


def _fused_plan(func, params, method, tensor_input, like, mlp64=False):
    """((engine, descriptor), '') when the fused kernel takes this backward, else (None, why not) - in the style of odeint.plan.
    mlp64: anything but False lets a float64 state take the float64 kernel (the engine then has dtype torch.float64)."""
    if not FUSED:
        return None, 'discrete.FUSED is False'
    if not tensor_input:
        return None, 'a tuple state'
    if not like.is_cuda:
        return None, 'a host tensor'
    if like.dtype != torch.float32 and (mlp64 is False or mlp64 is None):
        return None, 'dtype %s (the fused sweep is float32)' % str(like.dtype).replace('torch.', '')
    if like.dtype not in (torch.float32, torch.float64):
        return None, 'dtype %s (the fused sweeps are float32 and float64)' % str(like.dtype).replace('torch.', '')
    get = getattr(func, 'device_rhs', None)
    try:
        layers = (func.fc1, func.fc2, func.fc3)
    except AttributeError:
        get = None
    if not callable(get):
        return None, '%s is not a models.ODEFunc (no fused-MLP descriptor)' % type(func).__name__
    mlp = get()
    if mlp is None or getattr(mlp, 'kind', None) != N.RHS_MLP_TANH:
        return None, 'the activation has no fused MLP kernel (relu, softplus, tanh do)'
    y1 = like[0]
    if y1.dim() < 2 or not mlp.supports(y1):
        return None, 'outside the tile box of rhs.MLP.supports (dim <= %d, hidden <= %d, state [batch, dim])' % (mlp.MAX_DIM, mlp.MAX_HIDDEN)
    want = [p for l in layers for p in (l.weight, l.bias)]
    # any duplicate-free subset of the six, by identity: the kernel computes all six gradients, the call returns those it asked for
    if any(a is b for i, a in enumerate(want) for b in want[:i]):
        return None, 'tied parameters (two of the six slots of the network hold the same tensor: its gradient is the sum of two of the kernel\'s)'
    if any(a is b for i, a in enumerate(params) for b in params[:i]):
        return None, 'a tensor listed twice among the parameters'
    if any(not any(p is w_ for w_ in want) for p in params):
        return None, 'frozen or extra parameters (the kernel produces the gradients of the six tensors of the network, or of a subset of them)'
    if any(p.dtype != like.dtype or p.device != like.device for p in want):
        return None, 'parameters in another dtype or on another device than the state'
    n_points = int(like.shape[0])
    if n_points - 1 > 1024:
        return None, 'more than 1024 steps'
    batch = y1.numel() // y1.shape[-1]
    try:
        cached = _cached_engine64 if like.dtype == torch.float64 else _cached_engine
        eng = cached(batch, int(y1.shape[-1]), int(mlp.hidden), 'heun' if method == 'huen' else method, n_points, str(like.device), int(CHUNK_TILES),
                     bool(mlp.time_dependent))
    except N.NativeError as e:                           # e.g. no memory for the activation scratch
        return None, 'the fused engine could not be created (%s)' % e
    return (eng, mlp), ''


def _linear_io(eng, W, b):
    """What a sweep of f(y) = y W (+ b) on `eng` passes and returns: (the descriptor, the contiguous W and b it points into, (g_y0
    [batch, dim], g_w [dim, dim] in W's [in, out] layout, g_b [dim] or None)).  W, b: device tensors in the state dtype, read now."""
    r = N.Rhs()
    r.kind, r.sign, r.hidden = N.RHS_LINEAR, 1.0, 0
    W = W.contiguous()
    r.w[0] = W.data_ptr()
    if b is not None:
        b = b.contiguous()
        r.b[0] = b.data_ptr()
    g_y0 = torch.empty(eng.batch, eng.dim, dtype=eng.dtype, device=eng.device)
    g_w = torch.empty(eng.dim, eng.dim, dtype=eng.dtype, device=eng.device)
    g_b = torch.empty(eng.dim, dtype=eng.dtype, device=eng.device) if b is not None else None
    return r, (W, b), (g_y0, g_w, g_b)


class _FusedLinearEngine(_SweepEngine):
    """Owns one mi_ode_discrete_linear handle: the reverse sweep of `n_points - 1` steps of `method` for a [batch, dim] state and
    f(y) = y W (+ b), one launch."""
    _create, _destroy = 'mi_ode_discrete_linear_create', 'mi_ode_discrete_linear_destroy'

    def __init__(self, batch, dim, has_bias, method, n_points, device, dtype):
        self.dtype = dtype
        d = N.DiscreteLinearDesc()
        d.dtype, d.dim, d.batch, d.has_bias, d.n_points = N.dtype_code(dtype), int(dim), int(batch), int(bool(has_bias)), int(n_points)
        self._open(device, d, TABLEAUS[method], None)
        self.batch, self.dim, self.n_points, self.has_bias = int(batch), int(dim), int(n_points), bool(has_bias)

    def profile(self):
        """{'grid', 'sweep_us', 'store_us', 'fold_us'} of the last sweep: workgroup 0's clock over the tile sweep (all steps, the weight-gradient
        products included), the store of its partial block, the final hand-off and fold."""
        out = (C.c_double * 3)()
        g = self.lib.mi_ode_discrete_linear_profile(self.h, out)
        return {'grid': int(g), 'sweep_us': out[0], 'store_us': out[1], 'fold_us': out[2]}

    def sweep(self, W, b, t, ys, grad_ys):
        """(grad_y0 [batch, dim], grad_W [dim, dim] in W's [in, out] layout, grad_b [dim] or None) from the forward solution and its
        gradient, both [N, batch, dim].  W, b: device tensors in the state dtype, read now (nothing is cached between calls)."""
        r, _keep, (g_y0, g_w, g_b) = _linear_io(self, W, b)
        ys, grad_ys = ys.contiguous(), grad_ys.contiguous()
        tt = (C.c_double * self.n_points)(*[float(v) for v in t])
        return self._run('mi_ode_discrete_linear_sweep', (C.byref(r), tt, ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_w.data_ptr(),
                                                          None if g_b is None else g_b.data_ptr()), (g_y0, g_w, g_b))


def _cached_linear_engine(*key):
    """The engine of `key`, four cached at most.  The plan of a call holds its engine from the call to its backward, so eviction (and
    clear_engines) only drops the cache's reference: the handle is destroyed when the last pending plan lets go of it (__del__)."""
    return _cached(_LINEAR_ENGINES, key, lambda: _FusedLinearEngine(*key), False)


class _FusedLinearGridEngine(_SweepEngine):
    """Owns one mi_ode_discrete_linear_grid handle: the reverse sweep of `n_steps` grid steps of `method` with `n_out` interpolated outputs
    for a [batch, dim] state and f(y) = y W (+ b) - checkpoints recomputed from y0 into the handle's scratch, one launch."""
    _create, _destroy = 'mi_ode_discrete_linear_grid_create', 'mi_ode_discrete_linear_grid_destroy'

    def __init__(self, batch, dim, has_bias, method, n_steps, n_out, device, dtype):
        self.dtype = dtype
        d = N.DiscreteLinearGridDesc()
        d.dtype, d.dim, d.batch, d.has_bias = N.dtype_code(dtype), int(dim), int(batch), int(bool(has_bias))
        d.n_steps, d.n_out = int(n_steps), int(n_out)
        self._open(device, d, TABLEAUS[method], None)
        self.batch, self.dim, self.n_steps, self.n_out, self.has_bias = int(batch), int(dim), int(n_steps), int(n_out), bool(has_bias)

    def profile(self):
        """_FusedLinearEngine.profile() plus 'scratch_bytes': the checkpoint scratch the handle owns (grid x n_steps x 16 x D elements)."""
        out, nbytes = (C.c_double * 3)(), C.c_int64()
        g = self.lib.mi_ode_discrete_linear_grid_profile(self.h, out, C.byref(nbytes))
        return {'grid': int(g), 'sweep_us': out[0], 'store_us': out[1], 'fold_us': out[2], 'scratch_bytes': int(nbytes.value)}

    def sweep(self, W, b, gplan, y0, grad_out):
        """(grad_y0 [batch, dim], grad_W [dim, dim] in W's [in, out] layout, grad_b [dim] or None) from y0 [batch, dim] and the gradient of
        the loss with respect to the n_out outputs [n_out, batch, dim]; gplan: the GridPlan of the call."""
        r, _keep, (g_y0, g_w, g_b) = _linear_io(self, W, b)
        y0, grad_out = y0.contiguous(), grad_out.contiguous()
        grid = (C.c_double * (self.n_steps + 1))(*[float(v) for v in gplan.grid])
        step = (C.c_int32 * self.n_out)(*[int(v) for v in gplan.out_step])
        w = (C.c_double * self.n_out)(*[float(v) for v in gplan.out_w])
        return self._run('mi_ode_discrete_linear_grid_sweep', (C.byref(r), grid, step, w, y0.data_ptr(), grad_out.data_ptr(), g_y0.data_ptr(),
                                                               g_w.data_ptr(), None if g_b is None else g_b.data_ptr()), (g_y0, g_w, g_b))


def _cached_linear_grid_engine(*key):
    """_cached_linear_engine for the own-grid kernel: the same cache (and the same rule: eviction only drops the cache's reference), the
    key carries (n_steps, n_out)."""
    return _cached(_LINEAR_ENGINES, ('own grid',) + key, lambda: _FusedLinearGridEngine(*key), False)


def _on_device(x):
    return x.is_cuda


class _LinearPlan(object):
    """What the fused linear sweep of ONE call needs: the parameters themselves (read at the backward, so an in-place optimizer step is
    seen), how the matrix is laid out ('W': [in, out] as the kernel reads it; 'Wt': [out, in], torch.nn.Linear's), where their gradients
    go among the call's parameters, and the engine.  others: {n_points: engine} for the segments of an own-grid recompute whose length is
    not the first one's (the shorter last segment) - created at the call with the plan's own, and held by the plan like it."""

    def __init__(self, W, b, how, slots, engine, key=None, others=None):
        self.W, self.b, self.how, self.slots, self.engine, self.key, self.others = W, b, how, slots, engine, key, others or {}

    def _engine_for(self, n_points):
        """The engine of a trajectory of n_points: the plan's own, or the one planned at the call for that length.  (A length nobody
        planned - a caller of its own - is looked up in the cache, which may create it here.)"""
        if self.key is None or getattr(self.engine, 'n_points', n_points) == n_points:
            return self.engine
        if n_points not in self.others:
            self.others[n_points] = _cached_linear_engine(*(self.key[:4] + (int(n_points),) + self.key[5:]))
        return self.others[n_points]

    def sweep(self, t, ys, grad_ys, n_params):
        dim = int(ys.shape[-1])
        W = self.W.detach()
        self.used = self._engine_for(int(ys.shape[0]))       # (whose stats describe this sweep)
        g_y0, g_w, g_b = self.used.sweep(W if self.how == 'W' else W.t().contiguous(), None if self.b is None else self.b.detach().reshape(-1),
                                         t, ys.reshape(ys.shape[0], -1, dim), grad_ys.reshape(ys.shape[0], -1, dim))
        return g_y0, self._place(g_w, g_b, n_params)

    def sweep_grid(self, gplan, y0, grad_out, n_params):
        """The own-grid kernel (the plan's engine is a _FusedLinearGridEngine): y0 [..., dim], grad_out [n_out, ..., dim]."""
        dim = int(y0.shape[-1])
        W = self.W.detach()
        g_y0, g_w, g_b = self.engine.sweep(W if self.how == 'W' else W.t().contiguous(), None if self.b is None else self.b.detach().reshape(-1),
                                           gplan, y0.reshape(-1, dim), grad_out.reshape(grad_out.shape[0], -1, dim))
        return g_y0, self._place(g_w, g_b, n_params)

    def _place(self, g_w, g_b, n_params):
        gp = [None] * n_params
        gp[self.slots[0]] = (g_w if self.how == 'W' else g_w.t().contiguous()).reshape(self.W.shape)
        if self.b is not None:
            gp[self.slots[1]] = g_b.reshape(self.b.shape)
        return gp


def _state_refusal(y0, method, what):
    """Why `what` does not take a state like y0 under `method`, or ''."""
    if not isinstance(y0, torch.Tensor):
        return 'a tuple state (the %s takes one state tensor)' % what
    if y0.dtype not in (torch.float32, torch.float64):
        return 'dtype %s (the %s is float32 / float64)' % (str(y0.dtype).replace('torch.', ''), what)
    if method not in TABLEAUS:
        return 'method %r' % (method,)
    return ''


def _trace_kind(func, y0, method, accepted):
    """((trace, family, info), '') of the Python callable `func` on y0 - traced (or found in the trace cache) and classified - else
    (None, why not).  accepted: what the caller takes, for the refusal of a device descriptor."""
    from . import lower as L
    if getattr(func, 'kind', 0) or getattr(func, 'stage_rhs', None) is not None or not callable(func):
        return None, 'a device right-hand side descriptor, not %s' % accepted
    try:
        if isinstance(func, L.CompiledCallable):
            tr = func._trace_for(y0, method)
        else:
            tr, _hit = L._cached_trace(func, y0, None) if L.TRACE_CACHE else (None, False)
            if tr is None:
                tr = L.trace(func, y0)
        rows = 1
        for s_ in tr.batch_shape:
            rows *= int(s_)
        kind, info = L.classify(tr, rows=rows)
    except L.TraceError as e:
        return None, 'the callable cannot be lowered: %s' % e
    except Exception as e:                               # the callable itself failed on the proxies
        return None, 'tracing failed: %s: %s' % (type(e).__name__, e)
    return (tr, kind, info), ''


def _linear_plan(func, params, method, y0, like=None, n_points=None, own_grid=None):
    """(_LinearPlan, '') when the fused linear sweep takes this call, else (None, why not).  like: the solution (or any tensor of its
    shape [N, ...]); without one, n_points is the number of grid points - or a tuple of them, the distinct segment lengths of an own-grid
    recompute: the plan's engine is the first one's, the others' are created with it.  own_grid: (n_steps, n_out) of a solve on a grid
    of its own - the plan then holds the own-grid kernel's engine (the same conditions, n_steps <= 1024 in place of the limit on the
    points of `t`).  Creates (or finds) every engine - at the call, not in backward."""
    from . import models as M
    why = _state_refusal(y0, method, 'fused linear sweep')
    if why:
        return None, why
    if y0.dim() < 1:
        return None, 'a 0-d state'
    dim = int(y0.shape[-1])
    if isinstance(func, M.LinearODEFunc):
        if dim != func.dim:
            return None, 'the state\'s last axis is %d, the module\'s dim %d' % (dim, func.dim)
        W, b, how = func.weight, func.bias, 'W'
    else:
        nfe = getattr(func, 'nfe', None)                 # (tracing runs a module's forward on proxies: not an evaluation the caller counts)
        traced, why = _trace_kind(func, y0, method, 'a models.LinearODEFunc or a Python callable')
        if isinstance(nfe, int) and getattr(func, 'nfe', nfe) != nfe:
            func.nfe = nfe
        if traced is None:
            return None, why
        tr, kind, info = traced
        if kind != 'linear':
            return None, 'the callable lowers to the %r family, not to y @ W (+ b)' % kind
        how, widx = info['W']
        ents = [tr.tensors[widx]] + ([] if info.get('b') is None else [tr.tensors[info['b']]])
        for e in ents:
            x = e['t']
            if not x.is_leaf:
                return None, 'a derived (non-leaf) tensor of shape %s enters the product (W.t(), tanh(W), a slice): the kernel differentiates ' \
                             'with respect to the matrix and the bias the trace reads' % (list(x.shape),)
            if e['lead'] != 0:
                return None, 'a constant of shape %s with batch axes (every trajectory would need its own copy of the gradient)' % (list(x.shape),)
        W = ents[0]['t']
        b = ents[1]['t'] if len(ents) > 1 else None
    if dim > N.DISCRETE_LINEAR_MAX_DIM:
        return None, 'dim %d > %d (dims 129 .. 256 are forward-only on the streamed kernels)' % (dim, N.DISCRETE_LINEAR_MAX_DIM)
    if own_grid is not None:
        n_steps, n_out = (int(v) for v in own_grid)
        if n_steps > N.DISCRETE_MAX_STEPS:
            return None, 'more than %d grid steps (%d)' % (N.DISCRETE_MAX_STEPS, n_steps)
        if n_out > N.DISCRETE_MAX_STEPS + 1:
            return None, 'more than %d outputs (%d)' % (N.DISCRETE_MAX_STEPS + 1, n_out)
    else:
        lengths = tuple(n_points) if isinstance(n_points, (tuple, list)) else (n_points,)
        more = tuple(int(v) for v in lengths[1:])
        n_points = int(like.shape[0]) if like is not None else int(lengths[0])
        if n_points - 1 > N.DISCRETE_MAX_STEPS:
            return None, 'more than %d steps (%d)' % (N.DISCRETE_MAX_STEPS, n_points - 1)
    want = [W] + ([] if b is None else [b])
    slots = [next((j for j, p_ in enumerate(params) if p_ is w_), None) for w_ in want]
    if len(params) != len(want) or any(j is None for j in slots):
        return None, 'frozen or extra parameters (the kernel produces the gradients of exactly the matrix%s)' % ('' if b is None else ' and the bias')
    if any(p_.dtype != y0.dtype or p_.device != y0.device for p_ in want):
        return None, 'parameters in another dtype or on another device than the state'
    if not _on_device(y0):
        return None, 'a host tensor'
    batch = y0.numel() // dim
    others = {}
    try:
        if own_grid is not None:
            key = (batch, dim, b is not None, 'heun' if method == 'huen' else method, n_steps, n_out, str(y0.device), y0.dtype)
            eng = _cached_linear_grid_engine(*key)
        else:
            key = (batch, dim, b is not None, 'heun' if method == 'huen' else method, n_points, str(y0.device), y0.dtype)
            eng = _cached_linear_engine(*key)
            for n_ in more:
                if n_ != n_points:
                    others[n_] = _cached_linear_engine(*(key[:4] + (n_,) + key[5:]))
    except N.NativeError as e:
        return None, 'the fused engine could not be created (%s)' % e
    return _LinearPlan(W, b, how, slots, eng, key, others), ''


class _RowPlan(object):
    """What the fused row-local sweep of ONE call needs: the discrete plugin's table, the trace's parameter layout and a copy of the
    constants the forward call was bound with (the program's pool buffer is shared: the next odeint of the same program overwrites it)."""

    def __init__(self, lib, table, tr, targets, n_params, pool, scalars):
        self.lib, self.table, self.trace, self.targets, self.n_params, self.pool, self.scalars = lib, table, tr, targets, n_params, pool, scalars
        self.dim = 1
        for s_ in tr.tail:
            self.dim *= int(s_)


def _row_plan(func, params, method, y0, build=True, per_row_t=False):
    """(_RowPlan, '') when the fused row-local sweep takes this call, else (None, why not).  Traces, classifies, generates the vjp and
    builds the plugin - at the call, not in backward.  per_row_t: the discrete-t plugin (per-row times and lengths, _row_sweep_t)."""
    from . import lower as L
    why = _state_refusal(y0, method, 'fused row-local sweep')
    if why:
        return None, why
    traced, why = _trace_kind(func, y0, method, 'a Python callable')     # (func.nfe is left as the trace moved it - _linear_plan restores it)
    if traced is None:
        return None, why
    tr, kind, _info = traced
    if kind != 'rowlocal':
        return None, 'the callable lowers to the %r family, which has no generated vjp (row-local programs do)' % kind
    plist, n_params = L.vjp_params(tr)
    targets = []
    for idx, off, n in plist:
        e = tr.tensors[idx]
        x = e['t']
        if not x.is_leaf:
            return None, 'a derived (non-leaf) trainable tensor of shape %s enters the callable (W.t(), a slice, a product): the kernel ' \
                         'differentiates with respect to the tensors the trace reads' % (list(x.shape),)
        if e['lead'] != 0:
            return None, 'a trainable constant of shape %s with batch axes (every trajectory would need its own copy of the gradient)' % (list(x.shape),)
        k = [j for j, p_ in enumerate(params) if p_ is x]
        if not k:
            return None, 'the trace reads a trainable tensor of shape %s that the parameter search did not find' % (list(x.shape),)
        targets.append((k[0], off, n))
    for req in tr.tensors:
        if req['t'].requires_grad and not req['t'].dtype.is_floating_point:
            return None, 'a trainable tensor of dtype %s' % req['t'].dtype
    missing = [p_ for j, p_ in enumerate(params) if all(k != j for k, _o, _n in targets)]
    if missing:
        return None, 'a trainable tensor of shape %s does not enter the trace as it is (it is used through a derived tensor, or not at all)' \
                     % (list(missing[0].shape),)
    if n_params > N.DISCRETE_ROW_MAX_PARAMS:
        return None, '%d trainable elements (the kernel keeps up to %d per wavefront in LDS)' % (n_params, N.DISCRETE_ROW_MAX_PARAMS)
    try:
        source = L.discrete_source(tr)
    except L.TraceError as e:
        return None, str(e)
    if not y0.is_cuda:
        return None, 'a host tensor'
    if not build:
        return source, ''
    from . import rhs as R
    try:
        lib, table = R.discrete_t_plugin(R.discrete_t_source_of(source), y0.dtype) if per_row_t else R.discrete_plugin(source, y0.dtype)
    except N.NativeError as e:
        return None, 'the generated vjp did not compile (%s)' % str(e).split(';')[0]
    prog = L.program_for(tr)
    bound = prog.bind(tr, y0.device)
    pool = None if bound.pool is None else bound.pool.clone()
    return _RowPlan(lib, table, tr, targets, n_params, pool, list(bound.params)), ''


def _row_sweep(plan, method, t, ys, grad_ys):
    """(grad_y0 [batch, dim], grad_theta [P] in the trace's compact order, n_launches) - ys / grad_ys: [N, batch, dim], contiguous."""
    from .solvers import _fill_tableau
    n_pts, batch, dim = (int(v) for v in ys.shape)
    dev, dtype = ys.device, ys.dtype
    groups = (batch + N.DISCRETE_ROW_THREADS - 1) // N.DISCRETE_ROW_THREADS
    grid = min(groups, N.DISCRETE_ROW_MAX_GRID)
    if int(ROW_GRID) > 0:
        grid = max(1, min(int(ROW_GRID), grid))
    P = plan.n_params
    d = N.DiscreteRowDesc()
    d.dtype, d.n_points, d.batch, d.dim, d.n_params, d.grid = N.dtype_code(dtype), n_pts, batch, dim, P, grid
    _fill_tableau(d.tableau, TABLEAUS[method], None)
    t_dev = torch.as_tensor(t).detach().to(dtype).to(device=dev, dtype=torch.float64).contiguous()
    words = grid * max(P, 1)
    work = torch.zeros(words + 2, dtype=dtype, device=dev)   # [grid, P] partials, then the ticket word (zeroed)
    d.t_dev, d.partials_dev, d.ticket_dev = t_dev.data_ptr(), work.data_ptr(), work.data_ptr() + words * work.element_size()
    r = N.Rhs()
    r.kind, r.sign, r.plugin = N.RHS_PLUGIN, 1.0, plan.table
    for i, v in enumerate(plan.scalars[:8]):
        r.scalars[i] = v
    if plan.pool is not None:
        r.w[0] = plan.pool.data_ptr()
    g_y0 = torch.empty(batch, dim, dtype=dtype, device=dev)
    g_th = torch.empty(max(P, 1), dtype=dtype, device=dev)
    stats = N.Stats()
    with torch.cuda.device(dev):
        N.check(N.load().mi_ode_discrete_row_sweep(C.byref(d), C.byref(r), ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_th.data_ptr(),
                                                          C.byref(stats), N.stream_ptr(dev)), 'mi_ode_discrete_row_sweep')
    del t_dev, work
    return g_y0, g_th, int(stats.n_launches)


def _row_sweep_t(plan, method, t_rows, lengths, ys, grad_ys):
    """_row_sweep over per-row times: t_rows [batch, T] float64 on the device (values rounded to the state dtype, read as given), lengths
    [batch] int32 there or None - ys / grad_ys: [T, batch, dim], contiguous.  One launch (csrc/mi_ode_discrete_row_t.h)."""
    from .solvers import _fill_tableau
    n_pts, batch, dim = (int(v) for v in ys.shape)
    dev, dtype = ys.device, ys.dtype
    groups = (batch + N.DISCRETE_ROW_THREADS - 1) // N.DISCRETE_ROW_THREADS
    grid = min(groups, N.DISCRETE_ROW_MAX_GRID)
    if int(ROW_GRID) > 0:
        grid = max(1, min(int(ROW_GRID), grid))
    P = plan.n_params
    if tuple(t_rows.shape) != (batch, n_pts) or t_rows.dtype != torch.float64 or not t_rows.is_contiguous() or t_rows.device != dev:
        raise ValueError('odeint_discrete: per-row times must be a contiguous float64 [batch, T] tensor on the state\'s device')
    if lengths is not None and (tuple(lengths.shape) != (batch,) or lengths.dtype != torch.int32 or not lengths.is_contiguous() or lengths.device != dev):
        raise ValueError('odeint_discrete: per-row lengths must be a contiguous int32 [batch] tensor on the state\'s device')
    d = N.DiscreteRowTDesc()
    d.dtype, d.n_times, d.batch, d.dim, d.n_params, d.grid = N.dtype_code(dtype), n_pts, batch, dim, P, grid
    _fill_tableau(d.tableau, TABLEAUS[method], None)
    words = grid * max(P, 1)
    work = torch.zeros(words + 2, dtype=dtype, device=dev)   # [grid, P] partials, then the ticket word (zeroed)
    d.t_dev, d.len_dev = t_rows.data_ptr(), (lengths.data_ptr() if lengths is not None else None)
    d.partials_dev, d.ticket_dev = work.data_ptr(), work.data_ptr() + words * work.element_size()
    r = N.Rhs()
    r.kind, r.sign, r.plugin = N.RHS_PLUGIN, 1.0, plan.table
    for i, v in enumerate(plan.scalars[:8]):
        r.scalars[i] = v
    if plan.pool is not None:
        r.w[0] = plan.pool.data_ptr()
    g_y0 = torch.empty(batch, dim, dtype=dtype, device=dev)
    g_th = torch.empty(max(P, 1), dtype=dtype, device=dev)
    stats = N.Stats()
    with torch.cuda.device(dev):
        N.check(N.load().mi_ode_discrete_row_sweep_t(C.byref(d), C.byref(r), ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_th.data_ptr(),
                                                     C.byref(stats), N.stream_ptr(dev)), 'mi_ode_discrete_row_sweep_t')
    del work
    return g_y0, g_th, int(stats.n_launches)


class _OdeintDiscreteRowsT(torch.autograd.Function):
    """odeint_discrete with a 2-D `t`: the forward is the fixed_rows.py solve, the backward the one-launch sweep over per-row times."""

    @staticmethod
    def forward(ctx, func, fwd, method, options, t, plan, prepared, n_steps, n_params, *args):
        from . import fixed_rows
        params, y0 = args[:n_params], args[n_params]
        ctx.method, ctx.params, ctx.plan, ctx.n_steps = method, params, plan, n_steps
        rt = prepared[1]
        with torch.no_grad():                            # (the target and the times of the call's planning: nothing is validated twice)
            ans = fixed_rows.solve(fwd, y0, t, method, options, prepared=prepared)
        ctx.forward_stats = dict(odeint.last_stats) if isinstance(odeint.last_stats, dict) else {}
        ctx.t_rows = (-rt.t if rt.decreasing else rt.t).contiguous()      # (read as given: h < 0 for decreasing rows)
        ctx.lengths = rt.lengths
        ctx.save_for_backward(ans)
        return ans

    @staticmethod
    def backward(ctx, grad_output):
        ans, = ctx.saved_tensors
        plan, params = ctx.plan, ctx.params
        with torch.no_grad():
            g_y0, theta, n_launches = _row_sweep_t(plan, ctx.method, ctx.t_rows, ctx.lengths, ans.contiguous(), grad_output.contiguous())
            gp = [None] * len(params)
            for k, off, n in plan.targets:
                gp[k] = theta[off:off + n].reshape(params[k].shape).to(params[k].dtype)
        odeint_discrete.last_backward_stats = {'engine': 'fused row-local sweep (per-row times)', 'n_launches': n_launches, 'n_steps': ctx.n_steps,
                                               'n_params': plan.n_params, 'why': '', 'method': ctx.method, 'forward': ctx.forward_stats}
        return (None,) * 9 + tuple(gp) + (g_y0.reshape(ans.shape[1:]),)


def _odeint_discrete_rows_t(func, y0, t, method, options, lower, _forward_func):
    """odeint_discrete for `t` [batch, T] / options['t_lengths'] (fixed_rows.py): planned at the call - the fused row-local sweep over
    per-row times, or a ValueError with _row_plan's reason; there is no generic sweep over per-row grids."""
    from . import fixed_rows
    head = 'odeint_discrete: a 2-D `t` / options[\'t_lengths\']: '
    if lower is False:
        raise ValueError(head + 'lower=False asks for the generic (autograd) sweep, and there is none over per-row grids: the only backward is the '
                         "fused row-local sweep (lower=None, 'auto' or True)")
    if not isinstance(y0, torch.Tensor):
        raise ValueError(head + 'a tuple state: row i of `t` belongs to row i of ONE [batch, dim] state tensor')
    if method not in fixed_rows.D.FIXED_ROWS_T_METHODS:
        raise ValueError(fixed_rows.REFUSED + fixed_rows.D.fixed_rows_t_refusal(method, None, (y0,), options, check_rhs=False))
    fwd = func if _forward_func is None else _forward_func
    grad = torch.is_grad_enabled()
    if not grad:
        return odeint(fwd, y0, t, method=method, options=options)
    with torch.no_grad():                                # (every refusal of the forward, before anything is built)
        target = fixed_rows.target(fwd, y0.detach(), t, method, dict(options or {}))
    N.require_gpu_tensor(y0, 'y0')
    params = _params_of(func, y0, torch.as_tensor(t))
    plan, why = _row_plan(func, params, method, y0, per_row_t=True)
    if plan is None:
        raise ValueError(head + 'the fused row-local sweep, the only backward over per-row grids, does not take this call: ' + why)
    if y0.dim() != 2 or plan.dim != int(y0.shape[1]):
        raise ValueError(head + 'the callable lowers to rows of %d elements, the state is %s: row i of `t` must belong to row i of the program'
                         % (plan.dim, tuple(y0.shape)))
    rt = fixed_rows.times(y0, t, options)
    n_steps = (int(rt.lengths.max()) if rt.lengths is not None else rt.T) - 1
    return _OdeintDiscreteRowsT.apply(func, fwd, method, options, t, plan, (target, rt), n_steps, len(params), *(tuple(params) + (y0,)))


def _params_of(func, y0, t):
    """The tensors the gradient is taken with respect to, found the way odeint / odeint_adjoint find them: a module's grad-requiring
    parameters (then the bare tensors a wrapped callable carries), the grad-requiring leaves of a plain callable's evaluation."""
    if isinstance(func, torch.nn.Module):
        from .adjoint import _trainable
        return tuple(_trainable(func))
    if getattr(func, 'kind', 0) or getattr(func, 'stage_rhs', None) is not None or not callable(func):
        return ()                                        # a DeviceRHS descriptor: its weights are plain device tensors
    ys = y0 if isinstance(y0, (tuple, list)) else (y0,)
    if not all(isinstance(y, torch.Tensor) and y.is_floating_point() for y in ys):
        return ()
    return tuple(_graph_leaves(func, y0, t))


def _stored_sweep(ctx, t, ans, grad_output):
    """The reverse sweep over a stored trajectory - `ans`: the states at the grid points `t`, `grad_output`: the gradient of the loss with
    respect to each - on the first engine that takes it: fused linear, fused row-local, fused mlp (float32, or float64 behind
    ctx.mlp64), generic.  Returns (tuple of gradients
    at y0, list of parameter gradients, the last_backward_stats of the sweep)."""
    func, method, params = ctx.func, ctx.method, ctx.params
    like = ans[0]
    n_steps = int(like.shape[0]) - 1
    lin, lin_why = getattr(ctx, 'linear_plan', None) or (None, '')
    if lin is not None:
        try:
            with torch.no_grad():
                g_y0, gp = lin.sweep(t.to(like.dtype).double().cpu().numpy(), like, grad_output[0], len(params))
            stats = {'engine': 'fused linear sweep', 'n_steps': n_steps, 'n_launches': int(lin.used.stats.n_launches),
                     'why': '', 'method': method, 'forward': ctx.forward_stats}
            return (g_y0.reshape(like.shape[1:]),), gp, stats
        except HandoffTimeout as e:                  # the GPU is shared with another persistent kernel: nothing was committed
            lin_why = 'the fused kernel\'s grid hand-off timed out (%s)' % e
    row, row_why = getattr(ctx, 'row_plan', None) or (None, '')
    if row is not None:
        with torch.no_grad():
            shape = like.shape
            g_y0, theta, n_launches = _row_sweep(row, method, t, like.reshape(shape[0], -1, row.dim).contiguous(),
                                                 grad_output[0].reshape(shape[0], -1, row.dim).contiguous())
            gp = [None] * len(params)
            for k, off, n in row.targets:
                gp[k] = theta[off:off + n].reshape(params[k].shape).to(params[k].dtype)
        stats = {'engine': 'fused row-local sweep', 'n_steps': n_steps, 'n_launches': n_launches, 'why': '',
                 'method': method, 'n_params': row.n_params, 'forward': ctx.forward_stats}
        return (g_y0.reshape(shape[1:]),), gp, stats
    plan, why = _fused_plan(func, params, method, ctx.tensor_input, like, getattr(ctx, 'mlp64', False))
    if row_why:
        why = 'fused row-local sweep: %s; fused mlp sweep: %s' % (row_why, why)
    if lin_why:
        why = 'fused linear sweep: %s; %s' % (lin_why, why if row_why else 'fused mlp sweep: ' + why)
    if plan is not None:
        from .adjoint import canonical_to_module_order
        eng, mlp = plan
        try:
            with torch.no_grad():
                shape = like.shape
                g_y0, theta = eng.sweep(mlp, t.to(like.dtype).double().cpu().numpy(), like.reshape(shape[0], -1, shape[-1]),
                                        grad_output[0].reshape(shape[0], -1, shape[-1]))
                flat = canonical_to_module_order(func, theta)
                six = [p for l in (func.fc1, func.fc2, func.fc3) for p in (l.weight, l.bias)]
                of = {id(p): g for p, g in zip(six, torch.split(flat, [p.numel() for p in six]))}
                gp = [of[id(p)].reshape(p.shape).to(p.dtype) for p in params]        # (a frozen tensor is not among params)
            name = 'fused mlp sweep (float64)' if getattr(eng, 'dtype', None) is torch.float64 else 'fused mlp sweep'
            stats = {'engine': name, 'n_steps': n_steps, 'n_launches': int(eng.stats.n_launches),
                     'why': '', 'method': method, 'forward': ctx.forward_stats}
            return (g_y0.reshape(shape[1:]),), gp, stats
        except HandoffTimeout as e:                  # the GPU is shared with another persistent kernel: nothing was committed
            why = 'the fused kernel\'s grid hand-off timed out (%s)' % e
    if ctx.tensor_input:
        def tfunc(t_, y_, _f=func):
            return (_f(t_, y_[0]),)
    else:
        def tfunc(t_, y_, _f=func):
            return tuple(_f(t_, tuple(y_)))
    g_y0, gp = generic_sweep(tfunc, params, ans, t, grad_output, method)
    gp = [None if g is None else g.to(p.dtype) for g, p in zip(gp, params)]
    stats = {'engine': 'generic sweep', 'n_steps': n_steps, 'n_launches': None, 'why': why, 'method': method, 'forward': ctx.forward_stats}
    return tuple(g_y0), gp, stats


def _own_grid_sweep(ctx, gplan, y0, grad_output):
    """The backward of a solve on a grid of its own.  The linear system's kernel where the call has its plan (one launch, no stored
    trajectory); otherwise the grid states are recomputed from y0 - `odeint` on the grid as its default grid, one launch wherever the
    forward is fused - the output gradients are placed on the grid (_grid_plan) and _stored_sweep runs as on a default grid.  Beyond
    GRID_BYTES the grid is cut into segments: a forward pass keeps each segment's first state, the backward pass recomputes a segment,
    sweeps it and adds its lambda to the last gradient of the segment before (every output belongs to the segment of its step, so the
    boundary point's own gradient is counted once); parameter gradients add up."""
    method, params = ctx.method, ctx.params
    grid = gplan.grid
    n_steps, n_out = int(grid.shape[0]) - 1, len(gplan.out_step)
    kern, kern_why = getattr(ctx, 'linear_grid_plan', None) or (None, '')
    if kern is not None:
        try:
            with torch.no_grad():
                g_y0, gp = kern.sweep_grid(gplan, y0[0], grad_output[0], len(params))
            prof = kern.engine.profile()
            # (n_segments 0, recompute_launches 0: the kernel recomputes inside its own launch - no grid state is ever stored)
            stats = {'engine': 'fused linear sweep (own grid)', 'n_steps': n_steps, 'n_launches': int(kern.engine.stats.n_launches), 'why': '',
                     'method': method, 'forward': ctx.forward_stats,
                     'own_grid': {'n_grid_steps': n_steps, 'n_segments': 0, 'recompute_launches': 0, 'grid': prof['grid'],
                                  'scratch_bytes': prof['scratch_bytes']}}
            return (g_y0.reshape(y0[0].shape),), gp, stats
        except HandoffTimeout as e:                  # nothing was committed: the recompute on the grid takes the call ...
            kern_why = 'the fused kernel\'s grid hand-off timed out (%s)' % e
            # ... on the default-grid linear sweep, which was not planned while the kernel's plan stood (a refusal goes on to the
            # other engines with its reason, as it would have at the call)
            seg = _segments(n_steps, sum(y.numel() * y.element_size() for y in y0))
            ctx.linear_plan = _linear_plan(ctx.func, params, method, y0[0], n_points=_segment_points(seg))
    w_hi = [float(v) for v in gplan.out_w]
    w_lo = [float(v) for v in (torch.ones_like(gplan.out_w) - gplan.out_w)]              # 1 - w_j, formed in the state dtype
    bounds = _segments(n_steps, sum(y.numel() * y.element_size() for y in y0))
    n_seg = len(bounds) - 1
    launches = 0

    def solve(start, a, b):
        with torch.no_grad():
            out = odeint(ctx.fwd, start[0] if ctx.tensor_input else tuple(start), grid[a:b + 1], method=method)
        return (out,) if isinstance(out, torch.Tensor) else tuple(out)
    starts = [tuple(y.detach() for y in y0)]
    for s in range(n_seg - 1):                       # forward: only each segment's first state is kept
        starts.append(tuple(o[-1].clone() for o in solve(starts[-1], bounds[s], bounds[s + 1])))
        launches += 1
    lam, gp_sum, n_launches, stats = None, [None] * len(params), 0, None
    for s in range(n_seg - 1, -1, -1):
        a, b = bounds[s], bounds[s + 1]
        ys = solve(starts[s], a, b)
        launches += 1
        with torch.no_grad():
            gbar = tuple(torch.zeros_like(c) for c in ys)
            for j in range(n_out):                   # in the order of j: two calls give identical bits
                n = gplan.out_step[j]
                if not (a <= n < b or (j == 0 and a == 0)):
                    continue
                for gb_, g_ in zip(gbar, grad_output):
                    if w_hi[j] == 1.0:
                        gb_[n + 1 - a] += g_[j]
                    else:
                        gb_[n + 1 - a] += w_hi[j] * g_[j]
                        gb_[n - a] += w_lo[j] * g_[j]
            if lam is not None:
                for gb_, l_ in zip(gbar, lam):
                    gb_[b - a] += l_
        lam, gp, stats = _stored_sweep(ctx, grid[a:b + 1], ys, gbar)
        del ys, gbar
        for i, g in enumerate(gp):
            if g is not None:
                gp_sum[i] = g if gp_sum[i] is None else gp_sum[i] + g
        n_launches = None if n_launches is None or stats['n_launches'] is None else n_launches + stats['n_launches']
    stats = dict(stats, n_steps=n_steps, n_launches=n_launches)
    if kern_why:
        stats['why'] = 'fused linear sweep (own grid): %s%s' % (kern_why, '; ' + stats['why'] if stats['why'] else '')
    stats['own_grid'] = {'n_grid_steps': n_steps, 'n_segments': n_seg, 'recompute_launches': launches}
    return lam, gp_sum, stats


class _OdeintDiscrete(torch.autograd.Function):

    @staticmethod
    def forward(ctx, func, fwd, method, options, t, tensor_input, n_params, *args):
        params, y0 = args[:n_params], args[n_params:]
        ctx.func, ctx.fwd, ctx.method, ctx.tensor_input, ctx.n_params = func, fwd, method, tensor_input, n_params
        ctx.params = params
        with torch.no_grad():
            ans = odeint(fwd, y0[0] if tensor_input else tuple(y0), t, method=method, options=options)
        ctx.forward_stats = dict(odeint.last_stats) if isinstance(odeint.last_stats, dict) else {}
        if isinstance(ans, torch.Tensor):
            ans = (ans,)
        ctx.t = t
        step_size = (options or {}).get('step_size')
        gplan = getattr(ctx, 'grid_plan', None)          # (_OdeintDiscretePlanned has formed it for its planning)
        ctx.grid_plan = _grid_plan(t, step_size, ans[0].dtype) if gplan is None and step_size is not None else gplan
        if ctx.grid_plan is None:
            ctx.save_for_backward(*ans)
        else:                                            # (y0 is an input: keeping it costs nothing; the grid states are recomputed)
            ctx.save_for_backward(*(tuple(ans) + tuple(y0)))
        return tuple(ans)

    @staticmethod
    def backward(ctx, *grad_output):
        if ctx.grid_plan is None:
            ans = ctx.saved_tensors
        else:
            ans, y0 = ctx.saved_tensors[:len(grad_output)], ctx.saved_tensors[len(grad_output):]
        grad_output = tuple(g if g is not None else torch.zeros_like(a) for g, a in zip(grad_output, ans))
        if ctx.grid_plan is None:
            g_y0, gp, stats = _stored_sweep(ctx, ctx.t.detach(), ans, grad_output)
        else:
            g_y0, gp, stats = _own_grid_sweep(ctx, ctx.grid_plan, y0, grad_output)
        odeint_discrete.last_backward_stats = stats
        return (None,) * 7 + tuple(gp) + tuple(g_y0)


_Plans = collections.namedtuple('_Plans', 'mlp64 grid_plan linear_grid_plan linear_plan row_plan')


class _OdeintDiscretePlanned(torch.autograd.Function):
    """_OdeintDiscrete with what the call planned in front of its arguments: the call's `mlp64`, its GridPlan (None on the default grid)
    and the outcomes - (plan, '') or (None, why not); None where the route is off - of the own-grid kernel's, the linear and the
    row-local planning.  _stored_sweep and _own_grid_sweep read them from ctx."""

    @staticmethod
    def forward(ctx, plans, *args):
        ctx.mlp64, ctx.grid_plan, ctx.linear_grid_plan, ctx.linear_plan, ctx.row_plan = plans
        return _OdeintDiscrete.forward(ctx, *args)

    @staticmethod
    def backward(ctx, *grad_output):
        return (None,) + _OdeintDiscrete.backward(ctx, *grad_output)


def _mlp64_check(mlp64, func, params, method, tensor_input, ys, n_points):
    """odeint_discrete(mlp64=True): ValueError, at the call, where the float64 kernel will not take the backward (planned for a stored
    trajectory of n_points states like ys[0])."""
    if mlp64 is not True or not torch.is_grad_enabled():
        return
    y = ys[0].detach()
    if tensor_input and y.dtype != torch.float64:
        raise ValueError('odeint_discrete(mlp64=True): the fused float64 mlp sweep does not take this call: dtype %s'
                         % str(y.dtype).replace('torch.', ''))
    plan, why = _fused_plan(func, params, method, tensor_input, y.unsqueeze(0).expand((int(n_points),) + tuple(y.shape)), True)
    if plan is None:
        raise ValueError('odeint_discrete(mlp64=True): the fused float64 mlp sweep does not take this call: ' + why)


def odeint_discrete(func, y0, t, method='rk4', options=None, lower=None, linear=None, own_grid=None, mlp64=None, _forward_func=None):
    """`odeint(func, y0, t, method=method, options=options)` - same values, same engine - whose result is differentiable with respect to
    y0 and func's trainable tensors, with the gradient of the DISCRETE map the solver computed (what back-propagating through the
    reference's solver gives), not the continuous adjoint's.

    method: 'euler', 'midpoint', 'heun' / 'huen' or 'rk4' (the 3/8 rule) with eps == 0, on the default grid (`t` itself) or, with
    own_grid=True, on the grid of options['step_size'].  Anything else - adaptive and multistep methods, the grid_constructor / eps options,
    step_size without own_grid, a `t` that requires grad - raises ValueError and names `odeint_adjoint`.  Adaptive solves over a recorded step
    sequence are out of scope.  Tensor and tuple states are accepted;
    parameters are found as odeint / odeint_adjoint find them (module parameters; the grad-requiring leaves of a plain callable).
    own_grid: None - the module default `discrete.OWN_GRID` (False); False - options['step_size'] raises; True - it is accepted: the forward is
    the plain odeint call (one launch on the grid-walking kernel, len(t) outputs), the backward recomputes the grid states from y0 and runs
    the engines below on them (in segments beyond `discrete.GRID_BYTES`); with linear='auto' / True the linear system's whole backward is ONE
    launch that recomputes its own checkpoints ('fused linear sweep (own grid)', up to 1024 grid steps; `discrete.GRID_KERNEL = False` turns it
    off).  last_backward_stats then has 'own_grid': {'n_grid_steps', 'n_segments', 'recompute_launches'} and 'n_steps' counts grid steps;
    the own-grid kernel reports n_segments 0 and recompute_launches 0 - it recomputes inside its one launch and stores no grid state - and
    adds 'grid' (workgroups) and 'scratch_bytes' (its checkpoint scratch: grid x n_steps x 16 x D elements, independent of the batch).
    lower: None - the module default `discrete.LOWER` (False); False - the routes above; 'auto' - a callable the tracer lowers to a row-local
    program runs its whole backward in one launch (generated vjp, csrc/mi_ode_discrete_row.h), anything else falls to the routes above
    with the reason in last_backward_stats['why']; True - ValueError with that reason, here at the call.
    linear: None - the module default `discrete.LINEAR` (False); False - the routes above; 'auto' - f(t, y) = y W (+ b) (models.LinearODEFunc, or a
    callable the tracer puts in the 'linear' family: `y @ W`, `y @ W + b`, torch.nn.Linear(d, d)), float32 / float64, dim <= 128, runs its
    whole backward in one launch on the matrix cores (csrc/mi_ode_discrete_linear.h), anything else falls to the routes above with the
    reason in last_backward_stats['why']; True - ValueError with that reason, here at the call.
    mlp64: None - the module default `discrete.MLP64` (False); False - a float64 models.ODEFunc takes the generic sweep, as before; 'auto' - it
    runs its whole backward in one launch on the f64 matrix cores (csrc/mi_ode_discrete64.h: same box, parameter rules and step limit as the
    float32 fused mlp sweep, state and all six parameters float64; with own_grid=True through the same recompute, segments included),
    anything else falls to the generic sweep with the reason in last_backward_stats['why']; True - ValueError with that reason, here at
    the call.  The linear and row-local sweeps keep their precedence, and a float32 network is not affected.
    `t` of shape [batch, T] with y0 [batch, dim] (options['t_lengths'], an int tensor [batch]: how many of a row's times count), euler and rk4:
    every row on its own time grid (fixed_rows.py) - the forward is that solve, the backward the exact gradient of every row's own discrete
    map in ONE launch ('fused row-local sweep (per-row times)', csrc/mi_ode_discrete_row_t.h); grad y0[i] is what the call on
    (y0[i:i+1], t[i, :len_i]) with lower=True gives, the parameter gradients are summed over the rows in a fixed order, the cotangent of
    the padding is never read.  There lower=None, 'auto' and True all mean that sweep (a ValueError with the reason where it does not take
    the call), lower=False, linear=True and mlp64=True are ValueErrors, own_grid has nothing to act on (options['step_size'] is refused).
    `odeint_discrete.last_backward_stats`: {'engine': 'fused linear sweep' | 'fused linear sweep (own grid)' | 'fused row-local sweep' |
    'fused row-local sweep (per-row times)' | 'fused mlp sweep' | 'fused mlp sweep (float64)' | 'generic sweep', 'n_steps',
    'n_launches', 'why'} of the last backward ('why': the reason the fused kernels were not used)."""
    own_grid = OWN_GRID if own_grid is None else own_grid
    if own_grid not in (False, True):
        raise ValueError('odeint_discrete: own_grid must be False or True, not %r' % (own_grid,))
    check_supported(method, options, t, own_grid=own_grid)
    asked_lower = lower
    lower = LOWER if lower is None else lower
    if lower not in (False, True, 'auto'):
        raise ValueError("odeint_discrete: lower must be False, True or 'auto', not %r" % (lower,))
    linear = LINEAR if linear is None else linear
    if linear not in (False, True, 'auto'):
        raise ValueError("odeint_discrete: linear must be False, True or 'auto', not %r" % (linear,))
    mlp64 = MLP64 if mlp64 is None else mlp64
    if mlp64 not in (False, True, 'auto'):
        raise ValueError("odeint_discrete: mlp64 must be False, True or 'auto', not %r" % (mlp64,))
    from . import fixed_rows
    if fixed_rows.wanted(method, t, options):
        # `t` [batch, T] / options['t_lengths']: the only backward is the fused row-local sweep over per-row times.  lower=None means that
        # sweep here (not the module default); linear=True / mlp64=True promise an engine that has no per-row form: a ValueError, as
        # wherever their engine does not take the call ('auto' falls through to the one sweep there is).
        for name, value in (('linear', linear), ('mlp64', mlp64)):
            if value is True:
                raise ValueError('odeint_discrete(%s=True): a 2-D `t` / options[\'t_lengths\'] has one backward, the fused row-local sweep over '
                                 'per-row times; the fused %s sweep reads one shared grid' % (name, 'linear' if name == 'linear' else 'float64 mlp'))
        return _odeint_discrete_rows_t(func, y0, t, method, options, asked_lower, _forward_func)
    tensor_input = isinstance(y0, torch.Tensor)
    ys = (y0,) if tensor_input else tuple(y0)
    for y_ in ys:
        N.require_gpu_tensor(y_, 'y0')
    t = torch.as_tensor(t)
    params = _params_of(func, y0, t) if torch.is_grad_enabled() else ()
    # (_forward_func: models.ODEBlock hands the forward solve the network's own fused descriptor, as its inference branch does)
    fwd = func if _forward_func is None else _forward_func
    rest = (func, fwd, method, options, t, tensor_input, len(params)) + tuple(params) + tuple(ys)
    if linear is False and lower is False and mlp64 is False:
        out = _OdeintDiscrete.apply(*rest)
        return out[0] if tensor_input else tuple(out)
    # One planning pass, at the call.  n_sweep: the points of the stored trajectories the backward sweeps - `t` itself, or on a grid of
    # its own the distinct lengths of the segments of the recompute (the first segment's first).
    grad = torch.is_grad_enabled()
    off = (None, 'gradients are disabled')
    step_size = (options or {}).get('step_size')
    gplan, n_sweep = None, (t.numel(),)
    if step_size is not None:
        gplan = _grid_plan(t, step_size, ys[0].dtype)
        n_grid_steps = int(gplan.grid.shape[0]) - 1
        n_sweep = _segment_points(_segments(n_grid_steps, sum(y_.numel() * y_.element_size() for y_ in ys)))
    kern_plan = lin_plan = row_plan = None

    def taken():
        return any(p is not None and p[0] is not None for p in (kern_plan, lin_plan, row_plan))
    if linear is not False:
        if gplan is not None:                            # the kernel that recomputes its checkpoints
            kern_plan = off if not grad else (None, 'discrete.GRID_KERNEL is False') if not GRID_KERNEL else \
                _linear_plan(func, params, method, y0, own_grid=(n_grid_steps, len(gplan.out_step)))
        if not taken():                                  # the default-grid sweep, over the recompute where the grid is the call's own
            lin_plan = off if not grad else _linear_plan(func, params, method, y0, n_points=n_sweep)
            if linear is True and lin_plan[0] is None:
                raise ValueError('odeint_discrete(linear=True): the fused linear sweep does not take this call: ' + lin_plan[1])
    if lower is not False and not taken():
        row_plan = _row_plan(func, params, method, y0) if grad else off
        if lower is True and row_plan[0] is None:
            raise ValueError('odeint_discrete(lower=True): the fused row-local sweep does not take this call: ' + row_plan[1])
    if mlp64 is not False and not taken():
        _mlp64_check(mlp64, func, params, method, tensor_input, ys, n_sweep[0])
    out = _OdeintDiscretePlanned.apply(_Plans(mlp64, gplan, kern_plan, lin_plan, row_plan), *rest)
    return out[0] if tensor_input else tuple(out)


odeint_discrete.last_backward_stats = {}
