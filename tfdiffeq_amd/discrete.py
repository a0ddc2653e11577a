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

Four engines:
  * fused linear sweep - opt-in (`linear='auto'` / True, module default LINEAR): f(t, y) = y W (+ b) - models.LinearODEFunc, or a callable the
    tracer puts in the 'linear' family (`y @ W`, `y @ W + b`, torch.nn.Linear(d, d)) - float32 and float64, dim <= 128: the whole backward,
    all steps, is ONE launch on the matrix cores (csrc/mi_ode_discrete_linear.h);
  * fused row-local sweep - opt-in (`lower='auto'` / True, module default LOWER): a plain Python callable the tracer lowers to a row-local
    program (lower.py, state of up to 32 elements per trajectory) gets the vjp of its trace as generated device code, and the whole
    backward, all steps, is ONE launch with a trajectory per lane (csrc/mi_ode_discrete_row.h), float32 and float64;
  * fused mlp sweep - models.ODEFunc / rhs.MLP (relu, softplus, tanh), float32, time independent, dim <= 64, hidden <= 128, all six
    parameters trainable: the whole backward, all steps, is ONE launch (csrc/mi_ode_discrete.h);
  * generic sweep   - any `func`, any dtype, tuple states: per step one taped re-evaluation in torch ops and one torch.autograd.grad call.

Scope: euler, midpoint, heun / huen and rk4 (the 3/8 rule) on the default grid (`t` itself) with eps == 0.  Adaptive solves over a
recorded step sequence, the multistep family and grids of their own (step_size / grid_constructor / eps) are not covered: they raise
ValueError and name `odeint_adjoint`.
"""
import ctypes as C

import torch

from . import _native as N
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
ROW_GRID = 0                  # workgroups of the fused row-local sweep; 0: one per 256 trajectories, up to 1024
_ENGINES = {}
_LINEAR_ENGINES = {}


def check_supported(method, options=None, t=None):
    """ValueError for everything outside the scope of the discrete gradient, naming the reason and the alternative."""
    alt = '; use odeint_adjoint (the continuous adjoint) for this call'
    if method not in TABLEAUS:
        raise ValueError('odeint_discrete: method %r is not a fixed-grid Runge-Kutta method (%s): adaptive and multistep solves have no '
                         'fixed discrete map to transpose here%s' % (method, ', '.join(sorted(TABLEAUS)), alt))
    opts = options or {}
    for key in ('step_size', 'grid_constructor'):
        if opts.get(key) is not None:
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


class _FusedDiscreteEngine(object):
    """Owns one mi_ode_discrete handle: the reverse sweep of `n_points - 1` steps of `method` for a [batch, dim] float32 state and the
    dim -> hidden -> hidden -> dim MLP, one launch."""

    def __init__(self, batch, dim, hidden, method, n_points, device, chunk_tiles=0):
        from .solvers import _fill_tableau
        self.lib = N.load()
        self.device = torch.device(device)
        d = N.DiscreteDesc()
        d.batch, d.dim, d.hidden = int(batch), int(dim), int(hidden)
        _fill_tableau(d.tableau, TABLEAUS[method], None)
        d.n_points, d.chunk_tiles = int(n_points), int(chunk_tiles)
        self.desc = d
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self.lib.mi_ode_discrete_create(C.byref(d), C.byref(h)), 'mi_ode_discrete_create')
        self.h = h
        self.batch, self.dim, self.n_points = int(batch), int(dim), int(n_points)
        self.n_params = int(self.lib.mi_ode_discrete_num_params(h))
        self.stats = N.Stats()

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mi_ode_discrete_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sweep(self, mlp, t, ys, grad_ys):
        """(grad_y0 [batch, dim], grad_theta [P] in canonical order) from the forward solution and its gradient, both [N, batch, dim]."""
        r = N.Rhs()
        keep = mlp.fill(r, torch.float32, self.device)
        ys, grad_ys = ys.contiguous(), grad_ys.contiguous()
        g_y0 = torch.empty(self.batch, self.dim, dtype=torch.float32, device=self.device)
        g_th = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        tt = (C.c_double * self.n_points)(*[float(v) for v in t])
        with torch.cuda.device(self.device):
            rc = N.check(self.lib.mi_ode_discrete_sweep(self.h, C.byref(r), tt, ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_th.data_ptr(),
                                                        C.byref(self.stats), N.stream_ptr(self.device)), 'mi_ode_discrete_sweep')
        del keep
        if rc != 0:
            from .adjoint import HandoffTimeout
            if rc & N.ST_SYNC_TIMEOUT:
                raise HandoffTimeout(N.status_message(rc))
            raise AssertionError(N.status_message(rc))
        return g_y0, g_th


def _cached_engine(*key):
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _FusedDiscreteEngine(*key)                 # (evict only after a successful create: a refusal must not cost live engines)
        while len(_ENGINES) >= 4:
            _ENGINES.pop(next(iter(_ENGINES))).close()
        _ENGINES[key] = eng
    return eng


def clear_engines():
    """Empties both engine caches.  The MLP engines are closed here.  A linear engine is only dropped: a call that has run forward and not
    yet backward still holds it, so its device memory is released when the last such graph is gone, which need not be now."""
    while _ENGINES:
        _ENGINES.pop(next(iter(_ENGINES))).close()
    _LINEAR_ENGINES.clear()                              # (dropped, not closed: see _cached_linear_engine)


def _fused_plan(func, params, method, tensor_input, like):
    """((engine, descriptor), '') when the fused kernel takes this backward, else (None, why not) - in the style of odeint.plan."""
    if not FUSED:
        return None, 'discrete.FUSED is False'
    if not tensor_input:
        return None, 'a tuple state'
    if not like.is_cuda:
        return None, 'a host tensor'
    if like.dtype != torch.float32:
        return None, 'dtype %s (the fused sweep is float32)' % str(like.dtype).replace('torch.', '')
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
    if mlp.time_dependent:
        return None, 'a time-dependent network (the stage time enters the first layer)'
    y1 = like[0]
    if y1.dim() < 2 or not mlp.supports(y1):
        return None, 'outside the tile box of rhs.MLP.supports (dim <= %d, hidden <= %d, state [batch, dim])' % (mlp.MAX_DIM, mlp.MAX_HIDDEN)
    want = [p for l in layers for p in (l.weight, l.bias)]
    if len(params) != 6 or any(a is not b for a, b in zip(params, want)):
        return None, 'frozen or extra parameters (the kernel produces the gradients of all six tensors of the network)'
    if any(p.dtype != torch.float32 or p.device != like.device for p in want):
        return None, 'parameters in another dtype or on another device than the state'
    n_points = int(like.shape[0])
    if n_points - 1 > 1024:
        return None, 'more than 1024 steps'
    batch = y1.numel() // y1.shape[-1]
    try:
        eng = _cached_engine(batch, int(y1.shape[-1]), int(mlp.hidden), 'heun' if method == 'huen' else method, n_points, str(like.device), int(CHUNK_TILES))
    except N.NativeError as e:                           # e.g. no memory for the activation scratch
        return None, 'the fused engine could not be created (%s)' % e
    return (eng, mlp), ''


class _FusedLinearEngine(object):
    """Owns one mi_ode_discrete_linear handle: the reverse sweep of `n_points - 1` steps of `method` for a [batch, dim] state and
    f(y) = y W (+ b), one launch."""

    def __init__(self, batch, dim, has_bias, method, n_points, device, dtype):
        from .solvers import _fill_tableau
        self.lib = N.load()
        self.device = torch.device(device)
        self.dtype = dtype
        d = N.DiscreteLinearDesc()
        d.dtype, d.dim, d.batch, d.has_bias, d.n_points = N.dtype_code(dtype), int(dim), int(batch), int(bool(has_bias)), int(n_points)
        _fill_tableau(d.tableau, TABLEAUS[method], None)
        self.desc = d
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self.lib.mi_ode_discrete_linear_create(C.byref(d), C.byref(h)), 'mi_ode_discrete_linear_create')
        self.h = h
        self.batch, self.dim, self.n_points, self.has_bias = int(batch), int(dim), int(n_points), bool(has_bias)
        self.stats = N.Stats()

    def close(self):
        if getattr(self, 'h', None):
            self.lib.mi_ode_discrete_linear_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self):
        """{'grid', 'sweep_us', 'store_us', 'fold_us'} of the last sweep: workgroup 0's clock over the tile sweep (all steps, the weight-gradient
        products included), the store of its partial block, the final hand-off and fold."""
        out = (C.c_double * 3)()
        g = self.lib.mi_ode_discrete_linear_profile(self.h, out)
        return {'grid': int(g), 'sweep_us': out[0], 'store_us': out[1], 'fold_us': out[2]}

    def sweep(self, W, b, t, ys, grad_ys):
        """(grad_y0 [batch, dim], grad_W [dim, dim] in W's [in, out] layout, grad_b [dim] or None) from the forward solution and its
        gradient, both [N, batch, dim].  W, b: device tensors in the state dtype, read now (nothing is cached between calls)."""
        r = N.Rhs()
        r.kind, r.sign, r.hidden = N.RHS_LINEAR, 1.0, 0
        W = W.contiguous()
        r.w[0] = W.data_ptr()
        if b is not None:
            b = b.contiguous()
            r.b[0] = b.data_ptr()
        ys, grad_ys = ys.contiguous(), grad_ys.contiguous()
        g_y0 = torch.empty(self.batch, self.dim, dtype=self.dtype, device=self.device)
        g_w = torch.empty(self.dim, self.dim, dtype=self.dtype, device=self.device)
        g_b = torch.empty(self.dim, dtype=self.dtype, device=self.device) if b is not None else None
        tt = (C.c_double * self.n_points)(*[float(v) for v in t])
        with torch.cuda.device(self.device):
            rc = N.check(self.lib.mi_ode_discrete_linear_sweep(self.h, C.byref(r), tt, ys.data_ptr(), grad_ys.data_ptr(), g_y0.data_ptr(), g_w.data_ptr(),
                                                               None if g_b is None else g_b.data_ptr(), C.byref(self.stats),
                                                               N.stream_ptr(self.device)), 'mi_ode_discrete_linear_sweep')
        if rc != 0:
            from .adjoint import HandoffTimeout
            if rc & N.ST_SYNC_TIMEOUT:
                raise HandoffTimeout(N.status_message(rc))
            raise AssertionError(N.status_message(rc))
        return g_y0, g_w, g_b


def _cached_linear_engine(*key):
    """The engine of `key`, four cached at most.  The plan of a call holds its engine from the call to its backward, so eviction (and
    clear_engines) only drops the cache's reference: the handle is destroyed when the last pending plan lets go of it (__del__)."""
    eng = _LINEAR_ENGINES.get(key)
    if eng is None:
        eng = _FusedLinearEngine(*key)                   # (evict only after a successful create: a refusal must not cost live engines)
        while len(_LINEAR_ENGINES) >= 4:
            _LINEAR_ENGINES.pop(next(iter(_LINEAR_ENGINES)))
        _LINEAR_ENGINES[key] = eng
    return eng


def _on_device(x):
    return x.is_cuda


class _LinearPlan(object):
    """What the fused linear sweep of ONE call needs: the parameters themselves (read at the backward, so an in-place optimizer step is
    seen), how the matrix is laid out ('W': [in, out] as the kernel reads it; 'Wt': [out, in], torch.nn.Linear's), where their gradients
    go among the call's parameters, and the engine."""

    def __init__(self, W, b, how, slots, engine):
        self.W, self.b, self.how, self.slots, self.engine = W, b, how, slots, engine

    def sweep(self, t, ys, grad_ys, n_params):
        dim = int(ys.shape[-1])
        W = self.W.detach()
        g_y0, g_w, g_b = self.engine.sweep(W if self.how == 'W' else W.t().contiguous(), None if self.b is None else self.b.detach().reshape(-1),
                                           t, ys.reshape(ys.shape[0], -1, dim), grad_ys.reshape(ys.shape[0], -1, dim))
        gp = [None] * n_params
        gp[self.slots[0]] = (g_w if self.how == 'W' else g_w.t().contiguous()).reshape(self.W.shape)
        if self.b is not None:
            gp[self.slots[1]] = g_b.reshape(self.b.shape)
        return g_y0, gp


def _linear_plan(func, params, method, y0, like=None, n_points=None):
    """(_LinearPlan, '') when the fused linear sweep takes this call, else (None, why not).  like: the solution (or any tensor of its
    shape [N, ...]); without one, n_points is the number of grid points.  Creates (or finds) the engine - at the call, not in backward."""
    from . import lower as L
    from . import models as M
    if not isinstance(y0, torch.Tensor):
        return None, 'a tuple state (the fused linear sweep takes one state tensor)'
    if y0.dtype not in (torch.float32, torch.float64):
        return None, 'dtype %s (the fused linear sweep is float32 / float64)' % str(y0.dtype).replace('torch.', '')
    if method not in TABLEAUS:
        return None, 'method %r' % (method,)
    if y0.dim() < 1:
        return None, 'a 0-d state'
    dim = int(y0.shape[-1])
    if isinstance(func, M.LinearODEFunc):
        if dim != func.dim:
            return None, 'the state\'s last axis is %d, the module\'s dim %d' % (dim, func.dim)
        W, b, how = func.weight, func.bias, 'W'
    else:
        if getattr(func, 'kind', 0) or getattr(func, 'stage_rhs', None) is not None or not callable(func):
            return None, 'a device right-hand side descriptor, not a models.LinearODEFunc or a Python callable'
        nfe = getattr(func, 'nfe', None)                 # (tracing runs a module's forward on proxies: not an evaluation the caller counts)
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
        except Exception as e:                           # the callable itself failed on the proxies
            return None, 'tracing failed: %s: %s' % (type(e).__name__, e)
        finally:
            if isinstance(nfe, int) and getattr(func, 'nfe', nfe) != nfe:
                func.nfe = nfe
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
    n_points = int(like.shape[0]) if like is not None else int(n_points)
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
    try:
        eng = _cached_linear_engine(batch, dim, b is not None, 'heun' if method == 'huen' else method, n_points, str(y0.device), y0.dtype)
    except N.NativeError as e:
        return None, 'the fused engine could not be created (%s)' % e
    return _LinearPlan(W, b, how, slots, eng), ''


class _RowPlan(object):
    """What the fused row-local sweep of ONE call needs: the discrete plugin's table, the trace's parameter layout and a copy of the
    constants the forward call was bound with (the program's pool buffer is shared: the next odeint of the same program overwrites it)."""

    def __init__(self, lib, table, tr, targets, n_params, pool, scalars):
        self.lib, self.table, self.trace, self.targets, self.n_params, self.pool, self.scalars = lib, table, tr, targets, n_params, pool, scalars
        self.dim = 1
        for s_ in tr.tail:
            self.dim *= int(s_)


def _row_plan(func, params, method, y0, build=True):
    """(_RowPlan, '') when the fused row-local sweep takes this call, else (None, why not).  Traces, classifies, generates the vjp and
    builds the plugin - at the call, not in backward."""
    from . import lower as L
    if not isinstance(y0, torch.Tensor):
        return None, 'a tuple state (the fused row-local sweep takes one state tensor)'
    if y0.dtype not in (torch.float32, torch.float64):
        return None, 'dtype %s (the fused row-local sweep is float32 / float64)' % str(y0.dtype).replace('torch.', '')
    if method not in TABLEAUS:
        return None, 'method %r' % (method,)
    if getattr(func, 'kind', 0) or getattr(func, 'stage_rhs', None) is not None or not callable(func):
        return None, 'a device right-hand side descriptor, not a Python callable'
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
        kind, _info = L.classify(tr, rows=rows)
    except L.TraceError as e:
        return None, 'the callable cannot be lowered: %s' % e
    except Exception as e:                               # the callable itself failed on the proxies
        return None, 'tracing failed: %s: %s' % (type(e).__name__, e)
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
        lib, table = R.discrete_plugin(source, y0.dtype)
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


class _OdeintDiscrete(torch.autograd.Function):

    @staticmethod
    def forward(ctx, func, fwd, method, options, t, tensor_input, n_params, *args):
        params, y0 = args[:n_params], args[n_params:]
        ctx.func, ctx.method, ctx.tensor_input, ctx.n_params = func, method, tensor_input, n_params
        ctx.params = params
        with torch.no_grad():
            ans = odeint(fwd, y0[0] if tensor_input else tuple(y0), t, method=method, options=options)
        ctx.forward_stats = dict(odeint.last_stats) if isinstance(odeint.last_stats, dict) else {}
        if isinstance(ans, torch.Tensor):
            ans = (ans,)
        ctx.t = t
        ctx.save_for_backward(*ans)
        return tuple(ans)

    @staticmethod
    def backward(ctx, *grad_output):
        func, method, params = ctx.func, ctx.method, ctx.params
        ans = ctx.saved_tensors
        like = ans[0]
        t = ctx.t.detach()
        grad_output = tuple(g if g is not None else torch.zeros_like(a) for g, a in zip(grad_output, ans))
        n_steps = int(like.shape[0]) - 1
        lin, lin_why = getattr(ctx, 'linear_plan', None) or (None, '')
        if lin is not None:
            from .adjoint import HandoffTimeout
            try:
                with torch.no_grad():
                    g_y0, gp = lin.sweep(t.to(like.dtype).double().cpu().numpy(), like, grad_output[0], len(params))
                odeint_discrete.last_backward_stats = {'engine': 'fused linear sweep', 'n_steps': n_steps, 'n_launches': int(lin.engine.stats.n_launches),
                                                       'why': '', 'method': method, 'forward': ctx.forward_stats}
                return (None,) * 7 + tuple(gp) + (g_y0.reshape(like.shape[1:]),)
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
            odeint_discrete.last_backward_stats = {'engine': 'fused row-local sweep', 'n_steps': n_steps, 'n_launches': n_launches, 'why': '',
                                                   'method': method, 'n_params': row.n_params, 'forward': ctx.forward_stats}
            return (None,) * 7 + tuple(gp) + (g_y0.reshape(shape[1:]),)
        plan, why = _fused_plan(func, params, method, ctx.tensor_input, like)
        if row_why:
            why = 'fused row-local sweep: %s; fused mlp sweep: %s' % (row_why, why)
        if lin_why:
            why = 'fused linear sweep: %s; %s' % (lin_why, why if row_why else 'fused mlp sweep: ' + why)
        if plan is not None:
            from .adjoint import HandoffTimeout, canonical_to_module_order
            eng, mlp = plan
            try:
                with torch.no_grad():
                    shape = like.shape
                    g_y0, theta = eng.sweep(mlp, t.to(like.dtype).double().cpu().numpy(), like.reshape(shape[0], -1, shape[-1]),
                                            grad_output[0].reshape(shape[0], -1, shape[-1]))
                    flat = canonical_to_module_order(func, theta)
                    gp = [g.reshape(p.shape).to(p.dtype) for g, p in zip(torch.split(flat, [p.numel() for p in params]), params)]
                odeint_discrete.last_backward_stats = {'engine': 'fused mlp sweep', 'n_steps': n_steps, 'n_launches': int(eng.stats.n_launches),
                                                       'why': '', 'method': method, 'forward': ctx.forward_stats}
                return (None,) * 7 + tuple(gp) + (g_y0.reshape(shape[1:]),)
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
        odeint_discrete.last_backward_stats = {'engine': 'generic sweep', 'n_steps': n_steps, 'n_launches': None, 'why': why, 'method': method,
                                               'forward': ctx.forward_stats}
        return (None,) * 7 + tuple(gp) + tuple(g_y0)


class _OdeintDiscreteLowered(torch.autograd.Function):
    """_OdeintDiscrete with the outcome of the row-local planning - (plan, '') or (None, why not) - in front of its arguments."""

    @staticmethod
    def forward(ctx, row_plan, *args):
        ctx.row_plan = row_plan
        return _OdeintDiscrete.forward(ctx, *args)

    @staticmethod
    def backward(ctx, *grad_output):
        return (None,) + _OdeintDiscrete.backward(ctx, *grad_output)


class _OdeintDiscreteLinear(torch.autograd.Function):
    """_OdeintDiscrete with the outcomes of the linear and the row-local planning (the latter None when `lower` is off) in front of its arguments."""

    @staticmethod
    def forward(ctx, linear_plan, row_plan, *args):
        ctx.linear_plan, ctx.row_plan = linear_plan, row_plan
        return _OdeintDiscrete.forward(ctx, *args)

    @staticmethod
    def backward(ctx, *grad_output):
        return (None, None) + _OdeintDiscrete.backward(ctx, *grad_output)


def odeint_discrete(func, y0, t, method='rk4', options=None, lower=None, linear=None, _forward_func=None):
    """`odeint(func, y0, t, method=method, options=options)` - same values, same engine - whose result is differentiable with respect to
    y0 and func's trainable tensors, with the gradient of the DISCRETE map the solver computed (what back-propagating through the
    reference's solver gives), not the continuous adjoint's.

    method: 'euler', 'midpoint', 'heun' / 'huen' or 'rk4' (the 3/8 rule), on the default grid (`t` itself) with eps == 0.  Anything else -
    adaptive and multistep methods, the step_size / grid_constructor / eps options, a `t` that requires grad - raises ValueError and
    names `odeint_adjoint`.  Adaptive solves over a recorded step sequence are out of scope.  Tensor and tuple states are accepted;
    parameters are found as odeint / odeint_adjoint find them (module parameters; the grad-requiring leaves of a plain callable).
    lower: None - the module default `discrete.LOWER` (False); False - the routes above; 'auto' - a callable the tracer lowers to a row-local
    program runs its whole backward in one launch (generated vjp, csrc/mi_ode_discrete_row.h), anything else falls to the routes above
    with the reason in last_backward_stats['why']; True - ValueError with that reason, here at the call.
    linear: None - the module default `discrete.LINEAR` (False); False - the routes above; 'auto' - f(t, y) = y W (+ b) (models.LinearODEFunc, or a
    callable the tracer puts in the 'linear' family: `y @ W`, `y @ W + b`, torch.nn.Linear(d, d)), float32 / float64, dim <= 128, runs its
    whole backward in one launch on the matrix cores (csrc/mi_ode_discrete_linear.h), anything else falls to the routes above with the
    reason in last_backward_stats['why']; True - ValueError with that reason, here at the call.
    `odeint_discrete.last_backward_stats`: {'engine': 'fused linear sweep' | 'fused row-local sweep' | 'fused mlp sweep' | 'generic sweep', 'n_steps',
    'n_launches', 'why'} of the last backward ('why': the reason the fused kernels were not used)."""
    check_supported(method, options, t)
    lower = LOWER if lower is None else lower
    if lower not in (False, True, 'auto'):
        raise ValueError("odeint_discrete: lower must be False, True or 'auto', not %r" % (lower,))
    linear = LINEAR if linear is None else linear
    if linear not in (False, True, 'auto'):
        raise ValueError("odeint_discrete: linear must be False, True or 'auto', not %r" % (linear,))
    tensor_input = isinstance(y0, torch.Tensor)
    ys = (y0,) if tensor_input else tuple(y0)
    for y_ in ys:
        N.require_gpu_tensor(y_, 'y0')
    t = torch.as_tensor(t)
    params = _params_of(func, y0, t) if torch.is_grad_enabled() else ()
    # (_forward_func: models.ODEBlock hands the forward solve the network's own fused descriptor, as its inference branch does)
    fwd = func if _forward_func is None else _forward_func
    if linear is not False:
        lin_plan = _linear_plan(func, params, method, y0, n_points=t.numel()) if torch.is_grad_enabled() else (None, 'gradients are disabled')
        if linear is True and lin_plan[0] is None:
            raise ValueError('odeint_discrete(linear=True): the fused linear sweep does not take this call: ' + lin_plan[1])
        row_plan = None
        if lower is not False and lin_plan[0] is None:
            row_plan = _row_plan(func, params, method, y0) if torch.is_grad_enabled() else (None, 'gradients are disabled')
            if lower is True and row_plan[0] is None:
                raise ValueError('odeint_discrete(lower=True): the fused row-local sweep does not take this call: ' + row_plan[1])
        out = _OdeintDiscreteLinear.apply(lin_plan, row_plan, func, fwd, method, options, t, tensor_input, len(params), *params, *ys)
        return out[0] if tensor_input else tuple(out)
    if lower is not False:
        row_plan = _row_plan(func, params, method, y0) if torch.is_grad_enabled() else (None, 'gradients are disabled')
        if lower is True and row_plan[0] is None:
            raise ValueError('odeint_discrete(lower=True): the fused row-local sweep does not take this call: ' + row_plan[1])
        out = _OdeintDiscreteLowered.apply(row_plan, func, fwd, method, options, t, tensor_input, len(params), *params, *ys)
        return out[0] if tensor_input else tuple(out)
    out = _OdeintDiscrete.apply(func, fwd, method, options, t, tensor_input, len(params), *params, *ys)
    return out[0] if tensor_input else tuple(out)


odeint_discrete.last_backward_stats = {}
