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

Two engines:
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
_ENGINES = {}


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
    while _ENGINES:
        _ENGINES.pop(next(iter(_ENGINES))).close()


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
        plan, why = _fused_plan(func, params, method, ctx.tensor_input, like)
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


def odeint_discrete(func, y0, t, method='rk4', options=None, _forward_func=None):
    """`odeint(func, y0, t, method=method, options=options)` - same values, same engine - whose result is differentiable with respect to
    y0 and func's trainable tensors, with the gradient of the DISCRETE map the solver computed (what back-propagating through the
    reference's solver gives), not the continuous adjoint's.

    method: 'euler', 'midpoint', 'heun' / 'huen' or 'rk4' (the 3/8 rule), on the default grid (`t` itself) with eps == 0.  Anything else -
    adaptive and multistep methods, the step_size / grid_constructor / eps options, a `t` that requires grad - raises ValueError and
    names `odeint_adjoint`.  Adaptive solves over a recorded step sequence are out of scope.  Tensor and tuple states are accepted;
    parameters are found as odeint / odeint_adjoint find them (module parameters; the grad-requiring leaves of a plain callable).
    `odeint_discrete.last_backward_stats`: {'engine': 'fused mlp sweep' | 'generic sweep', 'n_steps', 'n_launches', 'why'} of the last
    backward ('why': the reason the fused kernel was not used)."""
    check_supported(method, options, t)
    tensor_input = isinstance(y0, torch.Tensor)
    ys = (y0,) if tensor_input else tuple(y0)
    for y_ in ys:
        N.require_gpu_tensor(y_, 'y0')
    t = torch.as_tensor(t)
    params = _params_of(func, y0, t) if torch.is_grad_enabled() else ()
    # (_forward_func: models.ODEBlock hands the forward solve the network's own fused descriptor, as its inference branch does)
    out = _OdeintDiscrete.apply(func, func if _forward_func is None else _forward_func, method, options, t, tensor_input, len(params), *params, *ys)
    return out[0] if tensor_input else tuple(out)


odeint_discrete.last_backward_stats = {}
