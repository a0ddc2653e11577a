"""Hypersolvers (tfdiffeq/hyper_solvers/ of the reference: base.py, euler.py): HyperEuler, HyperMidpoint and HyperHeun.

A hypersolver takes a fixed step of a base method and adds a learned correction dt^(p+1) * g(cat([y, f(t, y), dt])), g a small dense
network (Poli et al., "Hypersolvers: Toward Fast Continuous-Depth Models", arXiv:2007.09601).  The update formulas are the reference's
literally, quirks included: dt = t_span[1] - t_span[0] for every step, g sees dt as its time input, row i of a trajectory is the state
BEFORE step i, the second correction of midpoint / Heun is scaled by dt^3.  t_span is taken in the state dtype.

Two engines; `<solver>.last_stats` says which one ran a call and why:
  fused   ONE launch per trajectory / residual_trajectory / _hypersolver_residuals call (csrc/mi_ode_hyper.h): f on the row-local
          kernels' functor, g's layers on the matrix cores.  Taken when the state is a 2-D float32 / float64 CUDA tensor, f is a row-local
          device system (rhs.Lorenz, rhs.LotkaVolterra, the 2 x 2 rhs.Linear / rhs.CubicLinear, rhs.CustomRowLocal) or a Python callable
          that tfdiffeq_amd.lower maps to a row-local program, g is an nn.Sequential that `describe_g` accepts, and no result would
          require grad.  `last_stats['n_launches']` is 1 while g's weights fit in LDS beside the two activation tiles, and 2 (the weight
          pack into the workspace, then the kernel) for a larger g.
  eager   everything else: the reference's loop in torch operations on the GPU - differentiable, the training path.
CPU tensors are refused (NativeError), as on every path of this package.

Training on the fused engine is opt-in: options={'grad': False | 'auto' | True} on the constructor (module default FUSED_GRAD = False).
With 'auto' / True a `trajectory` or `_hypersolver_residuals` call in which something requires grad runs the SAME forward kernel inside
a torch.autograd.Function whose backward is ONE launch for all steps and rows (csrc/mi_ode_hyper_grad.h; two when g's weight images do
not fit in LDS): the gradient with respect to g's parameters and, for a trajectory, y.  `describe_grad` is the box, a pure host
function: f a Python callable the tracer lowers to a row-local program without trainable tensors, or rhs.Lorenz / rhs.LotkaVolterra
(differentiated through their traced equivalents); g whatever `describe_g` accepts whose activation tiles fit in LDS.  Outside the box
'auto' trains on the eager engine with the limit in last_stats['why']; True raises ValueError with it.  `last_backward_stats` is set by
the backward.
"""
import ctypes
import importlib

import torch
from torch import nn

from . import _native as N
from . import rhs as R

MAX_LAYERS = N.HYPER_MAX_LAYERS
MAX_WIDTH = 128
FUSED_GRAD = False               # the default of options['grad']: False (training on the eager engine), 'auto' or True
GRAD_GRID = 0                    # cap of the gradient kernel's grid; 0: GRAD_DEFAULT_GRID.  The [grid, P] partials stay small
GRAD_DEFAULT_GRID = 128

_ACTS = {nn.ReLU: N.HYPER_ACT_RELU, nn.LeakyReLU: N.HYPER_ACT_LEAKY_RELU, nn.PReLU: N.HYPER_ACT_PRELU, nn.Tanh: N.HYPER_ACT_TANH,
         nn.Softplus: N.HYPER_ACT_SOFTPLUS}


def describe_g(g, dim):
    """(table, None) when the fused kernels can evaluate `g` for a state of width `dim`, else (None, reason naming the layer).
    table: {'layers': [(nn.Linear, act code, activation module or None)], 'text': 'Linear(7, 64) PReLU(64) ...'}."""
    if not isinstance(g, nn.Sequential):
        return None, 'g is a %s, not an nn.Sequential of Linear layers and activations' % type(g).__name__
    layers = []
    for i, m in enumerate(g):
        if isinstance(m, nn.Linear):
            layers.append([m, N.HYPER_ACT_NONE, None])
            continue
        if isinstance(m, nn.Identity):
            continue
        code = _ACTS.get(type(m))
        if code is None:
            return None, 'layer %d (%s) is not a Linear or one of ReLU, LeakyReLU, PReLU, Tanh, Softplus' % (i, type(m).__name__)
        if not layers or layers[-1][1] != N.HYPER_ACT_NONE:
            return None, 'layer %d (%s) does not follow a Linear layer' % (i, type(m).__name__)
        if isinstance(m, nn.Softplus) and (float(m.beta) != 1.0 or float(m.threshold) != 20.0):
            return None, 'layer %d (Softplus): only beta 1, threshold 20 (got %g, %g)' % (i, m.beta, m.threshold)
        if isinstance(m, nn.PReLU) and m.num_parameters not in (1, layers[-1][0].out_features):
            return None, 'layer %d (PReLU): %d weights for %d channels' % (i, m.num_parameters, layers[-1][0].out_features)
        layers[-1][1], layers[-1][2] = code, m
    if not 2 <= len(layers) <= MAX_LAYERS:
        return None, 'g has %d Linear layers (2 .. %d supported)' % (len(layers), MAX_LAYERS)
    prev = 2 * dim + 1
    for j, (lin, _, _) in enumerate(layers):
        name = 'layer %d (Linear(%d, %d))' % (list(g).index(lin), lin.in_features, lin.out_features)
        if lin.in_features != prev:
            return None, '%s: input width %d, expected %s' % (name, lin.in_features, '2 * dim + 1 = %d' % prev if j == 0 else prev)
        if lin.out_features > MAX_WIDTH or lin.in_features > MAX_WIDTH:
            return None, '%s: width above %d' % (name, MAX_WIDTH)
        prev = lin.out_features
    if prev != dim:
        return None, 'last Linear layer has %d outputs, the state has %d' % (prev, dim)
    text = ' '.join('Linear(%d, %d)%s' % (l_.in_features, l_.out_features, '' if m is None else ' ' + type(m).__name__) for l_, _, m in layers)
    return {'layers': [tuple(x) for x in layers], 'text': text}, None


_WORKSPACES = {}


def _workspace(device):
    ws = _WORKSPACES.get(str(device))
    if ws is None:
        ws = torch.empty(N.HYPER_WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        _WORKSPACES[str(device)] = ws
    return ws


def _describe_f(f):
    if isinstance(f, R.DeviceRHS):
        return {'kind': type(f).__name__, 'dim': f.dim}
    return {'kind': 'callable', 'name': getattr(f, '__name__', type(f).__name__)}


def grad_tile_bytes(table, dtype):
    """LDS bytes of the gradient kernel's activation tiles for a `describe_g` table: the input [16][Kp + 1] and the pre-activation
    [16][Np + 1] of every layer and one cotangent tile [16][widest + 1] (csrc/mi_ode_hyper_grad.h: hyper_grad_layout)."""
    r16 = lambda n: (n + 15) // 16 * 16                                                              # noqa: E731
    elems, widest = 0, 16
    for lin, _, _ in table['layers']:
        kp, np_ = r16(lin.in_features), r16(lin.out_features)
        elems += 16 * (kp + 1) + 16 * (np_ + 1)
        widest = max(widest, kp, np_)
    elems += 16 * (widest + 1)
    return (elems + 1) // 2 * 2 * (8 if dtype == torch.float64 else 4) + 16


def _g_params(table):
    """g's parameters in layer order and, per layer, the indices (weight, bias | None, PReLU weight | None) into that list."""
    params, index = [], []
    for lin, _, act in table['layers']:
        row = [len(params), None, None]
        params.append(lin.weight)
        if lin.bias is not None:
            row[1] = len(params)
            params.append(lin.bias)
        if isinstance(act, nn.PReLU):
            row[2] = len(params)
            params.append(act.weight)
        index.append(tuple(row))
    return params, index


def describe_grad(f, g, mode, t_span, y, lower_mode='auto'):
    """The box of the fused gradient, a pure host function (CPU tensors are fine, nothing is compiled or launched): (plan, None) when the
    one-launch backward can differentiate this call, else (None, the limit that was hit).  mode: N.HYPER_TRAJECTORY (y: the state
    [batch, dim]) or N.HYPER_G_RESIDUALS (y: the base trajectory [T, batch, dim]).
    plan: {'source': the hyper-grad plugin's translation unit, 'g': describe_g's table, 'params', 'index': _g_params, 'low': the lowered f,
    'f_desc', 'tile_bytes'}."""
    if mode not in (N.HYPER_TRAJECTORY, N.HYPER_G_RESIDUALS):
        return None, 'residual_trajectory does not evaluate g: there is nothing to train'
    want = 2 if mode == N.HYPER_TRAJECTORY else 3
    if not isinstance(y, torch.Tensor) or y.dim() != want or y.dtype not in (torch.float32, torch.float64) or y.numel() == 0:
        return None, 'the state is not a non-empty %d-D float32 / float64 tensor' % want
    t_span = torch.as_tensor(t_span)
    if t_span.dim() != 1 or t_span.shape[0] < 2 or (mode != N.HYPER_TRAJECTORY and t_span.shape[0] != y.shape[0]):
        return None, 't_span must hold >= 2 times (one per row of the base trajectory)'
    if t_span.requires_grad:
        return None, 't_span requires grad (the fused gradient is with respect to g and y)'
    if mode == N.HYPER_G_RESIDUALS and y.requires_grad:
        return None, 'the base trajectory requires grad (the fused gradient of _hypersolver_residuals is with respect to g only)'
    state = (y if mode == N.HYPER_TRAJECTORY else y[0]).detach()
    dim = int(state.shape[-1])
    table, why = describe_g(g, dim)
    if table is None:
        return None, why
    params, index = _g_params(table)
    if any(p.device != y.device or p.dtype != y.dtype or not p.is_contiguous() for p in params):
        return None, "g's parameters are not contiguous %s tensors on %s (the state's)" % (y.dtype, y.device)
    tile = grad_tile_bytes(table, y.dtype)
    if tile > N.HYPER_GRAD_LDS_BYTES:
        return None, "g is beyond the size limit of the fused gradient: the input and the pre-activation of every layer for a tile of 16 " \
                     "rows take %d bytes of LDS, the limit is %d" % (tile, N.HYPER_GRAD_LDS_BYTES)
    f_desc = _describe_f(f)
    if isinstance(f, R.DeviceRHS):
        if type(f) not in (R.Lorenz, R.LotkaVolterra):
            return None, '%s has no vjp for the fused gradient (rhs.Lorenz, rhs.LotkaVolterra and lowered Python callables have)' % type(f).__name__
        if f.sign != 1.0:
            return None, 'f runs on a reversed time axis (sign %g)' % f.sign
        if f.dim != dim:
            return None, '%s is not a system of the state width %d' % (type(f).__name__, dim)
        func = f.forward                                 # (the traced equivalent: the same formulas, with a generated vjp)
    elif callable(f):
        if lower_mode is False or lower_mode == 'off':
            return None, 'f is a Python callable and lowering is off'
        if isinstance(f, nn.Module) and any(p.requires_grad for p in f.parameters()):
            return None, 'f closes over trainable tensors (its own parameters): the fused gradient is with respect to g and y'
        func = f
    else:
        return None, 'f is not callable'
    from . import lower as L
    try:
        low = L.lower(func, state)
        if low.kind != 'rowlocal' or tuple(low.state_shape) != tuple(state.shape):
            raise L.TraceError('the callable lowers to a %s program, not a row-local one' % low.kind)
        if L.vjp_params(low.trace)[1] or any(e_['t'].requires_grad for e_ in low.trace.tensors if isinstance(e_.get('t'), torch.Tensor)):
            return None, 'f closes over trainable tensors: the fused gradient is with respect to g and y'
        source = R.hyper_grad_source_of(L.discrete_source(low.trace))
    except Exception as e:
        return None, 'f was not lowered with a vjp: %s' % e
    if not isinstance(f, R.DeviceRHS):
        f_desc = dict(low.describe(), lowered=True)
    return {'source': source, 'g': table, 'params': params, 'index': index, 'low': low, 'f_desc': f_desc, 'tile_bytes': tile}, None


class _FusedGrad(torch.autograd.Function):
    """The forward kernel as it is; the backward is the one launch of csrc/mi_ode_hyper_grad.h."""

    @staticmethod
    def forward(ctx, solver, mode, t_span, y, plan, gplan, *params):
        out, n = solver._fused(mode, t_span, y, plan)
        ctx.solver, ctx.mode, ctx.gplan = solver, mode, gplan
        solver.last_stats = {'engine': 'fused', 'why': 'fused: one launch', 'n_launches': n, 'f': plan['f_desc'], 'g': plan['g']['text'],
                             'method': type(solver).__name__, 'grad': 'fused'}
        ctx.table = R.hyper_grad_plugin(gplan['source'], y.dtype)          # (compiled at the call, not in backward)
        low = gplan['low']
        ctx.scalars = list(low.rhs.params)
        ctx.pool = None if low.rhs.pool is None else low.rhs.pool.clone()  # (the program's pool is shared: the next call overwrites it)
        ctx.y_grad = mode == N.HYPER_TRAJECTORY and y.requires_grad
        ctx.p_grad = [p.requires_grad for p in params]
        ctx.save_for_backward(t_span, out if mode == N.HYPER_TRAJECTORY else y, *params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        saved = ctx.saved_tensors                        # (an in-place change of a parameter since the forward raises here)
        t_span, ys, params = saved[0], saved[1].detach().contiguous(), saved[2:]
        solver, gplan, mode = ctx.solver, ctx.gplan, ctx.mode
        dtype, device = ys.dtype, ys.device
        T, B, dim = (int(s_) for s_ in ys.shape)
        G = G.to(dtype).contiguous()
        tc = t_span.detach().contiguous()
        d = N.HyperGradDesc()
        d.dtype, d.method, d.mode = N.dtype_code(dtype), solver._method if mode == N.HYPER_TRAJECTORY else N.HYPER_EULER, mode
        d.batch, d.dim, d.T = B, dim, T
        work = B if mode == N.HYPER_TRAJECTORY else T * B
        cap = int(GRAD_GRID) if int(GRAD_GRID) > 0 else GRAD_DEFAULT_GRID
        grid = max(1, min((work + 15) // 16, cap, N.HYPER_GRAD_MAX_GRID))
        d.grid = grid
        d.t, d.ys, d.grad_out = tc.data_ptr(), ys.data_ptr(), G.data_ptr()
        gy = torch.empty((B, dim), dtype=dtype, device=device) if ctx.y_grad else None
        d.grad_y = gy.data_ptr() if gy is not None else None
        sizes = [p.numel() if need else 0 for p, need in zip(params, ctx.p_grad)]
        flat = torch.empty(max(sum(sizes), 1), dtype=dtype, device=device)
        grads, off = [], 0
        for p, n_ in zip(params, sizes):
            grads.append(flat[off:off + n_].view(p.shape) if n_ else None)
            off += n_
        layers = gplan['g']['layers']
        d.n_layers = len(layers)
        for j, ((lin, act, m), (iw, ib, ia)) in enumerate(zip(layers, gplan['index'])):
            L_ = d.layers[j]
            L_.in_, L_.out, L_.act = lin.in_features, lin.out_features, act
            L_.w = params[iw].data_ptr()
            L_.b = params[ib].data_ptr() if ib is not None else None
            if ia is not None:
                L_.alpha, L_.n_alpha = params[ia].data_ptr(), m.num_parameters
            elif isinstance(m, nn.LeakyReLU):
                L_.slope = float(m.negative_slope)
            d.grad_w[j] = grads[iw].data_ptr() if grads[iw] is not None else None
            d.grad_b[j] = grads[ib].data_ptr() if ib is not None and grads[ib] is not None else None
            d.grad_alpha[j] = grads[ia].data_ptr() if ia is not None and grads[ia] is not None else None
        d.rhs.kind, d.rhs.sign, d.rhs.plugin = N.RHS_PLUGIN, 1.0, ctx.table[1]
        for i, v in enumerate(ctx.scalars[:8]):
            d.rhs.scalars[i] = v
        if ctx.pool is not None:
            d.rhs.w[0] = ctx.pool.data_ptr()
        lib = N.load()
        nbytes = N.check(lib.mi_ode_hyper_grad_workspace_bytes(ctypes.byref(d)), 'mi_ode_hyper_grad_workspace_bytes')
        work_buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        ticket = torch.zeros(4, dtype=torch.int32, device=device)
        d.workspace, d.ticket = work_buf.data_ptr(), ticket.data_ptr()
        with torch.cuda.device(device):
            rc = lib.mi_ode_hyper_grad_run(ctypes.byref(d), N.stream_ptr(device))
        N.check(rc, 'mi_ode_hyper_grad_run')
        solver.last_backward_stats = {'engine': 'fused', 'n_launches': int(rc), 'grid': grid, 'why': 'fused: one launch for all steps and rows',
                                      'method': type(solver).__name__}
        del work_buf, ticket, G, tc                      # (stream-ordered: the caching allocator reuses the memory after the kernel)
        return (None, None, None, gy, None, None) + tuple(grads)


class AbstractHyperSolver(nn.Module):
    """base.py: `f` the ODE function, `g` the network that approximates the truncation error of the base method.
    options: {'lower': True | False | 'auto'} - trace a Python `f` onto a generated row-local kernel ('auto': odeint's LOWER_DEFAULT);
    {'grad': False | 'auto' | True} - train on the fused engine (default FUSED_GRAD; see the module's docstring)."""
    _method = None

    def __init__(self, func, hyper_solver, options=None):
        super(AbstractHyperSolver, self).__init__()
        self.f = func
        self.g = hyper_solver
        self.options = dict(options or {})
        if self.options.get('grad', False) not in (False, 'auto', True):
            raise ValueError("options['grad'] is False, 'auto' or True, not %r" % (self.options['grad'],))
        self.last_stats = {}
        self.last_backward_stats = {}

    def forward(self, t, y, dy):
        """g(cat([y, dy, t * ones(B, 1)], dim=1)) (base.py:27-41)."""
        t = torch.as_tensor(t, dtype=y.dtype, device=y.device)
        t = t * torch.ones((y.shape[0], 1) + tuple(y.shape[2:]), dtype=y.dtype, device=y.device)
        return self.g(torch.cat([y, dy, t], dim=1))

    def trajectory(self, t_span, y):
        return self._call(N.HYPER_TRAJECTORY, t_span, y)

    def residual_trajectory(self, t_span, base_traj):
        raise NotImplementedError()

    def _hypersolver_residuals(self, t_span, base_traj):
        """g at every row of a given trajectory: [T, B, d] (base.py:51-64)."""
        return self._call(N.HYPER_G_RESIDUALS, t_span, base_traj)

    # -- engines --------------------------------------------------------------------------------------------------------------
    def _call(self, mode, t_span, y):
        N.require_gpu_tensor(y, 'y' if mode == N.HYPER_TRAJECTORY else 'base_traj')
        t_span = torch.as_tensor(t_span).to(device=y.device, dtype=y.dtype)
        grad_opt = self.options.get('grad', FUSED_GRAD)
        if grad_opt is not False and self._needs_grad(t_span, y):
            out, why = self._call_fused_grad(mode, t_span, y)
            if out is not None:
                return out
            if grad_opt is True:
                raise ValueError("hypersolver(options={'grad': True}): the fused gradient does not take this call: %s" % why)
            out = self._eager(mode, t_span, y)
            self.last_stats = {'engine': 'eager', 'why': why, 'n_launches': None, 'f': _describe_f(self.f), 'g': self._g_text(y),
                               'method': type(self).__name__}
            return out
        plan, why = self._plan(mode, t_span, y)
        if plan is None:
            out = self._eager(mode, t_span, y)
            self.last_stats = {'engine': 'eager', 'why': why, 'n_launches': None, 'f': _describe_f(self.f), 'g': self._g_text(y),
                               'method': type(self).__name__}
            return out
        out, n = self._fused(mode, t_span, y, plan)
        self.last_stats = {'engine': 'fused', 'why': why, 'n_launches': n, 'f': plan['f_desc'], 'g': plan['g']['text'],
                           'method': type(self).__name__}
        return out

    def _g_text(self, y):
        dim = y.shape[-1] if y.dim() >= 1 else 0
        tab, why = describe_g(self.g, dim)
        return tab['text'] if tab is not None else why

    def _lower_mode(self):
        mode = self.options.get('lower', 'auto')
        if mode == 'auto':
            mode = importlib.import_module(__package__ + '.odeint').LOWER_DEFAULT
        return mode

    def _needs_grad(self, t_span, y):
        return torch.is_grad_enabled() and (y.requires_grad or t_span.requires_grad or any(p.requires_grad for p in self.g.parameters()) or
                                            (isinstance(self.f, nn.Module) and any(p.requires_grad for p in self.f.parameters())))

    def _call_fused_grad(self, mode, t_span, y):
        """(result, why) of a call that requires grad on the fused engine, or (None, the limit of the box that was hit)."""
        if isinstance(self.f, nn.Module) and any(p.requires_grad for p in self.f.parameters()):
            return None, 'f closes over trainable tensors (its own parameters): the fused gradient is with respect to g and y'
        gplan, why = describe_grad(self.f, self.g, mode, t_span, y, self._lower_mode())
        if gplan is None:
            return None, why
        with torch.no_grad():
            plan, why = self._plan(mode, t_span, y)
        if plan is None:
            return None, why
        out = _FusedGrad.apply(self, mode, t_span, y, plan, gplan, *gplan['params'])
        return out, None

    def _plan(self, mode, t_span, y):
        """(plan, why) for the fused engine, or (None, why not)."""
        state = y if mode == N.HYPER_TRAJECTORY else (y[0] if y.dim() == 3 else y)
        want = 2 if mode == N.HYPER_TRAJECTORY else 3
        if y.dim() != want or y.dtype not in (torch.float32, torch.float64) or y.numel() == 0:
            return None, 'the state is not a non-empty %d-D float32 / float64 tensor' % want
        if t_span.dim() != 1 or t_span.shape[0] < 2 or (mode != N.HYPER_TRAJECTORY and t_span.shape[0] != y.shape[0]):
            return None, 't_span must hold >= 2 times (one per row of the base trajectory)'
        dim = int(state.shape[-1])
        grad = torch.is_grad_enabled() and (y.requires_grad or t_span.requires_grad or any(p.requires_grad for p in self.g.parameters()) or
                                            (isinstance(self.f, nn.Module) and any(p.requires_grad for p in self.f.parameters())))
        if grad:
            return None, 'a result would require grad (training runs on autograd)'
        g = None
        if mode != N.HYPER_RESIDUAL:
            g, why = describe_g(self.g, dim)
            if g is None:
                return None, why
            for lin, _, act in g['layers']:
                ps = [lin.weight] + ([lin.bias] if lin.bias is not None else []) + ([act.weight] if isinstance(act, nn.PReLU) else [])
                if any(p.device != y.device or p.dtype != y.dtype or not p.is_contiguous() for p in ps):
                    return None, "g's parameters are not contiguous %s tensors on %s (the state's)" % (y.dtype, y.device)
        else:
            g = {'layers': [], 'text': ''}
        f = self.f
        f_desc = _describe_f(f)
        keep = []
        if isinstance(f, R.DeviceRHS):
            ok = f.row_local and f.dim == dim and f.sign == 1.0 and (
                f.kind in (N.RHS_LORENZ, N.RHS_LOTKA_VOLTERRA) or
                (f.kind in (N.RHS_LINEAR, N.RHS_CUBIC_LINEAR) and f.dim == 2 and getattr(f, 'b', None) is None) or
                (f.kind == N.RHS_PLUGIN and hasattr(f, 'hyper_plugin') and not getattr(f, 'coop', False)))
            if not ok:
                return None, '%s is not a row-local device system of the state width %d' % (type(f).__name__, dim)
            dev_rhs = f
        elif callable(f):
            lmode = self._lower_mode()
            if lmode is False or lmode == 'off':
                return None, 'f is a Python callable and lowering is off'
            from . import lower as L
            try:
                low = L.lower(f, state)
                if low.kind != 'rowlocal' or tuple(low.state_shape) != tuple(state.shape):
                    raise L.TraceError('the callable lowers to a %s program, not a row-local one' % low.kind)
            except Exception as e:
                if lmode is True:
                    raise ValueError("hypersolver(options={'lower': True}): f cannot be lowered onto a row-local kernel: %s" % e)
                return None, 'f was not lowered: %s' % e
            if torch.is_grad_enabled() and any(e_['t'].requires_grad for e_ in low.trace.tensors if isinstance(e_.get('t'), torch.Tensor)):
                return None, 'a result would require grad (f closes over trainable tensors)'
            dev_rhs = low.rhs
            f_desc = dict(low.describe(), lowered=True)
            keep.append(low)
        else:
            return None, 'f is not callable'
        return {'rhs': dev_rhs, 'g': g, 'f_desc': f_desc, 'keep': keep}, 'fused: one launch'

    def _fused(self, mode, t_span, y, plan):
        lib = N.load()
        dtype, device = y.dtype, y.device
        d = N.HyperDesc()
        d.dtype = N.dtype_code(dtype)
        d.method = self._method if mode == N.HYPER_TRAJECTORY else N.HYPER_EULER
        d.mode = mode
        if mode == N.HYPER_TRAJECTORY:
            B, dim, T = int(y.shape[0]), int(y.shape[1]), int(t_span.shape[0])
            out = torch.empty((T, B, dim), dtype=dtype, device=device)
        else:
            T, B, dim = (int(s) for s in y.shape)
            out = torch.empty((T - 1 if mode == N.HYPER_RESIDUAL else T, B, dim), dtype=dtype, device=device)
        yc = y.detach().contiguous()
        tc = t_span.detach().contiguous()
        keep = [yc, tc, out] + plan['keep']
        d.batch, d.dim, d.T = B, dim, T
        d.t, d.y, d.out = tc.data_ptr(), yc.data_ptr(), out.data_ptr()
        d.workspace = _workspace(device).data_ptr()
        rhs_obj = plan['rhs']
        if rhs_obj.kind == N.RHS_PLUGIN:                 # (the hyper plugin's table: the row-local plugin is not needed, nor compiled)
            d.rhs.kind, d.rhs.sign = N.RHS_PLUGIN, rhs_obj.sign
            for i, v in enumerate(list(rhs_obj.params)[:8]):
                d.rhs.scalars[i] = v
            pool = getattr(rhs_obj, 'pool', None)
            if pool is not None:
                d.rhs.w[0] = pool.data_ptr()
                keep.append(pool)
            hlib, table = rhs_obj.hyper_plugin(dtype)
            d.rhs.plugin = table
            keep.append(hlib)
        else:
            keep += rhs_obj.fill(d.rhs, dtype, device)
        layers = plan['g']['layers']
        d.n_layers = len(layers)
        for j, (lin, act, m) in enumerate(layers):
            L = d.layers[j]
            L.in_, L.out, L.act = lin.in_features, lin.out_features, act
            L.w = lin.weight.data_ptr()
            L.b = lin.bias.data_ptr() if lin.bias is not None else None
            if isinstance(m, nn.PReLU):
                L.alpha, L.n_alpha = m.weight.data_ptr(), m.num_parameters
            elif isinstance(m, nn.LeakyReLU):
                L.slope = float(m.negative_slope)
        rc = lib.mi_ode_hyper_run(ctypes.byref(d), N.stream_ptr(device))
        N.check(rc, 'mi_ode_hyper_run')
        del keep                                         # (stream-ordered: the caching allocator reuses the memory after the kernel)
        return out, int(rc)

    def _eager(self, mode, t_span, y):
        if mode == N.HYPER_TRAJECTORY:
            return self._eager_trajectory(t_span, y)
        dt = t_span[1] - t_span[0]
        if mode == N.HYPER_RESIDUAL:                     # euler.py:23-30
            fi = torch.stack([self.f(t_span[i], y[i]) for i in range(t_span.shape[0] - 1)])
            return (y[1:] - y[:-1] - dt * fi) / dt ** 2
        return torch.stack([self(dt, y[i], self.f(t_span[i], y[i])) for i in range(t_span.shape[0])])     # base.py:51-64

    def _eager_trajectory(self, t_span, y):
        raise NotImplementedError


class HyperEuler(AbstractHyperSolver):
    _method = N.HYPER_EULER

    def _eager_trajectory(self, t_span, y):
        traj = []
        dt = t_span[1] - t_span[0]
        for i in range(t_span.shape[0]):
            traj.append(y)
            if i == t_span.shape[0] - 1:
                break
            dy = self.f(t_span[i], y)
            y = y + dy * dt + (dt ** 2) * self(dt, y, dy)                                     # euler.py:16
        return torch.stack(traj)

    def residual_trajectory(self, t_span, base_traj):
        """(base[i+1] - base[i] - dt f(t_i, base[i])) / dt^2 for the T - 1 steps of a given trajectory (euler.py:20-30)."""
        return self._call(N.HYPER_RESIDUAL, t_span, base_traj)


class HyperMidpoint(AbstractHyperSolver):
    _method = N.HYPER_MIDPOINT

    def _eager_trajectory(self, t_span, y):
        traj = []
        dt = t_span[1] - t_span[0]
        for i in range(t_span.shape[0]):
            traj.append(y)
            if i == t_span.shape[0] - 1:
                break
            t = t_span[i]
            dy = self.f(t, y)
            y_mid = y + dy * dt / 2. + (dt ** 2) * self(dt, y, dy)                           # euler.py:46-48
            dy_2 = self.f(t + dt / 2., y_mid)
            y = y + dt * dy_2 + (dt ** 3) * self(dt, y_mid, dy_2)
        return torch.stack(traj)


class HyperHeun(AbstractHyperSolver):
    _method = N.HYPER_HEUN

    def _eager_trajectory(self, t_span, y):
        traj = []
        dt = t_span[1] - t_span[0]
        for i in range(t_span.shape[0]):
            traj.append(y)
            if i == t_span.shape[0] - 1:
                break
            t = t_span[i]
            dy = self.f(t, y)
            y2 = y + dy * dt + (dt ** 2) * self(dt, y, dy)                                     # euler.py:71-73
            dy_2 = self.f(t + dt, y2)
            y = y + dt / 2. * (dy + dy_2) + (dt ** 3) * self(dt, y2, dy_2)
        return torch.stack(traj)


def hyper_sources(f, y0, dtype=None):
    """The hyper plugin source(s) a call with this f and state would compile (build-time prebuilding; [] for catalogue systems)."""
    if isinstance(f, R.DeviceRHS):
        return [f.hyper_source(dtype or y0.dtype)] if hasattr(f, 'hyper_source') and f.kind == N.RHS_PLUGIN else []
    from . import lower as L
    return [R.hyper_source_of(s) for s in L.sources_for(f, y0)]


def hyper_grad_sources(f, y0, dtype=None):
    """The hyper-grad plugin source a fused backward with this f and state would compile (build-time prebuilding; [] outside the box)."""
    from . import lower as L
    state = y0.to(dtype) if dtype is not None else y0
    func = f.forward if type(f) in (R.Lorenz, R.LotkaVolterra) else f
    if isinstance(func, R.DeviceRHS) or not callable(func):
        return []
    tr = L.trace(func, state.detach())
    if L.program_for(tr).kind != 'rowlocal' or L.vjp_params(tr)[1]:
        return []
    return [R.hyper_grad_source_of(L.discrete_source(tr))]
