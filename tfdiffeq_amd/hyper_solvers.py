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
"""
import ctypes
import importlib

import torch
from torch import nn

from . import _native as N
from . import rhs as R

MAX_LAYERS = N.HYPER_MAX_LAYERS
MAX_WIDTH = 128

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


class AbstractHyperSolver(nn.Module):
    """base.py: `f` the ODE function, `g` the network that approximates the truncation error of the base method.
    options: {'lower': True | False | 'auto'} - trace a Python `f` onto a generated row-local kernel ('auto': odeint's LOWER_DEFAULT)."""
    _method = None

    def __init__(self, func, hyper_solver, options=None):
        super(AbstractHyperSolver, self).__init__()
        self.f = func
        self.g = hyper_solver
        self.options = dict(options or {})
        self.last_stats = {}

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
