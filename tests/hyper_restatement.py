"""numpy restatement of the reference's hypersolvers (tfdiffeq/hyper_solvers/base.py, euler.py): the yardstick of
tests/test_gpu_hyper_solvers.py and tests/test_gpu_hyper_edges.py.  g is given as a torch nn.Sequential and evaluated here in numpy.

Everything runs in the dtype of its inputs (t, y0 / base): float64 by default, and in float32 every intermediate stays float32 - dt, dt / 2,
dt^2, dt^3 (as the products dt * dt, dt * dt * dt the kernel forms), the ones column, g's parameters, and the PReLU / LeakyReLU slope cast
the way the kernel casts it ((T)slope).  The layers may be given in any dtype: g_eval casts them to its input's."""
import numpy as np
import torch


def g_layers(seq):
    """[(W [out, in], b [out] | None, act name | None, alpha [n] | slope)] in float64 (a float32 module's values widened: see g_layers_f32)."""
    out = []
    for m in seq:
        if isinstance(m, torch.nn.Identity):
            continue
        if isinstance(m, torch.nn.Linear):
            out.append([m.weight.detach().double().cpu().numpy(), None if m.bias is None else m.bias.detach().double().cpu().numpy(), None, None])
        elif isinstance(m, torch.nn.PReLU):
            out[-1][2], out[-1][3] = 'prelu', m.weight.detach().double().cpu().numpy()
        elif isinstance(m, torch.nn.LeakyReLU):
            out[-1][2], out[-1][3] = 'leaky', float(m.negative_slope)
        elif isinstance(m, torch.nn.ReLU):
            out[-1][2] = 'relu'
        elif isinstance(m, torch.nn.Tanh):
            out[-1][2] = 'tanh'
        elif isinstance(m, torch.nn.Softplus):
            out[-1][2] = 'softplus'
        else:
            raise TypeError(type(m).__name__)
    return out


def g_layers_f32(seq):
    """g's layers rounded to float32 and widened again: what a float32 copy of `seq` holds, as float64 arrays (the LeakyReLU slope too,
    which the float32 kernel casts to float32)."""
    def r(v):
        return None if v is None else np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    return [[r(W), r(b), act, a if a is None else (float(np.float32(a)) if act == 'leaky' else r(a))] for W, b, act, a in g_layers(seq)]


def g_eval(layers, x, pre=None):
    """g on the rows of x, in x's dtype.  pre: a list that receives every layer's pre-activations (the admission checks of the cases)."""
    dtype = x.dtype
    for W, b, act, a in layers:
        x = x @ np.asarray(W, dtype=dtype).T
        if b is not None:
            x = x + np.asarray(b, dtype=dtype)
        if pre is not None:
            pre.append((act, x))
        if act == 'relu':
            x = np.maximum(x, dtype.type(0))
        elif act in ('prelu', 'leaky'):
            x = np.where(x > 0, x, np.asarray(a, dtype=dtype) * x)
        elif act == 'tanh':
            x = np.tanh(x)
        elif act == 'softplus':
            x = np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, dtype.type(20)))))
        assert x.dtype == dtype
    return x


def hyper_g(layers, dt, y, dy, pre=None):
    """base.py:27-41: g(concat([y, dy, t * ones]))."""
    return g_eval(layers, np.concatenate([y, dy, dt * np.ones((y.shape[0], 1), dtype=y.dtype)], axis=1), pre)


def _typed(t, y, dtype):
    dtype = np.dtype(dtype if dtype is not None else np.float64)
    return np.asarray(t, dtype=dtype), np.asarray(y, dtype=dtype)


def trajectory(method, f, layers, t, y0, dtype=None, pre=None):
    """euler.py: HyperEuler / HyperMidpoint / HyperHeun .trajectory; row i = the state before step i.  dtype: float64 unless given."""
    t, y = _typed(t, y0, dtype)
    dt = t[1] - t[0]
    dt2, dt3, two = dt * dt, dt * dt * dt, t.dtype.type(2)
    traj = []
    for i in range(len(t)):
        traj.append(y)
        if i == len(t) - 1:
            break
        dy = f(t[i], y)
        if method == 'euler':
            y = y + dy * dt + dt2 * hyper_g(layers, dt, y, dy, pre)
        elif method == 'midpoint':
            y_mid = y + dy * dt / two + dt2 * hyper_g(layers, dt, y, dy, pre)
            dy2 = f(t[i] + dt / two, y_mid)
            y = y + dt * dy2 + dt3 * hyper_g(layers, dt, y_mid, dy2, pre)
        else:
            y2 = y + dy * dt + dt2 * hyper_g(layers, dt, y, dy, pre)
            dy2 = f(t[i] + dt, y2)
            y = y + dt / two * (dy + dy2) + dt3 * hyper_g(layers, dt, y2, dy2, pre)
        assert y.dtype == t.dtype
    return np.stack(traj)


def residual_trajectory(f, t, base, dtype=None):
    """euler.py:20-30 (HyperEuler)."""
    t, base = _typed(t, base, dtype)
    dt = t[1] - t[0]
    fi = np.stack([f(t[i], base[i]) for i in range(len(t) - 1)])
    out = (base[1:] - base[:-1] - dt * fi) / (dt * dt)
    assert out.dtype == t.dtype
    return out


def hypersolver_residuals(f, layers, t, base, dtype=None, pre=None):
    """base.py:51-64."""
    t, base = _typed(t, base, dtype)
    dt = t[1] - t[0]
    return np.stack([hyper_g(layers, dt, base[i], f(t[i], base[i]), pre) for i in range(len(t))])


def lorenz(t, y, s=10., b=8. / 3., r=28.):
    return np.stack([s * (y[:, 1] - y[:, 0]), y[:, 0] * (r - y[:, 2]) - y[:, 1], y[:, 0] * y[:, 1] - b * y[:, 2]], axis=1)


def van_der_pol(t, y, mu=5.0):
    return np.stack([y[:, 1], mu * (1 - y[:, 0] * y[:, 0]) * y[:, 1] - y[:, 0]], axis=1)


def lotka_volterra(t, y, a=1.5, b=1.0, c=3.0, d=1.0):
    """rhs.LotkaVolterra (RhsLotkaVolterra's operation order)."""
    u, v = y[:, 0], y[:, 1]
    return np.stack([a * u - b * u * v, -c * v + d * u * v], axis=1)


def linear2(W):
    """rhs.Linear with a bias-free 2 x 2 W: y @ W in RhsLinear2's order."""
    def f(t, y):
        w = np.asarray(W, dtype=y.dtype)
        return np.stack([y[:, 0] * w[0, 0] + y[:, 1] * w[1, 0], y[:, 0] * w[0, 1] + y[:, 1] * w[1, 1]], axis=1)
    return f


def cubic2(W):
    """rhs.CubicLinear with a 2 x 2 W: (y ** 3) @ W in RhsCubic2's order."""
    def f(t, y):
        w = np.asarray(W, dtype=y.dtype)
        c0, c1 = y[:, 0] * y[:, 0] * y[:, 0], y[:, 1] * y[:, 1] * y[:, 1]
        return np.stack([c0 * w[0, 0] + c1 * w[1, 0], c0 * w[0, 1] + c1 * w[1, 1]], axis=1)
    return f


def forced_oscillator(t, y, amp=0.7, w=2.0):
    """plugin_examples.forced_oscillator: y'' + y = amp cos(w t).  The time and the parameters in the state dtype, as the functor has them."""
    T = y.dtype.type
    return np.stack([y[:, 1], T(amp) * np.cos(T(w) * T(t)) - y[:, 0]], axis=1)


def forced_ring(D, p=(0.8, 1.7, 0.3)):
    """The time-dependent CustomRowLocal family of tests/hyper_cases.py at width D:
    k[i] = p[0] cos(p[1] t + i) - y[i] + p[2] y[(i + 1) % D] y[(i + D - 1) % D]."""
    def f(t, y):
        T = y.dtype.type
        i = np.arange(D, dtype=y.dtype)
        return T(p[0]) * np.cos(T(p[1]) * T(t) + i) - y + T(p[2]) * np.roll(y, -1, axis=1) * np.roll(y, 1, axis=1)
    return f


def forced_oscillator_torch(t, y):
    """The forced oscillator as a plain Python callable that uses t (lowered onto a generated row-local kernel)."""
    return torch.stack([y[..., 1], 0.7 * torch.cos(2.0 * t) - y[..., 0]], dim=-1)


def lorenz_torch(t, y):
    """A plain batched Python Lorenz callable (what tfdiffeq_amd.lower traces onto a generated row-local kernel)."""
    return torch.stack([10. * (y[..., 1] - y[..., 0]), y[..., 0] * (28. - y[..., 2]) - y[..., 1], y[..., 0] * y[..., 1] - 8. / 3. * y[..., 2]], dim=-1)
