"""float64 numpy restatement of the reference's hypersolvers (tfdiffeq/hyper_solvers/base.py, euler.py): the yardstick of
tests/test_gpu_hyper_solvers.py.  g is given as a torch nn.Sequential and evaluated here in numpy float64."""
import numpy as np
import torch


def g_layers(seq):
    """[(W [out, in], b [out] | None, act name | None, alpha [n] | slope)] in float64."""
    out = []
    for m in seq:
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


def g_eval(layers, x):
    for W, b, act, a in layers:
        x = x @ W.T
        if b is not None:
            x = x + b
        if act == 'relu':
            x = np.maximum(x, 0.0)
        elif act in ('prelu', 'leaky'):
            x = np.where(x > 0, x, np.asarray(a) * x)
        elif act == 'tanh':
            x = np.tanh(x)
        elif act == 'softplus':
            x = np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
    return x


def hyper_g(layers, dt, y, dy):
    """base.py:27-41: g(concat([y, dy, t * ones]))."""
    return g_eval(layers, np.concatenate([y, dy, dt * np.ones((y.shape[0], 1))], axis=1))


def trajectory(method, f, layers, t, y0):
    """euler.py: HyperEuler / HyperMidpoint / HyperHeun .trajectory; row i = the state before step i."""
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y0, dtype=np.float64)
    dt = t[1] - t[0]
    traj = []
    for i in range(len(t)):
        traj.append(y)
        if i == len(t) - 1:
            break
        dy = f(t[i], y)
        if method == 'euler':
            y = y + dy * dt + dt ** 2 * hyper_g(layers, dt, y, dy)
        elif method == 'midpoint':
            y_mid = y + dy * dt / 2. + dt ** 2 * hyper_g(layers, dt, y, dy)
            dy2 = f(t[i] + dt / 2., y_mid)
            y = y + dt * dy2 + dt ** 3 * hyper_g(layers, dt, y_mid, dy2)
        else:
            y2 = y + dy * dt + dt ** 2 * hyper_g(layers, dt, y, dy)
            dy2 = f(t[i] + dt, y2)
            y = y + dt / 2. * (dy + dy2) + dt ** 3 * hyper_g(layers, dt, y2, dy2)
    return np.stack(traj)


def residual_trajectory(f, t, base):
    """euler.py:20-30 (HyperEuler)."""
    dt = t[1] - t[0]
    fi = np.stack([f(t[i], base[i]) for i in range(len(t) - 1)])
    return (base[1:] - base[:-1] - dt * fi) / dt ** 2


def hypersolver_residuals(f, layers, t, base):
    """base.py:51-64."""
    dt = t[1] - t[0]
    return np.stack([hyper_g(layers, dt, base[i], f(t[i], base[i])) for i in range(len(t))])


def lorenz(t, y, s=10., b=8. / 3., r=28.):
    return np.stack([s * (y[:, 1] - y[:, 0]), y[:, 0] * (r - y[:, 2]) - y[:, 1], y[:, 0] * y[:, 1] - b * y[:, 2]], axis=1)


def van_der_pol(t, y, mu=5.0):
    return np.stack([y[:, 1], mu * (1 - y[:, 0] * y[:, 0]) * y[:, 1] - y[:, 0]], axis=1)


def lorenz_torch(t, y):
    """A plain batched Python Lorenz callable (what tfdiffeq_amd.lower traces onto a generated row-local kernel)."""
    return torch.stack([10. * (y[..., 1] - y[..., 0]), y[..., 0] * (28. - y[..., 2]) - y[..., 1], y[..., 0] * y[..., 1] - 8. / 3. * y[..., 2]], dim=-1)
