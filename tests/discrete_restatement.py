"""A taped restatement of the reference's four fixed-grid step functions on the default grid, in plain torch ops: the yardstick of the
discrete-gradient tests.  Written from tfdiffeq/fixed_grid.py:6-42 and rk_common.py:73-81; it does NOT import the package under test.

    euler     y + h f(t, y)
    midpoint  y + h f(t + h / 2, y + (h / 2) f(t, y))
    heun      y + (h / 2) (f(t, y) + f(t + h, y + h f(t, y)))
    rk4       the 3/8 rule: k1 = f(t, y), k2 = f(t + h / 3, y + h k1 / 3), k3 = f(t + 2 h / 3, y + h (k2 - k1 / 3)),
              k4 = f(t + h, y + h (k1 - k2 + k3)),  y + h (k1 + 3 (k2 + k3) + k4) / 8

The default grid: the steps are the intervals of `t` itself, every grid point is an output (solvers.py:82-104 with grid_constructor =
lambda f, y0, t: t).  States are tensors or tuples of tensors; autograd through `solve` gives the gradient of the discrete map.
"""
import torch

STAGES = {'euler': 1, 'midpoint': 2, 'heun': 2, 'huen': 2, 'rk4': 4}


def _tup(y):
    return (y,) if isinstance(y, torch.Tensor) else tuple(y)


def _axpy(y, pairs):
    """y + sum c_i k_i, componentwise over tuples."""
    out = []
    for c, y_ in enumerate(y):
        acc = y_
        for coef, k in pairs:
            acc = acc + coef * k[c]
        out.append(acc)
    return tuple(out)


def euler_step(f, t, h, y):
    return _axpy(y, [(h, f(t, y))])


def midpoint_step(f, t, h, y):
    k1 = f(t, y)
    return _axpy(y, [(h, f(t + h / 2, _axpy(y, [(h / 2, k1)])))])


def heun_step(f, t, h, y):
    k1 = f(t, y)
    k2 = f(t + h, _axpy(y, [(h, k1)]))
    return _axpy(y, [(h / 2, k1), (h / 2, k2)])


def rk4_step(f, t, h, y):
    k1 = f(t, y)
    k2 = f(t + h / 3, _axpy(y, [(h / 3, k1)]))
    k3 = f(t + 2 * h / 3, _axpy(y, [(-h / 3, k1), (h, k2)]))
    k4 = f(t + h, _axpy(y, [(h, k1), (-h, k2), (h, k3)]))
    return _axpy(y, [(h / 8, k1), (3 * h / 8, k2), (3 * h / 8, k3), (h / 8, k4)])


STEPS = {'euler': euler_step, 'midpoint': midpoint_step, 'heun': heun_step, 'huen': heun_step, 'rk4': rk4_step}


def solve(func, y0, t, method):
    """[len(t), *y0.shape] (a tuple of them for a tuple state), every op on the tape.  func(t, y) sees what the caller's y0 is (tensor or
    tuple); t is used in the state dtype, as the solvers do."""
    tensor_input = isinstance(y0, torch.Tensor)
    y = _tup(y0)
    f = (lambda t_, y_: (func(t_, y_[0]),)) if tensor_input else (lambda t_, y_: tuple(func(t_, y_)))
    tt = torch.as_tensor(t).to(device=y[0].device, dtype=y[0].dtype)
    step = STEPS[method]
    traj = [y]
    for n in range(tt.shape[0] - 1):
        y = step(f, tt[n], tt[n + 1] - tt[n], y)
        traj.append(y)
    out = tuple(torch.stack([s[c] for s in traj]) for c in range(len(y)))
    return out[0] if tensor_input else out


def gradients(func, params, y0, t, method, weights):
    """(solution, gradient at y0, gradients of params) of  sum_c sum(weights_c * solution_c)  - a loss with a nonzero gradient at EVERY
    grid point.  y0 / weights: tensors or tuples alike."""
    tensor_input = isinstance(y0, torch.Tensor)
    y0r = tuple(y.detach().clone().requires_grad_(True) for y in _tup(y0))
    sol = solve(func, y0r[0] if tensor_input else y0r, t, method)
    loss = sum((w * s).sum() for w, s in zip(_tup(weights), _tup(sol)))
    grads = torch.autograd.grad(loss, y0r + tuple(params), allow_unused=True)
    gy, gp = grads[:len(y0r)], grads[len(y0r):]
    return ([s.detach() for s in _tup(sol)], list(gy), list(gp))


def rel_max(got, ref):
    """The metric of the discrete-gradient tests, per tensor: max |got - ref| / max |ref|."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, 'shape %s vs %s' % (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / ref.abs().max())


EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


def ceiling32(n_steps, method):
    """tests/bands.case_ceiling(attempts=n_steps, stages=2 x stages of the method) - the forward and the transposed evaluation of every
    stage - with its 4e-6 floor; restated here so that the expression is in one place with its float64 twin."""
    from tests import bands
    return bands.case_ceiling(attempts=n_steps, stages=2 * STAGES[method])


def ceiling64(n_steps, method):
    """The same expression with eps64 = 2^-53, the floor scaled by 2^-29 (= eps64 / eps32)."""
    return max(4e-6 * 2.0 ** -29, 8.0 * EPS64 * 2 * STAGES[method] * max(int(n_steps), 1))
