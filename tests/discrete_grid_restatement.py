"""A taped restatement of the reference's fixed-grid solve on a grid of its own (options['step_size']): the yardstick of the own-grid
discrete-gradient tests.  Written from tfdiffeq/solvers.py:58-115 - the step-size grid with its clipped last point, the output loop and
_linear_interp with its two exact-hit returns - on top of tests/discrete_restatement.STEPS; it does NOT import the package under test.

    grid     niters = ceil((t[-1] - t[0]) / step_size + 1);  grid = arange(niters) * step_size + t[0];  a last point beyond t[-1] becomes t[-1]
    loop     for (t0, t1) in the grid's intervals:  y1 = step(t0, t1 - t0, y0);  while t1 >= t[j]:  output j = interp(t0, t1, y0, y1, t[j])
    interp   y0 if t == t0;  y1 if t == t1;  else y0 + ((y1 - y0) / (t1 - t0)) * (t - t0)

Times are used in the state dtype (solvers.py:84).  Autograd through `solve` gives the gradient of the discrete map, interpolation included.
"""
import math

import torch

from tests import discrete_restatement as DR


def grid_of(t, step_size, dtype):
    """solvers.py:58-71 on `t` in the state dtype."""
    tt = (t if isinstance(t, torch.Tensor) else torch.tensor(t, dtype=torch.float64)).detach().cpu().to(dtype)
    niters = int(math.ceil(float((tt[-1] - tt[0]) / step_size + 1)))
    grid = torch.arange(0, niters).to(dtype) * step_size + tt[0]
    if grid[-1] > tt[-1]:
        grid[-1] = tt[-1]
    assert bool(grid[0] == tt[0]) and bool(grid[-1] == tt[-1])                            # solvers.py:86
    return tt, grid


def assignment(t, step_size, dtype):
    """(grid, steps, weights): for every output j >= 1 the grid step the loop of solvers.py:93-100 interpolates it in, and the factor
    (t[j] - t0) / (t1 - t0) with which y1 enters it - 1.0 on an exact hit of t1, 0.0 on one of t0; entry 0 is (-1, 1.0): output 0 is y0."""
    tt, grid = grid_of(t, step_size, dtype)
    steps, weights = [-1], [1.0]
    j = 1
    for n in range(grid.shape[0] - 1):
        t0, t1 = grid[n], grid[n + 1]
        while j < tt.shape[0] and bool(t1 >= tt[j]):
            steps.append(n)
            weights.append(0.0 if bool(tt[j] == t0) else 1.0 if bool(tt[j] == t1) else float((tt[j] - t0) / (t1 - t0)))
            j += 1
    return grid, steps, weights


def solve(func, y0, t, method, step_size, time_dtype=None):
    """[len(t), *y0.shape] (a tuple of them for a tuple state), every op on the tape.  time_dtype: the dtype the grid is formed in when it
    is not the state's - a float64 restatement of a float32 solve walks the float32 solve's grid (its points are exact in float64)."""
    tensor_input = isinstance(y0, torch.Tensor)
    y = DR._tup(y0)
    f = (lambda t_, y_: (func(t_, y_[0]),)) if tensor_input else (lambda t_, y_: tuple(func(t_, y_)))
    tt, grid = grid_of(t, step_size, time_dtype or y[0].dtype)
    tt, grid = tt.to(device=y[0].device, dtype=y[0].dtype), grid.to(device=y[0].device, dtype=y[0].dtype)
    step = DR.STEPS[method]
    outs = [y]
    j = 1
    for n in range(grid.shape[0] - 1):
        t0, t1 = grid[n], grid[n + 1]
        y1 = step(f, t0, t1 - t0, y)
        while j < tt.shape[0] and bool(t1 >= tt[j]):
            if bool(tt[j] == t0):
                outs.append(y)
            elif bool(tt[j] == t1):
                outs.append(y1)
            else:
                outs.append(tuple(a + ((b - a) / (t1 - t0)) * (tt[j] - t0) for a, b in zip(y, y1)))
            j += 1
        y = y1
    assert j == tt.shape[0]
    out = tuple(torch.stack([s[c] for s in outs]) for c in range(len(y)))
    return out[0] if tensor_input else out


def gradients(func, params, y0, t, method, step_size, weights, time_dtype=None):
    """(solution, gradient at y0, gradients of params) of  sum_c sum(weights_c * solution_c);  DR.gradients for the own grid."""
    tensor_input = isinstance(y0, torch.Tensor)
    y0r = tuple(y.detach().clone().requires_grad_(True) for y in DR._tup(y0))
    sol = solve(func, y0r[0] if tensor_input else y0r, t, method, step_size, time_dtype)
    loss = sum((w * s).sum() for w, s in zip(DR._tup(weights), DR._tup(sol)))
    grads = torch.autograd.grad(loss, y0r + tuple(params), allow_unused=True)
    gy, gp = grads[:len(y0r)], grads[len(y0r):]
    return ([s.detach() for s in DR._tup(sol)], list(gy), list(gp))


def n_grid_steps(t, step_size, dtype):
    return int(grid_of(t, step_size, dtype)[1].shape[0]) - 1
