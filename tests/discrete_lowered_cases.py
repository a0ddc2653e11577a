"""The callables of the lowered discrete-sweep tests (tests/test_discrete_lowered_host.py, tests/test_gpu_discrete_lowered.py), shared with
`__graft_entry__.build()`, which compiles their discrete plugins ahead of the GPU tests - as tests/lower_cases.py is shared.

SYSTEMS: name -> make(device, dtype, seed=0) -> (func, params, y0).  Everything is built in float64 from a seeded generator and cast, so
the float32 case and its float64 twin see the same numbers.  `params` is what `odeint_discrete` finds by itself (the grad-requiring
leaves of the callable, a module's parameters), in its order.
"""
import torch


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _leaf(x, device, dtype):
    return x.to(device=device, dtype=dtype).requires_grad_(True)


def spiral(device, dtype, seed=0, batch=300):
    """Components of y0 uniform in [-0.5, 0.5], so |y0| <= 0.71: with |A| = 2.1 a step of h <= 1 then moves a state by at most
    h |A| |y|^3 <= 1.05 |y|, about its own size, and every method on every grid of the tests stays bounded.  (Unbounded normal draws do
    not: from |y0| = 2.1 four Heun steps of 0.125 reach 1e99, the gradient 1e102, and ONE ulp on y0 moves the float64 restatement's own
    gradient by 4.9e-13 of its size, 34 times ceiling64 - a yardstick that no evaluation order can meet.)"""
    g = torch.Generator().manual_seed(100 + seed)
    A = _leaf(torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], dtype=torch.float64) + 0.05 * _rand(g, 2, 2), device, dtype)
    y0 = (torch.rand(batch, 2, generator=g, dtype=torch.float64) - 0.5).to(device=device, dtype=dtype)
    return (lambda t, y: (y ** 3) @ A), (A,), y0


def tanh8(device, dtype, seed=0, batch=300):
    g = torch.Generator().manual_seed(200 + seed)
    A = _leaf(_rand(g, 8, 8) / 8 ** 0.5, device, dtype)
    b = _leaf(0.1 * _rand(g, 8), device, dtype)
    y0 = _rand(g, batch, 8).to(device=device, dtype=dtype)
    return (lambda t, y: torch.tanh(y @ A + b) - 0.5 * y), (A, b), y0


def demo_net(device, dtype, seed=0, state=(20, 1, 2)):
    torch.manual_seed(300 + seed)
    net = torch.nn.Sequential(torch.nn.Linear(2, 50), torch.nn.Tanh(), torch.nn.Linear(50, 2)).double()
    g = torch.Generator().manual_seed(300 + seed)
    y0 = (_rand(g, *state) * 0.8).to(device=device, dtype=dtype)
    net = net.to(device=device, dtype=dtype)

    class Demo(torch.nn.Module):
        def __init__(self):
            super(Demo, self).__init__()
            self.net = net

        def forward(self, t, y):
            return self.net(y ** 3)
    f = Demo()
    return f, tuple(f.parameters()), y0


def scalars(device, dtype, seed=0, batch=70):
    g = torch.Generator().manual_seed(400 + seed)
    a = _leaf(torch.tensor(0.8, dtype=torch.float64), device, dtype)
    c = _leaf(torch.tensor([0.5, 0.3, 0.7], dtype=torch.float64) + 0.05 * _rand(g, 3), device, dtype)
    w = (1.0 + 0.2 * _rand(g, 3)).to(device=device, dtype=dtype)
    y0 = _rand(g, batch, 3).to(device=device, dtype=dtype)
    return (lambda t, y: a * torch.sin(y * w) * t - c * y + torch.cos(t)), (a, c), y0


def lorenz(device, dtype, seed=0):
    sigma = _leaf(torch.tensor(10.0, dtype=torch.float64), device, dtype)
    rho = _leaf(torch.tensor(28.0, dtype=torch.float64), device, dtype)
    beta = _leaf(torch.tensor(8.0 / 3.0, dtype=torch.float64), device, dtype)
    g = torch.Generator().manual_seed(500 + seed)
    y0 = (torch.tensor([1., 1., 1.], dtype=torch.float64) + 0.1 * _rand(g, 3)).to(device=device, dtype=dtype)

    def f(t, y):
        return torch.stack([sigma * (y[1] - y[0]), y[0] * (rho - y[2]) - y[1], y[0] * y[1] - beta * y[2]])
    return f, (sigma, rho, beta), y0


SYSTEMS = {'spiral': spiral, 'tanh8': tanh8, 'demo_net': demo_net, 'scalars': scalars, 'lorenz': lorenz}
# the interval each system is integrated over (Lorenz grows fast), and the float32 exceptions (a single rk4 step of (y ** 3) @ A over
# [0, 1] takes up to half of the float32 ceiling in the float32 restatement itself)
T_END = {'spiral': 1.0, 'tanh8': 1.0, 'demo_net': 1.0, 'scalars': 1.0, 'lorenz': 0.1}
T_END32 = {'spiral': 0.5}


def t_end(name, dtype):
    return T_END32.get(name, T_END[name]) if dtype == torch.float32 else T_END[name]


def tanh8_batch(batch):
    def make(device, dtype, seed=0):
        return tanh8(device, dtype, seed, batch=batch)
    return make


def interleave_b(device, dtype, seed=0):
    """The code of `scalars` with other parameter values: the same program, another call."""
    return scalars(device, dtype, seed=seed + 17)


def refused_transposed(device, dtype, seed=0):
    """`y @ W.t()`: the trace sees the derived tensor W.t(), not the leaf."""
    g = torch.Generator().manual_seed(600 + seed)
    W = _leaf(_rand(g, 3, 3) * 0.4, device, dtype)
    y0 = _rand(g, 40, 3).to(device=device, dtype=dtype)
    return (lambda t, y: torch.tanh(y @ W.t())), (W,), y0


def refused_tuple(device, dtype, seed=0):
    g = torch.Generator().manual_seed(700 + seed)
    c = _leaf(torch.tensor([0.5, 0.3, 0.7], dtype=torch.float64), device, dtype)
    y0 = (_rand(g, 10, 3).to(device=device, dtype=dtype), _rand(g, 10, 3).to(device=device, dtype=dtype))
    return (lambda t, y: (-c * y[0], -c * y[1])), (c,), y0


def rel(got, ref):
    """discrete_restatement.rel_max per tensor.  Where the reference gradient is exactly zero (one Euler step from t = 0 of a term that
    carries a factor t: `a` of `scalars`) that metric is 0 / 0; the gradient under test must then be exactly zero as well."""
    import discrete_restatement as DR
    if float(ref.abs().max()) == 0.0:
        assert float(got.detach().abs().max()) == 0.0, got
        return 0.0
    return DR.rel_max(got, ref)


def discrete_sources(device='cpu'):
    """The discrete plugin sources the GPU tests compile (tracing needs no GPU), both dtypes."""
    from tfdiffeq_amd import lower
    out = []
    for dtype in (torch.float64, torch.float32):
        for make in list(SYSTEMS.values()) + [tanh8_batch(1100), interleave_b]:
            f, _params, y0 = make(device, dtype)
            src = lower.discrete_source(lower.trace(f, y0))
            if src not in out:
                out.append(src)
    return out
