"""CPU tests of the hypersolvers (tfdiffeq_amd.hyper_solvers): the API surface of the reference's tfdiffeq/hyper_solvers/, the
descriptor of g, the refusal of host tensors, the hyper plugin build and the C entry point without a device.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest
import torch
from torch import nn

from tfdiffeq_amd import _native as N
from tfdiffeq_amd import hyper_solvers as H
from tfdiffeq_amd import rhs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def notebook_g():
    return nn.Sequential(nn.Linear(7, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 64), nn.PReLU(64), nn.Linear(64, 3))


def test_api_surface_matches_the_reference():
    import tfdiffeq_amd
    assert tfdiffeq_amd.hyper_solvers is H
    for name in ('AbstractHyperSolver', 'HyperEuler', 'HyperMidpoint', 'HyperHeun'):
        assert hasattr(H, name)
    for cls in (H.HyperEuler, H.HyperMidpoint, H.HyperHeun):
        assert issubclass(cls, H.AbstractHyperSolver) and issubclass(cls, nn.Module)
        for m in ('forward', 'trajectory', 'residual_trajectory', '_hypersolver_residuals'):
            assert callable(getattr(cls, m))
    f, g = rhs.Lorenz(), notebook_g()
    s = H.HyperEuler(f, g)
    assert s.f is f and s.g is g


def test_forward_concatenates_y_dy_then_time():
    """base.py:27-41: g sees cat([y, dy, t * ones(B, 1)], dim=1) - checked with an identity-like g on the host."""
    seen = []

    class Probe(nn.Module):
        def forward(self, x):
            seen.append(x)
            return x[:, :3]
    s = H.HyperHeun(rhs.Lorenz(), Probe())
    y = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    dy = 10 + y
    out = s(torch.tensor(0.25, dtype=torch.float64), y, dy)
    assert torch.equal(seen[0], torch.cat([y, dy, torch.full((2, 1), 0.25, dtype=torch.float64)], dim=1))
    assert torch.equal(out, y)


def test_midpoint_and_heun_have_no_residual_trajectory():
    for cls in (H.HyperMidpoint, H.HyperHeun):
        with pytest.raises(NotImplementedError):
            cls(rhs.Lorenz(), notebook_g()).residual_trajectory(torch.linspace(0, 1, 3), torch.zeros(3, 2, 3))


def test_g_descriptor_accepts_the_supported_stacks():
    tab, why = H.describe_g(notebook_g(), 3)
    assert why is None and len(tab['layers']) == 4 and all(a == N.HYPER_ACT_PRELU for _, a, _ in tab['layers'][:3])
    assert tab['layers'][3][1] == N.HYPER_ACT_NONE
    tab, why = H.describe_g(nn.Sequential(nn.Linear(7, 50), nn.Tanh(), nn.Linear(50, 3)), 3)
    assert why is None and [a for _, a, _ in tab['layers']] == [N.HYPER_ACT_TANH, N.HYPER_ACT_NONE]
    tab, why = H.describe_g(nn.Sequential(nn.Linear(5, 128), nn.Softplus(), nn.Linear(128, 128), nn.Softplus(), nn.Linear(128, 2)), 2)
    assert why is None and tab['layers'][1][1] == N.HYPER_ACT_SOFTPLUS
    tab, why = H.describe_g(nn.Sequential(nn.Linear(7, 20), nn.PReLU(), nn.Linear(20, 20), nn.LeakyReLU(0.1), nn.Linear(20, 20), nn.ReLU(),
                                          nn.Linear(20, 3)), 3)
    assert why is None


def test_g_descriptor_refuses_with_a_reason_naming_the_layer():
    _, why = H.describe_g(nn.Sequential(nn.Linear(6, 64), nn.Tanh(), nn.Linear(64, 3)), 3)
    assert 'layer 0' in why and 'input width 6' in why
    _, why = H.describe_g(nn.Sequential(nn.Linear(7, 129), nn.Tanh(), nn.Linear(129, 3)), 3)
    assert 'layer 0' in why and 'above 128' in why
    _, why = H.describe_g(nn.Sequential(*([nn.Linear(7, 7), nn.Tanh()] * 6 + [nn.Linear(7, 3)])), 3)
    assert '7 Linear layers' in why
    _, why = H.describe_g(nn.Sequential(nn.Linear(7, 64), nn.ELU(), nn.Linear(64, 3)), 3)
    assert 'layer 1 (ELU)' in why
    _, why = H.describe_g(nn.Linear(7, 3), 3)
    assert 'Linear' in why and 'nn.Sequential' in why


def test_host_tensors_are_refused():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    for cls in (H.HyperEuler, H.HyperMidpoint, H.HyperHeun):
        s = cls(rhs.Lorenz(), notebook_g().double())
        with pytest.raises(N.NativeError):
            s.trajectory(torch.linspace(0, 1, 5), torch.ones(2, 3, dtype=torch.float64))
        with pytest.raises(N.NativeError):
            s._hypersolver_residuals(torch.linspace(0, 1, 5), torch.ones(5, 2, 3, dtype=torch.float64))
    with pytest.raises(N.NativeError):
        H.HyperEuler(lambda t, y: -y, notebook_g()).residual_trajectory(torch.linspace(0, 1, 5), torch.ones(5, 2, 3))


def test_hyper_plugin_builds_and_exports_its_table():
    from tfdiffeq_amd import _plugin_build, plugin_examples
    f = plugin_examples.van_der_pol(5.0)
    src = f.hyper_source(torch.float64)
    assert '#include "mi_ode_hyper_plugin.h"' in src and 'MI_ODE_DEFINE_HYPER_PLUGIN(mi::RhsUser)' in src and 'k[1] = p[0]' in src
    path = _plugin_build.build(src)
    mtime = os.path.getmtime(path)
    assert _plugin_build.build(src) == path and os.path.getmtime(path) == mtime        # cache hit, no recompile
    lib, table = f.hyper_plugin(torch.float64)

    class Table(C.Structure):
        _fields_ = [('abi', C.c_int), ('dtype', C.c_int), ('dim', C.c_int), ('launch_traj', C.c_void_p), ('launch_resid', C.c_void_p)]
    tb = Table.from_address(table)
    assert tb.abi == 0x48590001 and tb.dtype == N.F64 and tb.dim == 2
    assert tb.launch_traj and tb.launch_resid
    assert not lib.mi_ode_hyper_plugin_get(N.F32)                                       # built for one dtype only


def test_hyper_run_without_a_device_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    lib = N.load()
    d = N.HyperDesc()
    assert lib.mi_ode_hyper_run(C.byref(d), None) == N.E_NODEVICE
    assert 'HIP device' in N.last_error()


def test_hyper_descriptor_layout_matches_the_header(tmp_path):
    """ctypes' HyperDesc / HyperLayer against the C compiler's view of include/mi_ode.h."""
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi_ode.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mi_ode_hyper), '
                   'sizeof(mi_ode_hyper_layer), offsetof(mi_ode_hyper, rhs), offsetof(mi_ode_hyper, layers)); return 0; }\n')
    exe = tmp_path / 'sz'
    subprocess.run(['cc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.HyperDesc), C.sizeof(N.HyperLayer), N.HyperDesc.rhs.offset, N.HyperDesc.layers.offset]
