"""Conv2dODEFunc / Conv2dODENet / rhs.Conv2dODE on the host (tfdiffeq/models/conv_odenet.py): the torch modules against the float64
numpy restatement, the descriptor's refusals, the exported C entry point and the model plumbing.  No GPU needed."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_restatement as CR  # noqa: E402
from tfdiffeq_amd import _native as N  # noqa: E402
from tfdiffeq_amd import models, odeint, rhs  # noqa: E402


def _func(C_, F, aug, td, act, seed=0):
    torch.manual_seed(seed)
    fn = models.Conv2dODEFunc(C_, F, augment_dim=aug, time_dependent=td, non_linearity=act).double()
    with torch.no_grad():                      # non-trivial biases everywhere (torch's init keeps them small)
        for p in fn.parameters():
            p.mul_(2.0)
    return fn


@pytest.mark.parametrize('act', ['relu', 'softplus', 'tanh'])
@pytest.mark.parametrize('td', [False, True])
@pytest.mark.parametrize('aug', [0, 3])
@pytest.mark.parametrize('hw', [(5, 5), (1, 1)])
def test_module_forward_equals_restatement(act, td, aug, hw):
    fn = _func(2, 6, aug, td, act)
    y = torch.randn(3, 2 + aug, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = fn(torch.tensor(0.7, dtype=torch.float64), y).detach().numpy()
    ref = CR.f(CR.params(fn), 0.7, y.numpy(), act, td)
    assert got.shape == (3, 2 + aug) + hw
    assert np.max(np.abs(got - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))
    assert fn.nfe == 1


def test_time_channel_is_zero_padded_in_conv2():
    """At t = 0.7 the time channel's contribution to conv2 differs between border and interior pixels (the zero padding)."""
    fn = _func(1, 4, 0, True, 'relu')
    y = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    p = CR.params(fn)
    d = CR.f(p, 0.7, y.numpy(), 'relu', True) - CR.f(p, 0.0, y.numpy(), 'relu', True)
    assert abs(d[0, 0, 0, 0] - d[0, 0, 2, 2]) > 1e-6          # corner vs interior
    got = (fn(torch.tensor(0.7, dtype=torch.float64), y) - fn(torch.tensor(0.0, dtype=torch.float64), y)).detach()
    assert np.max(np.abs(got.numpy() - d)) <= 1e-13


def test_descriptor_refuses_host_tensors():
    fn = _func(2, 6, 0, False, 'relu')
    desc = fn.device_rhs()
    assert isinstance(desc, rhs.Conv2dODE) and desc.kind == 0 and desc.stage_rhs is desc
    with pytest.raises(N.NativeError, match='no CPU fallback'):
        desc(torch.tensor(0.0, dtype=torch.float64), torch.zeros(1, 2, 4, 4, dtype=torch.float64))
    # forward (the torch definition) is the module's function
    y = torch.randn(2, 2, 4, 4, dtype=torch.float64)
    assert torch.allclose(desc.forward(0.3, y), fn(0.3, y).detach(), rtol=0, atol=1e-14)


def test_descriptor_box_and_in_place_refresh():
    fn = _func(2, 6, 0, True, 'tanh')
    desc = fn.device_rhs()
    y = torch.zeros(1, 2, 3, 3, dtype=torch.float64)
    assert desc.in_box(y) == ''
    assert 'num_filters' in _func(2, 160, 0, False, 'relu').device_rhs().in_box(y)
    assert 'activation' in _func(2, 6, 0, False, 'elu').device_rhs().in_box(y)
    assert '16' in _func(14, 6, 3, False, 'relu').device_rhs().in_box(torch.zeros(1, 17, 3, 3, dtype=torch.float64))
    w2p = desc.w2p
    with torch.no_grad():
        fn.conv2.weight.data -= 0.5            # a hand-written optimizer step: no version bump on .data
    assert fn.device_rhs() is desc and desc.w2p is w2p
    W2 = fn.conv2.weight.detach()
    assert torch.equal(desc.w2p[4, :6, :6], W2[:, 1:, 1, 1].t())        # tap (1, 1): [in][out]
    assert torch.equal(desc.w2t[0], W2[:, 0, 0, 0])
    assert float(desc.w2p[:, 6:].abs().sum()) == 0.0


def test_conv_stage_symbol_exported():
    lib = N.load()
    assert hasattr(lib, 'mi_ode_conv_stage') and 'mi_ode_conv_stage' in N.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'mi_ode.h')).read()
    assert re.search(r'^int mi_ode_conv_stage\(', header, flags=re.M)
    assert lib.mi_ode_abi_version() == 13
    d = N.ConvDesc()
    assert lib.mi_ode_conv_stage(C.byref(d), None, None, 0, None, None, None, None, None, None) < 0      # null y0 / k_out refused
    assert C.sizeof(N.ConvDesc) == 4 * 4 + 8 + 8 + 4 * 4 + 7 * 8


def test_odeblock_is_conv_constructs_and_plan():
    fn = _func(3, 8, 2, False, 'relu')
    block = models.ODEBlock(fn, is_conv=True)
    assert block.channel_axis == 1 and block.is_conv
    p = odeint.plan(fn.device_rhs(), torch.zeros(2, 5, 6, 6, dtype=torch.float64), method='dopri5')
    assert p['family'] == 'conv2d' and p['fused_stage'] and 'k_conv_stage<double>' in p['kernel']
    assert p['odeblock'] == 'fused stage kernel'
    p = odeint.plan(fn.device_rhs(), torch.zeros(2, 5, 6, 6, dtype=torch.float64), method='dopri5', options={'graph': 'host'})
    assert p['engine'] == 'plane kernels' and 'DeviceControlledRK' not in p['kernel'], p      # the host loop: no stage hook
    p = odeint.plan(_func(3, 64, 2, False, 'relu').device_rhs(), torch.zeros(256, 5, 28, 28), method='dopri5')     # MNIST-sized: slower
    assert p['fused_stage'] and p['odeblock'].startswith('torch module')
    p = odeint.plan(_func(3, 200, 0, False, 'relu').device_rhs(), torch.zeros(2, 3, 6, 6), method='dopri5')
    assert not p['fused_stage'] and 'num_filters' in p['why']


def test_conv_odenet_out_strides_follow_tf_same():
    torch.manual_seed(0)
    for size, k, s in (((3, 5, 5), (1, 1), (1, 1)), ((3, 5, 5), (3, 3), (2, 2)), ((1, 28, 28), (3, 3), (2, 2)), ((2, 7, 6), (2, 2), (3, 3))):
        net = models.Conv2dODENet(size, 4, output_dim=2, out_kernel_size=k, out_strides=s)
        feats = torch.randn(2, size[0], size[1], size[2])
        out = net.output_layer(feats)
        assert tuple(out.shape) == (2, 2, -(-size[1] // s[0]), -(-size[2] // s[1]))
    # TF "same": the extra padding pixel goes after - a 2x2 kernel at stride 1 on a 3x3 image pads (0, 1)
    conv = models.Conv2dODENet((1, 3, 3), 2, output_dim=1, out_kernel_size=(2, 2)).output_layer
    with torch.no_grad():
        conv.weight.fill_(1.0)
        conv.bias.zero_()
    x = torch.arange(9.0).reshape(1, 1, 3, 3)
    assert conv(x)[0, 0].tolist() == [[8.0, 12.0, 7.0], [20.0, 24.0, 13.0], [13.0, 15.0, 8.0]]
