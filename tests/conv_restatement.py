"""float64 numpy restatement of the reference's Conv2dODEFunc (tfdiffeq/models/conv_odenet.py), NCHW: the yardstick of
tests/test_conv_host.py, tests/test_gpu_conv_odenet.py and tests/test_gpu_conv_edges.py.  The time channel is a real input channel
(channel 0), zero padded in the 3x3 convolution like every other channel.

`f32` is the same three convolutions with every array and every accumulation in numpy.float32 (the float32 oracle run, E32 of
tests/conv_cases.py).  `f(..., defect=...)` are restatements made WRONG on purpose - the three border / padding mistakes a tiled kernel
can make - so that tests/test_conv_cases_host.py can show that every case tells each of them from rounding:
    'time_taps_unclipped'   the time channel contributes all nine taps of conv2 at every pixel (it is not zero padded)
    'halo_is_act_b1'        conv2 sees act(conv1(0)) instead of 0 outside the image
    'drop_last_block'       the last 16 of conv2's Fp (F padded to a multiple of 16) input channels contribute nothing"""
import numpy as np

DEFECTS = ('time_taps_unclipped', 'halo_is_act_b1', 'drop_last_block')


def params(func):
    """[(W [out, in, k, k], b [out])] of conv1..3 of a tfdiffeq_amd.models.Conv2dODEFunc, float64."""
    return [(c.weight.detach().double().cpu().numpy(), c.bias.detach().double().cpu().numpy()) for c in (func.conv1, func.conv2, func.conv3)]


def conv2d_padded(xp, W, b):
    """xp [B, Cin, H + k - 1, W + k - 1] already padded; W [Cout, Cin, k, k]; stride 1.  In xp's dtype throughout."""
    k = W.shape[-1]
    H, Wd = xp.shape[2] - k + 1, xp.shape[3] - k + 1
    out = np.zeros((xp.shape[0], W.shape[0], H, Wd), dtype=xp.dtype)
    for dy in range(k):
        for dx in range(k):
            out += np.einsum('bchw,oc->bohw', xp[:, :, dy:dy + H, dx:dx + Wd], W[:, :, dy, dx], optimize=True)
    return out + b[None, :, None, None]


def conv2d(x, W, b, pad):
    """x [B, Cin, H, W]; W [Cout, Cin, k, k]; zero padding `pad`; stride 1."""
    return conv2d_padded(np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad))), W, b)


def act(name, x):
    if name == 'relu':
        return np.maximum(x, x.dtype.type(0))
    if name == 'tanh':
        return np.tanh(x)
    if name == 'softplus':
        c = x.dtype.type(20)
        return np.where(x > c, x, np.log1p(np.exp(np.minimum(x, c))))
    raise ValueError(name)


def _f(p, t, y, activation, time_dependent, dtype, defect=None):
    assert defect is None or defect in DEFECTS, defect
    dtype = np.dtype(dtype)
    y = np.asarray(y, dtype=dtype)
    p = [(W.astype(dtype), b.astype(dtype)) for W, b in p]
    tt = dtype.type(t)
    td = 1 if time_dependent else 0

    def cat(x):
        return np.concatenate([np.full_like(x[:, :1], tt), x], axis=1) if time_dependent else x
    h = act(activation, conv2d(cat(y), p[0][0], p[0][1], 0))
    xp = np.pad(cat(h), ((0, 0), (0, 0), (1, 1), (1, 1)))
    if defect == 'time_taps_unclipped' and time_dependent:
        xp[:, 0] = tt
    if defect == 'halo_is_act_b1':
        outside = act(activation, conv2d(cat(np.zeros((1, y.shape[1], 1, 1), dtype=dtype)), p[0][0], p[0][1], 0))[0, :, 0, 0]
        border = np.ones(xp.shape[2:], dtype=bool)
        border[1:-1, 1:-1] = False
        xp[:, td:][:, :, border] = outside[None, :, None]
    if defect == 'drop_last_block':
        F = h.shape[1]
        xp[:, td + (F + 15) // 16 * 16 - 16:] = 0
    h = act(activation, conv2d_padded(xp, p[1][0], p[1][1]))
    return conv2d(cat(h), p[2][0], p[2][1], 0)


def f(p, t, y, activation='relu', time_dependent=False, defect=None):
    """Conv2dODEFunc.forward(t, y) in float64; p = params(func)."""
    return _f(p, t, y, activation, time_dependent, np.float64, defect)


def f32(p, t, y, activation='relu', time_dependent=False):
    """The same in float32: weights, state, time, every product and every sum."""
    return _f(p, t, y, activation, time_dependent, np.float32)
