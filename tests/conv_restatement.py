"""float64 numpy restatement of the reference's Conv2dODEFunc (tfdiffeq/models/conv_odenet.py), NCHW: the yardstick of
tests/test_conv_host.py and tests/test_gpu_conv_odenet.py.  The time channel is a real input channel (channel 0), zero padded in the
3x3 convolution like every other channel."""
import numpy as np


def params(func):
    """[(W [out, in, k, k], b [out])] of conv1..3 of a tfdiffeq_amd.models.Conv2dODEFunc, float64."""
    return [(c.weight.detach().double().cpu().numpy(), c.bias.detach().double().cpu().numpy()) for c in (func.conv1, func.conv2, func.conv3)]


def conv2d(x, W, b, pad):
    """x [B, Cin, H, W]; W [Cout, Cin, k, k]; zero padding `pad`; stride 1."""
    k = W.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    H, Wd = x.shape[2] + 2 * pad - k + 1, x.shape[3] + 2 * pad - k + 1
    out = np.zeros((x.shape[0], W.shape[0], H, Wd))
    for dy in range(k):
        for dx in range(k):
            out += np.einsum('bchw,oc->bohw', xp[:, :, dy:dy + H, dx:dx + Wd], W[:, :, dy, dx])
    return out + b[None, :, None, None]


def act(name, x):
    if name == 'relu':
        return np.maximum(x, 0.0)
    if name == 'tanh':
        return np.tanh(x)
    if name == 'softplus':
        return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))
    raise ValueError(name)


def f(p, t, y, activation='relu', time_dependent=False):
    """Conv2dODEFunc.forward(t, y) in float64; p = params(func)."""
    y = np.asarray(y, dtype=np.float64)

    def cat(x):
        return np.concatenate([np.full_like(x[:, :1], float(t)), x], axis=1) if time_dependent else x
    h = act(activation, conv2d(cat(y), p[0][0], p[0][1], 0))
    h = act(activation, conv2d(cat(h), p[1][0], p[1][1], 1))
    return conv2d(cat(h), p[2][0], p[2][1], 0)
