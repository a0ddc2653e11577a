"""Mirror of tfdiffeq/models/conv_odenet.py for torch: Conv2dTime, Conv2dODEFunc, Conv2dODENet (re-exported by `models`).

Layout: NCHW - channels first, torch's nn.Conv2d convention and that of the augmented-neural-odes code the reference ports.  That is
the one deliberate difference from the reference's Keras default (channels last): images are [batch, channels, height, width] and
the time channel and the augmentation channels are concatenated along dim 1.

Inference of `ODEBlock(Conv2dODEFunc(...), is_conv=True)` runs every Runge-Kutta stage as ONE launch of the fused stage kernel
(`rhs.Conv2dODE`, csrc/mi_ode_conv.h) when the function is inside its box (C + augment_dim <= 16, num_filters <= 128, relu / softplus /
tanh, float32 / float64) and the shape is one where that measured faster than torch (rhs.Conv2dODE.FUSED_MAX_CONV2_FLOP); training runs
`odeint_adjoint` with autograd over these torch modules.
"""
import torch
from torch import nn
from torch.nn import functional as F_

from . import rhs as _rhs

_ACTS = {'relu': nn.ReLU, 'softplus': nn.Softplus, 'tanh': nn.Tanh}


class _Activation(nn.Module):
    """torch.nn.functional.<name> as a module (what Keras' Activation('name') gives the reference)."""

    def __init__(self, name):
        super(_Activation, self).__init__()
        self.name = name

    def forward(self, x):
        return getattr(F_, self.name)(x)


class Conv2dTime(nn.Module):
    """A 2d convolution with the time prepended as input channel 0 (conv_odenet.py:12-44): concat([t * ones, x], dim=1), then convolve.
    `padding=1` means "same" (as in the reference), anything else "valid".  `transpose=True` uses nn.ConvTranspose2d."""

    def __init__(self, in_channels, dim_out, kernel_size=3, stride=1, padding=0, dilation=1, bias=True, transpose=False):
        super(Conv2dTime, self).__init__()
        module = nn.ConvTranspose2d if transpose else nn.Conv2d
        pad = dilation * (kernel_size - 1) // 2 if padding == 1 else 0
        self._layer = module(in_channels + 1, dim_out, kernel_size=kernel_size, stride=stride, padding=pad, dilation=dilation, bias=bias)

    @property
    def weight(self):
        return self._layer.weight

    @property
    def bias(self):
        return self._layer.bias

    def forward(self, t, x):
        tt = torch.ones_like(x[:, :1, :, :]) * t                # (batch, 1, height, width)
        return self._layer(torch.cat([tt, x], dim=1))


class Conv2dODEFunc(nn.Module):
    """Convolutional block modelling the derivative of the ODE system (conv_odenet.py:47-137): conv1 1x1 -> act -> conv2 3x3 "same"
    -> act -> conv3 1x1, on NCHW images.  `img_size_or_channels`: the image's (channels, height, width) or its channel count - torch
    needs it up front (the reference builds conv3 on the first call); the ODE state has channels + augment_dim channels."""

    def __init__(self, img_size_or_channels, num_filters, augment_dim=0, time_dependent=False, non_linearity='relu'):
        super(Conv2dODEFunc, self).__init__()
        ch = img_size_or_channels[0] if isinstance(img_size_or_channels, (tuple, list)) else img_size_or_channels
        self.augment_dim = augment_dim
        self.channels = int(ch) + augment_dim
        self.num_filters = num_filters
        self.time_dependent = time_dependent
        self.nfe = 0                                              # number of function evaluations (:72)
        C, Fn = self.channels, num_filters
        if time_dependent:
            self.conv1 = Conv2dTime(C, Fn, kernel_size=1, stride=1, padding=0)
            self.conv2 = Conv2dTime(Fn, Fn, kernel_size=3, stride=1, padding=1)
            self.conv3 = Conv2dTime(Fn, C, kernel_size=1, stride=1, padding=0)
        else:
            self.conv1 = nn.Conv2d(C, Fn, kernel_size=1, stride=1, padding=0)
            self.conv2 = nn.Conv2d(Fn, Fn, kernel_size=3, stride=1, padding=1)
            self.conv3 = nn.Conv2d(Fn, C, kernel_size=1, stride=1, padding=0)
        self.non_linearity_name = non_linearity
        cls = _ACTS.get(non_linearity)
        if cls is None and hasattr(F_, non_linearity):           # tf.keras.layers.Activation(name): 'elu', 'selu', 'sigmoid', ...
            self.non_linearity = _Activation(non_linearity)
        else:
            self.non_linearity = cls() if cls is not None else getattr(nn, non_linearity)()

    def forward(self, t, x):
        self.nfe += 1                                             # :125
        if self.time_dependent:
            out = self.non_linearity(self.conv1(t, x))
            out = self.non_linearity(self.conv2(t, out))
            return self.conv3(t, out)
        out = self.non_linearity(self.conv1(x))
        out = self.non_linearity(self.conv2(out))
        return self.conv3(out)

    def device_rhs(self):
        """The fused stage kernel's descriptor of this function (`rhs.Conv2dODE`).  ONE descriptor per module; its weight copies are
        refreshed IN PLACE on every call, so in-place optimizer steps (which bump no version counter) are never missed."""
        layers = (self.conv1, self.conv2, self.conv3)
        params = [p.detach() for l in layers for p in (l.weight, l.bias)]
        w1, b1, w2, b2, w3, b3 = params
        cached = getattr(self, '_fused_rhs', None)
        if cached is not None and all(a.device == b.device and a.dtype == b.dtype for a, b in zip(cached.Ws, (w1, w2, w3))):
            return cached.refresh(w1, b1, w2, b2, w3, b3)
        desc = _rhs.Conv2dODE(w1, b1, w2, b2, w3, b3, activation=self.non_linearity_name, time_dependent=self.time_dependent)
        object.__setattr__(self, '_fused_rhs', desc)
        return desc


def _same_padding(size, k, s):
    """TF "same" padding along one axis: (before, after) - the extra pixel goes after."""
    out = (size + s - 1) // s
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


class _SameConv2d(nn.Conv2d):
    """nn.Conv2d with TF's "same" padding for any stride (torch's padding='same' refuses stride > 1): explicit, asymmetric zero padding."""

    def forward(self, x):
        ph = _same_padding(x.shape[-2], self.kernel_size[0], self.stride[0])
        pw = _same_padding(x.shape[-1], self.kernel_size[1], self.stride[1])
        return super(_SameConv2d, self).forward(F_.pad(x, (pw[0], pw[1], ph[0], ph[1])))


class Conv2dODENet(nn.Module):
    """An ODEBlock with a convolutional ODEFunc followed by a Conv2d output layer with TF "same" padding (conv_odenet.py:140-211).
    img_size: (channels, height, width); inputs are NCHW [batch, channels, height, width]."""

    def __init__(self, img_size, num_filters, output_dim=1, augment_dim=0, time_dependent=False, out_kernel_size=(1, 1),
                 non_linearity='relu', out_strides=(1, 1), tol=1e-3, adjoint=False, solver='dopri5'):
        super(Conv2dODENet, self).__init__()
        from .models import ODEBlock
        self.img_size = tuple(img_size)
        self.num_filters = num_filters
        self.augment_dim = augment_dim
        self.output_dim = output_dim
        self.time_dependent = time_dependent
        self.tol = tol
        self.solver = solver
        self.output_kernel = tuple(out_kernel_size) if isinstance(out_kernel_size, (tuple, list)) else (out_kernel_size,) * 2
        self.output_strides = tuple(out_strides) if isinstance(out_strides, (tuple, list)) else (out_strides,) * 2
        odefunc = Conv2dODEFunc(self.img_size, num_filters, augment_dim, time_dependent, non_linearity)
        self.odeblock = ODEBlock(odefunc, is_conv=True, tol=tol, adjoint=adjoint, solver=solver)
        self.output_layer = _SameConv2d(self.img_size[0] + augment_dim, output_dim, kernel_size=self.output_kernel, stride=self.output_strides)

    def forward(self, x, return_features=False):
        features = self.odeblock(x)
        pred = self.output_layer(features)
        if return_features:
            return features, pred
        return pred
