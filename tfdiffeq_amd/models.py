"""Mirror of tfdiffeq/models/dense_odenet.py for torch: ODEFunc, ODEBlock, ODENet.

`ODEBlock` is config 5's real caller: t = [0, 1], rtol = atol = tol (1e-3), `max_num_steps = 1000`, optional zero
augmentation, returns the state at t = 1 (dense_odenet.py:131-191).  When the ODEFunc has a relu (the reference's default),
softplus or tanh non-linearity, inference runs on the fused MFMA kernel (`rhs.MLP`, csrc/mi_ode_mlp.h; `time_dependent=True`
included: the stage time only shifts the first layer's bias) and training on it plus the fused adjoint kernel
(csrc/mi_ode_adjoint.h; time-dependent networks too); otherwise the plane-kernel engine (and the generic `odeint_adjoint`) take over.
"""
import torch
from torch import nn

from . import dispatch as _dispatch
from . import rhs as _rhs
from .adjoint import odeint_adjoint
from .discrete import TABLEAUS as _DISCRETE_METHODS, odeint_discrete
from .odeint import odeint

MAX_NUM_STEPS = 1000          # dense_odenet.py:14


class ODEFunc(nn.Module):
    """MLP modelling the derivative of the ODE system (dense_odenet.py:17-92): fc1 -> act -> fc2 -> act -> fc3."""

    def __init__(self, input_dim, hidden_dim, augment_dim=0, time_dependent=False, non_linearity='relu'):
        super(ODEFunc, self).__init__()
        self.augment_dim = augment_dim
        self.input_dim = input_dim + augment_dim
        self.hidden_dim = hidden_dim
        self.nfe = 0                                             # number of function evaluations (:38)
        self.time_dependent = time_dependent
        self.fc1 = nn.Linear(self.input_dim + (1 if time_dependent else 0), hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, hidden_dim)
        self.fc3 = nn.Linear(hidden_dim, self.input_dim)
        self.non_linearity_name = non_linearity
        self.non_linearity = {'relu': nn.ReLU(), 'softplus': nn.Softplus(), 'tanh': nn.Tanh()}.get(non_linearity)
        if self.non_linearity is None:
            self.non_linearity = getattr(nn, non_linearity)()

    def forward(self, t, x):
        self.nfe += 1                                            # :78
        if self.time_dependent:
            t_vec = torch.ones(x.shape[0], 1, dtype=x.dtype, device=x.device) * t
            out = self.fc1(torch.cat([t_vec, x], dim=-1))
        else:
            out = self.fc1(x)
        out = self.non_linearity(out)
        out = self.fc2(out)
        out = self.non_linearity(out)
        return self.fc3(out)

    def device_rhs(self):
        """The fused-kernel descriptor of this network, or None if the fused MLP kernel does not cover it.
        ONE descriptor per module; its [in, out] weight copies are refreshed IN PLACE on every call (six small device copies), so
        the cached engine - keyed on those buffers - keeps being hit and the kernels never see stale weights.  (A version stamp
        cannot decide "unchanged": `p.data -= lr * p.grad`, `p.data.clamp_()` and friends bump no version counter and keep
        data_ptr - hand-written SGD and weight clipping look exactly like that.)"""
        if self.non_linearity_name not in _rhs.MLP.ACTIVATIONS:
            return None
        layers = (self.fc1, self.fc2, self.fc3)
        cached = getattr(self, '_fused_rhs', None)
        with torch.no_grad():
            if cached is not None and all(w.device == l.weight.device and w.dtype == l.weight.dtype and w.shape == l.weight.t().shape
                                          for w, l in zip(cached.Ws, layers)):
                for w, b, l in zip(cached.Ws, cached.bs, layers):            # same storage: engines created on it stay valid
                    w.copy_(l.weight.t())
                    b.copy_(l.bias)
                return cached
            desc = _rhs.MLP(self.fc1.weight.detach().t().contiguous(), self.fc1.bias.detach().clone(),
                            self.fc2.weight.detach().t().contiguous(), self.fc2.bias.detach().clone(),
                            self.fc3.weight.detach().t().contiguous(), self.fc3.bias.detach().clone(),
                            activation=self.non_linearity_name, time_dependent=self.time_dependent)
        object.__setattr__(self, '_fused_rhs', desc)
        return desc


class LinearODEFunc(nn.Module):
    """f(t, y) = y W (+ b): the linear system of BASELINE config 4 as a trainable module (not a class of the reference - its
    models are the MLP above and a convolutional zoo; this is the headline workload's training analogue).
    `weight` is [dim, dim] in [in, out] layout, so that `forward` is one matmul and the fused kernels read it as it is.
    Forward: the whole-call MFMA kernel (`rhs.Linear`); backward under `odeint_adjoint`: the reference's augmented system
    (adjoint.py:69-105) with its three big products on MFMA kernels instead of autograd over rocBLAS (adjoint._linear_dynamics).
    Under `odeint_discrete(..., linear='auto')` / `discrete.LINEAR = 'auto'` (ODEBlock(gradient='discrete') reads the latter) the exact
    fixed-grid gradient is one launch of csrc/mi_ode_discrete_linear.h - also on the grid of options['step_size'] (discrete.OWN_GRID = True),
    where the kernel recomputes its checkpoints instead of reading a stored trajectory."""
    augment_dim = 0               # what ODEBlock asks every odefunc for: the state is never augmented

    def __init__(self, dim, bias=True, dtype=torch.float64):
        super(LinearODEFunc, self).__init__()
        self.dim = int(dim)
        self.nfe = 0
        w = -0.5 * torch.eye(dim, dtype=dtype) + 0.5 * torch.randn(dim, dim, dtype=dtype) / dim ** 0.5
        self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(dim, dtype=dtype)) if bias else None

    def forward(self, t, y):
        self.nfe += 1
        out = torch.matmul(y, self.weight)
        return out if self.bias is None else out + self.bias

    def device_rhs(self):
        """`rhs.Linear` over the parameters themselves (no copies: in-place optimizer steps stay visible to the cached engine)."""
        cached = getattr(self, '_fused_rhs', None)
        b = None if self.bias is None else self.bias.detach()
        if cached is None or cached.W.data_ptr() != self.weight.data_ptr() or (b is not None and cached.b.data_ptr() != b.data_ptr()):
            cached = _rhs.Linear(self.weight.detach(), b)
            object.__setattr__(self, '_fused_rhs', cached)
        return cached


class ODEBlock(nn.Module):
    """Solves the ODE defined by odefunc (dense_odenet.py:95-191)."""

    def __init__(self, odefunc, is_conv=False, tol=1e-3, adjoint=False, solver='dopri5', gradient='adjoint'):
        super(ODEBlock, self).__init__()
        # gradient: 'adjoint' (default) - the continuous adjoint solve; 'discrete' - the gradient of the discrete map the fixed-grid
        # solver computed, what back-propagating through the reference's solver gives (discrete.odeint_discrete)
        if gradient not in ('adjoint', 'discrete'):
            raise ValueError("gradient must be 'adjoint' or 'discrete', not %r" % (gradient,))
        if gradient == 'discrete' and solver not in _DISCRETE_METHODS:
            raise ValueError("gradient='discrete' is the gradient of a fixed-grid solver's discrete map: solver must be one of %s, not %r "
                             "(use gradient='adjoint' with adaptive and multistep solvers)" % (sorted(_DISCRETE_METHODS), solver))
        self.gradient = gradient
        self.is_conv = is_conv
        self.adjoint = adjoint
        self.odefunc = odefunc
        self.tol = tol
        self.method = solver
        self.channel_axis = 1 if is_conv else -1                 # conv: NCHW images, augmentation along the channels (dim 1)
        if solver == 'dopri5':
            self.options = {'max_num_steps': MAX_NUM_STEPS}      # :126-127
        else:
            self.options = None

    def forward(self, x, eval_times=None):
        self.odefunc.nfe = 0                                     # :147
        if eval_times is None:
            integration_time = torch.tensor([0., 1.], dtype=x.dtype)     # :150
        else:
            integration_time = torch.as_tensor(eval_times, dtype=x.dtype)
        if self.odefunc.augment_dim > 0:                         # :154-176 zero augmentation
            shape = list(x.shape)
            shape[self.channel_axis] = self.odefunc.augment_dim
            aug = torch.zeros(shape, dtype=x.dtype, device=x.device)
            x_aug = torch.cat([x, aug], dim=self.channel_axis)
        else:
            x_aug = x
        needs_grad = torch.is_grad_enabled() and (x_aug.requires_grad or any(p.requires_grad for p in self.odefunc.parameters()))
        kw = dict(rtol=self.tol, atol=self.tol, method=self.method, options=self.options)
        if needs_grad and self.gradient == 'discrete':
            # the forward solve as the inference branch below runs it (the fused kernels where the network has them), the backward as the
            # transpose of that discrete map
            func, fused = self._inference_func(x_aug)
            out = odeint_discrete(self.odefunc, x_aug, integration_time, method=self.method, options=self.options, _forward_func=func)
            if func is fused:
                self.odefunc.nfe += int(odeint.last_stats.get('nfe', 0))
        elif needs_grad:
            # adjoint=True: the reference's odeint_adjoint branch (:178-181).  adjoint=False: the reference differentiates
            # through the solver's ops; the kernels here are not taped, so the gradient is obtained from the adjoint
            # solve in that case too (same gradient up to the solver tolerance) - never silently dropped.
            out = odeint_adjoint(self.odefunc, x_aug, integration_time, **kw)
        else:
            func, fused = self._inference_func(x_aug)
            with torch.no_grad():
                out = odeint(func, x_aug, integration_time, **kw)                           # :184-186
            if func is fused:                                    # f ran inside the kernel: the counter the reference exposes
                self.odefunc.nfe += int(odeint.last_stats.get('nfe', 0))                    # (:38, :78, :147) stays meaningful
        if eval_times is None:
            return out[1]                                        # :188-189
        return out

    def _inference_func(self, x_aug):
        """(what an untaped forward solve hands to odeint, the network's fused descriptor or None)."""
        fused = self.odefunc.device_rhs()
        if self.is_conv:
            # rhs.Conv2dODE: the fused stage kernel where it takes the shape and is the faster route (larger shapes run the torch
            # module, rhs.Conv2dODE.FUSED_MAX_CONV2_FLOP); outside its box the descriptor says why, once
            why = fused.in_box(x_aug) if x_aug.is_cuda else 'a host tensor'
            if why and x_aug.is_cuda:
                fused.warn_limits(x_aug, why)
            func = fused if (not why and fused.faster_than_torch(x_aug)) else self.odefunc
        else:
            # (the tile kernels, or - float64 / wider networks, round 5 - the cooperative one-launch kernel; if neither takes the problem
            # the solver runs the descriptor's own forward() as a callable on the device-controlled engine and says so once)
            func = fused if (fused is not None and _dispatch.has_kernel(fused, x_aug)) else self.odefunc
        return func, fused

    def trajectory(self, x, timesteps):
        """dense_odenet.py:193-205."""
        return self.forward(x, eval_times=torch.linspace(0., 1., timesteps))


from .conv_models import Conv2dODEFunc, Conv2dODENet, Conv2dTime  # noqa: E402,F401  (conv_odenet.py's classes, re-exported)


class ODENet(nn.Module):
    """An ODEBlock followed by a linear layer (dense_odenet.py:208-259)."""

    def __init__(self, input_dim, hidden_dim, output_dim, augment_dim=0, time_dependent=False, non_linearity='relu',
                 tol=1e-3, adjoint=False, solver='dopri5', gradient='adjoint'):
        super(ODENet, self).__init__()
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.augment_dim = augment_dim
        odefunc = ODEFunc(input_dim, hidden_dim, augment_dim, time_dependent, non_linearity)
        self.odeblock = ODEBlock(odefunc, tol=tol, adjoint=adjoint, solver=solver, gradient=gradient)
        self.linear_layer = nn.Linear(odefunc.input_dim, output_dim)

    def forward(self, x, return_features=False):
        features = self.odeblock(x)
        pred = self.linear_layer(features)
        if return_features:
            return features, pred
        return pred
