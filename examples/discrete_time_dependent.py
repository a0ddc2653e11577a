"""Exact fixed-grid gradients of a TIME-DEPENDENT network: ODENet(time_dependent=True, gradient='discrete') with rk4 on [0, 1] - the first
layer sees concat([t, x]), so column 0 of fc1.weight (w_t) has a gradient of its own, sum over the stages of t_stage times the first
layer's column sums.  A few SGD steps; at every step the distance of each gradient from the taped one (the 3/8 rule written in torch ops
and back-propagated - what the reference's tape computes), with the w_t column reported separately, and the engine that ran the backward.

    python examples/discrete_time_dependent.py [--steps 5] [--batch 4096] [--freeze fc2.bias]

The backward is one launch of the fused sweep (csrc/mi_ode_discrete.h); a frozen tensor of the network (--freeze) keeps it there.
"""
import argparse
import copy

import torch

from tfdiffeq_amd import models, odeint_discrete


def taped_forward(net, x):
    """ODENet.forward with one step of the 3/8 rule over [0, 1] in torch ops."""
    f = net.odeblock.odefunc
    t = lambda v: torch.full((), v, device=x.device)         # noqa: E731
    k1 = f(t(0.), x)
    k2 = f(t(1. / 3.), x + k1 / 3.)
    k3 = f(t(2. / 3.), x + (k2 - k1 / 3.))
    k4 = f(t(1.), x + (k1 - k2 + k3))
    return net.linear_layer(x + (k1 + 3. * (k2 + k3) + k4) / 8.)


def distance(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--lr', type=float, default=0.05)
    ap.add_argument('--freeze', default='', help='a parameter of the network to freeze, e.g. fc2.bias')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = models.ODENet(64, 128, 10, time_dependent=True, non_linearity='tanh', solver='rk4', gradient='discrete').to(dev)
    if args.freeze:
        dict(net.odeblock.odefunc.named_parameters())[args.freeze].requires_grad_(False)
    x = torch.randn(args.batch, 64, device=dev)
    target = torch.randn(args.batch, 10, device=dev)
    for step in range(args.steps):
        ref = copy.deepcopy(net)
        ((taped_forward(ref, x) - target) ** 2).mean().backward()
        for p in net.parameters():
            p.grad = None
        loss = ((net(x) - target) ** 2).mean()
        loss.backward()
        pairs = [(p.grad, q.grad) for p, q in zip(net.parameters(), ref.parameters()) if p.requires_grad]
        w1, w1_ref = net.odeblock.odefunc.fc1.weight.grad, ref.odeblock.odefunc.fc1.weight.grad
        line = 'step %d: loss %.4f, gradients %.2e from the taped loop' % (step, float(loss), max(distance(a, b) for a, b in pairs))
        if w1 is not None:
            line += ', the w_t column %.2e (max |grad w_t| %.3e)' % (distance(w1[:, 0], w1_ref[:, 0]), float(w1[:, 0].abs().max()))
        print(line)
        with torch.no_grad():
            for p in net.parameters():
                if p.grad is not None:
                    p -= args.lr * p.grad
    st = odeint_discrete.last_backward_stats
    print('backward engine: %s, %s launch(es)%s' % (st.get('engine'), st.get('n_launches'), ('; why: ' + st['why']) if st.get('why') else ''))


if __name__ == '__main__':
    main()
