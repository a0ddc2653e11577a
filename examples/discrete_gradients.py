"""The two gradients of a fixed-grid solve, side by side: ODENet with ONE Euler step over [0, 1] (the reference's MNIST example trains
like this), a few SGD steps with gradient='discrete' and with the default gradient='adjoint', and at every step the distance of each
gradient from the taped one - the solver loop written in torch ops and back-propagated, which is what the reference's tape computes.

    python examples/discrete_gradients.py [--steps 5] [--batch 4096]

gradient='discrete' is the taped gradient to float32 rounding; the continuous adjoint, discretised with the same one step, evaluates
df/dtheta at y1 instead of y0 and is O(h) away with h = 1.
"""
import argparse
import copy

import torch

from tfdiffeq_amd import models, odeint_discrete


def taped_forward(net, x):
    """ODENet.forward with the Euler step in torch ops: features = x + 1 * f(0, x)."""
    f = net.odeblock.odefunc
    return net.linear_layer(x + 1.0 * f(torch.zeros((), device=x.device), x))


def distance(grads, ref):
    return max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads, ref))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--lr', type=float, default=0.05)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    nets = {'discrete': models.ODENet(64, 128, 10, non_linearity='tanh', solver='euler', gradient='discrete').to(dev)}
    nets['adjoint'] = models.ODENet(64, 128, 10, non_linearity='tanh', solver='euler').to(dev)
    nets['adjoint'].load_state_dict(nets['discrete'].state_dict())
    x = torch.randn(args.batch, 64, device=dev)
    target = torch.randn(args.batch, 10, device=dev)
    for step in range(args.steps):
        line = 'step %d' % step
        for name, net in nets.items():
            ref_net = copy.deepcopy(net)
            ((taped_forward(ref_net, x) - target) ** 2).mean().backward()
            for p in net.parameters():
                p.grad = None
            loss = ((net(x) - target) ** 2).mean()
            loss.backward()
            line += '   %s: loss %.4f, gradient %.2e from the taped loop' % (
                name, float(loss), distance([p.grad for p in net.parameters()], [p.grad for p in ref_net.parameters()]))
            with torch.no_grad():
                for p in net.parameters():
                    p -= args.lr * p.grad
        print(line)
    print('backward engine of gradient=\'discrete\':', odeint_discrete.last_backward_stats.get('engine'))


if __name__ == '__main__':
    main()
