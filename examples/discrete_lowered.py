"""Fit the matrix of the cubic spiral, dy/dt = (y ** 3) @ A, by back-propagating through rk4 - the reference's examples/ode_demo.py with
the `Lambda` right-hand side made trainable - with the whole backward in ONE launch:

    python examples/discrete_lowered.py [--iters 200] [--batch 64] [--points 11]

`odeint_discrete(f, y0, t, method='rk4', lower='auto')` traces the plain Python callable, generates the vjp of its trace as device code
and runs the reverse sweep of all steps with one trajectory per lane (csrc/mi_ode_discrete_row.h).  The gradient is the one the reference's
tape returns (the exact gradient of the discrete map), not the continuous adjoint's.
"""
import argparse

import torch

from tfdiffeq_amd import odeint, odeint_discrete


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--points', type=int, default=11)
    ap.add_argument('--lr', type=float, default=0.02)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    true_A = torch.tensor([[-0.1, 2.0], [-2.0, -0.1]], dtype=torch.float64, device=dev)
    y0 = (torch.rand(args.batch, 2, dtype=torch.float64, device=dev) * 2 - 1) * 1.5
    t = torch.linspace(0., 1., args.points, dtype=torch.float64)
    with torch.no_grad():
        target = odeint(lambda t_, y: (y ** 3) @ true_A, y0, t, method='rk4')
    A = (true_A + 0.5 * torch.randn(2, 2, dtype=torch.float64, device=dev)).requires_grad_(True)
    opt = torch.optim.Adam([A], lr=args.lr)

    def f(t_, y):
        return (y ** 3) @ A
    for it in range(args.iters):
        opt.zero_grad()
        loss = (odeint_discrete(f, y0, t, method='rk4', lower='auto') - target).abs().mean()
        loss.backward()
        opt.step()
        if it % 20 == 0 or it == args.iters - 1:
            st = odeint_discrete.last_backward_stats
            print('iter %4d  loss %.6f  |A - A_true| %.4f  backward: %s, %s launch(es)' % (
                it, float(loss), float((A.detach() - true_A).abs().max()), st.get('engine'), st.get('n_launches')))
    print('A =', A.detach().cpu().numpy().round(4).tolist())


if __name__ == '__main__':
    main()
