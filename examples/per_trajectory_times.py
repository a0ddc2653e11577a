"""Fit the Lotka-Volterra rates to members that were each observed at their OWN times - every member solved, and differentiated, on its own.

Every member of an ensemble has its own number of observations, at its own irregular times, over its own horizon.  With
options={'per_trajectory': True}, a `t` of shape [batch, T] and options['t_lengths'] row i is integrated over t[i, :len_i] and nowhere
else - no padding to the union of all times, no member integrated past its last observation - with its own step control, all rows in ONE
launch (csrc/mi_ode_rows_t.h).  solution[k, i] for k >= len_i is exactly 0, and t[i, len_i:] is never read (it holds NaN here).

odeint_adjoint takes the same inputs: the backward applies the adjoint method to every member alone, over its own times, for all rows in
ONE launch (csrc/mi_ode_rows_adjoint_t.h).  The cotangent of a member's padding is ignored, so the loss may be written on the whole
[T, batch, 2] solution; `last_backward_stats['rows']` holds the per-member pieces, and a `t` that requires grad gets a [batch, T] gradient.

usage: python examples/per_trajectory_times.py [--batch 512] [--max-obs 12] [--steps 150]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import odeint, odeint_adjoint  # noqa: E402


class LotkaVolterra(torch.nn.Module):
    def __init__(self, a, b, c, d, device):
        super(LotkaVolterra, self).__init__()
        self.a, self.b, self.c, self.d = (torch.nn.Parameter(torch.tensor(v, dtype=torch.float64, device=device)) for v in (a, b, c, d))

    def forward(self, t, y):
        x, u = y[..., 0], y[..., 1]
        return torch.stack([self.a * x - self.b * x * u, self.d * x * u - self.c * u], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--max-obs', type=int, default=12)
    ap.add_argument('--steps', type=int, default=150)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    B, T = args.batch, args.max_obs + 1
    y0 = (0.5 + 2.5 * torch.rand(B, 2, generator=g, dtype=torch.float64)).to(dev)
    # member i: len_i - 1 observations at sorted random times inside its own horizon (1 .. 4 time units); column 0 is the start
    lengths = torch.randint(3, T + 1, (B,), generator=g)
    horizon = 1.0 + 3.0 * torch.rand(B, 1, generator=g, dtype=torch.float64)
    times = torch.cat([torch.zeros(B, 1, dtype=torch.float64), torch.rand(B, T - 1, generator=g, dtype=torch.float64).cumsum(dim=1)], dim=1)
    valid = torch.arange(T)[None, :] < lengths[:, None]
    last = times.gather(1, (lengths - 1)[:, None])
    t = torch.where(valid, times / last * horizon, torch.full_like(times, float('nan')))
    call = dict(rtol=1e-7, atol=1e-9, method='dopri5', options={'per_trajectory': True, 't_lengths': lengths})
    mask = valid.t()[:, :, None].to(dev)

    truth = LotkaVolterra(1.5, 1.0, 3.0, 1.0, dev)
    with torch.no_grad():
        observed = odeint(truth, y0, t, **call)                                 # [T, B, 2], zeros beyond every member's length
        observed = observed + 0.01 * torch.randn(observed.shape, generator=g, dtype=torch.float64).to(dev) * mask
    att = odeint.last_stats['rows']['n_attempts']
    print('%d members, %d .. %d observations each, horizons %.2f .. %.2f: %d launch, %d .. %d attempts per member'
          % (B, int(lengths.min()) - 1, int(lengths.max()) - 1, float(horizon.min()), float(horizon.max()), odeint.last_stats['n_launches'],
             int(att.min()), int(att.max())))

    model = LotkaVolterra(1.2, 0.8, 2.5, 1.2, dev)
    plan = odeint_adjoint.plan(model, y0, t, **call)
    print(plan['forward']['kernel'])
    print(plan['kernel'])
    opt = torch.optim.Adam(model.parameters(), lr=0.02)
    for step in range(args.steps + 1):
        opt.zero_grad()
        sol = odeint_adjoint(model, y0, t, **call)
        loss = (sol - observed).pow(2).sum() / mask.sum()        # (the padding is 0 in both, and its cotangent is ignored)
        loss.backward()
        if step % 25 == 0:
            st = odeint_adjoint.last_backward_stats
            batt = st['rows']['n_attempts'].sum(dim=1)
            print('step %3d  loss %.3e  a %.4f b %.4f c %.4f d %.4f   backward: %d launch, %d .. %d attempts per member'
                  % (step, loss.item(), model.a.item(), model.b.item(), model.c.item(), model.d.item(), st['n_launches'], int(batt.min()), int(batt.max())))
        opt.step()
    print('recovered a %.3f (1.5), b %.3f (1.0), c %.3f (3.0), d %.3f (1.0)' % (model.a.item(), model.b.item(), model.c.item(), model.d.item()))


if __name__ == '__main__':
    main()
