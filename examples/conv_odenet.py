"""Train a small Conv2dODENet (tfdiffeq/models/conv_odenet.py, NCHW) for a few steps on synthetic images, then run inference.

Training goes through odeint_adjoint with autograd over the torch convolutions; inference runs each Runge-Kutta stage as one launch of
the fused convolutional stage kernel (csrc/mi_ode_conv.h).  No dataset is downloaded: the images are noisy
textures - horizontal stripes, vertical stripes, a checkerboard or a flat field - and the class is the texture.
    python examples/conv_odenet.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfdiffeq_amd import models, odeint  # noqa: E402


def batch(n, gen, dev):
    label = torch.randint(0, 4, (n,), generator=gen)
    r = torch.arange(12).view(1, 12, 1)
    c = torch.arange(12).view(1, 1, 12)
    ph = torch.randint(0, 2, (n, 1, 1), generator=gen)                # random phase of the pattern
    pats = torch.stack([((r + ph) % 2).expand(n, 12, 12), ((c + ph) % 2).expand(n, 12, 12), (r + c + ph) % 2], 1).float() * 2 - 1   # [n, 3, 12, 12]
    x = torch.zeros(n, 12, 12)
    textured = label < 3
    x[textured] = pats[torch.arange(n)[textured], label[textured]]
    x = x + 0.3 * torch.randn(n, 12, 12, generator=gen)
    return x.unsqueeze(1).to(dev), label.to(dev)


def main():
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    net = models.Conv2dODENet((1, 12, 12), num_filters=16, output_dim=4, augment_dim=2, time_dependent=True, adjoint=True).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    for step in range(60):
        x, y = batch(64, gen, dev)
        logits = net(x).mean(dim=(2, 3))
        loss = torch.nn.functional.cross_entropy(logits, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if step % 10 == 0 or step == 59:
            print('step %2d  loss %.4f  nfe %d' % (step, float(loss.detach()), net.odeblock.odefunc.nfe))
    x, y = batch(256, gen, dev)
    with torch.no_grad():
        acc = float((net(x).mean(dim=(2, 3)).argmax(1) == y).float().mean())
    print('inference: accuracy %.3f, nfe %d, engine: %s' % (acc, net.odeblock.odefunc.nfe, odeint.last_stats.get('engine')))


if __name__ == '__main__':
    main()
