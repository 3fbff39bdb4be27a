"""Data that isn't tabular: a subnetwork in front of DistributedIBNet.

One feature of each sample is a raw time series (64 samples of a noisy sinusoid), the other a plain scalar.  A small torch MLP
turns the series into a 2-dimensional summary, which DistributedIBNet treats as one feature with its own bottleneck next to the
scalar's; the label depends on both.  The loss is differentiable with respect to the model's inputs (dib_encoder_bank_input_grad
behind the autograd bridge), so one torch optimizer trains the subnetwork and the Distributed-IB model together:

    python examples/subnetwork_dib.py            (needs an MI355X; there is no CPU path)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dib_amd  # noqa: E402


def make_data(n, rng):
    freq = rng.uniform(0.5, 3.0, n)
    t = np.linspace(0.0, 2.0 * np.pi, 64)
    series = np.sin(freq[:, None] * t[None, :]) + 0.1 * rng.standard_normal((n, 64))
    scalar = rng.standard_normal(n)
    label = ((freq > 1.75) ^ (scalar > 0)).astype(np.float32)       # XOR of a property of the series and of the scalar
    return series.astype(np.float32), scalar.astype(np.float32)[:, None], label[:, None]


def main(steps=30, batch=256):
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    series, scalar, label = make_data(4096, rng)
    dib = dib_amd.DistributedIBModule(dib_amd.DistributedIBNet([2, 1], [128, 128], [256, 256], 1))
    dev = dib.flat_parameters.device
    subnet = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Tanh(), torch.nn.Linear(32, 2)).to(dev)
    dib.net.beta.assign(1e-3)
    opt = torch.optim.Adam(list(subnet.parameters()) + list(dib.parameters()), lr=1e-3)
    series, scalar, label = (torch.from_numpy(a).to(dev) for a in (series, scalar, label))
    losses = []
    for step in range(steps):
        idx = torch.from_numpy(rng.integers(0, series.shape[0], batch)).to(dev)
        x = torch.cat([subnet(series[idx]), scalar[idx]], dim=1)     # subnetwork -> DIB -> torch optimizer
        pred, kl_loss = dib(x)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, label[idx]) + kl_loss
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if step % 10 == 0 or step == steps - 1:
            gn = float(sum(p.grad.norm() ** 2 for p in subnet.parameters()) ** 0.5)
            print(f"step {step:3d}  loss {losses[-1]:.4f}  |grad subnetwork| {gn:.3e}")
    return losses


if __name__ == "__main__":
    main()
