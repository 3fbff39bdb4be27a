"""Float64 restatement of the chaos notebook's measurement-optimisation step (reference chaos/Chaos_experiments.ipynb cells 3
and 10: create_info_bott_encoder, match_batch, the Adam step, the symbolisation) with torch float64 autograd, driven by the
same Philox noise as the device (oracle/dib_oracle.py philox_normal, feature 0).  The checker only."""
import numpy as np
import torch

import dib_oracle as orc

SLOPES = {"leaky_relu": 0.2, "relu": 0.0, "linear": 1.0}


def posenc(x, first_exponent, n_freq):
    """PositionalEncoding(2**arange(first_exponent, first_exponent + n_freq - 1)): [x, sin(f x), ...]"""
    return torch.cat([x] + [torch.sin((2.0 ** (first_exponent + k)) * x) for k in range(n_freq - 1)], -1)


def mlp(x, weights, slope):
    n = len(weights) // 2
    for l in range(n):
        x = x @ weights[2 * l] + weights[2 * l + 1]
        if l < n - 1:
            x = torch.where(x > 0, x, slope * x)
    return x


def eps_rows(seed, step, rows, E):
    return orc.philox_normal(seed, step, np.asarray(rows), 0, E)


def match_batch(weights, states, eps, beta, kl_exponent, n_freq, reference_timestep=0, temperature=1.0, slope=0.2,
                grads=True):
    """weights: {"ib", "vq", "agg", "ref"} -> Keras-ordered lists of float64 arrays.  states [B, L, d]; eps [B * L, E].
    Returns (loss, loss_prediction, kl, {net: [gradients]})."""
    W = {k: [torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=grads) for w in v] for k, v in weights.items()}
    x = torch.tensor(np.asarray(states, dtype=np.float64))
    B, L, d = x.shape
    enc = mlp(posenc(x.reshape(-1, d), 1, n_freq), W["ib"], slope)
    E = enc.shape[1] // 2
    mu, lv = enc[:, :E], enc[:, E:]
    kl = torch.mean(torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1.0), -1))
    loss = beta * L * kl ** kl_exponent
    z = mu + torch.tensor(np.asarray(eps, dtype=np.float64)) * torch.exp(lv / 2.0)
    soft = torch.softmax(mlp(z, W["vq"], slope), -1).reshape(B, -1)
    seq = mlp(soft, W["agg"], slope)
    ref = mlp(posenc(x[:, reference_timestep], 0, n_freq), W["ref"], slope)
    sim = -torch.sum((seq[:, None, :] - ref[None, :, :]) ** 2, -1) / temperature
    lab = torch.arange(B)
    lp = (torch.nn.functional.cross_entropy(sim, lab) + torch.nn.functional.cross_entropy(sim.T, lab)) / 2.0
    loss = loss + lp
    g = None
    if grads:
        loss.backward()
        g = {k: [w.grad.numpy() for w in v] for k, v in W.items()}
    return float(loss.detach()), float(lp.detach()), float(kl.detach()), g


def adam(weights, grads, state, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """Keras Adam, one step (t = steps applied before this one)"""
    lr_t = lr * np.sqrt(1 - b2 ** (t + 1)) / (1 - b1 ** (t + 1))
    out = {}
    for k in weights:
        out[k] = []
        for i, (w, gr) in enumerate(zip(weights[k], grads[k])):
            m, v = state.setdefault((k, i), (np.zeros_like(w), np.zeros_like(w)))
            m = m + (1 - b1) * (gr - m)
            v = v + (1 - b2) * (gr * gr - v)
            state[(k, i)] = (m, v)
            out[k].append(w - lr_t * m / (np.sqrt(v) + eps))
    return out


def vq_logits(weights, mu, lv, noise, slope=0.2):
    """[K, N, A] float64 logits of VQ(mu + noise_k exp(lv / 2))"""
    W = [torch.tensor(np.asarray(w, dtype=np.float64)) for w in weights]
    mu, lv = torch.tensor(np.asarray(mu, np.float64)), torch.tensor(np.asarray(lv, np.float64))
    nz = torch.tensor(np.asarray(noise, np.float64))
    z = mu[None] + nz[:, None, :] * torch.exp(lv / 2.0)[None]
    return mlp(z.reshape(-1, mu.shape[1]), W, slope).reshape(nz.shape[0], mu.shape[0], -1).numpy()


def encode(weights, x, n_freq, slope=0.2):
    W = [torch.tensor(np.asarray(w, dtype=np.float64)) for w in weights]
    return mlp(posenc(torch.tensor(np.asarray(x, np.float64)), 1, n_freq), W, slope).numpy()
