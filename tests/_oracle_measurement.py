"""Float64 restatement of the chaos notebook's measurement-optimisation step (reference chaos/Chaos_experiments.ipynb cells 3
and 10: create_info_bott_encoder, match_batch, the Adam step, the symbolisation) with torch float64 autograd, driven by the
same Philox noise as the device (oracle/dib_oracle.py philox_normal, feature 0).  The checker only."""
import numpy as np
import torch

import dib_oracle as orc
from dib_torch_cpu import scaled_similarity_torch

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
                grads=True, similarity="l2sq"):
    """weights: {"ib", "vq", "agg", "ref"} -> Keras-ordered lists of float64 arrays.  states [B, L, d]; eps [B * L, E].
    reference_timestep indexes the sequence like NumPy (-1: the last state).
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
    sim = scaled_similarity_torch(seq, ref, similarity, temperature)
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


# ---- float64 restatement of the kernels' C ABI (include/dib_measure.h), one entry point each ----------------------------
def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def measure_fwd(vq, enc, seed, step, beta, kl_exponent, L, slope):
    """dib_measure_fwd: (z, h1, h2, soft, out3) of enc [rows, 2E] and the VQ weights [W1, b1, W2, b2, W3, b3]"""
    W = [_t(w) for w in vq]
    enc = _t(enc)
    rows, E = enc.shape[0], enc.shape[1] // 2
    mu, lv = enc[:, :E], enc[:, E:]
    z = mu + _t(eps_rows(seed, step, np.arange(rows), E)) * torch.exp(lv / 2.0)
    h1 = z @ W[0] + W[1]
    h1 = torch.where(h1 > 0, h1, slope * h1)
    h2 = h1 @ W[2] + W[3]
    h2 = torch.where(h2 > 0, h2, slope * h2)
    soft = torch.softmax(h2 @ W[4] + W[5], -1)
    kl = float(torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1.0)) / rows)
    out3 = np.array([kl, beta * L * kl ** kl_exponent, kl_exponent * beta * L * kl ** (kl_exponent - 1.0) / rows])
    return z.numpy(), h1.numpy(), h2.numpy(), soft.numpy(), out3


def measure_bwd(vq, enc, seed, step, h1, h2, soft, g_agg, w_agg0, coef, L, slope):
    """dib_measure_bwd on the given stashes: (g3, g2, g1, g_enc).  dsoft[b * L + l, a] = g_agg[b] . w_agg0[l * A + a];
    hidden-layer masks from the stashed post-activations (h > 0 ? 1 : slope); coef = out3[2] as the kernel reads it."""
    W = [_t(w) for w in vq]
    enc, h1, h2, soft = _t(enc), _t(h1), _t(h2), _t(soft)
    rows, E, A = enc.shape[0], enc.shape[1] // 2, soft.shape[1]
    B = rows // L
    dsoft = (_t(g_agg) @ _t(w_agg0).T).reshape(B * L, A)
    g3 = soft * (dsoft - torch.sum(soft * dsoft, -1, keepdim=True))
    mask = lambda h: torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    g2 = (g3 @ W[4].T) * mask(h2)
    g1 = (g2 @ W[2].T) * mask(h1)
    dz = g1 @ W[0].T
    mu, lv = enc[:, :E], enc[:, E:]
    eps = _t(eps_rows(seed, step, np.arange(rows), E))
    g_mu = dz + coef * mu
    g_lv = dz * 0.5 * eps * torch.exp(lv / 2.0) + coef * 0.5 * (torch.exp(lv) - 1.0)
    return g3.numpy(), g2.numpy(), g1.numpy(), torch.cat([g_mu, g_lv], -1).numpy()


def posenc_rows(x, row_idx, d, n_freq, first_exponent):
    """dib_measure_posenc_rows: [x, sin(2^f0 x), ..., sin(2^(f0 + n_freq - 2) x)] of rows row_idx of x[:, :d]"""
    return posenc(_t(x)[np.asarray(row_idx)][:, :d], first_exponent, n_freq).numpy()
