"""float64 NumPy restatement of the MI-bound characterization (dib_amd.mi_characterization, include/dib_mi_channel.h): the
Monte-Carlo term of a known diagonal-Gaussian channel in its log-sum-exp form and in the notebook's literal raw-exp form, the
samples from the shared Philox noise, and the closed-form information of one +-d bit through unit Gaussian noise."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dib_oracle as orc  # noqa: E402


def log_densities(mus, logvars, u):
    """l[i, j] = log N(u_i; mu_j, diag exp(logvar_j)), float64"""
    mus, logvars, u = (np.asarray(a, dtype=np.float64) for a in (mus, logvars, u))
    E = mus.shape[1]
    out = np.empty((u.shape[0], mus.shape[0]))
    inv = np.exp(-logvars / 2.0)
    c = -0.5 * logvars.sum(-1) - 0.5 * E * np.log(2.0 * np.pi)
    step = max(1, (1 << 24) // (mus.shape[0] * E))
    for i0 in range(0, u.shape[0], step):
        z = (u[i0:i0 + step, None, :] - mus[None]) * inv[None]
        out[i0:i0 + step] = c[None] - 0.5 * np.sum(z * z, -1)
    return out


def mc_terms_lse(mus, logvars, u, src):
    """term_i = l[i, src_i] - (LSE_j l[i, j] - log N) in nats: log p(u_i | x_src_i) / mean_j p(u_i | x_j), every row by position"""
    l = log_densities(mus, logvars, u)
    m = l.max(-1)
    lse = m + np.log(np.exp(l - m[:, None]).sum(-1))
    return l[np.arange(len(src)), np.asarray(src)] - (lse - np.log(l.shape[1]))


def mc_terms_literal(mus, u, src):
    """the notebook's raw-exp form at logvar 0, nats: p_ugx / p_u with the (2 pi)^(E/2) normalisation and norm distances"""
    mus, u, src = np.asarray(mus, dtype=np.float64), np.asarray(u, dtype=np.float64), np.asarray(src)
    n_rows, E = mus.shape
    stat_dists = np.linalg.norm(mus.reshape(-1, 1, E) - u.reshape(1, -1, E), ord=2, axis=-1)   # [rows, samples]
    normalization = (2.0 * np.pi) ** (E / 2.0)
    p_u = np.mean(np.exp(-stat_dists ** 2 / 2.0) / normalization, axis=0)
    dists_ugx = np.linalg.norm(mus[src] - u, ord=2, axis=-1)
    p_ugx = np.exp(-dists_ugx ** 2 / 2.0) / normalization
    return np.log(p_ugx / p_u)


def sample_u(mus, logvars, src, seed, step):
    """u_s = mu_r + sigma_r eps, r = src[s], eps = the shared Philox normals keyed (seed, step, row s, feature 0)"""
    mus, logvars = np.asarray(mus, dtype=np.float64), np.asarray(logvars, dtype=np.float64)
    eps = orc.philox_normal(seed, step, np.arange(len(src), dtype=np.uint32), 0, mus.shape[1])
    return mus[src] + np.exp(logvars[src] / 2.0) * eps


def one_bit_information(d):
    """I(X; X d + N(0, 1)) in bits for a fair X = +-1: (h(1/2 N(-d, 1) + 1/2 N(d, 1)) - 1/2 log(2 pi e)) / ln 2, by quadrature"""
    from scipy.integrate import quad

    def neg_p_log_p(y):
        p = 0.5 * (np.exp(-0.5 * (y - d) ** 2) + np.exp(-0.5 * (y + d) ** 2)) / np.sqrt(2.0 * np.pi)
        return -p * np.log(p) if p > 0.0 else 0.0
    h, _ = quad(neg_p_log_p, -d - 12.0, d + 12.0, epsabs=1e-13, epsrel=1e-13, limit=400, points=[-d, 0.0, d])
    return (h - 0.5 * np.log(2.0 * np.pi * np.e)) / np.log(2.0)


def balanced_signs(k, n_rows):
    """[n_rows, k] of +-1: every one of the 2^k patterns equally often (n_rows a multiple of 2^k)"""
    assert n_rows % (1 << k) == 0
    pats = np.array([[1.0 if (p >> b) & 1 else -1.0 for b in range(k)] for p in range(1 << k)])
    return np.tile(pats, (n_rows >> k, 1))
