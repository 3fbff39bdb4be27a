"""Float64 NumPy restatements of the set-transformer notebook's information tracking (the checker of
tests/test_gpu_st_information.py, pinned on the notebook's own statements by tests/test_st_information_oracle.py):
  - cell 5's compute_infos_mus_logvars: the literal exp-then-log form and the log-sum-exp form (per row and batch means);
  - the probe-grid map of cell 8 in log-sum-exp form (one batch, and the mean over batches);
  - the information-plane tail of cell 8."""
import numpy as np
from scipy.special import logsumexp

LN2PI = np.log(2.0 * np.pi)


def log_densities(u, mus, logvars):
    """l[i, j] = log N(u_i; mu_j, diag(exp(logvar_j))), float64"""
    u, mus, logvars = (np.asarray(a, np.float64) for a in (u, mus, logvars))
    d = (u[:, None, :] - mus[None, :, :]) / np.exp(logvars / 2.0)[None, :, :]
    return -0.5 * np.sum(d ** 2, -1) - 0.5 * np.sum(logvars, -1)[None, :] - 0.5 * mus.shape[-1] * LN2PI


def sandwich_rows_literal(mus, logvars, u):
    """compute_infos_mus_logvars per row, literally: p = exp(l); infonce_i = log(p_ii / mean_j p_ij);
    loo_i = log(p_ii / mean_j p_ij (1 - delta_ij))  (divides by n).  Underflows to +-inf / nan for separated Gaussians."""
    p = np.exp(log_densities(u, mus, logvars))
    n = p.shape[0]
    pii = np.diag(p).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        lower = np.log(pii / np.mean(p, axis=1))
        upper = np.log(pii / np.mean(p * (1.0 - np.eye(n)), axis=1))
    return lower, upper


def sandwich_rows_lse(mus, logvars, u):
    """the same with a log-sum-exp: lower_i = l_ii - (LSE_j l_ij - log n), upper_i = l_ii - (LSE_{j != i} l_ij - log n)"""
    l = log_densities(u, mus, logvars)
    n = l.shape[0]
    lii = np.diag(l).copy()
    off = l.copy()
    np.fill_diagonal(off, -np.inf)
    return lii - (logsumexp(l, axis=1) - np.log(n)), lii - (logsumexp(off, axis=1) - np.log(n))


def sandwich_bounds(mus, logvars, u, form="lse"):
    lo, up = (sandwich_rows_lse if form == "lse" else sandwich_rows_literal)(mus, logvars, u)
    return float(np.mean(lo)), float(np.mean(up))


def probe_rows_lse(mus_p, logvars_p, u, mus_d, logvars_d):
    """one batch of the probe map: lower = l_ii - (LSE(l_ii, l_i1..l_iN) - log(N + 1)), upper = l_ii - (LSE(l_i1..l_iN) - log N)"""
    lii = np.diag(log_densities(u, mus_p, logvars_p)).copy()
    ld = log_densities(u, mus_d, logvars_d)
    N = ld.shape[1]
    lse_d = logsumexp(ld, axis=1)
    return lii - (np.logaddexp(lii, lse_d) - np.log(N + 1.0)), lii - (lse_d - np.log(N))


def information_plane(bce_series_val, acc_series_val, info_bounds, entropy_y=1.0, smoothing_sigma=1):
    """cell 8's tail: bits, gaussian_filter1d smoothing, info_in = mean of the bounds, info_out = entropy_y - BCE"""
    from scipy.ndimage import gaussian_filter1d
    bce = np.float32(bce_series_val) / np.log(2)
    acc = np.float32(acc_series_val)
    ib = np.float32(info_bounds) / np.log(2)
    info_in = np.mean(ib, axis=-1)
    bce_s = gaussian_filter1d(bce, smoothing_sigma)
    acc_s = gaussian_filter1d(acc, smoothing_sigma)
    start = -len(info_in)
    return info_in, entropy_y - bce_s[start:], acc_s[start:]
