"""Characterization of the mutual-information bounds on synthetic Gaussian channels (the reference's
complex_systems "Characterization of mutual information bounds with synthetic data" notebook, paper Fig. S4).

A fixed dataset of N points x is mapped to unit-variance Gaussians in U whose centres are x * separation_scale (zero-padded to
the embedding dimension).  For such a channel I(U;X) can be estimated by brute force - draw x from the dataset, u ~ p(u|x),
average log p(u|x) / p(u) with p(u) the plain mean of the N conditionals - and the InfoNCE lower / leave-one-out upper bounds that
every model of this package reports (utils.estimate_mi_sandwich_bounds, InfoPerFeatureCallback, CircuitIB, MeasurementIB,
SetTransformerDIB) can be compared with it at the evaluation batch sizes they are used at.

Device path: the Monte-Carlo estimate is ONE dib_mi_monte_carlo launch sequence (table prep, tiled terms kernel, combine:
include/dib_mi_channel.h, csrc/dib_mi_channel.h) over every (separation scale, run) pair of a sweep; the bounds of every
(separation scale, batch) pair at one evaluation batch size are one dib_mi_sandwich_batched launch sequence (include/dib_st.h).
float64 with a log-sum-exp throughout.  There is no CPU fallback: without a device these functions raise."""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple, Sequence, Tuple

import numpy as np

from . import utils

LN2 = float(np.log(2.0))
# Most (group, sample) source-row indices uploaded for one launch: 2^24 int32 = 64 MiB.  A sweep with more is cut into chunks of
# whole groups; a group's value does not depend on the chunk it lands in (include/dib_mi_channel.h).
MAX_INDICES_PER_LAUNCH = 1 << 24
MAX_GROUPS_PER_LAUNCH = 65535   # the kernel's grid


class Variable(NamedTuple):
    """One random variable X of the figure: its sampler(rng, sample_size) -> [sample_size, d], the sweep of separation scales and
    the axis limits (bits) of the two panels"""
    name: str
    label: str
    sample: Callable[[np.random.Generator, int], np.ndarray]
    separation_scales: np.ndarray
    info_plot_lims: Tuple[float, float]
    info_residual_lims: Tuple[float, float]


def _signs(k: int):
    return lambda rng, sample_size: rng.integers(0, 2, size=(int(sample_size), k)) * 2 - 1


# The four discrete variables of the figure (k fair bits, coded +-1 per dimension) and the notebook's continuous extra one
VARIABLES = (
    Variable("bits1", "X ~ U({0, 1})", _signs(1), np.linspace(0.0, 3.0, 25), (0.0, 1.2), (-0.1, 0.1)),
    Variable("bits2", "X ~ U({0, 1}^2)", _signs(2), np.linspace(0.0, 3.0, 25), (0.0, 2.4), (-0.1, 0.1)),
    Variable("bits4", "X ~ U({0, 1}^4)", _signs(4), np.linspace(0.0, 3.0, 25), (0.0, 4.5), (-0.1, 0.1)),
    Variable("bits6", "X ~ U({0, 1}^6)", _signs(6), np.linspace(0.0, 3.0, 25), (0.0, 6.5), (-0.1, 0.1)),
    Variable("uniform", "Gaussian smear: X ~ U([0, 1])",
             lambda rng, sample_size: rng.uniform(size=(int(sample_size), 1)) - 0.5, np.linspace(0.0, 100.0, 25), (0.0, 6.0),
             (-0.1, 0.1)),
)


def gaussian_channel(x_samples, separation_scale, embedding_dimension: int = 32, logvar: float = 0.):
    """(mus, logvars) [N, embedding_dimension] of the channel x -> N(x * separation_scale padded with zeros, exp(logvar) I)."""
    x = np.asarray(x_samples, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    if d > embedding_dimension:
        raise ValueError(f"x has {d} dimensions, the embedding only {embedding_dimension}")
    mus = np.concatenate([x * float(separation_scale), np.zeros((n, int(embedding_dimension) - d))], -1)
    return mus, np.ones_like(mus) * float(logvar)


def _tables(mus, logvars) -> Tuple[np.ndarray, bool]:
    """[S, N, 2E] float32 (mu | logvar) from [N, E] or [S, N, E] parameters; whether a stack was passed"""
    mus, logvars = np.asarray(mus, dtype=np.float32), np.asarray(logvars, dtype=np.float32)
    if mus.shape != logvars.shape or mus.ndim not in (2, 3):
        raise ValueError(f"mus {mus.shape} and logvars {logvars.shape} must both be [N, E] or [S, N, E]")
    stacked = mus.ndim == 3
    if not stacked:
        mus, logvars = mus[None], logvars[None]
    return np.ascontiguousarray(np.concatenate([mus, logvars], -1)), stacked


def monte_carlo_source_rows(seed: int, group: int, n_rows: int, mc_sample_size: int) -> np.ndarray:
    """The dataset rows the samples of Monte-Carlo group `group` (= scale index * runs + run) are drawn from: a function of
    (seed, group) alone, so that a sweep cut into launches - or one scale evaluated on its own - draws the same rows."""
    return np.random.default_rng([int(seed), int(group)]).integers(0, n_rows, int(mc_sample_size)).astype(np.int32)


def monte_carlo_information(mus, logvars, mc_sample_size: int = 10_000, number_monte_carlo_runs: int = 200, seed: int = 0, *,
                            group_offset: int = 0):
    """Monte-Carlo I(U;X) in bits of the channel x_j -> N(mus[j], diag exp(logvars[j])), X uniform over the N dataset rows
    (repeated rows count once per position): per run, mc_sample_size samples (row r drawn with replacement, u ~ p(u|x_r)) of
    log2 p(u|x_r) / mean_j p(u|x_j), averaged.

    mus / logvars: [N, E], or a stack [S, N, E] of S channels over datasets of equal size (all the separation scales of a sweep),
    evaluated together: group g = (channel s, run r) = s * number_monte_carlo_runs + r draws its rows by
    monte_carlo_source_rows(seed, group_offset + g, ...) and its noise from the library's counter-based generator keyed
    (seed, step group_offset + g, sample, 0).  `group_offset` places this call inside a larger sweep: channel s of a stack equals
    the single-channel call with group_offset = s * number_monte_carlo_runs, bit for bit.
    Returns (mean over runs of the per-run means [S] (a float for [N, E] input), per-run means [S, runs] ([runs])).
    One launch sequence while groups * mc_sample_size <= MAX_INDICES_PER_LAUNCH (the index upload: 64 MiB) and groups <= 65535."""
    import torch

    from ._host import stream_ptr
    from ._lib import check, load_library
    tables, stacked = _tables(mus, logvars)
    S, N, E2 = tables.shape
    E, ns, runs = E2 // 2, int(mc_sample_size), int(number_monte_carlo_runs)
    if runs < 1 or ns < 1:
        raise ValueError("mc_sample_size and number_monte_carlo_runs must be positive")
    if not torch.cuda.is_available():
        raise RuntimeError("monte_carlo_information needs a GPU (there is no CPU fallback)")
    lib = load_library()
    G = S * runs
    per_launch = max(1, min(MAX_GROUPS_PER_LAUNCH, MAX_INDICES_PER_LAUNCH // ns, G))
    need = int(lib.dib_mi_monte_carlo_workspace_bytes(S, N, E, per_launch, ns))
    if need < 0:
        raise ValueError(f"dib_mi_monte_carlo: outside the envelope (tables {S}, rows {N}, E {E}, samples {ns})")
    dev = torch.device("cuda", torch.cuda.current_device())
    tab_d = torch.from_numpy(tables).to(dev)
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=dev)
    means = torch.empty(G, dtype=torch.float64, device=dev)
    stream = stream_ptr(dev)
    for g0 in range(0, G, per_launch):
        g1 = min(G, g0 + per_launch)
        src = np.stack([monte_carlo_source_rows(seed, group_offset + g, N, ns) for g in range(g0, g1)])
        src_d = torch.from_numpy(src).to(dev)
        table_of = torch.from_numpy((np.arange(g0, g1) // runs).astype(np.int32)).to(dev)
        check(lib.dib_mi_monte_carlo(ctypes.c_void_p(tab_d.data_ptr()), S, N, E, ctypes.c_void_p(table_of.data_ptr()),
                                     ctypes.c_void_p(src_d.data_ptr()), g1 - g0, ns, int(seed) & (2 ** 64 - 1),
                                     (int(group_offset) + g0) & 0xFFFFFFFF, ctypes.c_void_p(means[g0:].data_ptr()),
                                     ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(ws.data_ptr()), stream),
              "dib_mi_monte_carlo")
    per_run = means.cpu().numpy().reshape(S, runs) / LN2
    mean = per_run.mean(axis=1)
    return (mean, per_run) if stacked else (float(mean[0]), per_run[0])


def characterize(x_samples, separation_scales, evaluation_batch_sizes: Sequence[int] = (64, 256, 1024),
                 number_evaluation_batches: int = 512, embedding_dimension: int = 32, mc_sample_size: int = 10_000,
                 number_monte_carlo_runs: int = 200, seed: int = 0):
    """The figure's data for one dataset x_samples [N, d]: for every separation scale the Monte-Carlo I(U;X) and, at every
    evaluation batch size, number_evaluation_batches (InfoNCE lower, leave-one-out upper) bound pairs on batches drawn with
    replacement from the dataset.  Bits.  Returns a dict:
      monte_carlo [S], monte_carlo_runs [S, runs],
      info_bound_estimates [len(evaluation_batch_sizes), S, number_evaluation_batches, 2],
      info_bound_stats [len(evaluation_batch_sizes), S, 4] = (mean lower, std lower, mean upper, std upper) over the batches,
      separation_scales [S], evaluation_batch_sizes.
    The channels of all scales are stacked: one Monte-Carlo launch sequence for the sweep (monte_carlo_information) and one
    sandwich launch sequence per evaluation batch size."""
    scales = np.asarray(separation_scales, dtype=np.float64).reshape(-1)
    params = [gaussian_channel(x_samples, s, embedding_dimension) for s in scales]
    mus, logvars = np.stack([p[0] for p in params]), np.stack([p[1] for p in params])
    S, N, _ = mus.shape
    nb = int(number_evaluation_batches)
    monte_carlo, runs = monte_carlo_information(mus, logvars, mc_sample_size, number_monte_carlo_runs, seed)
    tables, _ = _tables(mus, logvars)
    estimates = np.empty((len(evaluation_batch_sizes), S, nb, 2))
    for k, bs in enumerate(evaluation_batch_sizes):
        rows = np.random.default_rng([int(seed), 1 << 20, k]).integers(0, N, (S * nb, int(bs)))
        rows += np.repeat(np.arange(S) * N, nb)[:, None]    # batch (s, b) draws from table s of the stack
        estimates[k] = utils._sandwich_bounds_of_rows(tables.reshape(S * N, -1), rows, seed, k * S * nb).reshape(S, nb, 2) / LN2
    stats = np.stack([estimates[..., 0].mean(-1), estimates[..., 0].std(-1), estimates[..., 1].mean(-1),
                      estimates[..., 1].std(-1)], -1)
    return {"monte_carlo": monte_carlo, "monte_carlo_runs": runs, "info_bound_estimates": estimates, "info_bound_stats": stats,
            "separation_scales": scales, "evaluation_batch_sizes": [int(b) for b in evaluation_batch_sizes]}


def largest_residuals(result):
    """{batch size: (largest |mean lower - Monte Carlo|, largest |mean upper - Monte Carlo|)} over the sweep, bits"""
    mc, stats = np.asarray(result["monte_carlo"]), np.asarray(result["info_bound_stats"])
    return {int(bs): (float(np.abs(stats[k, :, 0] - mc).max()), float(np.abs(stats[k, :, 2] - mc).max()))
            for k, bs in enumerate(result["evaluation_batch_sizes"])}


def save_figure(result, path, label: str = "", info_plot_lims=None, info_residual_lims=(-0.1, 0.1)):
    """The figure's two panels for one variable from characterize's dict: on top the Monte-Carlo curve (black) and, per evaluation
    batch size, the mean lower (^) and upper (v) bounds with a +-1 std band; below, the bounds' residuals against the Monte-Carlo
    curve.  Writes `path` and returns the matplotlib Figure."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    scales, mc = np.asarray(result["separation_scales"]), np.asarray(result["monte_carlo"])
    stats = np.asarray(result["info_bound_stats"])
    fig = plt.figure(figsize=(8, 8))
    gs = fig.add_gridspec(2, 1, height_ratios=(3, 1), left=0.1, right=0.9, bottom=0.1, top=0.9, hspace=0.05)
    top, bottom = fig.add_subplot(gs[0]), fig.add_subplot(gs[1])
    top.plot(scales, mc, "k", lw=3, label="Monte Carlo")
    bottom.axhline(0.0, color="k", lw=1)
    for k, bs in enumerate(result["evaluation_batch_sizes"]):
        color = f"C{k}"
        for col, marker, kind in ((0, "^", "lower"), (2, "v", "upper")):
            mean, std = stats[k, :, col], stats[k, :, col + 1]
            top.plot(scales, mean, marker + "-", color=color, markersize=5, lw=2, label=f"{kind}, batch {bs}")
            top.fill_between(scales, mean - std, mean + std, color=color, alpha=0.4, lw=0)
            bottom.plot(scales, mean - mc, marker + "-", color=color, markersize=5, lw=2, label=f"{kind} residual, batch {bs}")
            bottom.fill_between(scales, mean - std - mc, mean + std - mc, color=color, alpha=0.4, lw=0)
    top.set_ylabel("Information (bits)")
    top.set_title(label)
    top.set_xticklabels([])
    top.legend(fontsize=8)
    if info_plot_lims is not None:
        top.set_ylim(*info_plot_lims)
    if info_residual_lims is not None:
        bottom.set_ylim(*info_residual_lims)
    bottom.set_xlabel("Separation scale")
    bottom.set_ylabel("Bound - Monte Carlo (bits)")
    fig.savefig(path)
    plt.close(fig)
    return fig
