"""Artefacts of the hot path's callbacks, mirroring reference visualization.py:
  save_compression_matrices (visualization.py:14-81) and save_distributed_info_plane (:83-113).
The sampling rule and the exp(-Bhattacharyya) matrix follow the reference (with SURVEY App. A
defects A2 fixed); the figure layout is this project's own.
"""
from __future__ import annotations

import os

import numpy as np

from . import utils

default_mpl_colors = ['#1f77b4', '#ff7f0e', '#2ca02c', '#d62728', '#9467bd', '#8c564b', '#e377c2', '#7f7f7f',
                      '#bcbd22', '#17becf']


def _plt():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def select_display_inputs(inp_features_raw, max_number_to_display=128, rng=None):
    """reference visualization.py:17-28: <10 unique raw values -> evaluate exactly those (histogram mode);
    otherwise `max_number_to_display` random rows, sorted by raw value.  Returns
    (indices into the feature rows, sorted raw values, value frequencies or None)."""
    raw = np.asarray(inp_features_raw)
    unique_vals, unique_idx = np.unique(raw, return_index=True)
    if len(unique_vals) < 10:
        counts = [np.average(raw == v) for v in unique_vals]
        return unique_idx[np.argsort(unique_vals)], np.sort(unique_vals), counts
    return _draw_display_inputs(raw, max_number_to_display, rng)


def _draw_display_inputs(raw, max_number_to_display, rng):
    """the random branch of select_display_inputs: `max_number_to_display` rows drawn with replacement, sorted by raw value"""
    rng = rng or np.random
    sel = rng.choice(raw.shape[0], max_number_to_display)
    flat = raw[sel].reshape(len(sel), -1)[:, 0]
    order = np.argsort(flat)
    return sel[order], flat[order], None


def display_rows(x_raw, feature_dimensionalities, max_number_to_display=128, rng=None, cache=None):
    """The display sample of EVERY feature by the host rule: select_display_inputs on the columns of features 0 .. F-1 of
    x_raw [N, sum d_f], in that order - with the same `rng` exactly the rows the per-feature loop of
    SaveCompressionMatricesCallback draws.  Returns a dict:
      "indices" / "values" / "counts": per feature what select_display_inputs returns (row indices, sorted raw values, value
                 frequencies or None);
      "rows":    int32 [F, n_max], feature f's indices padded to the longest sample with its own first index;
      "n_rows":  int32 [F], the sample sizes (the `counts` of engine.compression_matrices).
    `cache` (a dict the caller keeps between calls on the same x_raw) stores what does not change from call to call: the
    selections of features with < 10 unique values - they are deterministic and consume no random draw - and, for the others,
    that they are drawn at random (cache[f] = None): a later call draws them without sorting the whole column for np.unique
    again, with the same draws of `rng`."""
    x_raw = np.asarray(x_raw)
    if x_raw.ndim == 1:
        x_raw = x_raw.reshape(-1, 1)
    dims = [int(d) for d in feature_dimensionalities]
    split = np.split(x_raw, np.cumsum(dims)[:-1], axis=-1)
    sel = []
    for f, raw_f in enumerate(split):
        if cache is not None and f in cache:
            s = cache[f] if cache[f] is not None else _draw_display_inputs(raw_f, max_number_to_display, rng)
        else:
            s = select_display_inputs(raw_f, max_number_to_display, rng)
            if cache is not None:
                cache[f] = s if s[2] is not None else None
        sel.append(s)
    n_rows = np.asarray([len(s[0]) for s in sel], dtype=np.int32)
    rows = np.empty((len(sel), max(1, int(n_rows.max()))), dtype=np.int32)
    for f, s in enumerate(sel):
        rows[f] = s[0][0] if len(s[0]) else 0
        rows[f, :len(s[0])] = s[0]
    return dict(indices=[s[0] for s in sel], values=[s[1] for s in sel], counts=[s[2] for s in sel], rows=rows, n_rows=n_rows)


def encoded_compression_matrix(feature_encoder, inputs, model=None):
    """(exp(-D), D) for D the Bhattacharyya distances between the Gaussians feature_encoder assigns to `inputs` [n, d_f]: the
    model engine's kernel when it has one, else utils.bhattacharyya_dist_mat."""
    enc = np.asarray(feature_encoder(inputs))
    emb_mus, emb_logvars = np.split(enc, 2, axis=-1)
    if model is not None and getattr(model, "_engine", None) is not None and hasattr(model._engine, "bhattacharyya"):
        bhat = model._engine.bhattacharyya(emb_mus, emb_logvars, emb_mus, emb_logvars).detach().cpu().numpy()
    else:
        bhat = utils.bhattacharyya_dist_mat(emb_mus, emb_logvars, emb_mus, emb_logvars)
    return np.exp(-bhat), bhat


def draw_compression_matrix(matrix, sorted_raw, counts, out_fname, feature_label=None):
    """The figure of one compression matrix: the matrix, and along its left and top edges the displayed raw values (a curve
    over the sample, or the value histogram when `counts` - the value frequencies - is given).  Saved to out_fname."""
    plt = _plt()
    n = len(sorted_raw)
    fig = plt.figure(figsize=(6, 6))
    gs = fig.add_gridspec(2, 2, width_ratios=(1, 2), height_ratios=(1, 2), left=0.1, right=0.9, bottom=0.1,
                          top=0.9, wspace=0.05, hspace=0.05)
    ax = fig.add_subplot(gs[1, 1])
    ax.imshow(matrix, vmin=0, vmax=1, cmap='Blues_r')
    ax.axis('off')
    axl = fig.add_subplot(gs[1, 0])
    axt = fig.add_subplot(gs[0, 1])
    if counts is not None:
        axl.barh(sorted_raw, counts, height=0.8)
        axt.bar(sorted_raw, counts, width=0.8)
        axl.set_xlim(0, 1)
        axt.set_ylim(0, 1)
    else:
        axl.plot(sorted_raw, np.arange(n), 'k', lw=3)
        axl.set_ylim(n, 0)
        axt.plot(np.arange(n), sorted_raw, 'k', lw=3)
        axt.set_xlim(0, n)
    for a in (axl, axt):
        a.set_xticks([]) if a is axt or counts is not None else None
        a.set_yticks([]) if a is axl and counts is None else None
        for s in ('right', 'top'):
            a.spines[s].set_visible(False)
    ax0 = fig.add_subplot(gs[0, 0])
    ax0.text(0, 0, feature_label if feature_label is not None else '')
    ax0.set_xlim(-0.5, 0.5)
    ax0.set_ylim(-0.5, 0.5)
    ax0.axis('off')
    fig.savefig(out_fname)
    plt.close(fig)


def save_compression_matrices(feature_encoder, inp_features, out_fname, inp_features_raw=None, feature_label=None,
                              max_number_to_display=128, model=None, rng=None):
    """Encode a sample of feature values (deterministically), compute exp(-Bhattacharyya) between
    their Gaussians, save as PNG (if out_fname) and return the matrix."""
    inp_features = np.asarray(inp_features)
    if inp_features_raw is None:
        inp_features_raw = inp_features
    inds, sorted_raw, counts = select_display_inputs(inp_features_raw, max_number_to_display, rng)
    compression_matrix, _ = encoded_compression_matrix(feature_encoder, inp_features[inds], model)
    if out_fname:
        draw_compression_matrix(compression_matrix, sorted_raw, counts, out_fname, feature_label)
    return compression_matrix


def save_distributed_info_plane(kl_series, loss_series, outdir, entropy_y=None):
    """Distributed information plane (reference visualization.py:83-113): total KL (bits) on x,
    task loss on y (black), per-feature KL on a twin axis.  kl_series [epochs, F] in bits."""
    kl_series = np.asarray(kl_series)
    loss_series = np.asarray(loss_series)
    number_features = kl_series.shape[1]
    desired = min(1000, kl_series.shape[0])
    sieve = max(1, kl_series.shape[0] // desired)
    start = desired // 2
    parts = kl_series[::sieve]
    full = np.sum(parts, axis=-1)
    perf = loss_series[::sieve]
    lims = [0, 15]
    plt = _plt()
    fig = plt.figure(figsize=(8, 4))
    ax = fig.gca()
    ax.plot(full[start:], perf[start:], lw=4, color='k')
    if entropy_y is not None:
        ax.plot(lims, [entropy_y] * 2, 'k:')
    ax.set_xlim(lims)
    if number_features > 1:
        ax2 = ax.twinx()
        for f in range(number_features):
            ax2.plot(full[start:], parts[start:, f], color=default_mpl_colors[f % len(default_mpl_colors)], lw=4)
        ax.set_zorder(ax2.get_zorder() + 1)
        ax.patch.set_visible(False)
    os.makedirs(outdir, exist_ok=True)
    saveto = os.path.join(outdir, 'distributed_info_plane.png')
    fig.savefig(saveto, dpi=150)
    plt.close(fig)
    return saveto


def save_distributed_info_plane_replicas(kl_series, loss_series, outdir, entropy_y=None):
    """save_distributed_info_plane for R replicas of one model (train.py --repeats) overlaid in one figure: kl_series
    [R, epochs, F] in bits, loss_series [R, epochs].  Every replica's curve (total KL against the task loss) is drawn thin and
    black, its per-feature KL thin on the twin axis in the feature's colour, with the sieve and the starting point of
    save_distributed_info_plane.  Writes distributed_info_plane_replicas.png."""
    kl_series, loss_series = np.asarray(kl_series), np.asarray(loss_series)
    R, epochs, number_features = kl_series.shape
    desired = min(1000, epochs)
    sieve = max(1, epochs // desired)
    start = desired // 2
    lims = [0, 15]
    plt = _plt()
    fig = plt.figure(figsize=(8, 4))
    ax = fig.gca()
    ax2 = ax.twinx() if number_features > 1 else None
    for r in range(R):
        parts = kl_series[r, ::sieve]
        full = np.sum(parts, axis=-1)
        ax.plot(full[start:], loss_series[r, ::sieve][start:], lw=1.5, color='k', alpha=0.6)
        if ax2 is not None:
            for f in range(number_features):
                ax2.plot(full[start:], parts[start:, f], color=default_mpl_colors[f % len(default_mpl_colors)], lw=1.5, alpha=0.6)
    if entropy_y is not None:
        ax.plot(lims, [entropy_y] * 2, 'k:')
    ax.set_xlim(lims)
    if ax2 is not None:
        ax.set_zorder(ax2.get_zorder() + 1)
        ax.patch.set_visible(False)
    os.makedirs(outdir, exist_ok=True)
    saveto = os.path.join(outdir, 'distributed_info_plane_replicas.png')
    fig.savefig(saveto, dpi=150)
    plt.close(fig)
    return saveto


def save_distributed_info_plane_mi(information, loss_series, outdir, entropy_y=None):
    """The distributed information plane in mutual-information bounds instead of KL: `information` is History.information of
    DistributedIBNet.fit(track_information=...) - "bounds" [n_evals, F, 2] (InfoNCE lower, leave-one-out upper) in nats, "epochs"
    [n_evals].  x: the summed mean-of-bounds (bits), with the band between the summed lower and upper bounds; y: the task loss
    of those epochs (black; `loss_series` is either one value per epoch, indexed by "epochs", or one per evaluation); per-feature
    mean-of-bounds on a twin axis.  A bound that is not finite (the upper bound of channels far apart) is drawn as its lower
    bound.  Writes distributed_info_plane_mi.png next to save_distributed_info_plane's file."""
    bounds = np.asarray(information["bounds"], dtype=np.float64) / np.log(2.0)
    epochs = np.asarray(information["epochs"], dtype=np.int64)
    if bounds.ndim != 3 or bounds.shape[2] != 2 or bounds.shape[0] != epochs.shape[0]:
        raise ValueError(f"information['bounds'] {bounds.shape} must be [n_evals, F, 2] with one entry of 'epochs' each")
    loss_series = np.asarray(loss_series, dtype=np.float64).reshape(-1)
    perf = loss_series if loss_series.shape[0] == epochs.shape[0] else loss_series[epochs]
    lower = bounds[..., 0]
    upper = np.where(np.isfinite(bounds[..., 1]), bounds[..., 1], lower)
    mid = 0.5 * (lower + upper)
    number_features = bounds.shape[1]
    full = np.sum(mid, axis=-1)
    plt = _plt()
    fig = plt.figure(figsize=(8, 4))
    ax = fig.gca()
    ax.fill_betweenx(perf, np.sum(lower, -1), np.sum(upper, -1), color='k', alpha=0.15, lw=0)
    ax.plot(full, perf, lw=4, color='k')
    hi = max(1.0, float(np.max(np.sum(upper, -1), initial=0.0)))
    if entropy_y is not None:
        ax.plot([0, hi], [entropy_y] * 2, 'k:')
    ax.set_xlim([0, hi])
    ax.set_xlabel('information about the features (bits)')
    if number_features > 1:
        ax2 = ax.twinx()
        for f in range(number_features):
            ax2.plot(full, mid[:, f], color=default_mpl_colors[f % len(default_mpl_colors)], lw=2)
        ax.set_zorder(ax2.get_zorder() + 1)
        ax.patch.set_visible(False)
    os.makedirs(outdir, exist_ok=True)
    saveto = os.path.join(outdir, 'distributed_info_plane_mi.png')
    fig.savefig(saveto, dpi=150)
    plt.close(fig)
    return saveto
