"""Exhaustive subset information of a small discrete table: I(X_S;Y) in bits for every subset S of the features, the ranks of
subsets among those of their size, and the Shapley value of every feature with respect to I(X_S;Y) (SAGE).  This is the ground
truth the Boolean-circuit notebook compares the Distributed IB against (reference complex_systems/
InfoDecomp_Boolean_circuits.ipynb: cell 7's `all_mis` and rank colours, cell 10's Shapley values and logistic-regression
baseline), for any empirical sample of up to 20 key bits and 16 classes.

Arithmetic (include/dib_subsets.h; the same rule on both backends).  Key of a row: its features' bit fields concatenated,
feature 0 lowest, B = sum(feature_bits).  T[key][k] = the number of rows with that key and class k, N = the number of rows.  For
a subset S, c[a][k] = the sum of T over the keys that agree with pattern a on S's bits, c[a] = sum_k c[a][k]:
    E[S] = sum_a xlog2(c[a]) - sum_{a,k} xlog2(c[a][k]),    xlog2(c) = c log2(c), xlog2(0) = 0
    H(Y) = (xlog2(N) - sum_k xlog2(n_k)) / N,    I(X_S;Y) = H(Y) - E[S] / N,    I of the empty subset = 0.0
`backend="device"`: T is counted on the host (np.bincount), uploaded as int32, and one dib_subset_information launch computes all
2^F values (csrc/dib_subsets.h); there is no CPU fallback behind it.  `backend="host"`: float64 NumPy, no GPU needed."""
from __future__ import annotations

import ctypes
from math import comb
from typing import Optional, Sequence

import numpy as np

MAX_BITS, MAX_CLASSES = 20, 16   # include/dib_subsets.h envelope


def subset_masks(all_on_off_combos) -> np.ndarray:
    """Notebook-ordered 0/1 inclusion rows [n, F] (cell 7: meshgrid 'xy' order, cell 10: 'ij') -> subset masks [n] (bit f set
    when column f is 1): `bits[subset_masks(all_on_off_combos)]` is the notebook's `all_mis`."""
    c = np.asarray(all_on_off_combos)
    if c.ndim != 2 or not np.isin(c, (0, 1)).all():
        raise ValueError("all_on_off_combos is [n, F] of 0 / 1")
    return (c.astype(np.int64) << np.arange(c.shape[1], dtype=np.int64)).sum(axis=1)


def _mask_of(subset, number_features: int) -> int:
    """a subset given as a mask (int) or as a sequence of feature indices"""
    if isinstance(subset, (int, np.integer)):
        m = int(subset)
    else:
        m = 0
        for f in subset:
            if not 0 <= int(f) < number_features:
                raise ValueError(f"feature {f} outside 0 .. {number_features - 1}")
            m |= 1 << int(f)
    if not 0 <= m < 1 << number_features:
        raise ValueError(f"subset mask {m} outside 0 .. 2^{number_features} - 1")
    return m


class SubsetInformation:
    """I(X_S;Y) of every subset of F features.  bits [2^F] float64 indexed by subset mask (bit f set when feature f is in S),
    entropy_y_bits, number_features."""

    def __init__(self, bits: np.ndarray, entropy_y_bits: float, number_features: int):
        self.bits = np.asarray(bits, dtype=np.float64)
        self.entropy_y_bits = float(entropy_y_bits)
        self.number_features = int(number_features)
        assert self.bits.shape == (1 << self.number_features,)
        masks = np.arange(1 << self.number_features, dtype=np.int64)
        self._sizes = np.zeros(masks.shape, dtype=np.int64)
        for f in range(self.number_features):
            self._sizes += (masks >> f) & 1

    def by_size(self, k: int):
        """(masks, bits) of the subsets of k features, by descending information; ties by ascending mask"""
        masks = np.where(self._sizes == int(k))[0]      # ascending
        order = np.argsort(-self.bits[masks], kind="stable")
        return masks[order], self.bits[masks[order]]

    def rank(self, subset) -> int:
        """position of `subset` (a mask or a sequence of feature indices) among the subsets of its size, 0 = the most
        informative: cell 7's colour index"""
        m = _mask_of(subset, self.number_features)
        masks, _ = self.by_size(int(self._sizes[m]))
        return int(np.where(masks == m)[0][0])

    def shapley_values(self) -> np.ndarray:
        """cell 10 (SAGE): phi_i = (1/F) sum_{S not containing i} (bits[S | i] - bits[S]) / C(F - 1, |S|), float64 [F], summed
        in ascending mask order"""
        F = self.number_features
        masks = np.arange(1 << F, dtype=np.int64)
        weight = np.array([1.0 / comb(F - 1, s) for s in range(F)])
        phi = np.zeros(F)
        for i in range(F):
            without = masks[(masks >> i) & 1 == 0]
            phi[i] = np.sum((self.bits[without | (1 << i)] - self.bits[without]) * weight[self._sizes[without]]) / F
        return phi

    def ceiling(self, kept_mask) -> float:
        """I(X_S;Y) of the kept features: the most predictive information a model that sees only them can have"""
        return float(self.bits[_mask_of(kept_mask, self.number_features)])


# ---- the table ----------------------------------------------------------------------------------------------------------
def joint_counts(x, y, feature_bits: Optional[Sequence[int]] = None):
    """(T [2^B, K] int64, feature_bits list, K) of an empirical sample: x [N, F] integers or the +-1 / 0,1 floats of the datasets
    (a 1-bit feature is x > 0; a b-bit feature holds values in [0, 2^b)), y [N] or [N, 1] integer classes >= 0."""
    x = np.asarray(x)
    y = np.asarray(y)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x is [N, F] with N, F >= 1; got shape {x.shape}")
    if not (y.ndim == 1 or (y.ndim == 2 and y.shape[1] == 1)):
        raise ValueError(f"y is [N] or [N, 1] class indices; got shape {y.shape}")
    y = y.reshape(-1)
    if y.shape[0] != x.shape[0]:
        raise ValueError(f"x has {x.shape[0]} rows, y {y.shape[0]}")
    if x.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    F = x.shape[1]
    fb = [1] * F if feature_bits is None else [int(b) for b in feature_bits]
    if len(fb) != F or min(fb) < 1:
        raise ValueError(f"feature_bits needs {F} widths >= 1; got {fb}")
    B = sum(fb)
    if B > MAX_BITS:
        raise ValueError(f"{B} key bits: the exhaustive table is limited to {MAX_BITS} bits ({F} features of widths {fb})")
    if not np.all(np.isfinite(y)) or np.any(y != np.floor(y)) or y.min() < 0:
        raise ValueError("y holds class indices: integers >= 0")
    y = y.astype(np.int64)
    K = int(y.max()) + 1
    if K > MAX_CLASSES:
        raise ValueError(f"{K} classes: at most {MAX_CLASSES}")
    key = np.zeros(x.shape[0], dtype=np.int64)
    off = 0
    for f, b in enumerate(fb):
        col = x[:, f]
        if b == 1 and feature_bits is None:
            v = (col > 0).astype(np.int64)
        else:
            if np.any(col != np.floor(col)) or col.min() < 0 or col.max() >= 1 << b:
                raise ValueError(f"feature {f} has values outside its {b}-bit field [0, {1 << b})")
            v = col.astype(np.int64)
        key |= v << off
        off += b
    T = np.bincount(key * K + y, minlength=(1 << B) * K).reshape(1 << B, K)
    return T, fb, K


def _xlog2(c):
    c = np.asarray(c, dtype=np.float64)
    return c * np.log2(np.where(c > 0, c, 1.0))


def _term(t):
    """sum over the leading axes' rows of xlog2(sum_k) - sum_k xlog2, for a table [..., K]"""
    return _xlog2(t.sum(-1)) - _xlog2(t).sum(-1)


_HOST_LOW_BITS = 6


def _host_key_mask_terms(T: np.ndarray) -> np.ndarray:
    """E[M] for every mask M of key bits, float64 [2^B]: a depth-first walk over the high bits (a dropped bit halves the table, a
    kept bit joins the pattern axis), the low bits of every leaf through the ternary lattice at once"""
    B = int(T.shape[0]).bit_length() - 1
    K = T.shape[1]
    low = min(B, _HOST_LOW_BITS)
    E = np.zeros(1 << B)
    # the low subsets as index tuples into a [3] * low array whose axis i is key bit low - 1 - i: 2 = summed out
    low_index = []
    for s in range(1 << low):
        low_index.append(tuple(slice(0, 2) if (s >> (low - 1 - i)) & 1 else 2 for i in range(low)))

    def leaf(tab, mask):
        # tab [P, 2^low, K] -> [P, 2, ..., 2, K] -> [P, 3, ..., 3, K]
        t = tab.reshape((tab.shape[0],) + (2,) * low + (K,))
        for ax in range(1, low + 1):
            t = np.concatenate([t, t.sum(axis=ax, keepdims=True)], axis=ax)
        e = _term(t).sum(0)
        for s, idx in enumerate(low_index):
            E[mask | s] = e[idx].sum()

    def walk(tab, j, mask):
        # tab [P, 2^j, K]: bits j - 1 .. 0 undecided
        if j == low:
            leaf(tab, mask)
            return
        half = tab.shape[1] // 2
        t = tab.reshape(tab.shape[0], 2, half, K)
        walk(t[:, 0] + t[:, 1], j - 1, mask)
        walk(t.reshape(tab.shape[0] * 2, half, K), j - 1, mask | 1 << (j - 1))

    walk(T.astype(np.int64).reshape(1, 1 << B, K), B, 0)
    return E


def _feature_key_masks(fb: Sequence[int]) -> np.ndarray:
    """key mask of every feature subset [2^F]"""
    F = len(fb)
    masks = np.arange(1 << F, dtype=np.int64)
    out = np.zeros(1 << F, dtype=np.int64)
    off = 0
    for f, b in enumerate(fb):
        out |= ((masks >> f) & 1) * (((1 << b) - 1) << off)
        off += b
    return out


def entropy_y_from_counts(T: np.ndarray) -> float:
    n_k = T.sum(0)
    n = int(n_k.sum())
    return float((_xlog2(n) - _xlog2(n_k).sum()) / n)


def _host_bits(T, fb):
    n = int(T.sum())
    E = _host_key_mask_terms(T)[_feature_key_masks(fb)]
    bits = entropy_y_from_counts(T) - E / n
    bits[0] = 0.0
    return bits


def _device_bits(T, fb, K, device="cuda:0"):
    import torch
    from . import _lib
    from ._host import stream_ptr
    if not torch.cuda.is_available():
        raise RuntimeError("subset_information(backend='device') runs on the GPU (libdib_hip); no device is available - "
                           "backend='host' is the float64 NumPy rule")
    lib = _lib.load_library()
    F, B = len(fb), sum(fb)
    if not lib.dib_subset_information_supported(B, F, K):
        raise ValueError(f"{B} key bits / {F} features / {K} classes outside the kernel's envelope "
                         f"(1 <= F <= B <= {MAX_BITS}, K <= {MAX_CLASSES})")
    dev = torch.device(device)
    counts = torch.from_numpy(T.astype(np.int32)).to(dev)
    out = torch.empty(1 << F, dtype=torch.float64, device=dev)
    nws = int(lib.dib_subset_information_workspace_bytes(B, K))
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
    widths = (ctypes.c_int * F)(*fb)
    _lib.check(lib.dib_subset_information(ctypes.c_void_p(counts.data_ptr()), B, K, widths, F, 0, 1 << F,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                          stream_ptr(dev)), "dib_subset_information")
    return out.cpu().numpy()


def subset_information(x, y, feature_bits: Optional[Sequence[int]] = None, backend: str = "device") -> SubsetInformation:
    """I(X_S;Y) in bits of every subset of the features of the sample (x [N, F], y [N] or [N, 1]); rows are an empirical sample
    (duplicates and missing patterns are fine, a full truth table is the special case).  feature_bits[f]: the bit width of
    feature f (default 1: a binary feature with value x > 0; a width b takes values in [0, 2^b)).  backend "device" (one
    dib_subset_information launch) or "host" (float64 NumPy, no GPU)."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend is 'device' or 'host'; got {backend!r}")
    T, fb, K = joint_counts(x, y, feature_bits)
    bits = _host_bits(T, fb) if backend == "host" else _device_bits(T, fb, K)
    return SubsetInformation(bits, entropy_y_from_counts(T), len(fb))


# ---- cell 10's baseline -----------------------------------------------------------------------------------------------------
def logistic_regression_baseline(table) -> dict:
    """cell 10: LogisticRegression(penalty=None, random_state=0) on a truth table [rows, G + 1] (0/1 inputs, y last).  Returns
    coefficients [G], intercept, accuracy and information_bits = H(Y) - cross-entropy of its predicted probabilities (bits).
    Host only; scikit-learn is imported here."""
    from sklearn.linear_model import LogisticRegression
    t = np.asarray(table)
    x, y = t[:, :-1], t[:, -1].astype(np.int64)
    clf = LogisticRegression(random_state=0, penalty=None, max_iter=10000).fit(x, y)
    p = np.clip(clf.predict_proba(x)[np.arange(len(y)), np.searchsorted(clf.classes_, y)], 1e-300, 1.0)
    hy = entropy_y_from_counts(np.bincount(y).reshape(1, -1))
    return {"coefficients": clf.coef_.reshape(-1).copy(), "intercept": float(clf.intercept_[0]),
            "accuracy": float(np.average(clf.predict(x) == y)), "information_bits": float(hy + np.mean(np.log2(p)))}


# ---- cell 7's figure ----------------------------------------------------------------------------------------------------------
def save_subset_information_figure(info: SubsetInformation, out_fname: str, selected=(), info_in_full=None,
                                   predictive_information_out=None, plot_start_ind: int = 5) -> str:
    """cell 7: every subset's I(X_S;Y) against its size (black), the subsets the Distributed IB selected blown up and coloured by
    their rank among the subsets of their size (blue = best, orange second, ... matplotlib's cycle), the DIB's curve (total
    information in, predictive information out; optional) and H(Y) dotted."""
    from .visualization import _plt, default_mpl_colors
    plt = _plt()
    fig = plt.figure(figsize=(10, 5))
    ax = fig.gca()
    F = info.number_features
    chosen = {_mask_of(s, F) for s in selected}
    for k in range(1, F + 1):
        masks, bits = info.by_size(k)
        ax.scatter(np.ones(len(bits)) * k, bits, s=50, c='k')
        for r, (m, b) in enumerate(zip(masks, bits)):
            if int(m) in chosen:
                ax.scatter(k, b, s=150, c=default_mpl_colors[r % len(default_mpl_colors)], zorder=3)
    if info_in_full is not None and predictive_information_out is not None:
        ax.plot(np.asarray(info_in_full)[plot_start_ind:], np.asarray(predictive_information_out)[plot_start_ind:], lw=4, color='k')
    ax.plot([-1, F + 1], [info.entropy_y_bits] * 2, 'k:', lw=2)
    ax.set_xlabel('Total information about inputs, I(Ui;Xi) (bits)', fontsize=15)
    ax.set_ylabel('Predictive information, I(U;Y) (bits)', fontsize=15)
    ax.set_xlim([0, F + 0.5])
    ax.set_ylim([0, max(1.0, info.entropy_y_bits * 1.05)])
    ax.tick_params(which='both', width=2, length=8, direction='in')
    fig.savefig(out_fname, dpi=150)
    plt.close(fig)
    return out_fname


def save_subset_information(info: SubsetInformation, outdir: str, **figure_kwargs) -> str:
    """subset_information.npz (masks, bits, entropy_y_bits, shapley_values) and subset_information.png in `outdir`"""
    import os
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "subset_information.npz")
    np.savez(path, masks=np.arange(info.bits.shape[0], dtype=np.int64), bits=info.bits,
             entropy_y_bits=np.float64(info.entropy_y_bits), shapley_values=info.shapley_values())
    save_subset_information_figure(info, os.path.join(outdir, "subset_information.png"), **figure_kwargs)
    return path
