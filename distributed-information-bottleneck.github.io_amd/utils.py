"""Host-side analysis helpers mirroring the reference's `utils.py` names that the hot path's callbacks
touch (reference utils.py:177-262).  The Bhattacharyya / KL matrices use the closed form for
diagonal Gaussians instead of the reference's dense [N,M,d,d] diagonal tensors (same values, see
tests/test_oracle_golden.py); the on-device version is dib_bhattacharyya (csrc/dib_elementwise.h).
"""
from __future__ import annotations

import numpy as np


def bhattacharyya_dist_mat(mus1, logvars1, mus2, logvars2):
    """[N, M] Bhattacharyya distances between diagonal Gaussians (reference utils.py:177-212)."""
    mu1 = np.asarray(mus1, dtype=np.float64)[:, None, :]
    mu2 = np.asarray(mus2, dtype=np.float64)[None, :, :]
    lv1 = np.asarray(logvars1, dtype=np.float64)[:, None, :]
    lv2 = np.asarray(logvars2, dtype=np.float64)[None, :, :]
    assert mu1.shape[-1] == mu2.shape[-1]
    sbar = 0.5 * (np.exp(lv1) + np.exp(lv2))
    term1 = 0.125 * np.sum((mu1 - mu2) ** 2 / sbar, axis=-1)
    term2 = 0.5 * (np.sum(np.log(sbar), axis=-1) - 0.5 * (np.sum(lv1, -1) + np.sum(lv2, -1)))
    return term1 + term2


def kl_divergence_mat(mus1, logvars1, mus2, logvars2):
    """[N, M] KL(N1 || N2) (reference utils.py:214-246)."""
    mu1 = np.asarray(mus1, dtype=np.float64)[:, None, :]
    mu2 = np.asarray(mus2, dtype=np.float64)[None, :, :]
    lv1 = np.asarray(logvars1, dtype=np.float64)[:, None, :]
    lv2 = np.asarray(logvars2, dtype=np.float64)[None, :, :]
    d = mu1.shape[-1]
    return 0.5 * (np.sum(lv2, -1) - np.sum(lv1, -1) - d + np.sum(np.exp(lv1 - lv2), -1)
                  + np.sum((mu2 - mu1) ** 2 * np.exp(-lv2), -1))


def compute_entropy_bits(probability_arr):
    """reference utils.py:248-249."""
    p = np.asarray(probability_arr, dtype=np.float64)
    return -np.sum(p * np.log2(np.where(p > 0, p, 1)))


def compute_entropy(seq):
    """reference utils.py:257-261: empirical entropy (bits) of a symbol sequence."""
    _, counts = np.unique(seq, return_counts=True)
    p = counts / np.sum(counts)
    return -np.sum(p * np.log2(p))


def entropy_rate_scaling_ansatz(N, h_inf, gamma, c):
    """reference utils.py:251-254 (Schurmann & Grassberger 1995)."""
    return h_inf + np.log2(N) / (N ** gamma) / np.abs(c)


def evaluation_batch_rows(n_rows, evaluation_batch_size, number_evaluation_batches, seed):
    """The dataset rows of the evaluation batches of estimate_mi_sandwich_bounds: int64 [number_evaluation_batches,
    evaluation_batch_size].  One np.random.default_rng(seed); per batch a shuffle without replacement (permutation(n)[:bs]),
    or bs draws with replacement when the dataset has fewer rows than a batch.  Every feature of a model draws the same rows:
    the rule takes nothing from the encoder."""
    n, bs = int(n_rows), int(evaluation_batch_size)
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
                     for _ in range(int(number_evaluation_batches))]).astype(np.int64).reshape(-1, bs)


def estimate_mi_sandwich_bounds(encoder, dataset, evaluation_batch_size=1024, number_evaluation_batches=8, seed=0):
    """Lower (InfoNCE) and upper (leave-one-out) bounds, in nats, on the information transmitted by one feature
    encoder (reference utils.py:10-73; Poole et al. 2019).

    `encoder` is `model.feature_encoders[f]`; `dataset` is that feature's data, array-like [N, d_f] (the reference
    takes a tf.data.Dataset and draws `number_evaluation_batches` shuffled batches with wrap-around, utils.py:68-71;
    here the batches are drawn with a seeded numpy generator).  The N x N x E pairwise Gaussian log-densities are
    evaluated on the GPU in float64 with a log-sum-exp (dib_mi_sandwich_rows), so well separated encodings give
    log N instead of the reference's underflow."""
    x = np.asarray(dataset, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    n = x.shape[0]
    bs = int(evaluation_batch_size)
    rng = np.random.default_rng(seed)
    if getattr(encoder, "_encoder", False):   # MeasurementIB.info_bott_encoder (chaos notebook cell 10): its [N, 2E] output
        return _encoder_mi_bounds(encoder, encoder._measurement, 0, x, n, bs, rng, int(number_evaluation_batches), seed)
    if getattr(encoder, "_circuit", None) is not None:   # CircuitIB.feature_encoders[g] (Boolean-circuit notebook cell 4): one
        # gate's [bs, 2] output, the per-gate form of CircuitIB.estimate_channel_mi_bounds' one-launch evaluation
        return _encoder_mi_bounds(encoder, encoder._circuit, encoder.index, x, n, bs, rng, int(number_evaluation_batches), seed)
    model = encoder._model
    eng = model._ensure_engine()
    estimates = []
    for b, rows in enumerate(evaluation_batch_rows(n, bs, number_evaluation_batches, seed)):
        enc_out = eng.encode_feature(encoder.index, x[rows])
        estimates.append(eng.mi_sandwich_bounds(enc_out, seed, b, encoder.index))
    return np.mean(np.stack(estimates, 0), 0)


def mi_sandwich_rows(lib, device, enc_out, seed, step, feature):
    """dib_mi_sandwich_rows on one batch: enc_out is a float32 tensor [n, 2E] (mu | logvar) on `device`, the noise is keyed
    (seed, step, row, feature).  Returns (lower_rows, upper_rows) in nats as the two rows of one float64 device tensor [2, n];
    the launches go to the current stream and nothing waits for them."""
    import torch

    from ._gemm_plan import _ptr
    from ._host import stream_ptr
    from ._lib import check
    enc_out = enc_out.contiguous()
    n, e = enc_out.shape[0], enc_out.shape[1] // 2
    ws = torch.empty(int(lib.dib_mi_workspace_bytes(n, e)) // 8 + 1, dtype=torch.float64, device=device)
    rows = torch.empty((2, n), dtype=torch.float64, device=device)
    check(lib.dib_mi_sandwich_rows(_ptr(enc_out), n, e, int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, int(feature),
                                   _ptr(rows[0]), _ptr(rows[1]), _ptr(ws),
                                   stream_ptr(device)), "dib_mi_sandwich_rows")
    return rows


def _encoder_mi_bounds(encoder, m, feature, x, n, bs, rng, number_evaluation_batches, seed):
    """batch by batch through mi_sandwich_rows on the output of a callable encoder owned by model `m` (its library and device)"""
    estimates = []
    for b in range(number_evaluation_batches):
        rows = rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
        estimates.append(mi_sandwich_rows(m.lib, m.device, encoder(x[rows]), seed, b, feature).mean(dim=1).cpu().numpy())
    return np.mean(np.stack(estimates, 0), 0)


# Most batch rows (batches x evaluation_batch_size) of one dib_mi_sandwich_batched launch: 2^24 (its index upload is 64 MiB and
# its workspace 24 bytes per row); more batches than that - or than the kernel's 65 535 groups - are evaluated in several launches
_SANDWICH_ROWS_PER_LAUNCH = 1 << 24


def _sandwich_bounds_of_rows(table, rows, seed, step0=0):
    """dib_mi_sandwich_batched with one row per "neighbourhood" (P = 1, logvar offset 0) on a parameter table [N, 2E] (mu | logvar):
    batch b = the table rows rows[b] (repeats allowed), its noise keyed (seed, step0 + b, position in the batch, 0).
    Returns [batches, 2] (lower, upper) per batch in nats."""
    import ctypes

    import torch

    from ._host import stream_ptr
    from ._lib import check, load_library
    table = np.ascontiguousarray(table, dtype=np.float32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n, e = table.shape[0], table.shape[1] // 2
    nb, bs = rows.shape
    if rows.size == 0 or rows.min() < 0 or rows.max() >= n:
        raise ValueError("batch rows must index the parameter table")
    if not torch.cuda.is_available():
        raise RuntimeError("the sandwich bounds are evaluated on the GPU (there is no CPU fallback)")
    lib = load_library()
    per_launch = max(1, min(65535, _SANDWICH_ROWS_PER_LAUNCH // bs, nb))
    # (the last launch may hold fewer batches, and fewer batches can mean more row splits: size the workspace for both)
    needs = [int(lib.dib_mi_sandwich_batched_workspace_bytes(n, 1, e, g, bs)) for g in {per_launch, nb % per_launch or per_launch}]
    need = min(needs) if min(needs) < 0 else max(needs)
    if need < 0:
        raise ValueError(f"dib_mi_sandwich_batched: outside the envelope (E {e} must be a multiple of 4 up to 256, batch size {bs} >= 2)")
    dev = torch.device("cuda", torch.cuda.current_device())
    tab_d = torch.from_numpy(table).to(dev)
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=dev)
    out = torch.empty((2, nb), dtype=torch.float64, device=dev)
    stream = stream_ptr(dev)
    null = ctypes.c_void_p(0)
    for b0 in range(0, nb, per_launch):
        b1 = min(nb, b0 + per_launch)
        idx_d = torch.from_numpy(rows[b0:b1]).to(dev)
        check(lib.dib_mi_sandwich_batched(ctypes.c_void_p(tab_d.data_ptr()), n, 1, e, ctypes.c_void_p(idx_d.data_ptr()), b1 - b0, bs,
                                          0.0, int(seed) & (2 ** 64 - 1), (int(step0) + b0) & 0xFFFFFFFF,
                                          ctypes.c_void_p(out[0, b0:].data_ptr()), ctypes.c_void_p(out[1, b0:].data_ptr()), null, null,
                                          null, ctypes.c_void_p(ws.data_ptr()), stream), "dib_mi_sandwich_batched")
    return out.cpu().numpy().T.copy()


def estimate_mi_sandwich_bounds_from_parameters(mus, logvars, evaluation_batch_size=1024, number_evaluation_batches=8, seed=0):
    """The sandwich bounds of a channel given by its parameters, with no encoder and no dataset (the MI-bound characterization
    notebook's estimate_mi_sandwich_bounds(mus, logvars, ...)): p(u|x_j) = N(mus[j], diag exp(logvars[j])), [N, E] each.

    Returns [number_evaluation_batches, 2]: per batch the (InfoNCE lower, leave-one-out upper) bound in BITS, as the notebook's
    function does.  Batch b is rows np.random.default_rng(seed).integers(0, N, (number_evaluation_batches,
    evaluation_batch_size))[b] of the table - drawn with replacement, where the notebook calls np.random.choice - with the noise
    of dib_mi_sandwich_rows keyed (seed, step b, position, feature 0).  All batches go through ONE dib_mi_sandwich_batched launch
    (P = 1), in float64 with a log-sum-exp; the call is split only beyond 2^24 batch rows or 65 535 batches."""
    mus, logvars = np.asarray(mus, dtype=np.float32), np.asarray(logvars, dtype=np.float32)
    if mus.ndim != 2 or mus.shape != logvars.shape:
        raise ValueError(f"mus {mus.shape} and logvars {logvars.shape} must both be [N, E]")
    rows = np.random.default_rng(seed).integers(0, mus.shape[0], (int(number_evaluation_batches), int(evaluation_batch_size)))
    return _sandwich_bounds_of_rows(np.concatenate([mus, logvars], -1), rows, seed) / np.log(2.0)
