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
        return _measurement_mi_bounds(encoder, x, n, bs, rng, int(number_evaluation_batches), seed)
    if getattr(encoder, "_circuit", None) is not None:   # CircuitIB.feature_encoders[g] (Boolean-circuit notebook cell 4)
        return _circuit_mi_bounds(encoder, x, n, bs, rng, int(number_evaluation_batches), seed)
    model = encoder._model
    eng = model._ensure_engine()
    estimates = []
    for b in range(int(number_evaluation_batches)):
        rows = rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
        enc_out = eng.encode_feature(encoder.index, x[rows])
        estimates.append(eng.mi_sandwich_bounds(enc_out, seed, b, encoder.index))
    return np.mean(np.stack(estimates, 0), 0)


def _measurement_mi_bounds(encoder, x, n, bs, rng, number_evaluation_batches, seed):
    import ctypes

    import torch

    from ._gemm_plan import _ptr
    from ._lib import check
    m = encoder._measurement
    estimates = []
    for b in range(number_evaluation_batches):
        rows = rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
        enc_out = encoder(x[rows])
        e = enc_out.shape[1] // 2
        ws = torch.empty(int(m.lib.dib_mi_workspace_bytes(bs, e)) // 8 + 1, dtype=torch.float64, device=m.device)
        r = torch.empty((2, bs), dtype=torch.float64, device=m.device)
        check(m.lib.dib_mi_sandwich_rows(_ptr(enc_out), bs, e, int(seed), b & 0xFFFFFFFF, 0, _ptr(r[0]), _ptr(r[1]), _ptr(ws),
                                         ctypes.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)), "dib_mi_sandwich_rows")
        estimates.append(r.mean(dim=1).cpu().numpy())
    return np.mean(np.stack(estimates, 0), 0)


def _circuit_mi_bounds(encoder, x, n, bs, rng, number_evaluation_batches, seed):
    """one gate's channel, batch by batch through dib_mi_sandwich_rows on its [bs, 2] output (noise feature = the gate index):
    the per-gate form of CircuitIB.estimate_channel_mi_bounds' one-launch evaluation"""
    import ctypes

    import torch

    from ._gemm_plan import _ptr
    from ._lib import check
    m = encoder._circuit
    ws = torch.empty(int(m.lib.dib_mi_workspace_bytes(bs, 1)) // 8 + 1, dtype=torch.float64, device=m.device)
    estimates = []
    for b in range(number_evaluation_batches):
        rows = rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
        enc_out = encoder(x[rows]).contiguous()
        r = torch.empty((2, bs), dtype=torch.float64, device=m.device)
        check(m.lib.dib_mi_sandwich_rows(_ptr(enc_out), bs, 1, int(seed) & (2 ** 64 - 1), b & 0xFFFFFFFF, encoder.index,
                                         _ptr(r[0]), _ptr(r[1]), _ptr(ws),
                                         ctypes.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)), "dib_mi_sandwich_rows")
        estimates.append(r.mean(dim=1).cpu().numpy())
    return np.mean(np.stack(estimates, 0), 0)
