"""Float64 restatement of the Keras loss and metric family (helper, not a test).

TensorFlow is not available to the tests: the contract is the list of per-row formulas in include/dib_losses.h (the table of
the pull request that added the family; SURVEY App. B for bce / bce_logits / mse), restated here as torch functions of
(y, p, param) -> one value per row, eps = 1e-7, e = p - y, C = out_dim:
    mae        mean_k |e_k|                                         mape   100 mean_k |e_k| / max(|y_k|, eps)
    msle       mean_k (log(max(p_k, eps) + 1) - log(max(y_k, eps) + 1))^2
    huber      mean_k (|e_k| <= delta ? e_k^2 / 2 : delta |e_k| - delta^2 / 2)
    log_cosh   mean_k (e_k + softplus(-2 e_k) - log 2)               poisson  mean_k (p_k - y_k log(p_k + eps))
    kl_divergence      sum_k y'_k log(y'_k / p'_k), y', p' clipped to [eps, 1]
    cosine_similarity  -sum_k yhat_k phat_k, xhat = x rsqrt(max(sum x^2, 1e-12))
    cce_logits  y <- y(1 - s) + s / C;  lse(z) sum_k y_k - sum_k y_k z_k
    cce         y <- y(1 - s) + s / C;  q = p / sum p;  c = clip(q, eps, 1 - eps);  -sum_k y_k log c_k
    sparse_cce  c = clip(p, eps, 1 - eps);  log sum_k c_k - log c_label
    bce_logits / bce  y <- y(1 - s) + s / 2, then SURVEY App. B's expressions;  mse  mean_k e_k^2
The loss is the batch mean of the row values and its gradient is torch.autograd of that mean - never a hand-derived expression,
so it is independent of the kernel's.  torch.clamp passes the gradient on the closed clip range and none outside it, which is
the contract's "no gradient where clipped".  The same functions run in float32 (dtype=torch.float32, CPU: IEEE float32 like
NumPy's) measure what the number format costs: the GPU tests allow 4 x that.  Metrics are NumPy.

loss_and_grad / accuracy have the signatures of oracle/dib_oracle.py's; a test swaps them in (monkeypatch) so that oracle.fit and
oracle.backward run a Case as their `loss_kind`."""
from collections import namedtuple

import numpy as np
import torch

EPS = 1e-7
Case = namedtuple("Case", "kind param metric", defaults=(0.0, None))

ELEMENTWISE = ("bce_logits", "bce", "mse", "mae", "mape", "msle", "huber", "log_cosh", "poisson", "kl_divergence")
CLASS_AXIS = ("cosine_similarity", "cce_logits", "cce", "sparse_cce")
KINDS = ELEMENTWISE + CLASS_AXIS
PARAM = {"huber": 1.0, "bce_logits": 0.1, "bce": 0.1, "cce_logits": 0.1, "cce": 0.1}   # the envelope's delta / label smoothing
PROBABILITY_KINDS = ("bce", "kl_divergence", "cce", "sparse_cce")     # p in (0, 1)
POSITIVE_KINDS = ("msle", "poisson")                                  # p > 0


def rows(kind, y, p, param=0.0):
    """per-row loss values [B] of torch tensors y, p [B, C] (sparse_cce: y [B, 1] of class indices)"""
    C = p.shape[1]
    e = p - y if kind != "sparse_cce" else None
    if kind == "mse":
        return (e * e).mean(1)
    if kind == "mae":
        return e.abs().mean(1)
    if kind == "mape":
        return 100.0 * (e.abs() / y.abs().clamp(min=EPS)).mean(1)
    if kind == "msle":
        a = torch.log(p.clamp(min=EPS) + 1.0) - torch.log(y.clamp(min=EPS) + 1.0)
        return (a * a).mean(1)
    if kind == "huber":
        ae = e.abs()
        return torch.where(ae <= param, 0.5 * e * e, param * ae - 0.5 * param * param).mean(1)
    if kind == "log_cosh":
        x = -2.0 * e
        softplus = x.clamp(min=0.0) + torch.log1p(torch.exp(-x.abs()))   # the overflow-free form: finite for |e| = 1e4
        return (e + softplus - float(np.log(2.0))).mean(1)
    if kind == "poisson":
        return (p - y * torch.log(p + EPS)).mean(1)
    if kind == "kl_divergence":
        yc, pc = y.clamp(EPS, 1.0), p.clamp(EPS, 1.0)
        return (yc * torch.log(yc / pc)).sum(1)
    if kind == "cosine_similarity":
        yh = y * torch.rsqrt((y * y).sum(1, keepdim=True).clamp(min=1e-12))
        ph = p * torch.rsqrt((p * p).sum(1, keepdim=True).clamp(min=1e-12))
        return -(yh * ph).sum(1)
    if kind == "cce_logits":
        ys = y * (1.0 - param) + param / C
        return torch.logsumexp(p, 1) * ys.sum(1) - (ys * p).sum(1)
    if kind == "cce":
        ys = y * (1.0 - param) + param / C
        c = (p / p.sum(1, keepdim=True)).clamp(EPS, 1.0 - EPS)
        return -(ys * torch.log(c)).sum(1)
    if kind == "sparse_cce":
        c = p.clamp(EPS, 1.0 - EPS)
        lab = y[:, :1].long()
        return torch.log(c.sum(1)) - torch.log(c.gather(1, lab))[:, 0]
    if kind == "bce_logits":
        ys = y * (1.0 - param) + 0.5 * param
        return (p.clamp(min=0.0) - p * ys + torch.log1p(torch.exp(-p.abs()))).mean(1)
    if kind == "bce":
        ys = y * (1.0 - param) + 0.5 * param
        c = p.clamp(EPS, 1.0 - EPS)
        return -(ys * torch.log(c) + (1.0 - ys) * torch.log(1.0 - c)).mean(1)
    raise ValueError(kind)


def rows_and_grad(kind, y, p, param=0.0, dtype=torch.float64):
    """(row values [B], d(sum of the row values)/dp [B, C]) evaluated in `dtype`, as float64 NumPy arrays"""
    yt = torch.tensor(np.asarray(y), dtype=dtype)
    pt = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    v = rows(kind, yt, pt, param)
    v.sum().backward()
    return v.detach().numpy().astype(np.float64), pt.grad.numpy().astype(np.float64)


def metric_rows(metric, y, p, dtype=np.float64):
    """per-row metric values [B] (NumPy, evaluated in `dtype`); arg-max takes the first of equal maxima"""
    y, p = np.asarray(y, dtype), np.asarray(p, dtype)
    if metric is None:
        return np.zeros(p.shape[0], dtype)
    if metric == "binary_accuracy":
        return ((p > 0.5).astype(dtype) == y).astype(dtype).mean(1, dtype=dtype)
    if metric == "categorical_accuracy":
        return (p.argmax(1) == y.argmax(1)).astype(dtype)
    if metric == "sparse_categorical_accuracy":
        return (p.argmax(1) == y[:, 0].astype(np.int64)).astype(dtype)
    if metric == "mae":
        return np.abs(p - y).mean(1, dtype=dtype)
    if metric == "mse":
        return ((p - y) ** 2).mean(1, dtype=dtype)
    raise ValueError(metric)


def act_grad_from_output(act, out, dtype=np.float64):
    """csrc/dib_common.h dib_act_grad: the output activation's derivative through its output (ids of include/dib_hip.h),
    evaluated in `dtype`"""
    out = np.asarray(out, dtype)
    one = dtype(1)
    res = {0: lambda o: np.ones_like(o), 1: lambda o: (o > 0).astype(dtype), 2: lambda o: np.where(o > 0, one, dtype(0.2)),
           3: lambda o: one - o * o, 4: lambda o: o * (one - o), 5: lambda o: np.where(o > 0, one, o + one),
           6: lambda o: one - np.exp(-o), 7: lambda o: np.where(o > 0, one, dtype(0.1))}[act](out)
    return res.astype(dtype)


# ---- the pair oracle/dib_oracle.py's backward / fit look up as module globals -------------------------------------------------
def _labels(case, y, pred):
    y = np.asarray(y, np.float64)
    return y.reshape(pred.shape[0], -1)


def loss_and_grad(case, y, pred):
    """(mean loss, dL/dpred) of a Case, signature of oracle.loss_and_grad"""
    v, g = rows_and_grad(case.kind, _labels(case, y, pred), pred, case.param)
    return float(v.mean()), g / pred.shape[0]


def accuracy(case, y, pred):
    """batch mean of the Case's metric, signature of oracle.accuracy"""
    return float(metric_rows(case.metric, _labels(case, y, pred), pred).mean())


# ---- inputs of the envelope --------------------------------------------------------------------------------------------------
def draw(kind, B, C, ldy, nrows, seed, metric=None):
    """(pred [B, C] float32, label table [nrows, ldy] float32) in the kind's domain.  Where a counted metric is asked for, the
    predictions keep an arg-max margin and a distance from the 0.5 threshold of at least 1e-3 (asserted by the caller)."""
    rng = np.random.default_rng([seed, B, C, KINDS.index(kind)])
    cols = 1 if kind == "sparse_cce" else C
    assert ldy >= cols
    Y = rng.standard_normal((nrows, ldy)).astype(np.float32)   # the padding columns hold noise the kernel must not read
    if kind in PROBABILITY_KINDS or kind == "cce_logits":
        p = rng.dirichlet(np.ones(C) * 0.7, B) if C > 1 else rng.uniform(0.02, 0.98, (B, 1))
        p = np.clip(p, 1e-4, 1.0 - 1e-4) if kind != "cce" else np.clip(p, 1e-4, None) * rng.uniform(0.5, 3.0, (B, 1))  # cce: unnormalised
        if kind == "cce_logits":
            p = rng.standard_normal((B, C)) * 3.0
    elif kind in POSITIVE_KINDS:
        p = rng.uniform(0.05, 4.0, (B, C))
    else:
        p = rng.standard_normal((B, C)) * 1.5
    if kind == "sparse_cce":
        Y[:, 0] = rng.integers(0, C, nrows)
    elif kind in ("cce_logits", "cce"):
        soft = rng.dirichlet(np.ones(C), nrows) if C > 1 else np.ones((nrows, 1))
        onehot = np.eye(C)[rng.integers(0, C, nrows)]
        Y[:, :C] = np.where(rng.random((nrows, 1)) < 0.5, onehot, soft)
    elif kind in ("bce_logits", "bce"):
        Y[:, :C] = rng.integers(0, 2, (nrows, C))
    elif kind == "kl_divergence":
        Y[:, :C] = rng.dirichlet(np.ones(C), nrows) if C > 1 else rng.uniform(0.02, 0.98, (nrows, 1))
    elif kind in POSITIVE_KINDS:
        Y[:, :C] = rng.uniform(0.0, 4.0, (nrows, C))
    p = p.astype(np.float32)
    if metric == "binary_accuracy":
        near = np.abs(p - 0.5) < 2e-3
        p[near] = 0.5 + 4e-3
    if metric in ("categorical_accuracy", "sparse_categorical_accuracy") and C > 1:
        top = p.argmax(1)
        p[np.arange(B), top] += np.float32(4e-3) * np.maximum(np.abs(p[np.arange(B), top]), 1).astype(np.float32)
    return p, Y


def margins_ok(metric, p, Y, rows_of_batch, C):
    """the property that makes a counted metric's float64 count unambiguous"""
    p = np.asarray(p, np.float64)
    if metric == "binary_accuracy":
        return bool((np.abs(p - 0.5) >= 1e-3).all())
    if metric in ("categorical_accuracy", "sparse_categorical_accuracy") and C > 1:
        s = np.sort(p, 1)
        ok = bool((s[:, -1] - s[:, -2] >= 1e-3).all())
        if metric == "categorical_accuracy":
            y = np.asarray(Y, np.float64)[rows_of_batch][:, :C]
            sy = np.sort(y, 1)
            ok = ok and bool(((sy[:, -1] - sy[:, -2]) > 0).all())
        return ok
    return True
