"""NumPy oracle of dL/dx for DistributedIBNet (checker of dib_encoder_bank_input_grad; calls nothing of the library).

L = loss(y, pred) + beta * sum_f KL_f, the loss whose parameter gradients dib_oracle.backward returns.  The forward and its cache
are dib_oracle.forward's; the gradient chain below restates dib_oracle.backward down to the pre-activation of encoder layer 0
(without the parameter gradients), then takes it through W1^T and the positional encoding (reference models.py:22-23,
P_f = [x_f, sin(2 x_f), ..., sin(2^(n-1) x_f)] blockwise):

    dP_f = G_f W1_f^T ;  dx[b, c0_f + q] = dP_f[b, q] + sum_{j >= 1} 2^j cos(2^j x[b, c0_f + q]) dP_f[b, j d_f + q]

Everything runs in the dtype of its arguments: float64 for the reference, float32 (arguments cast by `as_dtype`) for the CPU
restatement that measures what float32 arithmetic alone costs."""
import numpy as np

import dib_oracle as orc


def as_dtype(params: orc.DIBParams, dtype) -> orc.DIBParams:
    return orc.DIBParams([[w.astype(dtype) for w in ws] for ws in params.enc_W], [[b.astype(dtype) for b in bs] for bs in params.enc_b],
                         [w.astype(dtype) for w in params.int_W], [b.astype(dtype) for b in params.int_b])


def loss_value(spec, params, x, y, eps, beta, loss_kind):
    """L (a float) - what central differences of the oracle's own loss are taken of"""
    c = orc.forward(spec, params, x, eps)
    task, _ = orc.loss_and_grad(loss_kind, y, c.pred)
    return task + beta * float(c.kl.sum())


def input_grad(spec, params, x, y, cache, beta, loss_kind, g_pred=None):
    """dL/dx [B, sum_d].  g_pred: the caller's dL/dpred [B, out] instead of the loss `loss_kind` of (y, pred)."""
    F, E = spec.number_features, spec.feature_embedding_dimension
    B = x.shape[0]
    dt = x.dtype
    g = orc.loss_and_grad(loss_kind, y, cache.pred)[1] if g_pred is None else np.asarray(g_pred, dtype=dt)
    g = g.astype(dt)
    if spec.output_activation_fn not in (None, "linear"):
        g = g * orc._act_grad_from_output(spec.output_activation_fn, cache.int_hidden[-1])
    for l in reversed(range(len(params.int_W))):
        g = g @ params.int_W[l].T
        if l > 0:
            g = g * orc._act_grad_from_output(spec.activation_fn, cache.int_hidden[l])
    gu = g.reshape(B, F, E)
    mu, lv, eps = cache.mu, cache.logvar, cache.eps
    dmu = gu + dt.type(beta) * mu / B
    dlv = gu * eps * dt.type(0.5) * np.exp(lv / dt.type(2.0)) + dt.type(beta) * dt.type(0.5) * (np.exp(lv) - dt.type(1.0)) / B
    xs = orc.split_features(x, spec.feature_dimensionalities)
    n_blocks = len(spec.frequencies) + 1 if spec.use_positional_encoding else 1
    out = []
    for f in range(F):
        gf = np.concatenate([dmu[:, f], dlv[:, f]], axis=-1)      # [B, 2E]: gradient of (mu | logvar)
        hid = cache.enc_hidden[f]
        for l in reversed(range(1, len(params.enc_W[f]))):
            gf = (gf @ params.enc_W[f][l].T) * orc._act_grad_from_output(spec.activation_fn, hid[l])
        dP = gf @ params.enc_W[f][0].T                             # [B, n_blocks d_f]
        d = spec.feature_dimensionalities[f]
        dx = dP[:, :d].copy()
        for j in range(1, n_blocks):
            fr = dt.type(spec.frequencies[j - 1])
            dx += fr * np.cos(fr * xs[f]) * dP[:, j * d: (j + 1) * d]
        out.append(dx)
    return np.concatenate(out, axis=-1)


def knife_edge_rows(spec, params, x, cache, thresh=1e-5):
    """bool [B]: rows where a hidden pre-activation of a relu / leaky_relu network lies within `thresh` of 0 (float64 oracle):
    one flipped act' there moves the row's gradient by O(1) of its scale, in any float32 evaluation."""
    B = x.shape[0]
    edge = np.zeros(B, dtype=bool)
    if spec.activation_fn not in ("relu", "leaky_relu"):
        return edge
    for f in range(spec.number_features):
        hid = cache.enc_hidden[f]
        for l in range(len(params.enc_W[f]) - 1):
            z = hid[l] @ params.enc_W[f][l] + params.enc_b[f][l]
            edge |= (np.abs(z) < thresh).any(axis=1)
    for l in range(len(params.int_W) - 1):
        z = cache.int_hidden[l] @ params.int_W[l] + params.int_b[l]
        edge |= (np.abs(z) < thresh).any(axis=1)
    return edge


def block_errors(spec, dx, dx64, keep=None):
    """per feature block: max|dx - dx64| / max|dx64| over the rows `keep` (default: all)"""
    out, c0 = [], 0
    rows = slice(None) if keep is None else keep
    for d in spec.feature_dimensionalities:
        ref = dx64[rows, c0: c0 + d]
        out.append(float(np.abs(np.asarray(dx, dtype=np.float64)[rows, c0: c0 + d] - ref).max() / np.abs(ref).max()))
        c0 += d
    return out


# ---- the cases of tests/test_gpu_input_grad.py (built without the library, so that the float32 restatement can run anywhere) ----
BETA, SEED, STEP = 0.37, 11, 5


def loss_kind_of(name, spec):
    """each zoo entry's natural loss (as tests/test_gpu_parity.py)"""
    if spec.output_dimensionality == 1:
        return "bce" if spec.output_activation_fn == "sigmoid" else "bce_logits"
    return "mse" if name == "pendulum_ragged" else "sparse_cce_logits"


def make_case(name, spec, B, param_seed=None):
    """(float32 parameters, x [B, sum_d] float32, y, loss kind): N(0,1) inputs, glorot kernels, N(0, 0.1^2) biases"""
    import zlib
    from _helpers import random_params
    seed = zlib.crc32(name.encode()) % 1000 if param_seed is None else param_seed
    p32 = as_dtype(random_params(spec, seed), np.float32)
    rng = np.random.default_rng(B + seed)
    x = rng.standard_normal((B, sum(spec.feature_dimensionalities))).astype(np.float32)
    kind = loss_kind_of(name, spec)
    if kind in ("bce", "bce_logits"):
        y = rng.integers(0, 2, (B, 1)).astype(np.float32)
    elif kind == "mse":
        y = rng.standard_normal((B, spec.output_dimensionality)).astype(np.float32)
    else:
        y = rng.integers(0, spec.output_dimensionality, (B, 1)).astype(np.float32)
    return p32, x, y, kind


def reference(spec, p32, x, y, kind, eps32, beta=BETA, g_pred=None):
    """(dx float64 [B, sum_d], knife-edge rows bool [B]) from float32-valued parameters, inputs and noise"""
    p = as_dtype(p32, np.float64)
    x64 = np.asarray(x, dtype=np.float64)
    c = orc.forward(spec, p, x64, np.asarray(eps32, dtype=np.float64))
    return input_grad(spec, p, x64, y, c, beta, kind, g_pred=g_pred), knife_edge_rows(spec, p, x64, c)


def restatement_float32(spec, p32, x, y, kind, eps32, beta=BETA):
    """the same code in float32 arithmetic"""
    x32 = np.asarray(x, dtype=np.float32)
    c = orc.forward(spec, p32, x32, np.asarray(eps32, dtype=np.float32))
    return input_grad(spec, p32, x32, np.asarray(y, dtype=np.float32), c, np.float32(beta), kind)
