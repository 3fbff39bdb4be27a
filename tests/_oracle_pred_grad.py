"""float64 backward of the DIB model from a GIVEN dL/dpred - the custom-loss contract of HipEngine.backward_from_pred_grad
(reference train.py:216-219: the InfoNCE loop's tape.gradient with the model's add_loss KL term).  oracle/dib_oracle.py backward
starts from a loss kind; this is the same chain from its second line on."""
import numpy as np

import dib_oracle as orc


def backward_from_pred_grad(spec: orc.DIBSpec, params: orc.DIBParams, cache: orc.ForwardCache, g_pred: np.ndarray, beta: float,
                            inv_global_batch: float):
    """g_pred [B, out] = dL/dpred (after the output activation).  The KL term enters as beta * inv_global_batch * dKL_sum.
    Returns (grads: DIBParams, g_u [B, F*E])."""
    F, E = spec.number_features, spec.feature_embedding_dimension
    B = cache.u.shape[0]
    g = np.asarray(g_pred, dtype=np.float64)
    grads = params.zeros_like()
    nl = len(params.int_W)
    if spec.output_activation_fn not in (None, "linear"):
        g = g * orc._act_grad_from_output(spec.output_activation_fn, cache.int_hidden[-1])
    for l in reversed(range(nl)):
        h_in = cache.int_hidden[l]
        grads.int_W[l] = h_in.T @ g
        grads.int_b[l] = g.sum(0)
        g = g @ params.int_W[l].T
        if l > 0:
            g = g * orc._act_grad_from_output(spec.activation_fn, h_in)
    g_u = g
    gu = g_u.reshape(B, F, E)
    mu, lv, eps = cache.mu, cache.logvar, cache.eps
    kb = beta * inv_global_batch
    dmu = gu + kb * mu
    dlv = gu * eps * 0.5 * np.exp(lv / 2.0) + kb * 0.5 * (np.exp(lv) - 1.0)
    for f in range(F):
        gf = np.concatenate([dmu[:, f], dlv[:, f]], axis=-1)
        hid = cache.enc_hidden[f]
        for l in reversed(range(len(params.enc_W[f]))):
            h_in = hid[l]
            grads.enc_W[f][l] = h_in.T @ gf
            grads.enc_b[f][l] = gf.sum(0)
            if l > 0:
                gf = (gf @ params.enc_W[f][l].T) * orc._act_grad_from_output(spec.activation_fn, h_in)
    return grads, g_u
