"""float64 restatement of the token chain of include/dib_st.h (dib_st_chain_fwd / dib_st_chain_bwd), for the envelope tests.

    fwd: mha = ctx @ o_w + o_b; h = LN1(x_in + mha) (+ xhat1, rstd1); f_l = act(f_{l-1} ff_w[l] + ff_b[l]); x_out = LN2(h + f_last)
    bwd: from g_out = dL/dx_out: g_ff[l] = dL/d(pre-activation of layer l), g_in = dL/d(x_in + mha), g_ctx = g_in @ o_w^T and the
         four LayerNorm parameter gradients (gamma, beta of LN1 and LN2).

LayerNorm is Keras's: two-pass variance over the last axis, rstd = 1 / sqrt(var + eps).  The activation's derivative at the
kink is taken from `masks` when given (the device's own choices, `post-activation > 0`, as oracle/set_transformer_oracle.py does
for the model): float64 and float32 may put a pre-activation within round-off of 0 on different sides, and each such unit moves
one token's share of a gradient.  `boundary` (optional dict) receives, per layer, how many units the masks put on the other side
of float64's own `z > 0` and the largest |z| among them, so that the caller can bound both.
"""
import numpy as np

SLOPE = {0: 1.0, 1: 0.0, 2: 0.2}   # DIB_ACT_LINEAR, DIB_ACT_RELU, DIB_ACT_LEAKY_RELU (dib_neg_slope)


def _ln_fwd(s, g, b, eps):
    mean = s.mean(-1, keepdims=True)
    var = ((s - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (s - mean) * rstd
    return xhat * g + b, xhat, rstd[:, 0]


def _ln_bwd(dy, xhat, rstd, g):
    dxh = dy * g
    m1 = dxh.mean(-1, keepdims=True)
    m2 = (dxh * xhat).mean(-1, keepdims=True)
    return rstd[:, None] * (dxh - m1 - xhat * m2), (dy * xhat).sum(0), dy.sum(0)


def chain_forward(p, ctx, x_in, eps, act, masks=None, boundary=None):
    """p: dict of float64 arrays o_w [HK, D], o_b, ln1_g, ln1_b, ln2_g, ln2_b, ff_w (list), ff_b (list).
    Returns a dict: h, xhat1, rstd1, ff (list of post-activations), x_out, xhat2, rstd2, act_masks (list)."""
    slope = SLOPE[act]
    mha = ctx @ p["o_w"] + p["o_b"]
    h, xhat1, rstd1 = _ln_fwd(x_in + mha, p["ln1_g"], p["ln1_b"], eps)
    f, ff, am = h, [], []
    for l, (w, b) in enumerate(zip(p["ff_w"], p["ff_b"])):
        z = f @ w + b
        pos = z > 0
        if masks is not None:
            m = np.asarray(masks[l], dtype=bool)
            if boundary is not None:
                diff = m != pos
                boundary[l] = (int(diff.sum()), float(np.abs(z[diff]).max()) if diff.any() else 0.0)
            pos = m
        f = np.where(pos, z, slope * z)
        ff.append(f)
        am.append(pos)
    x_out, xhat2, rstd2 = _ln_fwd(h + f, p["ln2_g"], p["ln2_b"], eps)
    return dict(h=h, xhat1=xhat1, rstd1=rstd1, ff=ff, x_out=x_out, xhat2=xhat2, rstd2=rstd2, act_masks=am)


def chain_backward(p, fwd, g_out, act):
    """Gradients of sum(g_out * x_out) through chain_forward's result `fwd` (its act' masks)."""
    slope = SLOPE[act]
    n = len(p["ff_w"])
    d = lambda l: np.where(fwd["act_masks"][l], 1.0, slope)
    g_a, dg2, db2 = _ln_bwd(g_out, fwd["xhat2"], fwd["rstd2"], p["ln2_g"])
    g_ff = [None] * n
    g_ff[n - 1] = g_a * d(n - 1)
    for l in range(n - 1, 0, -1):
        g_ff[l - 1] = (g_ff[l] @ p["ff_w"][l].T) * d(l - 1)
    gh = g_ff[0] @ p["ff_w"][0].T + g_a
    g_in, dg1, db1 = _ln_bwd(gh, fwd["xhat1"], fwd["rstd1"], p["ln1_g"])
    return dict(g_ff=g_ff, g_in=g_in, g_ctx=g_in @ p["o_w"].T, ln1_g=dg1, ln1_b=db1, ln2_g=dg2, ln2_b=db2)
