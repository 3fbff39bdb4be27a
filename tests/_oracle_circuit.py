"""Float64 restatement of the Boolean-circuit notebook's training step (reference complex_systems/InfoDecomp_Boolean_circuits.ipynb
cells 4 and 6: SimpleEncoder, train_step, the Keras Adam step) and of its post-processing (cell 6's smoothed curves, cell 7's
selected subsets), driven by the same Philox draws as the device.  The checker only: it shares no code with the package."""
import numpy as np

import dib_oracle as orc

SLOPE = 0.2   # tf.nn.leaky_relu's default: the notebook's 'leaky_relu'


def draw_rows(seed, step, B, G):
    """r_b = x0 >> (32 - G), x0 = the first Philox4x32-10 output for counter (b, 0xFFFFFFFF, 0, step), key seed"""
    x0 = orc.philox4x32_10(np.arange(B, dtype=np.uint32), np.uint32(0xFFFFFFFF), np.uint32(0), np.uint32(step & 0xFFFFFFFF),
                           seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (x0 >> np.uint32(32 - G)).astype(np.int64)


def eps(seed, step, B, G):
    """[B, G]: the library's normal keyed (seed, step, row b, feature g, dim 0)"""
    return np.stack([orc.philox_normal(seed, step, np.arange(B), g, 1)[:, 0] for g in range(G)], -1)


def beta_schedule(step, n, beta_start, beta_end):
    """cell 6: beta_var.assign(np.exp(np.log(b0) + float(step) / n * (np.log(b1) - np.log(b0)))) into a float32 variable"""
    return float(np.float32(np.exp(np.log(beta_start) + float(step) / n * (np.log(beta_end) - np.log(beta_start)))))


class Params:
    """predictor [W0 [G, H], b0, ..., W_out [H, 1], b_out] (Keras order) and the scalars s [G], lv [G]; float64"""

    def __init__(self, weights, s, lv):
        self.weights = [np.array(w, dtype=np.float64) for w in weights]
        self.s, self.lv = np.array(s, dtype=np.float64).reshape(-1), np.array(lv, dtype=np.float64).reshape(-1)

    def tensors(self):
        return self.weights + [self.s, self.lv]

    def zeros_like(self):
        return Params([np.zeros_like(w) for w in self.weights], np.zeros_like(self.s), np.zeros_like(self.lv))


def _leaky(v):
    return np.where(v > 0, v, SLOPE * v)


def step(p: Params, table, rows, e, beta):
    """one train_step on the truth table's rows `rows` with noise e [B, G]: BCE (from logits, batch mean), KL [G] and the
    gradients of BCE + beta sum_g KL_g -> dict(bce, kl, loss, x, u, y, logit, grads: Params, grad_magnitudes: the sums of the
    terms' absolute values behind each weight / bias gradient - the scale of its summation-order rounding - and grad_max_terms:
    a bound on the largest single batch term of each)"""
    table = np.asarray(table)
    G = p.s.shape[0]
    x = 2.0 * table[rows, :G].astype(np.float64) - 1.0
    y = table[rows, -1].astype(np.float64)
    B = x.shape[0]
    sd = np.exp(p.lv / 2.0)
    u = x * p.s + sd * e
    n = len(p.weights) // 2
    acts, pres = [u], []
    h = u
    for l in range(n):
        z = h @ p.weights[2 * l] + p.weights[2 * l + 1]
        pres.append(z)
        h = _leaky(z) if l < n - 1 else z
        acts.append(h)
    logit = h[:, 0]
    bce = float(np.mean(np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))))
    kl = 0.5 * (p.s ** 2 + np.exp(p.lv) - p.lv - 1.0)
    # backward
    g = ((1.0 / (1.0 + np.exp(-logit)) - y) / B)[:, None]
    gw, mag, top = [None] * (2 * n), [None] * (2 * n), [None] * (2 * n)
    for l in range(n - 1, -1, -1):
        gw[2 * l] = acts[l].T @ g
        gw[2 * l + 1] = g.sum(0)
        mag[2 * l], mag[2 * l + 1] = np.abs(acts[l]).T @ np.abs(g), np.abs(g).sum(0)
        top[2 * l], top[2 * l + 1] = np.outer(np.abs(acts[l]).max(0), np.abs(g).max(0)), np.abs(g).max(0)
        g = g @ p.weights[2 * l].T
        if l > 0:
            g = g * np.where(pres[l - 1] > 0, 1.0, SLOPE)
    gu = g
    ds = np.sum(gu * x, 0) + beta * p.s
    dlv = np.sum(gu * e, 0) * 0.5 * sd + beta * 0.5 * (np.exp(p.lv) - 1.0)
    return {"bce": bce, "kl": kl, "loss": bce + beta * float(kl.sum()), "x": x, "u": u, "y": y, "logit": logit, "g_u": gu,
            "grads": Params(gw, ds, dlv), "grad_magnitudes": mag,
            "grad_max_terms": top}


def adam(p: Params, grads: Params, st, lr=1e-3):
    orc.adam_keras_step(p, grads, st, lr=lr)


def adam_init(p: Params):
    return orc.AdamState(p.zeros_like(), p.zeros_like(), 0)


def mi_bounds_batch(s, lv, x, eps_g):
    """the notebook's compute_batch (float64, exp then log) on one gate's encoder output for points x, sampled with the
    normals eps_g [n] (u = mu + exp(lv / 2) eps)"""
    mus = (np.asarray(x, np.float64) * np.float64(np.float32(s)))[:, None]
    lvs = np.full_like(mus, np.float64(np.float32(lv)))
    u = mus + np.exp(lvs / 2.0) * np.asarray(eps_g, np.float64)[:, None]
    return orc.mi_sandwich_bounds_batch(mus, lvs, u)


# ---- cells 6-7 post-processing, restated -----------------------------------------------------------------------------------
def information_plane(bounds_bits, bce_series, entropy_y, freq):
    from scipy import ndimage
    t = np.mean(np.asarray(bounds_bits), axis=-1)
    out = entropy_y - np.float32(bce_series) / np.log(2)
    return (ndimage.gaussian_filter1d(t, 1.5, axis=0), ndimage.gaussian_filter1d(t.sum(-1), 0.5),
            ndimage.gaussian_filter(out, 25)[::freq])


def selected_subsets(info_in_parts, threshold=0.1):
    above = np.cumprod(np.asarray(info_in_parts) > threshold, axis=0)
    active = above.sum(-1)
    out = [np.where(above[i + 1])[0] for i in np.where(np.diff(active) < 0)[0]]
    return out + [range(above.shape[-1])]
