"""Float64 restatement of the chaos notebook's random partitions (Chaos_experiments.ipynb cell 7), the checker of
dib_partition_symbolize and RandomPartition: the MLP on the float32 cast of the input (Keras casts the float64 trajectory),
symbol = argmax |output| with the first maximum winning (tf.argmax / np.argmax), H(U) of utils.compute_entropy."""
import numpy as np

ACT = {"linear": lambda v: v, "relu": lambda v: np.maximum(v, 0.0), "leaky_relu": lambda v: np.where(v > 0, v, 0.2 * v),
       "tanh": np.tanh}


def forward(weights, x, activation):
    """float64 outputs [n, A] of the Keras-layout network [W0, b0, ..., W_out, b_out]; hidden layers `activation`, output linear"""
    h = np.asarray(x).astype(np.float32).astype(np.float64)
    if h.ndim == 1:
        h = h[:, None]
    L = len(weights) // 2
    for l in range(L):
        h = h @ np.asarray(weights[2 * l], np.float64) + np.asarray(weights[2 * l + 1], np.float64)
        if l < L - 1:
            h = ACT[activation](h)
    return h


def abs_forward(weights, x, activation):
    """the same chain on |W|, |b|, |input| with |act(v)| <= |v| propagated: per output, the sum of the magnitudes of the terms that
    fp32 arithmetic adds up - the scale of its rounding error"""
    h = np.abs(np.asarray(x).astype(np.float32).astype(np.float64))
    if h.ndim == 1:
        h = h[:, None]
    L = len(weights) // 2
    for l in range(L):
        h = h @ np.abs(np.asarray(weights[2 * l], np.float64)) + np.abs(np.asarray(weights[2 * l + 1], np.float64))
    return h


def symbols(logits):
    """argmax |logit| per row, the first index winning exact ties (uint8)"""
    return np.argmax(np.abs(np.asarray(logits)), axis=-1).astype(np.uint8)


def margin(logits):
    """largest minus second-largest |logit| per row"""
    a = np.sort(np.abs(np.asarray(logits, np.float64)), axis=-1)
    return a[:, -1] - a[:, -2]


def compute_entropy(seq):
    """H(U) in bits of a symbol sequence (the notebook's utils.compute_entropy)"""
    _, counts = np.unique(np.asarray(seq), return_counts=True)
    p = counts / counts.sum()
    return float(-np.sum(p * np.log2(p)))


def logistic_trajectory(n, r=3.7115, x0=0.3, skip=100_000):
    """x_{t+1} = r x_t (1 - x_t), the first `skip` iterates discarded: float64 [n, 1]"""
    out = np.empty(n + skip)
    x = float(x0)
    for i in range(n + skip):
        out[i] = x
        x = r * x * (1.0 - x)
    return out[skip:, None]


def generating_partition_weights(hidden=16, activation_is_linear=True):
    """hand-set linear network of the logistic map's generating partition: h0 = x - 0.5, o0 = 1 + h0, o1 = 1 - h0, so that
    symbol 0 <=> x > 0.5 (|o0| > |o1|); the other hidden units are zero"""
    W0 = np.zeros((1, hidden), np.float32); W0[0, 0] = 1.0
    b0 = np.zeros(hidden, np.float32); b0[0] = -0.5
    W1 = np.zeros((hidden, 2), np.float32); W1[0] = [1.0, -1.0]
    b1 = np.ones(2, np.float32)
    return [W0, b0, W1, b1]
