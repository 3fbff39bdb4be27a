"""NumPy restatement of include/dib_grad_transform.h - the checker of the gradient-transform tests (a helper, not a test).

TensorFlow is not installed: the semantics are pinned to the statement in that header and to this restatement, not to
an executed reference.  `transform(..., dtype)` are the three clips of Keras optimizer_v2 on a flat buffer with a variable table,
`lr(descriptor, step, dtype)` the legacy `decay` and the five schedules.  With float64 they are what the device is compared with;
with float32 the SAME code measures what the number format alone costs, and `bound()` - the project's tolerance rule
(tests/test_gpu_optimizers.py) - allows FACTOR = 4 times that, never less than one float32 ulp of the compared scale.  No bound is
taken from the device.

The two algebraic orders of clipnorm, (g * c) / max(n, c) as stated and g * (c / max(n, c)), differ by one or two float32
roundings: this tolerance does NOT tell them apart (tests/test_grad_transforms_host.py prints the distance)."""
import functools

import numpy as np

FACTOR = 4.0
ULP = 2.0 ** -23
TILE = 4096   # DIB_GRAD_TILE


def bound(want64, got32):
    """FACTOR x max |float32 restatement - float64 restatement|, at least one float32 ulp of the largest |float64 value|"""
    want64, got32 = np.asarray(want64, dtype=np.float64), np.asarray(got32, dtype=np.float64)
    fmt = float(np.abs(got32 - want64).max()) if want64.size else 0.0
    return max(FACTOR * fmt, ULP * (float(np.abs(want64).max()) if want64.size else 0.0))


# ---- the three clips -------------------------------------------------------------------------------------------------------
def transform(flat, segments, grad_scale=1.0, clipvalue=None, clipnorm=None, global_clipnorm=None, dtype=np.float64,
              extra_ss=0.0, ignore_grad_scale_in_norm=False, swapped_order=False):
    """(transformed copy of `flat` in `dtype`, ss per segment in `dtype`): g = flat * grad_scale on the segments [(offset, count)],
    clipvalue, then clipnorm per segment or global_clipnorm over all of them (+ extra_ss: another buffer's sum of squares).
    Elements outside every segment are copied.  The last two arguments build the WRONG variants the host test tells apart."""
    T = np.dtype(dtype).type
    out = np.asarray(flat).astype(dtype).copy()
    gs = T(np.float32(grad_scale))   # the C ABI passes a float
    ss = np.zeros(len(segments), dtype=dtype)
    for k, (o, n) in enumerate(segments):
        g = out[o:o + n] * gs
        if clipvalue is not None:
            c = T(np.float32(clipvalue))
            g = np.minimum(np.maximum(g, -c), c)
        out[o:o + n] = g
        ss[k] = np.sum(g * g, dtype=dtype)
    if clipnorm is not None:
        c = T(np.float32(clipnorm))
        for k, (o, n) in enumerate(segments):
            s = ss[k]
            if ignore_grad_scale_in_norm and gs != 0:
                s = s / (gs * gs)
            nrm = np.sqrt(s) if s > 0 else T(0)
            den = max(nrm, c)
            out[o:o + n] = out[o:o + n] * (c / den) if swapped_order else (out[o:o + n] * c) / den
    if global_clipnorm is not None:
        c = T(np.float32(global_clipnorm))
        with np.errstate(divide="ignore", invalid="ignore"):
            N = np.sqrt(np.sum(ss, dtype=dtype) + T(extra_ss))
            scale = c * min(T(1) / N, T(1) / c) + (N - N)   # (N - N): 0, or NaN for a non-finite norm (tf.clip_by_global_norm)
            for o, n in segments:
                out[o:o + n] = out[o:o + n] * scale
    return out, ss


def sumsq_of_float32_products(flat, segments, grad_scale=1.0, clipvalue=None):
    """what dib_grad_sumsq states: g = grads[i] * grad_scale (and the value clip) rounded to float32 as the rule will see it, the
    squares and their sum in float64.  The device is compared with THIS to 1e-12 relative - the float64 ss of transform() differs
    from it by the float32 rounding of g (6e-8 relative) whenever grad_scale is not a power of two."""
    out = np.zeros(len(segments), dtype=np.float64)
    for k, (o, n) in enumerate(segments):
        g = np.asarray(flat[o:o + n], dtype=np.float32) * np.float32(grad_scale)
        if clipvalue is not None:
            g = np.minimum(np.maximum(g, -np.float32(clipvalue)), np.float32(clipvalue))
        out[k] = np.sum(g.astype(np.float64) ** 2)
    return out


def global_scale(ss_total, c):
    """the factor global_clipnorm multiplies with, in float64 (what the fit test asserts is below 1 on half of the steps)"""
    N = np.sqrt(np.float64(ss_total))
    return float(c * min(1.0 / N, 1.0 / c)) if N > 0 else 1.0


# ---- learning rates --------------------------------------------------------------------------------------------------------
def lr(d, step, dtype=np.float64):
    """the learning rate at `step` (iterations, before the step's increment).  d: dict(kind=..., ...) with Keras' argument names:
    decay(lr, decay) | exponential / inverse_time(initial_learning_rate, decay_steps, decay_rate, staircase) |
    polynomial(initial_learning_rate, decay_steps, end_learning_rate, power, cycle) | piecewise(boundaries, values) |
    cosine(initial_learning_rate, decay_steps, alpha).  Every parameter is a float32 (the descriptor's fields)."""
    T = np.dtype(dtype).type
    f = lambda k, default=0.0: T(np.float32(d.get(k, default)))
    s, one = T(step), T(1)
    kind = d["kind"]
    if kind == "decay":
        return f("lr") / (one + f("decay") * s)
    init, ds = f("initial_learning_rate"), f("decay_steps")
    if kind in ("exponential", "inverse_time"):
        p = s / ds
        if d.get("staircase"):
            p = np.floor(p)
        return init * f("decay_rate") ** p if kind == "exponential" else init / (one + f("decay_rate") * p)
    if kind == "polynomial":
        end, power = f("end_learning_rate", 1e-4), f("power", 1.0)
        if d.get("cycle"):
            ds = ds * max(one, np.ceil(s / ds))
        else:
            s = min(s, ds)
        return (init - end) * (one - s / ds) ** power + end
    if kind == "piecewise":
        for b, v in zip(d["boundaries"], d["values"]):
            if step <= b:
                return T(np.float32(v))
        return T(np.float32(d["values"][-1]))
    if kind == "cosine":
        s = min(s, ds)
        a = f("alpha")
        return init * (((one - a) * T(0.5)) * (one + np.cos((T(np.float32(np.pi)) * s) / ds)) + a)
    raise ValueError(kind)


DECAY_STEPS = 10
LR_STEPS = (0, 1, DECAY_STEPS - 1, DECAY_STEPS, DECAY_STEPS + 1, 3 * DECAY_STEPS + 2)


def lr_cases():
    """{case id: restatement descriptor}: staircase edges, cycle wrap, piecewise boundaries from both sides (1 and 10 are
    boundaries, 0 / 9 / 11 their neighbours), cosine and the clamped polynomial beyond their end"""
    i, ds = 3e-3, DECAY_STEPS
    return {
        "decay": dict(kind="decay", lr=i, decay=0.05),
        "exponential": dict(kind="exponential", initial_learning_rate=i, decay_steps=ds, decay_rate=0.7),
        "exponential_staircase": dict(kind="exponential", initial_learning_rate=i, decay_steps=ds, decay_rate=0.7, staircase=True),
        "inverse_time": dict(kind="inverse_time", initial_learning_rate=i, decay_steps=ds, decay_rate=0.5),
        "inverse_time_staircase": dict(kind="inverse_time", initial_learning_rate=i, decay_steps=ds, decay_rate=0.5, staircase=True),
        "polynomial": dict(kind="polynomial", initial_learning_rate=i, decay_steps=ds, end_learning_rate=1e-4, power=2.0),
        "polynomial_cycle": dict(kind="polynomial", initial_learning_rate=i, decay_steps=ds, end_learning_rate=1e-4, power=0.5,
                                 cycle=True),
        "piecewise": dict(kind="piecewise", boundaries=[1, ds, 3 * ds], values=[i, 0.5 * i, 0.25 * i, 0.1 * i]),
        "cosine": dict(kind="cosine", initial_learning_rate=i, decay_steps=ds, alpha=0.1),
    }


def make_schedule(case):
    """the package's object of a case of lr_cases(): (an optimizers.Optimizer kwargs dict for `decay`, or a schedules object)"""
    from dib_amd import schedules as S
    d = dict(lr_cases()[case])
    kind = d.pop("kind")
    if kind == "decay":
        return d
    cls = {"exponential": S.ExponentialDecay, "inverse_time": S.InverseTimeDecay, "polynomial": S.PolynomialDecay,
           "piecewise": S.PiecewiseConstantDecay, "cosine": S.CosineDecay}[kind]
    return cls(**d)


def lr_reference(case, steps=LR_STEPS):
    """(float64 values, float32 values of the same restatement, bound) at `steps`"""
    d = lr_cases()[case]
    w = np.array([lr(d, s, np.float64) for s in steps], dtype=np.float64)
    g = np.array([lr(d, s, np.float32) for s in steps], dtype=np.float32)
    return w, g, bound(w, g)


# ---- the kernel-envelope inputs ----------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 63, 64, 65, 640, TILE - 1, TILE, TILE + 1, 16384, 70001)   # one short of a tile, a tile, a tile plus one
SCALES = (1.0, 0.0, 1e-4, 30.0, 1.0, 30.0, 1e-4, 0.0, 1.0, 30.0, 1e-4, 30.0, 1.0)   # per segment, from {0, 1e-4, 1, 30}
GAPS = (0, 1, 2, 2, 0, 3, 1, 2, 0, 3, 0, 2, 1)   # floats left out BEFORE each segment: the starts take every residue mod 4
CLIPVALUE, CLIPNORM, GLOBAL_CLIPNORM = 1.5, 2.0, 500.0


@functools.lru_cache(maxsize=2)
def envelope(seed=0):
    """(flat float32 buffer, segments [(offset, count)], gap mask): normal gradients times the segment's scale; the elements
    of no segment hold GAP_MARK, which no kernel may read or write"""
    rng = np.random.default_rng(seed)
    segments, o = [], 0
    for n, gap in zip(SIZES, GAPS):
        o += gap
        segments.append((o, n))
        o += n
    total = (o + 3) // 4 * 4
    flat = np.full(total, GAP_MARK, dtype=np.float32)
    gap_mask = np.ones(total, dtype=bool)
    for (o, n), sc in zip(segments, SCALES):
        flat[o:o + n] = (rng.standard_normal(n) * sc).astype(np.float32) if sc else 0.0   # (+0: bit-zero in, bit-zero out)
        gap_mask[o:o + n] = False
    flat.setflags(write=False)
    gap_mask.setflags(write=False)
    return flat, tuple(segments), gap_mask


GAP_MARK = np.float32(-7777.25)

MODES = {
    "clipvalue": dict(clipvalue=CLIPVALUE),
    "clipnorm": dict(clipnorm=CLIPNORM),
    "global_clipnorm": dict(global_clipnorm=GLOBAL_CLIPNORM),
    "clipvalue_clipnorm": dict(clipvalue=CLIPVALUE, clipnorm=CLIPNORM),
}


@functools.lru_cache(maxsize=None)
def envelope_reference(mode, grad_scale):
    """(float64 transformed buffer, float64 ss, bound on the transformed gradients) of MODES[mode] on envelope(): computed once"""
    flat, segments, _ = envelope()
    kw = MODES[mode]
    w, ss = transform(flat, segments, grad_scale, dtype=np.float64, **kw)
    g, _ = transform(flat, segments, grad_scale, dtype=np.float32, **kw)
    live = ~envelope()[2]
    w.setflags(write=False)
    ss.setflags(write=False)
    return w, ss, bound(w[live], g[live])


# ---- an update rule behind the transform (tests of whole steps) -------------------------------------------------------------
def stepped(rule, lr_of_step, steps, w0, grads, segments, dtype, **clip):
    """(w, slots) after `steps` steps of tests/_oracle_optimizers.py `rule` on transform(grads[k]) at lr_of_step(k)"""
    w = np.asarray(w0).astype(dtype).copy()
    st = rule.init(w.size, dtype)
    for k in range(steps):
        g, _ = transform(grads[k], segments, dtype=dtype, **clip)
        rule.step(w, g, st, lr_of_step(k, dtype))
    return w, st["slots"]
