"""Learning-rate schedules with the class and argument names of tf.keras.optimizers.schedules (Keras optimizer_v2).  An object is
passed as an optimizer's `learning_rate`; the learning rate of a step is the schedule at `iterations`, the step count before that
step's increment.  On the GPU the schedule is evaluated by a one-thread kernel from the device step count
(include/dib_grad_transform.h dib_lr_schedule_eval), so a captured step replays with an advancing learning rate; `__call__` here is
the same float32 arithmetic on the host (tests compare it with a float64 restatement).  TensorFlow is not a dependency: the
formulas are pinned to DESIGN 10j, not to an executed reference."""
from __future__ import annotations

import numpy as np

# include/dib_grad_transform.h DIB_LR_*
LR_INVERSE_DECAY, LR_EXPONENTIAL, LR_INVERSE_TIME, LR_POLYNOMIAL, LR_PIECEWISE, LR_COSINE = range(1, 7)
LR_STAIRCASE, LR_CYCLE = 1, 2
MAX_BOUNDARIES = 8

_f = np.float32


class LearningRateSchedule:
    """base class: `descriptor()` are the fields of dib_lr_schedule, `__call__(step)` the float32 value at `step`"""

    def descriptor(self) -> dict:
        raise NotImplementedError

    def __call__(self, step) -> float:
        return float(evaluate(self.descriptor(), int(step)))

    def get_config(self) -> dict:
        return {k: v for k, v in vars(self).items() if not k.startswith("_")}

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


def _positive_steps(cls, decay_steps):
    if not float(decay_steps) > 0.0:
        raise ValueError(f"{cls}: decay_steps must be positive, got {decay_steps!r}")
    return float(decay_steps)


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ^ (step / decay_steps); staircase floors the exponent"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _positive_steps("ExponentialDecay", decay_steps)
        self.decay_rate, self.staircase = float(decay_rate), bool(staircase)
        if self.decay_rate < 0.0:
            raise ValueError(f"ExponentialDecay: decay_rate must be non-negative, got {decay_rate!r}")

    def descriptor(self):
        return dict(kind=LR_EXPONENTIAL, flags=LR_STAIRCASE if self.staircase else 0, initial=self.initial_learning_rate,
                    decay_steps=self.decay_steps, rate=self.decay_rate)


class InverseTimeDecay(LearningRateSchedule):
    """initial_learning_rate / (1 + decay_rate * step / decay_steps); staircase floors step / decay_steps"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _positive_steps("InverseTimeDecay", decay_steps)
        self.decay_rate, self.staircase = float(decay_rate), bool(staircase)
        if self.decay_rate < 0.0:
            raise ValueError(f"InverseTimeDecay: decay_rate must be non-negative, got {decay_rate!r}")

    def descriptor(self):
        return dict(kind=LR_INVERSE_TIME, flags=LR_STAIRCASE if self.staircase else 0, initial=self.initial_learning_rate,
                    decay_steps=self.decay_steps, rate=self.decay_rate)


class PolynomialDecay(LearningRateSchedule):
    """(initial - end) * (1 - step / decay_steps) ^ power + end, with step = min(step, decay_steps); cycle=True instead multiplies
    decay_steps by max(1, ceil(step / decay_steps))"""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=1e-4, power=1.0, cycle=False, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _positive_steps("PolynomialDecay", decay_steps)
        self.end_learning_rate, self.power, self.cycle = float(end_learning_rate), float(power), bool(cycle)
        if not self.power > 0.0:
            raise ValueError(f"PolynomialDecay: power must be positive, got {power!r}")

    def descriptor(self):
        return dict(kind=LR_POLYNOMIAL, flags=LR_CYCLE if self.cycle else 0, initial=self.initial_learning_rate,
                    decay_steps=self.decay_steps, end=self.end_learning_rate, power=self.power)


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] for step <= boundaries[0], values[i] for boundaries[i - 1] < step <= boundaries[i], values[-1] beyond"""

    def __init__(self, boundaries, values, name=None):
        self.boundaries, self.values = [int(b) for b in boundaries], [float(v) for v in values]
        if len(self.values) != len(self.boundaries) + 1:
            raise ValueError("PiecewiseConstantDecay: the length of boundaries should be 1 less than the length of values")
        if not 1 <= len(self.boundaries) <= MAX_BOUNDARIES:
            raise ValueError(f"PiecewiseConstantDecay: 1 to {MAX_BOUNDARIES} boundaries (the schedule kernel's descriptor is passed "
                             f"by value), got {len(self.boundaries)}")
        if any(b <= a for a, b in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError("PiecewiseConstantDecay: boundaries must be strictly increasing")

    def descriptor(self):
        return dict(kind=LR_PIECEWISE, boundaries=list(self.boundaries), values=list(self.values))


class CosineDecay(LearningRateSchedule):
    """initial * ((1 - alpha) * 0.5 * (1 + cos(pi * step / decay_steps)) + alpha), with step = min(step, decay_steps)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _positive_steps("CosineDecay", decay_steps)
        self.alpha = float(alpha)

    def descriptor(self):
        return dict(kind=LR_COSINE, initial=self.initial_learning_rate, decay_steps=self.decay_steps, alpha=self.alpha)


def inverse_decay_descriptor(learning_rate: float, decay: float) -> dict:
    """the legacy `decay` argument of optimizer_v2: lr / (1 + decay * iterations)"""
    return dict(kind=LR_INVERSE_DECAY, initial=float(learning_rate), rate=float(decay))


def evaluate(d: dict, step: int, dtype=np.float32):
    """the schedule `d` (fields of dib_lr_schedule) at `step` in `dtype`: float32 is the arithmetic of dib_lr_schedule_kernel
    operation for operation; float64 is what the tests' restatement is checked against"""
    T = np.dtype(dtype).type
    kind, flags = d["kind"], d.get("flags", 0)
    g = lambda k: T(_f(d.get(k, 0.0)))   # every field is a float32 on the device, whatever the arithmetic's width
    init, ds, rate, one = g("initial"), g("decay_steps"), g("rate"), T(1)
    s = T(step)
    if kind == LR_INVERSE_DECAY:
        return init / (one + rate * s)
    if kind in (LR_EXPONENTIAL, LR_INVERSE_TIME):
        p = s / ds
        if flags & LR_STAIRCASE:
            p = np.floor(p)
        return init * np.power(rate, p) if kind == LR_EXPONENTIAL else init / (one + rate * p)
    if kind == LR_POLYNOMIAL:
        if flags & LR_CYCLE:
            ds = ds * max(one, np.ceil(s / ds))
        else:
            s = min(s, ds)
        return (init - g("end")) * np.power(one - s / ds, g("power")) + g("end")
    if kind == LR_PIECEWISE:
        for b, v in zip(d["boundaries"], d["values"]):
            if step <= b:
                return T(_f(v))
        return T(_f(d["values"][-1]))
    if kind == LR_COSINE:
        s = min(s, ds)
        a = g("alpha")
        return init * (((one - a) * T(0.5)) * (one + np.cos((T(_f(np.pi)) * s) / ds)) + a)
    raise ValueError(f"schedule kind {kind!r}")
