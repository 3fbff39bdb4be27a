"""NumPy restatements of the Keras optimizer_v2 update rules of include/dib_optimizers.h - the checker of the optimizer tests.

`Rule(name, **hyper)` with `init(n, dtype)` and `step(w, g, state, lr)`: plain array formulas in the dtype of the state.  With
float64 they are the reference the device kernels are compared with; with float32 the SAME code measures what the number format
alone costs (tests/test_gpu_optimizers.py takes its tolerance from that difference, never from the device's output).  Nadam's
running product P is a float64 in both, as on the device.  `eps_swapped=True` (RMSprop) moves epsilon to the other side of the
square root in either branch: the tests show that their inputs can tell the two placements apart.

`cases()` are the rule configurations the tests run, `inputs()` the shared parameters / gradients / learning rates."""
import functools

import numpy as np


class Rule:
    def __init__(self, name, **hyper):
        self.name, self.h = name, hyper

    def init(self, n, dtype):
        z = lambda v=0.0: np.full(n, v, dtype=dtype)
        slots = {"sgd": [z()], "adagrad": [z(self.h.get("initial_accumulator_value", 0.1))], "adadelta": [z(), z()],
                 "adamax": [z(), z()], "nadam": [z(), z()], "amsgrad": [z(), z(), z()], "adam": [z(), z()]}.get(self.name)
        if self.name == "rmsprop":
            slots = [z()] + ([z()] if self.h.get("centered") else []) + ([z()] if self.h.get("momentum", 0.0) > 0 else [])
        return dict(slots=slots, t=0, P=1.0)

    def step(self, w, g, state, lr):
        """one update in place of (w, state); w, g and the slots share one dtype"""
        T = w.dtype.type
        h = {k: (T(v) if isinstance(v, float) else v) for k, v in self.h.items()}
        s, lr, one = state["slots"], T(lr), T(1)
        g = g.astype(w.dtype)
        t = state["t"] + 1
        if self.name == "sgd":
            mom = h["momentum"]
            s[0][:] = mom * s[0] - lr * g
            w += (mom * s[0] - lr * g) if h.get("nesterov") else s[0]
        elif self.name == "rmsprop":
            rho, mom, eps = h.get("rho", T(0.9)), h.get("momentum", T(0)), h.get("epsilon", T(1e-7))
            swapped = bool(self.h.get("eps_swapped"))
            s[0][:] = rho * s[0] + (one - rho) * (g * g)
            den = s[0]
            if h.get("centered"):
                s[1][:] = rho * s[1] + (one - rho) * g
                den = s[0] - s[1] * s[1]
            if mom > 0:
                m = s[-1]
                m[:] = mom * m + (lr * g) / ((np.sqrt(den) + eps) if swapped else np.sqrt(den + eps))
                w -= m
            else:
                w -= (lr * g) / (np.sqrt(den + eps) if swapped else (np.sqrt(den) + eps))
        elif self.name == "adagrad":
            eps = h.get("epsilon", T(1e-7))
            s[0] += g * g
            w -= (lr * g) / (np.sqrt(s[0]) + eps)
        elif self.name == "adadelta":
            rho, eps = h.get("rho", T(0.95)), h.get("epsilon", T(1e-7))
            s[0][:] = rho * s[0] + (one - rho) * (g * g)
            u = g * np.sqrt(s[1] + eps) / np.sqrt(s[0] + eps)
            s[1][:] = rho * s[1] + (one - rho) * (u * u)
            w -= lr * u
        elif self.name == "adamax":
            b1, b2, eps = h.get("beta_1", T(0.9)), h.get("beta_2", T(0.999)), h.get("epsilon", T(1e-7))
            s[0][:] = b1 * s[0] + (one - b1) * g
            s[1][:] = np.maximum(b2 * s[1], np.abs(g))
            w -= (lr / (one - b1 ** T(t))) * s[0] / (s[1] + eps)
        elif self.name == "nadam":
            b1, b2, eps = h.get("beta_1", T(0.9)), h.get("beta_2", T(0.999)), h.get("epsilon", T(1e-7))
            mu = lambda k: b1 * (one - T(0.5) * T(0.96) ** (T(0.004) * T(k)))
            u_t, u_n = mu(t), mu(t + 1)
            p_t = state["P"] * float(u_t)
            p_n = p_t * float(u_n)
            s[0][:] = b1 * s[0] + (one - b1) * g
            s[1][:] = b2 * s[1] + (one - b2) * (g * g)
            cg, cm = (one - u_t) / T(1.0 - p_t), u_n / T(1.0 - p_n)
            w -= (lr * (cg * g + cm * s[0])) / (np.sqrt(s[1] / (one - b2 ** T(t))) + eps)
            state["P"] = p_t
        elif self.name in ("amsgrad", "adam"):   # the project's Adam: m += (1 - b1)(g - m), v += (1 - b2)(g^2 - v)
            b1, b2, eps = h.get("beta_1", T(0.9)), h.get("beta_2", T(0.999)), h.get("epsilon", T(1e-7))
            s[0] += (one - b1) * (g - s[0])
            s[1] += (one - b2) * (g * g - s[1])
            lr_t = lr * np.sqrt(one - b2 ** T(t)) / (one - b1 ** T(t))
            if self.name == "amsgrad":
                s[2][:] = np.maximum(s[2], s[1])
            w -= (lr_t * s[0]) / (np.sqrt(s[2] if self.name == "amsgrad" else s[1]) + eps)
        else:
            raise ValueError(self.name)
        state["t"] = t


def cases():
    """{case id: (Rule, base learning rate of the tests)}: every rule of the family with every flag combination.  lr = 1e-2 moves
    the parameters a few 1e-2 in 8 steps; Adadelta's update is about sqrt(eps) * lr per step at first, so it runs at lr = 1."""
    return {
        "sgd_momentum": (Rule("sgd", momentum=0.9), 1e-2),
        "sgd_nesterov": (Rule("sgd", momentum=0.9, nesterov=True), 1e-2),
        "rmsprop": (Rule("rmsprop"), 1e-2),
        "rmsprop_centered": (Rule("rmsprop", centered=True), 1e-2),
        "rmsprop_momentum": (Rule("rmsprop", momentum=0.8), 1e-2),
        "rmsprop_centered_momentum": (Rule("rmsprop", centered=True, momentum=0.8), 1e-2),
        "adagrad": (Rule("adagrad"), 1e-2),
        "adadelta": (Rule("adadelta"), 1.0),
        "adamax": (Rule("adamax"), 1e-2),
        "nadam": (Rule("nadam"), 1e-2),
        # beta_2 = 0.9: at Keras' 0.999 v falls by at most 0.1 % a step, vhat = max(vhat, v) stays within 1 % of v over 8 steps
        # and a kernel that divided by sqrt(v) - plain Adam - would move the parameters like the right one to 5e-5
        "amsgrad": (Rule("amsgrad", beta_2=0.9), 1e-2),
    }


STEPS = 8
LR_FACTORS = (1.0, 0.5, 2.0, 1.0, 0.25, 1.5, 1.0, 0.75)   # the learning rate changes between steps (a device scalar on the GPU)


@functools.lru_cache(maxsize=4)
def inputs(n=4099, seed=0, steps=STEPS):
    """(w0 [n] float32 of unit scale, grads [steps][n] float32, zero block, small block): fresh gradients per step, normal x
    10^U(-4, 0) as in test_adam_matches_keras_form; exactly zero on `zero` (every step), +-1e-4 on `small`."""
    rng = np.random.default_rng(seed)
    w0 = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal((steps, n)) * 10.0 ** rng.uniform(-4, 0, size=(steps, n))).astype(np.float32)
    k = max(1, n // 8)
    zero, small = slice(0, k), slice(k, 2 * k)
    g[:, zero] = 0.0
    g[:, small] = np.float32(1e-4) * rng.choice(np.float32([-1.0, 1.0]), size=(steps, min(k, max(n - k, 0))))
    w0.setflags(write=False)
    g.setflags(write=False)
    return w0, g, zero, small


def run(rule, lr, dtype, n=4099, seed=0, steps=STEPS):
    """(w, slots, P) after `steps` steps of `rule` on inputs(n, seed, steps) in `dtype`"""
    w0, g, _, _ = inputs(n, seed, steps)
    w = w0.astype(dtype)
    st = rule.init(n, dtype)
    for k in range(steps):
        rule.step(w, g[k], st, lr * LR_FACTORS[k % len(LR_FACTORS)])
    return w, st["slots"], st["P"]


@functools.lru_cache(maxsize=None)
def reference(case, n=4099, seed=0, steps=STEPS):
    """float64 result of a case of cases() on inputs(n, seed, steps): computed once, shared by the tests, never modified"""
    rule, lr = cases()[case]
    w, slots, P = run(rule, lr, np.float64, n, seed, steps)
    for a in [w] + slots:
        a.setflags(write=False)
    return w, slots, P


@functools.lru_cache(maxsize=None)
def format_error(case, n=4099, seed=0, steps=STEPS):
    """(max |float32 restatement - float64 restatement| of the parameters, per slot the same relative to the slot's float64
    scale): what the fp32 number format alone costs on these inputs"""
    rule, lr = cases()[case]
    w64, s64, _ = reference(case, n, seed, steps)
    w32, s32, _ = run(rule, lr, np.float32, n, seed, steps)
    rel = [float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300)) for a, b in zip(s32, s64)]
    return float(np.abs(w32.astype(np.float64) - w64).max()), rel


FACTOR = 4.0   # on format_error: fused multiply-add contraction, the device's sqrt / divide / powf rounding
ULP = 2.0 ** -23


def bounds(case, n=4099, seed=0, steps=STEPS):
    """(absolute bound on the parameters, relative bound per state slot) of the float64 comparison: FACTOR x format_error, and
    never below one float32 ulp of the compared scale (a slot the float32 code happens to hit exactly still rounds on the device)"""
    pw, ps = format_error(case, n, seed, steps)
    return max(FACTOR * pw, ULP), [max(FACTOR * r, ULP) for r in ps]
