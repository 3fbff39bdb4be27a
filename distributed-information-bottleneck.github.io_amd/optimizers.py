"""Keras-shaped optimizer objects (reference train.py:128-129: tf.keras.optimizers.get(name); optimizer.learning_rate = 3e-4).
The update itself is a fused flat-buffer HIP kernel: dib_adam_kernel / dib_sgd_kernel (and the step tail) for Adam and
momentum-free SGD, the dib_opt_kernel family (csrc/dib_optimizers.h, include/dib_optimizers.h) for every other rule.  The rules
are Keras optimizer_v2's (TF 2.x before 2.11)."""
from __future__ import annotations

# include/dib_optimizers.h DIB_OPT_*
OPT_SGD_MOMENTUM, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADADELTA, OPT_ADAMAX, OPT_NADAM, OPT_AMSGRAD = range(1, 8)

SUPPORTED = ("adadelta", "adagrad", "adam", "adamax", "nadam", "rmsprop", "sgd")
# Keras arguments that change the update and that no kernel here applies: refused, never dropped
UNSUPPORTED_ARGUMENTS = ("clipnorm", "clipvalue", "global_clipnorm", "decay", "weight_decay", "use_ema")


def _reject(cls_name: str, kwargs: dict) -> None:
    for k in kwargs:
        if k in UNSUPPORTED_ARGUMENTS:
            raise ValueError(f"{cls_name}: argument {k!r} is not supported (gradient clipping, decay and EMA are not "
                             f"implemented; supported optimizers: {', '.join(SUPPORTED)})")
        if k != "name":   # (Keras' cosmetic `name` changes nothing)
            raise ValueError(f"{cls_name}: unknown argument {k!r} (supported optimizers: {', '.join(SUPPORTED)})")


class Optimizer:
    name = "optimizer"
    kind = 0   # DIB_OPT_* of the dib_optimizer_* entries; 0: the rule has launches of its own (Adam, momentum-free SGD)

    def __init__(self, learning_rate: float):
        self.learning_rate = float(learning_rate)

    @property
    def native(self) -> bool:
        """True: dib_adam_step / dib_sgd_step and the step tail's DIB_TAIL_ADAM / DIB_TAIL_SGD apply the rule"""
        return self.kind == 0

    def hyper(self) -> dict:
        """fields of include/dib_optimizers.h dib_optimizer_hyper"""
        return {}

    def slots(self) -> int:
        """state buffers the rule needs (dib_optimizer_slots; Adam's two are the engine's own)"""
        return 0


class Adam(Optimizer):
    """Keras Adam defaults: lr 1e-3, beta_1 0.9, beta_2 0.999, epsilon 1e-7.  amsgrad=True keeps
    vhat = max(vhat, v) in a third state buffer and divides by sqrt(vhat)."""
    name = "adam"

    def __init__(self, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-7, amsgrad: bool = False, **kwargs):
        _reject("Adam", kwargs)
        super().__init__(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.amsgrad = bool(amsgrad)

    @property
    def kind(self):
        return OPT_AMSGRAD if self.amsgrad else 0

    def hyper(self):
        return dict(rho=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)

    def slots(self):
        return 3 if self.amsgrad else 2


class SGD(Optimizer):
    """Keras SGD: lr 0.01, momentum 0.  momentum > 0: a = momentum a - lr g; w += a (nesterov: w += momentum a - lr g)."""
    name = "sgd"

    def __init__(self, learning_rate: float = 0.01, momentum: float = 0.0, nesterov: bool = False, **kwargs):
        _reject("SGD", kwargs)
        super().__init__(learning_rate)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        if not 0.0 <= self.momentum <= 1.0:
            raise ValueError(f"SGD: momentum must be in [0, 1], got {momentum!r}")

    @property
    def kind(self):
        return OPT_SGD_MOMENTUM if self.momentum > 0.0 else 0

    def hyper(self):
        return dict(momentum=self.momentum, nesterov=int(self.nesterov))

    def slots(self):
        return 1 if self.momentum > 0.0 else 0


class RMSprop(Optimizer):
    """Keras RMSprop: lr 1e-3, rho 0.9, momentum 0, epsilon 1e-7, centered False."""
    name = "rmsprop"
    kind = OPT_RMSPROP

    def __init__(self, learning_rate: float = 1e-3, rho: float = 0.9, momentum: float = 0.0, epsilon: float = 1e-7,
                 centered: bool = False, **kwargs):
        _reject("RMSprop", kwargs)
        super().__init__(learning_rate)
        self.rho, self.momentum, self.epsilon, self.centered = float(rho), float(momentum), float(epsilon), bool(centered)
        if not 0.0 <= self.momentum <= 1.0:
            raise ValueError(f"RMSprop: momentum must be in [0, 1], got {momentum!r}")

    def hyper(self):
        return dict(rho=self.rho, momentum=self.momentum, epsilon=self.epsilon, centered=int(self.centered))

    def slots(self):
        return 1 + int(self.centered) + int(self.momentum > 0.0)


class Adagrad(Optimizer):
    """Keras Adagrad: lr 1e-3, initial_accumulator_value 0.1, epsilon 1e-7."""
    name = "adagrad"
    kind = OPT_ADAGRAD

    def __init__(self, learning_rate: float = 1e-3, initial_accumulator_value: float = 0.1, epsilon: float = 1e-7, **kwargs):
        _reject("Adagrad", kwargs)
        super().__init__(learning_rate)
        self.initial_accumulator_value, self.epsilon = float(initial_accumulator_value), float(epsilon)
        if self.initial_accumulator_value < 0.0:
            raise ValueError(f"Adagrad: initial_accumulator_value must be non-negative, got {initial_accumulator_value!r}")

    def hyper(self):
        return dict(epsilon=self.epsilon, initial_accumulator=self.initial_accumulator_value)

    def slots(self):
        return 1


class Adadelta(Optimizer):
    """Keras Adadelta: lr 1e-3, rho 0.95, epsilon 1e-7."""
    name = "adadelta"
    kind = OPT_ADADELTA

    def __init__(self, learning_rate: float = 1e-3, rho: float = 0.95, epsilon: float = 1e-7, **kwargs):
        _reject("Adadelta", kwargs)
        super().__init__(learning_rate)
        self.rho, self.epsilon = float(rho), float(epsilon)

    def hyper(self):
        return dict(rho=self.rho, epsilon=self.epsilon)

    def slots(self):
        return 2


class Adamax(Optimizer):
    """Keras Adamax: lr 1e-3, beta_1 0.9, beta_2 0.999, epsilon 1e-7."""
    name = "adamax"
    kind = OPT_ADAMAX

    def __init__(self, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, **kwargs):
        _reject(type(self).__name__, kwargs)
        super().__init__(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    def hyper(self):
        return dict(rho=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)

    def slots(self):
        return 2


class Nadam(Adamax):
    """Keras Nadam: lr 1e-3, beta_1 0.9, beta_2 0.999, epsilon 1e-7; momentum schedule 0.96^(0.004 t), whose running product is
    one device float64 next to the step count."""
    name = "nadam"
    kind = OPT_NADAM


_BY_NAME = {"adam": Adam, "sgd": SGD, "rmsprop": RMSprop, "adagrad": Adagrad, "adadelta": Adadelta, "adamax": Adamax,
            "nadam": Nadam}


def get(identifier) -> Optimizer:
    """tf.keras.optimizers.get: an Optimizer instance, or one of the names (any letter case) with the Keras defaults."""
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        cls = _BY_NAME.get(identifier.lower())
        if cls is not None:
            return cls()
    raise ValueError(f"unsupported optimizer {identifier!r} (supported: {', '.join(repr(n) for n in SUPPORTED)})")
