"""Keras-shaped optimizer objects (reference train.py:128-129: tf.keras.optimizers.get(name); optimizer.learning_rate = 3e-4).
The update itself is a fused flat-buffer HIP kernel: dib_adam_kernel / dib_sgd_kernel (and the step tail) for Adam and
momentum-free SGD, the dib_opt_kernel family (csrc/dib_optimizers.h, include/dib_optimizers.h) for every other rule.  The rules
are Keras optimizer_v2's (TF 2.x before 2.11).  So are clipvalue, clipnorm, global_clipnorm (the gradient the rule
sees, include/dib_grad_transform.h), the legacy `decay` and a schedules.LearningRateSchedule as `learning_rate` (the rate of a step,
evaluated on the device from the step count).  The four clip / decay settings are ATTRIBUTES, as optimizer_v2 has them too -
`opt = Adam(3e-4); opt.clipnorm = 1.0`, `opt.configure(global_clipnorm=1.0)`, `optimizers.get("adam", clipnorm=1.0)`,
`optimizers.build(Adam, 3e-4, clipnorm=1.0)` - and NOT constructor keywords: the constructors keep refusing every keyword that
would change the update (tests/test_optimizers_host.py pins that), with a message that names the attribute route.  A change of
those settings is not a change of rule: it does not reset the optimizer state."""
from __future__ import annotations

from . import schedules as _schedules

# include/dib_optimizers.h DIB_OPT_*
OPT_SGD_MOMENTUM, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADADELTA, OPT_ADAMAX, OPT_NADAM, OPT_AMSGRAD = range(1, 8)

SUPPORTED = ("adadelta", "adagrad", "adam", "adamax", "nadam", "rmsprop", "sgd")
# Keras >= 2.11 arguments (optimizer_v2 never had them) that no kernel here applies: refused, never dropped
UNSUPPORTED_ARGUMENTS = ("weight_decay", "use_ema")
# optimizer_v2's arguments that change the gradient or the learning rate before the rule sees them (include/dib_grad_transform.h)
TRANSFORM_ARGUMENTS = ("clipnorm", "clipvalue", "global_clipnorm", "decay")
# include/dib_grad_transform.h DIB_CLIP_*
CLIP_NONE, CLIP_NORM, CLIP_GLOBAL_NORM = 0, 1, 2


def _reject(cls_name: str, kwargs: dict) -> None:
    for k in kwargs:
        if k in UNSUPPORTED_ARGUMENTS:
            raise ValueError(f"{cls_name}: argument {k!r} is not supported (weight_decay and use_ema belong to the Keras >= 2.11 "
                             f"optimizers, not to optimizer_v2 whose rules these are; supported optimizers: {', '.join(SUPPORTED)})")
        if k in TRANSFORM_ARGUMENTS:
            raise ValueError(f"{cls_name}: {k!r} is not a constructor argument here: set it on the object (optimizer.{k} = value, or "
                             f"optimizer.configure({k}=value)) or pass it to optimizers.get(name, {k}=value) / "
                             f"optimizers.build({cls_name}, ..., {k}=value) (supported optimizers: {', '.join(SUPPORTED)})")
        if k != "name":   # (Keras' cosmetic `name` changes nothing)
            raise ValueError(f"{cls_name}: unknown argument {k!r} (supported optimizers: {', '.join(SUPPORTED)})")


class Optimizer:
    name = "optimizer"
    kind = 0   # DIB_OPT_* of the dib_optimizer_* entries; 0: the rule has launches of its own (Adam, momentum-free SGD)

    def __init__(self, learning_rate):
        self._clip = dict(clipnorm=None, clipvalue=None, global_clipnorm=None)
        self._decay = 0.0
        self.learning_rate = learning_rate

    # ---- what happens to the gradient and the learning rate before the rule (include/dib_grad_transform.h) ----------------------
    def _set_threshold(self, key: str, value) -> None:
        """a clip threshold: None, or a finite number > 0; clipnorm and global_clipnorm exclude each other"""
        cls = type(self).__name__
        if value is not None:
            v = float(value)
            if not (v > 0.0 and v < float("inf")):
                raise ValueError(f"{cls}: {key} must be a positive number, got {value!r}")
            other = {"clipnorm": "global_clipnorm", "global_clipnorm": "clipnorm"}.get(key)
            if other is not None and self._clip[other] is not None:
                raise ValueError(f"{cls}: Cannot accept both `clipnorm` and `global_clipnorm`, got {key}={value!r} with "
                                 f"{other}={self._clip[other]!r}")
            value = v
        self._clip[key] = value

    clipnorm = property(lambda self: self._clip["clipnorm"], lambda self, v: self._set_threshold("clipnorm", v),
                        doc="per variable: g = (g * c) / max(||g||, c); None = off")
    clipvalue = property(lambda self: self._clip["clipvalue"], lambda self, v: self._set_threshold("clipvalue", v),
                         doc="per element: g = min(max(g, -c), c); None = off")
    global_clipnorm = property(lambda self: self._clip["global_clipnorm"], lambda self, v: self._set_threshold("global_clipnorm", v),
                               doc="over all variables: g = g * c * min(1 / N, 1 / c); None = off")

    @property
    def decay(self) -> float:
        """the legacy `decay`: lr_t = lr / (1 + decay * iterations); 0 = off"""
        return self._decay

    @decay.setter
    def decay(self, value) -> None:
        v = float(value or 0.0)
        if not (0.0 <= v < float("inf")):
            raise ValueError(f"{type(self).__name__}: decay must be non-negative, got {value!r}")
        if v > 0.0 and self._schedule is not None:
            raise ValueError(f"{type(self).__name__}: a LearningRateSchedule and the legacy `decay` cannot be combined")
        self._decay = v

    def configure(self, **settings) -> "Optimizer":
        """assign any of clipnorm, clipvalue, global_clipnorm, decay; returns self"""
        for k, v in settings.items():
            if k not in TRANSFORM_ARGUMENTS:
                raise ValueError(f"{type(self).__name__}.configure: unknown setting {k!r} (settings: {', '.join(TRANSFORM_ARGUMENTS)})")
            setattr(self, k, v)
        return self

    @property
    def learning_rate(self):
        """a float, or the schedules.LearningRateSchedule given; assigning a float replaces a schedule (reference train.py:129)"""
        return self._schedule if self._schedule is not None else self._lr

    @learning_rate.setter
    def learning_rate(self, value):
        if isinstance(value, _schedules.LearningRateSchedule):
            if self._decay > 0.0:
                raise ValueError(f"{type(self).__name__}: a LearningRateSchedule and the legacy `decay` cannot be combined")
            self._schedule, self._lr = value, float(value(0))
        else:
            self._schedule, self._lr = None, float(value)

    def lr_schedule(self):
        """None for a constant learning rate (HipEngine.set_lr), else the fields of dib_lr_schedule: the rate is evaluated on the
        device from the step count by dib_lr_schedule_eval"""
        if self._schedule is not None:
            return self._schedule.descriptor()
        if self._decay > 0.0:
            return _schedules.inverse_decay_descriptor(self._lr, self._decay)
        return None

    def clip(self):
        """None, or (clipvalue or 0.0, DIB_CLIP_* mode, norm threshold): the transform of include/dib_grad_transform.h that runs on
        the aggregated gradient before the rule.  An optimizer with one never rides in the step tail."""
        norm, value, global_norm = self._clip["clipnorm"], self._clip["clipvalue"], self._clip["global_clipnorm"]
        if norm is None and global_norm is None and value is None:
            return None
        mode = CLIP_NORM if norm is not None else CLIP_GLOBAL_NORM if global_norm is not None else CLIP_NONE
        return (value or 0.0, mode, norm or global_norm or 0.0)

    @property
    def native(self) -> bool:
        """True: dib_adam_step / dib_sgd_step and the step tail's DIB_TAIL_ADAM / DIB_TAIL_SGD apply the rule"""
        return self.kind == 0

    @property
    def rides_in_tail(self) -> bool:
        """the step's LAST launch applies this optimizer (DIB_TAIL_ADAM / DIB_TAIL_SGD); else launches of its own follow the tail"""
        return self.native and self.clip() is None

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
_LEGACY = {}   # ("adam", beta_1, beta_2, epsilon) / ("sgd",) -> its Optimizer: as_optimizer on a hot path is one dict lookup


def as_optimizer(x) -> Optimizer:
    """The Optimizer the engine's step entries work on: `x` itself, or the Adam / momentum-free SGD of the legacy tuples
    ("adam", beta_1, beta_2, epsilon) / ("sgd",) - one object per tuple, made on first sight.  Anything else: ValueError."""
    try:
        return x if isinstance(x, Optimizer) else _LEGACY[x]
    except (KeyError, TypeError):   # (not seen yet, or nothing that can be a key)
        pass
    if isinstance(x, tuple) and len(x) == 4 and x[0] == "adam" and all(isinstance(v, (int, float)) for v in x[1:]):
        return _LEGACY.setdefault(x, Adam(beta_1=x[1], beta_2=x[2], epsilon=x[3]))
    if x == ("sgd",):
        return _LEGACY.setdefault(x, SGD())
    raise ValueError(f"not an optimizer: {x!r} (an optimizers.Optimizer, ('adam', beta_1, beta_2, epsilon) or ('sgd',))")


def build(cls, *args, **kwargs) -> Optimizer:
    """cls(*args, **rule keywords) with the clip / decay keywords among `kwargs` assigned afterwards (Optimizer.configure)"""
    settings = {k: kwargs.pop(k) for k in TRANSFORM_ARGUMENTS if k in kwargs}
    return cls(*args, **kwargs).configure(**settings)


def get(identifier, **kwargs) -> Optimizer:
    """tf.keras.optimizers.get: an Optimizer instance, or one of the names (any letter case) with the Keras defaults.  Keyword
    arguments (not Keras': the training script's clip / decay flags) go with a name: `build` of the named class."""
    if isinstance(identifier, Optimizer):
        if kwargs:
            raise ValueError("optimizers.get: keyword arguments go with a name, not with an Optimizer instance")
        return identifier
    if isinstance(identifier, str):
        cls = _BY_NAME.get(identifier.lower())
        if cls is not None:
            return build(cls, **kwargs)
    raise ValueError(f"unsupported optimizer {identifier!r} (supported: {', '.join(repr(n) for n in SUPPORTED)})")
