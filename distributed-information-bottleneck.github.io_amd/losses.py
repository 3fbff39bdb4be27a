"""Keras-shaped loss objects and metric names accepted by DistributedIBNet.compile (reference train.py:138-142).

Only the *identity* of the loss lives here; the arithmetic runs on the device.  The reference's own kinds - data.py:65
BinaryCrossentropy(from_logits=True), data.py:343 SparseCategoricalCrossentropy(from_logits=True), 'mse' - run in
csrc/dib_elementwise.h (dib_loss_kernel) and the fused one-unit head; every other kind, every kind with a parameter (label
smoothing, Huber's delta) and every metric beyond today's 'accuracy' runs in csrc/dib_losses.h (dib_loss_ex_kernel), described to
the library by a LossDescriptor (include/dib_losses.h dib_loss_desc, which lists the formulas).
"""
from __future__ import annotations

from collections import namedtuple

# include/dib_hip.h DIB_LOSS_* (0..3) and include/dib_losses.h DIB_LOSS_* (4..14)
KIND_IDS = {"bce_logits": 0, "bce": 1, "sparse_cce_logits": 2, "mse": 3, "mae": 4, "mape": 5, "msle": 6, "huber": 7,
            "log_cosh": 8, "poisson": 9, "kl_divergence": 10, "cosine_similarity": 11, "cce_logits": 12, "cce": 13,
            "sparse_cce": 14}
LEGACY_KINDS = ("bce_logits", "bce", "sparse_cce_logits", "mse")   # dib_loss_fwd_bwd / the fused head
SPARSE_KINDS = ("sparse_cce_logits", "sparse_cce")                 # one label column
CATEGORICAL_KINDS = ("cce_logits", "cce")                          # one-hot (or soft) label rows
# include/dib_losses.h DIB_METRIC_*
METRIC_IDS = {None: 0, "binary_accuracy": 1, "categorical_accuracy": 2, "sparse_categorical_accuracy": 3, "mae": 4, "mse": 5}
# compile(metrics=[name]) -> (History key, metric kind or "accuracy" = resolved from the loss, square root at the epoch's end)
METRIC_NAMES = {
    "accuracy": ("accuracy", "accuracy", False), "acc": ("accuracy", "accuracy", False),
    "binary_accuracy": ("binary_accuracy", "binary_accuracy", False),
    "categorical_accuracy": ("categorical_accuracy", "categorical_accuracy", False),
    "sparse_categorical_accuracy": ("sparse_categorical_accuracy", "sparse_categorical_accuracy", False),
    "mae": ("mae", "mae", False), "mean_absolute_error": ("mean_absolute_error", "mae", False),
    "mse": ("mse", "mse", False), "mean_squared_error": ("mean_squared_error", "mse", False),
    "root_mean_squared_error": ("root_mean_squared_error", "mse", True),
}

# what HipEngine.train_step / eval_step / capture_step_graph take for a loss outside the legacy route
LossDescriptor = namedtuple("LossDescriptor", "kind kind_id metric_id param")

_DEFAULT_REDUCTIONS = (None, "auto", "sum_over_batch_size")


def _check_common(cls_name, reduction, axis, unknown):
    if unknown:
        raise ValueError(f"{cls_name}: unknown argument {sorted(unknown)[0]!r}")
    if reduction not in _DEFAULT_REDUCTIONS:
        raise ValueError(f"{cls_name}: reduction={reduction!r} is not supported: the step's loss is the mean over the batch "
                         "(Keras' default reduction) and the History accounting depends on it")
    if axis != -1:
        raise ValueError(f"{cls_name}: axis={axis!r} is not supported: the model output is [batch, out_dim] and the class "
                         "axis is the last one")


class Loss:
    kind = None
    name = "loss"
    param = 0.0

    def __init__(self, reduction="auto", name=None, **unknown):
        _check_common(type(self).__name__, reduction, -1, unknown)
        if name is not None:
            self.name = name

    @property
    def kind_id(self) -> int:
        return KIND_IDS[self.kind]

    @property
    def legacy(self) -> bool:
        """one of the reference's own kinds with no parameter: dib_loss_fwd_bwd and the fused one-unit head take it"""
        return self.kind in LEGACY_KINDS and self.param == 0.0

    def resolve_metric(self, metric):
        """the DIB_METRIC_* name 'accuracy' stands for under this loss (Keras: by the loss and the label layout)"""
        if metric != "accuracy":
            return metric
        if self.kind in SPARSE_KINDS:
            return "sparse_categorical_accuracy"
        if self.kind in CATEGORICAL_KINDS:
            return "categorical_accuracy"
        return "binary_accuracy"   # what dib_loss_kernel counts for its element-wise kinds: (pred > 0.5) == y

    def check_metric(self, metric):
        m = self.resolve_metric(metric)
        if m is None:
            return m
        sparse = self.kind in SPARSE_KINDS
        if sparse != (m == "sparse_categorical_accuracy"):
            raise ValueError(f"metric {m!r} does not fit loss {self.name!r}: " +
                             ("its labels are one class index per row" if sparse else "its labels are [batch, out_dim] rows"))
        return m

    def descriptor(self, metric=None) -> LossDescriptor:
        """metric: a DIB_METRIC_* name, 'accuracy' or None"""
        if self.kind == "sparse_cce_logits":
            raise ValueError("SparseCategoricalCrossentropy(from_logits=True) runs through dib_loss_fwd_bwd, not a descriptor")
        return LossDescriptor(self.kind, self.kind_id, METRIC_IDS[self.check_metric(metric)], float(self.param))

    def __repr__(self):
        return f"{type(self).__name__}(kind={self.kind!r}" + (f", param={self.param!r})" if self.param else ")")


def _smoothing(cls_name, s):
    s = float(s)
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"{cls_name}: label_smoothing must be in [0, 1], got {s!r}")
    return s


class BinaryCrossentropy(Loss):
    name = "binary_crossentropy"

    def __init__(self, from_logits: bool = False, label_smoothing: float = 0.0, axis=-1, reduction="auto", name=None, **unknown):
        _check_common("BinaryCrossentropy", reduction, axis, unknown)
        super().__init__(name=name)
        self.from_logits = bool(from_logits)
        self.kind = "bce_logits" if from_logits else "bce"
        self.label_smoothing = self.param = _smoothing("BinaryCrossentropy", label_smoothing)


class CategoricalCrossentropy(Loss):
    """one-hot (or soft) label rows [N, C] that sum to 1"""
    name = "categorical_crossentropy"

    def __init__(self, from_logits: bool = False, label_smoothing: float = 0.0, axis=-1, reduction="auto", name=None, **unknown):
        _check_common("CategoricalCrossentropy", reduction, axis, unknown)
        super().__init__(name=name)
        self.from_logits = bool(from_logits)
        self.kind = "cce_logits" if from_logits else "cce"
        self.label_smoothing = self.param = _smoothing("CategoricalCrossentropy", label_smoothing)


class SparseCategoricalCrossentropy(Loss):
    name = "sparse_categorical_crossentropy"

    def __init__(self, from_logits: bool = False, reduction="auto", name=None, **unknown):
        _check_common("SparseCategoricalCrossentropy", reduction, -1, unknown)
        super().__init__(name=name)
        self.from_logits = bool(from_logits)
        self.kind = "sparse_cce_logits" if from_logits else "sparse_cce"   # reference data.py:343 uses from_logits=True


class MeanSquaredError(Loss):
    name = "mean_squared_error"
    kind = "mse"


class MeanAbsoluteError(Loss):
    name = "mean_absolute_error"
    kind = "mae"


class MeanAbsolutePercentageError(Loss):
    name = "mean_absolute_percentage_error"
    kind = "mape"


class MeanSquaredLogarithmicError(Loss):
    name = "mean_squared_logarithmic_error"
    kind = "msle"


class Huber(Loss):
    name = "huber_loss"
    kind = "huber"

    def __init__(self, delta: float = 1.0, reduction="auto", name=None, **unknown):
        _check_common("Huber", reduction, -1, unknown)
        super().__init__(name=name)
        self.delta = self.param = float(delta)
        if not self.delta > 0.0:
            raise ValueError(f"Huber: delta must be positive, got {delta!r}")


class LogCosh(Loss):
    name = "log_cosh"
    kind = "log_cosh"


class Poisson(Loss):
    name = "poisson"
    kind = "poisson"


class KLDivergence(Loss):
    name = "kl_divergence"
    kind = "kl_divergence"


class CosineSimilarity(Loss):
    name = "cosine_similarity"
    kind = "cosine_similarity"

    def __init__(self, axis=-1, reduction="auto", name=None, **unknown):
        _check_common("CosineSimilarity", reduction, axis, unknown)
        super().__init__(name=name)


_BY_NAME = {
    "mse": MeanSquaredError, "mean_squared_error": MeanSquaredError, "meansquarederror": MeanSquaredError,
    "binary_crossentropy": BinaryCrossentropy, "bce": BinaryCrossentropy, "binarycrossentropy": BinaryCrossentropy,
    "mae": MeanAbsoluteError, "mean_absolute_error": MeanAbsoluteError, "meanabsoluteerror": MeanAbsoluteError,
    "mape": MeanAbsolutePercentageError, "mean_absolute_percentage_error": MeanAbsolutePercentageError,
    "meanabsolutepercentageerror": MeanAbsolutePercentageError,
    "msle": MeanSquaredLogarithmicError, "mean_squared_logarithmic_error": MeanSquaredLogarithmicError,
    "meansquaredlogarithmicerror": MeanSquaredLogarithmicError,
    "huber": Huber, "huber_loss": Huber,
    "log_cosh": LogCosh, "logcosh": LogCosh,
    "poisson": Poisson,
    "kl_divergence": KLDivergence, "kld": KLDivergence, "kullback_leibler_divergence": KLDivergence, "kldivergence": KLDivergence,
    "cosine_similarity": CosineSimilarity, "cosinesimilarity": CosineSimilarity,
    "categorical_crossentropy": CategoricalCrossentropy, "categoricalcrossentropy": CategoricalCrossentropy,
    "sparse_categorical_crossentropy": SparseCategoricalCrossentropy, "sparsecategoricalcrossentropy": SparseCategoricalCrossentropy,
}
# Keras converts 0/1 labels to -1/+1 for these by LOOKING at the data (losses.py _maybe_convert_labels): a property of the
# whole label array, not of a row, which the per-row kernel cannot see
_HINGES = ("hinge", "squared_hinge", "categorical_hinge", "squaredhinge", "categoricalhinge")
SUPPORTED = sorted(set(_BY_NAME))


def get(identifier) -> Loss:
    """tf.keras.losses.get equivalent for the kinds on this path: a Loss instance, or one of the names (any letter case) with
    the Keras defaults."""
    if isinstance(identifier, Loss):
        return identifier
    if isinstance(identifier, str):
        name = identifier.lower()
        if name == "infonce":
            raise NotImplementedError("'infonce' is not a Keras-path loss: it trains through the custom loop "
                                      "(reference train.py:180-289) -> dib_amd.infonce.fit_infonce / "
                                      "`python -m dib_amd.train --infonce_loss True`")
        if name in _HINGES:
            raise ValueError(f"unsupported loss {identifier!r}: Keras converts 0/1 labels to -1/+1 for the hinge losses by "
                             "inspecting the whole label array, which the per-row loss kernel does not do")
        if name in _BY_NAME:
            return _BY_NAME[name]()
    kind = getattr(identifier, "kind", None)
    if kind is not None:
        return identifier
    raise ValueError(f"unsupported loss {identifier!r} (supported: {', '.join(SUPPORTED)})")


def get_metric(name):
    """(History key, DIB_METRIC_* name or 'accuracy', take the square root at the end of the epoch) of a compile(metrics=) name"""
    if isinstance(name, str) and name.lower() in METRIC_NAMES:
        return METRIC_NAMES[name.lower()]
    raise ValueError(f"unsupported metric {name!r} (supported: {', '.join(sorted(METRIC_NAMES))})")
