"""CPU: the names, classes and arguments of the Keras loss and metric family (dib_amd/losses.py, compile) and the host-only
entries of include/dib_losses.h.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import dib_oracle as orc
import _oracle_losses as ol
from _helpers import spec_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {
    "mse": ("mse", 0.0), "MSE": ("mse", 0.0), "mean_squared_error": ("mse", 0.0),
    "mae": ("mae", 0.0), "MAE": ("mae", 0.0), "mean_absolute_error": ("mae", 0.0),
    "mape": ("mape", 0.0), "mean_absolute_percentage_error": ("mape", 0.0),
    "msle": ("msle", 0.0), "mean_squared_logarithmic_error": ("msle", 0.0),
    "huber": ("huber", 1.0), "Huber": ("huber", 1.0),
    "log_cosh": ("log_cosh", 0.0), "logcosh": ("log_cosh", 0.0), "LogCosh": ("log_cosh", 0.0),
    "poisson": ("poisson", 0.0), "kl_divergence": ("kl_divergence", 0.0), "kld": ("kl_divergence", 0.0), "KLD": ("kl_divergence", 0.0),
    "cosine_similarity": ("cosine_similarity", 0.0),
    "categorical_crossentropy": ("cce", 0.0), "sparse_categorical_crossentropy": ("sparse_cce", 0.0),
    "binary_crossentropy": ("bce", 0.0), "bce": ("bce", 0.0),
}


def _model(spec):
    import dib_amd
    return dib_amd.DistributedIBNet(**spec_kwargs(spec))


@pytest.mark.parametrize("name", sorted(NAMES))
def test_every_name_resolves_to_its_kind_and_parameter(name):
    from dib_amd import losses
    loss = losses.get(name)
    assert (loss.kind, loss.param) == NAMES[name]
    assert loss.kind_id == losses.KIND_IDS[loss.kind]
    assert losses.get(loss) is loss


def test_classes_carry_their_arguments():
    from dib_amd import losses as L
    assert (L.Huber().kind, L.Huber().param, L.Huber(delta=0.25).param) == ("huber", 1.0, 0.25)
    assert L.CategoricalCrossentropy().kind == "cce" and L.CategoricalCrossentropy(from_logits=True).kind == "cce_logits"
    assert L.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1).param == pytest.approx(0.1)
    assert L.SparseCategoricalCrossentropy().kind == "sparse_cce"                       # Keras' own default, from_logits=False
    assert L.SparseCategoricalCrossentropy(from_logits=True).kind == "sparse_cce_logits"
    for cls, kind in ((L.MeanAbsoluteError, "mae"), (L.MeanAbsolutePercentageError, "mape"), (L.MeanSquaredLogarithmicError, "msle"),
                      (L.LogCosh, "log_cosh"), (L.Poisson, "poisson"), (L.KLDivergence, "kl_divergence"),
                      (L.CosineSimilarity, "cosine_similarity"), (L.MeanSquaredError, "mse")):
        assert cls().kind == kind and cls(reduction="sum_over_batch_size", name="x").name == "x"


def test_binary_crossentropy_no_longer_drops_label_smoothing():
    from dib_amd import losses as L
    plain, smooth = L.BinaryCrossentropy(from_logits=True), L.BinaryCrossentropy(from_logits=True, label_smoothing=0.1)
    assert plain.kind == smooth.kind == "bce_logits"
    assert plain.param == 0.0 and plain.legacy                  # the reference's default: dib_loss_fwd_bwd / the fused head
    assert smooth.param == pytest.approx(0.1) and not smooth.legacy      # a parameter: a descriptor, never the fused head
    d = smooth.descriptor("accuracy")
    assert (d.kind, d.kind_id, d.metric_id, d.param) == ("bce_logits", 0, 1, pytest.approx(0.1))
    assert L.BinaryCrossentropy(label_smoothing=0.2).descriptor().param == pytest.approx(0.2)
    # the float64 helper tells the two apart by far more than any tolerance
    y, p = np.array([[1.0], [0.0]]), np.array([[2.0], [-1.0]])
    a, b = ol.rows_and_grad("bce_logits", y, p, 0.0)[0], ol.rows_and_grad("bce_logits", y, p, 0.1)[0]
    assert np.abs(a - b).max() > 0.04


@pytest.mark.parametrize("bad, reason", [
    ("hinge", "hinge"), ("squared_hinge", "hinge"), ("categorical_hinge", "hinge"), ("SquaredHinge", "hinge"),
    ("focal", "unsupported loss"), (3, "unsupported loss")])
def test_unsupported_names_raise_with_their_reason(bad, reason):
    from dib_amd import losses
    with pytest.raises(ValueError, match=reason):
        losses.get(bad)


def test_unsupported_arguments_raise_with_their_reason():
    from dib_amd import losses as L
    for cls in (L.BinaryCrossentropy, L.CategoricalCrossentropy, L.SparseCategoricalCrossentropy, L.MeanSquaredError,
                L.MeanAbsoluteError, L.Huber, L.LogCosh, L.Poisson, L.KLDivergence, L.CosineSimilarity):
        with pytest.raises(ValueError, match="reduction"):
            cls(reduction="sum")
        with pytest.raises(ValueError, match="reduction"):
            cls(reduction="none")
        with pytest.raises(ValueError, match="unknown argument 'ignore_class'"):
            cls(ignore_class=3)
    for cls in (L.BinaryCrossentropy, L.CategoricalCrossentropy, L.CosineSimilarity):
        with pytest.raises(ValueError, match="axis"):
            cls(axis=0)
        assert cls(axis=-1).kind
    with pytest.raises(ValueError, match="label_smoothing"):
        L.CategoricalCrossentropy(label_smoothing=1.5)
    with pytest.raises(ValueError, match="delta"):
        L.Huber(delta=0.0)


METRICS = {"accuracy": "accuracy", "acc": "accuracy", "binary_accuracy": "binary_accuracy",
           "categorical_accuracy": "categorical_accuracy", "mae": "mae", "mean_absolute_error": "mean_absolute_error",
           "mse": "mse", "mean_squared_error": "mean_squared_error", "root_mean_squared_error": "root_mean_squared_error"}


def test_metrics_resolve_and_a_second_metric_raises():
    from dib_amd import losses as L
    spec = orc.DIBSpec([1, 1], [4], [4], 3, feature_embedding_dimension=4)
    m = _model(spec)
    for name, key in METRICS.items():
        m.compile(optimizer="adam", loss=L.CategoricalCrossentropy(from_logits=True), metrics=[name])
        assert m._metric[0] == key
        logs = m._epoch_logs(np.array([1.0, 2.0, 30.0, 16.0, 4.0]), 2, "val_")
        assert logs["val_" + key] == (2.0 if name == "root_mean_squared_error" else 4.0)    # 16 / 4 rows, the root at the end
    # 'accuracy' by the loss: arg-max against arg-max under the categorical losses, the label index under the sparse ones,
    # the 0.5 threshold (today's count) elsewhere
    for loss, want in ((L.CategoricalCrossentropy(), 2), (L.CategoricalCrossentropy(from_logits=True), 2),
                       (L.SparseCategoricalCrossentropy(), 3), (L.MeanAbsoluteError(), 1), (L.BinaryCrossentropy(label_smoothing=0.1), 1)):
        assert loss.descriptor("accuracy").metric_id == want
    assert L.Huber().descriptor("mae").metric_id == 4 and L.Huber().descriptor("mse").metric_id == 5 and L.Huber().descriptor().metric_id == 0
    m.compile(optimizer="adam", loss=L.SparseCategoricalCrossentropy(), metrics=["sparse_categorical_accuracy"])
    assert m._loss_arg().metric_id == 3
    with pytest.raises(ValueError, match="one metric per compile"):
        m.compile(optimizer="adam", loss="mse", metrics=["mae", "mse"])
    with pytest.raises(ValueError, match="unsupported metric"):
        m.compile(optimizer="adam", loss="mse", metrics=["auc"])
    with pytest.raises(ValueError, match="does not fit"):
        m.compile(optimizer="adam", loss="mse", metrics=["sparse_categorical_accuracy"])
    with pytest.raises(ValueError, match="does not fit"):
        m.compile(optimizer="adam", loss=L.SparseCategoricalCrossentropy(from_logits=True), metrics=["mae"])


def test_the_reference_kinds_keep_the_name_route():
    """bce_logits / mse / sparse_cce_logits with no metric or 'accuracy' reach the engine by name, as before; a metric beyond it
    or a parameter makes a descriptor"""
    from dib_amd import losses as L
    m = _model(orc.DIBSpec([1, 1], [4], [4], 1, feature_embedding_dimension=4))
    for loss, kind in ((L.BinaryCrossentropy(from_logits=True), "bce_logits"), ("mse", "mse"), (L.BinaryCrossentropy(), "bce"),
                       (L.SparseCategoricalCrossentropy(from_logits=True), "sparse_cce_logits")):
        for metrics in (None, ["accuracy"], ["acc"]):
            m.compile(optimizer="adam", loss=loss, metrics=metrics)
            assert m._loss_arg() == kind
    m.compile(optimizer="adam", loss="mse", metrics=["mae"])
    assert tuple(m._loss_arg()) == ("mse", 3, 4, 0.0)
    m.compile(optimizer="adam", loss="huber", metrics=["root_mean_squared_error"])
    assert tuple(m._loss_arg()) == ("huber", 7, 5, 1.0)


def test_header_and_library_say_abi_7_and_the_host_entries_answer():
    from dib_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "dib_hip.h")).read()
    assert re.search(r"#define DIB_ABI_VERSION 7\b", hdr) and L.ABI_VERSION == 7
    lib = L.load_library()
    assert lib.dib_abi_version() == 7
    lh = open(os.path.join(ROOT, "include", "dib_losses.h")).read()
    declared = set(re.findall(r"^int (dib_\w+)\(", lh, re.M))
    assert declared == set(L.SIGNATURES_LOSSES), declared ^ set(L.SIGNATURES_LOSSES)
    from dib_amd import losses
    for name, value in re.findall(r"#define DIB_LOSS_(\w+) (\d+)", lh):
        py = {"LOGCOSH": "log_cosh", "KLD": "kl_divergence", "COSINE": "cosine_similarity"}.get(name, name.lower())
        assert losses.KIND_IDS[py] == int(value), name
    for name, value in re.findall(r"#define DIB_METRIC_(\w+) (\d+)", lh):
        assert losses.METRIC_IDS[None if name == "NONE" else name.lower()] == int(value), name
    sup = lambda k, m, p, c=3: lib.dib_loss_ex_supported(ctypes.byref(L.LossDesc(k, m, p)), c)
    assert all(sup(k, 0, 0.0) == 1 for k in (0, 1, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14)) and sup(7, 0, 1.0) == 1
    assert sup(2, 0, 0.0) == 0 and sup(15, 0, 0.0) == 0 and sup(-1, 0, 0.0) == 0            # dib_loss_fwd_bwd's own; unknown
    assert sup(7, 0, 0.0) == 0 and sup(7, 0, -1.0) == 0 and sup(7, 0, float("nan")) == 0    # Huber's delta
    assert sup(12, 0, 1.0) == 1 and sup(12, 0, 1.5) == 0 and sup(4, 0, 0.1) == 0             # smoothing where it means something
    assert sup(14, 3, 0.0) == 1 and sup(14, 4, 0.0) == 0 and sup(4, 3, 0.0) == 0 and sup(4, 6, 0.0) == 0
    assert sup(4, 0, 0.0, 0) == 0 and lib.dib_loss_ex_supported(None, 3) == 0
    assert [lib.dib_loss_ex_lanes(c) for c in (0, 1, 2, 4, 5, 16, 17, 1000)] == [-1, 1, 4, 4, 16, 16, 64, 64]
