"""CPU checks of the measurement-partition model (chaos notebook cell 10): the float64 oracle's gradients against central
finite differences, the notebook's beta schedule, sequence indices and majority rule, the C ABI bindings, and that the
product refuses to run without the kernels."""
import os
import re

import numpy as np
import pytest

import _oracle_measurement as om
import dib_amd
from dib_amd import _lib, measurement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(rng, d=1, E=2, H=3, A=3, L=3, D=4, n_freq=3):
    lay = lambda dims: sum(([rng.standard_normal((i, o)) * 0.5, rng.standard_normal(o) * 0.1] for i, o in zip(dims[:-1], dims[1:])), [])
    return {"ib": lay([d * n_freq, H, H, 2 * E]), "vq": lay([E, H, H, A]), "agg": lay([L * A, H, H, D]), "ref": lay([d * n_freq, H, H, D])}


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0])
def test_oracle_gradients_agree_with_central_differences(p):
    rng = np.random.default_rng(0)
    w = _tiny(rng)
    states = rng.uniform(-1, 1, (4, 3, 1))
    eps = rng.standard_normal((12, 2))
    f = lambda ww: om.match_batch(ww, states, eps, 0.7, p, 3, grads=False)[0]
    _, _, _, g = om.match_batch(w, states, eps, 0.7, p, 3)
    h = 1e-6
    for net in w:
        for i, arr in enumerate(w[net]):
            for idx in [tuple(rng.integers(0, s) for s in arr.shape) for _ in range(3)]:
                wp = {k: [a.copy() for a in v] for k, v in w.items()}
                wm = {k: [a.copy() for a in v] for k, v in w.items()}
                wp[net][i][idx] += h
                wm[net][i][idx] -= h
                fd = (f(wp) - f(wm)) / (2 * h)
                assert abs(fd - g[net][i][idx]) <= 1e-6 * max(1.0, abs(fd)), (net, i, idx, fd, g[net][i][idx])


def _central_difference_check(w, f, g, rng, h=1e-6, per_array=3):
    for net in w:
        for i, arr in enumerate(w[net]):
            for idx in [tuple(rng.integers(0, s) for s in arr.shape) for _ in range(per_array)]:
                wp = {k: [a.copy() for a in v] for k, v in w.items()}
                wm = {k: [a.copy() for a in v] for k, v in w.items()}
                wp[net][i][idx] += h
                wm[net][i][idx] -= h
                fd = (f(wp) - f(wm)) / (2 * h)
                assert abs(fd - g[net][i][idx]) <= 1e-6 * max(1.0, abs(fd)), (net, i, idx, fd, g[net][i][idx], "bound 1e-6")


# the loss options the constructor accepts: similarity, temperature, reference state, hidden activation (leaky_relu 0.2,
# relu 0, linear 1), each away from the notebook's default
OPTIONS = {
    "l1": dict(similarity="l1"),
    "cosine": dict(similarity="cosine"),
    "temperature0.5": dict(temperature=0.5),
    "l2sq_temperature3": dict(similarity="l2sq", temperature=3.0),
    "reference_timestep2": dict(reference_timestep=2),
    "reference_timestep-1": dict(reference_timestep=-1),
    "relu": dict(slope=0.0),
    "linear": dict(slope=1.0),
    "cosine_relu_ref1": dict(similarity="cosine", slope=0.0, reference_timestep=1, temperature=0.7),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_oracle_gradients_over_the_loss_options_agree_with_central_differences(name):
    kw = OPTIONS[name]
    rng = np.random.default_rng(1)
    w = _tiny(rng)
    states = rng.uniform(-1, 1, (4, 3, 1))
    eps = rng.standard_normal((12, 2))
    f = lambda ww: om.match_batch(ww, states, eps, 0.7, 2.0, 3, grads=False, **kw)[0]
    _, _, _, g = om.match_batch(w, states, eps, 0.7, 2.0, 3, **kw)
    _central_difference_check(w, f, g, rng)


def test_oracle_options_change_the_loss():
    """each option reaches the loss (a parameter the restatement dropped would pass the difference check above)"""
    rng = np.random.default_rng(1)
    w = _tiny(rng)
    states = rng.uniform(-1, 1, (4, 3, 1))
    eps = rng.standard_normal((12, 2))
    base = om.match_batch(w, states, eps, 0.7, 2.0, 3, grads=False)[0]
    for kw in OPTIONS.values():
        assert abs(om.match_batch(w, states, eps, 0.7, 2.0, 3, grads=False, **kw)[0] - base) > 1e-6, kw
    # NumPy indexing: -1 is the last state of the sequence
    last = om.match_batch(w, states, eps, 0.7, 2.0, 3, grads=False, reference_timestep=2)[0]
    assert om.match_batch(w, states, eps, 0.7, 2.0, 3, grads=False, reference_timestep=-1)[0] == last


@pytest.mark.parametrize("ref", [3, 4, 100, -4, -5])
def test_reference_timestep_outside_the_sequence_is_refused(ref):
    """states_batch[:, reference_timestep] for L = 3 accepts -3 .. 2; anything else read a state of the next sequence or past
    the trajectory.  Validated before the device check, so this runs without a GPU."""
    with pytest.raises(ValueError, match="reference_timestep"):
        measurement.MeasurementIB(1, number_states=3, reference_timestep=ref)


def test_beta_schedule_is_the_notebook_formula():
    for step, n in [(0, 20_000), (1, 20_000), (9_999, 20_000), (19_999, 20_000), (25_000, 20_000), (3, 30)]:
        want = np.exp(np.log(10) + min(float(step) / n, 1.) * (np.log(1e-4) - np.log(10)))
        assert measurement.beta_schedule(step, n, 10, 1e-4) == float(np.float32(want))
    assert measurement.beta_schedule(0, 100, 10, 1e-4) == pytest.approx(10.0)


def test_sequence_indices_and_majority_rule():
    starts = np.array([0, 5, 17])
    idx = measurement.sequence_indices(starts, 4)
    assert idx.tolist() == [[0, 1, 2, 3], [5, 6, 7, 8], [17, 18, 19, 20]]
    # A = 2: 51 of 100 draws on symbol 1 -> 1, exactly 50 -> 0 (mean 0.5 is not > 0.5)
    a = np.zeros((100, 3), dtype=np.int64)
    a[:51, 0] = 1
    a[:50, 1] = 1
    a[:, 2] = 1
    assert measurement.majority_symbols(a).tolist() == [1, 0, 1]
    # A = 4: the reference's rule is the mean symbol index, not a vote (30 draws of symbol 2 already give mean 0.6)
    b = np.zeros((100, 3), dtype=np.int64)
    b[:30, 0] = 2
    b[:25, 1] = 2
    b[:17, 2] = 3
    assert measurement.majority_symbols(b).tolist() == [1, 0, 1]


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dib_measure.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(dib_\w+)\(", hdr, re.M))
    assert declared == set(_lib.SIGNATURES_MEASURE), declared ^ set(_lib.SIGNATURES_MEASURE)
    assert {"dib_measure_fwd", "dib_measure_bwd", "dib_measure_symbolize", "dib_measure_supported"} <= declared
    assert _lib.ABI_VERSION == 7
    assert re.search(r"#define DIB_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "dib_hip.h")).read())
    assert dib_amd.MeasurementIB is measurement.MeasurementIB


def test_product_raises_without_the_kernels():
    """no CPU fallback: without a GPU the constructor raises; with one, a shape outside the envelope does"""
    with pytest.raises((RuntimeError, ValueError)):
        measurement.MeasurementIB(2, information_bottleneck_embedding_dimension=64)
