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
