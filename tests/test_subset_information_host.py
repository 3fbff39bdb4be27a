"""dib_amd.subset_information on the CPU (backend="host", float64 NumPy): the exhaustive I(X_S;Y) of every subset against the
notebook's own numbers (tests/golden/subset_mi.npz: cell 7's statements executed), the Shapley values against the oracle's loop,
known answers (parity, y = x_j, constant y), the pinned tie order of by_size / rank, circuit.subset_comparison, multi-bit
features against a brute-force np.unique restatement, the refusals and the logistic-regression baseline."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import dib_oracle as orc  # noqa: E402
import dib_amd  # noqa: E402
from dib_amd import circuit  # noqa: E402
from dib_amd import subset_information as si  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "subset_mi.npz")
# tests/test_oracle_golden.py _SI_PRINTED: the accuracies the notebook printed for the six SI circuits
SI_ACCURACY = [0.500, 0.750, 0.875, 0.625, 0.938, 0.500]


def _cube(n):
    """[2^n, n] 0/1 rows, row r = the bits of r (bit f in column f)"""
    return (np.arange(1 << n)[:, None] >> np.arange(n)) & 1


def test_paper_circuit_matches_the_notebooks_all_mis():
    fx = np.load(GOLDEN)
    tt = fx["truth_table"]
    info = si.subset_information(tt[:, :10], tt[:, 10], backend="host")
    assert info.number_features == 10 and info.bits.shape == (1024,) and info.bits.dtype == np.float64
    masks = si.subset_masks(fx["all_on_off_combos"])
    assert sorted(masks.tolist()) == list(range(1024))
    assert np.abs(info.bits[masks] - fx["all_mis_bits"]).max() <= 1e-12
    assert abs(info.entropy_y_bits - float(fx["entropy_y_bits"])) <= 1e-12
    assert info.bits[0] == 0.0
    # the +-1 floats of data.fetch_boolean_circuit are the same table
    d = dib_amd.data.fetch_boolean_circuit()
    again = si.subset_information(d["x_train"], d["y_train"], backend="host")
    assert np.array_equal(again.bits, info.bits)
    assert info.ceiling(1023) == info.bits[1023] and info.ceiling([2, 9]) == info.bits[(1 << 2) | (1 << 9)]


def test_subset_masks_in_both_meshgrid_orders():
    for indexing in ("xy", "ij"):
        combos = np.reshape(np.stack(np.meshgrid(*[[0, 1]] * 4, indexing=indexing), -1), [-1, 4])
        masks = si.subset_masks(combos)
        assert sorted(masks.tolist()) == list(range(16))
        for c, m in zip(combos, masks):
            assert [f for f in range(4) if m >> f & 1] == np.where(c)[0].tolist()
    with pytest.raises(ValueError):
        si.subset_masks([[0, 2]])


@pytest.mark.parametrize("k", range(6))
def test_shapley_values_of_the_si_circuits_match_the_oracle(k):
    table = circuit.truth_table(circuit.SI_CIRCUITS[k])
    G = table.shape[1] - 1
    info = si.subset_information(table[:, :G], table[:, -1], backend="host")
    want = orc.shapley_values_bits(2 * table[:, :G] - 1, table[:, -1].astype(np.int64))
    got = info.shapley_values()
    assert got.shape == (G,) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12
    assert abs(got.sum() - info.entropy_y_bits) <= 1e-12   # deterministic circuit: the values share out all of H(Y)


def test_known_answers_are_exact():
    n = 6
    x = _cube(n)
    for inputs in ([0, 1, 2, 3, 4, 5], [1, 4], [0, 2, 5]):
        y = x[:, inputs].sum(1) & 1
        need = sum(1 << i for i in inputs)
        bits = si.subset_information(x, y, backend="host").bits
        for m in range(1 << n):
            assert bits[m] == (1.0 if m & need == need else 0.0), (inputs, m, bits[m])
    for j in (0, 3):
        bits = si.subset_information(x, x[:, j], backend="host").bits
        assert all(bits[m] == float(m >> j & 1) for m in range(1 << n))
    const = si.subset_information(x, np.zeros(1 << n, dtype=np.int64), backend="host")
    assert (const.bits == 0.0).all() and const.entropy_y_bits == 0.0
    ones = si.subset_information(x, np.ones(1 << n, dtype=np.int64), backend="host")   # class 0 is empty
    assert (ones.bits == 0.0).all()


def test_tie_order_of_by_size_and_rank_is_pinned():
    """y = x0 XOR x1 on 3 inputs: singles all carry 0 bits, pairs {0,1} 1 bit and the others 0 - ties go by ascending mask"""
    x = _cube(3)
    info = si.subset_information(x, x[:, 0] ^ x[:, 1], backend="host")
    m1, b1 = info.by_size(1)
    assert m1.tolist() == [1, 2, 4] and b1.tolist() == [0.0, 0.0, 0.0]
    m2, b2 = info.by_size(2)
    assert m2.tolist() == [3, 5, 6] and b2.tolist() == [1.0, 0.0, 0.0]
    assert [info.rank(m) for m in (1, 2, 4)] == [0, 1, 2]
    assert info.rank([0, 1]) == 0 and info.rank([0, 2]) == 1 and info.rank([1, 2]) == 2 and info.rank(6) == 2
    assert info.by_size(0)[0].tolist() == [0] and info.rank(0) == 0 and info.rank(7) == 0
    # a strict order: y = x2 on 3 inputs, pairs with gate 2 first
    info = si.subset_information(x, x[:, 2], backend="host")
    assert info.by_size(2)[0].tolist() == [5, 6, 3] and info.by_size(1)[0].tolist() == [4, 1, 2]
    with pytest.raises(ValueError):
        info.rank(8)
    with pytest.raises(ValueError):
        info.rank([3])


def test_subset_comparison_on_a_crafted_curve():
    """y = x2 OR (x0 AND x1): crafted per-gate curves drop gate 0 first, then gate 2 (a poor choice: {1} is the worst single)"""
    x = _cube(3)
    y = x[:, 2] | (x[:, 0] & x[:, 1])
    table = np.concatenate([x, y[:, None]], 1)
    parts = np.array([[1.0, 1.0, 1.0], [0.05, 1.0, 1.0], [0.05, 0.9, 0.05], [0.05, 0.01, 0.05]])
    rows = circuit.subset_comparison(parts, table, backend="host")
    info = si.subset_information(x, y, backend="host")
    assert [r["gates"] for r in rows] == [[1, 2], [1], [], [0, 1, 2]]
    assert [r["mask"] for r in rows] == [6, 2, 0, 7] and [r["size"] for r in rows] == [2, 1, 0, 3]
    # pairs: {0,2} and {1,2} tie (ascending mask: 5 before 6), {0,1} is last; singles: gate 2, then 0 and 1 tie
    assert info.by_size(2)[0].tolist() == [5, 6, 3] and info.by_size(1)[0].tolist() == [4, 1, 2]
    assert [r["rank"] for r in rows] == [1, 2, 0, 0]
    for r in rows:
        assert r["information_bits"] == info.bits[r["mask"]] and r["best_bits_of_size"] == info.by_size(r["size"])[1][0]
    assert rows[-1]["information_bits"] == pytest.approx(info.entropy_y_bits, abs=1e-12)


def _brute(x, y, fb):
    """I(X_S;Y) by np.unique over the selected columns, every subset"""
    n = len(y)
    ent = lambda c: float(-(c / n * np.log2(c / n)).sum())
    hy = ent(np.unique(y, return_counts=True)[1])
    out = np.zeros(1 << len(fb))
    for m in range(1, 1 << len(fb)):
        cols = [f for f in range(len(fb)) if m >> f & 1]
        hx = ent(np.unique(x[:, cols], axis=0, return_counts=True)[1])
        hxy = ent(np.unique(np.concatenate([x[:, cols], y[:, None]], 1), axis=0, return_counts=True)[1])
        out[m] = hx + hy - hxy
    return out, hy


def test_multi_bit_features_match_a_brute_force_restatement():
    rng = np.random.default_rng(5)
    fb = [2, 1, 3]
    x = np.stack([rng.integers(0, 1 << b, 300) for b in fb], 1)
    y = (x[:, 0] + x[:, 2] + rng.integers(0, 2, 300)) % 3
    info = si.subset_information(x, y, feature_bits=fb, backend="host")
    want, hy = _brute(x, y, fb)
    assert info.number_features == 3 and np.abs(info.bits - want).max() <= 1e-12 and abs(info.entropy_y_bits - hy) <= 1e-12
    # an [N, 1] y is the same sample
    assert np.array_equal(si.subset_information(x, y[:, None], feature_bits=fb, backend="host").bits, info.bits)


def test_refusals():
    x = np.zeros((4, 21))
    with pytest.raises(ValueError, match="20 bits"):
        si.subset_information(x, np.zeros(4), backend="host")
    with pytest.raises(ValueError, match="20 bits"):
        si.subset_information(np.zeros((4, 3), dtype=np.int64), np.zeros(4), feature_bits=[7, 7, 7], backend="host")
    with pytest.raises(ValueError, match="outside its 2-bit field"):
        si.subset_information(np.array([[0, 1], [4, 0]]), np.array([0, 1]), feature_bits=[2, 1], backend="host")
    with pytest.raises(ValueError, match="outside its 1-bit field"):
        si.subset_information(np.array([[0, -1], [1, 0]]), np.array([0, 1]), feature_bits=[2, 1], backend="host")
    with pytest.raises(ValueError, match=r"y is \[N\] or \[N, 1\]"):
        si.subset_information(np.zeros((4, 2)), np.zeros((4, 1, 1)), backend="host")
    with pytest.raises(ValueError, match="classes"):
        si.subset_information(np.zeros((4, 2)), np.array([0, 1, 2, 16]), backend="host")
    with pytest.raises(ValueError, match="backend"):
        si.subset_information(np.zeros((4, 2)), np.zeros(4), backend="numpy")


@pytest.mark.parametrize("k", range(6))
def test_logistic_baseline_reproduces_the_printed_accuracies(k):
    table = circuit.truth_table(circuit.SI_CIRCUITS[k])
    r = si.logistic_regression_baseline(table)
    assert f"{r['accuracy']:.3f}" == f"{SI_ACCURACY[k]:.3f}"
    assert r["coefficients"].shape == (table.shape[1] - 1,)
    hy = si.subset_information(table[:, :-1], table[:, -1], backend="host").entropy_y_bits
    assert -1e-9 <= r["information_bits"] <= hy + 1e-9   # the maximum-likelihood fit is no worse than the class prior


def test_save_writes_the_npz_and_the_figure(tmp_path):
    table = circuit.truth_table(circuit.SI_CIRCUITS[2])
    info = si.subset_information(table[:, :-1], table[:, -1], backend="host")
    path = si.save_subset_information(info, str(tmp_path), selected=[[0, 1, 2, 3], [1, 3], [1]])
    z = np.load(path)
    assert np.array_equal(z["bits"], info.bits) and z["masks"].tolist() == list(range(16))
    assert float(z["entropy_y_bits"]) == info.entropy_y_bits and np.array_equal(z["shapley_values"], info.shapley_values())
    assert os.path.getsize(os.path.join(str(tmp_path), "subset_information.png")) > 1000
