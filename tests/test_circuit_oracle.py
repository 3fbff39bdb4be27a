"""CPU checks of the Boolean-circuit model's host side and of its float64 oracle (tests/_oracle_circuit.py): the oracle's
gradients against finite differences, the truth tables against the notebook's own fixture and the oracle, the beta ramp,
cells 6-7's read-out against numbers the notebook's own statements produced (tests/golden/circuit_selection.npz), and the
host-side refusals."""
import os

import numpy as np
import pytest

import _oracle_circuit as oc
import dib_oracle as orc
from dib_amd import circuit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _random_params(G, units, seed=0):
    rng = np.random.default_rng(seed)
    dims = [G] + list(units) + [1]
    w = []
    for i, o in zip(dims[:-1], dims[1:]):
        w += [rng.standard_normal((i, o)) * 0.5, rng.standard_normal(o) * 0.1]
    return oc.Params(w, rng.uniform(0.5, 1.5, G), rng.uniform(-3, 0, G))


@pytest.mark.parametrize("beta", [0.0, 0.7])
def test_oracle_gradients_match_finite_differences(beta):
    spec = circuit.SI_CIRCUITS[2]
    table = circuit.truth_table(spec)
    G = table.shape[1] - 1
    p = _random_params(G, (8, 8, 8))
    rows = oc.draw_rows(3, 5, 12, G)
    e = oc.eps(3, 5, 12, G)
    res = oc.step(p, table, rows, e, beta)
    h = 1e-6
    for t_idx, (t, gt) in enumerate(zip(p.tensors(), res["grads"].tensors())):
        flat, gflat = t.reshape(-1), gt.reshape(-1)
        for k in range(0, flat.size, max(1, flat.size // 7)):
            old = flat[k]
            flat[k] = old + h
            up = oc.step(p, table, rows, e, beta)["loss"]
            flat[k] = old - h
            dn = oc.step(p, table, rows, e, beta)["loss"]
            flat[k] = old
            assert abs((up - dn) / (2 * h) - gflat[k]) < 1e-6 * (1 + abs(gflat[k])), (t_idx, k)


def test_paper_truth_table_is_the_notebooks_bit_for_bit():
    g = np.load(os.path.join(GOLDEN, "subset_mi.npz"))
    t = circuit.truth_table(circuit.PAPER_CIRCUIT)
    assert t.shape == (1024, 11)
    assert np.array_equal(t, g["truth_table"].astype(np.int32))
    assert round(circuit.entropy_bits(t[:, -1]), 3) == 0.758
    assert abs(circuit.entropy_bits(t[:, -1]) - float(g["entropy_y_bits"])) < 1e-15
    assert circuit.PAPER_CIRCUIT == orc.PAPER_CIRCUIT


@pytest.mark.parametrize("k", range(6))
def test_si_truth_tables_equal_the_oracles(k):
    spec = circuit.SI_CIRCUITS[k]
    assert spec == orc.SI_CIRCUITS[k]
    G = circuit.number_input_gates(spec)
    assert 3 <= G <= 6
    t = circuit.truth_table(spec)
    x, y = orc.boolean_circuit_truth_table(spec, G)
    assert np.array_equal(t[:, :G], (x > 0).astype(np.int32)) and np.array_equal(t[:, -1], y)
    # the packed device words: bit g = input g, bit G = y
    w = circuit.pack_truth_table(t)
    for g in range(G + 1):
        assert np.array_equal((w >> g) & 1, t[:, g])


def test_beta_ramp_is_cell_6s_per_step_log_linear_float32():
    n = 50_000
    for b1 in (5.0, 1.0):
        betas = np.array([circuit.beta_schedule(s, n, 1e-3, b1) for s in range(0, n, 97)])
        ref = np.array([oc.beta_schedule(s, n, 1e-3, b1) for s in range(0, n, 97)])
        assert np.array_equal(betas, ref)
        assert betas[0] == np.float32(1e-3) and np.all(np.diff(betas) > 0)
        assert abs(circuit.beta_schedule(n - 1, n, 1e-3, b1) / b1 - 1) < 2e-4   # the last step stops one step short of beta_end
        assert betas.dtype == np.float64 and np.all(betas == betas.astype(np.float32))


def test_row_draw_rule_is_uniform_over_the_table():
    G = 10
    r = np.concatenate([oc.draw_rows(0, s, 2048, G) for s in range(20)])
    assert r.min() >= 0 and r.max() < 1 << G
    counts = np.bincount(r, minlength=1 << G)
    exp = r.size / (1 << G)
    chi2 = ((counts - exp) ** 2 / exp).sum()
    assert chi2 < (1 << G) + 5 * np.sqrt(2 * (1 << G))


def test_read_out_equals_the_notebooks_own_statements():
    g = np.load(os.path.join(GOLDEN, "circuit_selection.npz"))
    G, freq = 10, int(g["evaluate_mutual_info_freq"])
    history = {"mutual_information_bounds": g["bounds_nats"].reshape(-1, G, 2) / np.log(2), "bce_loss_series": g["bce_loss_series"],
               "evaluate_mutual_info_freq": freq}
    ip = circuit.information_plane(history, float(g["entropy_y_bits"]))
    np.testing.assert_allclose(ip["info_in_parts"], g["info_in_parts"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ip["info_in_full"], g["info_in_full"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ip["predictive_information_out"], g["predictive_information_out"], rtol=0, atol=1e-6)
    subsets = circuit.selected_subsets(ip["info_in_parts"])
    assert isinstance(subsets[-1], range) and list(subsets[-1]) == list(range(G))
    masks = g["selected_subset_masks"]
    assert len(subsets) - 1 == masks.shape[0] >= 5
    for s, m in zip(subsets[:-1], masks):
        assert list(s) == list(np.where(m)[0])
    # the oracle's restatement agrees
    parts, full, out = oc.information_plane(history["mutual_information_bounds"], g["bce_loss_series"], float(g["entropy_y_bits"]),
                                            freq)
    np.testing.assert_allclose(parts, ip["info_in_parts"], rtol=0, atol=1e-12)
    assert [list(s) for s in oc.selected_subsets(parts)] == [list(s) for s in subsets]


def test_host_refusals():
    t = circuit.truth_table(circuit.SI_CIRCUITS[0])
    with pytest.raises(ValueError):
        circuit.pack_truth_table(t[:-1])                 # not 2^G rows
    with pytest.raises(ValueError):
        circuit.pack_truth_table(np.zeros((1, 1), np.int32))   # G = 0
    with pytest.raises(ValueError):
        circuit.pack_truth_table(np.zeros((1 << 17, 18), np.int32))   # G = 17
    bad = t.copy()
    bad[0, 0] = 2
    with pytest.raises(ValueError):
        circuit.pack_truth_table(bad)
