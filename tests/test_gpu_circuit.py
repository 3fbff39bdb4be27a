"""The Boolean-circuit model (InfoDecomp_Boolean_circuits.ipynb cells 4-7) on the device against the float64 oracle
(tests/_oracle_circuit.py) with the same Philox draws: drawn rows, noise and embeddings; BCE, KL and every gradient for the
paper circuit and the six SI circuits at four batch sizes; a 30-step Adam loop through the beta ramp; the one-launch
sandwich bounds against the notebook's compute_batch and the per-gate dib_mi_sandwich_rows loop; determinism; the envelope;
and the paper's Fig. 1 run."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import _oracle_circuit as oc
from dib_amd import _lib, circuit, utils
from dib_amd._gemm_plan import _ptr
from dib_amd.circuit import CircuitIB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCUITS = {"paper": circuit.PAPER_CIRCUIT, **{f"si_{'abcdef'[k]}": s for k, s in enumerate(circuit.SI_CIRCUITS)}}


def _oracle_params(m):
    w = [np.asarray(a, dtype=np.float64) for a in m.predictive_model.get_weights()]
    s = np.array([e.get_weights()[0][0, 0] for e in m.feature_encoders], dtype=np.float64)
    lv = np.array([e.get_weights()[1][0, 0] for e in m.feature_encoders], dtype=np.float64)
    return oc.Params(w, s, lv)


def _device_grads(m):
    g = m.grads.cpu().numpy().astype(np.float64)
    out = []
    for l, (i, o) in enumerate(m.dims):
        k = g[m.w_off[l]: m.w_off[l] + i * o].reshape(i, o)
        out += [k, g[m.b_off[l]: m.b_off[l] + o]]
    return out, g[m.sc_off: m.sc_off + m.G], g[m.sc_off + m.G: m.sc_off + 2 * m.G]


def _perturb(m, seed):
    """scalars away from the initial (1, -3) so that both terms of each scalar gradient matter"""
    rng = np.random.default_rng(seed)
    for e in m.feature_encoders:
        e.set_weights([np.float32([[rng.uniform(0.3, 1.5)]]), np.float32([[rng.uniform(-3.0, 0.5)]])])


def test_drawn_rows_eps_and_u_match_oracle():
    G, B, seed = 10, 512, 7
    m = CircuitIB(G, noise_seed=seed, init_seed=1)
    _perturb(m, 0)
    table = circuit.truth_table(circuit.PAPER_CIRCUIT)
    p = _oracle_params(m)
    for step in range(3):
        p = _oracle_params(m)
        m.train_step(table, 0.1, batch_size=B)
        v = m.last_step(B)
        rows = oc.draw_rows(seed, step, B, G)
        assert np.array_equal(v["rows"].cpu().numpy(), rows), step
        e = oc.eps(seed, step, B, G)
        u = v["u"].cpu().numpy().astype(np.float64)
        x = 2.0 * table[rows, :G] - 1.0
        assert np.abs(u[:, :G] - (x * p.s + np.exp(p.lv / 2) * e)).max() < 2e-5 * np.abs(e).max()
        assert np.all(u[:, G:] == 0.0)
        assert np.array_equal(v["y"].cpu().numpy(), table[rows, -1].astype(np.float32))
    # the draw is uniform with replacement over the 1024 rows: every row of a 2^10 table turns up within 3 x 512 draws often
    assert len(np.unique(np.concatenate([oc.draw_rows(seed, s, B, G) for s in range(3)]))) > 700


@pytest.mark.parametrize("B", [1, 17, 512, 2048])
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_step_bce_kl_and_all_gradients_match_oracle(name, B):
    spec = CIRCUITS[name]
    table = circuit.truth_table(spec)
    G = table.shape[1] - 1
    seed, beta = 3, 0.37
    m = CircuitIB(G, noise_seed=seed, init_seed=2)
    _perturb(m, B)
    m.step = 11
    p = _oracle_params(m)
    lib = m.lib
    n0 = lib.dib_launch_count()
    bce = m.train_step(table, beta, batch_size=B)
    launches = lib.dib_launch_count() - n0
    torch.cuda.synchronize()
    bf = m._bufs[B]
    assert lib.dib_mlp_small_head_supported(ctypes.byref(m._desc), B) == 1
    # the row-tile head kernel ran: the step is exactly fwd, head, grouped wgrad, bwd, reduce + Adam
    assert launches == 5, launches
    assert (bf["nsplit"] > 1) == (B >= 128)
    ref = oc.step(p, table, oc.draw_rows(seed, 11, B, G), oc.eps(seed, 11, B, G), beta)
    v = m.last_step(B)
    assert abs(float(bce) - ref["bce"]) < 2e-5 * (1 + ref["bce"])
    kl = v["kl"].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(kl[:G], ref["kl"], rtol=1e-5, atol=1e-6)
    assert abs(kl[G] - beta * ref["kl"].sum()) < 1e-5 * (1 + beta * ref["kl"].sum())
    np.testing.assert_allclose(v["pred"].cpu().numpy(), ref["logit"], rtol=0, atol=2e-4 * (1 + np.abs(ref["logit"]).max()))
    w, ds, dlv = _device_grads(m)
    for l, (gd, gr, mag, top) in enumerate(zip(w, ref["grads"].weights, ref["grad_magnitudes"], ref["grad_max_terms"])):
        if l == 0:
            assert np.all(gd[G:] == 0.0)        # the pad rows of the first kernel get no gradient
            gd = gd[:G]
        # fp32 against float64: relative to the largest gradient, plus the summation-order scale of the batch sums.  A hidden
        # pre-activation within fp32 rounding of 0 takes the other leaky-ReLU slope on one side; that row then moves the
        # entries it touches by at most one batch term.  Among the 2^19 - 2^20 pre-activations of the large batches this
        # happens in most steps, so there every entry may also differ by its largest batch term (the small batches: never seen)
        err, scale = np.abs(gd - gr), np.abs(gr).max() + 1e-6
        tol = 3e-4 * scale + 1e-5 * mag + (top if B >= 512 else 0.0)
        assert np.all(err <= tol), (l, err.max(), scale)
    for gd, gr in ((ds, ref["grads"].s), (dlv, ref["grads"].lv)):
        assert np.abs(gd - gr).max() < 3e-4 * (np.abs(gr).max() + 1e-6), (gd, gr)


def test_thirty_adam_steps_through_the_beta_ramp_match_oracle():
    spec = circuit.SI_CIRCUITS[4]
    table = circuit.truth_table(spec)
    G, B, n, seed = table.shape[1] - 1, 96, 30, 5
    m = CircuitIB(G, predictive_arch_spec=(64, 64, 64), noise_seed=seed, init_seed=4)
    m.set_lr(1e-2)
    p = _oracle_params(m)
    st = oc.adam_init(p)
    for step in range(n):
        beta = circuit.beta_schedule(step, n, 1e-3, 5.0)
        m.train_step(table, beta, batch_size=B)
        r = oc.step(p, table, oc.draw_rows(seed, step, B, G), oc.eps(seed, step, B, G), beta)
        oc.adam(p, r["grads"], st, lr=1e-2)
    q = _oracle_params(m)
    for a, b in zip(q.tensors(), p.tensors()):
        err = np.abs(a - b)
        assert err.max() < 2e-3, err.max()
        assert np.mean(err < 1e-4) > 0.98, np.mean(err < 1e-4)
    np.testing.assert_allclose(q.s, p.s, rtol=0, atol=1e-4)
    np.testing.assert_allclose(q.lv, p.lv, rtol=0, atol=1e-4)


def _rows_loop(m, x, seed):
    """[G, nb, 2]: dib_mi_sandwich_rows per gate and batch on the encoder output (feature = gate)"""
    nb, n = x.shape
    ws = torch.empty(int(m.lib.dib_mi_workspace_bytes(n, 1)) // 8 + 1, dtype=torch.float64, device=m.device)
    out = np.zeros((m.G, nb, 2))
    st = ctypes.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)
    for g, enc in enumerate(m.feature_encoders):
        for b in range(nb):
            e = enc(x[b][:, None]).contiguous()
            r = torch.empty((2, n), dtype=torch.float64, device=m.device)
            assert m.lib.dib_mi_sandwich_rows(_ptr(e), n, 1, seed, b, g, _ptr(r[0]), _ptr(r[1]), _ptr(ws), st) == 0
            out[g, b] = r.mean(dim=1).cpu().numpy()
    return out


def test_mi_bounds_match_compute_batch_and_the_per_gate_loop():
    G, n, nb, seed = 10, 1024, 8, 123
    m = CircuitIB(G)
    s = [1.0, 0.05, 0.3, 2.0, 0.0, 1e-3, 0.8, 0.5, 4.0, 0.2]
    lv = [-3.0, 0.0, -1.0, -12.0, -3.0, 1.0, -11.0, -0.5, -14.0, 2.0]     # three gates with lv < -10
    for g in range(G):
        m.feature_encoders[g].set_weights([np.float32([[s[g]]]), np.float32([[lv[g]]])])
    n0 = m.lib.dib_launch_count()
    dev = m.estimate_channel_mi_bounds(seed, n, nb, per_batch=True)
    assert m.lib.dib_launch_count() - n0 == 1
    assert np.isfinite(dev).all()
    rng = np.random.default_rng(seed)
    x = np.stack([np.array([-1.0, 1.0], np.float32)[rng.integers(0, 2, n)] for _ in range(nb)], 0)
    loop = _rows_loop(m, x, seed)
    tol = 1e-12 * np.abs(loop) + 1e-14
    assert np.all(np.abs(dev - loop) <= tol), np.abs(dev - loop).max()
    # the notebook's compute_batch in float64 on the same sampled u (the device's fp32 Box-Muller noise, dib_philox_normal_fill;
    # the draw itself is checked against the float64 generator here and in test_drawn_rows_eps_and_u_match_oracle)
    eps = torch.empty((n, G, 1), dtype=torch.float32, device="cuda")
    for b in range(nb):
        assert m.lib.dib_philox_normal_fill(_ptr(eps), None, 0, n, G, 1, seed, b, None) == 0
        e = eps.cpu().numpy()[:, :, 0].astype(np.float64)
        assert np.abs(e - np.stack([oc.orc.philox_normal(seed, b, np.arange(n), g, 1)[:, 0] for g in range(G)], -1)).max() < 1e-5
        for g in range(G):
            lo, up = oc.mi_bounds_batch(s[g], lv[g], x[b], e[:, g])
            if np.isfinite(lo) and np.isfinite(up):
                assert abs(dev[g, b, 0] - lo) < 1e-9 and abs(dev[g, b, 1] - up) < 1e-9, (g, b, dev[g, b], lo, up)
    # well separated channels carry the batch's empirical entropy of x (lower) / its leave-one-out form (upper), closed ones nothing
    for b in range(nb):
        n1 = int((x[b] > 0).sum())
        cnt = np.where(x[b] > 0, n1, n - n1).astype(np.float64)
        assert np.all(np.abs(dev[[3, 6, 8], b, 0] - np.mean(np.log(n / cnt))) < 1e-9)
        assert np.all(np.abs(dev[[3, 6, 8], b, 1] - np.mean(np.log(n / (cnt - 1)))) < 1e-9)   # compute_batch's mean over n
    assert np.all(np.abs(dev[4, :, 0]) < 1e-12) and np.all(np.abs(dev[4, :, 1] - np.log(n / (n - 1))) < 1e-12)
    # a second evaluation reuses the self-cleaning workspace and gives the same bits
    assert np.array_equal(m.estimate_channel_mi_bounds(seed, n, nb, per_batch=True), dev)


def test_utils_estimate_equals_fits_evaluation():
    table = circuit.truth_table(circuit.SI_CIRCUITS[5])
    G = table.shape[1] - 1
    m = CircuitIB(G, noise_seed=2, init_seed=2)
    h = m.fit(table, number_training_steps=1, batch_size=64, evaluate_mutual_info_freq=1, seed=9)
    assert h["mutual_information_bounds"].shape == (1, G, 2) and list(h["evaluation_steps"]) == [0]
    for g in range(G):
        est = utils.estimate_mi_sandwich_bounds(m.feature_encoders[g], [[-1.], [1.]], seed=circuit.evaluation_seed(9, 0))
        fitv = h["mutual_information_bounds"][0, g] * np.log(2)
        assert np.all(np.abs(est - fitv) <= 1e-12 * np.abs(est) + 1e-14), (g, est, fitv)


def test_two_fits_with_the_same_seeds_are_bit_identical():
    table = circuit.truth_table(circuit.PAPER_CIRCUIT)
    runs = []
    for _ in range(2):
        m = CircuitIB(10, noise_seed=1, init_seed=1)
        h = m.fit(table, number_training_steps=400, batch_size=512, evaluate_mutual_info_freq=100, seed=3)
        runs.append((h, m.params.cpu().numpy()))
    (h1, p1), (h2, p2) = runs
    assert np.array_equal(h1["bce_loss_series"], h2["bce_loss_series"])
    assert np.array_equal(h1["mutual_information_bounds"], h2["mutual_information_bounds"])
    assert np.array_equal(h1["beta"], h2["beta"]) and np.array_equal(p1, p2)
    assert h1["mutual_information_bounds"].shape == (4, 10, 2) and list(h1["evaluation_steps"]) == [0, 100, 200, 300]
    assert np.isfinite(h1["bce_loss_series"]).all() and h1["bce_loss_series"][-50:].mean() < h1["bce_loss_series"][:50].mean()


def test_refusals_launch_nothing():
    lib = _lib.load_library()
    n0 = lib.dib_launch_count()
    for G in (0, 17):
        with pytest.raises(ValueError):
            CircuitIB(G)
    m = CircuitIB(4)
    table = circuit.truth_table(circuit.SI_CIRCUITS[2])
    for B in (0, 2049):
        with pytest.raises(ValueError):
            m.train_step(table, 0.1, batch_size=B)
        with pytest.raises(ValueError):
            m.fit(table, number_training_steps=2, batch_size=B)
    with pytest.raises(ValueError):
        m.train_step(table[:-1], 0.1, batch_size=8)                             # not 2^G rows
    with pytest.raises(ValueError):
        m.train_step(circuit.truth_table(circuit.SI_CIRCUITS[0]), 0.1, batch_size=8)   # a table of another G
    with pytest.raises(ValueError):
        m.estimate_channel_mi_bounds(0, evaluation_batch_size=1)
    assert lib.dib_launch_count() == n0
    assert lib.dib_circuit_supported(16, 2048) == 1 and lib.dib_circuit_supported(17, 1) == 0
    assert lib.dib_circuit_supported(1, 0) == 0 and lib.dib_circuit_supported(1, 2049) == 0


def _drop_evaluations(info_in_parts, threshold=0.1):
    """per gate: the number of evaluations it stays in cell 7's cumulative selected set"""
    return np.cumprod(np.asarray(info_in_parts) > threshold, axis=0).sum(0)


def test_fig1_full_run_drops_the_gates_in_the_notebooks_group_order():
    """cell 6's configuration: 50 000 steps of 512 rows, beta 1e-3 -> 5, evaluations every 250 steps; seed 0"""
    spec = importlib.util.spec_from_file_location("paper_circuit_run", os.path.join(ROOT, "tools", "paper_circuit_run.py"))
    pcr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pcr)
    table = circuit.truth_table(circuit.PAPER_CIRCUIT)
    m = CircuitIB(10)
    h = m.fit(table, number_training_steps=50_000, batch_size=512, learning_rate=1e-3, beta_start=1e-3, beta_end=5.0, seed=0)
    assert h["mutual_information_bounds"].shape == (200, 10, 2)
    ip = circuit.information_plane(h, circuit.entropy_bits(table[:, -1]))
    seq = circuit.selected_subsets(ip["info_in_parts"])
    print("Sequence of selected subsets:", [list(map(int, s)) for s in seq[:-1]])
    drop = _drop_evaluations(ip["info_in_parts"])
    print("evaluations in the selected set per gate:", drop.tolist())
    # early in training every channel transmits (nearly 1 bit), at the end none does
    assert np.all(ip["info_in_parts"][5] > 0.1) and np.all(ip["info_in_parts"][-1] < 0.1)
    assert pcr.group_order_violations(drop, slack=1) == []
