"""Host side of the random partitions (dib_amd.random_partition, Chaos_experiments.ipynb cells 7-8), no GPU: the float64
oracle's tie rule, draw_weights' distributions, the survey's loop / skip rule / files with the kernel call replaced by the
oracle, the CTW thread bound, and the logistic map's generating partition as a known answer for the whole characterisation."""
import os

import numpy as np
import pytest

import _oracle_random_partition as orp
from dib_amd import chaos_data, ctw, measurement, random_partition as rp

H_LOGISTIC = 0.5203   # the notebook's entropy_rate_dict['logistic']


def test_oracle_argmax_of_magnitude_first_index_wins():
    lg = np.array([[0.0, 0.0, 0.0],       # all zero -> 0
                   [1.0, -1.0, 0.5],      # |1| = |-1| -> the lower index
                   [0.2, -3.0, 2.0],      # magnitude, not sign: 1 (the signed argmax is 2)
                   [-2.0, 2.0, 2.0],      # three-way tie -> 0
                   [0.1, 0.3, -0.3]])     # tie at 1 and 2 -> 1
    assert orp.symbols(lg).tolist() == [0, 0, 1, 0, 1]
    assert orp.symbols(lg).dtype == np.uint8
    np.testing.assert_allclose(orp.margin(lg), [0.0, 0.0, 1.0, 0.0, 0.0])


@pytest.mark.parametrize("d,A,N", [(2, 4, 3), (1, 2, 1), (4, 16, 2)])
def test_draw_weights_shapes_and_keras_layout(d, A, N):
    w = rp.draw_weights(d, A, N, seed=1)
    dims = [d] + [64] * N + [A]
    assert len(w) == 2 * (N + 1)
    for l, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        assert w[2 * l].shape == (i, o) and w[2 * l + 1].shape == (o,)
        assert w[2 * l].dtype == np.float32 and w[2 * l + 1].dtype == np.float32
    assert not w[-1].any(), "the output bias is zero (Keras default)"
    assert np.array_equal(rp.draw_weights(d, A, N, seed=1)[0], w[0]), "seeded draws repeat"
    assert not np.array_equal(rp.draw_weights(d, A, N, seed=2)[0], w[0])


def test_draw_weights_moments_over_many_seeds():
    hid, bias, out = [], [], []
    for s in range(200):
        w = rp.draw_weights(2, 4, 2, seed=s)
        hid += [w[0].ravel(), w[2].ravel()]
        bias += [w[1], w[3]]
        out.append(w[4].ravel())
    hid, bias, out = np.concatenate(hid), np.concatenate(bias), np.concatenate(out)
    # N(0.05, 0.5^2): 845 800 kernel and 25 600 bias samples - 5 standard errors
    for v in (hid, bias):
        se = 0.5 / np.sqrt(v.size)
        assert abs(v.mean() - 0.05) < 5 * se, v.mean()
        assert abs(v.std() - 0.5) < 5 * 0.5 / np.sqrt(2 * v.size), v.std()
    lim = np.sqrt(6.0 / (64 + 4))
    assert np.abs(out).max() <= lim and np.abs(out).max() > 0.99 * lim, "glorot-uniform limit sqrt(6 / (fan_in + A))"
    assert abs(out.mean()) < 5 * lim / np.sqrt(3 * out.size)
    assert abs(out.var() - lim ** 2 / 3) < 0.02 * lim ** 2 / 3


def test_entropy_from_counts_equals_compute_entropy():
    rng = np.random.default_rng(0)
    s = rng.choice(4, 10_000, p=[0.5, 0.3, 0.2, 0.0]).astype(np.uint8)
    assert rp.entropy_from_counts(np.bincount(s, minlength=4)) == orp.compute_entropy(s)
    from dib_amd import utils
    assert rp.entropy_from_counts(np.bincount(s, minlength=4)) == utils.compute_entropy(s)


# ---- the CTW thread bound --------------------------------------------------------------------------------------------------
def test_ctw_threads_is_bounded(monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    assert rp.ctw_threads() == 4
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert rp.ctw_threads() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert rp.ctw_threads() == min(16, len(os.sched_getaffinity(0)))


def test_characterize_partition_passes_threads_and_keeps_its_default(monkeypatch):
    seen = []
    real = ctw.estimate_entropy_batch

    def spy(seqs, A, threads=0):
        seen.append(threads)
        return real(seqs, A, threads=threads)
    monkeypatch.setattr(ctw, "estimate_entropy_batch", spy)
    s = (np.random.default_rng(0).random(20_000) < 0.4).astype(np.uint8)
    a = measurement.characterize_partition(s, 2, number_data_points=[500, 1000, 4000], number_rand_draws=3)
    b = measurement.characterize_partition(s, 2, number_data_points=[500, 1000, 4000], number_rand_draws=3, threads=3)
    assert seen == [0, 3], "default: all hardware threads, as before"
    assert a["entropy_rate"] == b["entropy_rate"] and np.array_equal(a["entropy_rate_values"], b["entropy_rate_values"])
    assert sorted(a) == ["entropy_rate", "entropy_rate_err", "entropy_rate_values", "entropy_single_timestep",
                         "number_data_points"]


# ---- the survey (cell 7) with the kernel replaced by the oracle ------------------------------------------------------------
@pytest.fixture()
def oracle_survey(monkeypatch):
    calls = []

    def symbolize(weights, activation, trajectory, cache):
        s = orp.symbols(orp.forward(weights, trajectory, activation))
        calls.append((len(weights) // 2 - 1, weights[-1].shape[0], activation))
        return s, np.bincount(s, minlength=weights[-1].shape[0])
    monkeypatch.setattr(rp, "_symbolize_partition", symbolize)
    threads = []
    real = measurement.entropy_rate_fit

    def fit(*a, **k):
        threads.append(k.get("threads"))
        return real(*a, **k)
    monkeypatch.setattr(measurement, "entropy_rate_fit", fit)
    return calls, threads


def _cell8_loader(out_dir, repeats, alphabet_sizes=(2, 4), layer_counts=(1, 2, 3), activations=("tanh", "relu")):
    """cell 8's reading loop, restated: the files it finds and the three values it plots"""
    got = []
    for rand_iter in range(repeats):
        for A in alphabet_sizes:
            for N in layer_counts:
                for act in activations:
                    f = os.path.join(out_dir, f"{N}layers_{act}_{A}alphabet_{rand_iter}.npz")
                    if not os.path.exists(f):
                        continue
                    z = np.load(f, allow_pickle=True)
                    got.append(((rand_iter, A, N, act), float(z["entropy_single_timestep"]), float(z["entropy_rate"]),
                                float(z["entropy_rate_err"])))
    return got


def test_survey_loop_order_skip_rule_and_files(oracle_survey, tmp_path, monkeypatch):
    calls, threads = oracle_survey
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    traj = chaos_data.generate_data("ikeda", 30_000, 1000, seed=0)
    ndp = [400, 1000, 3000, 8000]
    th = 0.9   # above some of the partitions' H(U): both branches run
    recs = rp.random_partition_survey(traj, number_random_repeats=2, seed=5, entropy_threshold=th, number_data_points=ndp,
                                      number_rand_draws=3, out_dir=str(tmp_path))
    order = [(r["rand_iter"], r["alphabet_size"], r["number_mlp_layers"], r["activation"]) for r in recs]
    assert order == [(i, A, N, act) for i in range(2) for A in (2, 4) for N in (1, 2, 3) for act in ("tanh", "relu")]
    assert calls == [(N, A, act) for _ in range(2) for A in (2, 4) for N in (1, 2, 3) for act in ("tanh", "relu")]
    skipped = [r for r in recs if r["skipped"]]
    kept = [r for r in recs if not r["skipped"]]
    assert skipped and kept, [r["entropy_single_timestep"] for r in recs]
    for r in recs:
        assert r["skipped"] == (r["entropy_single_timestep"] < th)
        w = rp.draw_weights(2, r["alphabet_size"], r["number_mlp_layers"], seed=r["seed"])
        assert r["entropy_single_timestep"] == orp.compute_entropy(orp.symbols(orp.forward(w, traj, r["activation"])))
    assert threads == [3] * len(kept), "the survey passes the bounded CTW thread count"
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"{r['number_mlp_layers']}layers_{r['activation']}_{r['alphabet_size']}alphabet_{r['rand_iter']}.npz"
                           for r in kept)
    for r in kept:
        z = np.load(r["file"])
        assert sorted(z.files) == ["entropy_rate", "entropy_rate_err", "entropy_rate_values", "entropy_single_timestep"]
        assert z["entropy_rate_values"].shape == (len(ndp), 3)
        assert float(z["entropy_rate"]) == r["entropy_rate"]
    loaded = _cell8_loader(str(tmp_path), 2)
    assert [k for k, *_ in loaded] == [(r["rand_iter"], r["alphabet_size"], r["number_mlp_layers"], r["activation"]) for r in kept]
    assert [v[1:] for v in loaded] == [(r["entropy_single_timestep"], r["entropy_rate"], r["entropy_rate_err"]) for r in kept]


def test_survey_point_assignments(oracle_survey, tmp_path):
    traj = chaos_data.generate_data("ikeda", 70_000, 1000, seed=1)
    recs = rp.random_partition_survey(traj, alphabet_sizes=(4,), layer_counts=(2,), activations=("relu",), entropy_threshold=0.0,
                                      number_data_points=[500, 1000, 2000, 4000], number_rand_draws=2, out_dir=str(tmp_path),
                                      save_point_assignments=True)
    z = np.load(recs[0]["file"])
    assert sorted(z.files) == ["entropy_rate", "entropy_rate_err", "entropy_rate_values", "entropy_single_timestep",
                               "raw_data_points", "symbolic_sequence"]
    assert np.array_equal(z["raw_data_points"], traj[:64_000])
    w = rp.draw_weights(2, 4, 2, seed=recs[0]["seed"])
    assert np.array_equal(z["symbolic_sequence"], orp.symbols(orp.forward(w, traj[:64_000], "relu")))


def test_partition_seeds_differ_across_the_grid():
    seeds = {rp.partition_seed(0, i, A, N, act) for i in range(20) for A in (2, 4) for N in (1, 2, 3) for act in ("tanh", "relu")}
    assert len(seeds) == 240


# ---- known answer: the logistic map's generating partition ----------------------------------------------------------------
def test_logistic_generating_partition_entropy_rate():
    """r = 3.7115, 2e6 points, h0 = x - 0.5, o = (1 + h0, 1 - h0): symbol 0 iff x > 0.5.  Calibrated on the host: over three
    initial conditions and four window seeds the fit gave 0.5192 .. 0.5207 (window lengths 2e3 .. 1e6, the trajectory being
    2e6 long), so the bound is 0.003 bits around the notebook's 0.5203."""
    x = orp.logistic_trajectory(2_000_000)
    w = orp.generating_partition_weights()
    s = orp.symbols(orp.forward(w, x, "linear"))
    assert np.array_equal(s, (x[:, 0] <= 0.5).astype(np.uint8))
    ndp = np.logspace(np.log10(2000), np.log10(1_000_000), 15, dtype=np.int32)
    r = measurement.characterize_partition(s, 2, number_data_points=ndp, threads=rp.ctw_threads())
    assert abs(r["entropy_rate"] - H_LOGISTIC) <= 0.003, r["entropy_rate"]
    assert r["entropy_rate"] <= r["entropy_single_timestep"]
