"""CircuitEnsemble (R Boolean-circuit models in lockstep) on the device: every replica of a step against the float64 oracle
(tests/_oracle_circuit.py) with the tolerances of tests/test_gpu_circuit.py, thirty Adam steps through per-replica beta ramps,
R = 1 against CircuitIB bit for bit, isolation of the replicas, a launch count that does not depend on R, fit, to_model and the
argument errors."""
import numpy as np
import pytest
import torch

import _oracle_circuit as oc
from dib_amd import _lib, circuit
from dib_amd.circuit import CircuitEnsemble, CircuitIB

pytestmark = pytest.mark.gpu

SI_TABLES = [circuit.truth_table(s) for s in circuit.SI_CIRCUITS]
KEYS = {"bce_loss_series", "beta", "mutual_information_bounds", "evaluation_steps", "evaluate_mutual_info_freq"}


def _oracle_params(ens, r):
    w = ens.get_weights(r)
    return oc.Params([np.asarray(a, dtype=np.float64) for a in w["predictive_model"]], w["mu_scaling"], w["logvar"])


def _perturb(ens, seed):
    """scalars away from the initial (1, -3) so that both terms of each scalar gradient matter"""
    rng = np.random.default_rng(seed)
    for r, G in enumerate(ens.G):
        ens.set_weights(r, {"mu_scaling": rng.uniform(0.3, 1.5, G), "logvar": rng.uniform(-3.0, 0.5, G)})


def _device_grads(ens, r):
    g = ens.grads[r * ens.n_params: (r + 1) * ens.n_params].cpu().numpy().astype(np.float64)
    out, G = [], ens.G[r]
    for l, (i, o) in enumerate(ens.dims):
        out += [g[ens.w_off[l]: ens.w_off[l] + i * o].reshape(i, o), g[ens.b_off[l]: ens.b_off[l] + o]]
    return out, g[ens.sc_off: ens.sc_off + G], g[ens.sc_off + G: ens.sc_off + 2 * G]


@pytest.mark.parametrize("B", [17, 512])
def test_step_of_every_replica_matches_oracle(B):
    """the six SI circuits (G = 3 .. 6) in one ensemble, rows given: BCE, KL, logits and ALL gradients of every replica"""
    R, step0 = len(SI_TABLES), 11
    seeds, betas = [3 + 5 * r for r in range(R)], [0.37 + 0.1 * r for r in range(R)]
    ens = CircuitEnsemble(SI_TABLES, init_seeds=[2 + r for r in range(R)], noise_seeds=seeds)
    _perturb(ens, B)
    ens.step = step0
    ps = [_oracle_params(ens, r) for r in range(R)]
    rng = np.random.default_rng(B)
    rows = np.stack([rng.integers(0, 1 << G, B) for G in ens.G]).astype(np.int32)
    n0 = ens.lib.dib_launch_count()
    bce = ens.train_step(betas, row_idx=rows)
    launches = ens.lib.dib_launch_count() - n0
    torch.cuda.synchronize()
    assert launches == 5, launches       # fwd, head, grouped wgrad, bwd, reduce + Adam - the unsplit and the slab path alike
    assert (ens._bufs[B]["nsplit"] > 1) == (B >= 128) and (B < 128 or ens._bufs[B]["nsplit"] == 8)
    bce = bce.cpu().numpy()
    for r, (table, G) in enumerate(zip(SI_TABLES, ens.G)):
        beta = float(np.float32(betas[r]))
        ref = oc.step(ps[r], table, rows[r].astype(np.int64), oc.eps(seeds[r], step0, B, G), beta)
        v = ens.last_step(r, B)
        assert np.array_equal(v["rows"].cpu().numpy(), rows[r])
        assert abs(float(bce[r]) - ref["bce"]) < 2e-5 * (1 + ref["bce"]), r
        kl = v["kl"].cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(kl[:G], ref["kl"], rtol=1e-5, atol=1e-6)
        assert abs(kl[G] - beta * ref["kl"].sum()) < 1e-5 * (1 + beta * ref["kl"].sum())
        np.testing.assert_allclose(v["pred"].cpu().numpy(), ref["logit"], rtol=0, atol=2e-4 * (1 + np.abs(ref["logit"]).max()))
        w, ds, dlv = _device_grads(ens, r)
        for l, (gd, gr, mag, top) in enumerate(zip(w, ref["grads"].weights, ref["grad_magnitudes"], ref["grad_max_terms"])):
            if l == 0:
                assert np.all(gd[G:] == 0.0)        # the pad rows of the first kernel get no gradient
                gd = gd[:G]
            # tests/test_gpu_circuit.py test_step_bce_kl_and_all_gradients_match_oracle's bound (see its comment)
            err, scale = np.abs(gd - gr), np.abs(gr).max() + 1e-6
            tol = 3e-4 * scale + 1e-5 * mag + (top if B >= 512 else 0.0)
            assert np.all(err <= tol), (r, l, err.max(), scale)
        for gd, gr in ((ds, ref["grads"].s), (dlv, ref["grads"].lv)):
            assert np.abs(gd - gr).max() < 3e-4 * (np.abs(gr).max() + 1e-6), (r, gd, gr)


def test_thirty_adam_steps_through_per_replica_beta_ramps_match_oracle():
    tables = [SI_TABLES[4], SI_TABLES[1], SI_TABLES[5]]
    R, B, n = 3, 96, 30
    seeds, b0, b1 = [5, 6, 7], [1e-3, 1e-2, 1e-3], [5.0, 1.0, 0.5]
    ens = CircuitEnsemble(tables, predictive_arch_spec=(64, 64, 64), init_seeds=[4, 5, 6], noise_seeds=seeds)
    ens.set_lr(1e-2)
    ps = [_oracle_params(ens, r) for r in range(R)]
    sts = [oc.adam_init(p) for p in ps]
    for step in range(n):
        betas = [circuit.beta_schedule(step, n, b0[r], b1[r]) for r in range(R)]
        ens.train_step(betas, batch_size=B)
        for r, G in enumerate(ens.G):
            ref = oc.step(ps[r], tables[r], oc.draw_rows(seeds[r], step, B, G), oc.eps(seeds[r], step, B, G), betas[r])
            oc.adam(ps[r], ref["grads"], sts[r], lr=1e-2)
    for r in range(R):
        q, p = _oracle_params(ens, r), ps[r]
        for a, b in zip(q.tensors(), p.tensors()):
            err = np.abs(a - b)
            assert err.max() < 2e-3, (r, err.max())
            assert np.mean(err < 1e-4) > 0.98, (r, np.mean(err < 1e-4))
        np.testing.assert_allclose(q.s, p.s, rtol=0, atol=1e-4)
        np.testing.assert_allclose(q.lv, p.lv, rtol=0, atol=1e-4)


@pytest.mark.parametrize("B", [17, 512])
def test_one_replica_equals_the_single_model_bit_for_bit(B):
    table = SI_TABLES[3]
    m = CircuitIB(table.shape[1] - 1, noise_seed=9, init_seed=4)
    ens = CircuitEnsemble([table], init_seeds=[4], noise_seeds=[9])
    assert np.array_equal(ens.params.cpu().numpy(), m.params.cpu().numpy())
    for step in range(5):
        beta = circuit.beta_schedule(step, 5, 1e-2, 2.0)
        a, b = m.train_step(table, beta, batch_size=B), ens.train_step(beta, batch_size=B)
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()[0]), step
    for k in ("params", "grads", "adam_m", "adam_v", "t_dev"):
        assert np.array_equal(getattr(m, k).cpu().numpy(), getattr(ens, k).cpu().numpy()), k
    assert np.array_equal(m.estimate_channel_mi_bounds(21, 256, 3, per_batch=True),
                          ens.estimate_channel_mi_bounds([21], 256, 3, per_batch=True)[0])


def test_a_replica_does_not_see_the_others():
    B, steps = 96, 4

    def run(tables, init, noise, betas):
        ens = CircuitEnsemble(tables, predictive_arch_spec=(64, 64), init_seeds=init, noise_seeds=noise)
        losses = np.stack([ens.train_step(betas, batch_size=B).cpu().numpy() for _ in range(steps)])
        return losses, [ens.replica_params(r).cpu().numpy() for r in range(ens.R)]

    la, pa = run([SI_TABLES[2], SI_TABLES[0]], [1, 2], [3, 4], [0.1, 0.2])
    lb, pb = run([SI_TABLES[2], SI_TABLES[5]], [1, 7], [3, 8], [0.1, 0.9])
    assert np.array_equal(la[:, 0], lb[:, 0]) and np.array_equal(pa[0], pb[0]), "replica 0 saw a change of replica 1"
    assert not np.array_equal(la[:, 1], lb[:, 1]) and not np.array_equal(pa[1], pb[1])


def test_launches_per_step_do_not_depend_on_the_number_of_replicas():
    lib = _lib.load_library()
    paper = circuit.truth_table(circuit.PAPER_CIRCUIT)
    counts = {}
    for B in (17, 512):          # the unsplit and the slab weight-gradient path
        m = CircuitIB(10, predictive_arch_spec=(32, 32))
        n0 = lib.dib_launch_count()
        m.train_step(paper, 0.1, batch_size=B)
        single = lib.dib_launch_count() - n0
        for R, tables in ((1, [paper]), (6, SI_TABLES), (20, [paper] * 20)):
            ens = CircuitEnsemble(tables, predictive_arch_spec=(32, 32))
            ens.train_step(0.1, batch_size=B)                      # (buffers and descriptor tables: the first step's)
            n0 = lib.dib_launch_count()
            ens.train_step(0.1, batch_size=B)
            counts[B, R] = lib.dib_launch_count() - n0
            assert counts[B, R] == single, (B, R, counts[B, R], single)
            n0 = lib.dib_launch_count()
            ens.estimate_channel_mi_bounds(evaluation_batch_size=64, number_evaluation_batches=2)
            assert lib.dib_launch_count() - n0 == 1, "an evaluation is one launch whatever R"
    print("library launches per step:", counts)
    assert set(counts.values()) == {5}, counts


def test_fit_is_reproducible_and_evaluates_like_the_single_model():
    tables, seeds = [SI_TABLES[0], SI_TABLES[2], SI_TABLES[4]], [11, 12, 13]
    kw = dict(predictive_arch_spec=(32, 32), init_seeds=[1, 2, 3], noise_seeds=[4, 5, 6])
    runs = []
    for _ in range(2):
        ens = CircuitEnsemble(tables, **kw)
        h = ens.fit(number_training_steps=40, batch_size=64, evaluate_mutual_info_freq=10, beta_start=[1e-3, 1e-2, 1e-3],
                    beta_end=5.0, seeds=seeds)
        runs.append((h, ens.params.cpu().numpy()))
    (h1, p1), (h2, p2) = runs
    assert np.array_equal(p1, p2)
    for r, (a, b) in enumerate(zip(h1, h2)):
        G = tables[r].shape[1] - 1
        assert set(a) == KEYS
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), (r, k)
        assert a["bce_loss_series"].shape == (40,) and a["beta"].shape == (40,) and np.isfinite(a["bce_loss_series"]).all()
        assert a["mutual_information_bounds"].shape == (4, G, 2) and list(a["evaluation_steps"]) == [0, 10, 20, 30]
        assert a["beta"][0] == circuit.beta_schedule(0, 40, [1e-3, 1e-2, 1e-3][r], 5.0)
        circuit.information_plane(a, circuit.entropy_bits(tables[r][:, -1]))     # the single model's post-processing applies
    # step 0's evaluation: the single model after its first step, evaluated with evaluation_seed(seeds[r], 0)
    for r, table in enumerate(tables):
        m = CircuitIB(table.shape[1] - 1, predictive_arch_spec=(32, 32), init_seed=kw["init_seeds"][r], noise_seed=kw["noise_seeds"][r])
        m.train_step(table, circuit.beta_schedule(0, 40, [1e-3, 1e-2, 1e-3][r], 5.0), batch_size=64)
        ref = m.estimate_channel_mi_bounds(circuit.evaluation_seed(seeds[r], 0)) / np.log(2)
        assert np.array_equal(h1[r]["mutual_information_bounds"][0], ref), r


def test_to_model_continues_a_replica_with_the_same_bits():
    tables, B = [SI_TABLES[1], SI_TABLES[5]], 160
    ens = CircuitEnsemble(tables, predictive_arch_spec=(64, 64), init_seeds=[3, 4], noise_seeds=[5, 6])
    for step in range(3):
        ens.train_step([0.2, 0.4], batch_size=B)
    r = 1
    m = ens.to_model(r)
    assert isinstance(m, CircuitIB) and m.G == ens.G[r] and m.step == ens.step
    rows = np.random.default_rng(0).integers(0, 1 << ens.G[r], (2, B)).astype(np.int32)
    a = ens.train_step([0.2, 0.4], row_idx=rows)
    b = m.train_step(tables[r], 0.4, row_idx=rows[r])
    assert np.array_equal(a.cpu().numpy()[r], b.cpu().numpy())
    sl = slice(r * ens.n_params, (r + 1) * ens.n_params)
    for k in ("params", "adam_m", "adam_v"):
        assert np.array_equal(getattr(ens, k)[sl].cpu().numpy(), getattr(m, k).cpu().numpy()), k
    # get / set round trip of a replica's weights
    w = ens.get_weights(0)
    assert w["predictive_model"][0].shape == (ens.G[0], 64) and w["mu_scaling"].shape == (ens.G[0],)
    before = ens.params.cpu().numpy()
    ens.set_weights(0, w)
    assert np.array_equal(ens.params.cpu().numpy(), before)


def test_argument_errors_raise_before_any_launch():
    lib = _lib.load_library()
    t = SI_TABLES[0]
    ens = CircuitEnsemble([t, SI_TABLES[2]], predictive_arch_spec=(16,))
    n0 = lib.dib_launch_count()
    for bad in (dict(truth_tables=[]), dict(truth_tables=[t, t], init_seeds=[1]), dict(truth_tables=[t, t], noise_seeds=[1, 2, 3]),
                dict(truth_tables=[t[:-1]]), dict(truth_tables=[np.zeros((1 << 17, 18), np.int32)]),
                dict(truth_tables=[t], predictive_arch_spec=(24,)), dict(truth_tables=[t], predictive_arch_spec=(16, 16, 16, 16))):
        with pytest.raises(ValueError):
            CircuitEnsemble(**bad)
    for B in (0, 2049):
        with pytest.raises(ValueError):
            ens.train_step(0.1, batch_size=B)
        with pytest.raises(ValueError):
            ens.fit(number_training_steps=2, batch_size=B)
    with pytest.raises(ValueError):
        ens.train_step([0.1, 0.2, 0.3], batch_size=8)                   # a beta list of the wrong length
    with pytest.raises(ValueError):
        ens.fit(number_training_steps=2, batch_size=8, beta_end=[1.0])
    with pytest.raises(ValueError):
        ens.fit(number_training_steps=2, batch_size=8, seeds=[1])
    with pytest.raises(ValueError):
        ens.train_step(0.1, row_idx=np.zeros((3, 8), np.int32))         # rows of another number of replicas
    with pytest.raises(ValueError):
        ens.estimate_channel_mi_bounds([1])
    with pytest.raises(ValueError):
        ens.estimate_channel_mi_bounds(evaluation_batch_size=1)
    assert lib.dib_launch_count() == n0
