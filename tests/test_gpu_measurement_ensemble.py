"""MeasurementEnsemble: R measurement models of one architecture trained in lockstep, every launch shared.  Against the float64
oracle (tests/_oracle_measurement.py) replica by replica - each with its own initial weights, its own Philox seed and its own
batches - on the shapes of tests/test_gpu_measurement.py, at that file's bounds; then what only an ensemble has: a launch count
that does not depend on R, replicas that cannot see one another, retirement of replicas in fit, and access to one replica."""
import numpy as np
import pytest
import torch

import _oracle_measurement as om
import test_gpu_measurement as tm
from dib_amd import MeasurementEnsemble, _lib
from dib_amd.measurement import MeasurementIB, beta_schedule

pytestmark = pytest.mark.gpu

R = 3
INIT, NOISE = [5, 21, 40], [11, 3, 29]
NETS = ["ib", "vq", "agg", "ref"]
# the ragged_p1.5 shapes and the variants that change a kernel's path: logits in two lane groups, two embedding tiles, L = 1,
# a ragged row count, the reference state at the other end, cosine / temperature in the batched InfoNCE, and l1, which has no
# batched InfoNCE and takes the loop over the single entry point
CASES = {n: tm.CONFIGS[n] for n in ["ragged_p1.5", "a5", "e17", "l1", "ragged_rows259", "reference_minus1", "cosine",
                                    "temperature0.5"]}
CASES["similarity_l1"] = dict(traj="uniform", B=96, kw=dict(tm._SMALL, infonce_similarity="l1"), p=2.0)


def _grads(e, r):
    P = e.n_params
    g = e.grads[r * P: (r + 1) * P].cpu().numpy().astype(np.float64)
    return {k: sum(([g[s.base + w: s.base + w + i * o].reshape(i, o), g[s.base + b: s.base + b + o]]
                    for (i, o), w, b in zip(s.dims, s.w_off, s.b_off)), []) for k, s in e._nets.items()}


def _same(a, b):
    return all(np.array_equal(x, y) for k in NETS for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("name", list(CASES))
def test_step_losses_and_all_gradients_of_every_replica_match_oracle(name):
    c = CASES[name]
    e = MeasurementEnsemble(R, init_seeds=INIT, noise_seeds=NOISE, **c["kw"])
    L, d, B, E = e.L, e.d, c["B"], e.E
    traj = tm._traj(c["traj"], 20_000, d)
    states = np.stack([traj[tm.om_idx(np.random.default_rng(1 + r).choice(len(traj) - L, size=B), L)] for r in range(R)])
    w = [e.get_weights(r) for r in range(R)]
    if name == "ragged_p1.5":   # replica r starts from the weights of MeasurementIB(init_seed=init_seeds[r])
        for r in range(R):
            assert _same(w[r], tm._weights(MeasurementIB(**c["kw"], init_seed=INIT[r], noise_seed=NOISE[r]))), r
    beta = 0.37
    e.beta = beta
    loss, lp, kl = e.match_batch(states, training=True)
    for r in range(R):
        eps = om.eps_rows(NOISE[r], 0, np.arange(B * L), E)
        rl, rlp, rkl, rg = om.match_batch(w[r], states[r].astype(np.float64), eps, np.float32(beta), c["p"], e.n_freq,
                                          **tm._oracle_options(c["kw"]))
        assert abs(kl[r] - rkl) <= 1e-5 * abs(rkl), (r, kl[r], rkl)
        assert abs(lp[r] - rlp) <= 1e-5 * abs(rlp), (r, lp[r], rlp)
        assert abs(loss[r] - rl) <= 1e-5 * abs(rl), (r, loss[r], rl)
        g = _grads(e, r)
        for net in rg:
            for i, (a, b) in enumerate(zip(g[net], rg[net])):
                assert tm._rel(a, b) <= 1e-4, (r, net, i, tm._rel(a, b))


def test_train_steps_through_the_beta_ramp_match_oracle_adam():
    kw = tm.CONFIGS["ragged_p1.5"]["kw"]
    init, noise, seeds = [9, 30, 50], [2, 7, 1], [4, 9, 13]
    e = MeasurementEnsemble(R, init_seeds=init, noise_seeds=noise, **kw)
    traj = tm._traj("uniform", 5000, 1)
    w0 = [e.get_weights(r) for r in range(R)]
    steps, B, lr = 30, 64, 1e-3
    hist = e.fit(traj, number_training_steps=steps, batch_size=B, learning_rate=lr, beta_start=10, beta_end=1e-4, seeds=seeds)
    for r in range(R):
        rng, state, losses, w = np.random.default_rng(seeds[r]), {}, [], w0[r]
        for s in range(steps):
            starts = rng.choice(len(traj) - e.L, size=B)
            eps = om.eps_rows(noise[r], s, np.arange(B * e.L), e.E)
            l, _, _, g = om.match_batch(w, traj[tm.om_idx(starts, e.L)].astype(np.float64), eps, np.float32(tm.om_beta(s, steps)), 1.5,
                                        e.n_freq)
            losses.append(l)
            w = om.adam(w, g, state, s, lr)
        assert hist[r]["steps"] == steps and hist[r]["beta"] == [beta_schedule(s, steps, 10, 1e-4) for s in range(steps)]
        np.testing.assert_allclose(hist[r]["loss"], losses, rtol=1e-4)
        got = e.get_weights(r)
        for net in w:
            for a, b in zip(got[net], w[net]):
                assert tm._rel(a, b) <= 1e-4, (r, net, tm._rel(a, b))


def _launches_of_one_step(replicas, kw, B=64):
    lib = _lib.load_library()
    e = MeasurementEnsemble(replicas, **kw)
    traj = torch.from_numpy(tm._traj("uniform", 3000, e.d)).cuda()
    starts = np.stack([np.random.default_rng(r).choice(3000 - e.L, size=B) for r in range(replicas)])
    e.match_batch_from_starts(traj, starts)          # builds the plans
    n0 = lib.dib_launch_count()
    e.match_batch_from_starts(traj, starts)
    torch.cuda.synchronize()
    return lib.dib_launch_count() - n0


@pytest.mark.parametrize("name", ["ragged_p1.5", "cosine"])
def test_launches_of_a_step_do_not_depend_on_the_number_of_replicas(name):
    kw = CASES[name]["kw"]
    one, four = _launches_of_one_step(1, kw), _launches_of_one_step(4, kw)
    assert one == four and one > 0, (one, four)
    # ... and the similarity without a batched kernel pays one InfoNCE sequence per replica
    l1 = CASES["similarity_l1"]["kw"]
    assert _launches_of_one_step(4, l1) > _launches_of_one_step(1, l1)


def test_a_replica_does_not_see_the_others():
    """other seeds (weights, noise, batches) for replica 1: replica 0's losses and weights keep their bits, replica 1's change"""
    kw = tm.CONFIGS["ragged_p1.5"]["kw"]
    traj = tm._traj("uniform", 5000, 1)
    out = []
    for init, noise, seeds in [(INIT, NOISE, [4, 9, 13]), ([5, 77, 40], [11, 8, 29], [4, 10, 13])]:
        e = MeasurementEnsemble(R, init_seeds=init, noise_seeds=noise, **kw)
        h = e.fit(traj, number_training_steps=5, batch_size=64, learning_rate=1e-3, seeds=seeds)
        out.append((h, [e.get_weights(r) for r in range(R)]))
    (ha, wa), (hb, wb) = out
    for r in (0, 2):
        assert ha[r]["loss"] == hb[r]["loss"] and _same(wa[r], wb[r]), r
    assert ha[1]["loss"] != hb[1]["loss"] and not _same(wa[1], wb[1])


def test_fit_retires_replicas_at_their_own_thresholds():
    """thresholds [0, inf, 0] on an encoder that transmits information from the start (beta 1e-2): replicas 0 and 2 retire at the
    first evaluation - their snapshots are the weights of a fit cut there - while replica 1 trains on as in a fit that never stops"""
    kw = tm.CONFIGS["ragged_p1.5"]["kw"]
    traj, ev = tm._traj("uniform", 4000, 1), tm._traj("uniform", 3000, 1)[::-1].copy()
    every, steps = 4, 12

    def run(thr):
        e = MeasurementEnsemble(R, init_seeds=INIT, noise_seeds=NOISE, **kw)
        h = e.fit(traj, number_training_steps=steps, batch_size=64, learning_rate=1e-3, beta_start=1e-2, beta_end=1e-4,
                  info_eval_data=ev, evaluate_info_every=every, info_evaluation_batch_size=256, info_evaluation_number_batches=2,
                  info_stopping_point=thr, seeds=[0, 1, 2])
        return e, h

    e, h = run([0.0, float("inf"), 0.0])
    cut, hc = run(0.0)
    full, hf = run(float("inf"))
    assert [x["steps"] for x in hc] == [every] * R and [x["steps"] for x in hf] == [steps] * R
    assert [x["steps"] for x in h] == [every, steps, every]
    assert sorted(e.snapshots) == [0, 2]
    for r in (0, 2):
        assert _same(e.get_weights(r), cut.get_weights(r)), r
        assert h[r]["loss"] == hc[r]["loss"] and len(h[r]["loss"]) == every and len(h[r]["beta"]) == every
        assert len(h[r]["info_in"]) == 1 and len(h[r]["info_out"]) == 1
        np.testing.assert_array_equal(h[r]["info_in"][0], hc[r]["info_in"][0])
        assert np.mean(h[r]["info_in"][0]) >= 0.0
        # the lockstep step went on computing the retired replica: its live weights moved on, the snapshot did not
        live = e.params[r * e.n_params: (r + 1) * e.n_params]
        assert not torch.equal(live, e.snapshots[r])
    assert _same(e.get_weights(1), full.get_weights(1))
    assert h[1]["loss"] == hf[1]["loss"] and len(h[1]["loss"]) == steps
    assert len(h[1]["info_in"]) == steps // every and len(h[1]["info_out"]) == steps // every
    assert all(np.all(np.isfinite(i)) and i[0] <= i[1] + 1e-6 for x in h for i in x["info_in"])


def test_one_replica_as_a_model_and_its_symbols():
    kw = tm.CONFIGS["ragged_p1.5"]["kw"]
    e = MeasurementEnsemble(R, init_seeds=INIT, noise_seeds=NOISE, **kw)
    traj = tm._traj("uniform", 5000, 1)
    e.fit(traj, number_training_steps=3, batch_size=64, learning_rate=1e-3)
    x = traj[:3001]
    noise = np.random.default_rng(7).standard_normal((100, e.E)).astype(np.float32)
    for r in range(R):
        w = e.get_weights(r)
        ref = MeasurementIB(**kw)
        for net, k in zip([ref.info_bott_encoder, ref.vector_quantization_network, ref.measurement_aggregator_network,
                           ref.reference_state_encoder], NETS):
            net.set_weights(w[k])
        want = ref.symbolize(x, noise_vector=noise, return_counts=True, chunk_size=1024)
        m = e.to_model(r)
        assert isinstance(m, MeasurementIB) and _same(tm._weights(m), w) and m.noise_seed == NOISE[r]
        for got in (m.symbolize(x, noise_vector=noise, return_counts=True, chunk_size=1024),
                    e.symbolize(r, x, noise_vector=noise, return_counts=True, chunk_size=1024)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), r
    assert len({e.symbolize(r, x, noise_vector=noise).tobytes() for r in range(R)}) > 1, "the replicas' partitions differ"
    e.set_weights(0, e.get_weights(1))
    assert _same(e.get_weights(0), e.get_weights(1))
    with pytest.raises(IndexError):
        e.get_weights(R)


def test_constructor_outside_the_envelope_raises_before_any_launch():
    lib = _lib.load_library()
    n0 = lib.dib_launch_count()
    with pytest.raises(ValueError, match="envelope"):
        MeasurementEnsemble(R, input_dimensionality=2, alphabet_size=17)
    with pytest.raises(ValueError, match="envelope"):
        MeasurementEnsemble(R, input_dimensionality=2, vector_quant_arch_spec=(256, 256))
    with pytest.raises(ValueError, match="one seed per replica"):
        MeasurementEnsemble(R, init_seeds=[1, 2], input_dimensionality=2)
    assert lib.dib_launch_count() == n0
