"""DistributedIBEnsemble against the float64 oracle and against itself: every replica's History over a fit with its own seeds and
beta ramp (tests/test_gpu_parity.py::_fit_trajectory's setting, key set and tolerances), every gradient block of every replica
read through the single model's layout, a launch count that does not depend on R or F, isolation of the replicas, to_model and
the weight access, and an 'mse' pair."""
import numpy as np
import pytest
import torch

import dib_amd
import dib_oracle as orc
from _helpers import flat_to_params, params_to_flat, spec_kwargs

pytestmark = pytest.mark.gpu

BCE = "bce_logits"


def _circuit_c():
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)  # SI circuit (c)
    return np.tile(x, (8, 1)).astype(np.float32), np.tile(y, 8).astype(np.float32)


def _adam(lr):
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = lr
    return opt


def _ensemble(spec, R, loss, metrics=None, lr=3e-3, **seeds):
    ens = dib_amd.DistributedIBEnsemble(R, **spec_kwargs(spec), **seeds)
    return ens.compile(optimizer=_adam(lr), loss=loss, metrics=metrics)


def _params(ens, spec, r):
    return flat_to_params(ens.param_blocks(), ens.get_flat_weights(r), spec)


def _check_history(got, ref, what):
    assert set(ref) == set(got), (what, sorted(set(ref) ^ set(got)))
    for k in ref:
        g, want = np.array(got[k]), np.array(ref[k])
        tol = 1e-3 if "KL" in k else 2e-3
        assert np.abs(g - want).max() < tol * (1 + np.abs(want).max()), (what, k, g, want)


TRAJ_SPEC = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
SEEDS = dict(init_seeds=[2, 12, 5], noise_seeds=[4, 9, 1], shuffle_seeds=[6, 3, 8])
RAMPS = ([1e-3, 1e-2, 3e-4], [1.0, 0.3, 2.0], 2, 6)   # beta_start, beta_end per replica; pretraining, annealing epochs


def test_every_replicas_history_matches_the_oracle_fit_with_its_seeds_and_ramp():
    x, y = _circuit_c()
    ens = _ensemble(TRAJ_SPEC, 3, dib_amd.losses.BinaryCrossentropy(from_logits=True), ["accuracy"], **SEEDS)
    start = [_params(ens, TRAJ_SPEC, r) for r in range(3)]
    epochs, bs = 8, 48   # 128 rows -> two full batches and a partial one
    hists = ens.fit(x, y, batch_size=bs, epochs=epochs, validation_data=(x[:40], y[:40]), shuffle=True, beta_start=RAMPS[0],
                    beta_end=RAMPS[1], number_pretraining_epochs=RAMPS[2], number_annealing_epochs=RAMPS[3])
    assert len(hists) == 3 and ens._step == epochs * 3
    for r in range(3):
        ref = orc.fit(TRAJ_SPEC, start[r], x, y, epochs=epochs, batch_size=bs, loss_kind=BCE,
                      beta_fn=lambda e: orc.beta_schedule(e, RAMPS[0][r], RAMPS[1][r], RAMPS[2], RAMPS[3]), lr=3e-3, shuffle=True,
                      validation_data=(x[:40], y[:40]), noise_seed=SEEDS["noise_seeds"][r], shuffle_seed=SEEDS["shuffle_seeds"][r],
                      metrics=["accuracy"])
        _check_history(hists[r].history, ref, f"replica {r}")
        assert hists[r].epoch == list(range(epochs))


@pytest.mark.parametrize("B", [37, 150])   # one slab written straight into the gradient buffer / two slabs and the reduce
def test_gradients_of_both_replicas_match_the_oracle(B):
    spec = orc.DIBSpec([2, 2, 2], [17, 9], [13], 3, activation_fn="tanh", feature_embedding_dimension=6,
                       number_positional_encoding_frequencies=3)
    ens = _ensemble(spec, 2, dib_amd.losses.SparseCategoricalCrossentropy(from_logits=True), init_seeds=[3, 8], noise_seeds=[11, 5])
    rng = np.random.default_rng(B)
    n = B + 40
    x = rng.standard_normal((n, 6)).astype(np.float32)
    y = rng.integers(0, 3, (n, 1)).astype(np.float32)
    rows = np.stack([rng.permutation(n)[:B] for _ in range(2)]).astype(np.int32)
    betas = [0.37, 0.05]
    ens.set_data(x, y)
    ens._step = 5
    ens.train_step(rows, beta=betas, apply_optimizer=False)
    blocks = ens.param_blocks()
    for r in range(2):
        p = _params(ens, spec, r)
        eps = orc.philox_normal_all(ens.noise_seeds[r], 5, rows[r], 3, 6)
        c = orc.forward(spec, p, x[rows[r]].astype(np.float64), eps)
        _, grads, _ = orc.backward(spec, p, x[rows[r]].astype(np.float64), y[rows[r]], c, betas[r], "sparse_cce_logits")
        gflat = ens.get_flat_grads(r)
        gref = params_to_flat(blocks, grads, len(gflat)).astype(np.float64)
        for b in blocks:
            sl = slice(b["offset"], b["offset"] + b["rows"] * b["cols"])
            err = np.abs(gflat[sl] - gref[sl]).max()
            assert err <= 3e-4 * (np.abs(gref[sl]).max() + 1e-3), (r, b, err, np.abs(gref[sl]).max())


def test_launches_per_step_do_not_depend_on_replicas_or_features():
    counts = {}
    for R, F in ((1, 2), (3, 4), (6, 10)):
        spec = orc.DIBSpec([1] * F, [32, 32], [64, 64], 1, feature_embedding_dimension=8)
        ens = _ensemble(spec, R, dib_amd.losses.BinaryCrossentropy(from_logits=True))
        rng = np.random.default_rng(F)
        x = rng.standard_normal((200, F)).astype(np.float32)
        ens.set_data(x, (x[:, :1] > 0).astype(np.float32))
        for b in (32, 160):   # one gradient slab / two and the reduce
            rows = np.stack([rng.permutation(200)[:b] for _ in range(R)]).astype(np.int32)
            n0 = ens.lib.dib_launch_count()
            ens.train_step(rows)
            counts.setdefault(b, []).append(ens.lib.dib_launch_count() - n0)
        torch.cuda.synchronize()
        assert np.isfinite(ens.get_flat_weights(R - 1)).all()
    for b, c in counts.items():
        assert len(set(c)) == 1, (b, c)
    assert counts[160][0] == counts[32][0] + 1, (counts, "the two-slab batch adds dib_reduce_splits and nothing else")


def test_a_replica_does_not_see_the_others():
    x, y = _circuit_c()
    rng = np.random.default_rng(0)
    rows = np.stack([np.stack([rng.permutation(128)[:48] for _ in range(2)]) for _ in range(3)]).astype(np.int32)   # [step, R, b]

    def run(change):
        seeds = dict(init_seeds=[2, 7], noise_seeds=[4, 9])
        betas = [0.1, 0.5]
        if change == "seeds":
            seeds = dict(init_seeds=[2, 70], noise_seeds=[4, 90])
        if change == "beta":
            betas = [0.1, 5.0]
        ens = _ensemble(TRAJ_SPEC, 2, dib_amd.losses.BinaryCrossentropy(from_logits=True), **seeds)
        if change == "weights":
            ens.set_flat_weights(1, 0.5 * ens.get_flat_weights(1))
        ens.set_data(x, y)
        for s in range(3):
            r = rows[s].copy()
            if change == "rows":
                r[1] = r[1][::-1]
            ens.train_step(r, beta=betas)
        return ens.get_flat_weights(0), ens.get_flat_weights(1)

    base0, base1 = run(None)
    for change in ("seeds", "beta", "weights", "rows"):
        w0, w1 = run(change)
        assert np.array_equal(w0, base0), f"replica 0 moved when replica 1's {change} changed"
        if change != "rows":   # (a reversed batch is the same batch: the sums run in another order)
            assert not np.array_equal(w1, base1), change


def test_to_model_continues_the_replica_and_weight_access_round_trips():
    x, y = _circuit_c()
    ens = _ensemble(TRAJ_SPEC, 3, dib_amd.losses.BinaryCrossentropy(from_logits=True), ["accuracy"], **SEEDS)
    bs, r = 48, 1
    ens.fit(x, y, batch_size=bs, epochs=2, validation_data=(x[:40], y[:40]), beta_start=RAMPS[0], beta_end=RAMPS[1],
            number_pretraining_epochs=RAMPS[2], number_annealing_epochs=RAMPS[3])
    m = ens.to_model(r)
    assert isinstance(m, dib_amd.DistributedIBNet) and m._step == ens._step == 6
    assert (m.noise_seed, m.init_seed, m.shuffle_seed) == (9, 12, 3)
    w = ens.get_flat_weights(r)
    assert np.array_equal(m.get_flat_weights(), w)
    assert float(m.beta.value()) == float(orc.beta_schedule(1, RAMPS[0][r], RAMPS[1][r], RAMPS[2], RAMPS[3]))
    eng = m._ensure_engine()
    assert int(eng.t_dev.item()) == 6 and float(eng.opt_state.m.abs().max()) > 0
    bounds = m.information_per_feature(x, evaluation_batch_size=64, number_evaluation_batches=2)
    assert bounds.shape == (4, 2) and np.isfinite(bounds).all()
    # one further epoch as a single model against oracle.fit continued from the same state: the oracle runs the three epochs and
    # takes the device's parameters and Adam state at the end of epoch 1 (its on_epoch_end hook)
    state = (flat_to_params(eng.blocks, w, TRAJ_SPEC), flat_to_params(eng.blocks, eng.opt_state.m.cpu().numpy(), TRAJ_SPEC),
             flat_to_params(eng.blocks, eng.opt_state.v.cpu().numpy(), TRAJ_SPEC))

    def resync(epoch, p, st):
        if epoch == 1:
            for dst, src in zip((p, st.m, st.v), state):
                for a, b in zip(dst.tensors(), src.tensors()):
                    a[...] = b
            st.t = 6

    ref = orc.fit(TRAJ_SPEC, orc.glorot_uniform_init(TRAJ_SPEC, 0), x, y, epochs=3, batch_size=bs, loss_kind=BCE,
                  beta_fn=lambda e: orc.beta_schedule(e, RAMPS[0][r], RAMPS[1][r], RAMPS[2], RAMPS[3]), lr=3e-3, shuffle=True,
                  validation_data=(x[:40], y[:40]), noise_seed=9, shuffle_seed=3, metrics=["accuracy"], on_epoch_end=resync)
    cb = dib_amd.InfoBottleneckAnnealingCallback(RAMPS[0][r], RAMPS[1][r], RAMPS[2], RAMPS[3])
    hist = m.fit(x, y, epochs=3, initial_epoch=2, shuffle=True, batch_size=bs, callbacks=[cb], verbose=False,
                 validation_data=(x[:40], y[:40]))
    _check_history(hist.history, {k: v[2:] for k, v in ref.items()}, "the replica continued as a DistributedIBNet")
    # weight access: the single model's layout in, the same vector out, the other replicas untouched
    others = [ens.get_flat_weights(q) for q in (0, 2)]
    new = np.random.default_rng(1).standard_normal(len(w)).astype(np.float32)
    gaps = np.ones(len(w), dtype=bool)
    for b in ens.param_blocks():
        gaps[b["offset"]: b["offset"] + b["rows"] * b["cols"]] = False
    new[gaps] = 0.0
    ens.set_flat_weights(r, new)
    assert np.array_equal(ens.get_flat_weights(r), new)
    assert all(np.array_equal(ens.get_flat_weights(q), o) for q, o in zip((0, 2), others))
    res = ens.evaluate(x[:40], y[:40], batch_size=16)
    assert len(res) == 3 and set(res[0]) == {"loss", "accuracy", "beta"} | {f"KL{f}" for f in range(4)}


def test_an_mse_pair_with_two_outputs_matches_the_oracle():
    spec = orc.DIBSpec([2, 2], [16], [24], 2, activation_fn="tanh", feature_embedding_dimension=4)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((100, 4)).astype(np.float32)
    y = np.stack([x[:, 0] * x[:, 2], np.sin(x[:, 1]) + x[:, 3]], 1).astype(np.float32)
    ens = _ensemble(spec, 2, "mse", init_seeds=[1, 2], noise_seeds=[3, 4], shuffle_seeds=[5, 6])
    start = [_params(ens, spec, r) for r in range(2)]
    hists = ens.fit(x, y, batch_size=32, epochs=2, validation_data=(x[:30], y[:30]), beta_start=[1e-2, 1e-1], beta_end=[1e-2, 1e-1])
    for r in range(2):
        ref = orc.fit(spec, start[r], x, y, epochs=2, batch_size=32, loss_kind="mse", beta_fn=lambda e: np.float32([1e-2, 1e-1][r]),
                      lr=3e-3, shuffle=True, validation_data=(x[:30], y[:30]), noise_seed=3 + r, shuffle_seed=5 + r)
        _check_history(hists[r].history, ref, f"mse replica {r}")
