"""The measurement-partition model (chaos notebook cell 10) on the device against the float64 oracle
(tests/_oracle_measurement.py) with the same Philox noise: one step's losses and all four networks' gradients, a short
Adam loop through the beta ramp, the fused symbolisation, its determinism, and the envelope."""
import numpy as np
import pytest
import torch

import _oracle_measurement as om
from _helpers import dispatch_path
from dib_amd import chaos_data
from dib_amd.measurement import MeasurementIB

pytestmark = pytest.mark.gpu


def _ikeda(n, seed=0):
    return np.asarray(chaos_data.generate_data("ikeda", n, number_skip_iterations=1000, seed=seed), dtype=np.float32)


def _weights(m):
    return {"ib": m.info_bott_encoder.get_weights(), "vq": m.vector_quantization_network.get_weights(),
            "agg": m.measurement_aggregator_network.get_weights(), "ref": m.reference_state_encoder.get_weights()}


def _grads(m):
    out = {}
    for k, s in zip(["ib", "vq", "agg", "ref"], m._stacks):
        g = s.grads.cpu().numpy().astype(np.float64)
        out[k] = sum(([g[w: w + i * o].reshape(i, o), g[b: b + o]] for (i, o), w, b in zip(s.dims, s.w_off, s.b_off)), [])
    return out


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-30))


CONFIGS = {
    "notebook": dict(traj="ikeda", B=2048, kw=dict(input_dimensionality=2), p=2.0),
    "ragged_p1": dict(traj="uniform", B=96, kw=dict(input_dimensionality=1, number_states=5, alphabet_size=3,
                                                     information_bottleneck_embedding_dimension=4,
                                                     info_bott_encoder_arch_spec=(48, 48), vector_quant_arch_spec=(48, 64),
                                                     measurement_aggregator_arch_spec=(64, 64),
                                                     reference_state_encoder_arch_spec=(48, 48), kl_loss_exponent=1.0), p=1.0),
    "ragged_p1.5": dict(traj="uniform", B=96, kw=dict(input_dimensionality=1, number_states=5, alphabet_size=3,
                                                       information_bottleneck_embedding_dimension=4,
                                                       info_bott_encoder_arch_spec=(48, 48), vector_quant_arch_spec=(48, 64),
                                                       measurement_aggregator_arch_spec=(64, 64),
                                                       reference_state_encoder_arch_spec=(48, 48), kl_loss_exponent=1.5), p=1.5),
}
# the kernels' envelope and the loss options, one short step each (from the ragged_p1.5 shapes)
_SMALL = dict(CONFIGS["ragged_p1.5"]["kw"], kl_loss_exponent=2.0)
for _name, _b, _kw in [("relu", 96, dict(activation_function="relu")),
                       ("linear", 96, dict(activation_function="linear")),
                       ("e17", 96, dict(information_bottleneck_embedding_dimension=17)),
                       ("e32", 96, dict(information_bottleneck_embedding_dimension=32)),
                       ("a5", 96, dict(alphabet_size=5)),
                       ("a16", 96, dict(alphabet_size=16)),
                       ("l1", 96, dict(number_states=1)),
                       ("l32", 96, dict(number_states=32)),
                       ("d3", 96, dict(input_dimensionality=3)),
                       ("d4", 96, dict(input_dimensionality=4)),
                       ("ragged_rows259", 37, dict(number_states=7)),
                       ("reference_last", 96, dict(reference_timestep=4)),
                       ("reference_minus1", 96, dict(reference_timestep=-1)),
                       ("temperature0.5", 96, dict(infonce_temperature=0.5)),
                       ("cosine", 96, dict(infonce_similarity="cosine")),
                       # 2E = 16 and B L = 480 <= 2048: the IB encoder on the row-tile kernel (dib_mlp_small_fwd, gathered rows)
                       ("ib_row_tiles_e8", 96, dict(information_bottleneck_embedding_dimension=8))]:
    CONFIGS[_name] = dict(traj="uniform", B=_b, kw=dict(_SMALL, **_kw), p=2.0)


def _oracle_options(kw):
    return dict(reference_timestep=kw.get("reference_timestep", 0), temperature=kw.get("infonce_temperature", 1.0),
                similarity=kw.get("infonce_similarity", "l2sq"), slope=om.SLOPES[kw.get("activation_function", "leaky_relu")])


def _traj(kind, n, d):
    if kind == "ikeda":
        return _ikeda(n)
    return np.random.default_rng(3).uniform(-1, 1, (n, d)).astype(np.float32)


# both sides of the DenseStack switch (tests/_helpers.py DISPATCH_PATHS): "default" takes the row-tile kernels for batches of
# <= 2048 rows whose layer widths are multiples of 16, "large_batch" the grouped GEMMs everywhere; dib_measure_bwd reads the
# aggregator's g1 from whichever ran
@pytest.mark.parametrize("name,path", [pytest.param(n, p, id=n if p == "default" else f"{n}-{p}")
                                       for p in ("default", "large_batch") for n in CONFIGS])
def test_step_losses_and_all_gradients_match_oracle(name, path):
    c = CONFIGS[name]
    with dispatch_path(path):
        m = MeasurementIB(**c["kw"], noise_seed=11, init_seed=5)
        loss, lp, kl, w, states, beta = _one_step(m, c)
        # which kernels ran: the VQ chain always in dib_measure_fwd; the other three networks on DenseStack
        assert m.vq._last is None
        for s, n in [(m.ib, c["B"] * m.L), (m.agg, c["B"]), (m.ref, c["B"])]:
            want = path == "default" and n <= 2048 and all(o % 16 == 0 for _, o in s.dims)
            assert s._last["small"] == want, (path, s.dims, n, s._last["small"])
    L, d, B, E = m.L, m.d, c["B"], m.E
    eps = om.eps_rows(11, 0, np.arange(B * L), E)
    rl, rlp, rkl, rg = om.match_batch(w, states.astype(np.float64), eps, np.float32(beta), c["p"], m.n_freq,
                                      **_oracle_options(c["kw"]))
    assert abs(kl - rkl) <= 1e-5 * abs(rkl), (kl, rkl)
    assert abs(lp - rlp) <= 1e-5 * abs(rlp), (lp, rlp)
    assert abs(loss - rl) <= 1e-5 * abs(rl), (loss, rl)
    g = _grads(m)
    for net in rg:
        for i, (a, b) in enumerate(zip(g[net], rg[net])):
            assert _rel(a, b) <= 1e-4, (net, i, _rel(a, b))


def test_config_grid_reaches_the_row_tile_ib_encoder():
    """at least one config puts the IB encoder on the row-tile kernel by default (2E % 16 == 0, B L <= 2048)"""
    assert any(2 * c["kw"].get("information_bottleneck_embedding_dimension", 8) % 16 == 0
               and c["B"] * c["kw"].get("number_states", 12) <= 2048 for c in CONFIGS.values())


def _one_step(m, c):
    """one training step of config c on model m: (loss, loss_prediction, kl, the weights before it, states, beta)"""
    L, d, B = m.L, m.d, c["B"]
    traj = _traj(c["traj"], 20_000, d)
    starts = np.random.default_rng(1).choice(len(traj) - L, size=B)
    states = traj[om_idx(starts, L)]
    w = _weights(m)
    beta = 0.37
    m.beta = beta
    loss, lp, kl = m.match_batch(states, training=True)
    return loss, lp, kl, w, states, beta


def test_reference_timestep_minus_one_is_the_last_state():
    """NumPy indexing: reference_timestep = -1 is stored as L - 1 and gives the same bits as L - 1"""
    c = CONFIGS["reference_last"]
    out = []
    for r in (-1, 4):
        m = MeasurementIB(**dict(c["kw"], reference_timestep=r), noise_seed=11, init_seed=5)
        assert m.reference_timestep == m.L - 1
        loss, lp, kl, _, _, _ = _one_step(m, c)
        out.append(((loss, lp, kl), _grads(m)))
    assert out[0][0] == out[1][0], out
    for net in out[0][1]:
        for a, b in zip(out[0][1][net], out[1][1][net]):
            assert np.array_equal(a, b), net


def om_idx(starts, L):
    from dib_amd.measurement import sequence_indices
    return sequence_indices(starts, L)


def test_train_steps_through_the_beta_ramp_match_oracle_adam():
    kw = CONFIGS["ragged_p1.5"]["kw"]
    m = MeasurementIB(**kw, noise_seed=2, init_seed=9)
    traj = _traj("uniform", 5000, 1)
    w = _weights(m)
    steps, B, lr = 30, 64, 1e-3
    hist = m.fit(traj, number_training_steps=steps, batch_size=B, learning_rate=lr, beta_start=10, beta_end=1e-4, seed=4)
    rng = np.random.default_rng(4)
    state, losses = {}, []
    for s in range(steps):
        beta = om_beta(s, steps)
        starts = rng.choice(len(traj) - m.L, size=B)
        eps = om.eps_rows(2, s, np.arange(B * m.L), m.E)
        l, _, _, g = om.match_batch(w, traj[om_idx(starts, m.L)].astype(np.float64), eps, np.float32(beta), 1.5, m.n_freq)
        losses.append(l)
        w = om.adam(w, g, state, s, lr)
    np.testing.assert_allclose(hist["loss"], losses, rtol=1e-4)
    got = _weights(m)
    for net in w:
        for a, b in zip(got[net], w[net]):
            assert _rel(a, b) <= 1e-4, (net, _rel(a, b))


def om_beta(s, n):
    from dib_amd.measurement import beta_schedule
    return beta_schedule(s, n, 10, 1e-4)


@pytest.fixture(scope="module")
def trained():
    m = MeasurementIB(2, noise_seed=0, init_seed=1)
    traj = _ikeda(30_000)
    m.fit(traj, number_training_steps=20, batch_size=512, seed=0)
    return m, traj


def test_symbolize_matches_oracle(trained):
    m, traj = trained
    # 20 steps leave the partition's logits close together, so that with 100 draws per point some draw of almost every
    # fifth point falls within 1e-3 of a tie; the last VQ layer scaled by 2^10 (exact in fp32: the argmaxes do not change)
    # separates the logits so that the near-tie exclusion below stays under 0.1 %
    vw = m.vector_quantization_network.get_weights()
    m.vector_quantization_network.set_weights(vw[:4] + [vw[4] * 1024.0, vw[5] * 1024.0])
    x = traj[:16_384 + 37]
    noise = np.random.default_rng(7).standard_normal((100, m.E)).astype(np.float32)
    sym, counts = m.symbolize(x, noise_vector=noise, return_counts=True)
    enc = om.encode(m.info_bott_encoder.get_weights(), x, m.n_freq)
    lg = om.vq_logits(m.vector_quantization_network.get_weights(), enc[:, :m.E], enc[:, m.E:], noise)
    ref = np.uint8(np.mean(np.argmax(lg, -1), 0) > 0.5)
    top2 = np.sort(lg, -1)[..., -2:]
    near = np.any(top2[..., 1] - top2[..., 0] < 1e-3, axis=0)
    assert near.mean() <= 1e-3, near.mean()
    assert np.array_equal(sym[~near], ref[~near])
    assert counts.sum(1).tolist() == [100] * len(x)
    m.vector_quantization_network.set_weights(vw)


def test_symbolize_a5_symbols_and_counts_match_oracle():
    """A = 5: logits in two lane groups, symbols >= 4 in the counts, the mean-argmax rule (not a vote) in sym"""
    m = MeasurementIB(2, alphabet_size=5, information_bottleneck_embedding_dimension=17, noise_seed=0, init_seed=3)
    x = _ikeda(3000, seed=2)
    noise = np.random.default_rng(8).standard_normal((100, m.E)).astype(np.float32)
    sym, counts = m.symbolize(x, noise_vector=noise, return_counts=True)
    enc = om.encode(m.info_bott_encoder.get_weights(), x, m.n_freq)
    lg = om.vq_logits(m.vector_quantization_network.get_weights(), enc[:, :m.E], enc[:, m.E:], noise)
    am = np.argmax(lg, -1)
    top2 = np.sort(lg, -1)[..., -2:]
    # an untrained partition: near-ties (top two within 1e-5 of the draw's largest |logit|, where the fp32 encoder and the
    # fp64 oracle may disagree) exclude a few points in a thousand
    near = np.any(top2[..., 1] - top2[..., 0] < 1e-5 * np.abs(lg).max(-1), axis=0)
    assert near.mean() <= 1e-2, (near.mean(), "near-tie exclusions above 1 %")
    ref_counts = np.stack([(am == a).sum(0) for a in range(5)], 1)
    assert np.array_equal(counts[~near], ref_counts[~near])
    assert np.array_equal(sym[~near], np.uint8(np.mean(am, 0) > 0.5)[~near])
    assert counts.sum(1).tolist() == [100] * len(x)
    assert counts[:, 4].any() and counts[:, 0].any(), "symbols of both lane groups are drawn"


def test_symbolize_is_bit_identical_across_runs_chunks_and_noise_source(trained):
    m, traj = trained
    x = traj[:50_001]
    a = m.symbolize(x, seed=3)
    b = m.symbolize(x, seed=3, chunk_size=4097)
    c = m.symbolize(x, noise_vector=np.random.default_rng(3).standard_normal((100, m.E)))
    _, cnt1 = m.symbolize(x, seed=3, return_counts=True)
    _, cnt2 = m.symbolize(x, seed=3, return_counts=True, chunk_size=1000)
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(cnt1, cnt2)


def test_unsupported_shape_is_refused():
    import ctypes
    from dib_amd.measurement import _MeasureDesc
    from dib_amd import _lib
    lib = _lib.load_library()
    d = _MeasureDesc()
    d.in_dim, d.E, d.H1, d.H2, d.A, d.L, d.act = 2, 32, 256, 256, 16, 12, 2
    assert lib.dib_measure_supported(ctypes.byref(d)) == 0
    d.H1, d.H2, d.E, d.A = 128, 128, 8, 2
    assert lib.dib_measure_supported(ctypes.byref(d)) == 1
    with pytest.raises(ValueError, match="envelope"):
        MeasurementIB(2, vector_quant_arch_spec=(256, 256), information_bottleneck_embedding_dimension=32)
    with pytest.raises(ValueError, match="envelope"):
        MeasurementIB(2, alphabet_size=17)


def test_mi_sandwich_bounds_of_the_ib_encoder_match_oracle(trained):
    """utils.estimate_mi_sandwich_bounds(model.info_bott_encoder, ...) (fit's I(U~;X)) vs the float64 restatement of reference
    utils.py:36-62 on the float64 encoder output, with the kernel's Philox key (seed, batch, row, feature 0)"""
    import dib_oracle as orc
    from dib_amd import utils
    m, traj = trained
    x = traj[:5000]
    got = utils.estimate_mi_sandwich_bounds(m.info_bott_encoder, x, evaluation_batch_size=1024, number_evaluation_batches=3, seed=6)
    rng = np.random.default_rng(6)
    w = m.info_bott_encoder.get_weights()
    est = []
    for b in range(3):
        rows = rng.permutation(len(x))[:1024]
        e = om.encode(w, x[rows], m.n_freq)
        u = orc.mi_sandwich_sample_u(e[:, :m.E], e[:, m.E:], 6, b, 0)
        est.append(orc.mi_sandwich_bounds_batch(e[:, :m.E], e[:, m.E:], u))
    ref = np.mean(np.asarray(est), 0)
    assert np.all(np.abs(np.asarray(got) - ref) <= 1e-4 * (1 + np.abs(ref))), (got, ref)
    assert got[0] <= got[1] + 1e-9


def test_fit_information_evaluations_and_early_stop():
    """fit's cell-10 bookkeeping: info_in = the sandwich bounds in bits every `evaluate_info_every` steps (equal to a direct
    estimate at the same weights), info_out = (log2 B - loss_prediction / ln 2) / L, and the stop once mean(info_in) reaches
    the stopping point"""
    from dib_amd import utils
    kw = CONFIGS["ragged_p1"]["kw"]
    traj = _traj("uniform", 4000, 1)
    ev = _traj("uniform", 3000, 1)
    m = MeasurementIB(**kw, noise_seed=1, init_seed=2)
    h = m.fit(traj, number_training_steps=12, batch_size=64, info_eval_data=ev, evaluate_info_every=4,
              info_evaluation_batch_size=256, info_evaluation_number_batches=2, info_stopping_point=1e9, seed=0)
    assert h["steps"] == 12 and len(h["loss"]) == 12 and len(h["info_in"]) == 3 and len(h["info_out"]) == 3
    direct = np.float32(utils.estimate_mi_sandwich_bounds(m.info_bott_encoder, ev, 256, 2, seed=11)) / np.log(2)
    np.testing.assert_allclose(h["info_in"][-1], direct, rtol=1e-6, atol=1e-9)
    assert all(np.all(np.isfinite(i)) and i[0] <= i[1] + 1e-6 for i in h["info_in"])
    assert all(np.isfinite(o) and o <= np.log2(64) / m.L + 1e-6 for o in h["info_out"])
    # the loss of the evaluated step carries loss_prediction: info_out restates it
    m2 = MeasurementIB(**kw, noise_seed=1, init_seed=2)
    h2 = m2.fit(traj, number_training_steps=12, batch_size=64, info_eval_data=ev, evaluate_info_every=4,
                info_evaluation_batch_size=256, info_evaluation_number_batches=2, info_stopping_point=-1.0, seed=0)
    assert h2["steps"] == 4 and len(h2["info_in"]) == 1 and len(h2["loss"]) == 4
    np.testing.assert_array_equal(h2["loss"], h["loss"][:4])
    np.testing.assert_array_equal(h2["info_in"][0], h["info_in"][0])
