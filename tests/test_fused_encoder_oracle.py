"""CPU: the float64 oracle of the encoder bank alone (tests/_oracle_fused_encoder.py) pinned to dib_oracle.forward / backward, the
shape arithmetic the cases of tests/test_gpu_fused_envelope.py rest on (grid, trips, tails, probe rows), the knife-edge guard of the
case builder, and the float32-arithmetic figures that module's tolerances are 8 x of, re-measured here."""
import numpy as np
import pytest

import dib_oracle as orc
import _oracle_fused_encoder as fe
from _helpers import SPECS, random_params


@pytest.mark.parametrize("name", ["boolean4_32x32", "fused_leaky"])
def test_encoder_oracle_is_dib_oracle_restricted_to_the_encoder_bank(name):
    """the same forward tensors, and - fed the g_u that dib_oracle.backward returns - the same six gradient blocks per feature"""
    spec, B, beta = SPECS[name], 37, 0.37
    F, E = spec.number_features, spec.feature_embedding_dimension
    p = random_params(spec, 5)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B, sum(spec.feature_dimensionalities)))
    y = rng.integers(0, 2, (B, 1)).astype(np.float64)
    eps = orc.philox_normal_all(3, 2, np.arange(B), F, E)
    c = orc.forward(spec, p, x, eps)
    _, grads, g_u = orc.backward(spec, p, x, y, c, beta, "bce_logits")
    fw = fe.encoder_forward(spec, p, x, eps)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * (1.0 + np.abs(b).max())
    for f in range(F):
        assert close(fw.P[f], c.enc_hidden[f][0]) and close(fw.h1[f], c.enc_hidden[f][1]) and close(fw.h2[f], c.enc_hidden[f][2])
    assert close(fw.mu, c.mu) and close(fw.logvar, c.logvar) and close(fw.u.reshape(B, F * E), c.u)
    assert close(fw.kl / B, c.kl)
    mine = fe.encoder_backward(spec, p, fw, g_u, beta, 1.0 / B)
    for f in range(F):
        for l in range(3):
            assert close(mine.enc_W[f][l], grads.enc_W[f][l]) and close(mine.enc_b[f][l], grads.enc_b[f][l]), (f, l)
    assert all(np.abs(w).max() == 0 for w in mine.int_W)


# name -> (gx, tiles, rows of the tail tile, encoder input widths, fused instantiation (H1, H2, E))
TABLE = {
    "trips_f64_h32_relu": (4, 6, 20, {5}, (32, 32, 32)),
    "trips_f64_h128_relu": (4, 5, 76, {5}, (128, 128, 32)),
    "trips_f128_h128_leaky_ragged": (2, 4, 232, {5, 10, 15}, (128, 128, 32)),
    "trips_f100_h32_leaky_in15": (2, 4, 32, {3, 9, 15}, (32, 32, 32)),
    "trips_f50_e16_relu": (5, 7, 1, {1, 7, 8, 9, 16}, (64, 64, 16)),
    "trips_f300_e8_linear": (1, 3, 88, {5}, (32, 32, 8)),
    "edges_single_trip_b32": (1, 1, 32, {5, 10, 15}, (32, 32, 32)),
    "edges_single_trip_b33": (1, 1, 33, {5, 10, 15}, (32, 32, 32)),
    "edges_single_trip_b256": (1, 1, 256, {5, 10, 15}, (32, 32, 32)),
    "edges_single_trip_b257": (2, 2, 1, {5, 10, 15}, (32, 32, 32)),
}


def test_cases_reach_what_their_table_says():
    assert set(TABLE) == set(fe.CASES)
    for name, (gx, tiles, tail, widths, inst) in TABLE.items():
        c = fe.CASES[name]
        spec, B, F = c.spec, c.B, c.spec.number_features
        assert fe.fused_gx(F, B) == gx and -(-B // 256) == tiles and B - (tiles - 1) * 256 == tail, name
        assert {spec.encoder_input_dim(f) for f in range(F)} == widths, name
        assert (*spec.feature_encoder_architecture, spec.feature_embedding_dimension) == inst
        # the backward's d(W1|b1) tile keeps row in_dim for the bias: inputs at most 15 wide (csrc/host/encoder.h fused_bwd_ok)
        assert c.backward == (inst[2] == 32 and max(widths) <= 15), name
        rows = fe.probe_rows(F, B)
        assert len(set(rows)) == len(rows) and all(0 <= r < B for r in rows) and {0, B - 1, (tiles - 1) * 256} <= set(rows), name
        if name.startswith("trips_"):
            # more tiles than workgroups: a second trip exists, its first tile's first and last row are probed, and the default
            # dispatch is past the row-tile regime
            assert tiles > gx and gx * 256 < B and {gx * 256, min(gx * 256 + 255, B - 1)} <= set(rows), name
            assert {0, 31, 32, 255, 256} <= set(rows)
            assert not fe.in_row_tile_regime(F, B) and c.path == "default", name
        else:
            assert c.path == "large_batch" and tiles == gx, name      # one trip per workgroup, nothing else going on
    # the tail tile arrives as a LATER trip of its workgroup (tile index >= gx) in every trips case
    for name in fe.TRIPS:
        gx, tiles = TABLE[name][:2]
        assert tiles - 1 >= gx, name
    # rows_valid of the tail tile's last live wave: 20 (partial), 12 after two full waves, 8, 32 exactly, 1, 24
    last_wave = {n: (TABLE[n][2] - 1) % 32 + 1 for n in fe.TRIPS}
    assert last_wave == {"trips_f64_h32_relu": 20, "trips_f64_h128_relu": 12, "trips_f128_h128_leaky_ragged": 8,
                         "trips_f100_h32_leaky_in15": 32, "trips_f50_e16_relu": 1, "trips_f300_e8_linear": 24}


def test_dead_units_are_exactly_zero_in_both_precisions():
    for name, c in fe.CASES.items():
        if not c.dead:
            continue
        bc = fe.build(name)
        H = c.spec.feature_encoder_architecture[0]
        for dt in (np.float32, np.float64):
            fw = fe.run(bc, "plain", dt, want=())[1]
            for f in (0, c.spec.number_features - 1):
                for z in (fw.z1[f], fw.z2[f]):
                    assert (z[:, [0, 31, H - 1]] == 0).all(), (name, f, dt)
        assert np.signbit(bc.p32.enc_b[0][0][31]) and np.signbit(bc.p32.enc_b[c.spec.number_features - 1][1][0])


def test_noise_in_float32_is_the_float64_noise_up_to_the_radius_uniforms_rounding():
    """dib_eps4's host expressions in float32 from the same Philox bits against dib_oracle.philox_normal: beyond the slack that
    _oracle_fused_encoder.noise_float32_slack derives from the rounding of u0, what is left is ordinary: the rounding of
    2 pi u1 (2^-24 x 2 pi x 1/2 of absolute angle error) times r <= 5.9, and of the logarithm - under 3e-6.  Without the slack the
    same comparison is off by more than 1e-5 on some draw: the term the GPU test's bound for u adds."""
    f32 = np.float32
    B, F, E = 1300, 64, 32
    ids = np.arange(B)
    eps64 = orc.philox_normal_all(fe.SEED, fe.STEP, ids, F, E)
    slack = fe.noise_float32_slack(ids, F, E, eps64)
    rows = np.asarray(ids, dtype=np.uint32).reshape(-1, 1)
    blk = np.arange(E // 4, dtype=np.uint32).reshape(1, -1)
    worst_plain, worst_left = 0.0, 0.0
    for f in range(F):
        x = orc.philox4x32_10(rows, np.uint32(f), blk, np.uint32(fe.STEP), fe.SEED & 0xFFFFFFFF, 0)
        u = [((xi >> np.uint32(8)).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0) for xi in x]
        r0, r1 = np.sqrt(f32(-2.0) * np.log(u[0])), np.sqrt(f32(-2.0) * np.log(u[2]))
        t0, t1 = f32(6.283185307179586) * u[1], f32(6.283185307179586) * u[3]
        z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)
        assert z.dtype == f32
        d = np.abs(z.reshape(B, E).astype(np.float64) - eps64[:, f])
        worst_plain = max(worst_plain, float(d.max()))
        worst_left = max(worst_left, float((d - slack[:, f]).max()))
    print("float32 noise against float64: largest difference", worst_plain, "beyond the slack", worst_left)
    assert worst_left <= 3e-6 and worst_plain > 1e-5


def test_figures_the_gpu_tolerances_rest_on():
    """Over every variant of every case: the oracle in float32 arithmetic against itself in float64 - per quantity the largest
    max|f32 - f64| / max|f64| (tests/test_gpu_fused_envelope.py RATIO32_*), the largest |z32 - z64| of a hidden pre-activation
    (GUARD = 8 x), the redraw rounds the builder took, and that no pre-activation of a built case lies inside the guard."""
    import test_gpu_fused_envelope as t
    fig = dict(fwd=0.0, kl=0.0, dense=0.0, probe=0.0)
    zdiff, rounds = 0.0, 0
    for name, mode in fe.VARIANTS:
        bc = fe.build(name)
        spec = bc.case.spec
        rounds = max(rounds, bc.redraw_rounds)
        _, f64, g64 = fe.run(bc, mode, np.float64)
        _, f32, g32 = fe.run(bc, mode, np.float32)
        if spec.activation_fn in ("relu", "leaky_relu") and mode == "plain":
            p64 = bc.p32.astype(np.float64)
            assert fe._near_edge(spec, p64, np.asarray(bc.x, dtype=np.float64)) == [], name      # every row of x, the padding too
        for a, b in zip(f32.z1 + f32.z2, f64.z1 + f64.z2):
            zdiff = max(zdiff, float(np.abs(a - b).max()))
            if spec.activation_fn in ("relu", "leaky_relu"):
                assert ((a > 0) == (b > 0)).all(), (name, mode)       # what the guard is for: the float32 masks are the float64 ones
        as_dict = lambda fw: dict(h1=fw.h1, h2=fw.h2, mu=fw.mu, logvar=fw.logvar, u=fw.u)
        e = fe.worst(fe.forward_errors(spec, as_dict(f32), as_dict(f64)))
        kl = float((np.abs(f32.kl - f64.kl) / np.abs(f64.kl)).max())
        line = [f"{name}/{mode}: forward {e[0]:.3g} {e[1]}", f"KL {kl:.3g}"]
        fig["fwd"], fig["kl"] = max(fig["fwd"], e[0]), max(fig["kl"], kl)
        for kind in g64:
            e = fe.worst(fe.grad_errors(spec, g32[kind], g64[kind]))
            key = "probe" if kind == "probe" else "dense"       # the complement sums B - 9 rows: a dense block by its arithmetic
            fig[key] = max(fig[key], e[0])
            line.append(f"{kind} {e[0]:.3g} {e[1]}")
        print("; ".join(line))
    print("RATIO32_FWD", fig["fwd"], "RATIO32_KL", fig["kl"], "RATIO32_DENSE", fig["dense"], "RATIO32_PROBE", fig["probe"])
    print("largest |z32 - z64|", zdiff, "GUARD", fe.GUARD, "redraw rounds", rounds)
    assert fig["fwd"] <= t.RATIO32_FWD and fig["kl"] <= t.RATIO32_KL
    assert fig["dense"] <= t.RATIO32_DENSE and fig["probe"] <= t.RATIO32_PROBE
    assert 8 * zdiff <= fe.GUARD
    assert rounds <= fe.MAX_REDRAW_ROUNDS
    # no bound looser than the parity test's (tests/test_gpu_parity.py: 2e-4 forward, 3e-4 of a gradient block's largest entry)
    assert 8 * t.RATIO32_FWD <= 2e-4 and 8 * t.RATIO32_KL <= 2e-4 and 8 * t.RATIO32_DENSE <= 3e-4 and 8 * t.RATIO32_PROBE <= 3e-4
