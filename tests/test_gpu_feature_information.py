"""Every feature's information bounds in one evaluation, on the device (include/dib_mi_features.h, csrc/dib_mi_features.h,
HipEngine.feature_information, DistributedIBNet.information_per_feature / fit(track_information=...),
InfoPerFeatureCallback(one_launch=True), train.py --info_bounds_frequency):
  - dib_mi_features_bounds against the float64 oracle (tests/_oracle_st_information.py) on the device's own samples, and the
    samples against the Philox reference with the per-feature keys, across the envelope (partial quads, E in registers and in
    LDS, sample tiles, row splits, row0 / step0 / feature0 offsets), every output inside NaN payloads between guard bands;
  - equality with the path it replaces: dib_mi_sandwich_rows per (feature, batch) on the contiguous slice;
  - far-apart Gaussians and duplicated rows; bit-identical replay, feature splits and batch splits; refusals that write nothing;
  - the model level on every dispatch path: the rows of evaluation_batch_rows, encodings against the oracle's encoder, bounds
    against the oracle on those encodings; the loop beyond the envelope; the callback, the tracked fit and the train script."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle_st_information as osi  # noqa: E402
import dib_oracle as orc  # noqa: E402
from _helpers import DISPATCH_PATHS, SPECS, dispatch_path, flat_to_params, spec_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -777.25
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED
SEED, STEP0, FEATURE0 = 77, 5, 3


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n):
    """(whole buffer, the n payload doubles inside it): NaN payload between sentinel guards"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all()


def _planes(rng, F, plane_rows, E, spread=1.0):
    """synthetic feature-major encoder outputs [F, plane_rows, 2E] (mu | raw logvar), built as test_gpu_st_information's _table"""
    mu = rng.standard_normal((F, plane_rows, E)) * spread
    lv = rng.standard_normal((F, plane_rows, E)) * 0.4 + 1.0
    return np.concatenate([mu, lv], -1).astype(np.float32)


def _bounds(lib, planes, n, nb, row0, seed=SEED, step0=STEP0, feature0=FEATURE0, want_rows=True, want_u=True, enc_d=None,
            f0=0, F=None):
    """one dib_mi_features_bounds call on planes[f0 : f0 + F] -> (out [F, nb, 2], lower [F, nb, n], upper, u [F, nb, n, E]);
    every output and the workspace sit between guard bands that must come back untouched"""
    Ft, plane_rows, E2 = planes.shape
    E = E2 // 2
    F = Ft - f0 if F is None else F
    need = int(lib.dib_mi_features_workspace_bytes(F, E, n, nb))
    assert need > 0 and need % 8 == 0, need
    wb, ws = _guarded(need // 8)
    assert ws.data_ptr() % 16 == 0
    enc_d = torch.tensor(planes, device="cuda") if enc_d is None else enc_d
    ob, out = _guarded(F * nb * 2)
    lb, lo = _guarded(F * nb * n)
    upb, up = _guarded(F * nb * n)
    ub, u = _guarded(F * nb * n * E)
    rc = lib.dib_mi_features_bounds(_p(enc_d[f0:]), plane_rows, row0, F, E, n, nb, seed, step0, feature0, _p(out),
                                    _p(lo) if want_rows else None, _p(up) if want_rows else None, _p(u) if want_u else None,
                                    _p(ws), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _guards_intact(wb, need // 8) and _guards_intact(ob, F * nb * 2) and _guards_intact(lb, F * nb * n)
    assert _guards_intact(upb, F * nb * n) and _guards_intact(ub, F * nb * n * E)
    assert not torch.isnan(out).any()
    if not want_rows:
        assert torch.isnan(lo).all() and torch.isnan(up).all()
    if not want_u:
        assert torch.isnan(u).all()
    return (out.cpu().numpy().reshape(F, nb, 2), lo.cpu().numpy().reshape(F, nb, n), up.cpu().numpy().reshape(F, nb, n),
            u.cpu().numpy().reshape(F, nb, n, E))


# F, E, n, nb, row0: partial quads (E = 1, 3), blocks of 8 dimensions that are not whole (4, 36), E in registers (<= 32, <= 64) and
# in LDS (68, 256), one sample tile and several, n that is no multiple of the tile, two row splits (n = 2100; up to 2047 rows are one)
CASES = [(3, 4, 70, 3, 5), (5, 1, 2, 1, 0), (2, 3, 65, 2, 1), (2, 32, 130, 2, 0), (2, 36, 64, 2, 7), (1, 68, 33, 1, 0),
         (1, 256, 20, 2, 0), (2, 32, 1024, 2, 0), (64, 32, 64, 1, 0), (2, 5, 300, 2, 3), (1, 132, 300, 1, 2), (2, 64, 130, 2, 1),
         (1, 4, 2100, 2, 1)]


@functools.lru_cache(maxsize=None)
def _case(F, E, n, nb, row0):
    """the planes of a case and the kernel's outputs on them (shared by the oracle test and the loop-equality test)"""
    rng = np.random.default_rng(1000 * E + n)
    planes = _planes(rng, F, row0 + nb * n + 9, E)
    return planes, _bounds(_lib(), planes, n, nb, row0)


@pytest.mark.parametrize("F,E,n,nb,row0", CASES)
def test_kernel_matches_oracle_across_the_envelope(F, E, n, nb, row0):
    """samples = mu + sigma Philox(seed, step0 + b, i, feature0 + f); per-row and per-group bounds against the log-sum-exp
    restatement on the device's samples"""
    planes, (out, lo, up, u) = _case(F, E, n, nb, row0)
    for f in range(F):
        for b in range(nb):
            x = planes[f, row0 + b * n: row0 + (b + 1) * n].astype(np.float64)
            mus, lvs = x[:, :E], x[:, E:]
            ref_u = mus + np.exp(lvs / 2.0) * orc.philox_normal(SEED, STEP0 + b, np.arange(n), FEATURE0 + f, E)
            assert np.abs(u[f, b] - ref_u).max() < 1e-5 * (1 + np.abs(ref_u).max()), (f, b)
            rlo, rup = osi.sandwich_rows_lse(mus, lvs, u[f, b])
            tol = 1e-8 * (1 + max(np.abs(rlo).max(), np.abs(rup).max()))
            assert np.abs(lo[f, b] - rlo).max() < tol and np.abs(up[f, b] - rup).max() < tol, (f, b)
            assert abs(out[f, b, 0] - rlo.mean()) < tol and abs(out[f, b, 1] - rup.mean()) < tol, (f, b)
            assert (lo[f, b] <= np.log(n) + 1e-9).all()


@pytest.mark.parametrize("F,E,n,nb,row0", CASES)
def test_kernel_equals_the_sandwich_rows_loop(F, E, n, nb, row0):
    """the path it replaces: dib_mi_sandwich_rows on the contiguous slice of (feature, batch), keyed seed, step0 + b, feature0 + f"""
    lib = _lib()
    planes, (out, lo, up, _) = _case(F, E, n, nb, row0)
    enc_d = torch.tensor(planes, device="cuda")
    ws = torch.empty(int(lib.dib_mi_workspace_bytes(n, E)) // 8 + 2, dtype=torch.float64, device="cuda")
    r = torch.empty((F, nb, 2, n), dtype=torch.float64, device="cuda")
    for f in range(F):
        for b in range(nb):
            eb = enc_d[f, row0 + b * n: row0 + (b + 1) * n]
            assert eb.is_contiguous()
            assert lib.dib_mi_sandwich_rows(_p(eb), n, E, SEED, STEP0 + b, FEATURE0 + f, _p(r[f, b, 0]), _p(r[f, b, 1]), _p(ws),
                                            _st()) == 0
    r = r.cpu().numpy()
    for f in range(F):
        for b in range(nb):
            scale = 1 + np.abs(r[f, b]).max()
            assert np.abs(lo[f, b] - r[f, b, 0]).max() <= 1e-12 * scale and np.abs(up[f, b] - r[f, b, 1]).max() <= 1e-12 * scale, (f, b)
            assert np.abs(out[f, b] - r[f, b].mean(axis=1)).max() <= 1e-12 * scale


def test_far_apart_gaussians_and_duplicated_rows():
    lib = _lib()
    n, E = 64, 32
    # far apart: mu = 100 x row index, unit variances - every other density underflows, the log-sum-exp leaves log n
    mu = (np.arange(2 * n + 3, dtype=np.float32)[:, None] * 100.0) * np.ones((1, E), dtype=np.float32)
    planes = np.stack([np.concatenate([mu, np.zeros_like(mu)], 1)] * 2)
    out, lo, up, u = _bounds(lib, planes, n, 2, 1)
    assert np.isfinite(lo).all() and np.abs(lo - np.log(64)).max() <= 1e-9
    assert not np.isnan(up).any() and not np.isnan(out).any() and not np.isnan(u).any()
    assert np.abs(out[..., 0] - np.log(64)).max() <= 1e-9 and (out[..., 1] > 1e3).all()
    # duplicates: a batch that repeats one row n times - all densities equal: lower = 0, upper = log(n / (n - 1))
    rng = np.random.default_rng(4)
    planes = _planes(rng, 2, 2 * n + 5, E)
    planes[:, 3:3 + n] = planes[:, 3:4]
    out, lo, up, _ = _bounds(lib, planes, n, 2, 3)
    assert np.abs(lo[:, 0]).max() <= 1e-9 and np.isfinite(up).all()
    assert np.abs(up[:, 0] - np.log(n / (n - 1.0))).max() <= 1e-9
    assert np.abs(lo[:, 1]).max() > 1e-3   # the second batch is ordinary rows


@pytest.mark.parametrize("F,E,n,nb,row0", [(5, 32, 300, 4, 2), (4, 3, 70, 3, 0), (3, 68, 40, 2, 1), (2, 64, 300, 2, 0), (2, 3, 2100, 2, 1)])
def test_replay_and_splits_are_bit_identical(F, E, n, nb, row0):
    lib = _lib()
    rng = np.random.default_rng(E + n)
    planes = _planes(rng, F, row0 + nb * n + 4, E)
    a = _bounds(lib, planes, n, nb, row0)
    b = _bounds(lib, planes, n, nb, row0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = _bounds(lib, planes, n, nb, row0, want_rows=False, want_u=False)
    assert np.array_equal(a[0], c[0])
    # features split over two calls: enc offset by the planes done, feature0 advanced
    k = F // 2
    f1 = _bounds(lib, planes, n, nb, row0, F=k)
    f2 = _bounds(lib, planes, n, nb, row0, feature0=FEATURE0 + k, f0=k)
    assert all(np.array_equal(x, np.concatenate([y, z], 0)) for x, y, z in zip(a, f1, f2))
    # batches split over two calls: row0 and step0 advanced
    k = nb // 2
    b1 = _bounds(lib, planes, n, k, row0)
    b2 = _bounds(lib, planes, n, nb - k, row0 + k * n, step0=STEP0 + k)
    assert all(np.array_equal(x, np.concatenate([y, z], 1)) for x, y, z in zip(a, b1, b2))


def test_refusals_return_their_code_and_write_nothing():
    lib = _lib()
    F, E, n, nb, rows = 2, 8, 16, 2, 40
    enc = torch.zeros((F, rows, 2 * E), dtype=torch.float32, device="cuda")
    wb, ws = _guarded(int(lib.dib_mi_features_workspace_bytes(F, E, n, nb)) // 8)
    ob, out = _guarded(F * nb * 2)
    lb, lo = _guarded(F * nb * n)
    upb, up = _guarded(F * nb * n)
    ub, u = _guarded(F * nb * n * E)
    z = ctypes.c_void_p(0)
    n0 = lib.dib_launch_count()

    def call(enc_p=_p(enc), plane_rows=rows, row0=0, F=F, E=E, n=n, nb=nb, out_p=_p(out), lo_p=_p(lo), up_p=_p(up), ws_p=_p(ws)):
        return lib.dib_mi_features_bounds(enc_p, plane_rows, row0, F, E, n, nb, 1, 0, 0, out_p, lo_p, up_p, _p(u), ws_p, _st())

    assert call(E=65) == UNSUPPORTED and call(E=260) == UNSUPPORTED and call(n=1) == UNSUPPORTED
    assert call(F=65536, nb=1) == UNSUPPORTED and call(F=256, nb=256) == UNSUPPORTED and call(n=16385) == UNSUPPORTED
    assert call(F=0) == ARG and call(E=0) == ARG and call(n=0) == ARG and call(nb=-1) == ARG
    assert call(enc_p=z) == ARG and call(out_p=z) == ARG and call(ws_p=z) == ARG
    assert call(ws_p=ctypes.c_void_p(ws.data_ptr() + 8)) == ARG            # not 16-byte aligned
    assert call(row0=rows - nb * n + 1) == ARG and call(row0=-1) == ARG and call(plane_rows=nb * n - 1) == ARG
    assert call(lo_p=z) == ARG and call(up_p=z) == ARG                     # only one of the two row outputs
    assert lib.dib_launch_count() == n0                                     # a refused call launches nothing
    torch.cuda.synchronize()
    for buf, payload, cnt in ((wb, ws, ws.numel()), (ob, out, out.numel()), (lb, lo, lo.numel()), (upb, up, up.numel()), (ub, u, u.numel())):
        assert _guards_intact(buf, cnt) and torch.isnan(payload).all()
    assert call(row0=rows - nb * n) == 0                                    # the last admissible row0
    assert lib.dib_launch_count() == n0 + 3                                 # table prep, tiled bounds, combine: whatever F and nb
    assert call(F=1, nb=1) == 0 and lib.dib_launch_count() == n0 + 6
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and _guards_intact(ob, out.numel()) and _guards_intact(wb, ws.numel())


# ---- model level --------------------------------------------------------------------------------------------------------
SMALL_12 = orc.DIBSpec([1, 2], [24, 16], [8], 1, feature_embedding_dimension=32)


def _model(spec, seed=3):
    import dib_amd
    return dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=1, init_seed=seed)


def _device_samples(lib, enc, n, nb, seed):
    """the samples dib_mi_features_bounds draws on encodings enc [F, nb n, 2E] with the model-level keys (seed, b, i, f): a
    replay of the evaluation's launch (bit-identical: test_replay_and_splits_are_bit_identical), with u_out"""
    out, lo, up, u = _bounds(lib, enc, n, nb, 0, seed=seed, step0=0, feature0=0)
    return out, u


def _check_model(spec, n_rows, bs, nb, seed):
    from dib_amd import utils
    lib = _lib()
    m = _model(spec)
    eng = m._ensure_engine()
    F, E = spec.number_features, spec.feature_embedding_dimension
    rng = np.random.default_rng(n_rows + bs)
    x = rng.standard_normal((n_rows, sum(spec.feature_dimensionalities))).astype(np.float32)
    got = m.information_per_feature(x, evaluation_batch_size=bs, number_evaluation_batches=nb, seed=seed, per_batch=True)
    assert got.shape == (F, nb, 2) and got.dtype == np.float64
    mean = m.information_per_feature(x, evaluation_batch_size=bs, number_evaluation_batches=nb, seed=seed)
    assert mean.shape == (F, 2) and np.array_equal(mean, got.mean(axis=1))
    rows = utils.evaluation_batch_rows(n_rows, bs, nb, seed)
    again, lo, up, enc = eng.feature_information(eng.to_device(x), rows.astype(np.int32), bs, nb, seed, 0, want_rows=True,
                                                 want_encodings=True)
    assert np.array_equal(again, got) and enc.shape == (F, nb * bs, 2 * E)
    # the encodings the evaluation used: the oracle's encoder on the rows of evaluation_batch_rows
    p = flat_to_params(m.param_blocks(), m.get_flat_weights(), spec)
    col = np.concatenate([[0], np.cumsum(spec.feature_dimensionalities)])
    for f in range(F):
        ref = orc.encode_feature(spec, p, f, x[rows.reshape(-1), col[f]: col[f + 1]].astype(np.float64))
        assert np.abs(enc[f] - ref).max() < 2e-4 * (1 + np.abs(ref).max()), f
    # the bounds: the float64 oracle on those encodings and the device's own samples (keys seed, b, i, f)
    kernel, u = _device_samples(lib, enc, bs, nb, seed)
    assert np.array_equal(kernel, got)
    for f in range(F):
        for b in range(nb):
            e = enc[f, b * bs: (b + 1) * bs].astype(np.float64)
            ref_u = e[:, :E] + np.exp(e[:, E:] / 2.0) * orc.philox_normal(seed, b, np.arange(bs), f, E)
            assert np.abs(u[f, b] - ref_u).max() < 1e-5 * (1 + np.abs(ref_u).max()), (f, b)
            rlo, rup = osi.sandwich_rows_lse(e[:, :E], e[:, E:], u[f, b])
            scale = 1 + max(np.abs(rlo).max(), np.abs(rup).max())
            assert np.abs(lo[f, b] - rlo).max() < 1e-8 * scale and np.abs(up[f, b] - rup).max() < 1e-8 * scale, (f, b)
            assert abs(got[f, b, 0] - rlo.mean()) < 1e-8 * scale and abs(got[f, b, 1] - rup.mean()) < 1e-8 * scale, (f, b)
    return m, x, got


@pytest.mark.parametrize("path", DISPATCH_PATHS)
@pytest.mark.parametrize("bs,nb", [(100, 3), (1024, 2)])
@pytest.mark.parametrize("name", ["pendulum_ragged", "small_12"])
def test_information_per_feature_matches_oracle_on_every_dispatch_path(name, bs, nb, path):
    spec = SPECS[name] if name in SPECS else SMALL_12
    with dispatch_path(path):
        _check_model(spec, 1500, bs, nb, seed=9)


def test_chunks_of_batches_do_not_change_the_bits():
    """4 batches of 100 rows as one chunk, as chunks of 2 batches and batch by batch (with a tail chunk of another size)"""
    m = _model(SMALL_12)
    eng = m._ensure_engine()
    x = np.random.default_rng(0).standard_normal((700, 3)).astype(np.float32)
    ref = m.information_per_feature(x, 100, 5, seed=2, per_batch=True)
    for rows_per_encode in (200, 100, 350):
        eng.FEATURE_INFORMATION_ROWS = rows_per_encode
        assert np.array_equal(m.information_per_feature(x, 100, 5, seed=2, per_batch=True), ref), rows_per_encode


def test_validation_set_smaller_than_the_batch_draws_with_replacement():
    m, x, got = _check_model(SMALL_12, 60, 100, 2, seed=5)
    from dib_amd import utils
    rows = utils.evaluation_batch_rows(60, 100, 2, 5)
    assert all(len(set(r)) < 100 for r in rows)
    assert np.isfinite(got).all() and (got[..., 0] <= np.log(100) + 1e-9).all() and (got[..., 0] <= got[..., 1] + 1e-9).all()


def test_all_features_equal_the_per_feature_loop_and_a_shape_beyond_the_envelope_takes_it():
    """E = 65 is outside dib_mi_features_bounds' envelope: information_per_feature silently runs the launches of the loop
    utils.estimate_mi_sandwich_bounds itself (same kernels, same inputs: 1e-12).  E = 32 takes the one-launch path: its
    encodings come from the encoder bank, the loop's from dib_encode_deterministic - two float32 kernels, each within 2e-4 of
    the float64 encoder (test_encode_deterministic_and_bhattacharyya) - so the two agree only as far as the bounds carry
    that difference: |d bound / d (mu, logvar)| is at most a few |u - mu| / sigma per dimension, over 32 dimensions of O(1)
    encodings ~1e2, times the ~1e-6 two float32 evaluations of a 3-layer encoder differ by: 1e-3 is an order above it."""
    from dib_amd import utils
    lib = _lib()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((400, 3)).astype(np.float32)
    for E, tol in ((32, 1e-3), (65, 1e-12)):
        spec = orc.DIBSpec([1, 2], [24, 16], [8], 1, feature_embedding_dimension=E)
        assert lib.dib_mi_features_supported(2, E, 128, 1) == (1 if E == 32 else 0)
        m = _model(spec)
        got = m.information_per_feature(x, 128, 3, seed=4)
        assert got.shape == (2, 2) and np.isfinite(got).all()
        for f, xf in enumerate((x[:, :1], x[:, 1:])):
            ref = utils.estimate_mi_sandwich_bounds(m.feature_encoders[f], xf, 128, 3, seed=4)
            assert np.abs(got[f] - ref).max() <= tol * (1 + np.abs(ref).max()), (E, f, got[f], ref)


def _circuit_c():
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)  # SI circuit (c)
    return np.tile(x, (8, 1)).astype(np.float32), np.tile(y, 8).astype(np.float32)


def _circuit_model():
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = 3e-3
    model.compile(optimizer=opt, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    return model


def test_callback_in_one_launch_fills_bounds_like_information_per_feature():
    import dib_amd
    x, y = _circuit_c()
    model = _circuit_model()
    cb = dib_amd.InfoPerFeatureCallback(2, x[:100], info_bound_batch_size=64, info_bound_number_batches=3, one_launch=True)
    model.fit(x, y, epochs=3, batch_size=48, callbacks=[cb], verbose=False)
    assert cb.epochs == [0, 2] and len(cb.bounds) == 2 * 4
    ref = model.information_per_feature(x[:100], 64, 3, seed=2)   # the parameters are those of the end of epoch 2
    assert cb.bounds[4:] == [[float(lo), float(up)] for lo, up in ref]   # the reference's flat order: feature-major per evaluation
    assert all(isinstance(v, float) for pair in cb.bounds for v in pair)
    assert dib_amd.InfoPerFeatureCallback(1, x[:10]).one_launch is False


def test_tracked_fit_trains_exactly_like_the_untracked_fit():
    import dib_amd
    x, y = _circuit_c()
    hists, models, cbs = [], [], []
    for track in (None, dict(every=2, evaluation_batch_size=32, number_evaluation_batches=2)):
        model = _circuit_model()
        cb = dib_amd.InfoBottleneckAnnealingCallback(1e-3, 1.0, 1, 3)
        hists.append(model.fit(x, y, epochs=5, shuffle=True, batch_size=48, callbacks=[cb], verbose=False,
                               validation_data=(x[:40], y[:40]), track_information=track))
        models.append(model)
        cbs.append(cb)
    a, b = hists
    assert a.information is None
    info = b.information
    assert info["epochs"] == [0, 2, 4]
    assert info["beta"] == [float(cbs[1].beta_at(e)) for e in (0, 2, 4)]
    assert info["bounds"].shape == (3, 4, 2) and np.isfinite(info["bounds"][..., 0]).all()
    assert (info["bounds"][..., 0] <= np.log(32) + 1e-9).all() and (info["bounds"][..., 0] <= info["bounds"][..., 1] + 1e-9).all()
    assert np.array_equal(info["bounds"][2], models[1].information_per_feature(x[:40], 32, 2, seed=4))
    assert a.history == b.history and a.epoch == b.epoch and all(len(v) == 5 for v in b.history.values())
    ea, eb = models[0]._ensure_engine(), models[1]._ensure_engine()
    assert torch.equal(ea.params, eb.params) and torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.adam_v, eb.adam_v)
    assert torch.equal(ea.t_dev, eb.t_dev) and models[0]._step == models[1]._step
    with pytest.raises(ValueError):
        _circuit_model().fit(x, y, epochs=1, batch_size=48, verbose=False, track_information=dict(every=1))   # no inputs
    with pytest.raises(ValueError):
        _circuit_model().fit(x, y, epochs=1, batch_size=48, verbose=False, track_information=dict(x=x[:40], frequency=1))


def test_train_script_writes_the_information_bounds(tmp_path):
    from dib_amd import train
    hist = train.main(["--dataset", "boolean_circuit", "--number_pretraining_epochs", "2", "--number_annealing_epochs", "3",
                       "--batch_size", "128", "--artifact_outdir", str(tmp_path), "--info_bounds_frequency", "2",
                       "--feature_encoder_architecture", "32", "32", "--integration_network_architecture", "64",
                       "--feature_embedding_dimension", "8"])
    F = len(hist.model.feature_dimensionalities)
    f = np.load(tmp_path / "info_bounds.npz")
    assert f["bounds"].shape == (3, F, 2) and list(f["epochs"]) == [0, 2, 4] and f["beta"].shape == (3,)
    assert np.array_equal(f["bounds"], hist.information["bounds"]) and np.isfinite(f["bounds"][..., 0]).all()
    assert (tmp_path / "distributed_info_plane_mi.png").stat().st_size > 1000
    assert (tmp_path / "distributed_info_plane.png").exists() and (tmp_path / "history.npz").exists()
