"""Every feature's compression matrix in one evaluation, on the device (include/dib_compression.h, csrc/dib_compression.h,
HipEngine.compression_matrices, DistributedIBNet.compression_matrices, SaveCompressionMatricesCallback(one_launch=True),
train.py --compression_matrices_one_launch and --save_compression_matrices_frequency on the InfoNCE loop):
  - dib_compression_matrices against the float64 oracle (tests/_oracle_compression.py) across the envelope - E 1 .. 256, ragged
    counts around the 64-row tile, n_max no multiple of it, row0 > 0, plane_rows > row0 + n_max - every output inside NaN
    payloads between guard bands; exact zeros outside counts[f]; bit-symmetry;
  - bit-identical replay, placement (plane index, F, n_max, row0) and feature splits;
  - dib_compression_gather against numpy; refusals that write nothing; an out-of-range row table raises before any launch;
  - the model level on every dispatch path against the float64 chain, with the per-feature loop as the yardstick; the launch
    count independent of F; the loop beyond the envelope; the callback; both script paths."""
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
import _oracle_compression as ocm  # noqa: E402
import dib_oracle as orc  # noqa: E402
from _helpers import DISPATCH_PATHS, dispatch_path, flat_to_params, spec_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -777.25
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED
T = 64                      # csrc/dib_compression.h DIB_CMP_TILE
MAX_E, MAX_ROWS, MAX_F = 256, 2048, 65535   # include/dib_compression.h DIB_COMPRESSION_MAX_*


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n):
    """(whole buffer, the n payload floats inside it): NaN payload between sentinel guards"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:GUARD] == SENTINEL).all() and (b[GUARD + n:] == SENTINEL).all()


def _planes(rng, F, plane_rows, E):
    """synthetic feature-major encoder outputs [F, plane_rows, 2E]: mu ~ N(0, 1), logvar uniform in [-12, 4]"""
    mu = rng.standard_normal((F, plane_rows, E))
    lv = rng.uniform(-12.0, 4.0, (F, plane_rows, E))
    return np.concatenate([mu, lv], -1).astype(np.float32)


def _matrices(lib, planes, counts, n_max, row0, f0=0, F=None, want_dist=True, want_comp=True):
    """one dib_compression_matrices call on planes[f0 : f0 + F] -> (dist, comp) float32 [F, n_max, n_max]; both outputs sit
    between guard bands that must come back untouched, and an output that was not asked for stays NaN"""
    Ft, plane_rows, E2 = planes.shape
    F = Ft - f0 if F is None else F
    enc_d = torch.tensor(planes, device="cuda")
    cnt_d = torch.tensor(np.asarray(counts, dtype=np.int32), device="cuda")
    db, dist = _guarded(F * n_max * n_max)
    cb, comp = _guarded(F * n_max * n_max)
    n0 = lib.dib_launch_count()
    rc = lib.dib_compression_matrices(_p(enc_d[f0:]), plane_rows, row0, F, E2 // 2, _p(cnt_d[f0:]), n_max,
                                      _p(dist) if want_dist else None, _p(comp) if want_comp else None, _st())
    assert rc == 0, rc
    assert lib.dib_launch_count() == n0 + 1   # one launch whatever F is
    torch.cuda.synchronize()
    assert _guards_intact(db, dist.numel()) and _guards_intact(cb, comp.numel())
    for want, out in ((want_dist, dist), (want_comp, comp)):
        assert not torch.isnan(out).any() if want else torch.isnan(out).all()
    return dist.cpu().numpy().reshape(F, n_max, n_max), comp.cpu().numpy().reshape(F, n_max, n_max)


# ragged counts around the tile: 1, T - 1, T, T + 1, 2 T + 3 (and an empty feature, and a count beyond n_max that is clamped)
COUNTS = (1, T - 1, T, T + 1, 2 * T + 3, 0, 5000)
# E, n_max (no multiple of T), row0, rows of the planes beyond row0 + n_max
CASES = [(1, 2 * T + 3, 0, 0), (3, 2 * T + 9, 5, 7), (32, 2 * T + 3, 1, 3), (33, 2 * T + 5, 2, 1), (256, 2 * T + 3, 3, 2)]


@functools.lru_cache(maxsize=None)
def _case(E, n_max, row0, extra):
    """the planes of a case and the kernel's outputs on them"""
    rng = np.random.default_rng(1000 * E + n_max)
    planes = _planes(rng, len(COUNTS), row0 + n_max + extra, E)
    dist, comp = _matrices(_lib(), planes, COUNTS, n_max, row0)
    return planes, dist, comp


@pytest.mark.parametrize("E,n_max,row0,extra", CASES)
def test_kernel_matches_the_float64_oracle(E, n_max, row0, extra):
    """|dist - dist64| <= (E + 16) 2^-24 A_ij per entry, A_ij the float64 sum of the absolute values of every term of the formula:
    E sequential float32 additions of terms bounded by A, plus a few ulp each for expf, logf (both documented at 1 ulp in the HIP
    math API), the correctly rounded division and the products.  |comp - exp(-dist64)| <= the same bound (|d e^-D| <= |dD|)
    + 2^-22."""
    planes, dist, comp = _case(E, n_max, row0, extra)
    dist64, comp64, A = ocm.plane_matrices(planes, COUNTS, row0, n_max)
    bound = (E + 16) * 2.0 ** -24 * A
    for f, c in enumerate(COUNTS):
        c = min(c, n_max)
        ed, ec = np.abs(dist[f] - dist64[f]), np.abs(comp[f] - comp64[f])
        worst = np.unravel_index(np.argmax(ed - bound[f]), ed.shape)
        print(f"E={E} count={c}: max |dist - dist64| = {ed.max():.3e} (largest excess over the bound {np.max(ed - bound[f]):.3e} at "
              f"{worst}, A = {A[f][worst]:.3e}), max |comp - comp64| = {ec.max():.3e}")
        assert (ed <= bound[f]).all(), (f, c, float(ed.max()))
        assert (ec <= bound[f] + 2.0 ** -22).all(), (f, c, float(ec.max()))
        # exactly 0.0f (not -0.0f) outside the feature's sample
        outside = np.ones((n_max, n_max), dtype=bool)
        outside[:c, :c] = False
        for out in (dist[f], comp[f]):
            assert (out[outside].view(np.uint32) == 0).all(), (f, c)


@pytest.mark.parametrize("E,n_max,row0,extra", CASES)
def test_matrices_equal_their_transposes_bit_for_bit(E, n_max, row0, extra):
    _, dist, comp = _case(E, n_max, row0, extra)
    for out in (dist, comp):
        assert np.array_equal(out.view(np.uint32), out.transpose(0, 2, 1).view(np.uint32))


def test_one_output_alone_gives_the_same_bits():
    E, n_max, row0, extra = CASES[1]
    planes, dist, comp = _case(E, n_max, row0, extra)
    lib = _lib()
    d_only, _ = _matrices(lib, planes, COUNTS, n_max, row0, want_comp=False)
    _, c_only = _matrices(lib, planes, COUNTS, n_max, row0, want_dist=False)
    assert np.array_equal(d_only.view(np.uint32), dist.view(np.uint32)) and np.array_equal(c_only.view(np.uint32), comp.view(np.uint32))


def test_replay_placement_and_feature_splits_are_bit_identical():
    lib = _lib()
    E, n_max, row0, extra = CASES[3]
    planes, dist, comp = _case(E, n_max, row0, extra)
    bits = lambda a: a.view(np.uint32)
    # a replay
    d2, c2 = _matrices(lib, planes, COUNTS, n_max, row0)
    assert np.array_equal(bits(d2), bits(dist)) and np.array_equal(bits(c2), bits(comp))
    # a split of the features over two calls
    for f0, F in ((0, 2), (2, len(COUNTS) - 2)):
        dp, cp = _matrices(lib, planes, COUNTS, n_max, row0, f0=f0, F=F)
        assert np.array_equal(bits(dp), bits(dist[f0:f0 + F])) and np.array_equal(bits(cp), bits(comp[f0:f0 + F]))
    # feature 3's rows (T + 1 of them: two tiles) alone in plane 0 of a one-feature call, with another n_max and row0 = 0 ...
    c = COUNTS[3]
    own = planes[3:4, row0: row0 + c]
    d1, c1 = _matrices(lib, np.ascontiguousarray(own), [c], c, 0)
    assert np.array_equal(bits(d1[0]), bits(dist[3, :c, :c])) and np.array_equal(bits(c1[0]), bits(comp[3, :c, :c]))
    # ... and as plane 5 of 9 with a larger n_max and row0
    big = _planes(np.random.default_rng(1), 9, 11 + 3 * T + 2, E)
    big[5, 11: 11 + c] = own[0]
    d9, c9 = _matrices(lib, big, [7, 1, 200, 3, 64, c, 9, 130, 2], 3 * T + 1, 11)
    assert np.array_equal(bits(d9[5, :c, :c]), bits(dist[3, :c, :c])) and np.array_equal(bits(c9[5, :c, :c]), bits(comp[3, :c, :c]))


def _engine(dims, E=8, enc=(32, 32)):
    from dib_amd.engine import HipEngine
    return HipEngine(dims, list(enc), [16], 1, feature_embedding_dimension=E)


def test_gather_equals_numpy():
    """dims [2, 1, 3], ldx > sum_d, repeated rows and rows padded with the feature's first index"""
    lib = _lib()
    eng = _engine([2, 1, 3])
    rng = np.random.default_rng(0)
    N, n_max, ldx = 37, 9, 8
    wide = rng.standard_normal((N, ldx)).astype(np.float32)
    rows = np.stack([np.r_[rng.integers(0, N, 5), [3, 3, 3, 3]], np.r_[[36, 0, 36, 0], np.full(5, 36)], rng.permutation(N)[:9]]).astype(np.int32)
    xb, xg = _guarded(n_max * 6)
    wide_d, rows_d = torch.tensor(wide, device="cuda"), torch.tensor(rows, device="cuda")
    n0 = lib.dib_launch_count()
    rc = lib.dib_compression_gather(eng.layout, _p(wide_d), ldx, N, _p(rows_d), n_max, _p(xg), _st())
    assert rc == 0 and lib.dib_launch_count() == n0 + 1
    torch.cuda.synchronize()
    want = np.concatenate([wide[rows[0], 0:2], wide[rows[1], 2:3], wide[rows[2], 3:6]], axis=1)
    assert np.array_equal(xg.cpu().numpy().reshape(n_max, 6), want) and _guards_intact(xb, n_max * 6)
    # an index outside [0, n_rows) is clamped by the kernel: a wrong row, never out of bounds
    bad = rows.copy()
    bad[0, 0], bad[2, 8] = -5, N + 100
    bad_d = torch.tensor(bad, device="cuda")
    rc = lib.dib_compression_gather(eng.layout, _p(wide_d), ldx, N, _p(bad_d), n_max, _p(xg), _st())
    assert rc == 0
    torch.cuda.synchronize()
    clamped = np.clip(bad, 0, N - 1)
    want = np.concatenate([wide[clamped[0], 0:2], wide[clamped[1], 2:3], wide[clamped[2], 3:6]], axis=1)
    assert np.array_equal(xg.cpu().numpy().reshape(n_max, 6), want) and _guards_intact(xb, n_max * 6)


def test_row_table_out_of_range_raises_before_any_launch():
    lib = _lib()
    eng = _engine([2, 1, 3])
    x = eng.to_device(np.zeros((20, 6), dtype=np.float32))
    rows = np.zeros((3, 4), dtype=np.int32)
    torch.cuda.synchronize()
    n0 = lib.dib_launch_count()
    for r, c in ((20, 4), (-1, 4), (0, 5), (0, -1)):
        bad = rows.copy()
        bad[1, 2] = r
        with pytest.raises(ValueError):
            eng.compression_matrices(x, bad, np.array([4, c, 4], dtype=np.int32))
    with pytest.raises(ValueError):
        eng.compression_matrices(x, rows[:2], np.array([4, 4], dtype=np.int32))   # a table for another F
    assert lib.dib_launch_count() == n0
    got = eng.compression_matrices(x, rows, np.array([4, 2, 0], dtype=np.int32))
    assert got.shape == (3, 4, 4) and got.dtype == np.float32
    assert np.allclose(got[0], 1, atol=1e-6) and np.allclose(got[1, :2, :2], 1, atol=1e-6) and (got[1, 2:] == 0).all() and (got[2] == 0).all()


def test_refusals_return_their_code_and_write_nothing():
    lib = _lib()
    F, E, n_max, rows = 3, 8, 16, 40
    enc = torch.zeros((F, rows, 2 * E), dtype=torch.float32, device="cuda")
    cnt = torch.full((F,), n_max, dtype=torch.int32, device="cuda")
    db, dist = _guarded(F * n_max * n_max)
    cb, comp = _guarded(F * n_max * n_max)
    z = ctypes.c_void_p(0)
    n0 = lib.dib_launch_count()

    def call(enc_p=_p(enc), plane_rows=rows, row0=0, F=F, E=E, cnt_p=_p(cnt), n_max=n_max, dist_p=_p(dist), comp_p=_p(comp)):
        return lib.dib_compression_matrices(enc_p, plane_rows, row0, F, E, cnt_p, n_max, dist_p, comp_p, _st())

    assert call(E=MAX_E + 1) == UNSUPPORTED and call(n_max=MAX_ROWS + 1, plane_rows=MAX_ROWS + 1) == UNSUPPORTED
    assert call(F=MAX_F + 1) == UNSUPPORTED
    assert call(F=0) == ARG and call(E=0) == ARG and call(n_max=0) == ARG and call(F=-2) == ARG
    assert call(enc_p=z) == ARG and call(cnt_p=z) == ARG and call(dist_p=z, comp_p=z) == ARG
    assert call(row0=rows - n_max + 1) == ARG and call(row0=-1) == ARG and call(plane_rows=n_max - 1) == ARG and call(plane_rows=0) == ARG

    eng = _engine([2, 1, 3], E=E)
    x = torch.zeros((10, 6), dtype=torch.float32, device="cuda")
    tab = torch.zeros((3, n_max), dtype=torch.int32, device="cuda")
    gb, xg = _guarded(n_max * 6)

    def gather(l=eng.layout, x_p=_p(x), ldx=6, n_rows=10, tab_p=_p(tab), n_max=n_max, xg_p=_p(xg)):
        return lib.dib_compression_gather(l, x_p, ldx, n_rows, tab_p, n_max, xg_p, _st())

    assert gather(l=None) == ARG and gather(x_p=z) == ARG and gather(tab_p=z) == ARG and gather(xg_p=z) == ARG
    assert gather(ldx=5) == ARG and gather(n_rows=0) == ARG and gather(n_max=0) == ARG and gather(n_max=MAX_ROWS + 1) == UNSUPPORTED
    assert lib.dib_launch_count() == n0                                     # a refused call launches nothing
    torch.cuda.synchronize()
    for buf, payload in ((db, dist), (cb, comp), (gb, xg)):
        assert _guards_intact(buf, payload.numel()) and torch.isnan(payload).all()
    assert call(row0=rows - n_max) == 0 and call(dist_p=z) == 0 and gather() == 0   # the last admissible row0; one output; the gather
    assert lib.dib_launch_count() == n0 + 3
    torch.cuda.synchronize()
    assert torch.isfinite(dist).all() and torch.isfinite(comp).all() and (xg == 0).all()
    assert _guards_intact(db, dist.numel()) and _guards_intact(cb, comp.numel()) and _guards_intact(gb, xg.numel())


# ---- model level --------------------------------------------------------------------------------------------------------
SMALL = orc.DIBSpec([2, 1, 1], [32, 32], [16], 1, feature_embedding_dimension=8)
SHOWN = 40


def _model(spec, seed=3):
    import dib_amd
    return dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=1, init_seed=seed)


def _inputs(dims, n=300, seed=0):
    """continuous columns, the last one with 3 unique values (the histogram mode of the display rule)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, sum(dims))).astype(np.float32)
    x[:, -1] = rng.integers(0, 3, n).astype(np.float32) - 1.0
    return x


def _loop(model, x, dims, shown, seed):
    """today's per-feature loop under one seeded generator -> (matrices, indices): the indices from a second generator in the
    same state (save_compression_matrices does not return them)"""
    from dib_amd import visualization
    rng, rng_idx = np.random.RandomState(seed), np.random.RandomState(seed)
    split = np.split(x, np.cumsum(dims)[:-1], axis=-1)
    mats = [visualization.save_compression_matrices(model.feature_encoders[f], xf, None, inp_features_raw=xf,
                                                    max_number_to_display=shown, model=model, rng=rng) for f, xf in enumerate(split)]
    idx = [visualization.select_display_inputs(xf, shown, rng_idx)[0] for xf in split]
    return mats, idx


@pytest.mark.parametrize("path", DISPATCH_PATHS)
def test_model_matches_the_float64_chain_no_worse_than_the_loop(path):
    """err_new <= 2 err_loop + 1e-6 for the largest |matrix - float64 chain| of the two paths on the same rows: the loop is
    the yardstick, the factor 2 allows for the different summation orders of two float32 encoders (the bank kernel and
    dib_encode_deterministic)."""
    spec, dims = SMALL, SMALL.feature_dimensionalities
    x = _inputs(dims)
    with dispatch_path(path):
        m = _model(spec)
        eng = m._ensure_engine()
        loop, loop_idx = _loop(m, x, dims, SHOWN, seed=5)
        res = m.compression_matrices(x, max_number_to_display=SHOWN, rng=np.random.RandomState(5), return_distances=True)
        sel_rows = np.stack([np.r_[r["indices"], np.full(SHOWN - len(r["indices"]), r["indices"][0])] for r in res]).astype(np.int32)
        _, enc = eng.compression_matrices(eng.to_device(x), sel_rows, np.array([len(r["indices"]) for r in res], dtype=np.int32),
                                          want_encodings=True)
    assert [len(r["indices"]) for r in res] == [SHOWN, SHOWN, 3] and res[2]["counts"] is not None and res[0]["counts"] is None
    p = flat_to_params(m.param_blocks(), m.get_flat_weights(), spec)
    col = np.concatenate([[0], np.cumsum(dims)])
    err_new = err_loop = 0.0
    for f, r in enumerate(res):
        assert np.array_equal(r["indices"], loop_idx[f]), f
        n = len(r["indices"])
        assert r["matrix"].shape == (n, n) and r["matrix"].dtype == np.float32 and r["distances"].shape == (n, n)
        xf = x[r["indices"], col[f]: col[f + 1]]
        assert np.array_equal(r["values"], xf[:, 0])
        ref, ref_enc = ocm.chain(spec, p, f, xf)
        assert np.abs(enc[f, :n] - ref_enc).max() < 2e-4 * (1 + np.abs(ref_enc).max()), f
        assert np.abs(r["matrix"] - np.exp(-r["distances"].astype(np.float64))).max() <= 2.0 ** -22
        err_new = max(err_new, float(np.abs(r["matrix"] - ref).max()))
        err_loop = max(err_loop, float(np.abs(loop[f] - ref).max()))
    print(f"{path}: err_new = {err_new:.3e}, err_loop = {err_loop:.3e}")
    assert err_new <= 2 * err_loop + 1e-6, (err_new, err_loop)


@pytest.mark.parametrize("path", DISPATCH_PATHS)
def test_launch_count_does_not_depend_on_the_number_of_features(path):
    counts = []
    with dispatch_path(path):
        for F in (3, 10):
            spec = orc.DIBSpec([1] * F, [32, 32], [16], 1, feature_embedding_dimension=8)
            m = _model(spec)
            eng = m._ensure_engine()
            xd = eng.to_device(np.random.default_rng(F).standard_normal((200, F)).astype(np.float32))
            m.compression_matrices(xd, x_raw=xd.cpu().numpy(), max_number_to_display=SHOWN)   # the evaluation workspace exists
            n0 = eng.lib.dib_launch_count()
            res = m.compression_matrices(xd, x_raw=xd.cpu().numpy(), max_number_to_display=SHOWN)
            counts.append(eng.lib.dib_launch_count() - n0)
            assert len(res) == F and all(r["matrix"].shape == (SHOWN, SHOWN) for r in res)
    print(f"{path}: launches of one evaluation {counts}")
    assert counts[0] == counts[1] and counts[0] >= 3, counts


@pytest.mark.parametrize("E,shown", [(MAX_E + 4, SHOWN), (8, MAX_ROWS + 2)])
def test_a_shape_beyond_the_envelope_takes_the_loop_and_equals_it(E, shown):
    lib = _lib()
    spec = orc.DIBSpec([2, 1, 1], [24, 16], [8], 1, feature_embedding_dimension=E)
    dims = spec.feature_dimensionalities
    assert lib.dib_compression_supported(3, E, shown) == 0 and lib.dib_compression_supported(3, min(E, MAX_E), min(shown, MAX_ROWS)) == 1
    x = _inputs(dims)
    m = _model(spec)
    loop, loop_idx = _loop(m, x, dims, shown, seed=8)
    res = m.compression_matrices(x, max_number_to_display=shown, rng=np.random.RandomState(8))
    for f, r in enumerate(res):
        assert np.array_equal(r["indices"], loop_idx[f]) and r["matrix"].dtype == loop[f].dtype
        assert np.array_equal(r["matrix"], loop[f]), f


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


def test_callback_one_launch_and_loop_agree_and_neither_changes_the_training(tmp_path):
    import dib_amd
    x, y = _circuit_c()
    runs = {}
    for mode in (None, False, True):
        model = _circuit_model()
        cbs = [dib_amd.InfoBottleneckAnnealingCallback(1e-3, 1.0, 1, 3)]
        if mode is not None:
            out = tmp_path / f"one_launch_{mode}"
            cbs.append(dib_amd.SaveCompressionMatricesCallback(2, x[:40], x[:40], str(out), one_launch=mode))
        hist = model.fit(x, y, epochs=3, shuffle=True, batch_size=48, callbacks=cbs, verbose=False)
        runs[mode] = (model, hist, cbs[-1])
    loop, one = runs[False][2], runs[True][2]
    assert one.one_launch is True and loop.one_launch is False
    assert sorted(one.matrices) == sorted(loop.matrices) == [(e, f) for e in (0, 2) for f in range(4)]
    for k in loop.matrices:
        assert one.matrices[k].shape == loop.matrices[k].shape == (2, 2) and one.matrices[k].dtype == loop.matrices[k].dtype
        assert np.abs(np.diag(one.matrices[k]) - 1).max() <= 1e-6 and np.abs(np.diag(loop.matrices[k]) - 1).max() <= 1e-6
        assert np.abs(one.matrices[k] - loop.matrices[k]).max() < 1e-4, k
    names = [sorted(os.listdir(tmp_path / f"one_launch_{mode}")) for mode in (False, True)]
    assert names[0] == names[1] and len(names[0]) == 8 and all(n.startswith("feature_") and n.endswith(".png") for n in names[0])
    assert sorted(one.betas) == [0, 2] and one.betas == loop.betas
    # a fit with the callback (either mode) trains bit-identically to a fit without it
    base_model, base_hist, _ = runs[None]
    eb = base_model._ensure_engine()
    for mode in (False, True):
        model, hist, _ = runs[mode]
        e = model._ensure_engine()
        assert hist.history == base_hist.history
        assert torch.equal(e.params, eb.params) and torch.equal(e.adam_m, eb.adam_m) and torch.equal(e.adam_v, eb.adam_v)
        assert torch.equal(e.t_dev, eb.t_dev) and model._step == base_model._step


def test_train_script_keras_path_writes_the_matrices_in_one_launch(tmp_path):
    from dib_amd import train
    hist = train.main(["--dataset", "boolean_circuit", "--number_pretraining_epochs", "2", "--number_annealing_epochs", "3",
                       "--batch_size", "128", "--artifact_outdir", str(tmp_path), "--save_compression_matrices_frequency", "2",
                       "--compression_matrices_one_launch", "True", "--feature_encoder_architecture", "32", "32",
                       "--integration_network_architecture", "64", "--feature_embedding_dimension", "8"])
    F = len(hist.model.feature_dimensionalities)
    z = np.load(tmp_path / "compression_matrices.npz")
    assert list(z["epochs"]) == [0, 2, 4] and z["beta"].shape == (3,) and z["beta"].dtype == np.float32
    assert np.array_equal(z["beta"], np.float32(hist.history["beta"])[[0, 2, 4]])
    assert z["beta"][0] == z["beta"][1] < z["beta"][2]   # epochs 0 and 2 are pretraining: one beta, one file name per feature
    pngs = sorted(n for n in os.listdir(tmp_path) if n.startswith("feature_"))
    assert pngs == sorted({f"feature_{f}_log10beta_{np.log10(float(beta)):.3f}.png" for beta in z["beta"] for f in range(F)})
    assert len(pngs) == 2 * F and all((tmp_path / n).stat().st_size > 1000 for n in pngs)
    for e in (0, 2, 4):
        for f in range(F):
            m = z[f"epoch{e}_feature{f}"]
            assert m.shape == (2, 2) and m.dtype == np.float32 and (np.diag(m) == 1).all() and np.array_equal(m, m.T)


@pytest.mark.parametrize("one_launch", ["False", "True"])
def test_train_script_infonce_path_saves_the_matrices_at_the_epoch_boundaries(tmp_path, one_launch):
    """the double_pendulum call of tests/test_gpu_parity.py::test_infonce_training_loop_on_pendulum with the saving flag: the loop
    closes epochs 0 .. 3, so epochs 0 and 2 are saved, each named by the beta just assigned"""
    from dib_amd import train
    art = tmp_path / "artifacts"
    out = train.main(["--dataset", "double_pendulum", "--infonce_loss", "True", "--data_path", str(tmp_path),
                      "--pendulum_number_trajectories", "6", "--number_pretraining_epochs", "2",
                      "--number_annealing_epochs", "3", "--batch_size", "256", "--learning_rate", "1e-3",
                      "--artifact_outdir", str(art), "--beta_start", "1e-4", "--beta_end", "1e-2",
                      "--save_compression_matrices_frequency", "2", "--compression_matrices_one_launch", one_launch])
    assert out["beta"].shape == (4,)
    # (both are pretraining epochs: one beta, so the second save overwrites the first's four files - as in the reference)
    want = sorted({f"feature_{f}_log10beta_{np.log10(float(out['beta'][e])):.3f}.png" for e in (0, 2) for f in range(4)})
    got = sorted(n for n in os.listdir(art) if n.startswith("feature_"))
    assert got == want and len(got) == 4 and all((art / n).stat().st_size > 1000 for n in got)
    z = np.load(art / "compression_matrices.npz")
    assert list(z["epochs"]) == [0, 2] and np.array_equal(z["beta"], out["beta"][[0, 2]])
    for e in (0, 2):
        for f in range(4):
            mat = z[f"epoch{e}_feature{f}"]
            assert mat.shape == (128, 128) and np.isfinite(mat).all() and np.abs(np.diag(mat) - 1).max() < 1e-4
