"""Every feature's compression matrix in one evaluation, without a device: the host-only envelope call of
include/dib_compression.h at its edges and the argument refusals of its entry points (they return before any device call), the
binding, the display rule for all features (visualization.display_rows) against select_display_inputs feature by feature, the
figure (visualization.draw_compression_matrix) against the recorded reference content, and the one-launch callback on the
test-only oracle engine, where it takes the per-feature loop."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED
MAX_E, MAX_ROWS, MAX_F = 256, 2048, 65535   # include/dib_compression.h DIB_COMPRESSION_MAX_*


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def test_envelope_edges():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "dib_compression.h")).read()
    for name, v in (("MAX_E", MAX_E), ("MAX_ROWS", MAX_ROWS), ("MAX_F", MAX_F)):
        assert f"#define DIB_COMPRESSION_{name} {v}\n" in header
    for F in (1, MAX_F):
        for E in (1, MAX_E):
            for n in (1, MAX_ROWS):
                assert lib.dib_compression_supported(F, E, n) == 1, (F, E, n)
    for F, E, n in ((MAX_F + 1, 8, 8), (1, MAX_E + 1, 8), (1, 8, MAX_ROWS + 1), (0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8),
                    (1, -4, 8), (1, 8, -1)):
        assert lib.dib_compression_supported(F, E, n) == 0, (F, E, n)


def test_argument_refusals_need_no_device():
    """every refusal is decided on the host before anything is enqueued: the pointers below are never dereferenced"""
    lib = _lib()
    buf = (ctypes.c_float * 16)()
    p, z = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    n0 = lib.dib_launch_count()
    mat = lambda enc=p, plane_rows=8, row0=0, F=1, E=1, cnt=p, n_max=2, dist=p, comp=p: \
        lib.dib_compression_matrices(enc, plane_rows, row0, F, E, cnt, n_max, dist, comp, z)
    assert mat(enc=z) == ARG and mat(cnt=z) == ARG and mat(dist=z, comp=z) == ARG
    assert mat(F=0) == ARG and mat(E=0) == ARG and mat(n_max=0) == ARG and mat(n_max=-7) == ARG
    assert mat(row0=-1) == ARG and mat(row0=7) == ARG and mat(plane_rows=1) == ARG and mat(plane_rows=0) == ARG
    assert mat(E=MAX_E + 1) == UNSUPPORTED and mat(F=MAX_F + 1) == UNSUPPORTED
    assert mat(n_max=MAX_ROWS + 1, plane_rows=1 << 20) == UNSUPPORTED
    assert lib.dib_compression_gather(z, p, 4, 4, p, 2, p, z) == ARG                      # no layout
    handle = ctypes.c_void_p()
    ci = lambda xs: (ctypes.c_int * len(xs))(*xs)
    assert lib.dib_layout_create(3, ci([2, 1, 3]), 2, ci([8, 8]), 4, 1, ci([8]), 1, 1, 5, 1, 0, ctypes.byref(handle)) == 0
    try:
        gat = lambda x=p, ldx=6, n_rows=4, rows=p, n_max=2, xg=p: lib.dib_compression_gather(handle, x, ldx, n_rows, rows, n_max, xg, z)
        assert gat(x=z) == ARG and gat(rows=z) == ARG and gat(xg=z) == ARG
        assert gat(ldx=5) == ARG and gat(n_rows=0) == ARG and gat(n_max=0) == ARG and gat(n_max=MAX_ROWS + 1) == UNSUPPORTED
        assert gat() == ARG                                                               # the layout's tables were never uploaded
    finally:
        lib.dib_layout_destroy(handle)
    assert lib.dib_launch_count() == n0


def test_binding_header_and_flags():
    from dib_amd import _lib
    header = open(os.path.join(ROOT, "include", "dib_compression.h")).read()
    for name, (_, args) in _lib.SIGNATURES_COMPRESSION.items():
        decl = header[header.index("int " + name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == len(args), name
    lib = _lib.load_library()
    assert lib.dib_compression_matrices.argtypes == _lib.SIGNATURES_COMPRESSION["dib_compression_matrices"][1]
    assert lib.dib_abi_version() == 7 == _lib.ABI_VERSION
    import dib_amd
    assert callable(dib_amd.DistributedIBNet.compression_matrices)
    from dib_amd import train
    a = train.get_args([])
    assert a.compression_matrices_one_launch is False and a.save_compression_matrices_frequency == 0
    assert train.get_args(["--compression_matrices_one_launch", "True"]).compression_matrices_one_launch is True
    assert dib_amd.SaveCompressionMatricesCallback(1, np.zeros((2, 1)), np.zeros((2, 1)), "x").one_launch is False


def _mixed_inputs(n=200, seed=0):
    """dims [2, 1, 1, 1]: a 2-dimensional continuous feature, a continuous one, one with 3 and one with 9 unique values"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 5))
    x[:, 3] = rng.integers(0, 3, n) * 0.5
    x[:, 4] = rng.integers(0, 9, n)
    return x, [2, 1, 1, 1]


@pytest.mark.parametrize("shown", [128, 7, 2])
def test_display_rows_is_the_per_feature_rule_under_one_generator(shown):
    from dib_amd import visualization
    x, dims = _mixed_inputs()
    got = visualization.display_rows(x, dims, shown, rng=np.random.RandomState(11))
    rng = np.random.RandomState(11)
    split = np.split(x, np.cumsum(dims)[:-1], axis=-1)
    want = [visualization.select_display_inputs(xf, shown, rng) for xf in split]
    n_max = max(shown, 9)
    assert got["rows"].shape == (4, n_max) and got["rows"].dtype == np.int32 and got["n_rows"].dtype == np.int32
    assert list(got["n_rows"]) == [shown, shown, 3, 9]
    for f, (idx, vals, freq) in enumerate(want):
        assert np.array_equal(got["indices"][f], idx) and np.array_equal(got["values"][f], vals)
        assert (got["counts"][f] is None) == (freq is None) and (freq is None or np.allclose(got["counts"][f], freq, atol=0))
        assert np.array_equal(got["rows"][f, :len(idx)], idx) and (got["rows"][f, len(idx):] == idx[0]).all()   # padded with its own first index
        assert got["rows"][f].min() >= 0 and got["rows"][f].max() < x.shape[0]
    assert want[0][1].shape == (shown,) and np.array_equal(want[0][1], np.sort(x[want[0][0], 0]))   # 2-d feature: sorted by its first column
    assert want[2][2] is not None and abs(sum(want[2][2]) - 1) < 1e-12
    # the global generator when rng is None, like the loop
    np.random.seed(3)
    a = visualization.display_rows(x, dims, shown)
    np.random.seed(3)
    b = [visualization.select_display_inputs(xf, shown) for xf in split]
    assert all(np.array_equal(u, v[0]) for u, v in zip(a["indices"], b))


def test_display_rows_cache_keeps_the_deterministic_selections_and_the_draws():
    from dib_amd import visualization
    x, dims = _mixed_inputs()
    cache = {}
    first = visualization.display_rows(x, dims, 16, rng=np.random.RandomState(1), cache=cache)
    assert sorted(cache) == [0, 1, 2, 3] and cache[0] is None and cache[1] is None   # drawn at random: only that fact is kept
    assert cache[2] is not None and cache[3] is not None                               # < 10 unique values: the selection
    rng_a, rng_b = np.random.RandomState(2), np.random.RandomState(2)
    again = visualization.display_rows(x, dims, 16, rng=rng_a, cache=cache)
    plain = visualization.display_rows(x, dims, 16, rng=rng_b)
    for f in range(4):
        assert np.array_equal(again["indices"][f], plain["indices"][f])
    assert again["indices"][2] is first["indices"][2] and rng_a.randint(1 << 30) == rng_b.randint(1 << 30)   # the same draws were consumed
    one = visualization.display_rows(np.arange(5.0), [1], 4)   # a 1-d array is one feature
    assert one["rows"].shape == (1, 5) and list(one["n_rows"]) == [5]


def test_draw_compression_matrix_content_matches_the_reference_figure(monkeypatch, tmp_path):
    """the drawing half on its own: the matrix handed to imshow and the side-plot arrays against what the reference's function
    draws (tests/golden/compression_matrix_figure.npz, recorded with the matplotlib stand-in)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from plt_recorder import Recorder
    from dib_amd import visualization
    g = np.load(os.path.join(ROOT, "tests", "golden", "compression_matrix_figure.npz"))
    rec = Recorder()
    monkeypatch.setattr(visualization, "_plt", lambda: rec)
    idx, vals, freq = visualization.select_display_inputs(g["raw_a"])
    visualization.draw_compression_matrix(g["a_matrix"], vals, freq, str(tmp_path / "a.png"), feature_label="Feature 3")
    c = rec.content()
    assert np.array_equal(c[((1, 1), "imshow")][0], g["a_matrix"])
    assert np.array_equal(c[((1, 0), "barh")][0], g["a_barh_y"]) and np.allclose(c[((1, 0), "barh")][1], g["a_barh_w"], atol=1e-15)
    assert np.array_equal(c[((0, 1), "bar")][0], g["a_bar_x"]) and np.allclose(c[((0, 1), "bar")][1], g["a_bar_h"], atol=1e-15)
    assert rec.saved == [str(tmp_path / "a.png")]
    rec = Recorder()
    monkeypatch.setattr(visualization, "_plt", lambda: rec)
    np.random.seed(123)
    idx, vals, freq = visualization.select_display_inputs(g["raw_b"])
    assert freq is None
    visualization.draw_compression_matrix(g["b_matrix_intent"], vals, freq, str(tmp_path / "b.png"))
    c = rec.content()
    assert np.array_equal(c[((1, 1), "imshow")][0], g["b_matrix_intent"])
    assert np.array_equal(c[((1, 0), "plot")][0], g["b_left_x"]) and np.array_equal(c[((1, 0), "plot")][1], g["b_left_y"])
    assert np.array_equal(c[((0, 1), "plot")][0], g["b_top_x"]) and np.array_equal(c[((0, 1), "plot")][1], g["b_top_y"])
    assert rec.saved == [str(tmp_path / "b.png")]


def test_one_launch_callback_on_the_oracle_engine_takes_the_loop(monkeypatch, tmp_path):
    """the test-only oracle engine has no compression_matrices: the callback's one call per save runs the per-feature loop on
    the same display rows and gives the float64 chain's matrices"""
    import dib_oracle as orc
    from _oracle_engine import OracleEngine
    from dib_amd import models, visualization
    monkeypatch.setattr(models.DistributedIBNet, "_make_engine",
                        lambda self: OracleEngine(**self._spec_kwargs(), init_seed=self.init_seed))
    x, dims = _mixed_inputs(120)
    spec = orc.DIBSpec(dims, [8, 8], [8], 1, feature_embedding_dimension=4)
    model = models.DistributedIBNet(dims, [8, 8], [8], 1, feature_embedding_dimension=4, init_seed=2)
    model.beta.assign(0.01)
    eng = model._ensure_engine()
    assert not hasattr(eng, "compression_matrices")
    cb = models.SaveCompressionMatricesCallback(2, x, x, str(tmp_path), one_launch=True)
    cb.set_model(model)
    np.random.seed(5)
    cb.on_epoch_end(1)
    assert cb.matrices == {} and os.listdir(tmp_path) == []
    cb.on_epoch_end(4)
    np.random.seed(5)
    split = np.split(x, np.cumsum(dims)[:-1], axis=-1)
    assert sorted(cb.matrices) == [(4, f) for f in range(4)] and cb.betas == {4: float(np.float32(0.01))}
    for f, xf in enumerate(split):
        idx = visualization.select_display_inputs(xf)[0]
        want = orc.compression_matrix(spec, eng.p, f, xf[idx].astype(np.float64))
        assert cb.matrices[(4, f)].shape == want.shape and np.abs(cb.matrices[(4, f)] - want).max() < 1e-9, f
    assert sorted(os.listdir(tmp_path)) == sorted(f"feature_{f}_log10beta_-2.000.png" for f in range(4))
    assert [f for f, s in sorted(cb._selection_cache.items()) if s is not None] == [2, 3] and cb._x_dev is None
