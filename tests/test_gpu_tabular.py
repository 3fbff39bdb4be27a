"""The tabular front end on the device (include/dib_tabular.h, csrc/dib_tabular.h, dib_amd.tabular, data.fetch_table, device-tensor
inputs of DistributedIBNet.fit / evaluate / predict):
  - dib_quantile_transform against the float64 restatement tests/_oracle_tabular.py (which tests/test_tabular_host.py holds to
    scikit-learn bit for bit) across the envelope - both kernels, the one that stages the tables in LDS and the one that searches
    them in global memory, on both sides of both thresholds between them - and on crafted data: float32 outputs within 1 ulp,
    >= 99.9 % bit-equal, NaN in the same places; the float64 u of finite inputs by EQUALITY; guard bands and row padding untouched;
  - placement (column permutations, row slices), graph replay, refusals that write nothing;
  - the reference-executed fixture through TabularPreprocessor's device backend; fetch_table -> fit against the float64 oracle
    fit; fit on a device tensor against fit on the same values as NumPy."""
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
import _oracle_tabular as otb  # noqa: E402
import dib_oracle as orc  # noqa: E402
from _helpers import flat_to_params, spec_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -777.25
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED
THREADS, MAX_BLOCKS = 256, 4096   # csrc/dib_tabular.h DIB_TAB_THREADS, DIB_TAB_MAX_BLOCKS
GOLDEN = os.path.join(ROOT, "tests", "golden", "tabular_preprocessor.npz")


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _columns(rng, n, d):
    """[n, d] float32: column c is of kind c % 6 - normal, exponential, 5-level, rounded to 0.1, heavy-tailed, binary"""
    kinds = [lambda: rng.standard_normal(n), lambda: rng.exponential(size=n), lambda: rng.integers(0, 5, n).astype(float),
             lambda: np.round(rng.standard_normal(n), 1), lambda: rng.standard_cauchy(n), lambda: rng.integers(0, 2, n).astype(float)]
    return _f32(np.stack([kinds[c % 6]() * (1.0 + c // 6) for c in range(d)], 1))


def _device_transform(x, quantiles, references, distribution, pad_x=0, pad_out=0, want_u=True):
    """one dib_quantile_transform call -> (out float32 [n, d], u float64 [n, d] or None).  x and out live in matrices of leading
    dimension d + pad between guard bands; the bands and the padding columns of out must come back untouched."""
    lib = _lib()
    n, d = x.shape
    ldx, ldo = d + pad_x, d + pad_out
    xh = np.full((n, ldx), 12345.0, np.float32)
    xh[:, :d] = x
    x_d = torch.tensor(xh, device="cuda")
    q_d = torch.tensor(np.ascontiguousarray(np.asarray(quantiles, np.float64).T), device="cuda")
    r_d = torch.tensor(np.asarray(references, np.float64), device="cuda")
    buf = torch.full((n * ldo + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ubuf = torch.full((n * d + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    out, u = buf[GUARD:GUARD + n * ldo], ubuf[GUARD:GUARD + n * d]
    n0 = lib.dib_launch_count()
    rc = lib.dib_quantile_transform(_p(x_d), ldx, n, d, _p(q_d), _p(r_d), len(references), distribution, _p(out), ldo,
                                    _p(u) if want_u else None, _st())
    assert rc == 0, rc
    assert lib.dib_launch_count() == n0 + 1   # one launch per call
    torch.cuda.synchronize()
    b, ub = buf.cpu().numpy(), ubuf.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + n * ldo:] == SENTINEL).all()
    assert (ub[:GUARD] == SENTINEL).all() and (ub[GUARD + n * d:] == SENTINEL).all()
    o = b[GUARD:GUARD + n * ldo].reshape(n, ldo)
    assert (o[:, d:] == SENTINEL).all()
    uo = ub[GUARD:GUARD + n * d].reshape(n, d)
    assert want_u or (uo == SENTINEL).all()
    return o[:, :d].copy(), (uo.copy() if want_u else None)


def _check(x, quantiles, references, distribution, **kw):
    got, u = _device_transform(x, quantiles, references, distribution, **kw)
    want, u_want = otb.transform(x, quantiles, references, distribution)
    otb.float32_criterion(got, want)
    if u is not None:
        finite = np.isfinite(x)
        assert np.array_equal(u[finite], u_want[finite])   # NumPy's bits: the interpolation is compiled without contraction
        assert np.isnan(u[np.isnan(x)]).all() and np.array_equal(u[np.isinf(x)], u_want[np.isinf(x)])
    return got, u


@functools.lru_cache(maxsize=None)
def _fitted(n_quantiles, n_cols):
    """tables of n_quantiles knots: the sorted values of n_quantiles rows of the column kinds - what the fit gives on as many rows
    as quantiles, and every knot a float32, so that inputs can sit exactly on knots"""
    rng = np.random.default_rng(100 * n_quantiles + n_cols)
    quantiles = np.sort(_columns(rng, n_quantiles, n_cols).astype(np.float64), axis=0)
    return quantiles, np.linspace(0, 1, n_quantiles)


# (n_quantiles, n_cols, n_rows, distribution): both ends of the quantile envelope and the reference's 2000; one element, one wave
# short of / exactly / beyond a multiple, workgroups with a ragged last one (n_rows n_cols no multiple of 256), more columns than a
# wave (77: the lanes of a wave span two rows).  The tables are staged in LDS from STAGE_ROWS n_quantiles rows on while one
# column's table fits (n_quantiles <= STAGE_MAX): both sides of both thresholds; a last column group of one column (77 = 19 x 4 + 1
# at 2000 quantiles); two and three slabs of rows; all 77 columns in one group.  Unstaged, a table of more elements than the grid
# has lanes (a second pass of the loop).
STAGE_ROWS, STAGE_MAX = 4, 8192   # csrc/dib_tabular.h DIB_TAB_STAGE_MIN_ROWS_PER_QUANTILE, DIB_TAB_STAGE_BYTES / 8
ENVELOPE = [(2, 1, 1, 0), (2, 77, 1000, 1), (3, 3, 63, 0), (3, 1, 257, 1), (240, 5, 64, 0), (240, 1, 65, 1), (2000, 77, 65, 0),
            (2000, 5, 1000, 0), (2000, 3, 257, 1), (10000, 3, 257, 0), (10000, 1, 64, 1),
            (240, 5, STAGE_ROWS * 240 - 1, 0), (240, 5, STAGE_ROWS * 240, 0), (240, 5, 3 * STAGE_ROWS * 240 + 7, 1),
            (2000, 77, STAGE_ROWS * 2000 + 37, 0), (2000, 5, 2 * STAGE_ROWS * 2000 + 123, 0),
            (STAGE_MAX, 3, STAGE_ROWS * STAGE_MAX + 5, 0), (STAGE_MAX + 1, 3, STAGE_ROWS * STAGE_MAX + 5, 0),
            (10000, 77, (THREADS * MAX_BLOCKS) // 77 + 300, 0)]


@pytest.mark.parametrize("n_quantiles,n_cols,n_rows,distribution", ENVELOPE)
def test_envelope_matches_the_float64_oracle(n_quantiles, n_cols, n_rows, distribution):
    quantiles, references = _fitted(n_quantiles, n_cols)
    rng = np.random.default_rng(n_rows)
    x = _columns(rng, n_rows, n_cols)
    x[::7] *= 30.0                      # rows outside the fitted range
    k = rng.integers(0, n_quantiles, n_rows)
    x[::5] = _f32(quantiles)[k[::5]]    # rows on (float32-representable) knots
    assert n_rows * n_cols <= THREADS * MAX_BLOCKS or n_rows == ENVELOPE[-1][2]
    _check(x, quantiles, references, distribution)


@pytest.mark.parametrize("distribution", [0, 1])
def test_crafted_values(distribution):
    """knots, runs of equal quantiles (a 5-level and a constant column: where the mean of the two directions matters), the 1e-7
    band around the end quantiles from both sides, far outside, +-inf, NaN, -0.0 and denormals, in padded matrices"""
    n_q = 240
    rng = np.random.default_rng(11)
    fit = np.stack([rng.standard_normal(n_q), rng.integers(0, 5, n_q).astype(float), np.full(n_q, 2.5),
                    rng.uniform(0.3, 0.45, n_q), rng.standard_normal(n_q) * 1e-40, rng.exponential(size=n_q)], 1)
    fit[0, 3], fit[1, 3] = 0.3, 0.45
    quantiles, references = np.sort(_f32(fit).astype(np.float64), axis=0), np.linspace(0, 1, n_q)   # every knot a float32
    q32 = _f32(quantiles)
    rows = [q32[i] for i in (0, 1, 7, 119, 120, 238, 239)]
    for end in (0, n_q - 1):   # float32 neighbours of the end quantiles: in column 3 (an ulp is 3e-8) 3e-8 and 9e-8 away, inside
        for steps in (1, 3, 4, 40):   # the 1e-7 band, 1.2e-7 and 1.2e-6 away, outside it
            up = down = q32[end].copy()
            for _ in range(steps):
                up, down = np.nextafter(up, _f32(np.inf)), np.nextafter(down, _f32(-np.inf))
            rows += [up, down]
    rows += [np.full(6, v, np.float32) for v in (np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 3e38, -3e38, 2.5, 1.0,
                                                 2.0000002, 0.29999995, 0.45000005)]
    rows += list(_f32(0.5 * (quantiles[:-1] + quantiles[1:]))[::9])   # between knots
    rows += list(_f32(fit[:40] * 1.0001))
    x = np.stack(rows)
    x[5, 1] = x[9, 4] = np.nan   # NaN beside finite values in a row
    assert np.isnan(x).any() and np.isinf(x).any() and np.signbit(x[x == 0]).any()
    got, u = _check(x, quantiles, references, distribution, pad_x=3, pad_out=5)
    finite = ~np.isnan(x)
    if distribution == 0:
        assert np.abs(got[finite]).max() == np.float32(5.1993375) and (u[finite] >= otb.U_LO).all() and (u[finite] <= otb.U_HI).all()
    else:
        assert got[finite].min() == 0.0 and got[finite].max() == 1.0
    # the constant column: every value at or around 2.5 lands on one of the three answers of the rule, nothing else
    assert set(np.unique(u[finite[:, 2], 2])) <= ({otb.U_LO, otb.U_HI} if distribution == 0 else {0.0, 0.5, 1.0})
    _check(x, quantiles, references, distribution, want_u=False)
    copies = -(-STAGE_ROWS * n_q // len(x))   # enough rows for the tables to be staged in LDS: the same values on the other kernel
    assert len(x) < STAGE_ROWS * n_q <= copies * len(x)
    got2, u2 = _check(np.tile(x, (copies, 1)), quantiles, references, distribution, pad_x=1)
    assert np.array_equal(got2, np.tile(got, (copies, 1)), equal_nan=True) and np.array_equal(u2, np.tile(u, (copies, 1)), equal_nan=True)


def test_placement_does_not_change_the_bits():
    """an element's result depends on its value and its column's table alone: permuted columns, row slices, other leading
    dimensions and a launch that shares the grid with many more rows all give the same bits"""
    quantiles, references = _fitted(2000, 5)
    rng = np.random.default_rng(3)
    x = _columns(rng, 1000, 5)
    x[::9] *= 20.0
    base, u = _device_transform(x, quantiles, references, 0)
    perm = np.array([3, 0, 4, 2, 1])
    got, up = _device_transform(x[:, perm], quantiles[:, perm], references, 0)
    assert np.array_equal(got, base[:, perm]) and np.array_equal(up, u[:, perm])
    for rows in (slice(0, 1), slice(63, 64), slice(100, 357), slice(999, 1000)):
        got, us = _device_transform(x[rows], quantiles, references, 0, pad_x=2, pad_out=1)
        assert np.array_equal(got, base[rows]) and np.array_equal(us, u[rows])
    got, _ = _device_transform(x[:, 2:3], quantiles[:, 2:3], references, 0)
    assert np.array_equal(got, base[:, 2:3])
    big = np.tile(x, (THREADS * MAX_BLOCKS // x.size + 2, 1))   # the rows again, now computed by lanes on their second pass
    got, _ = _device_transform(big, quantiles, references, 0, want_u=False)
    assert np.array_equal(got, np.tile(base, (big.shape[0] // 1000, 1)))


def test_graph_replay_has_the_eager_bits():
    lib = _lib()
    quantiles, references = _fitted(240, 5)   # 1000 rows: the staged kernel, dynamic LDS
    x = _columns(np.random.default_rng(4), 1000, 5)
    eager, u_eager = _device_transform(x, quantiles, references, 0)
    x_d = torch.tensor(x, device="cuda")
    q_d = torch.tensor(np.ascontiguousarray(quantiles.T), device="cuda")
    r_d = torch.tensor(references, device="cuda")
    out = torch.zeros((1000, 5), dtype=torch.float32, device="cuda")
    u = torch.zeros((1000, 5), dtype=torch.float64, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # the call neither allocates nor synchronises: it can be captured
        rc = lib.dib_quantile_transform(_p(x_d), 5, 1000, 5, _p(q_d), _p(r_d), 240, 0, _p(out), 5, _p(u), _st())
    assert rc == 0
    for _ in range(2):
        out.zero_()
        u.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager) and np.array_equal(u.cpu().numpy(), u_eager)
    x_d.copy_(torch.tensor(x[::-1].copy(), device="cuda"))   # a replay reads the buffers as they are now
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), eager[::-1])


def test_refused_calls_launch_nothing_and_write_nothing():
    lib = _lib()
    x = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    q = torch.zeros((4, 16), dtype=torch.float64, device="cuda")
    r = torch.linspace(0, 1, 16, dtype=torch.float64, device="cuda")
    out = torch.full((8, 4), SENTINEL, dtype=torch.float32, device="cuda")
    u = torch.full((8, 4), SENTINEL, dtype=torch.float64, device="cuda")
    n0 = lib.dib_launch_count()
    call = lambda x_=x, ldx=4, n=8, d=4, q_=q, r_=r, nq=16, dist=0, out_=out, ldo=4: lib.dib_quantile_transform(
        _p(x_), ldx, n, d, _p(q_), _p(r_), nq, dist, _p(out_), ldo, _p(u), _st())
    assert call(x_=None) == ARG and call(q_=None) == ARG and call(r_=None) == ARG and call(out_=None) == ARG
    assert call(ldx=3) == ARG and call(ldo=3) == ARG and call(n=0) == ARG and call(n=-1) == ARG and call(d=0) == ARG and call(nq=0) == ARG
    assert call(nq=1) == UNSUPPORTED and call(nq=10001) == UNSUPPORTED and call(d=65536, ldx=65536, ldo=65536) == UNSUPPORTED
    assert call(dist=2) == UNSUPPORTED and call(dist=-1) == UNSUPPORTED
    torch.cuda.synchronize()
    assert lib.dib_launch_count() == n0
    assert (out == SENTINEL).all() and (u == SENTINEL).all()
    assert call() == 0   # and the accepted call does write
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any() and not (u == SENTINEL).any()


@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture_through_the_device_backend(case):
    """the rows the reference's own MyPreprocessor transformed (tests/golden/make_golden_tabular.py), here fitted on the host and
    transformed in one launch"""
    from dib_amd import tabular
    g = np.load(GOLDEN)
    x, y = g[f"{case}_x_train"].astype(np.float64), g[f"{case}_y_train"].astype(np.float64)
    pre = tabular.TabularPreprocessor(random_state=1337, quantile_transform=True, quantile_noise=1e-3, y_normalize=True).fit(x, y)
    lib = _lib()
    n0 = lib.dib_launch_count()
    t_train, y_norm = pre.transform(x, y, backend="device")
    assert lib.dib_launch_count() == n0 + 1 and isinstance(t_train, np.ndarray)
    otb.float32_criterion(t_train, g[f"{case}_t_train"])
    t = pre.transform(g[f"{case}_x_valid"], backend="device", as_tensor=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    otb.float32_criterion(t.cpu().numpy(), g[f"{case}_t_valid"])
    otb.float32_criterion(t.cpu().numpy(), pre.transform(g[f"{case}_x_valid"], backend="host"))
    # a table already on the device is transformed where it lies
    x_d = torch.tensor(g[f"{case}_x_valid"], device="cuda")
    assert np.array_equal(pre.transform(x_d, as_tensor=True).cpu().numpy(), t.cpu().numpy())
    assert np.abs(y_norm - g[f"{case}_y_norm"]).max() <= np.spacing(np.float32(np.abs(y_norm).max()))
    # without the quantile transform nothing is launched
    n0 = lib.dib_launch_count()
    plain = tabular.TabularPreprocessor().fit(x).transform(x)
    assert lib.dib_launch_count() == n0 and np.array_equal(plain, _f32(x))


def _mixed_table(path, n=512):
    """three continuous columns, one discrete, one 3-level categorical; y depends on a continuous column and on the category"""
    rng = np.random.default_rng(8)
    x = _f32(np.stack([rng.standard_normal(n), rng.exponential(size=n), rng.standard_normal(n) * 3.0 + 1.0,
                       rng.integers(0, 6, n).astype(float), rng.integers(0, 3, n).astype(float)], 1))
    y = (x[:, 0] + 1.5 * (x[:, 4] == 1) - 0.5 > 0).astype(np.int64)
    np.savez(path, x=x, y=y, columns=np.array(["a", "b", "c", "count", "kind"]))
    return x, y


def test_table_end_to_end_against_the_oracle_fit(tmp_path):
    import dib_amd
    path = str(tmp_path / "table.npz")
    x_raw, y_raw = _mixed_table(path)
    d = dib_amd.data.fetch_table(table_path=path, table_categorical=["kind"], seed=5)
    assert d["feature_dimensionalities"] == [1, 1, 1, 1, 3] and d["output_dimensionality"] == 2
    # the oracle's preprocessing of the same split
    order = np.random.RandomState(5).permutation(512)
    n_train = 512 - int(512 * 0.2)
    _, categories, _ = otb.one_hot(x_raw[order[:n_train]].astype(np.float64).tolist(), [4])
    enc = otb.one_hot(x_raw[order].astype(np.float64).tolist(), [4], categories)[0]
    q, r = otb.fit_quantiles(otb.noisy(enc[:n_train], 1e-3, 1337), 2000, 10000, 1337)
    x_train, x_valid = otb.transform(enc[:n_train], q, r, 0)[0], otb.transform(enc[n_train:], q, r, 0)[0]
    otb.float32_criterion(d["x_train"], x_train)
    otb.float32_criterion(d["x_valid"], x_valid)
    assert np.array_equal(d["x_valid_raw"], _f32(enc[n_train:]))
    y_train, y_valid = _f32(y_raw[order[:n_train]])[:, None], _f32(y_raw[order[n_train:]])[:, None]
    assert np.array_equal(d["y_train"], y_train) and np.array_equal(d["y_valid"], y_valid)

    spec = orc.DIBSpec(d["feature_dimensionalities"], [32, 32], [64], d["output_dimensionality"], feature_embedding_dimension=8)
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = 3e-3
    model.compile(optimizer=opt, loss=d["loss"], metrics=d["metrics"])
    cb = dib_amd.InfoBottleneckAnnealingCallback(1e-3, 1.0, 1, 3)
    saver = dib_amd.SaveCompressionMatricesCallback(2, d["x_valid"], d["x_valid_raw"], str(tmp_path / "matrices"), save_png=False,
                                                    one_launch=True)
    p = flat_to_params(model.param_blocks(), model.get_flat_weights(), spec)
    epochs, bs = 4, 64
    hist = model.fit(d["x_train"], d["y_train"], epochs=epochs, shuffle=True, batch_size=bs, callbacks=[cb, saver], verbose=False,
                     validation_data=(d["x_valid"], d["y_valid"]))
    ref = orc.fit(spec, p, x_train, y_train, epochs=epochs, batch_size=bs, loss_kind="sparse_cce_logits",
                  beta_fn=lambda e: orc.beta_schedule(e, 1e-3, 1.0, 1, 3), lr=3e-3, shuffle=True,
                  validation_data=(x_valid, y_valid), noise_seed=4, shuffle_seed=6, metrics=["accuracy"])
    assert set(ref) == set(hist.history) and {f"KL{f}" for f in range(5)} <= set(ref)
    for k in ref:   # the tolerances of tests/test_gpu_losses.py _fit_against_oracle
        got, want = np.array(hist.history[k]), np.array(ref[k])
        tol = 1e-3 if "KL" in k else 2e-3
        assert np.abs(got - want).max() < tol * (1 + np.abs(want).max()), (k, got, want)
    # the compression matrices are saved from the raw values: one per (save, feature), labelled by x_valid_raw
    assert sorted(saver.matrices) == [(e, f) for e in (0, 2) for f in range(5)]
    assert all(np.isfinite(m).all() and m.shape[0] == m.shape[1] for m in saver.matrices.values())


def test_fit_on_a_device_tensor_equals_fit_on_numpy_bit_for_bit():
    import dib_amd
    rng = np.random.default_rng(12)
    x = _f32(rng.standard_normal((200, 4)))
    y = _f32(x[:, :1] * x[:, 1:2] > 0)

    def run(as_tensor):
        model = dib_amd.DistributedIBNet([1, 1, 2], [16], [32], 1, feature_embedding_dimension=4, noise_seed=1, shuffle_seed=2, init_seed=3)
        model.compile(optimizer="adam", loss=dib_amd.losses.BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
        dev = model._ensure_engine().device
        xt, xv = (torch.tensor(x, device=dev), torch.tensor(x[:50], device=dev)) if as_tensor else (x, x[:50])
        ptr = xt.data_ptr() if as_tensor else None
        hist = model.fit(xt, y, epochs=3, batch_size=64, shuffle=True, verbose=False, validation_data=(xv, y[:50]))
        logs = model.evaluate(xv, y[:50], batch_size=64)
        pred = model.predict(xv)
        if as_tensor:   # used where it lies, and left as it was
            assert xt.data_ptr() == ptr and np.array_equal(xt.cpu().numpy(), x)
        return hist.history, model.get_flat_weights(), logs, pred

    h0, w0, l0, p0 = run(False)
    h1, w1, l1, p1 = run(True)
    assert set(h0) == set(h1) and all(h0[k] == h1[k] for k in h0)
    assert np.array_equal(w0, w1) and l0 == l1 and np.array_equal(p0, p1)
    model = dib_amd.DistributedIBNet([1, 1, 2], [16], [32], 1, feature_embedding_dimension=4)
    model.compile(optimizer="adam", loss="mse")
    with pytest.raises(AssertionError, match="input width"):
        model.fit(torch.zeros((8, 3), device=model._ensure_engine().device), np.zeros(8, np.float32), epochs=1, verbose=False)
