"""The tabular front end on the host (dib_amd.tabular, data.fetch_table, train.py --dataset table), no GPU needed:
  - the fit and the "host" transform against scikit-learn's QuantileTransformer, bit for bit on a float64 ndarray;
  - against the fixture the reference's own MyPreprocessor produced (tests/golden/make_golden_tabular.py);
  - the product's host backend against the independent restatement tests/_oracle_tabular.py, bit for bit;
  - the one-hot rule (a written restatement: category_encoders is not installed, so there is nothing to compare it with);
  - fetch_table, the command line, the envelope of dib_quantile_supported."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle_tabular as otb  # noqa: E402
from dib_amd import data, tabular, train  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tabular_preprocessor.npz")


def mixed_table(n, seed=0):
    """float32-representable float64 [n, 6]: normal, exponential, 5-level, rounded to 0.1, heavy-tailed, binary"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.standard_normal(n), rng.exponential(size=n), rng.integers(0, 5, n).astype(float),
                  np.round(rng.standard_normal(n), 1), rng.standard_cauchy(n), rng.integers(0, 2, n).astype(float)], 1)
    return x.astype(np.float32).astype(np.float64)


def held_out(x, quantiles, seed=1):
    """rows of another draw, some far outside the fitted range, some exactly on the end quantiles and on inner knots"""
    t = mixed_table(700, seed)[:, :x.shape[1]]
    t[:40] *= 100.0
    t[40:50] = quantiles[0]
    t[50:60] = quantiles[-1]
    t[60:70] = quantiles[quantiles.shape[0] // 2]
    return t.astype(np.float32).astype(np.float64)


float32_criterion = otb.float32_criterion


@pytest.mark.parametrize("n_rows", [400, 12000])
@pytest.mark.parametrize("distribution", ["normal", "uniform"])
def test_fit_and_host_transform_equal_sklearn_bit_for_bit(n_rows, distribution):
    sk = pytest.importorskip("sklearn.preprocessing")
    x = mixed_table(n_rows)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # n_quantiles > n_samples at 400 rows
        qt = sk.QuantileTransformer(n_quantiles=2000, output_distribution=distribution, random_state=1337).fit(x.copy())
    quantiles, references = tabular.quantile_fit(x, 2000, 10000, 1337)
    assert quantiles.shape == (min(2000, n_rows), 6)
    assert np.array_equal(quantiles, qt.quantiles_) and np.array_equal(references, qt.references_)
    if n_rows > 10000:   # the subsample is sklearn.utils.resample's
        from sklearn.utils import resample
        idx = np.arange(n_rows)
        np.random.RandomState(1337).shuffle(idx)
        assert np.array_equal(resample(x, replace=False, n_samples=10000, random_state=np.random.RandomState(1337)), x[idx[:10000]])
    for table in (x, held_out(x, quantiles)):
        want = qt.transform(table.copy()).astype(np.float32)
        got = tabular.quantile_transform_host(table, quantiles, references, distribution)
        assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.mark.parametrize("distribution", [0, 1])
def test_host_backend_and_the_oracle_agree_bit_for_bit(distribution):
    x = mixed_table(3000, seed=5)
    quantiles, references = tabular.quantile_fit(x[:900], 240, 10000, 3)
    t = held_out(x, quantiles)
    t[100:110] = np.nan
    t[110:115], t[115:120], t[120:125] = np.inf, -np.inf, -0.0
    t[125:130] = 1e-42
    name = ("normal", "uniform")[distribution]
    for table in (x, t):
        got, u = tabular.quantile_transform_host(table, quantiles, references, name, return_u=True)
        want, u_want = otb.transform(table, quantiles, references, distribution)
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(u, u_want, equal_nan=True)
        assert np.isnan(got[np.isnan(table)]).all() and not np.isnan(got[~np.isnan(table)]).any()
    q2, r2 = otb.fit_quantiles(x[:900], 240, 10000, 3)
    assert np.array_equal(q2, quantiles) and np.array_equal(r2, references)


def test_inverse_normal_cdf_is_as241():
    """the rational against the standard library's AS 241 (statistics.NormalDist.inv_cdf) at the branch edges and in the tails"""
    from statistics import NormalDist
    p = np.concatenate([np.linspace(1e-7, 1 - 1e-7, 4001), [0.075, 0.925, 0.0749999, 0.9250001, otb.U_LO, otb.U_HI,
                                                           np.exp(-25.0), np.exp(-25.0000001), 1e-300]])
    want = np.array([NormalDist().inv_cdf(float(v)) for v in p])
    for got in (tabular.ndtri(p), otb.ndtri(p)):
        assert np.abs(got - want).max() <= 4 * np.spacing(np.abs(want)).max()
    assert np.array_equal(tabular.ndtri(p), otb.ndtri(p))
    assert np.isnan(tabular.ndtri(np.array([np.nan]))).all()


@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture_of_the_reference_preprocessor(case):
    g = np.load(GOLDEN)
    x, y = g[f"{case}_x_train"].astype(np.float64), g[f"{case}_y_train"].astype(np.float64)
    pre = tabular.TabularPreprocessor(random_state=1337, quantile_transform=True, quantile_noise=1e-3, y_normalize=True)
    assert pre.fit(x, y) is pre
    # the noise rule: the product fits on the table the restatement of data.py:243-247 gives
    q_noise, _ = otb.fit_quantiles(otb.noisy(x, 1e-3, 1337), 2000, 10000, 1337)
    assert np.array_equal(pre.quantiles_, q_noise)
    assert not np.array_equal(pre.quantiles_, otb.fit_quantiles(x, 2000, 10000, 1337)[0])
    q = g[f"{case}_quantiles"]
    assert pre.quantiles_.shape == q.shape and (np.abs(pre.quantiles_ - q) <= 1e-12 * np.maximum(1.0, np.abs(q))).all()
    assert np.array_equal(pre.references_, g[f"{case}_references"])
    t_train, y_norm = pre.transform(x, y, backend="host")
    float32_criterion(t_train, g[f"{case}_t_train"])
    float32_criterion(pre.transform(g[f"{case}_x_valid"], backend="host"), g[f"{case}_t_valid"])
    assert abs(pre.y_mu - g[f"{case}_y_mu"]) <= 4 * np.spacing(abs(g[f"{case}_y_mu"]))
    assert abs(pre.y_std - g[f"{case}_y_std"]) <= 4 * np.spacing(g[f"{case}_y_std"])
    assert y_norm.dtype == np.float32 and np.abs(y_norm - g[f"{case}_y_norm"]).max() <= np.spacing(np.float32(np.abs(y_norm).max()))
    assert pre.feature_dimensionalities == [1] * x.shape[1]


def test_one_hot_order_position_unseen_values_and_labels():
    rows = [[0.5, "red", 3.0, 7], [1.5, "blue", 4.0, 9], [2.5, "red", 5.0, 7], [3.5, "green", 6.0, 8]]
    table = np.array(rows, dtype=object)
    pre = tabular.TabularPreprocessor(cat_features=["colour", "code"]).fit(table, columns=["a", "colour", "b", "code"])
    assert pre.categories_ == {"colour": ["red", "blue", "green"], "code": [7, 9, 8]}   # first appearance, not sorted
    assert pre.feature_dimensionalities == [1, 3, 1, 3] and pre.feature_labels == ["a", "colour", "b", "code"]
    assert pre.column_labels == ["a", "colour=red", "colour=blue", "colour=green", "b", "code=7", "code=9", "code=8"]
    want, categories, dims = otb.one_hot(rows, [1, 3])
    got = pre.transform(table, backend="host", columns=["a", "colour", "b", "code"])
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32)) and dims == pre.feature_dimensionalities
    assert np.array_equal(got[0], [0.5, 1, 0, 0, 3.0, 1, 0, 0])   # the group stands where the column stood
    unseen = np.array([[9.0, "violet", 1.0, 9]], dtype=object)
    got = pre.transform(unseen, backend="host", columns=["a", "colour", "b", "code"])
    assert np.array_equal(got, otb.one_hot(unseen.tolist(), [1, 3], categories)[0].astype(np.float32))
    assert np.array_equal(got[0], [9.0, 0, 0, 0, 1.0, 0, 1, 0])   # an unseen value gives all zeros
    with pytest.raises(NotImplementedError):
        tabular.TabularPreprocessor(one_hot=False)
    with pytest.raises(ValueError):
        pre.transform(table, backend="host", columns=["a", "b", "colour", "code"])


def test_one_hot_columns_pass_through_the_noise_and_the_quantiles():
    """the noise and the quantile tables cover every column after the one-hot (data.py:239-247)"""
    rng = np.random.default_rng(2)
    x = np.stack([rng.standard_normal(300), rng.integers(0, 3, 300).astype(float)], 1).astype(np.float32).astype(np.float64)
    pre = tabular.TabularPreprocessor(random_state=7, cat_features=[1], quantile_transform=True).fit(x)
    enc, _, dims = otb.one_hot(x.tolist(), [1])
    assert pre.feature_dimensionalities == dims == [1, 3] and pre.quantiles_.shape == (300, 4)
    q, r = otb.fit_quantiles(otb.noisy(enc, 1e-3, 7), 2000, 10000, 7)
    assert np.array_equal(pre.quantiles_, q)
    assert np.array_equal(pre.transform(x, backend="host"), otb.transform(enc, q, r, 0)[0])


def test_device_backend_without_a_gpu_raises_and_pandas_is_not_imported():
    import subprocess
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import dib_amd; assert 'pandas' not in sys.modules; "
            "import torch; pre = dib_amd.TabularPreprocessor(quantile_transform=True).fit(np.arange(12.0).reshape(6, 2)); "
            "pre.transform(np.zeros((2, 2)), backend='host'); assert 'pandas' not in sys.modules\n"
            "if not torch.cuda.is_available():\n"
            "    try:\n        pre.transform(np.zeros((2, 2)))\n    except RuntimeError as e:\n        assert 'needs a GPU' in str(e)\n"
            "    else:\n        raise SystemExit('the device backend fell back')\n" % ROOT)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_dataframe_input():
    pd = pytest.importorskip("pandas")
    x = mixed_table(200)[:, :3]
    frame = pd.DataFrame(x, columns=["u", "v", "w"])
    pre = tabular.TabularPreprocessor(random_state=3, quantile_transform=True).fit(frame)
    assert pre.feature_labels == ["u", "v", "w"]
    ref = tabular.TabularPreprocessor(random_state=3, quantile_transform=True).fit(x)
    assert np.array_equal(pre.quantiles_, ref.quantiles_)
    assert np.array_equal(pre.transform(frame, backend="host"), ref.transform(x, backend="host"))


def _write_table(path, n=200, seed=0):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.standard_normal(n), rng.exponential(size=n), rng.standard_normal(n), rng.integers(0, 4, n).astype(float),
                  rng.integers(0, 3, n).astype(float)], 1).astype(np.float32)
    y = (x[:, 0] + (x[:, 4] == 1) > 0.3).astype(np.int64)
    np.savez(path, x=x, y=y, columns=np.array(["a", "b", "c", "d", "kind"]))
    return x, y


def test_fetch_table_keys_shapes_split_and_nan_refusal(tmp_path):
    path = str(tmp_path / "table.npz")
    x, y = _write_table(path)
    d = data.DATASETS["table"](table_path=path, table_categorical=["kind"], table_backend="host", seed=4)
    for key in ("x_train", "y_train", "x_valid", "y_valid", "feature_dimensionalities", "number_features", "output_dimensionality",
                "output_activation_fn", "loss", "loss_is_info_based", "metrics", "x_valid_raw", "feature_labels", "preprocessor"):
        assert key in d, key
    assert d["feature_dimensionalities"] == [1, 1, 1, 1, 3] and d["number_features"] == 5
    assert d["feature_labels"] == ["a", "b", "c", "d", "kind"]
    assert d["x_train"].shape == (160, 7) and d["x_valid"].shape == (40, 7) and d["x_valid_raw"].shape == (40, 7)
    assert d["x_train"].dtype == d["x_valid"].dtype == d["x_valid_raw"].dtype == np.float32
    assert d["y_train"].shape == (160, 1) and d["y_valid"].shape == (40, 1)
    assert d["output_dimensionality"] == 2 and d["loss_is_info_based"] and d["metrics"] == ["accuracy"]
    assert d["loss"].kind.startswith("sparse_cce")
    # the split: a seeded shuffle, the first 80 % train; the preprocessor is fitted on the training rows alone
    order = np.random.RandomState(4).permutation(200)
    assert np.array_equal(d["y_train"][:, 0], y[order[:160]]) and np.array_equal(d["y_valid"][:, 0], y[order[160:]])
    raw = d["x_valid_raw"]
    assert np.array_equal(raw[:, :4], x[order[160:], :4]) and set(np.unique(raw[:, 4:])) <= {0.0, 1.0}
    enc, _, _ = otb.one_hot(x[order[:160]].astype(np.float64).tolist(), [4])
    q, r = otb.fit_quantiles(otb.noisy(enc, 1e-3, 1337), 2000, 10000, 1337)
    assert np.array_equal(d["preprocessor"].quantiles_, q)
    assert np.array_equal(d["x_train"], otb.transform(enc, q, r, 0)[0])
    # regression: a normalised target, mse, not information based; the target taken from the table by name
    np.savez(path, x=x, columns=np.array(["a", "b", "c", "d", "kind"]))
    d = data.fetch_table(table_path=path, table_problem="regression", table_target="b", table_backend="host", table_valid_fraction=0.25)
    assert d["loss"] == "mse" and not d["loss_is_info_based"] and d["output_dimensionality"] == 1
    assert d["feature_labels"] == ["a", "c", "d", "kind"] and d["x_train"].shape == (150, 4)
    assert abs(float(d["y_train"].mean())) < 1e-6 and abs(float(d["y_train"].std()) - 1.0) < 1e-5
    x[3, 2] = x[17, 0] = np.nan
    np.savez(path, x=x, y=y)
    with pytest.raises(ValueError, match="2 of the table's 200 rows"):
        data.fetch_table(table_path=path, table_backend="host")
    with pytest.raises(ValueError):
        data.fetch_table()


def test_train_command_line_takes_the_table_dataset():
    a = train.get_args(["--dataset", "table", "--table_path", "t.npz", "--table_problem", "regression", "--table_categorical", "kind", "4",
                        "--table_n_quantiles", "500", "--table_valid_fraction", "0.1", "--table_quantile_noise", "0.01", "--table_target", "y"])
    assert (a.dataset, a.table_path, a.table_problem, a.table_categorical) == ("table", "t.npz", "regression", ["kind", "4"])
    assert (a.table_n_quantiles, a.table_valid_fraction, a.table_quantile_noise, a.table_target) == (500, 0.1, 0.01, "y")
    d = train.get_args([])   # the existing flags and their defaults do not move
    assert (d.dataset, d.batch_size, d.learning_rate, d.seed, d.table_path, d.table_categorical) == ("boolean_circuit", 128, 3e-4, 0, None, [])


def test_quantile_supported_at_the_edges_of_the_envelope():
    from dib_amd import _lib
    lib = _lib.load_library()
    lo, hi, cols = _lib.TABULAR_MIN_QUANTILES, _lib.TABULAR_MAX_QUANTILES, _lib.TABULAR_MAX_COLS
    assert (lo, hi, cols) == (2, 10000, 65535)
    for nq, nc, dist, want in [(lo, 1, 0, 1), (hi, cols, 1, 1), (lo - 1, 1, 0, 0), (hi + 1, 1, 0, 0), (lo, cols + 1, 0, 0), (lo, 0, 0, 0),
                               (0, 1, 0, 0), (-5, 1, 0, 0), (2000, 64, 2, 0), (2000, 64, -1, 0)]:
        assert lib.dib_quantile_supported(nq, nc, dist) == want, (nq, nc, dist)
    # a refused call returns before it touches the device: the codes, without a GPU
    null = None
    assert lib.dib_quantile_transform(null, 1, 1, 1, null, null, 2000, 0, null, 1, null, null) == -1   # DIB_E_ARG
