"""The tabular front end: the reference's `MyPreprocessor` (reference data.py:178-297) with its quantile transform on the device.

    pre = TabularPreprocessor(random_state=1337, cat_features=['colour'], quantile_transform=True, y_normalize=True)
    pre.fit(x_train, y_train)                       # host, NumPy
    x, y = pre.transform(x_train, y_train)          # one-hot on the host, one upload, one dib_quantile_transform launch

The four steps of the reference, in its order:
  one-hot    every `cat_features` column is replaced, in place, by one 0/1 column per category, the categories in order of first
             appearance in the fit data; a value unseen at fit time gives all zeros.  (The reference calls category_encoders'
             OneHotEncoder; that package is not a dependency here and this rule is a written restatement of it, not a comparison.)
  noise      for the quantile FIT only (data.py:243-247): RandomState(random_state).randn scaled by
             quantile_noise / maximum(std, quantile_noise), added to every column after the one-hot
  quantiles  sklearn's QuantileTransformer(n_quantiles, output_distribution, subsample, random_state): `quantile_fit` and
             `quantile_transform_host` restate its dense fit and its forward transform in float64 NumPy, bit for bit on a float64
             ndarray (tests/test_tabular_host.py holds them to sklearn); `quantile_transform_device` is the same rule in one HIP
             launch (include/dib_tabular.h)
  target     (y - mean) / std when y_normalize

Both transform backends read the table as float32 - what the model trains on - and widen it exactly: a float64 table whose
values are float32-representable gives sklearn's float64 result cast to float32.  sklearn fed a float32 DataFrame keeps float32
working arrays and lands up to 3.5e-3 away in the tails; that accident of dtype handling is not replicated.
pandas is never imported here: a DataFrame is recognised by its `columns` and `values`.
"""
from __future__ import annotations

import ctypes

import numpy as np

BOUNDS_THRESHOLD = 1e-7   # sklearn.preprocessing._data.BOUNDS_THRESHOLD
_U_LO = BOUNDS_THRESHOLD - np.spacing(1.0)
_U_HI = 1.0 - _U_LO
_MISSING = object()


def _horner(coefficients, r):
    acc = np.full_like(r, coefficients[0])
    for c in coefficients[1:]:
        acc = acc * r + c
    return acc


_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
      6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def ndtri(p):
    """The normal quantile by Wichura's Algorithm AS 241 (PPND16), float64, p in (0, 1); NaN stays NaN.  The kernel's rational
    (csrc/dib_tabular.h dib_tab_ndtri), operation for operation."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    q = p - 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        central = np.abs(q) <= 0.425
        r = 0.180625 - q[central] * q[central]
        out[central] = _horner(_A, r) * q[central] / _horner(_B, r)
        tail = ~central & ~np.isnan(p)
        qt = q[tail]
        r = np.sqrt(-np.log(np.where(qt <= 0.0, p[tail], 1.0 - p[tail])))
        near = r <= 5.0
        x = np.empty_like(r)
        x[near] = _horner(_C, r[near] - 1.6) / _horner(_D, r[near] - 1.6)
        x[~near] = _horner(_E, r[~near] - 5.0) / _horner(_F, r[~near] - 5.0)
        out[tail] = np.where(qt < 0.0, -x, x)
    return out


def quantile_fit(x, n_quantiles=2000, subsample=10000, random_state=None):
    """sklearn's QuantileTransformer._dense_fit on a float64 matrix [n, d] -> (quantiles_ [n_q, d], references_ [n_q]):
    n_q = max(1, min(n_quantiles, n)), references = linspace(0, 1, n_q), the rows above `subsample` drawn as
    sklearn.utils.resample(replace=False) draws them, quantiles = maximum.accumulate(nanpercentile(x, 100 references))."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if subsample is not None and n_quantiles > subsample:
        raise ValueError(f"n_quantiles ({n_quantiles}) cannot be greater than subsample ({subsample})")
    n_q = max(1, min(int(n_quantiles), n))
    references = np.linspace(0, 1, n_q, endpoint=True)
    if subsample is not None and subsample < n:
        idx = np.arange(n)
        np.random.RandomState(random_state).shuffle(idx)
        x = x[idx[:subsample]]
    quantiles = np.maximum.accumulate(np.nanpercentile(x, references * 100, axis=0))
    return quantiles, references


def quantile_transform_host(x, quantiles, references, output_distribution="normal", return_u=False):
    """sklearn's QuantileTransformer._transform_col (forward) on every column of x [n, d], in float64 from the float32 values of
    x -> float32 [n, d] (and, with return_u, the float64 u that entered the inverse CDF): the rule of include/dib_tabular.h."""
    distribution = _distribution(output_distribution)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    quantiles, references = np.asarray(quantiles, dtype=np.float64), np.asarray(references, dtype=np.float64)
    if x.ndim != 2 or quantiles.ndim != 2 or quantiles.shape != (references.shape[0], x.shape[1]):
        raise ValueError(f"x {x.shape}, quantiles {quantiles.shape}, references {references.shape} do not fit together")
    u = np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for c in range(x.shape[1]):
            col, q = x[:, c], quantiles[:, c]
            if distribution == 0:
                lower, upper = col - BOUNDS_THRESHOLD < q[0], col + BOUNDS_THRESHOLD > q[-1]
            else:
                lower, upper = col == q[0], col == q[-1]
            finite = ~np.isnan(col)
            uc = np.full(col.shape, np.nan)
            uc[finite] = 0.5 * (np.interp(col[finite], q, references) - np.interp(-col[finite], -q[::-1], -references[::-1]))
            uc[upper] = 1.0
            uc[lower] = 0.0
            u[:, c] = np.clip(uc, _U_LO, _U_HI) if distribution == 0 else uc
    out = (ndtri(u) if distribution == 0 else u).astype(np.float32)
    return (out, u) if return_u else out


def _distribution(name):
    from ._lib import TABULAR_DISTRIBUTIONS
    if name not in TABULAR_DISTRIBUTIONS:
        raise ValueError(f"output_distribution must be one of {sorted(TABULAR_DISTRIBUTIONS)}, got {name!r}")
    return TABULAR_DISTRIBUTIONS[name]


def quantile_transform_device(x, quantiles_t, references, output_distribution="normal", out=None, u64=None, n_cols=None):
    """One dib_quantile_transform launch on the current stream.  x: float32 CUDA tensor [n, >= n_cols] (its row stride is the
    leading dimension); quantiles_t: float64 CUDA tensor [n_cols, n_q] (every column's table contiguous); references: float64
    CUDA tensor [n_q]; out (optional) float32 [n, >= n_cols]; u64 (optional) float64 [n, n_cols] contiguous.  Returns out."""
    import torch
    from . import _lib
    from ._host import stream_ptr
    lib = _lib.load_library()
    n_cols = int(quantiles_t.shape[0] if n_cols is None else n_cols)
    for t, dt in ((x, torch.float32), (quantiles_t, torch.float64), (references, torch.float64)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt):
            raise ValueError("quantile_transform_device takes float32 x and float64 tables on the GPU")
    if x.dim() != 2 or x.stride(1) != 1 or not quantiles_t.is_contiguous() or not references.is_contiguous():
        raise ValueError("x must be a row-major matrix and the tables contiguous")
    if quantiles_t.shape != (n_cols, references.shape[0]) or x.shape[1] < n_cols:
        raise ValueError(f"x {tuple(x.shape)}, quantiles {tuple(quantiles_t.shape)}, references {tuple(references.shape)} do not fit together")
    if out is None:
        out = torch.empty((x.shape[0], n_cols), dtype=torch.float32, device=x.device)
    if u64 is not None and not (u64.is_contiguous() and u64.dtype == torch.float64 and u64.numel() == x.shape[0] * n_cols):
        raise ValueError("u64 must be a contiguous float64 [n_rows, n_cols]")
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(lib.dib_quantile_transform(p(x), x.stride(0), x.shape[0], n_cols, p(quantiles_t), p(references), references.shape[0],
                                          _distribution(output_distribution), p(out), out.stride(0), p(u64),
                                          stream_ptr(x.device)),
               "dib_quantile_transform")
    return out


def _table(X, columns=None):
    """(2-D array of the values, list of column names) of a NumPy array or of a DataFrame (anything with columns and values)"""
    if hasattr(X, "columns") and hasattr(X, "values"):
        values, names = np.asarray(X.values), list(X.columns)
    else:
        values = np.asarray(X)
        names = None
    if values.ndim == 1:
        values = values[:, None]
    if values.ndim != 2:
        raise ValueError(f"a table is two-dimensional, got shape {values.shape}")
    if columns is not None:
        names = list(columns)
    if names is None:
        names = list(range(values.shape[1]))
    if len(names) != values.shape[1]:
        raise ValueError(f"{len(names)} column names for {values.shape[1]} columns")
    return values, names


class TabularPreprocessor:
    """The reference's MyPreprocessor (data.py:178-297; its signature and defaults, plus sklearn's `subsample`); see the module
    docstring.  After fit: feature_dimensionalities (1 per continuous column, k per one-hot group, in column order),
    feature_labels (one per feature), column_labels (one per output column), categories_, quantiles_ [n_q, width],
    references_ [n_q], y_mu, y_std."""

    def __init__(self, random_state=1377, cat_features=None, y_normalize=False, quantile_transform=False,
                 output_distribution='normal', n_quantiles=2000, quantile_noise=1e-3, one_hot=True, subsample=10000):
        if not one_hot:
            raise NotImplementedError("one_hot=False is NODE-GAM's leave-one-out target encoding; the reference's modification, "
                                      "and the only encoding here, is the one-hot")
        _distribution(output_distribution)
        self.random_state = random_state
        self.cat_features = None if cat_features is None else list(cat_features)
        self.y_normalize = y_normalize
        self.quantile_transform = quantile_transform
        self.output_distribution = output_distribution
        self.n_quantiles = n_quantiles
        self.quantile_noise = quantile_noise
        self.one_hot = one_hot
        self.subsample = subsample
        self.y_mu, self.y_std = 0, 1
        self.feature_names = None
        self.categories_ = {}
        self.quantiles_ = self.references_ = None
        self.feature_dimensionalities = self.feature_labels = self.column_labels = None
        self._device_tables = {}

    # ---- host -----------------------------------------------------------------------------------
    def _encode(self, values, names):
        """float64 [n, width]: every categorical column replaced by its 0/1 columns"""
        if names != self.feature_names:
            raise ValueError(f"columns {names} are not the fitted columns {self.feature_names}")
        if not self.categories_:
            return np.asarray(values, dtype=np.float64)
        cols = []
        for j, name in enumerate(names):
            if name in self.categories_:
                cols += [(values[:, j] == cat).astype(np.float64) for cat in self.categories_[name]]
            else:
                cols.append(np.asarray(values[:, j], dtype=np.float64))
        return np.stack(cols, axis=1)

    def fit(self, X, y=None, columns=None):
        values, names = _table(X, columns)
        self.feature_names = names
        self.categories_ = {}
        for name in self.cat_features or ():
            if name not in names:
                raise ValueError(f"cat_features: no column {name!r} among {names}")
            seen = {}
            for v in values[:, names.index(name)].tolist():
                seen.setdefault(v, None)   # order of first appearance
            self.categories_[name] = list(seen)
        self.feature_dimensionalities = [len(self.categories_[n]) if n in self.categories_ else 1 for n in names]
        self.feature_labels = [str(n) for n in names]
        self.column_labels = []
        for n in names:
            self.column_labels += [f"{n}={c}" for c in self.categories_[n]] if n in self.categories_ else [str(n)]
        self._device_tables = {}
        self.quantiles_ = self.references_ = None
        if self.quantile_transform:
            quantile_train = self._encode(values, names).copy()
            if self.quantile_noise:   # data.py:243-247, literally
                r = np.random.RandomState(self.random_state)
                stds = np.std(quantile_train, axis=0, keepdims=True)
                noise_std = self.quantile_noise / np.maximum(stds, self.quantile_noise)
                quantile_train += noise_std * r.randn(*quantile_train.shape)
            self.quantiles_, self.references_ = quantile_fit(quantile_train, self.n_quantiles, self.subsample, self.random_state)
        if y is not None and self.y_normalize:
            y = np.asarray(y)
            self.y_mu, self.y_std = y.mean(axis=0), y.std(axis=0)
        return self

    def _tables_on(self, device):
        import torch
        key = str(device)
        if key not in self._device_tables:
            self._device_tables[key] = (torch.from_numpy(np.ascontiguousarray(self.quantiles_.T)).to(device),
                                        torch.from_numpy(np.ascontiguousarray(self.references_)).to(device))
        return self._device_tables[key]

    def transform(self, X, y=_MISSING, backend="device", as_tensor=False, device=None, columns=None):
        """-> X float32 [n, width] (a NumPy array; the device tensor with as_tensor=True), or (X, y) when y is passed.
        backend "device": one upload, one launch (a float32 tensor already on the GPU is used where it lies when there are no
        categorical columns); "host": the same rule in float64 NumPy.  "device" without a GPU raises: there is no fallback.
        With quantile_transform=False the transform is the one-hot and a cast, and nothing is launched."""
        if backend not in ("device", "host"):
            raise ValueError(f"backend must be 'device' or 'host', got {backend!r}")
        if self.feature_names is None:
            raise RuntimeError("fit() the preprocessor first")
        x_dev = None
        if type(X).__module__.startswith("torch") and getattr(X, "is_cuda", False):
            if self.categories_:
                raise ValueError("categorical columns are encoded on the host: pass the raw table, not a device tensor")
            x_dev = X
        else:
            values, names = _table(X, columns)
            x32 = self._encode(values, names).astype(np.float32)
        if not self.quantile_transform:
            out = x_dev if x_dev is not None else x32
        elif backend == "host":
            if as_tensor:
                raise ValueError("as_tensor=True returns the device backend's tensor")
            out = quantile_transform_host(x_dev.cpu().numpy() if x_dev is not None else x32, self.quantiles_, self.references_,
                                          self.output_distribution)
        else:
            if self.references_.shape[0] < 2:
                raise ValueError("the device transform needs at least 2 quantiles (a preprocessor fitted on one row has 1)")
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("TabularPreprocessor.transform(backend='device') needs a GPU; backend='host' prepares data "
                                   "without one")
            if x_dev is None:
                x_dev = torch.from_numpy(x32).to(torch.device(device if device is not None else "cuda"))
            out = quantile_transform_device(x_dev, *self._tables_on(x_dev.device), self.output_distribution)
        if not as_tensor and not isinstance(out, np.ndarray):
            out = out.cpu().numpy()
        elif as_tensor and isinstance(out, np.ndarray):
            raise ValueError("as_tensor=True needs the device backend and quantile_transform=True")
        if y is _MISSING:
            return out
        if y is None:
            return out, None
        if self.y_normalize and self.y_mu is not None and self.y_std is not None:
            y = ((y - self.y_mu) / self.y_std).astype(np.float32)
        return out, y
