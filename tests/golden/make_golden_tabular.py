"""Fixture of the tabular front end (dib_amd.tabular): the reference's own `MyPreprocessor` (reference data.py:178-297) EXECUTED
on two small tables.  Run where the reference lies, only there:
    python tests/golden/make_golden_tabular.py
The reference's data.py is imported as it stands behind empty stand-in modules for tensorflow, category_encoders and nodegam
(cat_features=None touches none of them); nothing of it is copied here, only the arrays it produces are stored, in
tests/golden/tabular_preprocessor.npz:
  a  400 x 5, no subsampling: normal, exponential, 5-level discrete, rounded-to-0.1 and binary columns; 120 held-out rows, some
     of them far outside the fitted range
  b  12 000 x 2, which subsamples 10 000 rows: a heavy-tailed column and a normal one rounded to 0.001; 400 held-out rows
per case the raw tables and y (float32: every value is float32-representable, the reference is fed their float64 widening in a
float64 DataFrame), quantiles_, references_, the transformed training and held-out rows, y_mu, y_std and the normalised y.
MyPreprocessor(random_state=1337, quantile_transform=True, quantile_noise=1e-3, y_normalize=True) as the reference's fetchers
build it.  The arrays record the behaviour of the scikit-learn installed where this ran (1.7.2, NumPy's nanpercentile and
SciPy's norm.ppf behind it)."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _Empty(types.ModuleType):
    """a module whose every attribute is another empty module: `import x`, `from x import y`, `x.y.z` all succeed"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        m = _Empty(self.__name__ + "." + name)
        setattr(self, name, m)
        return m


def reference_data_module():
    for name in ("tensorflow", "category_encoders", "nodegam"):
        sys.modules.setdefault(name, _Empty(name))
    spec = importlib.util.spec_from_file_location("reference_data", os.path.join(REF, "data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tables():
    rng = np.random.default_rng(20260)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    n, nv = 400, 120
    a = np.stack([rng.standard_normal(n + nv), rng.exponential(size=n + nv), rng.integers(0, 5, n + nv).astype(np.float64),
                  np.round(rng.standard_normal(n + nv), 1), rng.integers(0, 2, n + nv).astype(np.float64)], 1)
    a[n:n + 20] *= 50.0          # held-out rows far outside the fitted range
    a[n + 20:n + 30] -= 40.0
    ya = a[:, 0] * 3.0 + a[:, 2] + 0.1 * rng.standard_normal(n + nv) + 7.0
    n2, nv2 = 12000, 400
    b = np.stack([rng.standard_t(2.0, n2 + nv2), np.round(rng.standard_normal(n2 + nv2), 3)], 1)
    yb = np.round(np.tanh(b[:, 0]) - 0.5 * b[:, 1] + 0.05 * rng.standard_normal(n2 + nv2), 2)
    return {"a": (f32(a[:n]), f32(ya[:n]), f32(a[n:])), "b": (f32(b[:n2]), f32(yb[:n2]), f32(b[n2:]))}


def main():
    import pandas as pd
    import sklearn
    data = reference_data_module()
    out = {}
    for case, (x_train, y_train, x_valid) in tables().items():
        pre = data.MyPreprocessor(random_state=1337, quantile_transform=True, quantile_noise=1e-3, y_normalize=True)
        frame = lambda a: pd.DataFrame(a.astype(np.float64), columns=np.arange(a.shape[1]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            pre.fit(frame(x_train), y_train.astype(np.float64))
            t_train, y_norm = pre.transform(frame(x_train), y_train.astype(np.float64))
            t_valid = pre.transform(frame(x_valid))
        qt = pre.transformers[-1]
        assert t_train.dtype == np.float32 and t_valid.dtype == np.float32 and y_norm.dtype == np.float32
        out.update({f"{case}_x_train": x_train, f"{case}_y_train": y_train, f"{case}_x_valid": x_valid,
                    f"{case}_quantiles": qt.quantiles_, f"{case}_references": qt.references_, f"{case}_t_train": t_train,
                    f"{case}_t_valid": t_valid, f"{case}_y_mu": np.float64(pre.y_mu), f"{case}_y_std": np.float64(pre.y_std),
                    f"{case}_y_norm": y_norm})
        print(case, x_train.shape, "quantiles", qt.quantiles_.shape, "range of the transformed rows", t_train.min(), t_train.max(),
              t_valid.min(), t_valid.max())
    path = os.path.join(HERE, "tabular_preprocessor.npz")
    np.savez_compressed(path, sklearn_version=np.array(sklearn.__version__), **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
