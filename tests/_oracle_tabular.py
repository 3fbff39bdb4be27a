"""Float64 restatement of the tabular front end (dib_amd.tabular, include/dib_tabular.h), independent of the product's code: the
interpolation is written out on np.searchsorted (the product's host backend calls np.interp), the AS 241 rational as the nested
expressions of the paper with every branch evaluated and selected (the product evaluates each branch on its own elements), the
one-hot as a loop over rows.  Used by tests/test_tabular_host.py (against sklearn and the product's host backend) and
tests/test_gpu_tabular.py (against the kernel)."""
import numpy as np

BOUNDS_THRESHOLD = 1e-7
U_LO = BOUNDS_THRESHOLD - 2.0 ** -52
U_HI = 1.0 - U_LO


def interp(x, xp, fp):
    """np.interp's rule for finite-or-infinite x on n >= 2 knots, element by element in float64"""
    x, xp, fp = np.asarray(x, np.float64), np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    n = xp.shape[0]
    j = np.searchsorted(xp, x, side="right") - 1          # the largest index with xp[j] <= x; -1 below the first knot
    jc = np.clip(j, 0, n - 2)
    with np.errstate(all="ignore"):
        slope = (fp[jc + 1] - fp[jc]) / (xp[jc + 1] - xp[jc])
        r = slope * (x - xp[jc]) + fp[jc]
        r2 = slope * (x - xp[jc + 1]) + fp[jc + 1]
    r = np.where(np.isnan(r), np.where(np.isnan(r2) & (fp[jc] == fp[jc + 1]), fp[jc], r2), r)
    r = np.where(xp[jc] == x, fp[jc], r)
    r = np.where(j >= n - 1, fp[n - 1], r)
    r = np.where(x > xp[n - 1], fp[n - 1], r)
    return np.where(j < 0, fp[0], r)


def ndtri(p):
    """Wichura (1988), Algorithm AS 241, PPND16"""
    p = np.asarray(p, np.float64)
    q = p - 0.5
    with np.errstate(all="ignore"):
        r = 0.180625 - q * q
        central = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
                       + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
                     + 1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q / \
                  (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
                       + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
                     + 4.2313330701600911252e+1) * r + 1.0)
        t = np.sqrt(-np.log(np.where(q <= 0.0, p, 1.0 - p)))
        r = t - 1.6
        near = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
                    + 1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r
                  + 4.63033784615654529590e+0) * r + 1.42343711074968357734e+0) / \
               (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
                    + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r
                  + 2.05319162663775882187e+0) * r + 1.0)
        r = t - 5.0
        far = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
                   + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r
                 + 5.46378491116411436990e+0) * r + 6.65790464350110377720e+0) / \
              (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
                   + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
                 + 5.99832206555887937690e-1) * r + 1.0)
        tail = np.where(t <= 5.0, near, far)
        tail = np.where(q < 0.0, -tail, tail)
        out = np.where(np.abs(q) <= 0.425, central, tail)
    return np.where(np.isnan(p), np.nan, out)


def transform(x, quantiles, references, distribution=0):
    """x [n, d] (read as float32), quantiles [n_q, d], references [n_q]; distribution 0 normal, 1 uniform
    -> (out float32 [n, d], u float64 [n, d] as it enters the inverse CDF)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    quantiles, references = np.asarray(quantiles, np.float64), np.asarray(references, np.float64)
    u = np.empty_like(x)
    for c in range(x.shape[1]):
        col, q = x[:, c], quantiles[:, c]
        nan = np.isnan(col)
        safe = np.where(nan, 0.0, col)
        uc = 0.5 * (interp(safe, q, references) - interp(-safe, -q[::-1], -references[::-1]))
        with np.errstate(all="ignore"):
            if distribution == 0:
                uc = np.where(safe + BOUNDS_THRESHOLD > q[-1], 1.0, uc)
                uc = np.where(safe - BOUNDS_THRESHOLD < q[0], 0.0, uc)
                uc = np.minimum(np.maximum(uc, U_LO), U_HI)
            else:
                uc = np.where(safe == q[-1], 1.0, uc)
                uc = np.where(safe == q[0], 0.0, uc)
        u[:, c] = np.where(nan, np.nan, uc)
    out = ndtri(u) if distribution == 0 else u
    return out.astype(np.float32), u


def fit_quantiles(x, n_quantiles=2000, subsample=10000, seed=None):
    """-> (quantiles [n_q, d], references [n_q]) of a float64 matrix"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    n_q = max(1, min(n_quantiles, n))
    references = np.linspace(0, 1, n_q)
    if subsample is not None and subsample < n:
        idx = np.arange(n)
        np.random.RandomState(seed).shuffle(idx)
        x = x[idx[:subsample]]
    return np.maximum.accumulate(np.nanpercentile(x, 100 * references, axis=0)), references


def noisy(x, quantile_noise, seed):
    """the table the quantiles are fitted on (reference data.py:243-247)"""
    x = np.array(x, np.float64)
    std = x.std(axis=0, keepdims=True)
    return x + quantile_noise / np.maximum(std, quantile_noise) * np.random.RandomState(seed).randn(*x.shape)


def one_hot(rows, cat_columns, categories=None):
    """rows: a list of rows (lists); cat_columns: the indices of the categorical columns.  -> (float64 [n, width], categories
    {column: values in order of first appearance}, feature dimensionalities).  With `categories` given nothing is learned and
    an unseen value gives zeros."""
    learn = categories is None
    if learn:
        categories = {c: [] for c in cat_columns}
        for row in rows:
            for c in cat_columns:
                if row[c] not in categories[c]:
                    categories[c].append(row[c])
    width = len(rows[0])
    out = []
    for row in rows:
        line = []
        for c in range(width):
            if c in categories:
                line += [1.0 if row[c] == v else 0.0 for v in categories[c]]
            else:
                line.append(float(row[c]))
        out.append(line)
    dims = [len(categories[c]) if c in categories else 1 for c in range(width)]
    return np.array(out, np.float64), categories, dims


def float32_criterion(got, want):
    """the criterion for float32 outputs: NaN in the same places, every finite element within 1 ulp, >= 99.9 % bit-equal"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    steps = np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64))
    steps = np.where(got[ok] == want[ok], 0, steps)   # -0.0 against 0.0
    print(f"{int((steps > 0).sum())} of {steps.size} elements differ, by at most {int(steps.max(initial=0))} ulp")
    assert (steps <= 1).all()
    assert (steps == 0).mean() >= 0.999
