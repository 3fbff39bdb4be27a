"""Dataset dicts for the hot path, mirroring the reference's `data.DATASETS[name](**kwargs)` contract
(reference data.py:69-81, 397-406).  Shipped: the Boolean circuit (data.py:21-81, pure numpy), the
synthetic tabular generator BASELINE.md section 4 defines for the north-star benchmark, the double pendulum, and `table`: a
table of the user's own (.npz or .csv) through the pipeline every tabular fetcher of the reference feeds, its `MyPreprocessor`
(data.py:178-297; tabular.TabularPreprocessor, the quantile transform on the device).  The NODE-GAM fetchers themselves are
stubs returning None in the reference and download their data: those stay out of scope.
"""
from __future__ import annotations

import numpy as np

from . import losses

PAPER_CIRCUIT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, [1, 0, 1], [2, 8, 7], [0, 4, 3], [1, 11, 5], [2, 6, 12], [2, 13, 9],
                 [1, 14, 10], [0, 15, 2], [0, 17, 16]]  # reference data.py:40
_GATES = [np.logical_and, np.logical_or, np.logical_xor]


def random_circuit(number_input_gates, rng=None):
    """reference data.py:27-37: repeatedly join two live wires with a random gate until one remains."""
    rng = rng or np.random
    live = list(range(number_input_gates))
    spec = list(range(number_input_gates))
    while len(live) > 1:
        gate = int(rng.choice(len(_GATES)))
        a, b = [int(v) for v in rng.choice(live, size=2, replace=False)]
        live.append(len(spec))
        live.remove(a)
        live.remove(b)
        spec.append([gate, a, b])
    return spec


def truth_table(circuit_specification, number_input_gates):
    """reference data.py:42-53: full truth table in np.meshgrid (default 'xy') order."""
    grids = np.meshgrid(*[[0, 1]] * number_input_gates)
    table = np.reshape(np.stack(grids, -1), [-1, number_input_gates])
    for gate, a, b in circuit_specification[number_input_gates:]:
        table = np.concatenate([table, np.int32(_GATES[gate](table[:, a], table[:, b]))[:, None]], -1)
    return table


def fetch_boolean_circuit(**kwargs):
    """reference data.py:21-81."""
    number_input_gates = kwargs.get('boolean_number_input_gates', 10)
    if kwargs.get('boolean_random_circuit', False):
        spec = random_circuit(number_input_gates)
    else:
        spec, number_input_gates = PAPER_CIRCUIT, 10
    table = truth_table(spec, number_input_gates)
    x_train = 2 * table[:, :number_input_gates] - 1  # x -> {-1, +1}
    y_train = table[:, -1]
    feature_dimensionalities = [1] * number_input_gates
    return dict(x_train=x_train, y_train=y_train, x_valid=x_train, y_valid=y_train,
                feature_dimensionalities=feature_dimensionalities, number_features=len(feature_dimensionalities),
                output_dimensionality=1, output_activation_fn=None,
                loss=losses.BinaryCrossentropy(from_logits=True), loss_is_info_based=True, metrics=['accuracy'],
                circuit_specification=spec)


def fetch_synthetic_tabular(**kwargs):
    """BASELINE.md section 4 / SURVEY 8(d): x ~ N(0,1) [n, F] from default_rng(20241008);
    y = 1[sum_{j<8} w_j x_j + 0.5 x_0 x_1 > 0], w ~ N(0,1) from the same generator; BCE-from-logits."""
    n = int(kwargs.get('synthetic_rows', 1 << 20))
    F = int(kwargs.get('synthetic_features', 64))
    nv = int(kwargs.get('synthetic_valid_rows', min(n, 1 << 16)))
    rng = np.random.default_rng(20241008)
    x = rng.standard_normal((n, F), dtype=np.float32)
    w = rng.standard_normal(8).astype(np.float32)
    k = min(8, F)
    y = ((x[:, :k] @ w[:k] + (0.5 * x[:, 0] * x[:, 1] if F > 1 else 0.0)) > 0).astype(np.float32)
    return dict(x_train=x, y_train=y, x_valid=x[:nv], y_valid=y[:nv], feature_dimensionalities=[1] * F,
                number_features=F, output_dimensionality=1, output_activation_fn=None,
                loss=losses.BinaryCrossentropy(from_logits=True), loss_is_info_based=True, metrics=['accuracy'])


def fetch_double_pendulum(**kwargs):
    """reference data.py:83-147: predict the state `pendulum_time_delta` seconds ahead; 4 features
    (theta1 as a unit vector [2], dtheta1 [1], theta2 as a unit vector [2], dtheta2 [1]); loss 'infonce'.
    Generates the trajectories on first use (simulate_pendulum, `pendulum_number_trajectories` to keep it small).
    Defect A11 of SURVEY App. A (the reference's np.split makes the FIRST 10 % the training set) is not replicated:
    10 % of the trajectories are held out for validation."""
    import os
    data_path = kwargs.get('data_path', './data/')
    fname = os.path.join(data_path, 'double_pendulum.npy')
    if not os.path.exists(fname):
        from . import simulate_pendulum
        prm = {}
        if kwargs.get('pendulum_number_trajectories'):
            prm['number_trajectories'] = int(kwargs['pendulum_number_trajectories'])
        simulate_pendulum.simulate_double_pendulum(data_path=data_path, simulation_params_dict=prm,
                                                   rng=np.random.default_rng(kwargs.get('seed', 0)))
    arr = np.load(fname)
    time_delta = kwargs.get('pendulum_time_delta', 2.)

    def preprocess(a):  # data.py:100-107: angles -> (sin, -cos), velocities as is
        return np.stack([np.sin(a[:, :, 0]), -np.cos(a[:, :, 0]), a[:, :, 1], np.sin(a[:, :, 2]), -np.cos(a[:, :, 2]),
                         a[:, :, 3]], -1)

    n_valid = max(1, int(arr.shape[0] * 0.1))
    train, valid = preprocess(arr[n_valid:]), preprocess(arr[:n_valid])
    steps = int(time_delta / 0.02)  # dt_saving of the simulation (data.py:116-117)
    pair = lambda a: (a[:, :-steps].reshape(-1, 6).astype(np.float32), a[:, steps:].reshape(-1, 6).astype(np.float32))
    x_train, y_train = pair(train)
    x_valid, y_valid = pair(valid)
    dims = [2, 1, 2, 1]
    return dict(x_train=x_train, y_train=y_train, x_valid=x_valid, y_valid=y_valid, feature_dimensionalities=dims,
                number_features=len(dims), output_dimensionality=6, output_activation_fn=None, loss='infonce',
                loss_is_info_based=True, feature_labels=['theta1', 'theta1_dot', 'theta2', 'theta2_dot'])


def _load_table(path, target):
    """(x [n, d] float or object, y [n], column names of x) of an .npz with x, y and optional columns, or of a .csv"""
    if str(path).endswith('.npz'):
        with np.load(path, allow_pickle=False) as f:
            x = f['x']
            columns = [c.item() if hasattr(c, 'item') else c for c in f['columns']] if 'columns' in f.files else list(range(x.shape[1]))
            y = f['y'] if 'y' in f.files else None
        if y is not None:
            return x, np.asarray(y).reshape(len(x)), columns
    elif str(path).endswith('.csv'):
        try:
            import pandas as pd
        except ImportError as e:
            raise RuntimeError("a .csv table is read with pandas, which is not installed: save the table as an .npz with x, y "
                               "(and columns)") from e
        frame = pd.read_csv(path)
        x, columns = frame.values, list(frame.columns)
    else:
        raise ValueError(f"table_path must be an .npz or a .csv, got {path!r}")
    # the target is a column of the table: by name, by index, the last one by default
    j = len(columns) - 1 if target is None else _column_index(columns, target)
    keep = [k for k in range(len(columns)) if k != j]
    return x[:, keep], x[:, j], [columns[k] for k in keep]


def _column_index(columns, c):
    """a column given by its name, or by its index (an int, or its digits from the command line)"""
    if c in columns:
        return columns.index(c)
    try:
        j = int(c)
    except (TypeError, ValueError):
        raise ValueError(f"no column {c!r} among {columns}") from None
    if not -len(columns) <= j < len(columns):
        raise ValueError(f"column index {j} outside a table of {len(columns)} columns")
    return j % len(columns)


def fetch_table(**kwargs):
    """A table of the user's own through the reference's tabular pipeline (data.py:299-369 with MyPreprocessor(random_state=1337,
    quantile_transform=True) as every fetcher builds it): keys `table_path` (.npz with x, y, optional columns; .csv where pandas
    is installed), `table_target` (the target's column name or index when it is a column of the table; default the last),
    `table_problem` ('classification' | 'regression'), `table_categorical` (names or indices of the one-hot columns),
    `table_quantile_noise` (1e-3), `table_n_quantiles` (2000), `table_valid_fraction` (0.2), `table_backend` ('device' | 'host':
    where the quantile transform runs), `seed`.  The rows are shuffled with RandomState(seed) (the reference's shuffle is
    unseeded, data.py:325-340) and the first 1 - table_valid_fraction of them are the training set, on which the preprocessor
    is fitted.  Rows with NaN are refused.  Besides the reference's keys the dict carries `x_valid_raw` (the raw validation
    columns, one-hot groups as their 0/1 columns: what the compression matrices are labelled with), `feature_labels` and
    `preprocessor`."""
    from . import tabular
    path = kwargs.get('table_path')
    if not path:
        raise ValueError("dataset 'table' needs table_path (--table_path): an .npz with x, y and optional columns, or a .csv")
    problem = kwargs.get('table_problem', 'classification')
    if problem not in ('classification', 'regression'):
        raise ValueError(f"table_problem must be 'classification' or 'regression', got {problem!r}")
    x, y, columns = _load_table(path, kwargs.get('table_target'))
    cat = [columns[_column_index(columns, c)] for c in (kwargs.get('table_categorical') or [])]
    numeric = [j for j, c in enumerate(columns) if c not in cat]
    bad = np.isnan(np.asarray(x[:, numeric], dtype=np.float64)).any(axis=1)
    if problem == 'regression':
        bad |= np.isnan(np.asarray(y, dtype=np.float64).reshape(len(x), -1)).any(axis=1)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} of the table's {len(x)} rows hold NaN: fill or drop them first")
    order = np.random.RandomState(int(kwargs.get('seed', 0))).permutation(len(x))
    x, y = x[order], np.asarray(y)[order]
    n_train = len(x) - int(len(x) * float(kwargs.get('table_valid_fraction', 0.2)))
    if problem == 'classification':
        classes, y = np.unique(y, return_inverse=True)
        y = y.astype(np.float32).reshape(-1, 1)   # class indices, the layout SparseCategoricalCrossentropy reads
        loss, output_dimensionality, metrics, info_based = losses.SparseCategoricalCrossentropy(from_logits=True), len(classes), ['accuracy'], True
    else:
        y = np.asarray(y, dtype=np.float64).reshape(len(x), -1)
        loss, output_dimensionality, metrics, info_based = 'mse', 1, None, False
    pre = tabular.TabularPreprocessor(random_state=1337, cat_features=cat or None, y_normalize=(problem == 'regression'),
                                      quantile_transform=True, output_distribution='normal',
                                      n_quantiles=int(kwargs.get('table_n_quantiles', 2000)),
                                      quantile_noise=float(kwargs.get('table_quantile_noise', 1e-3)))
    pre.fit(x[:n_train], y[:n_train], columns=columns)
    backend = kwargs.get('table_backend', 'device')
    x_train, y_train = pre.transform(x[:n_train], y[:n_train], backend=backend, columns=columns)
    x_valid, y_valid = pre.transform(x[n_train:], y[n_train:], backend=backend, columns=columns)
    dims = list(pre.feature_dimensionalities)
    out = dict(x_train=x_train, y_train=y_train, x_valid=x_valid, y_valid=y_valid, feature_dimensionalities=dims,
               number_features=len(dims), output_dimensionality=output_dimensionality, output_activation_fn=None, loss=loss,
               loss_is_info_based=info_based, metrics=metrics,
               x_valid_raw=pre._encode(x[n_train:], columns).astype(np.float32), feature_labels=list(pre.feature_labels),
               preprocessor=pre)
    if problem == 'classification':
        out['classes'] = classes
    return out


DATASETS = {'boolean_circuit': fetch_boolean_circuit, 'synthetic_tabular': fetch_synthetic_tabular,
            'double_pendulum': fetch_double_pendulum, 'table': fetch_table}
