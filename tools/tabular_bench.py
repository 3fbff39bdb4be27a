"""The tabular front end's quantile transform, on one box in one process:

    python tools/tabular_bench.py --out profiles/tabular_bench.json [--variant NAME=exp/lib_NAME.so ...]

for the benchmark's table (2^20 x 64 at 2000 quantiles) and the mice-protein width (2^16 x 77):
  - dib_quantile_transform alone (include/dib_tabular.h): HIP events around the launch, median of --repeats after warm-up, next to
    a plain device copy of the same bytes (4 in + 4 out per element) - the floor it is judged against - timed the same way,
    the two alternating; every --variant library (tools/build_variant.sh) is timed in the same loop on the same buffers and
    its output compared with the product's bit for bit;
  - TabularPreprocessor.transform(backend="device") from host table to host result (upload, launch, read-back: host clock);
  - the "host" backend (float64 NumPy) and, where scikit-learn is importable, QuantileTransformer.transform on the same table:
    host clock, --host-repeats runs (these take seconds each);
  - TabularPreprocessor.fit (noise, subsample, nanpercentile; host).
The device output is compared with the host backend's before anything is timed."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": len(ms)}


def _events_alternating(fns, repeats):
    """{name: stats} of device-event timings; the candidates take turns inside every repeat"""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: _stat(v) for k, v in ms.items()}


def _host(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stat(ms)


def bench(n_rows, n_cols, n_quantiles, args, variants):
    import torch

    from dib_amd import _lib, tabular
    rng = np.random.default_rng(n_cols)
    x = rng.standard_normal((n_rows, n_cols), dtype=np.float32)
    x[:, 1::4] = np.round(x[:, 1::4], 1)       # discrete columns: runs of equal quantiles
    x[:, 2::4] = np.exp(x[:, 2::4])
    pre = tabular.TabularPreprocessor(random_state=1337, quantile_transform=True, n_quantiles=n_quantiles)
    rec = {"rows": n_rows, "columns": n_cols, "quantiles": n_quantiles, "bytes_in_and_out": 8 * n_rows * n_cols}
    rec["fit_host"] = _host(lambda: pre.fit(x), args.host_repeats)
    lib = _lib.load_library()
    x_d = torch.from_numpy(x).cuda()
    q_d, r_d = pre._tables_on(x_d.device)
    out, copy = torch.empty_like(x_d), torch.empty_like(x_d)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(library, dst):
        return lambda: _lib.check(library.dib_quantile_transform(p(x_d), n_cols, n_rows, n_cols, p(q_d), p(r_d), n_quantiles, 0,
                                                                 p(dst), n_cols, None, stream), "dib_quantile_transform")

    launch(lib, out)()
    torch.cuda.synchronize()
    host_out = pre.transform(x, backend="host")
    got = out.cpu().numpy()
    rec["device_vs_host_backend"] = {"elements": int(got.size), "not_bit_equal": int((got != host_out).sum()),
                                     "max_abs_difference": float(np.abs(got - host_out).max())}
    fns = {"dib_quantile_transform": launch(lib, out), "device_copy": lambda: copy.copy_(x_d)}
    outs = {}
    for name, vlib in variants.items():
        outs[name] = torch.empty_like(x_d)
        fns["variant_" + name] = launch(vlib, outs[name])
    rec.update(_events_alternating(fns, args.repeats))
    for name, t in outs.items():
        rec["variant_" + name]["bit_equal_to_product"] = bool(torch.equal(t, out))
    k, c = rec["dib_quantile_transform"]["median_ms"], rec["device_copy"]["median_ms"]
    rec["kernel_over_copy"] = k / c
    rec["kernel_GB_per_s"] = rec["bytes_in_and_out"] / (k * 1e-3) / 1e9
    rec["copy_GB_per_s"] = rec["bytes_in_and_out"] / (c * 1e-3) / 1e9
    torch.cuda.synchronize()
    rec["transform_device_backend_host_to_host"] = _host(lambda: pre.transform(x, backend="device"), max(args.host_repeats, 5))
    rec["transform_host_backend"] = _host(lambda: pre.transform(x, backend="host"), args.host_repeats)
    try:
        import warnings

        import sklearn
        from sklearn.preprocessing import QuantileTransformer
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            qt = QuantileTransformer(n_quantiles=n_quantiles, output_distribution="normal", random_state=1337).fit(x[:20000].astype(np.float64))
        qt.quantiles_, qt.references_ = pre.quantiles_, pre.references_
        x64 = x.astype(np.float64)
        rec["transform_sklearn"] = _host(lambda: qt.transform(x64), args.host_repeats)
        rec["transform_sklearn"]["version"] = sklearn.__version__
    except ImportError:
        rec["transform_sklearn"] = "scikit-learn not importable on this box: not measured"
    rec["host_seconds_removed_per_table"] = (rec["transform_host_backend"]["median_ms"]
                                             - rec["transform_device_backend_host_to_host"]["median_ms"]) * 1e-3
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabular_bench.json"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library to time alongside")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tabular_bench.py needs a GPU")
    if args.repeats < 20:
        raise SystemExit("--repeats: at least 20 (the figures are medians)")
    from dib_amd import _lib
    variants = {}
    for spec in args.variant:
        name, path = spec.split("=", 1)
        v = ctypes.CDLL(os.path.abspath(path))
        v.dib_quantile_transform.restype, v.dib_quantile_transform.argtypes = _lib.SIGNATURES_TABULAR["dib_quantile_transform"]
        variants[name] = v
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "kernel, copy and variants: HIP events, alternating, median of repeats after 3 warm-up calls each; host entries: "
                     "host clock, the device synchronised by the read-back",
           "benchmark_table_2^20x64": bench(1 << 20, 64, 2000, args, variants),
           "mice_protein_width_2^16x77": bench(1 << 16, 77, 2000, args, variants)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
