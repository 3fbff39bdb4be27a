"""Kernel times of the MI-bound characterization at the notebook's sizes (one variable: 1 024 rows, 32 dimensions, 25 separation
scales), HIP events around whole entry-point calls, each figure the median of --repeats launches after one warm-up launch:

    python tools/mi_bounds_bench.py --out profiles/mi_bounds_bench.json

  - dib_mi_monte_carlo: one launch of the sweep's Monte-Carlo estimate (runs of 10 000 samples; a launch holds as many (scale,
    run) groups as mi_characterization.MAX_INDICES_PER_LAUNCH allows, the 5 000 groups of a sweep take three such launches);
  - dib_mi_sandwich_batched: the three launches of the bounds (25 scales x 512 batches at batch sizes 64, 256, 1 024);
  - the notebook's NumPy formulation of ONE Monte-Carlo run on the host at a reduced size, labelled as such.
Rates: pairwise terms (sample x row pairs) per second and float64 FMAs per second (2 per pair and dimension: the count the
algorithm needs, not a hardware counter).  No share of peak is given: no float64 vector peak is on record for this device."""
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


def _timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def numpy_run(mus, n_samples, rng):
    """one Monte-Carlo run as the notebook states it (raw exp, norm distances, logvar 0), bits"""
    n_rows, E = mus.shape
    src = rng.choice(n_rows, size=n_samples)
    u = np.float32(rng.normal(loc=mus[src], scale=1.0))
    dists = np.linalg.norm(mus.reshape(-1, 1, E) - u.reshape(1, -1, E), ord=2, axis=-1)
    norm = (2.0 * np.pi) ** (E / 2.0)
    p_u = np.mean(np.exp(-dists ** 2 / 2.0) / norm, axis=0)
    p_ugx = np.exp(-np.linalg.norm(mus[src] - u, ord=2, axis=-1) ** 2 / 2.0) / norm
    return float(np.average(np.log2(p_ugx / p_u)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mi_bounds_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--variable", default="bits6")
    ap.add_argument("--numpy-samples", type=int, default=1000)
    args = ap.parse_args()
    import torch

    from dib_amd import mi_characterization as mic
    from dib_amd._lib import check, load_library
    if not torch.cuda.is_available():
        raise SystemExit("mi_bounds_bench.py needs a GPU")
    lib = load_library()
    var = next(v for v in mic.VARIABLES if v.name == args.variable)
    N, E, ns, runs, nb = 1024, 32, 10_000, 200, 512
    x = var.sample(np.random.default_rng(0), N)
    params = [mic.gaussian_channel(x, s, E) for s in var.separation_scales]
    tables, _ = mic._tables(np.stack([p[0] for p in params]), np.stack([p[1] for p in params]))
    S = tables.shape[0]
    dev = torch.device("cuda", 0)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)   # noqa: E731
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null = ctypes.c_void_p(0)
    tab_d = torch.from_numpy(tables).to(dev)
    rec = {"device": torch.cuda.get_device_name(0), "variable": var.name, "rows": N, "embedding_dimension": E, "separation_scales": S,
           "timing": "HIP events around the entry-point call (table prep + tiled kernel + combine), median of repeats after one warm-up"}

    # ---- Monte Carlo: one launch of the sweep ----
    G = min(mic.MAX_GROUPS_PER_LAUNCH, mic.MAX_INDICES_PER_LAUNCH // ns, S * runs)
    src = torch.from_numpy(np.stack([mic.monte_carlo_source_rows(0, g, N, ns) for g in range(G)])).to(dev)
    table_of = torch.from_numpy((np.arange(G) // runs).astype(np.int32)).to(dev)
    ws = torch.empty(int(lib.dib_mi_monte_carlo_workspace_bytes(S, N, E, G, ns)) // 8 + 2, dtype=torch.float64, device=dev)
    means = torch.empty(G, dtype=torch.float64, device=dev)
    t = _timed(lambda: check(lib.dib_mi_monte_carlo(p(tab_d), S, N, E, p(table_of), p(src), G, ns, 0, 0, p(means), null, null, p(ws),
                                                    st()), "dib_mi_monte_carlo"), args.repeats)
    pairs = G * ns * N
    t.update(groups=G, samples_per_group=ns, pairwise_terms=pairs, pairwise_terms_per_s=pairs / (t["median_ms"] * 1e-3),
             f64_fma_per_s=2 * E * pairs / (t["median_ms"] * 1e-3), launches_per_sweep=-(-S * runs // G),
             workspace_bytes=ws.numel() * 8)
    rec["monte_carlo_launch"] = t
    del ws, src

    # ---- the bounds: one launch per evaluation batch size ----
    rec["sandwich_launches"] = {}
    for bs in (64, 256, 1024):
        rows = np.random.default_rng(bs).integers(0, N, (S * nb, bs)) + np.repeat(np.arange(S) * N, nb)[:, None]
        idx = torch.from_numpy(rows.astype(np.int32)).to(dev)
        ws = torch.empty(int(lib.dib_mi_sandwich_batched_workspace_bytes(S * N, 1, E, S * nb, bs)) // 8 + 2, dtype=torch.float64, device=dev)
        out = torch.empty((2, S * nb), dtype=torch.float64, device=dev)
        t = _timed(lambda: check(lib.dib_mi_sandwich_batched(p(tab_d), S * N, 1, E, p(idx), S * nb, bs, 0.0, 0, 0, p(out[0]), p(out[1]),
                                                             null, null, null, p(ws), st()), "dib_mi_sandwich_batched"), args.repeats)
        pairs = S * nb * bs * bs
        t.update(batches=S * nb, batch_size=bs, pairwise_terms=pairs, pairwise_terms_per_s=pairs / (t["median_ms"] * 1e-3),
                 f64_fma_per_s=2 * E * pairs / (t["median_ms"] * 1e-3))
        rec["sandwich_launches"][str(bs)] = t
        del ws, idx

    # ---- the notebook's NumPy formulation on the host, REDUCED size: one run of --numpy-samples samples (not 200 x 10 000) ----
    mus = tables[S // 2, :, :E].astype(np.float64)
    rng = np.random.default_rng(1)
    numpy_run(mus, 64, rng)
    t0 = time.perf_counter()
    value = numpy_run(mus, args.numpy_samples, rng)
    sec = time.perf_counter() - t0
    pairs = args.numpy_samples * N
    rec["numpy_host_reduced_size"] = {"note": "host NumPy, ONE run at a reduced sample count; not the device path, not the notebook's size",
                                      "samples": args.numpy_samples, "rows": N, "seconds": sec, "pairwise_terms_per_s": pairs / sec,
                                      "host_cpus": len(os.sched_getaffinity(0)), "value_bits": value}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
