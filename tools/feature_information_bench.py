"""One evaluation of every feature's information bounds (8 batches of 1 024 rows) on a DistributedIBNet, both ways, on one box
in one process:

    python tools/feature_information_bench.py --out profiles/feature_information_bench.json

for the BASELINE config-3 architecture (F = 64, E = 32, encoders [128, 128]) and the reference's default F = 10:
  (a) DistributedIBNet.information_per_feature: one encoder-bank forward + one dib_mi_features_bounds per chunk of batches, one
      read-back (include/dib_mi_features.h);
  (b) the loop it replaces: utils.estimate_mi_sandwich_bounds feature by feature, as InfoPerFeatureCallback's default path runs
      it - per (feature, batch) a host gather and upload, dib_encode_deterministic, dib_mi_sandwich_rows and a read-back.
Wall time of a whole evaluation, the device idle before and after (host clock around the call and a synchronize; the loop ends
in a read-back anyway), median of --repeats after one warm-up evaluation; the library's launch counts (dib_launch_count) of one
evaluation; the chunk size of (a) swept (HipEngine.FEATURE_INFORMATION_ROWS) with the scratch it costs; and the tiled kernel's
own time (HIP events around dib_mi_features_bounds on the model's encodings of all 8 batches) with its float64 FMA rate: 2 per
(sample, row, dimension), the count the algorithm needs, against the device's float64 vector peak (256 CUs x 64 lanes x 2.4 GHz
FMAs per second, the 78.6 TFLOP/s of AMD's specification sheet)."""
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

F64_VECTOR_PEAK_FMA_PER_S = 256 * 64 * 2.4e9   # = 78.6 TFLOP/s / 2


def _wall(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats": repeats}


def _events(fn, repeats):
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


def bench(F, args):
    import torch

    import dib_amd
    from dib_amd import utils
    from dib_amd._lib import check
    E, bs, nb = 32, args.batch_size, args.batches
    model = dib_amd.DistributedIBNet([1] * F, [128, 128], [256, 256], 1, feature_embedding_dimension=E, init_seed=1)
    eng = model._ensure_engine()
    lib = eng.lib
    x = np.random.default_rng(F).standard_normal((args.rows, F)).astype(np.float32)
    xd = eng.to_device(x)
    rec = {"features": F, "embedding_dimension": E, "encoder": [128, 128], "validation_rows": args.rows,
           "evaluation_batch_size": bs, "number_evaluation_batches": nb}

    def one_launch():
        return model.information_per_feature(xd, bs, nb, seed=3)

    def loop():
        return np.stack([utils.estimate_mi_sandwich_bounds(model.feature_encoders[f], x[:, f], bs, nb, seed=3) for f in range(F)])

    sweep = {}
    for rows_per_encode in args.chunk_rows:
        eng.FEATURE_INFORMATION_ROWS = rows_per_encode
        eng._eval_ws.clear()
        t = _wall(one_launch, args.repeats)
        k = max(1, min(nb, rows_per_encode // bs))
        t["scratch_bytes"] = int(lib.dib_workspace_bytes(eng.layout, k * bs)) + int(lib.dib_mi_features_workspace_bytes(F, E, bs, k))
        sweep[str(rows_per_encode)] = t
    rec["information_per_feature_by_rows_per_encode"] = sweep
    eng.FEATURE_INFORMATION_ROWS = type(eng).FEATURE_INFORMATION_ROWS
    eng._eval_ws.clear()
    rec["rows_per_encode"] = eng.FEATURE_INFORMATION_ROWS
    rec["information_per_feature"] = _wall(one_launch, args.repeats)
    n0 = lib.dib_launch_count()
    a = one_launch()
    rec["information_per_feature"]["launches"] = int(lib.dib_launch_count() - n0)
    rec["per_feature_loop"] = _wall(loop, args.repeats)
    n0 = lib.dib_launch_count()
    b = loop()
    rec["per_feature_loop"]["launches"] = int(lib.dib_launch_count() - n0)
    rec["per_feature_loop"]["host_syncs"] = F * nb
    rec["speedup"] = rec["per_feature_loop"]["median_ms"] / rec["information_per_feature"]["median_ms"]
    # (the two encode with different float32 kernels: the bounds agree to ~1e-4 nats, not to the bit)
    rec["max_abs_difference_nats"] = float(np.abs(a - b)[np.isfinite(a) & np.isfinite(b)].max())

    # the bound kernels alone, on the encodings of all nb batches
    rows = utils.evaluation_batch_rows(args.rows, bs, nb, 3).astype(np.int32)
    enc = eng.feature_information(xd, rows, bs, nb, 3, want_encodings=True)[1]
    enc_d = torch.from_numpy(enc).to(eng.device)
    ws = torch.empty(int(lib.dib_mi_features_workspace_bytes(F, E, bs, nb)) // 8 + 2, dtype=torch.float64, device=eng.device)
    out = torch.empty((F, nb, 2), dtype=torch.float64, device=eng.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    null = ctypes.c_void_p(0)
    t = _events(lambda: check(lib.dib_mi_features_bounds(p(enc_d), nb * bs, 0, F, E, bs, nb, 3, 0, 0, p(out), null, null, null, p(ws),
                                                         eng._stream()), "dib_mi_features_bounds"), args.repeats)
    pairs = F * nb * bs * bs
    rate = 2 * E * pairs / (t["median_ms"] * 1e-3)
    t.update(groups=F * nb, pairwise_terms=pairs, f64_fma=2 * E * pairs, f64_fma_per_s=rate,
             fraction_of_f64_vector_peak=rate / F64_VECTOR_PEAK_FMA_PER_S, workspace_bytes=ws.numel() * 8)
    rec["dib_mi_features_bounds_all_batches"] = t
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_information_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--features", type=int, nargs="+", default=[64, 10])
    ap.add_argument("--rows", type=int, default=16384, help="rows of the validation set the batches are drawn from")
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--chunk-rows", type=int, nargs="+", default=[1024, 2048, 4096, 8192])
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feature_information_bench.py needs a GPU")
    if args.repeats < 5:
        raise SystemExit("--repeats: at least 5 (the figures are medians)")
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "whole evaluations: host clock around the call + synchronize, device idle before; the kernel entry: HIP events; "
                     "median of repeats after one warm-up",
           "f64_vector_peak_fma_per_s": F64_VECTOR_PEAK_FMA_PER_S,
           "configs": {str(F): bench(F, args) for F in args.features}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
