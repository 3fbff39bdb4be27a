"""One save of every feature's compression matrix by SaveCompressionMatricesCallback (save_png=False), both ways, on one box in
one process:

    python tools/compression_matrices_bench.py --out profiles/compression_matrices_bench.json

for the BASELINE config-3 architecture (F = 64, E = 32, encoders [128, 128], 128 display rows per feature) and the reference's
default run (the F = 10 Boolean circuit: 2 display rows per feature):
  (a) one_launch=True: the display rows of all features, one dib_compression_gather, one deterministic encoder-bank forward, one
      dib_compression_matrices and one read-back (include/dib_compression.h; the validation matrix is uploaded once);
  (b) the loop it replaces (one_launch=False): visualization.save_compression_matrices feature by feature - per feature a host
      gather and upload, dib_encode_deterministic and a read-back, four uploads, dib_bhattacharyya and a read-back.
Wall time of a whole save, the device idle before and after (host clock around the call and a synchronize), median of --repeats
after one warm-up save; the library's launch counts (dib_launch_count) of one save; and the matrices kernel alone (HIP events
around dib_compression_matrices on the encodings of the display rows) next to the F dib_bhattacharyya launches it replaces."""
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


def bench(name, model, x, x_raw, args):
    import torch

    import dib_amd
    from dib_amd import visualization
    from dib_amd._lib import check
    eng = model._ensure_engine()
    lib, F, E = eng.lib, model.number_features, model.feature_embedding_dimension
    rec = {"features": F, "embedding_dimension": E, "encoder": model.feature_encoder_architecture, "validation_rows": int(x.shape[0])}
    saves = {}
    for mode in (True, False):
        cb = dib_amd.SaveCompressionMatricesCallback(1, x, x_raw, os.path.join(args.scratch, name), save_png=False, one_launch=mode)
        cb.set_model(model)
        np.random.seed(0)
        t = _wall(lambda: cb.on_epoch_end(0), args.repeats)
        n0 = lib.dib_launch_count()
        cb.on_epoch_end(0)
        t["launches"] = int(lib.dib_launch_count() - n0)
        saves[mode] = (t, cb)
    rec["one_launch"], rec["per_feature_loop"] = saves[True][0], saves[False][0]
    rec["per_feature_loop"]["read_backs"] = 2 * F
    rec["one_launch"]["read_backs"] = 1
    rec["display_rows"] = int(saves[True][1].matrices[(0, 0)].shape[0])
    rec["loop_over_one_launch"] = rec["per_feature_loop"]["median_ms"] / rec["one_launch"]["median_ms"]
    # the two paths on the SAME rows (the two encode with different float32 kernels: agreement to ~1e-6, not to the bit)
    sel = visualization.display_rows(x_raw, model.feature_dimensionalities, rng=np.random.RandomState(1))
    xd = eng.to_device(x)
    comp, enc = eng.compression_matrices(xd, sel["rows"], sel["n_rows"], want_encodings=True)
    cuts = np.cumsum(model.feature_dimensionalities)[:-1]
    split, raw_split = np.split(x, cuts, axis=-1), np.split(x_raw, cuts, axis=-1)
    rng = np.random.RandomState(1)
    loop = [visualization.save_compression_matrices(model.feature_encoders[f], split[f], None, inp_features_raw=raw_split[f],
                                                    model=model, rng=rng) for f in range(F)]
    rec["max_abs_difference"] = float(max(np.abs(comp[f, :n, :n] - loop[f]).max() for f, n in enumerate(sel["n_rows"])))

    # the kernels alone, on the encodings of the display rows
    n_max = int(sel["rows"].shape[1])
    enc_d = torch.from_numpy(enc).to(eng.device)
    cnt_d = torch.from_numpy(sel["n_rows"]).to(eng.device)
    out = torch.empty((F, n_max, n_max), dtype=torch.float32, device=eng.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    t = _events(lambda: check(lib.dib_compression_matrices(p(enc_d), n_max, 0, F, E, p(cnt_d), n_max, None, p(out), eng._stream()),
                              "dib_compression_matrices"), args.repeats)
    pairs = int((sel["n_rows"].astype(np.int64) ** 2).sum())
    t.update(pair_dimension_terms=pairs * E, terms_per_s=pairs * E / (t["median_ms"] * 1e-3))
    rec["dib_compression_matrices_alone"] = t
    mus = [enc_d[f, :n, :E].contiguous() for f, n in enumerate(sel["n_rows"])]
    lvs = [enc_d[f, :n, E:].contiguous() for f, n in enumerate(sel["n_rows"])]
    outs = [torch.empty((int(n), int(n)), dtype=torch.float32, device=eng.device) for n in sel["n_rows"]]

    def bhattacharyya_loop():
        for mu, lv, o in zip(mus, lvs, outs):
            check(lib.dib_bhattacharyya(p(mu), p(lv), mu.shape[0], p(mu), p(lv), mu.shape[0], E, p(o), eng._stream()), "dib_bhattacharyya")

    rec["dib_bhattacharyya_per_feature_alone"] = _events(bhattacharyya_loop, args.repeats)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compression_matrices_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=16384, help="rows of the F = 64 validation set the display rows are drawn from")
    ap.add_argument("--scratch", default=None, help="directory for the callbacks' output directory and the dataset cache "
                                                    "(default: a temporary directory, removed at the end)")
    args = ap.parse_args()
    if args.scratch is None:
        import tempfile
        with tempfile.TemporaryDirectory(prefix="compression_matrices_bench") as tmp:
            args.scratch = tmp
            return run(args)
    return run(args)


def run(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compression_matrices_bench.py needs a GPU")
    if args.repeats < 5:
        raise SystemExit("--repeats: at least 5 (the figures are medians)")
    import dib_amd
    from dib_amd import data
    configs = {}
    F = 64
    model = dib_amd.DistributedIBNet([1] * F, [128, 128], [256, 256], 1, feature_embedding_dimension=32, init_seed=1)
    x = np.random.default_rng(F).standard_normal((args.rows, F)).astype(np.float32)
    configs["config3_f64_128_rows"] = bench("f64", model, x, x, args)
    d = data.DATASETS["boolean_circuit"](data_path=os.path.join(args.scratch, "data"), boolean_random_circuit=False,
                                         boolean_number_input_gates=10, seed=0)
    model = dib_amd.DistributedIBNet(d["feature_dimensionalities"], [128, 128], [256, 256], d["output_dimensionality"],
                                     feature_embedding_dimension=32, init_seed=1)
    xv = np.asarray(d["x_valid"], dtype=np.float32)
    configs["reference_default_boolean_circuit_f10"] = bench("boolean", model, xv, np.asarray(d.get("x_valid_raw", xv)), args)
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "whole saves (SaveCompressionMatricesCallback.on_epoch_end, save_png=False): host clock around the call + "
                     "synchronize, device idle before; the kernel entries: HIP events; median of repeats after one warm-up",
           "configs": configs}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
