"""What the loss-family kernel (include/dib_losses.h, csrc/dib_losses.h) costs, on one box in one process:

    python tools/loss_bench.py --out profiles/loss_bench.json

  (a) dib_loss_ex_kernel alone (dib_loss_rows_ex on given buffers) at B = 65 536, out_dim C in {1, 10, 100, 1000}, for `mae`
      (element-wise, one pass over a row) and CategoricalCrossentropy(from_logits=True) (three passes: max and label sums, the
      exponential sum, the gradient), with no metric and with the kind's natural metric (one more pass).  HIP events around
      --batch back-to-back launches, divided by their number; median of --repeats.  Bytes = the compulsory traffic, pred and y
      read once and g_pred written once (12 B C per row; re-reads of a row are cache hits and not counted), next to the
      6.29 TB/s HBM figure measured on this part (MI355X_MICROARCH).  Up to C = 100 the three buffers (79 MB) stay in the 256 MB
      infinity cache between launches: only C = 1000 (786 MB) is an HBM rate.
  (b) the yardstick: dib_loss_kernel (one thread per row, lanes out_dim floats apart) on sparse_cce_logits through dib_loss_rows
      at the same shapes (it reads one label per row: 8 B C + 4 per row).
  (c) --pair: the reference-default train + validation pair (F = 10 Boolean circuit, B = 128, train.py defaults) under
      bce_logits: HipEngine.train_step + eval_step, host clock around --pairs pairs and a synchronize.  None of its kernels is
      touched by the loss family; `--pair-only --package-root DIR` times the pair with the package found under DIR (a checkout
      of another commit, its library through DIB_LIB_PATH) so that two commits can be interleaved on one box."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.29e12


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _events(fn, batch, repeats):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / batch)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "repeats": repeats, "batch": batch}


def _rate(rec, nbytes):
    rec["bytes"] = nbytes
    rec["gb_per_s"] = nbytes / (rec["median_us"] * 1e-6) / 1e9
    rec["fraction_of_hbm_6.29_tb_per_s"] = rec["gb_per_s"] * 1e9 / HBM_BYTES_PER_S
    return rec


def kernels(args):
    import torch

    from dib_amd import _lib, losses
    from dib_amd._lib import check
    lib = _lib.load_library()
    B = args.rows
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    out = {}
    for C in (1, 10, 100, 1000):
        gen = torch.Generator(device="cuda").manual_seed(C)
        pred = torch.randn((B, C), device="cuda", generator=gen)
        y = torch.softmax(torch.randn((B, C), device="cuda", generator=gen), 1)
        lab = torch.randint(0, C, (B, 1), device="cuda", generator=gen).float()
        g = torch.empty((B, C), device="cuda")
        part = torch.empty(2 * ((B + 255) // 256), device="cuda")
        out3 = torch.empty(3, device="cuda")
        batch = max(3, args.batch // max(1, C // 10))
        rec = {"rows": B, "out_dim": C, "lanes": int(lib.dib_loss_ex_lanes(C)), "buffers_bytes": 12 * B * C}
        for kind, metric in (("mae", None), ("mae", "mse"), ("cce_logits", None), ("cce_logits", "categorical_accuracy")):
            d = _lib.LossDesc(losses.KIND_IDS[kind], losses.METRIC_IDS[metric], 0.0)
            fn = lambda: check(lib.dib_loss_rows_ex(ctypes.byref(d), _p(pred), C, _p(y), C, None, 0, B, 1.0 / B, 0, _p(g), _p(part),   # noqa: E731
                                                    st()), "dib_loss_rows_ex")
            rec[f"dib_loss_ex_kernel {kind} metric={metric}"] = _rate(_events(fn, batch, args.repeats), 12 * B * C)
        fn = lambda: check(lib.dib_loss_rows(_lib.LOSS_KINDS["sparse_cce_logits"], _p(pred), C, _p(lab), 1, B, 1.0 / B, _p(g), _p(out3),   # noqa: E731
                                             _p(part), st()), "dib_loss_rows")
        rec["dib_loss_kernel sparse_cce_logits (+ its 2-workgroup finalize)"] = _rate(_events(fn, batch, args.repeats), 8 * B * C + 4 * B)
        out[f"C={C}"] = rec
    return out


def pair(args):
    import torch

    from dib_amd.engine import HipEngine
    F, B = 10, 128
    eng = HipEngine([1] * F, [128, 128], [256, 256], 1, feature_embedding_dimension=32, init_seed=1)
    rng = np.random.default_rng(F)
    x = eng.to_device(rng.integers(0, 2, size=(B, F)).astype(np.float32) * 2 - 1)
    y = eng.to_device((rng.random((B, 1)) > 0.5).astype(np.float32))
    eng.set_lr(3e-4)

    def one(k):
        eng.train_step(x, y, None, 0, B, 1, k, "bce_logits", optimizer=("adam", 0.9, 0.999, 1e-7))
        eng.eval_step(x, y, None, 0, B, 1, (1 << 31) + k, "bce_logits", metrics_acc=eng.metrics_acc_val)

    for k in range(20):
        one(k)
    torch.cuda.synchronize()
    n0 = eng.lib.dib_launch_count()
    one(0)
    launches = int(eng.lib.dib_launch_count() - n0)
    torch.cuda.synchronize()
    us = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for k in range(args.pairs):
            one(k)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / args.pairs)
    return {"features": F, "batch": B, "loss": "bce_logits", "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us),
            "repeats": args.repeats, "pairs_per_repeat": args.pairs, "launches": launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back launches per event pair in (a), (b) at C <= 10; fewer for wider C")
    ap.add_argument("--pairs", type=int, default=200, help="train + validation pairs per timed repeat in (c)")
    ap.add_argument("--pair", action="store_true", help="also time (c)")
    ap.add_argument("--pair-only", action="store_true", help="time (c) alone and print it")
    ap.add_argument("--package-root", default=ROOT, help="directory holding dib_amd.py and the package to time in (c)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench.py needs a GPU")
    if args.repeats < 5:
        raise SystemExit("--repeats: at least 5 (the figures are medians)")
    if args.pair_only:
        print(json.dumps(pair(args)))
        return
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events around `batch` back-to-back launches / batch; medians of `repeats` after warm-up",
           "kernels_at_65536_rows": kernels(args)}
    if args.pair:
        rec["reference_default_train_validation_pair_f10_b128"] = pair(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
