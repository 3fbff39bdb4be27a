"""What gradient clipping and a learning-rate schedule (include/dib_grad_transform.h) cost, on one box in one process:

    python tools/grad_transform_bench.py --out profiles/grad_transform_bench.json

  (a) the transform launches alone on BASELINE config 3's flat buffer (F = 64: 390 variables of 1 to 524 288 elements in
      2 224 897 floats), per mode: dib_grad_sumsq (tile sums + segment sums), dib_grad_clip_apply, both, and the one-thread
      dib_lr_schedule_eval - next to their HBM floor at the 6.29 TB/s the microarchitecture guide measured (8.9 MB read for the
      sums; 8.9 MB read + 8.9 MB written for the apply) and next to dib_adam_step on the same buffer.  HIP events around --batch
      back-to-back calls, divided by their number; median of --repeats.  The buffer stays in the 256 MB infinity cache between
      calls: the rates are those of the cache, not of HBM.
  (b) the reference-default train + validation pair (F = 10 Boolean circuit, B = 128, train.py defaults) under Adam, Adam +
      clipnorm, Adam + global_clipnorm and Adam + ExponentialDecay: HipEngine.train_step + eval_step, host clock around --pairs
      pairs and a synchronize; the library's launches per pair.  A clipped step leaves the one-launch tail (tail without the
      update, 3 transform launches, dib_adam_step's 2); a schedule adds its one launch and keeps the tail.
  (c) the BASELINE config-3 step (F = 64, B = 65 536) under the same four.
Adam is measured first, between the variants and last: drift of the box shows as the spread of the Adam entries."""
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


def kernels(args):
    import torch

    from dib_amd import optimizers as O, schedules as S
    from dib_amd.engine import HipEngine
    eng = HipEngine([1] * 64, [128, 128], [256, 256], 1, feature_embedding_dimension=32, init_seed=1)
    gt = eng.grad_transform()
    n = eng.n_params
    rng = np.random.default_rng(0)
    src = torch.from_numpy((rng.standard_normal(eng.grads.numel()) * 1e-2).astype(np.float32)).to(eng.device)
    eng.grads.copy_(src)
    eng.set_lr(1e-6)
    live = sum(gt.host.counts)
    out = {"parameters": n, "variables": gt.n_segments, "tiles": gt.host.n_tiles, "largest_variable": max(gt.host.counts),
           "floor_us_read": live * 4 / HBM_BYTES_PER_S * 1e6, "floor_us_read_write": 2 * live * 4 / HBM_BYTES_PER_S * 1e6}
    out["adam (dib_adam_step)"] = _events(lambda: eng.adam_step(), args.batch, args.repeats)
    # thresholds far above the norms: the apply rewrites the buffer with what it read (times 1), so every call sees the same data
    for name, opt in (("clipvalue", O.build(O.Adam, clipvalue=1e30)), ("clipnorm", O.build(O.Adam, clipnorm=1e30)),
                      ("global_clipnorm", O.build(O.Adam, global_clipnorm=1e30)),
                      ("clipvalue_clipnorm", O.build(O.Adam, clipvalue=1e30, clipnorm=1e30))):
        clip = opt.clip()
        rec = {"launches": 1 if clip[1] == 0 else 3}
        if clip[1] != 0:
            rec["sumsq"] = _events(lambda: gt.sumsq(clip), args.batch, args.repeats)
            rec["sumsq"]["over_floor"] = rec["sumsq"]["median_us"] / out["floor_us_read"]
        rec["apply"] = _events(lambda: gt.apply(clip), args.batch, args.repeats)
        rec["apply"]["over_floor"] = rec["apply"]["median_us"] / out["floor_us_read_write"]
        rec["transform"] = _events(lambda: gt.transform(clip), args.batch, args.repeats)
        rec["transform_over_adam"] = rec["transform"]["median_us"] / out["adam (dib_adam_step)"]["median_us"]
        out[name] = rec
    sched = O.Adam(S.ExponentialDecay(3e-4, 1000, 0.9))
    out["lr_schedule_eval"] = _events(lambda: eng.apply_lr(sched), args.batch, args.repeats)
    out["adam_again (dib_adam_step)"] = _events(lambda: eng.adam_step(), args.batch, args.repeats)
    del eng
    torch.cuda.empty_cache()
    return out


def _steps(eng, x, y, B, opt, with_validation, pairs, repeats):
    import torch

    def pair(k):
        eng.apply_lr(opt)   # what fit does ahead of every step: nothing for an unchanged constant, one launch for a schedule
        eng.train_step(x, y, None, 0, B, 1, k, "bce_logits", optimizer=opt)
        if with_validation:
            eng.eval_step(x, y, None, 0, B, 1, (1 << 31) + k, "bce_logits", metrics_acc=eng.metrics_acc_val)

    for k in range(5):
        pair(k)
    torch.cuda.synchronize()
    n0 = eng.lib.dib_launch_count()
    pair(0)
    launches = int(eng.lib.dib_launch_count() - n0)
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for k in range(pairs):
            pair(k)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6 / pairs)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "repeats": repeats, "steps_per_repeat": pairs,
            "launches": launches}


def model_steps(args, F, B, with_validation, pairs):
    import torch

    from dib_amd import optimizers as O, schedules as S
    from dib_amd.engine import HipEngine
    eng = HipEngine([1] * F, [128, 128], [256, 256], 1, feature_embedding_dimension=32, init_seed=1)
    eng.grad_transform()
    rng = np.random.default_rng(F)
    x = eng.to_device(rng.integers(0, 2, size=(B, F)).astype(np.float32) * 2 - 1)
    y = eng.to_device((rng.random((B, 1)) > 0.5).astype(np.float32))
    rec = {"features": F, "batch": B, "parameters": eng.n_params}
    variants = [("adam", O.Adam(3e-4)), ("adam_clipnorm", O.build(O.Adam, 3e-4, clipnorm=1.0)), ("adam_between", O.Adam(3e-4)),
                ("adam_global_clipnorm", O.build(O.Adam, 3e-4, global_clipnorm=1.0)),
                ("adam_exponential_decay", O.Adam(S.ExponentialDecay(3e-4, 1000, 0.9))), ("adam_again", O.Adam(3e-4))]
    for name, opt in variants:
        rec[name] = _steps(eng, x, y, B, opt, with_validation, pairs, args.repeats)
    plain = [rec[k]["median_us"] for k in ("adam", "adam_between", "adam_again")]
    rec["adam_spread_us"] = max(plain) - min(plain)
    for k in ("adam_clipnorm", "adam_global_clipnorm", "adam_exponential_decay"):
        rec[k]["extra_us"] = rec[k]["median_us"] - statistics.median(plain)
        rec[k]["extra_launches"] = rec[k]["launches"] - rec["adam"]["launches"]
    del eng
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_transform_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back calls per event pair in (a)")
    ap.add_argument("--pairs", type=int, default=200, help="train + validation pairs per timed repeat in (b)")
    ap.add_argument("--steps", type=int, default=10, help="config-3 steps per timed repeat in (c)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grad_transform_bench.py needs a GPU")
    if args.repeats < 5:
        raise SystemExit("--repeats: at least 5 (the figures are medians)")
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "kernels: HIP events around `batch` back-to-back calls / batch; steps: host clock around the steps and a "
                     "synchronize / steps; medians of `repeats` after warm-up; the Adam entries are interleaved with the variants",
           "hbm_bytes_per_s_of_the_floor": HBM_BYTES_PER_S,
           "kernels_at_config3": kernels(args),
           "reference_default_train_validation_pair_f10_b128": model_steps(args, 10, 128, True, args.pairs),
           "config3_step_f64_b65536": model_steps(args, 64, 65536, False, args.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
