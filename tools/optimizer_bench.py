"""What the Keras optimizer family (include/dib_optimizers.h) costs next to Adam, on one box in one process:

    python tools/optimizer_bench.py --out profiles/optimizer_bench.json

  (a) per rule, at BASELINE config 3's 2 224 897 parameters: one update of the whole flat buffer - dib_optimizer_step alone and
      dib_optimizer_step + dib_optimizer_advance - next to dib_adam_step (dib_adam_kernel + its counter bump) on the same
      buffers.  HIP events around --batch back-to-back updates, divided by their number; median of --repeats.  Bytes moved per
      element: parameter read + write, gradient read, every state slot read + write.  The buffers (8.9 MB each, at most 44 MB
      per rule) stay in the 256 MB infinity cache between updates: the rates are those of the cache, not of HBM.
  (b) the reference-default train + validation pair (F = 10 Boolean circuit, B = 128, train.py defaults) under rmsprop against
      adam: HipEngine.train_step + eval_step, host clock around --pairs pairs and a synchronize; the library's launches per pair.
      The difference is the price of the rule's two extra launches (its update cannot ride in the step tail).
  (c) the BASELINE config-3 step (F = 64, B = 65 536) under nadam against adam, the same way."""
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

N_CONFIG3 = 2224897


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

    from dib_amd import _lib, optimizers as O
    from dib_amd._lib import check
    lib = _lib.load_library()
    n = N_CONFIG3
    dev = "cuda"
    rng = np.random.default_rng(0)
    w = torch.from_numpy(rng.standard_normal(n + 3).astype(np.float32)).to(dev)
    g = torch.from_numpy((rng.standard_normal(n + 3) * 1e-2).astype(np.float32)).to(dev)
    s = [torch.zeros(n + 3, dtype=torch.float32, device=dev) for _ in range(3)]
    lr = torch.full((1,), 1e-6, dtype=torch.float32, device=dev)
    t = torch.zeros(1, dtype=torch.int64, device=dev)
    P = torch.ones(1, dtype=torch.float64, device=dev)
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    out = {}
    adam = _events(lambda: check(lib.dib_adam_step(_p(w), _p(g), _p(s[0]), _p(s[1]), n, _p(lr), _p(t), 0.9, 0.999, 1e-7, 1.0, st()),
                                 "dib_adam_step"), args.batch, args.repeats)
    adam.update(slots=2, bytes=n * 4 * (3 + 2 * 2), launches=2)
    adam["bytes_per_s"] = adam["bytes"] / (adam["median_us"] * 1e-6)
    out["adam (dib_adam_step: dib_adam_kernel + counter bump)"] = adam
    rules = {"sgd_momentum": O.SGD(momentum=0.9), "sgd_nesterov": O.SGD(momentum=0.9, nesterov=True), "rmsprop": O.RMSprop(),
             "rmsprop_centered": O.RMSprop(centered=True), "rmsprop_momentum": O.RMSprop(momentum=0.9),
             "rmsprop_centered_momentum": O.RMSprop(centered=True, momentum=0.9), "adagrad": O.Adagrad(), "adadelta": O.Adadelta(),
             "adamax": O.Adamax(), "nadam": O.Nadam(), "amsgrad": O.Adam(amsgrad=True)}
    for name, opt in rules.items():
        h = _lib.OptimizerHyper(**opt.hyper())
        k = opt.slots()
        sl = [_p(s[i]) if i < k else None for i in range(3)]
        sc = _p(P) if opt.name == "nadam" else None
        t.zero_()
        check(lib.dib_optimizer_init(opt.kind, ctypes.byref(h), *sl, n, sc, st()), "dib_optimizer_init")
        step = lambda: check(lib.dib_optimizer_step(opt.kind, ctypes.byref(h), _p(w), _p(g), *sl, n, _p(lr), _p(t), sc, 1.0, st()),   # noqa: E731
                             "dib_optimizer_step")

        def both():
            step()
            check(lib.dib_optimizer_advance(opt.kind, ctypes.byref(h), _p(t), sc, st()), "dib_optimizer_advance")

        rec = {"slots": k, "bytes": n * 4 * (3 + 2 * k), "step_alone": _events(step, args.batch, args.repeats),
               "step_and_advance": _events(both, args.batch, args.repeats)}
        rec["bytes_per_s_step_alone"] = rec["bytes"] / (rec["step_alone"]["median_us"] * 1e-6)
        rec["time_over_adam"] = rec["step_and_advance"]["median_us"] / adam["median_us"]
        rec["bytes_over_adam"] = rec["bytes"] / adam["bytes"]
        out[name] = rec
    return out


def _steps(eng, x, y, B, optimizer, with_validation, pairs, repeats):
    import torch

    def pair(k):
        eng.train_step(x, y, None, 0, B, 1, k, "bce_logits", optimizer=optimizer)
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


def model_steps(args, F, B, enc, integ, rule_name, with_validation, pairs):
    import torch

    from dib_amd import optimizers as O
    from dib_amd.engine import HipEngine
    eng = HipEngine([1] * F, enc, integ, 1, feature_embedding_dimension=32, init_seed=1)
    rng = np.random.default_rng(F)
    x = eng.to_device(rng.integers(0, 2, size=(B, F)).astype(np.float32) * 2 - 1)
    y = eng.to_device((rng.random((B, 1)) > 0.5).astype(np.float32))
    eng.set_lr(3e-4)
    rec = {"features": F, "batch": B, "parameters": eng.n_params}
    # interleaved A / B / A: drift of the box shows as a difference between the two Adam entries
    opt = O.get(rule_name)
    rec["adam"] = _steps(eng, x, y, B, O.Adam(), with_validation, pairs, args.repeats)
    eng.set_optimizer(opt)
    rec[rule_name] = _steps(eng, x, y, B, opt, with_validation, pairs, args.repeats)
    eng.set_optimizer(O.Adam())
    rec["adam_again"] = _steps(eng, x, y, B, O.Adam(), with_validation, pairs, args.repeats)
    rec["extra_us"] = rec[rule_name]["median_us"] - 0.5 * (rec["adam"]["median_us"] + rec["adam_again"]["median_us"])
    rec["extra_launches"] = rec[rule_name]["launches"] - rec["adam"]["launches"]
    del eng
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50, help="back-to-back updates per event pair in (a)")
    ap.add_argument("--pairs", type=int, default=200, help="train + validation pairs per timed repeat in (b)")
    ap.add_argument("--steps", type=int, default=10, help="config-3 steps per timed repeat in (c)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench.py needs a GPU")
    if args.repeats < 5:
        raise SystemExit("--repeats: at least 5 (the figures are medians)")
    rec = {"device": torch.cuda.get_device_name(0),
           "timing": "kernels: HIP events around `batch` back-to-back updates / batch; steps: host clock around the steps and a "
                     "synchronize / steps; medians of `repeats` after warm-up; adam / rule / adam_again are interleaved on one box",
           "kernels_at_2224897_parameters": kernels(args),
           "reference_default_train_validation_pair_f10_b128": model_steps(args, 10, 128, [128, 128], [256, 256], "rmsprop", True, args.pairs),
           "config3_step_f64_b65536": model_steps(args, 64, 65536, [128, 128], [256, 256], "nadam", False, args.steps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
