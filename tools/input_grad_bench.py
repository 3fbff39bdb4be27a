"""What dL/dx costs: the training step with and without HipEngine.input_grad, same process, alternating A/B.

  python tools/input_grad_bench.py [out.json]        (default: the record, profiles/input_grad_bench.json)

Sizes: BASELINE config 3 (64 features, B = 65 536), its 8-GPU strong-scaling share (B = 8 192), the reference's default
(10 features, B = 128); config 3 once more with h1 stashed ("wgrad_recompute_h1" 0).  Method: HIP events around STEPS back-to-back steps (train_step with the optimizer in the tail launch
[+ input_grad]), A then B, five times after a warm-up of both; the figure is the median of the five per-step times.

A timing loop, not a usage example: train_step applies the optimizer in its tail launch, so the input_grad that follows reads
parameters the forward did not see (include/dib_hip.h asks for the parameters it saw).  That costs the same time; a caller who
wants the gradient of the step's loss calls input_grad before the parameters change, as the autograd bridge does."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = [("config3_f64_b65536", 64, 65536, 30, {}), ("config3_f64_b8192", 64, 8192, 200, {}),
         ("reference_default_f10_b128", 10, 128, 1000, {}),
         # the same step with h1 stashed by the forward: what dib_workspace_h1_materialize costs the input gradient at config 3
         ("config3_f64_b65536_h1_stashed", 64, 65536, 30, {"wgrad_recompute_h1": 0})]
REPS = 5


def measure(name, F, B, steps, tuning):
    from dib_amd import _lib
    old = {k: _lib.get_tuning(k) for k in tuning}
    for k, v in tuning.items():
        _lib.set_tuning(k, v)
    try:
        return _measure(name, F, B, steps, tuning)
    finally:
        for k, v in old.items():
            _lib.set_tuning(k, v)


def _measure(name, F, B, steps, tuning):
    from dib_amd.engine import HipEngine
    eng = HipEngine([1] * F, [128, 128], [256, 256], 1, init_seed=0)
    eng.set_beta(0.1)
    eng.set_lr(3e-4)
    rng = np.random.default_rng(0)
    x = eng.to_device(rng.standard_normal((B, F)).astype(np.float32))
    y = eng.to_device(rng.integers(0, 2, (B, 1)).astype(np.float32))
    opt = ("adam", 0.9, 0.999, 1e-7)
    lib = eng.lib

    def run(with_dx, n):
        for i in range(n):
            eng.train_step(x, y, None, 0, B, 0, i, "bce_logits", optimizer=opt)
            if with_dx:
                eng.input_grad(x, None, 0, B)

    n0 = lib.dib_launch_count()
    run(False, 1)
    n1 = lib.dib_launch_count()
    run(True, 1)
    n2 = lib.dib_launch_count()
    run(False, 3)
    run(True, 3)
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(REPS):
        for with_dx in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(with_dx, steps)
            b.record()
            b.synchronize()
            times[with_dx].append(a.elapsed_time(b) / steps)
    base, dx = float(np.median(times[False])), float(np.median(times[True]))
    out = dict(name=name, features=F, batch=B, tuning=tuning, steps_per_block=steps, blocks=REPS, step_ms=base, step_with_input_grad_ms=dx,
               input_grad_ms=dx - base, overhead_percent=100.0 * (dx - base) / base, launches_step=int(n1 - n0),
               launches_step_with_input_grad=int(n2 - n1), h1_stashed=int(lib.dib_workspace_h1_stashed(eng.layout, ctypes.c_void_p(eng.workspace(B).data_ptr()))),
               blocks_ms=dict(step=[round(t, 4) for t in times[False]], with_input_grad=[round(t, 4) for t in times[True]]))
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "input_grad_bench.json")
    assert torch.cuda.is_available(), "needs a GPU"
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events, median of 5 alternating blocks after warm-up",
               sizes=[measure(*s) for s in SIZES])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
