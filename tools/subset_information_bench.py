"""Times the exhaustive subset informations (dib_amd.subset_information, include/dib_subsets.h) on full truth tables of random
circuits (data.random_circuit, K = 2) and writes profiles/subset_information_bench.json:
  - per B in 10, 14, 16, 18, 20: the kernel (device events around dib_subset_information, median of the repeats after a warm-up),
    host to host (subset_information(x, y): counting the table, upload, launch, download), the work the algorithm needs - reads
    2^(2B - L) K, additions (3^L - 2^L) 3^(B - L) K, float64 logarithms 3^B (K + 1) - and the achieved rates;
  - where the time goes: the workgroup of H = all high bits alone (a chunk of the top 2^L subsets: every other workgroup leaves
    at once) against the whole launch, and the fold width swept through dib_set_tuning("subset_low_bits") at B = 14 and 16;
  - the float64 NumPy host backend at 10, 14 and 16 bits, the largest |device - host| there, and the parent's only means at 10
    gates: the loop of oracle.dib_oracle.shapley_values_bits.
    python tools/subset_information_bench.py [--out profiles/subset_information_bench.json] [--bits 10 14 16 18 20]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def table_of(B):
    import dib_amd
    t = dib_amd.data.truth_table(dib_amd.data.random_circuit(B, np.random.default_rng(B)), B)
    return t[:, :B], t[:, -1]


def low_bits(B, K, forced=0):
    """csrc/host/subsets.h subset_low_bits"""
    most = 0
    while most < 8 and most < B and 3 ** (most + 1) * ((K + 1) // 2 * 2) * 4 + 640 <= 65536:
        most += 1
    return min(forced, most) if forced > 0 else most


def work(B, K, L):
    return {"low_bits": L, "workgroups": 1 << (B - L), "reads": 2 ** (2 * B - L) * K,
            "adds": (3 ** L - 2 ** L) * 3 ** (B - L) * K, "log2_f64": 3 ** B * (K + 1)}


def kernel_ms(lib, counts, B, K, out, mask0, n_masks, reps):
    import torch
    widths = (ctypes.c_int * B)(*([1] * B))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: lib.dib_subset_information(ctypes.c_void_p(counts.data_ptr()), B, K, widths, B, mask0, n_masks,
                                              ctypes.c_void_p(out.data_ptr()), None, st)
    assert call() == 0   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert call() == 0
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(t, 4) for t in times]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_information_bench.json"))
    ap.add_argument("--bits", type=int, nargs="+", default=[10, 14, 16, 18, 20])
    ap.add_argument("--host-bits", type=int, nargs="+", default=[10, 14, 16])
    a = ap.parse_args(argv)
    import torch
    from dib_amd import _lib, subset_information as si
    import dib_oracle as orc
    assert torch.cuda.is_available(), "the benchmark needs the GPU"
    lib = _lib.load_library()
    K = 2
    rec = {"device": torch.cuda.get_device_name(0), "K": K, "rows": "full truth tables of random circuits (data.random_circuit, seed B)",
           "sizes": {}, "host_backend": {}, "fold_width_sweep": {}}
    max_err = 0.0
    for B in a.bits:
        x, y = table_of(B)
        t0 = time.perf_counter()
        info = si.subset_information(x, y)          # first call of this size: includes the code object's load at the first B
        first = time.perf_counter() - t0
        t0 = time.perf_counter()
        info = si.subset_information(x, y)
        h2h = time.perf_counter() - t0
        T, fb, _ = si.joint_counts(x, y)
        counts = torch.from_numpy(T.astype(np.int32)).cuda()
        out = torch.zeros(1 << B, dtype=torch.float64, device="cuda")
        L = low_bits(B, K)
        reps = 20 if B <= 16 else 5
        ms, all_ms = kernel_ms(lib, counts, B, K, out, 0, 1 << B, reps)
        assert np.array_equal(out.cpu().numpy(), info.bits)
        tail_ms, _ = kernel_ms(lib, counts, B, K, out, (1 << B) - (1 << L), 1 << L, reps)
        w = work(B, K, L)
        s = {"kernel_ms": round(ms, 4), "kernel_ms_repeats": all_ms, "host_to_host_s": round(h2h, 5), "first_call_s": round(first, 4),
             "heaviest_workgroup_alone_ms": round(tail_ms, 4), **w,
             "reads_per_s": w["reads"] / (ms * 1e-3), "adds_per_s": w["adds"] / (ms * 1e-3), "log2_f64_per_s": w["log2_f64"] / (ms * 1e-3),
             "entropy_y_bits": info.entropy_y_bits}
        if B in a.host_bits:
            t0 = time.perf_counter()
            host = si.subset_information(x, y, backend="host")
            s["host_backend_s"] = round(time.perf_counter() - t0, 4)
            s["max_abs_error_vs_host_bits"] = float(np.abs(host.bits - info.bits).max())
            max_err = max(max_err, s["max_abs_error_vs_host_bits"])
            rec["host_backend"][str(B)] = {"seconds": s["host_backend_s"], "extrapolated": False}
        if B == 10:
            t0 = time.perf_counter()
            shap = orc.shapley_values_bits(2 * x - 1, y.astype(np.int64))
            s["parent_oracle_shapley_loop_s"] = round(time.perf_counter() - t0, 4)
            s["max_abs_shapley_difference_bits"] = float(np.abs(shap - info.shapley_values()).max())
        if B in (14, 16):
            sweep = {}
            for forced in range(2, 9):
                _lib.set_tuning("subset_low_bits", forced)
                try:
                    sweep[str(forced)] = round(kernel_ms(lib, counts, B, K, out, 0, 1 << B, 5)[0], 4)
                finally:
                    _lib.set_tuning("subset_low_bits", 0)
            rec["fold_width_sweep"][str(B)] = sweep
        rec["sizes"][str(B)] = s
        print(B, json.dumps(s), flush=True)
    rec["max_abs_error_vs_host_bits"] = max_err
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
