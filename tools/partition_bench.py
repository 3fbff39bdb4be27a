"""Random-MLP partitions (Chaos_experiments.ipynb cell 7) at the notebook's size: one JSON line with
  - dib_partition_symbolize on 2e7 Ikeda points for the 12 notebook configurations (A in {2, 4}, N in {1, 2, 3} x 64 units,
    tanh / relu) and the widest envelope shape (3 x 128, A = 16): kernel time from device events after warm-up (median of
    --reps), points/s, useful FLOPs per point 2 (d H1 + H1 H2 + ... + HN A) and their fraction of the fp32 MFMA peak
    (157.3 TFLOP/s, a computed floor), fp32 against fp64 input;
  - the same-run baseline: DenseStack forward (the library's GEMM path) + torch abs().argmax() + bincount in chunks of 2^20 rows,
    its time and its symbols against the fused kernel's (a mismatch must sit where the float64 margin is below the fp32
    rounding bound of tests/test_gpu_random_partition.py);
  - one survey partition end to end: host->device copy of the float64 trajectory, symbolisation, CTW windows, the fit.
The input is a seeded 2e6-point Ikeda trajectory tiled to --points (the per-point cost does not depend on which points).
    python tools/partition_bench.py [--points 20000000] [--base-points 2000000] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TFLOPS = 157.3   # MI355X fp32 MFMA


def flops_per_point(d, widths, A):
    dims = [d] + list(widths) + [A]
    return 2 * sum(i * o for i, o in zip(dims[:-1], dims[1:]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--base-points", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true")
    ap.add_argument("--e2e-trajectory", default=None,
                    help="float64 .npy of an untiled evaluation trajectory for the end-to-end partition (tools/partition_run.py's "
                         "cache); the tiled bench input repeats itself, so CTW windows longer than its period mean nothing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import dib_amd
    from dib_amd import chaos_data, measurement
    from dib_amd import random_partition as rp
    from dib_amd.dense import DenseStack
    from dib_amd.measurement import _Eng
    import _oracle_random_partition as orp

    t0 = time.perf_counter()
    base = chaos_data.generate_data("ikeda", a.base_points, 100_000, seed=0)
    gen_s = time.perf_counter() - t0
    reps = -(-a.points // a.base_points)
    traj = np.tile(base, (reps, 1))[: a.points]
    n = len(traj)
    x64 = torch.from_numpy(traj).cuda()
    x32 = x64.float()
    sym = torch.empty(n, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(16, dtype=torch.int64, device="cuda")

    def kernel_ms(part, x):
        for _ in range(2):
            part._launch(x, sym, None, counts)
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            part._launch(x, sym, None, counts)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    configs = [(A, N, 64, act) for A in (2, 4) for N in (1, 2, 3) for act in ("tanh", "relu")]
    configs += [(16, 3, 128, "tanh"), (16, 3, 128, "relu")]
    eng = _Eng("cuda:0")
    rows = []
    for A, N, H, act in configs:
        w = rp.draw_weights(2, A, N, H, seed=1000 * A + 10 * N + H + len(act))
        part = rp.RandomPartition(2, A, N, act, H, weights=w)
        f = flops_per_point(2, [H] * N, A)
        r = {"A": A, "N": N, "H": H, "act": act, "flops_per_point": f}
        for name, x in (("fp64", x64), ("fp32", x32)):
            ms = kernel_ms(part, x)
            r[f"kernel_ms_{name}"] = round(ms, 4)
            r[f"points_per_s_{name}"] = n / (ms * 1e-3)
            r[f"peak_fraction_{name}"] = round(f * n / (ms * 1e-3) / (PEAK_TFLOPS * 1e12), 4)
        r["floor_ms_at_peak"] = round(f * n / (PEAK_TFLOPS * 1e12) * 1e3, 4)
        part._launch(x64, sym, None, None)
        fused = sym.cpu().numpy()
        if not a.skip_baseline:
            stack = DenseStack(eng, 2, [H] * N, A, act, use_positional_encoding=False)
            for l in range(N + 1):
                stack.kernel(l).copy_(torch.from_numpy(w[2 * l]))
                stack.bias(l).copy_(torch.from_numpy(w[2 * l + 1]))
            chunk = 1 << 20
            bsym = torch.empty(n, dtype=torch.uint8, device="cuda")

            def baseline():
                bc = torch.zeros(A, dtype=torch.int64, device="cuda")
                for c0 in range(0, n, chunk):
                    out = stack.forward(x32[c0: c0 + chunk])
                    s = out.abs().argmax(1)
                    bsym[c0: c0 + chunk] = s.to(torch.uint8)
                    bc += torch.bincount(s, minlength=A)
                return bc
            baseline()
            ts = []
            for _ in range(max(2, a.reps // 2)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                baseline()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            r["baseline_ms"] = round(float(np.median(ts)), 3)
            r["speedup_vs_baseline"] = round(r["baseline_ms"] / r["kernel_ms_fp64"], 2)
            bs = bsym.cpu().numpy()
            bad = np.flatnonzero(bs != fused)
            r["symbol_mismatches_vs_baseline"] = int(bad.size)
            if bad.size:
                pts = traj[bad[:10_000]]
                ref = orp.forward(w, pts, act)
                bound = 2 * 1e-5 * orp.abs_forward(w, pts, act).max(1)
                r["mismatches_outside_margin_bound"] = int((orp.margin(ref) >= bound).sum())
            else:
                r["mismatches_outside_margin_bound"] = 0
            del stack
        rows.append(r)
        print(json.dumps(r), flush=True)

    # one survey partition end to end (A = 4, N = 3, tanh): copy, symbolise, CTW, fit
    e2e_src = "tiled bench input"
    if a.e2e_trajectory:
        traj, e2e_src = np.load(a.e2e_trajectory), os.path.basename(a.e2e_trajectory)
        n = len(traj)
    del x64, x32
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xd = torch.from_numpy(traj).cuda()
    torch.cuda.synchronize()
    t_copy = time.perf_counter() - t0
    part = rp.RandomPartition(2, 4, 3, "tanh", seed=7)
    part.symbolize(xd[:1000])
    t0 = time.perf_counter()
    s, c = part.symbolize(xd, chunk_size=n, return_counts=True)
    t_sym = time.perf_counter() - t0
    h_u = rp.entropy_from_counts(c)
    from scipy import optimize
    from dib_amd import ctw, utils
    ndp = np.logspace(np.log10(2000), np.log10(2_000_000), 15, dtype=np.int32)
    rng = np.random.default_rng(0)
    wins = []
    for m in ndp:
        for _ in range(5):
            st = rng.choice(len(s) - int(m))
            wins.append(s[st: st + int(m)])
    th = rp.ctw_threads()
    t0 = time.perf_counter()
    rates = ctw.estimate_entropy_batch(wins, 4, threads=th).reshape(-1, 5)
    t_ctw = time.perf_counter() - t0
    t0 = time.perf_counter()
    try:
        fit, _ = optimize.curve_fit(utils.entropy_rate_scaling_ansatz, ndp, rates.mean(1), p0=[1, 0.5, 1], sigma=rates.std(1))
    except RuntimeError:
        fit = [float("nan")]
    t_fit = time.perf_counter() - t0
    e2e = {"config": f"A=4, N=3 x 64, tanh, {n} float64 points", "trajectory": e2e_src, "h2d_copy_s": round(t_copy, 3), "symbolize_s": round(t_sym, 3),
           "ctw_s": round(t_ctw, 3), "ctw_threads": th, "fit_s": round(t_fit, 4), "total_s": round(t_copy + t_sym + t_ctw + t_fit, 3),
           "H_U": h_u, "entropy_rate": float(fit[0]),
           "reference_per_partition_s": [49.8, 89.9],
           "note": "the reference's per-partition times are from its own (different) hardware and TensorFlow stack"}
    rec = {"what": "random-MLP partitions (cell 7): dib_partition_symbolize vs DenseStack + abs().argmax() + bincount",
           "device": torch.cuda.get_device_name(0), "points": n,
           "input": f"seeded Ikeda trajectory of {a.base_points} points (seed 0) tiled to {n}", "trajectory_gen_s": round(gen_s, 1),
           "peak_tflops_fp32_mfma": PEAK_TFLOPS, "reps": a.reps, "configs": rows, "survey_partition_end_to_end": e2e,
           "dib_amd": dib_amd.__name__}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
