"""The CTW entropy-rate estimator on the device (dib_amd.ctw.estimate_entropy_windows, csrc/dib_ctw_levels.h) against the host
estimator on the same box (estimate_entropy_batch on 16 threads) - never against itself.

    python tools/ctw_device_bench.py --out profiles/ctw_device_bench.json

Workloads: the default 75 windows of measurement.entropy_rate_fit (15 log-spaced lengths 2e3 .. 2e6 x 5 draws, seed 0) on
logistic-map symbols (A = 2) and on a random partition of the Ikeda map (A = 4); one window of 2e6 symbols alone; one
random_partition_survey of a single partition under each backend; and the largest relative difference of the unrounded code
length from the float64 restatement over the 288-case grid of tests/_oracle_ctw_levels.py (the bound of
tests/test_gpu_ctw_levels.py is 16 x that figure)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_SECOND = 8.0e12   # MI355X peak
# bytes an element of a level's list moves through global memory in one level step: count reads (t, node) = 8 and two symbols
# = 2; place reads (t, node) = 8, one symbol = 1 and the child's key record = 8, and writes (t, node) = 8.  The per-node arrays
# (histograms, scan, records) are not included: they are shared by the elements of a node.
BYTES_PER_ELEMENT_STEP = 43


def default_windows(n_symbols: int, seed: int = 0, draws: int = 5):
    """the windows measurement.entropy_rate_fit draws by default: the same rng.choice calls"""
    rng = np.random.default_rng(seed)
    starts, lengths = [], []
    for n in np.logspace(np.log10(2000), np.log10(2_000_000), 15, dtype=np.int32):
        for _ in range(draws):
            starts.append(int(rng.choice(n_symbols - int(n))))
            lengths.append(int(n))
    return np.array(starts, dtype=np.int64), np.array(lengths, dtype=np.int64)


def logistic_symbols(n: int) -> np.ndarray:
    out = np.empty(n, dtype=np.uint8)
    v = 0.3
    for i in range(n):
        v = 4.0 * v * (1.0 - v)
        out[i] = v >= 0.5
    return out


def measure(ctw, torch, sym_host, sym_dev, starts, lengths, A, threads, reps):
    t0 = time.perf_counter()
    host = ctw.estimate_entropy_batch([sym_host[s: s + n] for s, n in zip(starts, lengths)], A, threads=threads)
    host_s = time.perf_counter() - t0
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rates, det = ctw.estimate_entropy_windows(sym_dev, starts, lengths, A, return_details=True)
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, rates, det)
    dt, rates, det = best
    steps = np.abs(np.asarray(rates, np.float32).view(np.int32).astype(np.int64) - np.asarray(host, np.float32).view(np.int32).astype(np.int64))
    moved = det["element_steps"] * BYTES_PER_ELEMENT_STEP
    return {"windows": int(len(starts)), "window_symbols": int(lengths.sum()), "alphabet_size": A, "host_threads": threads,
            "host_seconds": round(host_s, 4), "device_seconds_end_to_end": round(dt, 4),
            "device_seconds_level_steps": round(det["level_seconds"], 4), "device_seconds_bottom_up": round(det["mix_seconds"], 4),
            "device_seconds_read_back": round(det["readback_seconds"], 5), "chunks": det["chunks"], "levels": det["levels"],
            "element_steps": int(det["element_steps"]), "element_steps_per_symbol": round(det["element_steps"] / max(1, lengths.sum()), 2),
            "bytes_per_element_step": BYTES_PER_ELEMENT_STEP,
            "fraction_of_hbm_bandwidth": round(moved / max(det["level_seconds"], 1e-9) / HBM_BYTES_PER_SECOND, 4),
            "host_over_device": round(host_s / dt, 2), "windows_recomputed_on_host": int(det["fallback"].sum()),
            "rates_off_by_one_float32_step": int((steps == 1).sum()), "rates_off_by_more": int((steps > 1).sum())}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--symbols", type=int, default=4_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-survey", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    import dib_amd  # noqa: F401
    from dib_amd import chaos_data, ctw
    from dib_amd import random_partition as rp
    import _oracle_ctw_levels as lv

    out = {"what": "CTW entropy rates of windows of one symbol sequence: device level build against the host estimator",
           "device": torch.cuda.get_device_name(0), "symbols": a.symbols}
    # ---- the grid: the figure the test's bound is 16 x of
    worst = 0.0
    for A in lv.GRID_ALPHABETS:
        seqs = [s for al, s in lv.grid_cases() if al == A]
        lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        _, det = ctw.estimate_entropy_windows(np.concatenate(seqs), starts, lengths, A, return_details=True)
        for s, bits, fb in zip(seqs, det["code_length_bits"], det["fallback"]):
            if not fb:
                want = lv.ctw_levels(s, A)["code_length_bits"]
                worst = max(worst, abs(bits - want) / want)
    out["grid_max_relative_code_length_difference"] = worst
    print("grid_max_relative_code_length_difference", worst, flush=True)

    # ---- logistic map, A = 2
    sym = logistic_symbols(a.symbols)
    dev = torch.from_numpy(sym).to("cuda")
    starts, lengths = default_windows(a.symbols)
    ctw.estimate_entropy_windows(dev, starts[:5], lengths[:5], 2)   # warm-up: the library, the lgamma tables
    out["default_75_windows_logistic_A2"] = measure(ctw, torch, sym, dev, starts, lengths, 2, a.threads, a.reps)
    print(json.dumps(out["default_75_windows_logistic_A2"]), flush=True)
    out["one_window_2e6_logistic_A2"] = measure(ctw, torch, sym, dev, starts[-1:], lengths[-1:], 2, a.threads, a.reps)
    print(json.dumps(out["one_window_2e6_logistic_A2"]), flush=True)
    small = lengths <= 20_000
    out["windows_up_to_2e4_logistic_A2"] = measure(ctw, torch, sym, dev, starts[small], lengths[small], 2, a.threads, a.reps)
    print(json.dumps(out["windows_up_to_2e4_logistic_A2"]), flush=True)

    # ---- Ikeda map through a random partition, A = 4
    traj = chaos_data.generate_data("ikeda", a.symbols, seed=0)
    seed4 = rp.partition_seed(0, 0, 4, 2, "tanh")
    part = rp.RandomPartition(traj.shape[1], 4, 2, "tanh", seed=seed4)
    dev4, counts = part.symbolize_device(torch.from_numpy(np.ascontiguousarray(traj)).to("cuda"), return_counts=True)
    sym4 = dev4.cpu().numpy()
    out["ikeda_partition_entropy_single_timestep"] = rp.entropy_from_counts(counts.cpu().numpy())
    out["default_75_windows_ikeda_A4"] = measure(ctw, torch, sym4, dev4, starts, lengths, 4, a.threads, a.reps)
    print(json.dumps(out["default_75_windows_ikeda_A4"]), flush=True)

    # ---- what a user sees: one partition of the survey, end to end, under each backend
    if not a.skip_survey:
        for backend in ("host", "device"):
            t0 = time.perf_counter()
            recs = rp.random_partition_survey(traj, alphabet_sizes=(4,), layer_counts=(2,), activations=("tanh",), seed=0,
                                              threads=a.threads, ctw_backend=backend)
            out[f"survey_one_partition_{backend}"] = {
                "seconds": round(time.perf_counter() - t0, 3), "symbolize_s": round(recs[0]["symbolize_s"], 4),
                "characterize_s": round(recs[0].get("characterize_s", 0.0), 4), "entropy_rate": recs[0]["entropy_rate"],
                "entropy_rate_err": recs[0]["entropy_rate_err"]}
            print(backend, json.dumps(out[f"survey_one_partition_{backend}"]), flush=True)
    line = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
