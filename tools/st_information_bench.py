"""Information tracking of the set-transformer notebook at its own size, one JSON record (default
profiles/st_information_bench.json):
  - both particle types' information maps (100 x 100 probes in chunks of 100, 16 batches of 512 validation neighbourhoods x 50
    particles per chunk): SetTransformerDIB.information_maps (one launch per type) against two information_map calls (a host loop
    of 1 600 dib_mi_probe_bounds per type), alternated in one process, with the largest difference between them;
  - the I(U;X) evaluation (16 batches x 32 neighbourhoods x 50 particles, information_bounds);
  - kernel times from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--kernels-only), with the FLOP and
    issue-slot model of the map kernel (below) and its fraction of the FP64 vector peak;
  - a 25 000-step fit at the notebook's schedule with and without track_information.
Synthetic data: 2 000 validation (and 2 000 training) neighbourhoods of 50 particles drawn so that
convert_to_per_particle_feature_set applies (60 particles in a disc, nearest 50 kept, types 1 / 2).
    python tools/st_information_bench.py [--out FILE] [--fit-steps 25000] [--reps 2] [--no-profile]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_VAL, P, E = 2000, 50, 32
FP64_PEAK = 78.6e12   # AMD's published MI355X FP64 vector figure (not in the microarchitecture notes; unmeasured here)


def _data(n, seed):
    from dib_amd.set_transformer import convert_to_per_particle_feature_set
    rng = np.random.default_rng(seed)
    feats, y = [], []
    for _ in range(n):
        r = 3.5 * np.sqrt(rng.random(60))
        a = rng.random(60) * 2 * np.pi
        pos = np.stack([r * np.cos(a), r * np.sin(a)], -1).astype(np.float32)
        feats.append(convert_to_per_particle_feature_set(pos, rng.integers(1, 3, 60), P))
        y.append(float(rng.random() < 0.5))
    return np.stack(feats).astype(np.float32), np.asarray(y, np.float32)


def map_model():
    """per type: pairs = probes x batches x N data rows; a pair costs E x (fma + fma) + one log-sum-exp update"""
    M, nb, N = 10000, 16, 512 * P
    pairs = M * nb * N
    return dict(pairs_per_type=pairs, fp64_flop_per_type=4 * E * pairs,
                issue_slots_per_pair="2E FP64 FMA + 2 LDS broadcast reads of (1/sigma, mu/sigma) per dimension pair + ~20 for the "
                                     "exp and compare of the log-sum-exp update",
                fp64_fma_issue_floor_ms_both_types=2 * 2 * E * pairs * 2 / FP64_PEAK * 1e3)


def kernels_only():
    import torch
    import dib_amd
    from dib_amd.set_transformer import notebook_probe_grid
    m = dib_amd.SetTransformerDIB()
    xv, _ = _data(N_VAL, 1)
    pos = notebook_probe_grid()
    m.information_maps(pos, xv)
    m.information_bounds(xv)
    torch.cuda.synchronize()


def profile_kernels():
    """kernel time of one information_maps + one information_bounds under rocprofv3 --kernel-trace --stats"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "run", "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only"]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            return dict(error=f"rocprofv3 rc {res.returncode}", tail=(res.stdout + res.stderr)[-1500:])
        stats = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Name"]
                    if "dib_sti" in name or "dib_mi_" in name:
                        stats[name.split("(")[0]] = dict(calls=int(row["Calls"]), total_ms=float(row["TotalDurationNs"]) / 1e6,
                                                         avg_us=float(row["AverageNs"]) / 1e3)
        return stats


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "st_information_bench.json"))
    ap.add_argument("--fit-steps", type=int, default=25000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args(argv)
    if a.kernels_only:
        return kernels_only()
    import torch
    import dib_amd
    from dib_amd.set_transformer import notebook_probe_grid
    sync = torch.cuda.synchronize
    rec = dict(workload=f"set-transformer notebook model (default constructor), E = {E}; {N_VAL} validation neighbourhoods x {P} "
                        "particles (synthetic); maps: 100 x 100 probes, chunks of 100, 16 batches x 512 neighbourhoods per chunk; "
                        "bounds: 16 batches x 32 neighbourhoods",
               device=torch.cuda.get_device_name(0))
    m = dib_amd.SetTransformerDIB()
    xv, yv = _data(N_VAL, 1)
    pos = notebook_probe_grid()
    # ---- maps: new (one launch per type) against the information_map loop, alternated ----
    m.information_maps(pos[:200], xv, num_eval_batches=2)   # warm-up of every shape
    m.information_map(pos[:200], 0, xv, num_eval_batches=1)
    sync()
    t_new, t_old, new, old = [], [], None, None
    for _ in range(a.reps):
        sync()
        t0 = time.perf_counter()
        new = m.information_maps(pos, xv)
        sync()
        t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        old = np.stack([m.information_map(pos, t, xv) for t in (0, 1)])
        sync()
        t_old.append(time.perf_counter() - t0)
    diff = np.abs(new - old)
    rec["maps"] = dict(new_s=t_new, old_s=t_old, new_ms_min=1e3 * min(t_new), old_ms_min=1e3 * min(t_old),
                       speedup=min(t_old) / min(t_new), max_abs_diff=float(diff.max()),
                       max_rel_diff=float(diff.max() / (1 + np.abs(old).max())),
                       protocol="wall clock of the whole call incl. the validation and probe encodes, the index draws and the copy "
                                "back, synchronised; new and old alternated, same process, same inputs and seed")
    # ---- I(U;X) ----
    m.information_bounds(xv)
    ts = []
    for i in range(10):
        sync()
        t0 = time.perf_counter()
        b = m.information_bounds(xv, seed=i)
        ts.append(time.perf_counter() - t0)
    rec["bounds"] = dict(ms_median=1e3 * float(np.median(ts)), ms=[1e3 * t for t in ts], last=b,
                         protocol="information_bounds (encode of the 100 000 validation particles + one launch + copy back), median of 10")
    rec["model"] = map_model()
    if not a.no_profile:
        k = profile_kernels()
        rec["kernels"] = k
        mk = k.get("void dib_sti_bounds_kernel<32>") or next((v for n, v in k.items() if "dib_sti_bounds_kernel" in n), None) \
            if isinstance(k, dict) else None
        if mk:
            # the rocprof run made one information_maps (2 map launches) and one information_bounds (1 launch) of this kernel
            map_ms = mk["total_ms"] * 2 * rec["model"]["fp64_flop_per_type"] / (
                2 * rec["model"]["fp64_flop_per_type"] + 4 * E * 16 * (32 * P) ** 2)
            rec["map_kernel"] = dict(ms_both_types_est=map_ms, tflops=2 * rec["model"]["fp64_flop_per_type"] / map_ms / 1e9,
                                     fraction_of_fp64_peak=2 * rec["model"]["fp64_flop_per_type"] / (map_ms / 1e3) / FP64_PEAK,
                                     note="bounds-kernel time split between the two map launches and the bounds launch by FLOPs")
    # ---- fit at the notebook's schedule, with and without tracking ----
    if a.fit_steps > 0:
        xtr, ytr = _data(N_VAL, 2)
        for track in (False, True):
            mm = dib_amd.SetTransformerDIB(init_seed=0)
            sync()
            t0 = time.perf_counter()
            h = mm.fit(xtr, ytr, number_training_steps=a.fit_steps, particle_features_val=xv, loci_val=yv,
                       track_information=track)
            sync()
            rec[f"fit_{'tracked' if track else 'untracked'}"] = dict(
                s=time.perf_counter() - t0, steps=a.fit_steps, evaluations=len(h["eval_steps"]),
                info_evaluations=len(h.get("info_eval_steps", [])), maps=sorted(h.get("information_maps", {})),
                last_info_bounds_nats=(h["info_bounds"][-1] if track and h["info_bounds"] else None),
                final_bce_val=h["bce_series_val"][-1] if h["bce_series_val"] else None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in rec if k in ("maps", "bounds", "map_kernel")}))


if __name__ == "__main__":
    main()
