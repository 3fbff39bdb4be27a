"""Cell 7 of Chaos_experiments.ipynb at full size (the paper's Fig. 1): random partitions of the Ikeda map's 2e7-point evaluation
trajectory, through dib_amd.random_partition_survey.  The trajectory (chaos_data.generate_data, seeded, host Python) is cached
as .npy in --cache-dir and is not part of the repository; its generation time is reported on its own.  Writes one JSON record
with every partition's H(U), h +- err and whether it was skipped, checks h <= h_KS = 0.726 within its error, and notes (does
not assert) how the spread compares with the notebook's printed 0.266 .. 0.688.
    python tools/partition_run.py --cache-dir DIR [--points 20000000] [--repeats 1] [--out FILE] [--npz-dir DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H_KS = 0.726


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-dir", required=True)
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--npz-dir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ctw_backend", default="host", choices=("host", "device"),
                    help="where the CTW entropy rates are estimated (dib_amd.ctw.estimate_entropy_windows)")
    a = ap.parse_args(argv)
    import torch
    from dib_amd import chaos_data
    from dib_amd import random_partition as rp

    os.makedirs(a.cache_dir, exist_ok=True)
    path = os.path.join(a.cache_dir, f"ikeda_eval_{a.points}_seed{a.seed}.npy")
    t0 = time.perf_counter()
    if os.path.exists(path):
        traj, gen_s = np.load(path), None
    else:
        traj = chaos_data.generate_data("ikeda", a.points, seed=a.seed)
        gen_s = time.perf_counter() - t0
        np.save(path, traj)
    t0 = time.perf_counter()
    recs = rp.random_partition_survey(traj, number_random_repeats=a.repeats, seed=a.seed, out_dir=a.npz_dir,
                                      ctw_backend=a.ctw_backend)
    survey_s = time.perf_counter() - t0
    kept = [r for r in recs if not r["skipped"]]
    rates = [r["entropy_rate"] for r in kept]
    below = all(r["entropy_rate"] <= H_KS + r["entropy_rate_err"] for r in kept)
    out = {"what": "Chaos_experiments.ipynb cell 7 (Fig. 1): random-MLP partitions of the Ikeda map",
           "device": torch.cuda.get_device_name(0), "points": len(traj), "trajectory_seed": a.seed,
           "trajectory_generation_s": None if gen_s is None else round(gen_s, 1), "repeats": a.repeats, "survey_s": round(survey_s, 1),
           "ctw_threads": rp.ctw_threads(), "ctw_backend": a.ctw_backend, "h_ks": H_KS, "all_rates_below_h_ks_within_err": below,
           "partitions": len(recs), "skipped": len(recs) - len(kept),
           "rate_min": min(rates) if rates else None, "rate_max": max(rates) if rates else None,
           "notebook_printed_rate_range": [0.266, 0.688],
           "records": [{k: v for k, v in r.items() if k not in ("entropy_rate_values", "file")} for r in recs]}
    print(json.dumps({k: v for k, v in out.items() if k != "records"}))
    for r in recs:
        print(f"iter {r['rand_iter']} A={r['alphabet_size']} N={r['number_mlp_layers']} {r['activation']:4s}: "
              f"H(U) = {r['entropy_single_timestep']:.4f}" + ("  skipped" if r["skipped"] else
              f"  h = {r['entropy_rate']:.6f} +- {r['entropy_rate_err']:.6f}  ({r['symbolize_s']:.2f} s + {r['characterize_s']:.1f} s)"))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out) + "\n")
    if not below:
        sys.exit(1)


if __name__ == "__main__":
    main()
