"""The MI-bound characterization (paper Fig. S4) at the notebook's sizes, on the GPU: for each of the five variables of
dib_amd.mi_characterization.VARIABLES a dataset of 1 024 points, 25 separation scales, the Monte-Carlo I(U;X) from 200 runs of
10 000 samples and the InfoNCE / leave-one-out bounds of 512 batches (--figure-quality: 4 096) at batch sizes 64, 256, 1 024 in
32 dimensions.  Writes one <out>/mi_bounds_run_<variable>.json per variable (and, with --figures, the two-panel figure):

    python tools/mi_bounds_run.py --out profiles [--variables bits1,uniform] [--figure-quality] [--figures] [--seed 0]

Each record holds the separation scales, the Monte-Carlo curve with the standard error of its 200 run means, the bound statistics
(mean lower, std lower, mean upper, std upper over the batches), the largest |mean bound - Monte Carlo| per batch size, and for
the discrete variables the entropy of the sampled dataset beside the curve's large-separation plateau."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dataset_entropy_bits(x):
    _, counts = np.unique(np.asarray(x), axis=0, return_counts=True)
    p = counts / counts.sum()
    return float(-(p * np.log2(p)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--variables", default="")
    ap.add_argument("--figure-quality", action="store_true", help="4 096 evaluation batches instead of 512")
    ap.add_argument("--figures", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--train-size", type=int, default=1024)
    ap.add_argument("--mc-sample-size", type=int, default=10_000)
    ap.add_argument("--mc-runs", type=int, default=200)
    args = ap.parse_args()
    import torch

    from dib_amd import mi_characterization as mic
    if not torch.cuda.is_available():
        raise SystemExit("mi_bounds_run.py needs a GPU")
    os.makedirs(args.out, exist_ok=True)
    wanted = [v for v in args.variables.split(",") if v]
    nb = 4096 if args.figure_quality else 512
    for i, var in enumerate(mic.VARIABLES):
        if wanted and var.name not in wanted:
            continue
        x = var.sample(np.random.default_rng([args.seed, i]), args.train_size)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mic.characterize(x, var.separation_scales, number_evaluation_batches=nb, mc_sample_size=args.mc_sample_size,
                               number_monte_carlo_runs=args.mc_runs, seed=args.seed)
        wall = time.perf_counter() - t0
        resid = mic.largest_residuals(res)
        runs = res["monte_carlo_runs"]
        rec = {
            "variable": var.name, "label": var.label, "device": torch.cuda.get_device_name(0), "seed": args.seed,
            "train_size": args.train_size, "embedding_dimension": 32, "mc_sample_size": args.mc_sample_size,
            "number_monte_carlo_runs": args.mc_runs, "number_evaluation_batches": nb,
            "evaluation_batch_sizes": res["evaluation_batch_sizes"], "wall_seconds_characterize": round(wall, 3),
            "separation_scales": res["separation_scales"].tolist(), "monte_carlo_bits": res["monte_carlo"].tolist(),
            "monte_carlo_standard_error_bits": (runs.std(axis=1, ddof=1) / np.sqrt(runs.shape[1])).tolist(),
            "info_bound_stats_bits": res["info_bound_stats"].tolist(),
            "largest_abs_residual_bits": {str(bs): {"lower": lo, "upper": up} for bs, (lo, up) in resid.items()},
            "largest_upper_minus_lower_bits": {str(bs): float((res["info_bound_stats"][k, :, 2] - res["info_bound_stats"][k, :, 0]).max())
                                               for k, bs in enumerate(res["evaluation_batch_sizes"])},
        }
        if var.name != "uniform":
            rec["dataset_entropy_bits"] = dataset_entropy_bits(x)
            rec["monte_carlo_plateau_bits"] = float(res["monte_carlo"][-1])
        with open(os.path.join(args.out, f"mi_bounds_run_{var.name}.json"), "w") as f:
            json.dump(rec, f, indent=1)
        if args.figures:
            mic.save_figure(res, os.path.join(args.out, f"mi_bounds_run_{var.name}.png"), var.label, var.info_plot_lims,
                            var.info_residual_lims)
        print(var.name, f"{wall:.2f} s", "largest |residual| (lower, upper) per batch size:", resid, flush=True)


if __name__ == "__main__":
    main()
