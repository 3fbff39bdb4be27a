"""MeasurementEnsemble at the chaos notebook's size (Ikeda d = 2, L = 12, B = 2048, default widths) for R in {1, 4, 20}: ms per
lockstep step, ms per replica-step, library launches per step and bytes of workspace - against R sequential MeasurementIB steps
(the class the ensemble does not touch) measured in the same process, blocks of the two interleaved.  One JSON line.

    python tools/measurement_ensemble_bench.py [--replicas 1 4 20] [--steps 50] [--out profiles/measurement_ensemble_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ensemble_workspace_bytes(e, B):
    """device bytes the ensemble holds beyond its parameters: row buffers, slabs, kernel workspaces, descriptor tables"""
    bf = e._buffers(B)
    n = sum(t.numel() * t.element_size() for t in bf.values() if hasattr(t, "numel"))
    for pl in bf["pl"].values():
        n += pl["ws"].numel() * 4 + sum(g.dev.numel() for g in list(pl["g"].values()) + list(pl["wgrad"].values()))
    return int(n)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4, 20])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from dib_amd import MeasurementEnsemble, chaos_data
    from dib_amd.measurement import MeasurementIB

    sync = torch.cuda.synchronize
    B = 2048
    traj = chaos_data.generate_data("ikeda", 1_000_000, seed=0).astype(np.float32)
    tdev = torch.from_numpy(traj).cuda()
    rec = {"workload": "chaos notebook cell 10 at its size: Ikeda d = 2, L = 12, B = 2048, E = 8, A = 2, IB / VQ [128, 128], "
                       "aggregator / reference [256, 256], InfoNCE 32 l2sq; R identical models (seeds differ)",
           "protocol": f"per R: {a.blocks} blocks x {a.steps} lockstep steps interleaved with {a.blocks} blocks of the baseline "
                       "(R MeasurementIB models stepped one after another, per model-step); synchronize around each block; "
                       "medians", "rows": []}
    for R in a.replicas:
        e = MeasurementEnsemble(R, input_dimensionality=2)
        L, lib = e.L, e.lib
        singles = [MeasurementIB(2, init_seed=4 * r, noise_seed=r) for r in range(R)]
        rng = np.random.default_rng(0)
        starts = [torch.from_numpy(rng.choice(len(traj) - L, size=(R, B)).astype(np.int32)).cuda() for _ in range(a.steps)]
        for s in starts[:5]:
            e.match_batch_from_starts(tdev, s, True, 1.0)
            for k, m in enumerate(singles):
                m.match_batch_from_starts(tdev, s[k], True, 1.0)
        sync()
        n0 = lib.dib_launch_count()
        e.match_batch_from_starts(tdev, starts[0], True, 1.0)
        launches = int(lib.dib_launch_count() - n0)
        n0 = lib.dib_launch_count()
        singles[0].match_batch_from_starts(tdev, starts[0][0], True, 1.0)
        launches_single = int(lib.dib_launch_count() - n0)
        ens_ms, base_ms = [], []
        for _ in range(a.blocks):
            sync()
            t0 = time.perf_counter()
            for s in starts:
                e.match_batch_from_starts(tdev, s, True, 1.0)
            sync()
            ens_ms.append((time.perf_counter() - t0) * 1e3 / len(starts))
            sync()
            t0 = time.perf_counter()
            for s in starts:
                for k, m in enumerate(singles):
                    m.match_batch_from_starts(tdev, s[k], True, 1.0)
            sync()
            base_ms.append((time.perf_counter() - t0) * 1e3 / len(starts) / len(singles))
        ens, base = float(np.median(ens_ms)), float(np.median(base_ms))
        rec["rows"].append({"replicas": R, "ms_per_lockstep_step": round(ens, 4), "ms_per_replica_step": round(ens / R, 4),
                            "single_model_ms_per_step": round(base, 4), "replica_step_over_single_step": round(ens / R / base, 4),
                            "library_launches_per_step": launches, "single_model_launches_per_step": launches_single,
                            "workspace_bytes": _ensemble_workspace_bytes(e, B),
                            "parameter_buffer_bytes": int(e._flat.numel() * 4),
                            "blocks_ms_per_lockstep_step": [round(v, 4) for v in ens_ms],
                            "blocks_single_model_ms_per_step": [round(v, 4) for v in base_ms]})
        del e, singles, starts
        torch.cuda.empty_cache()
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
