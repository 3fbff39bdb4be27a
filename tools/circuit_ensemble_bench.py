"""CircuitEnsemble at the Boolean-circuit notebook's size (B = 512, predictor (256, 256, 256)) for R = 1 (one SI circuit),
R = 6 (the six SI circuits of Fig. S1) and R = 20 (the paper circuit over seeds): ms per lockstep step, ms per replica-step and
library launches per step - against R sequential CircuitIB steps (the class the ensemble does not touch) measured in the same
process, blocks of the two interleaved; every block is bracketed by a device synchronisation and preceded by warm-up steps, the
figures are medians over the blocks and the blocks themselves are kept (their spread is the noise floor).  One JSON line.

    python tools/circuit_ensemble_bench.py [--steps 2000] [--blocks 7] [--out profiles/circuit_ensemble_bench.json]
(a block of 2000 steps is 0.16 s of device time for the ensemble at R = 1 and 3.3 s for the 20 sequential models)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuit_ensemble_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from dib_amd import circuit

    sync = torch.cuda.synchronize
    B, beta = 512, 0.1
    si = [circuit.truth_table(s) for s in circuit.SI_CIRCUITS]
    paper = circuit.truth_table(circuit.PAPER_CIRCUIT)
    cases = [("one SI circuit (c)", [si[2]]), ("the six SI circuits", si), ("the paper circuit over 20 seeds", [paper] * 20)]
    rec = {"workload": "Boolean-circuit notebook cell 6 / 10 at its size: B = 512, predictor (256, 256, 256) leaky_relu, Adam",
           "protocol": f"per case: {a.warmup} warm-up steps of both, then {a.blocks} blocks x {a.steps} lockstep steps interleaved "
                       f"with {a.blocks} blocks of the baseline (R CircuitIB models stepped one after another, reported per "
                       "model-step); synchronize around each block; medians, all blocks kept", "rows": []}
    for name, tables in cases:
        R = len(tables)
        ens = circuit.CircuitEnsemble(tables)
        lib = ens.lib
        singles = [circuit.CircuitIB(t.shape[1] - 1, noise_seed=r, init_seed=r) for r, t in enumerate(tables)]
        for _ in range(a.warmup):
            ens.train_step(beta, batch_size=B)
            for m, t in zip(singles, tables):
                m.train_step(t, beta, batch_size=B)
        sync()
        n0 = lib.dib_launch_count()
        ens._step(B, [beta] * R)
        launches = int(lib.dib_launch_count() - n0)
        tab0 = singles[0]._table(tables[0])
        n0 = lib.dib_launch_count()
        singles[0]._step(tab0, B, beta)
        launches_single = int(lib.dib_launch_count() - n0)
        dev_tables = [m._table(t) for m, t in zip(singles, tables)]
        betas = [beta] * R
        ens_ms, base_ms = [], []
        for _ in range(a.blocks):      # (the bare steps of both: no loss read-back, as in fit)
            sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                ens._step(B, betas)
            sync()
            ens_ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                for m, t in zip(singles, dev_tables):
                    m._step(t, B, beta)
            sync()
            base_ms.append((time.perf_counter() - t0) * 1e3 / a.steps / R)
        e, b = float(np.median(ens_ms)), float(np.median(base_ms))
        rec["rows"].append({"case": name, "replicas": R, "ms_per_lockstep_step": round(e, 4), "ms_per_replica_step": round(e / R, 4),
                            "single_model_ms_per_step": round(b, 4), "replica_step_over_single_step": round(e / R / b, 4),
                            "library_launches_per_step": launches, "single_model_launches_per_step": launches_single,
                            "blocks_ms_per_replica_step": [round(v / R, 4) for v in ens_ms],
                            "blocks_single_model_ms_per_step": [round(v, 4) for v in base_ms]})
        del ens, singles
        torch.cuda.empty_cache()
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
