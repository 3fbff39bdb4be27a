"""Boolean-circuit model at the paper's size (G = 10 input gates, B = 512, predictor Dense(256, leaky_relu) x3 -> Dense(1)):
one JSON line with
  - the training step: ms per step (no host sync inside the timed block), library launches per step (dib_launch_count) and
    the launches / ms dib_profile_summary attributes to its bracketed categories;
  - one information evaluation of all 10 channels (8 batches of 1024): the one-launch dib_circuit_mi_bounds against the
    80-launch loop of dib_mi_sandwich_rows over gates and batches on the same box (same inputs, same noise);
  - the wall time of the whole Fig. 1 run (50 000 steps, 200 evaluations, fit());
  - the float64 oracle's time per step (tests/_oracle_circuit.py, NumPy on the host) as the CPU baseline.
    python tools/circuit_bench.py [--steps 2000] [--no-fig1] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--no-fig1", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    import _oracle_circuit as oc
    from dib_amd import circuit
    from dib_amd._gemm_plan import _ptr
    from dib_amd._lib import check

    sync = torch.cuda.synchronize
    G, B = 10, 512
    table = circuit.truth_table(circuit.PAPER_CIRCUIT)
    m = circuit.CircuitIB(G)
    lib = m.lib
    rec = {"workload": "Boolean-circuit notebook cell 6 at its size: G = 10, B = 512, predictor [256, 256, 256] leaky_relu, "
                       "Keras Adam lr 1e-3; evaluation 8 batches x 1024 points per channel"}
    # ---- training step -----------------------------------------------------------------------
    for _ in range(50):
        m.train_step(table, 0.1, B)
    sync()
    n0 = lib.dib_launch_count()
    m.train_step(table, 0.1, B)
    launches = int(lib.dib_launch_count() - n0)
    sync()
    lib.dib_profile_enable(1)
    m.train_step(table, 0.1, B)
    ms = (ctypes.c_double * 17)()
    cnt = (ctypes.c_int * 17)()
    check(lib.dib_profile_summary(ms, cnt), "dib_profile_summary")
    lib.dib_profile_enable(0)
    blocks = []
    for _ in range(3):
        sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            m.train_step(table, 0.1, B)
        sync()
        blocks.append((time.perf_counter() - t0) * 1e3 / a.steps)
    rec["train_step"] = {"ms_per_step": round(float(np.median(blocks)), 5), "blocks_ms_per_step": [round(b, 5) for b in blocks],
                         "library_launches_per_step": launches,
                         "profiled_categories": {str(c): [int(cnt[c]), round(float(ms[c]), 5)] for c in range(17) if cnt[c]},
                         "protocol": f"median of 3 blocks x {a.steps} train_step calls, synchronize around each block"}
    # ---- one information evaluation ------------------------------------------------------------
    n, nb, seed = 1024, 8, 17
    for _ in range(3):
        m.estimate_channel_mi_bounds(seed, n, nb)
    rng = np.random.default_rng(seed)
    x = np.stack([np.array([-1.0, 1.0], np.float32)[rng.integers(0, 2, n)] for _ in range(nb)], 0)
    xd = torch.from_numpy(x).cuda()
    out = torch.empty((G, nb, 2), dtype=torch.float64, device="cuda")
    ws = m._mi_ws[(n, nb)]
    st = m.eng._stream()

    def fused():
        check(lib.dib_circuit_mi_bounds(_ptr(m.params, m.sc_off), G, _ptr(xd), n, nb, seed, _ptr(out), _ptr(ws), st), "mi")

    encs = [[m.feature_encoders[g](xd[b][:, None]).contiguous() for b in range(nb)] for g in range(G)]
    rws = torch.empty(int(lib.dib_mi_workspace_bytes(n, 1)) // 8 + 1, dtype=torch.float64, device="cuda")
    rr = torch.empty((G, nb, 2, n), dtype=torch.float64, device="cuda")

    def loop():
        for g in range(G):
            for b in range(nb):
                check(lib.dib_mi_sandwich_rows(_ptr(encs[g][b]), n, 1, seed, b, g, _ptr(rr[g, b, 0]), _ptr(rr[g, b, 1]), _ptr(rws),
                                               st), "rows")

    def timed(fn, reps=20):
        fn()
        sync()
        ts = []
        for _ in range(reps):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    n0 = lib.dib_launch_count()
    fused()
    l_fused = int(lib.dib_launch_count() - n0)
    n0 = lib.dib_launch_count()
    loop()
    l_loop = int(lib.dib_launch_count() - n0)
    sync()
    agree = float(np.abs(out.cpu().numpy() - rr.mean(dim=3).cpu().numpy()).max())
    rec["mi_evaluation"] = {"fused_ms": round(timed(fused), 4), "fused_launches": l_fused,
                            "rows_loop_ms": round(timed(loop), 4), "rows_loop_launches": l_loop,
                            "whole_estimate_channel_mi_bounds_ms": round(timed(lambda: m.estimate_channel_mi_bounds(seed, n, nb)), 4),
                            "max_abs_difference_nats": agree,
                            "protocol": "median of 20 synchronised calls; rows loop = 10 gates x 8 batches of dib_mi_sandwich_rows "
                                        "(prep + rows kernels) on pre-encoded inputs, the per-row means left out"}
    # ---- the whole Fig. 1 run --------------------------------------------------------------------
    if not a.no_fig1:
        m1 = circuit.CircuitIB(G)
        sync()
        t0 = time.perf_counter()
        h = m1.fit(table, number_training_steps=50_000, batch_size=B, beta_start=1e-3, beta_end=5.0, seed=0)
        sync()
        rec["fig1_fit"] = {"wall_s": round(time.perf_counter() - t0, 3), "steps": 50_000, "evaluations": int(len(h["evaluation_steps"]))}
    # ---- float64 oracle per step (CPU baseline) ----------------------------------------------------
    p = oc.Params([np.asarray(w, np.float64) for w in m.predictive_model.get_weights()],
                  np.ones(G), np.full(G, -3.0))
    stt = oc.adam_init(p)
    t0 = time.perf_counter()
    k = 20
    for s in range(k):
        r = oc.step(p, table, oc.draw_rows(0, s, B, G), oc.eps(0, s, B, G), 0.1)
        oc.adam(p, r["grads"], stt)
    rec["float64_oracle_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / k, 3)
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
