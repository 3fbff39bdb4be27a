"""Measurement-partition model at the chaos notebook's size (d = 2 Ikeda, L = 12, E = 8, A = 2, B = 2048): one JSON line with
  - the training step: ms per step (fwd + bwd + Adam, no host sync inside the timed block) and library launches per step;
  - symbolisation of N = 2e7 points x K = 100 draws: points/s and the fraction of the fp32 MFMA peak the VQ FLOPs reach
    (whole symbolize() call: IB encoder chunks + fused kernel + the symbols' copy to the host), and the fused kernel alone;
  - a same-box A/B on one chunk: the fused dib_measure_symbolize against the composition the reference itself runs
    (VQ DenseStack forward on the expanded [K * chunk, E] matrix + torch.argmax + the majority), same encodings;
  - host characterisation time (CTW batch + curve_fit) of the 2e7 symbols.
    python tools/measurement_bench.py [--points 20000000] [--out FILE]
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
PEAK_TFLOPS = 157.3   # MI355X fp32 MFMA


def _median_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    from dib_amd import chaos_data
    from dib_amd._gemm_plan import _ptr
    from dib_amd._lib import check
    from dib_amd.measurement import MeasurementIB, characterize_partition

    sync = torch.cuda.synchronize
    traj = chaos_data.generate_data("ikeda", 1_000_000, seed=0).astype(np.float32)
    m = MeasurementIB(2, noise_seed=0, init_seed=0)
    lib, K, E, A = m.lib, 100, m.E, m.A
    rec = {"workload": "chaos notebook cell 10 at its size: Ikeda d = 2, L = 12, B = 2048, E = 8, A = 2, IB / VQ [128, 128], "
                       "aggregator / reference [256, 256], InfoNCE 32 l2sq; symbolisation K = 100 draws"}
    # ---- training step --------------------------------------------------------------------
    tdev = torch.from_numpy(traj).cuda()
    rng = np.random.default_rng(0)
    starts = [torch.from_numpy(rng.choice(len(traj) - m.L, size=2048).astype(np.int32)).cuda() for _ in range(a.steps)]
    for s in starts[:20]:
        m.match_batch_from_starts(tdev, s, True, 1.0)
    sync()
    n0 = lib.dib_launch_count()
    m.match_batch_from_starts(tdev, starts[0], True, 1.0)
    launches = int(lib.dib_launch_count() - n0)
    blocks = []
    for _ in range(3):
        sync()
        t0 = time.perf_counter()
        for s in starts:
            m.match_batch_from_starts(tdev, s, True, 1.0)
        sync()
        blocks.append((time.perf_counter() - t0) * 1e3 / len(starts))
    rec["train_step"] = {"ms_per_step": round(float(np.median(blocks)), 4), "blocks_ms_per_step": [round(b, 4) for b in blocks],
                         "library_launches_per_step": launches, "rows_per_step": 2048 * m.L,
                         "protocol": f"median of 3 blocks x {a.steps} steps, synchronize around each block"}
    # ---- symbolisation at N = 2e7 -------------------------------------------------------------
    ev = chaos_data.generate_data("ikeda", 2_000_000, seed=1).astype(np.float32)
    x = np.tile(ev, (a.points // len(ev) + 1, 1))[:a.points]
    noise = np.random.default_rng(0).standard_normal((K, E)).astype(np.float32)
    vq_flop = 2.0 * (E * 128 + 128 * 128 + 128 * A)
    m.symbolize(x[:1 << 20], noise_vector=noise)
    sync()
    t0 = time.perf_counter()
    sym = m.symbolize(x, noise_vector=noise)
    t_sym = time.perf_counter() - t0
    # the fused kernel alone on one resident chunk of 2^18 encoded points
    chunk = 1 << 18
    xc = torch.from_numpy(x[:chunk]).cuda()
    enc = m.ib.forward(xc).clone()
    nz = torch.from_numpy(noise).cuda()
    out = torch.empty(chunk, dtype=torch.uint8, device="cuda")
    st = m.eng._stream()
    fused = lambda: check(lib.dib_measure_symbolize(ctypes.byref(m._desc), _ptr(m.vq.params), _ptr(enc), chunk, _ptr(nz), K,
                                                    _ptr(out), None, st), "dib_measure_symbolize")
    fused()
    k_ms = _median_ms(fused, 10, sync)
    rec["symbolize"] = {"points": a.points, "K": K, "seconds": round(t_sym, 3), "points_per_s": round(a.points / t_sym, 1),
                        "vq_tflops": round(a.points * K * vq_flop / t_sym / 1e12, 2),
                        "frac_of_fp32_mfma_peak": round(a.points * K * vq_flop / t_sym / 1e12 / PEAK_TFLOPS, 4),
                        "kernel_only": {"chunk": chunk, "ms": round(k_ms, 3), "points_per_s": round(chunk / k_ms * 1e3, 1),
                                        "vq_tflops": round(chunk * K * vq_flop / k_ms / 1e9, 2),
                                        "frac_of_fp32_mfma_peak": round(chunk * K * vq_flop / k_ms / 1e9 / PEAK_TFLOPS, 4)},
                        "vq_flop_per_point_draw": vq_flop, "symbol_fraction_1": float(sym.mean())}
    # ---- A/B on one chunk: fused kernel vs VQ DenseStack on [K * n, E] + torch.argmax ----------------
    n = 1 << 14
    enc_n = enc[:n]
    out_n = torch.empty(n, dtype=torch.uint8, device="cuda")
    fused_n = lambda: check(lib.dib_measure_symbolize(ctypes.byref(m._desc), _ptr(m.vq.params), _ptr(enc_n), n, _ptr(nz), K,
                                                      _ptr(out_n), None, st), "dib_measure_symbolize")
    res = {}

    def composed():
        mu, lv = enc_n[:, :E], enc_n[:, E:]
        z = (mu[None] + nz[:, None, :] * torch.exp(lv / 2.0)[None]).reshape(-1, E)
        lg = m.vq.forward(z)
        res["sym"] = (torch.argmax(lg.view(K, n, A), -1).float().mean(0) > 0.5).to(torch.uint8)

    fused_n(); composed()
    f_ms, c_ms = _median_ms(fused_n, 20, sync), _median_ms(composed, 20, sync)
    rec["ab_symbolize_chunk"] = {"points": n, "K": K, "fused_ms": round(f_ms, 4), "composed_ms": round(c_ms, 4),
                                 "speedup": round(c_ms / f_ms, 2),
                                 "symbols_differing": int((out_n != res["sym"]).sum()),
                                 "composed": "z = mu + noise sigma (torch), VQ DenseStack forward on [K * n, E] (grouped fp32 GEMMs), "
                                             "torch.argmax, mean > 0.5"}
    # ---- host characterisation ----------------------------------------------------------------
    t0 = time.perf_counter()
    ch = characterize_partition(sym, 2, seed=0)
    rec["characterize"] = {"seconds": round(time.perf_counter() - t0, 2), "sequence_length": int(len(sym)),
                           "windows": "15 log-spaced lengths 2e3 .. 2e6 x 5 draws", "entropy_rate_bits": round(ch["entropy_rate"], 4)}
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
