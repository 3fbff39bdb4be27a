"""DistributedIBEnsemble against R sequential DistributedIBNet engine steps, in one process on one MI355X, at
    the reference default   F = 10, B = 128, encoders [128, 128], E = 32, integration [256, 256], BCE from logits
    a tabular-sized shape   F = 64, B = 512, the same widths
for R = 1, 4 and 20: ms per lockstep step, ms per replica-step, the single model's ms per step (HipEngine.train_step with the
optimizer in its tail, default dispatch: that code's own best path), their ratio, library launches per step and the bytes
of the ensemble's state and step workspace.  Blocks of lockstep steps are interleaved with blocks of the R sequential steps; every
block is bracketed by a device synchronisation and preceded by warm-up steps; the figures are medians over the blocks and the
blocks themselves are kept (their spread is the noise floor).  Also timed, once per shape at R = 20: the gather + positional
encoding of all (replica, feature) by dib_ens_posenc_rows against the existing dib_positional_encoding_rows on x viewed as
[N F, d] with a device index tensor (built once, outside the timing).  One JSON line.

    python tools/dib_ensemble_bench.py [--steps 300] [--blocks 5] [--out profiles/dib_ensemble_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("reference default", 10, 128), ("tabular-sized", 64, 512)]
ARCH = dict(feature_encoder_architecture=[128, 128], integration_network_architecture=[256, 256], output_dimensionality=1,
            feature_embedding_dimension=32)


def _posenc_compare(ens, x, R, F, B, reps, torch):
    """us per call of the two ways to gather and encode a batch for every (replica, feature), same process, same data"""
    from dib_amd._gemm_plan import _ptr
    lib, st = ens.lib, ens._stream()
    rows = torch.randint(0, x.shape[0], (R, B), dtype=torch.int32, device=ens.device)
    pl = ens._plan(B)
    out = _ptr(pl["enc_ws"], pl["enc_off"]["a0"])
    idx = (rows.view(R, 1, B) * F + torch.arange(F, dtype=torch.int32, device=ens.device).view(1, F, 1)).reshape(-1).contiguous()
    xv = x.view(-1, ens.d)

    def timed(call):
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / reps

    new = timed(lambda: lib.dib_ens_posenc_rows(_ptr(x), x.stride(0), _ptr(rows), R, F, ens.d, ens.n_blocks, B, out, st))
    old = timed(lambda: lib.dib_positional_encoding_rows(_ptr(xv), xv.stride(0), _ptr(idx), R * F * B, ens.d, ens.n_blocks, out, st))
    return round(new, 2), round(old, 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4, 20])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dib_ensemble_bench.json"))
    a = ap.parse_args(argv)
    if a.blocks < 5:
        ap.error("--blocks: medians are taken over at least 5 block pairs")
    import torch
    import dib_amd
    from dib_amd.engine import HipEngine

    sync = torch.cuda.synchronize
    rec = {"workload": "DistributedIBNet Keras-path training step, Adam lr 3e-4, BCE from logits, beta 0.1",
           "protocol": f"per entry: {a.warmup} warm-up steps of both, then {a.blocks} blocks x {a.steps} lockstep steps interleaved with "
                       f"{a.blocks} blocks of R sequential HipEngine.train_step(optimizer=Adam) calls (reported per model-step); "
                       "synchronize around each block; medians, all blocks kept", "rows": [], "posenc_rows_at_R20_us": {}}
    N = 4096
    for name, F, B in SHAPES:
        rng = np.random.default_rng(F)
        x = rng.standard_normal((N, F)).astype(np.float32)
        y = (x[:, :1] * x[:, 1:2] > 0).astype(np.float32)
        for R in a.replicas:
            ens = dib_amd.DistributedIBEnsemble(R, [1] * F, **ARCH)
            opt = dib_amd.optimizers.Adam(3e-4)
            ens.compile(optimizer=opt, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True))
            ens.set_data(x, y)
            ens.set_beta(0.1)
            lib = ens.lib
            engines = [HipEngine([1] * F, **ARCH, init_seed=r) for r in range(R)]
            xd, yd = ens._x, ens._y
            for e in engines:
                e.set_beta(0.1)
                e.set_lr(3e-4)
            rows = torch.from_numpy(np.stack([rng.permutation(N)[:B] for _ in range(R)]).astype(np.int32)).to(ens.device)
            single_rows = [rows[r].contiguous() for r in range(R)]
            step = [0]

            def sequential():
                for r, e in enumerate(engines):
                    e.train_step(xd, yd, single_rows[r], 0, B, r, step[0], "bce_logits", inv_global_batch=1.0 / B, optimizer=opt)
                step[0] += 1

            for _ in range(a.warmup):
                ens._train(rows)
                sequential()
            sync()
            n0 = lib.dib_launch_count()
            ens._train(rows)
            launches = int(lib.dib_launch_count() - n0)
            n0 = lib.dib_launch_count()
            sequential()
            launches_single = (lib.dib_launch_count() - n0) / R
            ens_ms, base_ms = [], []
            for _ in range(a.blocks):
                sync()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ens._train(rows)
                sync()
                ens_ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
                nseq = max(1, a.steps // R)
                sync()
                t0 = time.perf_counter()
                for _ in range(nseq):
                    sequential()
                sync()
                base_ms.append((time.perf_counter() - t0) * 1e3 / nseq / R)
            e_ms, b_ms = float(np.median(ens_ms)), float(np.median(base_ms))
            assert np.isfinite(ens.get_flat_weights(R - 1)).all()
            rec["rows"].append({"shape": name, "features": F, "batch": B, "replicas": R, "ms_per_lockstep_step": round(e_ms, 4),
                                "ms_per_replica_step": round(e_ms / R, 4), "single_model_ms_per_step": round(b_ms, 4),
                                "replica_step_over_single_step": round(e_ms / R / b_ms, 4), "library_launches_per_step": launches,
                                "single_model_launches_per_step": round(float(launches_single), 2),
                                "workspace_bytes": ens.workspace_bytes(B),
                                "blocks_ms_per_replica_step": [round(v / R, 4) for v in ens_ms],
                                "blocks_single_model_ms_per_step": [round(v, 4) for v in base_ms]})
            if R == 20:
                new, old = _posenc_compare(ens, xd, R, F, B, 2000, torch)
                rec["posenc_rows_at_R20_us"][name] = {"dib_ens_posenc_rows": new, "dib_positional_encoding_rows": old}
            del ens, engines
            torch.cuda.empty_cache()
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
