"""Worker for tests/test_gpu_grad_transforms.py: a small fit() under Adam + global_clipnorm + ExponentialDecay with 1, 2 and 3
gradient buckets; under torch.distributed.run it takes fit()'s RCCL data-parallel path, otherwise the single-process path (where
the number of buckets changes nothing)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(out_path, batch=2048):
    import torch.distributed as dist
    distributed = "RANK" in os.environ
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        lr = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(lr)
        dist.init_process_group("nccl", device_id=torch.device(f"cuda:{lr}"))
    import dib_amd
    rng = np.random.default_rng(0)
    n = 2 * batch + 1  # a tail batch of one row
    x = rng.standard_normal((n, 8)).astype(np.float32)
    y = (x[:, 0] * x[:, 1] > 0).astype(np.float32)
    out = {}
    for buckets in (1, 2, 3):
        model = dib_amd.DistributedIBNet([1] * 8, [128, 128], [256, 256], 1, noise_seed=1, shuffle_seed=2, init_seed=3)
        model.dp_buckets = buckets
        opt = dib_amd.optimizers.Adam(dib_amd.schedules.ExponentialDecay(1e-3, 2, 0.5))
        opt.global_clipnorm, opt.clipvalue = 0.05, 0.01   # attributes, as in optimizer_v2
        model.compile(optimizer=opt, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
        hist = model.fit(x, y, epochs=2, batch_size=batch, verbose=False)
        eng = model._ensure_engine()
        out[f"params{buckets}"] = model.get_flat_weights()
        out[f"lr{buckets}"] = eng.lr_dev.cpu().numpy()
        out[f"t{buckets}"] = eng.t_dev.cpu().numpy()
        out[f"ss{buckets}"] = eng.grad_transform().ss.cpu().numpy()
        for k, v in hist.history.items():
            out[f"{k}{buckets}"] = np.array(v)
    if not distributed or dist.get_rank() == 0:
        np.savez(out_path, **out)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    run(sys.argv[1])
