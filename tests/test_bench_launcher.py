"""bench.py --gpus N must really start N ranks (round-1 verdict: it silently ran one).  CPU dry run over gloo: the same
re-exec-under-torch.distributed.run path the GPU run takes, stopping after the rendezvous + one all-reduce."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_gpus_flag_spawns_that_many_ranks():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run-backend", "gloo"],
                         capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out == {"dry_run": True, "n_gpus": 2, "ranks_joined": 2}


@pytest.mark.timeout(300)
def test_bench_refuses_world_size_mismatch():
    """Launched by a launcher with a different rank count than --gpus: refuse instead of printing a wrong n_gpus."""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run-backend", "gloo"],
                         capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert res.returncode != 0 and "WORLD_SIZE=1" in res.stderr


def test_flop_model_matches_survey():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.gemm_flops_per_sample(64) == 13141504   # SURVEY 8(a) totals, config 3
    assert bench.gemm_flops_per_sample(50) == 10353152   # config 4
    assert sum(bench.flops_by_kernel().values()) == 13141504


def test_plain_run_measures_the_headline_only_and_full_restores_the_rest():
    """A plain `bench.py --gpus 1 --steps K --warmup W` runs no kernel-timing block, no `extra` and no CPU baseline; `--full`
    turns all three back on, the `--no-*` switches still leave single parts out, and `--force-dp-extras` implies `--full`."""
    sys.path.insert(0, ROOT)
    import bench
    off = lambda a: (a.no_kernel_timing, a.no_extra, a.no_cpu_baseline)
    plain = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3"])
    assert not plain.full and off(plain) == (True, True, True)
    assert (plain.steps, plain.warmup, plain.blocks, plain.dump_outputs) == (20, 3, 3, None)
    full = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "3", "--full"])
    assert full.full and off(full) == (False, False, False)
    assert off(bench.parse_args(["--full", "--no-extra", "--no-cpu-baseline"])) == (False, True, True)
    assert off(bench.parse_args(["--full", "--no-kernel-timing"])) == (True, False, False)
    dp = bench.parse_args(["--force-dp-extras", "--only-dp-breakdown"])
    assert dp.full and off(dp) == (False, False, False)


@pytest.mark.parametrize("rank", [0, 1])
def test_multi_gpu_extras_deadline_prints_the_headline_and_every_rank_leaves(rank):
    """A collective that never completes inside a multi-GPU `extra` must not take the measured headline down: on expiry
    rank 0 prints the line assembled BEFORE the extras, every rank exits with status 0."""
    code = ("import sys, time; sys.path.insert(0, %r); import bench\n"
            "out = {'metric': 'm', 'value': 1.0}; extra = {'weak_scaling': {'value': 2.0}}\n"
            "d = bench._ExtrasDeadline(0.3, %d, out, extra); d.start()\n"
            "time.sleep(30)\n"          # the hung collective
            "print('not reached'); sys.exit(3)\n") % (ROOT, rank)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    if rank == 0:
        out = json.loads(lines[-1])
        assert out["metric"] == "m" and out["value"] == 1.0
        assert out["extra"]["weak_scaling"] == {"value": 2.0} and "did not finish" in out["extra"]["error"]
    else:
        assert lines == [] and "not reached" not in res.stdout


def test_multi_gpu_extras_deadline_cancelled_in_time_is_silent():
    sys.path.insert(0, ROOT)
    import bench
    import time
    out, extra = {"metric": "m"}, {}
    d = bench._ExtrasDeadline(0.5, 0, out, extra)
    d.start()
    d.cancel()
    time.sleep(0.8)
    assert "extra" not in out


def _bench_dp_worker(rank, world, port, out_dir, buckets, scaling):
    """one rank of the CPU run of bench.Workload's own data-parallel step (the code the driver's SCALE run executes), gloo"""
    import numpy as np
    import torch
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (ROOT, os.path.join(ROOT, "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    d = None
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        d = dist
    import bench
    import dib_oracle as orc
    from _helpers import spec_kwargs
    from _oracle_engine import OracleEngine
    F, gb = 8, 24      # (bench.synthetic's label uses the first 8 features)
    spec = orc.DIBSpec([1] * F, [8], [8], 1, feature_embedding_dimension=4)
    eng = OracleEngine(**spec_kwargs(spec), init_seed=0)
    wl = bench.Workload(F, "cpu", rank, world, d, scaling, gb if scaling == "strong" else gb // world, buckets, engine=eng,
                        n_rows=4 * gb)
    for i in range(4):
        wl.step(i)
    np.save(os.path.join(out_dir, f"p_{scaling}_w{world}_b{buckets}_r{rank}.npy"), eng.get_flat_params())
    if world > 1:
        # the scaling record's own breakdown: collective-free steps, every bucket's all-reduce alone, the three protocols -
        # every rank must get through it (same collectives in the same order on every rank) and report the same keys
        out = wl.dp_breakdown(2, "cpu")
        assert set(out["step_ms_by_protocol"]) == {"buckets_1", "buckets_2", "buckets_3"}
        assert set(out["all_reduce_alone"]) == {"integration", "encoder_front", "encoder_last", "encoder_bank", "all"}
        m, _ = wl.measure(1, 2, 2, "cpu")      # barrier + max-over-ranks timing blocks
        assert m > 0
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_bench_data_parallel_step_equals_single_process(tmp_path, world):
    """bench.Workload.step under 1 / 2 / 3 gradient buckets over gloo (world 2 and 3; strong scaling: rank r takes rows
    [r B / N, (r + 1) B / N) of each global batch - uneven shards at N = 3) leaves every rank with the parameters of the
    single-process step on the whole batch; dp_breakdown and the timed blocks complete on every rank.  Float64 test engine."""
    import socket
    import numpy as np
    import torch.multiprocessing as mp

    def port():
        s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
        return p

    _bench_dp_worker(0, 1, port(), str(tmp_path), 3, "strong")
    ref = np.load(tmp_path / "p_strong_w1_b3_r0.npy")
    for buckets in (1, 2, 3):
        mp.spawn(_bench_dp_worker, args=(world, port(), str(tmp_path), buckets, "strong"), nprocs=world, join=True)
        got = [np.load(tmp_path / f"p_strong_w{world}_b{buckets}_r{r}.npy") for r in range(world)]
        for g in got[1:]:
            assert np.array_equal(g, got[0])                      # every rank applied the same update
        assert np.abs(got[0] - ref).max() < 1e-9 * (1 + np.abs(ref).max()), buckets
    # weak scaling (every rank steps through its own batches): the ranks still end with one set of parameters
    mp.spawn(_bench_dp_worker, args=(world, port(), str(tmp_path), 3, "weak"), nprocs=world, join=True)
    got = [np.load(tmp_path / f"p_weak_w{world}_b3_r{r}.npy") for r in range(world)]
    assert all(np.array_equal(g, got[0]) for g in got[1:]) and np.isfinite(got[0]).all()


def test_dump_outputs_writes_the_last_steps_arrays_within_the_limit(tmp_path, monkeypatch):
    """bench.py --dump-outputs: after the timed steps the arrays of the last step land as DIR/<name>.npy, identical for two
    runs with the same arguments; past the size limit an array is replaced by a fixed, seeded sample.  Float64 test engine."""
    import numpy as np
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bench
    import dib_oracle as orc
    from _helpers import spec_kwargs
    from _oracle_engine import OracleEngine

    def run(out_dir):
        F, gb = 8, 24
        spec = orc.DIBSpec([1] * F, [8], [8], 1, feature_embedding_dimension=4)
        wl = bench.Workload(F, "cpu", 0, 1, None, "strong", gb, 3, engine=OracleEngine(**spec_kwargs(spec), init_seed=0),
                            n_rows=4 * gb)
        wl.measure(1, 2, 2, "cpu")
        return wl, bench.dump_outputs(wl, str(out_dir))

    wl, info = run(tmp_path / "a")
    assert set(info) == {"params", "grads", "step_out", "metrics"} and not any(v[2] for v in info.values())
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in info}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["params"], wl.eng.get_flat_params()) and got["params"].size == wl.eng.n_params
    assert got["grads"].size == wl.eng.n_params and np.abs(got["grads"]).max() > 0
    assert got["step_out"].shape == (wl.F + 3,) and got["metrics"].shape == (wl.F + 3,)
    _, info_b = run(tmp_path / "b")
    for k in info:
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy")), k
    # over the limit: the largest array is sampled down to what is left of the budget, the same elements every run
    small = 8 * (2 * (wl.F + 3) + wl.eng.n_params + 10)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", small)
    _, info_c = run(tmp_path / "c")
    _, _ = run(tmp_path / "d")
    sampled = [k for k, v in info_c.items() if v[2]]
    assert len(sampled) == 1 and sum(np.load(tmp_path / "c" / f"{k}.npy").nbytes for k in info_c) <= small
    k = sampled[0]
    assert np.array_equal(np.load(tmp_path / "c" / f"{k}.npy"), np.load(tmp_path / "d" / f"{k}.npy"))
    assert np.isin(np.load(tmp_path / "c" / f"{k}.npy"), got[k]).all()
