"""What DistributedIBNet.fit / evaluate (models.py) are made of: input handling, the engine's capabilities, the training step's
three protocols - chosen once per fit - and the evaluation pass.  Plain functions over the engine API (engine.HipEngine; the
checker engines of tests/ implement a part of it), no state of their own: what a fit changes lives in the model and the engine."""
import os

import numpy as np
import torch


def device_matrix(eng, a):
    """a float32 tensor already on the engine's device as the row-major matrix the kernels read - itself when it is one, no trip
    through the host - or None for anything else"""
    if not (isinstance(a, torch.Tensor) and a.device == eng.device and a.dtype == torch.float32):
        return None
    a = a.detach()
    return (a.view(-1, 1) if a.dim() == 1 else a).contiguous()


def host_rows(a) -> np.ndarray:
    """array-like -> float32 [N, d] on the host; a 1-D array is one column"""
    a = np.asarray(a, dtype=np.float32)
    return a[:, None] if a.ndim == 1 else a


def device_rows(eng, a) -> torch.Tensor:
    """fit / evaluate inputs as one float32 [N, d] device tensor: a table already on the device (tabular.TabularPreprocessor) is
    used where it lies, anything else is uploaded once"""
    on_device = device_matrix(eng, a)
    return on_device if on_device is not None else eng.to_device(host_rows(a))


def parse_track_information(eng, track_information, validation_inputs):
    """fit(track_information=...) checked and completed: None, or the dict with `x` on the device (default: the validation
    inputs) and `every` a positive int"""
    if track_information is None:
        return None
    track = dict(track_information)
    unknown = set(track) - {"x", "every", "evaluation_batch_size", "number_evaluation_batches"}
    if unknown:
        raise ValueError(f"track_information: unknown keys {sorted(unknown)}")
    if track.get("x") is not None:
        track["x"] = device_rows(eng, track["x"])
    elif validation_inputs is not None:
        track["x"] = validation_inputs
    else:
        raise ValueError("track_information needs inputs: give it `x` or fit(validation_data=...)")
    track["every"] = int(track.get("every", 1))
    if track["every"] < 1:
        raise ValueError("track_information['every'] must be a positive number of epochs")
    return track


def epoch_order(eng, n, shuffle, shuffle_seed, epoch):
    """row order of `epoch` on the device (int32): Keras reshuffles every epoch; seeded by (shuffle_seed, epoch)"""
    order = (np.random.default_rng([shuffle_seed, epoch]).permutation(n) if shuffle else np.arange(n)).astype(np.int32)
    return eng.to_device(order, dtype=torch.int32)


def bind_optimizer(eng, opt) -> bool:
    """Hands the optimizer to the engine, or refuses what the engine cannot run (the checker engines of tests/ know Adam and plain
    SGD at a constant rate); returns whether the engine can capture the step as a graph."""
    if hasattr(eng, "set_optimizer"):
        eng.set_optimizer(opt)   # a change of rule re-initialises the optimizer state; the same rule: nothing
    elif not opt.native:
        raise ValueError(f"optimizer {opt.name!r} needs the HIP engine (include/dib_optimizers.h)")
    if not hasattr(eng, "apply_lr") and (opt.clip() is not None or opt.lr_schedule() is not None):
        raise ValueError("gradient clipping, decay and learning-rate schedules need the HIP engine (include/dib_grad_transform.h)")
    return hasattr(eng, "capture_step_graph")


def sync_noise_step(eng, value) -> None:
    """the device-resident noise step counter of an engine that keys its noise by one (enable_step_counter) := value"""
    if getattr(eng, "step_dev", None) is not None:
        eng.set_step_counter(value)


def set_lr(eng, opt) -> None:
    """the next step's learning rate on the device: a constant (free when unchanged), `decay` or a schedule (HipEngine.apply_lr)"""
    if opt.lr_schedule() is None:
        eng.set_lr(opt.learning_rate)
    else:
        eng.apply_lr(opt)


def choose_step(model, eng, xd, yd, bs, epochs, kind, dist, rank, world, can_capture, graphs):
    """The step of this fit, `step(order_dev, s0, gb)`: global batch rows order_dev[s0: s0 + gb] - forward, backward, the
    collectives, the optimizer, the History sums, model._step += 1.  Nothing it is chosen by changes during a fit.  A captured
    step is left in `graphs` for the caller to release."""
    opt, seed = model.optimizer, model.noise_seed

    def end_step(counter_bumped=False):
        model._step += 1
        if not counter_bumped:
            sync_noise_step(eng, model._step)   # eager step under the device counter: keep it in sync

    def single_step(order_dev, s0, gb):
        # one process: the step's LAST launch reduces the gradient partials, sums the KL / loss partials, accumulates the History
        # metrics and applies the optimizer (csrc/dib_tail.h) - or the engine steps an optimizer that does not ride there right
        # behind it
        set_lr(eng, opt)
        eng.train_step(xd, yd, order_dev[s0: s0 + gb], 0, gb, seed, model._step, kind, inv_global_batch=1.0 / gb, optimizer=opt)
        end_step()

    def replay_step(order_dev, s0, gb):
        if gb != bs:   # the graph holds full batches: the partial last one runs eagerly
            return single_step(order_dev, s0, gb)
        g, stage = graphs["train"]
        set_lr(eng, opt)
        stage.copy_(order_dev[s0: s0 + bs])
        g.replay()  # fwd + loss + bwd + optimizer + metrics + step-counter bump
        end_step(counter_bumped=True)

    def data_parallel_step(order_dev, s0, gb):
        lo, hi = (gb * rank) // world, (gb * (rank + 1)) // world   # this rank's rows of the global batch
        # Every rank issues the SAME collectives every step, rows or no rows (a tail batch with fewer rows than ranks leaves some
        # ranks empty: they contribute zeros).  Gradient buckets of the layer-major flat buffer, each all-reduced
        # (RCCL, async) as soon as it is final:
        #   1 integration network   - under the whole encoder-bank backward
        #   2 encoder front layers  - under the last encoder layer's weight gradient      (dp_buckets == 3)
        #   3 last encoder layer    - the only exposed one                                (dp_buckets == 3)
        #   0 = 2 + 3 as one bucket after the backward                                    (dp_buckets == 2)
        pending = []
        nb = model.dp_buckets
        if nb > 1 and gb // world <= model.dp_small_batch_rows:
            # small per-rank batches (<= 1024 rows: a handful of kernels per step, one grouped launch for every weight
            # gradient): the backward is a handful of launches with nothing to hide an all-reduce under - one bucket after it,
            # and the launches (hence the bits) of the single-process step.  Decided from the GLOBAL batch: identical on every
            # rank - and per batch: the partial last one may fall under the threshold.
            nb = 1
        issue = lambda g: pending.append(dist.all_reduce(g, async_op=True))
        if hi > lo:
            eng.train_step(xd, yd, order_dev[s0 + lo: s0 + hi], 0, hi - lo, seed, model._step, kind, inv_global_batch=1.0 / gb,
                           on_integration_grads_ready=issue if nb >= 2 else None,
                           **(dict(on_encoder_front_grads_ready=issue) if nb == 3 else {}))
        else:
            eng.grads.zero_()
            for part in ((1,) if nb == 2 else (1, 2) if nb == 3 else ()):
                off, cnt = eng.part_range(part)
                issue(eng.grads[off: off + cnt])
        if nb >= 2:
            off, cnt = eng.part_range(3 if nb == 3 else 0)
            issue(eng.grads[off: off + cnt])
            # each bucket is stepped as soon as ITS all-reduce has landed: buckets 1 (and 2) are updated on the compute stream
            # while the last bucket is still on the wire; every launch reads the same Adam step count, the last one advances it
            set_lr(eng, opt)
            parts = (1, 2, 3) if nb == 3 else (1, 0)
            for k, (w, part) in enumerate(zip(pending, parts)):
                w.wait()
                eng.optimizer_step_part(max(hi - lo, 1), part, opt, bump=k == len(parts) - 1)
        else:
            dist.all_reduce(eng.grads)
            set_lr(eng, opt)
            eng.optimizer_step(opt)
        end_step()

    # Optional hipGraph replay of the whole step (DIB_ENABLE_GRAPHS=1; needs the device-resident noise step counter;
    # single-process only).  Bit-identical to the eager launch sequence (tests).  OFF by default: measured on MI355X for the
    # reference's default Boolean-circuit run (B = 128, ~30 launches/step) the replay is ~8 % SLOWER than eager (4.09 vs 3.76
    # ms/epoch, tools/small_batch_bench.py) - the step is bound by the latency of its dependent kernels, not by launch overhead.
    # (The rules of include/dib_optimizers.h and every step behind a gradient transform always run eagerly: their step is not
    # part of capture_step_graph; a schedule alone keeps the captured step - its one-thread launch goes ahead of each replay.)
    use_graphs = (dist is None and can_capture and bs <= 8192 and (xd.shape[0] // bs) * epochs >= 64 and opt.rides_in_tail
                  and os.environ.get("DIB_ENABLE_GRAPHS", "0") == "1")
    if not use_graphs:
        sync_noise_step(eng, model._step)
        return single_step if dist is None else data_parallel_step
    eng.enable_step_counter(model._step)
    set_lr(eng, opt)
    graphs["train"] = eng.capture_step_graph(xd, yd, bs, kind, 1.0 / bs, seed, True, opt)
    eng.set_step_counter(model._step)
    return replay_step


def evaluation_pass(eng, xd, yd, bs, kind, noise_seed, noise_step, merge_rows, rank, world, metrics_acc) -> int:
    """Every row of (xd, yd) through eval_step in batches of `bs` under ONE noise key; the History sums go to `metrics_acc` (None:
    the engine's training accumulator).  Returns the number of steps (batches) to average the per-step quantities over.

    Evaluation batches do not depend on each other - no state changes between them, one noise key per pass (rows keyed by their
    dataset index) - and every History quantity is linear in per-row sums: k full batches are evaluated as ONE launch set of
    k * bs <= merge_rows rows with the per-batch 1 / bs scaling and counted as k steps.  Same per-row numbers, sums in another
    order (fp32 rounding).  At the reference's default (8 validation batches of 128 rows per epoch, train.py:30-34) that is 3
    launches per epoch instead of 24.  A partial batch is never merged.  Under data parallelism (world > 1) batches stay single
    and each is split row-wise like a training batch; a rank without rows launches nothing."""
    kmerge = max(1, merge_rows // bs) if world == 1 else 1
    n, s0, steps = xd.shape[0], 0, 0
    while s0 < n:
        gb = min(bs, n - s0)
        nb = min(kmerge, (n - s0) // bs) if gb == bs else 1
        rows = gb * nb
        lo, hi = (rows * rank) // world, (rows * (rank + 1)) // world
        if hi > lo:
            eng.eval_step(xd, yd, None, s0 + lo, hi - lo, noise_seed, noise_step, kind, inv_global_batch=1.0 / gb,
                          metrics_acc=metrics_acc)
        steps += nb
        s0 += rows
    return steps


def reduce_metrics(eng, dist, sums: np.ndarray) -> np.ndarray:
    """the History sums of all ranks (one all-reduce; the single process: as they are)"""
    if dist is None:
        return sums
    t = torch.from_numpy(sums.copy()).to(eng.metrics_acc.device)
    dist.all_reduce(t)
    return t.cpu().numpy()
