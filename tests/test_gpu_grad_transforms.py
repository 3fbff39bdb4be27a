"""GPU: gradient clipping and learning-rate schedules (include/dib_grad_transform.h, csrc/dib_grad_transform.h) from the C ABI up
to compile / fit, the one-rank bucket protocol, the custom InfoNCE loop and the training script.

The reference is tests/_oracle_grad_transforms.py in float64 - a restatement of the header's statement, not an executed
TensorFlow.  The tolerance is the project's rule (tests/test_gpu_optimizers.py): the same restatement in float32 on the same
inputs measures what the number format costs, the test allows 4 times that and never less than one float32 ulp of the compared
scale; nothing is taken from the device.  tests/test_grad_transforms_host.py prints those figures on the CPU and shows that the
inputs tell the modes (and a norm that ignored grad_scale) apart by more than 100 bounds."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dib_oracle as orc
import _oracle_grad_transforms as og
import _oracle_optimizers as oo
from _helpers import SPECS, dispatch_path, flat_to_params, params_to_flat, spec_kwargs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PAD = 64
CANARY = 12345.5
NONE, NORM, GLOBAL = 0, 1, 2


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, copy=True)).to("cuda", dtype=dtype)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buffer:
    """one gradient buffer with a variable table on the device; grads, tile partials and ss are each followed by PAD canaries"""

    def __init__(self, flat, segments, extra_ss=0):
        from dib_amd import _lib
        self.lib, self.n = _lib.load_library(), int(flat.size)
        self.host = _lib.HostGradTable([o for o, _ in segments], [c for _, c in segments], self.n)
        self.table, self._keep = self.host.upload("cuda")
        self.g = torch.full((self.n + PAD,), CANARY, dtype=torch.float32, device="cuda")
        self.g[:self.n] = _dev(flat)
        self.partials = torch.full((self.host.n_tiles + PAD,), CANARY, dtype=torch.float64, device="cuda")
        self.n_ss = self.host.n_segments + extra_ss
        self.ss = torch.full((self.n_ss + PAD,), CANARY, dtype=torch.float64, device="cuda")

    def sumsq(self, gs=1.0, cv=0.0, first=0, count=None, g=None):
        return self.lib.dib_grad_sumsq(ctypes.byref(self.table), first, self.host.n_segments if count is None else count,
                                       _ptr(self.g if g is None else g), gs, cv, _ptr(self.partials), _ptr(self.ss), _stream())

    def apply(self, mode, c, gs=1.0, cv=0.0, first=0, count=None, g=None):
        return self.lib.dib_grad_clip_apply(ctypes.byref(self.table), first, self.host.n_segments if count is None else count,
                                            _ptr(self.g if g is None else g), gs, cv, mode, c, _ptr(self.ss), _ptr(self.ss),
                                            self.n_ss, _stream())

    def run(self, gs=1.0, clipvalue=None, clipnorm=None, global_clipnorm=None):
        cv = clipvalue or 0.0
        mode, c = (NORM, clipnorm) if clipnorm else (GLOBAL, global_clipnorm) if global_clipnorm else (NONE, 0.0)
        if mode != NONE:
            assert self.sumsq(gs, cv) == 0
        assert self.apply(mode, c, gs, cv) == 0

    def grads(self):
        torch.cuda.synchronize()
        return self.g[:self.n].cpu().numpy()

    def canaries_intact(self):
        return all(bool((b[k:] == CANARY).all().item()) for b, k in ((self.g, self.n), (self.partials, self.host.n_tiles),
                                                                     (self.ss, self.n_ss)))


# ---- the kernels across their envelope -------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("mode", sorted(og.MODES))
def test_envelope_matches_the_float64_restatement(mode, grad_scale):
    """segments of 1 ... 70 001 elements around the tile size, starts of every residue mod 4, per-segment scales 0 / 1e-4 / 1 / 30"""
    flat, segments, gaps = og.envelope()
    want, ss64, bound = og.envelope_reference(mode, grad_scale)
    b = Buffer(flat, segments)
    n0 = b.lib.dib_launch_count()
    b.run(grad_scale, **og.MODES[mode])
    assert b.lib.dib_launch_count() - n0 == (1 if mode == "clipvalue" else 3)
    got = b.grads()
    if mode != "clipvalue":
        ss = b.ss[:len(segments)].cpu().numpy()
        ss64 = og.sumsq_of_float32_products(flat, segments, grad_scale, og.MODES[mode].get("clipvalue"))
        rel = np.abs(ss - ss64) / np.maximum(ss64, 1e-300)
        print(f"{mode} grad_scale {grad_scale:.3g}: ss max relative error {rel.max():.3g}")
        assert (rel <= 1e-12).all(), rel
        assert all(ss[k] == 0.0 for k, sc in enumerate(og.SCALES) if sc == 0.0)
    live = ~gaps
    err = float(np.abs(got[live] - want[live]).max())
    print(f"{mode} grad_scale {grad_scale:.3g}: max |device - float64| {err:.3g} (bound {bound:.3g})")
    assert err <= bound, (mode, grad_scale, err, bound)
    for (o, n), sc in zip(segments, og.SCALES):
        if sc == 0.0:
            assert got[o:o + n].view(np.uint32).max() == 0, "an exactly-zero gradient stays bit-zero"
    assert (got[gaps] == og.GAP_MARK).all(), "the elements of no variable are neither read nor written"
    assert b.canaries_intact()


# ragged [1, 2, 1] features with output_dimensionality 1 (a one-element bias); the smallest entry; widths 17 / 9 / 13 / 3: biases
# of feature f start at o + 17 f, off the 16-byte grid
@pytest.mark.parametrize("name", ["fused_leaky", "no_hidden", "odd_shapes_tanh"])
def test_real_layouts(name):
    from dib_amd import optimizers as O
    from dib_amd.engine import HipEngine
    spec = SPECS[name]
    eng = HipEngine(**spec_kwargs(spec), init_seed=1)
    segments = [(b["offset"], b["rows"] * b["cols"]) for b in eng.blocks]
    assert min(c for _, c in segments) == (3 if name == "odd_shapes_tanh" else 1)
    assert (name != "odd_shapes_tanh") or {o % 4 for o, _ in segments} == {0, 1, 2}   # (the envelope test has all four)
    rng = np.random.default_rng(5)
    flat = (rng.standard_normal(eng.grads.numel()) * 10.0 ** rng.uniform(-3, 1, eng.grads.numel())).astype(np.float32)
    gaps = np.ones(flat.size, dtype=bool)
    for o, c in segments:
        gaps[o:o + c] = False
    for opt, kw in ((O.build(O.Adam, clipvalue=2.0, global_clipnorm=3.0), dict(clipvalue=2.0, global_clipnorm=3.0)),
                    (O.build(O.RMSprop, clipnorm=0.5), dict(clipnorm=0.5))):
        eng.grads.copy_(_dev(flat))
        eng.transform_gradients(opt, grad_scale=1.0 / 3.0)
        torch.cuda.synchronize()
        got = eng.get_flat_grads()
        want, ss64 = og.transform(flat, segments, 1.0 / 3.0, **kw)
        g32, _ = og.transform(flat, segments, 1.0 / 3.0, dtype=np.float32, **kw)
        bound = og.bound(want[~gaps], g32[~gaps])
        err = float(np.abs(got[~gaps] - want[~gaps]).max())
        print(f"{name} {kw}: max |device - float64| {err:.3g} (bound {bound:.3g})")
        assert err <= bound
        ss = eng.grad_transform().ss.cpu().numpy()
        ss64 = og.sumsq_of_float32_products(flat, segments, 1.0 / 3.0, kw.get("clipvalue"))
        assert (np.abs(ss - ss64) <= 1e-12 * ss64).all()
        assert np.array_equal(got[gaps], flat[gaps])
        assert np.abs(want[~gaps] - flat[~gaps].astype(np.float64) / 3.0).max() > 100 * bound   # the clip was active


def test_buckets_in_any_order_give_the_bits_of_the_whole_buffer():
    """the data-parallel protocol reduces a bucket as it lands: sums of squares per bucket in landing order 1, 2, 3 and in the
    reverse order, then the apply, are the whole-buffer calls bit for bit; so is the engine's per-bucket entry point"""
    from dib_amd import optimizers as O
    from dib_amd.engine import HipEngine
    spec = SPECS["boolean4_32x32"]
    eng = HipEngine(**spec_kwargs(spec), init_seed=3)
    gt = eng.grad_transform()
    rng = np.random.default_rng(9)
    flat = _dev((rng.standard_normal(eng.grads.numel()) * 10.0 ** rng.uniform(-3, 0, eng.grads.numel())).astype(np.float32))
    flat[eng.n_params:] = 0.0   # the allocation's padding to 4 floats is no parameter: no backward writes it (the tail's float4 pass reads it)
    for clip in ((0.05, GLOBAL, 0.7), (0.0, NORM, 0.2)):
        eng.grads.copy_(flat)
        gt.ss.fill_(-1.0)
        gt.sumsq(clip, None, 0.5)
        gt.apply(clip, None, 0.5)
        torch.cuda.synchronize()
        whole, ss_whole = eng.grads.clone(), gt.ss.clone()
        assert not torch.equal(whole, flat * 0.5) and float(ss_whole.min().item()) >= 0.0
        for order in ((1, 2, 3), (3, 2, 1), (1, 0)):
            eng.grads.copy_(flat)
            gt.ss.fill_(-1.0)
            gt.partials.fill_(-1.0)
            for part in order:
                gt.sumsq(clip, eng.part_segments(part), 0.5)
                if clip[1] == NORM:
                    gt.apply(clip, eng.part_segments(part), 0.5)
            if clip[1] == GLOBAL:
                for part in reversed(order):
                    gt.apply(clip, eng.part_segments(part), 0.5)
            torch.cuda.synchronize()
            assert torch.equal(gt.ss, ss_whole) and torch.equal(eng.grads, whole), (clip, order)
    # optimizer_step_part (what fit calls per landed bucket) against optimizer_step, two steps
    a, b = (HipEngine(**spec_kwargs(spec), init_seed=3) for _ in range(2))
    for opt in (O.build(O.Adam, 1e-2, global_clipnorm=0.7, clipvalue=0.05), O.build(O.RMSprop, 1e-2, clipnorm=0.2),
                O.build(O.SGD, 1e-2, clipvalue=0.05)):
        for step in range(2):
            for e in (a, b):
                e.set_optimizer(opt)
                e.set_lr(1e-2)
                e.grads.copy_(flat * (step + 1))
            a.optimizer_step(opt)
            for k, part in enumerate((1, 2, 3)):
                b.optimizer_step_part(16, part, opt, bump=k == 2)
            torch.cuda.synchronize()
            for name in ("params", "grads", "adam_m", "adam_v", "t_dev"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (opt.name, step, name)


def test_two_buffers_sharing_one_ss_array_take_the_norm_of_their_union():
    flat, segments, gaps = og.envelope()
    rng = np.random.default_rng(3)
    other = (rng.standard_normal(5000) * 20.0).astype(np.float32)
    other_segments = [(0, 4097), (4100, 900)]
    nx = len(segments)
    a, b = Buffer(flat, segments, extra_ss=2), Buffer(other, other_segments)
    ss_all = a.ss
    c = og.GLOBAL_CLIPNORM
    assert a.sumsq() == 0
    assert b.lib.dib_grad_sumsq(ctypes.byref(b.table), 0, 2, _ptr(b.g), 1.0, 0.0, _ptr(b.partials), _ptr(ss_all[nx:]), _stream()) == 0
    assert a.apply(GLOBAL, c) == 0
    assert b.lib.dib_grad_clip_apply(ctypes.byref(b.table), 0, 2, _ptr(b.g), 1.0, 0.0, GLOBAL, c, None, _ptr(ss_all), nx + 2,
                                     _stream()) == 0
    union = np.concatenate([flat, other])
    union_segments = list(segments) + [(o + flat.size, n) for o, n in other_segments]
    live = np.concatenate([~gaps, np.array([True] * 4097 + [False] * 3 + [True] * 900)])
    want, ss64 = og.transform(union, union_segments, global_clipnorm=c)
    g32, _ = og.transform(union, union_segments, global_clipnorm=c, dtype=np.float32)
    alone, _ = og.transform(flat, segments, global_clipnorm=c)
    bound = og.bound(want[live], g32[live])
    got = np.concatenate([a.grads(), b.grads()])
    assert np.abs(got[live] - want[live]).max() <= bound
    assert np.abs(alone[~gaps] - want[:flat.size][~gaps]).max() > 100 * bound     # the other buffer's share of the norm counts
    assert (np.abs(ss_all[:nx + 2].cpu().numpy() - ss64) <= 1e-12 * ss64).all()
    assert np.array_equal(got[~live], union[~live]) and a.canaries_intact() and b.canaries_intact()


# ---- the learning rate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(og.lr_cases()))
def test_learning_rate_on_the_device(case):
    from dib_amd import _lib, optimizers as O
    from dib_amd.grad_transform import eval_lr
    want, _, bound = og.lr_reference(case)
    sched = og.make_schedule(case)
    opt = O.build(O.SGD, learning_rate=sched["lr"], decay=sched["decay"]) if isinstance(sched, dict) else O.Adam(learning_rate=sched)
    lib = _lib.load_library()
    t = torch.zeros(1, dtype=torch.int64, device="cuda")
    lr = torch.full((1 + PAD,), CANARY, dtype=torch.float32, device="cuda")
    got = []
    n0 = lib.dib_launch_count()
    for step in og.LR_STEPS:
        t.fill_(step)
        eval_lr(lib, opt.lr_schedule(), t, lr, _stream())
        got.append(float(lr[0].item()))
    assert lib.dib_launch_count() - n0 == len(og.LR_STEPS)
    err = float(np.abs(np.array(got, dtype=np.float64) - want).max())
    print(f"{case}: device {got}; max |device - float64| {err:.3g} (bound {bound:.3g})")
    assert err <= bound, (case, got, want)
    assert bool((lr[1:] == CANARY).all().item()) and int(t.item()) == og.LR_STEPS[-1]


# ---- whole steps -----------------------------------------------------------------------------------------------------------
N = 4099
STEP_SEGMENTS = ((0, 1000), (1001, 7), (1008, 3091))   # element 1000 belongs to no variable
STEP_CASES = {
    "adam_global_clipnorm": (oo.Rule("adam"), dict(global_clipnorm=5.0), None),
    "rmsprop_clipnorm": (oo.Rule("rmsprop"), dict(clipnorm=3.0), None),
    "sgd_momentum_clipvalue_decay": (oo.Rule("sgd", momentum=0.9), dict(clipvalue=0.1), 0.25),
}
LR0 = 1e-2


def _lr_of_step(decay):
    return (lambda k, dtype: og.lr(dict(kind="decay", lr=LR0, decay=decay), k, dtype)) if decay else (lambda k, dtype: LR0)


class Stepper:
    """parameters, gradients, state, lr and t of one flat buffer; one step = [schedule] + transform + rule [+ advance]"""

    def __init__(self, case):
        from dib_amd import _lib, optimizers as O
        rule, clip, decay = STEP_CASES[case]
        self.opt = O.build({"adam": O.Adam, "rmsprop": O.RMSprop, "sgd": O.SGD}[rule.name], learning_rate=LR0, **rule.h, **clip,
                           **(dict(decay=decay) if decay else {}))
        w0, g, _, _ = oo.inputs(N, 0, oo.STEPS)
        self.src = g
        self.buf = Buffer(np.zeros(N, np.float32), STEP_SEGMENTS)
        self.lib = self.buf.lib
        pad = lambda: torch.full((N + PAD,), CANARY, dtype=torch.float32, device="cuda")
        self.w = pad()
        self.w[:N] = _dev(w0)
        self.slots = [pad() for _ in range(max(2, self.opt.slots()))]
        for s in self.slots:
            s[:N] = 0.0
        self.lr = torch.full((1,), LR0, dtype=torch.float32, device="cuda")
        self.t = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.hyper = _lib.OptimizerHyper(**self.opt.hyper())
        self.staged = torch.zeros(N, dtype=torch.float32, device="cuda")

    def step(self):
        from dib_amd.grad_transform import eval_lr
        o, b = self.opt, self.buf
        b.g[:N].copy_(self.staged)
        if o.lr_schedule() is not None:
            eval_lr(self.lib, o.lr_schedule(), self.t, self.lr, _stream())
        cv, mode, c = o.clip()
        if mode != NONE:
            assert b.sumsq(1.0, cv) == 0
        assert b.apply(mode, c, 1.0, cv) == 0
        if o.name == "adam":
            rc = self.lib.dib_adam_step(_ptr(self.w), _ptr(b.g), _ptr(self.slots[0]), _ptr(self.slots[1]), N, _ptr(self.lr),
                                        _ptr(self.t), o.beta_1, o.beta_2, o.epsilon, 1.0, _stream())
            assert rc == 0
            return
        s = [self.slots[k] if k < o.slots() else None for k in range(3)]
        assert self.lib.dib_optimizer_step(o.kind, ctypes.byref(self.hyper), _ptr(self.w), _ptr(b.g), *(_ptr(x) for x in s), N,
                                           _ptr(self.lr), _ptr(self.t), None, 1.0, _stream()) == 0
        assert self.lib.dib_optimizer_advance(o.kind, ctypes.byref(self.hyper), _ptr(self.t), None, _stream()) == 0

    def state(self):
        torch.cuda.synchronize()
        return self.w[:N].cpu().numpy(), [s[:N].cpu().numpy() for s in self.slots[:max(self.opt.slots(), 2 if self.opt.name == "adam" else 0)]]


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_eight_steps_with_the_rules_match_the_composed_restatement(case):
    rule, clip, decay = STEP_CASES[case]
    w0, g, zero, _ = oo.inputs(N, 0, oo.STEPS)
    w64, s64 = og.stepped(rule, _lr_of_step(decay), oo.STEPS, w0, g, STEP_SEGMENTS, np.float64, **clip)
    w32, s32 = og.stepped(rule, _lr_of_step(decay), oo.STEPS, w0, g, STEP_SEGMENTS, np.float32, **clip)
    plain64, _ = og.stepped(rule, _lr_of_step(decay), oo.STEPS, w0, g, STEP_SEGMENTS, np.float64)
    bw = max(og.FACTOR * float(np.abs(w32 - w64).max()), og.ULP)
    f = Stepper(case)
    for k in range(oo.STEPS):
        f.staged.copy_(_dev(g[k]))
        f.step()
    w, slots = f.state()
    err = float(np.abs(w - w64).max())
    print(f"{case}: parameters max |device - float64| {err:.3g} (bound {bw:.3g})")
    assert err <= bw
    assert np.abs(plain64 - w64).max() > 100 * bw, "the transform must matter on these inputs"
    assert len(slots) == len(s64)
    for k, (a, b64, b32) in enumerate(zip(slots, s64, s32)):
        scale = max(np.abs(b64).max(), 1e-300)
        bound = max(og.FACTOR * float(np.abs(b32 - b64).max() / scale), og.ULP)
        rel = float(np.abs(a - b64).max() / scale)
        print(f"    slot {k}: relative error {rel:.3g} (bound {bound:.3g})")
        assert rel <= bound
    assert np.array_equal(w[zero], w0[zero]) and int(f.t.item()) == oo.STEPS
    assert f.buf.canaries_intact() and all(bool((b[N:] == CANARY).all().item()) for b in [f.w] + f.slots)
    if decay:
        assert abs(float(f.lr.item()) - float(og.lr(dict(kind="decay", lr=LR0, decay=decay), oo.STEPS - 1))) <= 4 * og.ULP * LR0


def test_a_captured_step_replays_with_an_advancing_learning_rate():
    """schedule + transform + rule + advance captured once: one eager step and 4 replays are 5 eager steps bit for bit, and
    lr_dev differs from replay to replay (the schedule reads the device step count)"""
    case = "sgd_momentum_clipvalue_decay"
    _, g, _, _ = oo.inputs(N, 0, oo.STEPS)
    eager = Stepper(case)
    eager.staged.copy_(_dev(g[0]))
    for _ in range(5):
        eager.step()
    want = eager.state()
    f = Stepper(case)
    f.staged.copy_(_dev(g[0]))
    f.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        f.step()
    assert int(f.t.item()) == 1          # capture enqueues nothing
    lrs = [float(f.lr.item())]
    for _ in range(4):
        graph.replay()
        lrs.append(float(f.lr.item()))
    got = f.state()
    assert int(f.t.item()) == 5 and np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    assert len(set(lrs)) == 5 and lrs == sorted(lrs, reverse=True), lrs
    assert float(eager.lr.item()) == lrs[-1]


def test_refused_calls_launch_nothing_and_write_nothing():
    flat, segments, _ = og.envelope()
    b = Buffer(flat, segments)
    before = [t.clone() for t in (b.g, b.partials, b.ss)]
    n0 = b.lib.dib_launch_count()
    nseg = len(segments)
    assert b.sumsq(g=b.g[1:]) == -1 and b.apply(NORM, 1.0, g=b.g[1:]) == -1            # 4 bytes off a 16-byte boundary
    assert b.sumsq(first=1, count=nseg) == -1 and b.apply(NORM, 1.0, first=-1) == -1 and b.sumsq(count=nseg + 1) == -1
    assert b.sumsq(cv=-1.0) == -1 and b.apply(NONE, 0.0, cv=0.0) == -1 and b.apply(NORM, 0.0) == -1 and b.apply(GLOBAL, -2.0) == -1
    assert b.apply(3, 1.0) == -1 and b.apply(NORM, float("nan")) == -1
    assert b.lib.dib_grad_sumsq(ctypes.byref(b.table), 0, nseg, _ptr(b.g), 1.0, 0.0, None, _ptr(b.ss), _stream()) == -1
    assert b.lib.dib_grad_clip_apply(ctypes.byref(b.table), 0, nseg, _ptr(b.g), 1.0, 0.0, GLOBAL, 1.0, None, None, nseg, _stream()) == -1
    assert b.sumsq(count=0) == 0 and b.apply(NORM, 1.0, first=nseg, count=0) == 0     # nothing to do: no launch
    torch.cuda.synchronize()
    assert b.lib.dib_launch_count() == n0
    assert all(torch.equal(x, y) for x, y in zip(before, (b.g, b.partials, b.ss)))
    assert b.sumsq() == 0 and b.apply(NORM, 1.0) == 0 and b.lib.dib_launch_count() == n0 + 3


# ---- model level ---------------------------------------------------------------------------------------------------------
FIT_LR = dict(kind="exponential", initial_learning_rate=3e-3, decay_steps=2, decay_rate=0.7)
FIT_CLIP = 0.5


def _oracle_fit(spec, blocks, w0, x, y, epochs, bs, beta, noise_seed, shuffle_seed):
    """oracle/dib_oracle.py fit (float64 gradients, flattened in the engine's layout) with global_clipnorm, the schedule and the
    float64 Adam of tests/_oracle_optimizers.py -> (History of loss / KL{f}, final flat parameters, clip factor per step)"""
    n, F, E = x.shape[0], spec.number_features, spec.feature_embedding_dimension
    segments = [(b["offset"], b["rows"] * b["cols"]) for b in blocks]
    w = np.asarray(w0, dtype=np.float64).copy()
    rule = oo.Rule("adam")
    st = rule.init(w.size, np.float64)
    hist, step, scales = {}, 0, []
    for epoch in range(epochs):
        order = orc.epoch_permutation(shuffle_seed, epoch, n)
        loss_sum, nseen, kl_steps = 0.0, 0, []
        for s0 in range(0, n, bs):
            rows = order[s0:s0 + bs]
            p = flat_to_params(blocks, w, spec)
            c = orc.forward(spec, p, x[rows].astype(np.float64), orc.philox_normal_all(noise_seed, step, rows, F, E))
            task, grads, _ = orc.backward(spec, p, x[rows].astype(np.float64), y[rows], c, beta, "bce_logits")
            g, ss = og.transform(params_to_flat(blocks, grads, w.size, dtype=np.float64), segments, global_clipnorm=FIT_CLIP)
            scales.append(og.global_scale(ss.sum(), FIT_CLIP))
            rule.step(w, g, st, float(og.lr(FIT_LR, step)))
            loss_sum += (task + beta * float(c.kl.sum())) * len(rows)
            nseen += len(rows)
            kl_steps.append(c.kl.copy())
            step += 1
        hist.setdefault("loss", []).append(loss_sum / nseen)
        for f, v in enumerate(np.mean(kl_steps, axis=0)):
            hist.setdefault(f"KL{f}", []).append(float(v))
    return hist, w, scales


@pytest.mark.parametrize("path", ["default", "grouped_gemm"])
def test_fit_with_global_clipnorm_and_exponential_decay_matches_the_float64_oracle_fit(path):
    """compile(optimizer=Adam(ExponentialDecay) with global_clipnorm set) + 6 fit steps at B = 16 on the small Boolean zoo entry, on the
    row-tile kernels and on the grouped-GEMM path; the tolerance form of test_fit_with_rmsprop_matches_the_float64_oracle_fit"""
    import dib_amd
    spec = SPECS["boolean4_32x32"]
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)
    x, y = np.tile(x, (3, 1)).astype(np.float32), np.tile(y, 3).astype(np.float32)   # 48 rows: 3 steps per epoch
    with dispatch_path(path):
        model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        sched = dib_amd.schedules.ExponentialDecay(3e-3, 2, 0.7)
        model.compile(optimizer=dib_amd.optimizers.build(dib_amd.optimizers.Adam, sched, global_clipnorm=FIT_CLIP),
                      loss=dib_amd.losses.BinaryCrossentropy(from_logits=True))
        w0 = model.get_flat_weights()
        beta = float(model.beta.value())
        eng = model._ensure_engine()
        hist = model.fit(x, y, epochs=2, shuffle=True, batch_size=16, verbose=False)
        assert int(eng.t_dev.item()) == 6
        got_w = model.get_flat_weights()
        lr_last = float(eng.lr_dev.item())
    ref, w, scales = _oracle_fit(spec, model.param_blocks(), w0, x, y, 2, 16, beta, 4, 6)
    print("oracle clip factors per step:", np.round(scales, 4))
    assert sum(s < 1.0 for s in scales) >= len(scales) / 2, scales      # the threshold clips on at least half of the steps
    for k in ref:
        got, want = np.array(hist.history[k]), np.array(ref[k])
        tol = 1e-3 if "KL" in k else 2e-3
        assert np.abs(got - want).max() < tol * (1 + np.abs(want).max()), (k, got, want)
    n_params = eng.n_params
    assert np.abs(got_w[:n_params] - w[:n_params]).max() < 2e-3 * (1 + np.abs(w).max())
    assert abs(lr_last - float(og.lr(FIT_LR, 5))) <= 4 * og.ULP * 3e-3     # the last step ran at iterations = 5


def test_fit_infonce_with_clipnorm_matches_the_float64_loop_oracle():
    """fit_infonce(optimizer=get("adam", clipnorm=...)): 4 steps at B = 16; every variable of both networks is clipped to its own norm
    before the one Adam (the Y encoder's gradient is final before the clip: no fused sum-and-Adam launch)"""
    import dib_amd
    import infonce_loop_oracle as ilo
    from dib_amd import infonce
    from dib_amd.dense import DenseStack
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 8, feature_embedding_dimension=8)
    rng = np.random.default_rng(11)
    xt, yt = rng.standard_normal((32, 4)).astype(np.float32), rng.standard_normal((32, 3)).astype(np.float32)
    xv, yv = rng.standard_normal((16, 4)).astype(np.float32), rng.standard_normal((16, 3)).astype(np.float32)
    seed, lr, clipnorm = 3, 3e-3, 0.2   # between the median (0.11) and the upper quartile (0.49) of a variable's gradient norm in the float64 loop oracle
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=5, init_seed=seed)
    eng = model._ensure_engine()
    yenc = DenseStack(eng, 3, [32], 8, "relu", True, 5, seed=seed + 1)
    L = len(yenc.dims)
    p0 = flat_to_params(model.param_blocks(), model.get_flat_weights(), spec)
    y0 = ([yenc.kernel(l).cpu().numpy().astype(np.float64) for l in range(L)],
          [yenc.bias(l).cpu().numpy().astype(np.float64) for l in range(L)])
    kw = dict(batch_size=16, number_pretraining_epochs=1, number_annealing_epochs=2, beta_start=1e-3, beta_end=1e-2)
    got = infonce.fit_infonce(model, xt, yt, xv, yv, learning_rate=lr, similarity="l2", temperature=1.0, seed=seed,
                              output_encoder=yenc, optimizer=dib_amd.optimizers.get("adam", clipnorm=clipnorm), shared_dimensionality=8, **kw)
    assert int(eng.t_dev.item()) == int(yenc.t_dev.item()) == 4

    class ClipLoop(ilo.InfoNCELoopOracle):
        clipped = 0
        seen = 0

        def _adam(self, grads):   # every variable is one segment: (g * c) / max(||g||, c), then the oracle's own float64 Adam
            out = []
            for g in grads:
                flat, _ = og.transform(g.detach().numpy().reshape(-1), [(0, g.numel())], clipnorm=clipnorm)
                self.clipped += int(float(g.norm()) > clipnorm)
                self.seen += 1
                out.append(torch.from_numpy(flat).reshape(g.shape))
            super()._adam(out)

    o = ClipLoop(spec, p0, ilo.YEncoder(y0[0], y0[1], "relu", True, 5, dtype=torch.float64), "l2", 1.0, lr, noise_seed=5)
    want = o.fit(xt, yt, xv, yv, seed=seed, **kw)
    assert o.t == 4
    print(f"oracle: {o.clipped} of {o.seen} variable gradients were above the threshold")
    assert o.seen / 4 <= o.clipped <= 3 * o.seen / 4
    for k in ("kl", "kl_validation", "loss_infonce", "loss_infonce_validation"):
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        tol = 1e-3 if "kl" in k else 2e-3
        assert g.shape == w.shape and np.abs(g - w).max() < tol * (1 + np.abs(w).max()), (k, g, w)
    xs = [t for t in flat_to_params(model.param_blocks(), model.get_flat_weights(), spec).tensors()]
    yb = yenc.params.cpu().numpy()
    ys = []
    for l, (i, o_) in enumerate(yenc.dims):
        ys += [yb[yenc.w_off[l]: yenc.w_off[l] + i * o_].reshape(i, o_), yb[yenc.b_off[l]: yenc.b_off[l] + o_]]
    assert len(xs) + len(ys) == len(o.vars)
    for a, b in zip(xs + ys, o.vars):
        b = b.detach().numpy()
        assert np.abs(np.asarray(a).reshape(b.shape) - b).max() < 2e-3 * (1 + np.abs(b).max())


def test_train_script_runs_with_global_clipnorm(tmp_path):
    from dib_amd import train
    hist = train.main(["--dataset", "boolean_circuit", "--number_pretraining_epochs", "1", "--number_annealing_epochs", "1",
                       "--batch_size", "128", "--artifact_outdir", str(tmp_path), "--global_clipnorm", "1.0",
                       "--learning_rate_decay", "0.01", "--feature_encoder_architecture", "32", "32",
                       "--integration_network_architecture", "64", "--feature_embedding_dimension", "8"])
    assert len(hist.history["loss"]) == 2 and np.isfinite(hist.history["loss"]).all()
    opt = hist.model.optimizer
    assert opt.name == "adam" and opt.global_clipnorm == 1.0 and opt.decay == 0.01 and opt.learning_rate == 3e-4
    eng = hist.model._ensure_engine()
    t = int(eng.t_dev.item())
    assert t > 0 and abs(float(eng.lr_dev.item()) - 3e-4 / (1 + 0.01 * (t - 1))) < 1e-9


def test_unchanged_paths_keep_their_launches_and_their_bits():
    """without the new arguments Adam and plain SGD still end the step in the fused tail, with the same launch count; a schedule
    alone keeps the tail; a clip leaves it (tail without the update, transform launches, the rule).  A fit compiled without the
    new arguments is bit-identical to the same fit pushed through the transform route by a clipvalue that clips nothing."""
    import dib_amd
    from dib_amd import optimizers as O
    from dib_amd.engine import HipEngine
    spec = SPECS["boolean4_32x32"]
    eng = HipEngine(**spec_kwargs(spec), init_seed=0)
    rng = np.random.default_rng(0)
    B = 16
    x = eng.to_device(rng.standard_normal((B, 4)).astype(np.float32))
    y = eng.to_device((rng.random((B, 1)) > 0.5).astype(np.float32))
    eng.grad_transform()   # (the table's upload is not a launch of the library, and happens once)

    def launches(optimizer):
        n0 = eng.lib.dib_launch_count()
        eng.train_step(x, y, None, 0, B, 1, 0, "bce_logits", optimizer=optimizer)
        return eng.lib.dib_launch_count() - n0

    launches(None)
    base = launches(None)
    assert launches(("adam", 0.9, 0.999, 1e-7)) == base and launches(("sgd",)) == base
    assert launches(O.build(O.Adam, clipnorm=1.0)) == base + 3 + 2            # tile sums, segment sums, apply; dib_adam_step's two
    assert launches(O.build(O.Adam, global_clipnorm=1.0)) == base + 3 + 2
    assert launches(O.build(O.SGD, clipvalue=1.0)) == base + 1 + 1            # apply; dib_sgd_step
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
    for opt, tup in ((O.Adam(), "adam"), (O.Adam(dib_amd.schedules.CosineDecay(1e-3, 10)), "adam"), (O.build(O.SGD, decay=0.1), "sgd"),
                     (O.build(O.Adam, clipvalue=1.0), None)):   # (None: does not ride in the tail)
        model.compile(optimizer=opt, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True))
        assert model.optimizer.rides_in_tail == (tup is not None) and tup in (None, model.optimizer.name)
    xs, ys = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)
    xs, ys = np.tile(xs, (3, 1)).astype(np.float32), np.tile(ys, 3).astype(np.float32)
    out = []
    for kw in ({}, dict(clipvalue=1e30)):
        m = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        m.compile(optimizer=O.build(O.Adam, 3e-3, **kw), loss=dib_amd.losses.BinaryCrossentropy(from_logits=True))
        h = m.fit(xs, ys, epochs=2, shuffle=True, batch_size=16, verbose=False)
        e = m._ensure_engine()
        out.append((m.get_flat_weights(), e.adam_m.cpu().numpy(), e.adam_v.cpu().numpy(), np.array(h.history["loss"])))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.timeout(900)
def test_fit_with_global_clipnorm_under_rccl_one_rank_equals_single_process(tmp_path):
    """fit() under torch.distributed.run (nccl = RCCL, world size 1) with Adam + clipvalue + global_clipnorm + ExponentialDecay and
    1, 2 and 3 gradient buckets: each bucket's sums of squares as it lands, the apply and the per-bucket updates after the last
    - the bits of the plain single-process run, whatever the number of buckets.  (More than one rank cannot be run on one GPU.)"""
    a, b = str(tmp_path / "single.npz"), str(tmp_path / "rccl.npz")
    worker = os.path.join(HERE, "_dp_grad_transform_worker.py")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, worker, a], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
                        "127.0.0.1", "--master-port", port, worker, b], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    s, d = np.load(a), np.load(b)
    assert set(s.files) == set(d.files)
    assert int(s["t1"][0]) == 6 and float(s["lr1"][0]) < 1e-3 and float(s["ss1"].sum()) > 0.05 ** 2   # decayed, and the clip was active
    for k in s.files:
        assert np.array_equal(s[k], d[k]), k
    for k in ("params", "lr", "t", "loss"):
        assert np.array_equal(d[k + "1"], d[k + "2"]) and np.array_equal(d[k + "1"], d[k + "3"]), k
