"""GPU: the Keras optimizer family on the flat buffer (include/dib_optimizers.h, csrc/dib_optimizers.h) from the C ABI up to
compile / fit, the custom InfoNCE loop and the training script.

The float64 comparison.  The reference is tests/_oracle_optimizers.py in float64.  The tolerance is NOT taken from the device:
the same restatement run in float32 on the same inputs measures what the number format costs, and the test allows FACTOR = 4
times that (fused multiply-add contraction, the device's sqrt / divide / powf rounding), never less than one float32 ulp of the
compared scale.  Measured on the CPU for n = 4099, 8 steps, parameters of unit scale (tests/test_optimizers_host.py prints them):
    max |float32 - float64| of the parameters: 4.5e-7 (SGD momentum) ... 7.3e-7 (Nadam) - the rounding of w itself dominates
    state slots, relative to the slot's largest value: 8e-8 ... 4.2e-7; Nadam's v: 1.3e-5 - float32 loses that much of
    1 - beta_2 = 0.001 (AMSGrad runs at beta_2 = 0.9 so that vhat differs from v: 2.4e-7)
so the asserted bounds are about 1.8e-6 ... 2.9e-6 on the parameters and 3e-7 ... 5e-5 on the slots.  test_optimizers_host.py
shows on the CPU that these inputs move the parameters by more than 1000 bounds, tell RMSprop's two epsilon placements apart and
tell every two rules apart by more than 100 bounds."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as orc
import _oracle_optimizers as oo
from _helpers import SPECS, dispatch_path, flat_to_params, params_to_flat, spec_kwargs

pytestmark = pytest.mark.gpu

CASES = sorted(oo.cases())
PAD = 64            # canary floats after every buffer
CANARY = 12345.5


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _dev(a):
    """a (possibly read-only, shared) NumPy array as a fresh CUDA tensor"""
    return torch.from_numpy(np.array(a, copy=True)).to("cuda")


def _make_optimizer(case, lr=None):
    """the optimizers.Optimizer of a case of tests/_oracle_optimizers.py cases()"""
    from dib_amd import optimizers as O
    rule, base_lr = oo.cases()[case]
    cls = {"sgd": O.SGD, "rmsprop": O.RMSprop, "adagrad": O.Adagrad, "adadelta": O.Adadelta, "adamax": O.Adamax, "nadam": O.Nadam,
           "amsgrad": O.Adam}[rule.name]
    kw = dict(rule.h, amsgrad=True) if rule.name == "amsgrad" else dict(rule.h)
    return cls(learning_rate=base_lr if lr is None else lr, **kw)


class Flat:
    """parameters, gradients, three state slots, lr, t and P on the device, each fp32 buffer followed by PAD canary floats"""

    def __init__(self, n, opt, w0):
        from dib_amd import _lib
        self.lib, self.n, self.opt = _lib.load_library(), n, opt
        self.hyper = _lib.OptimizerHyper(**opt.hyper())
        dev = "cuda"
        buf = lambda: torch.full((n + PAD,), CANARY, dtype=torch.float32, device=dev)
        self.w, self.g = buf(), buf()
        self.slots = [buf() if k < opt.slots() else None for k in range(3)]
        self.w[:n] = _dev(w0)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.P = torch.full((1,), -7.0, dtype=torch.float64, device=dev) if opt.name == "nadam" else None
        self.stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.dib_optimizer_init(opt.kind, ctypes.byref(self.hyper), *(_ptr(s) for s in self.slots), n, _ptr(self.P),
                                         self.stream())
        assert rc == 0, rc

    def step(self, offset=0, count=None):
        sl = lambda b: None if b is None else b[offset:]
        return self.lib.dib_optimizer_step(self.opt.kind, ctypes.byref(self.hyper), _ptr(sl(self.w)), _ptr(sl(self.g)),
                                           *(_ptr(sl(s)) for s in self.slots), self.n if count is None else count, _ptr(self.lr),
                                           _ptr(self.t), _ptr(self.P), 1.0, self.stream())

    def advance(self):
        return self.lib.dib_optimizer_advance(self.opt.kind, ctypes.byref(self.hyper), _ptr(self.t), _ptr(self.P), self.stream())

    def canaries_intact(self):
        return all(bool((b[self.n:] == CANARY).all().item()) for b in [self.w, self.g] + [s for s in self.slots if s is not None])

    def state(self):
        torch.cuda.synchronize()
        return (self.w[:self.n].cpu().numpy(), [s[:self.n].cpu().numpy() for s in self.slots if s is not None],
                None if self.P is None else float(self.P.item()), int(self.t.item()))


def _run(case, n, steps):
    rule, lr = oo.cases()[case]
    w0, g, _, _ = oo.inputs(n, 0, steps)
    f = Flat(n, _make_optimizer(case), w0)
    for k in range(steps):
        f.g[:n] = _dev(g[k])
        f.lr.fill_(lr * oo.LR_FACTORS[k % len(oo.LR_FACTORS)])   # the learning rate changes between steps: a device scalar
        assert f.step() == 0 and f.advance() == 0
    return f


def _compare(case, f, n, steps):
    w, slots, P, t = f.state()
    w64, s64, P64 = oo.reference(case, n, 0, steps)
    bw, bs = oo.bounds(case, n, 0, steps)
    w0, _, zero, _ = oo.inputs(n, 0, steps)
    err = float(np.abs(w - w64).max())
    print(f"{case} n={n}: parameters max |device - float64| {err:.3g} (bound {bw:.3g})")
    assert err <= bw, (case, n, err, bw)
    assert len(slots) == len(s64)
    for k, (a, b, bound) in enumerate(zip(slots, s64, bs)):
        rel = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
        print(f"    slot {k}: relative error {rel:.3g} (bound {bound:.3g})")
        assert rel <= bound, (case, n, k, rel, bound)
    assert np.array_equal(w[zero], w0[zero]), "exactly-zero gradients must leave the parameters bit-identical"
    assert t == steps
    if P is not None:
        assert abs(P - P64) <= 1e-6 * P64, (P, P64)   # float32 momentum schedule, float64 product
    assert f.canaries_intact()


@pytest.mark.parametrize("case", CASES)
def test_every_rule_matches_the_float64_restatement(case):
    """8 steps, fresh gradients per step, a block of exactly-zero and one of 1e-4 gradients, lr set between steps; parameters
    and every state slot after the last step"""
    _compare(case, _run(case, 4099, oo.STEPS), 4099, oo.STEPS)


# 4 * 256 * 4096 + 4 * 256 + 3: the smallest n at which a thread takes a second grid-stride pass AND a scalar tail is left
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, 4 * 256 * 4096 + 4 * 256 + 3])
@pytest.mark.parametrize("case", ["adagrad", "nadam", "rmsprop_centered_momentum"])   # 1, 2 (+ P) and 3 state slots
def test_envelope_of_sizes(case, n):
    steps = 2
    _compare(case, _run(case, n, steps), n, steps)


def test_refused_calls_launch_nothing_and_write_nothing():
    n = 1023
    w0, g, _, _ = oo.inputs(n, 0, 2)
    f = Flat(n, _make_optimizer("rmsprop_centered_momentum"), w0)
    f.g[:n] = _dev(g[0])
    f.lr.fill_(1e-2)
    before = f.state()
    n0 = f.lib.dib_launch_count()
    assert f.step(offset=1, count=n - 1) == -1          # every pointer 4 bytes off a 16-byte boundary
    s2, f.slots[2] = f.slots[2], None
    assert f.step() == -1                               # centred + momentum: the third slot is missing
    f.slots[2] = s2
    assert f.step(count=-1) == -1
    f.opt.kind, kind = 99, f.opt.kind
    assert f.step() == -1 and f.advance() == -1
    f.opt.kind = kind
    assert f.lib.dib_launch_count() == n0
    after = f.state()
    assert np.array_equal(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert after[3] == 0 and f.canaries_intact()
    assert f.step() == 0 and f.advance() == 0 and f.lib.dib_launch_count() == n0 + 2   # one launch each
    assert f.state()[3] == 1


@pytest.mark.parametrize("case", ["nadam", "rmsprop_centered_momentum"])
def test_buckets_then_one_advance_equal_the_whole_buffer_step(case):
    """the data-parallel fit steps the three gradient buckets (dib_layout_part_range 1, 2, 3) separately, the last with the
    advance: bit for bit one whole-buffer step - checked at t = 1 and t = 3"""
    from dib_amd.engine import HipEngine
    spec = SPECS["boolean4_32x32"]
    a, b = (HipEngine(**spec_kwargs(spec), init_seed=3) for _ in range(2))
    opt = _make_optimizer(case)
    rng = np.random.default_rng(7)
    for eng in (a, b):
        eng.set_optimizer(opt)
        eng.set_lr(1e-2)
    covered = sorted(a.part_range(p) for p in (1, 2, 3))
    assert covered[0][0] == 0 and sum(c for _, c in covered) == a.n_params and all(o % 4 == 0 for o, _ in covered)
    for step in range(3):
        g = torch.from_numpy((rng.standard_normal(a.params.numel()) * 10.0 ** rng.uniform(-4, 0, a.params.numel())).astype(np.float32))
        for eng in (a, b):
            eng.grads.copy_(g)
        a.optimizer_step(opt)
        for k, part in enumerate((1, 2, 3)):
            b.optimizer_step_part(16, part, opt, bump=k == 2)
        torch.cuda.synchronize()
        if step in (0, 2):
            for name in ("params", "adam_m", "adam_v", "opt_s2", "opt_scalar", "t_dev"):
                ta, tb = getattr(a, name, None), getattr(b, name, None)
                assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb)), (name, step)
            assert int(b.t_dev.item()) == step + 1
    assert not torch.equal(a.params, torch.from_numpy(a.glorot_uniform(3)).to(a.params.device))


@pytest.mark.parametrize("case", ["nadam", "amsgrad"])
def test_captured_steps_replay_bit_identically_and_advance_t_and_P(case):
    n, steps = 4099, 3
    w0, g, _, _ = oo.inputs(n, 0, 2)

    def fresh():
        f = Flat(n, _make_optimizer(case), w0)
        f.g[:n] = _dev(g[0])
        f.lr.fill_(1e-2)
        return f

    eager = fresh()
    for _ in range(steps):
        assert eager.step() == 0 and eager.advance() == 0
    want = eager.state()
    f = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):      # one stream, a linear chain of three (step, advance) pairs
        for _ in range(steps):
            assert f.step() == 0 and f.advance() == 0
    assert f.state()[3] == 0           # capture enqueues nothing
    graph.replay()
    got = f.state()
    assert np.array_equal(got[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1]))
    assert got[2] == want[2] and got[3] == want[3] == steps
    graph.replay()
    again = f.state()
    assert again[3] == 2 * steps and not np.array_equal(again[0], got[0])
    if case == "nadam":
        mu = lambda t: np.float32(0.9) * (np.float32(1) - np.float32(0.5) * np.float32(0.96) ** (np.float32(0.004) * np.float32(t)))
        assert abs(got[2] - np.prod([float(mu(t)) for t in (1, 2, 3)])) < 1e-6 * got[2]
        assert abs(again[2] - np.prod([float(mu(t)) for t in range(1, 7)])) < 1e-6 * again[2]
    assert f.canaries_intact()


# ---- model level ----------------------------------------------------------------------------------------------------------
def _oracle_fit(spec, blocks, w0, rule, lr, x, y, epochs, bs, beta, noise_seed, shuffle_seed):
    """oracle/dib_oracle.py fit with the float64 rule in the place of Adam: the oracle's float64 gradients, flattened in the
    engine's layout, fed to tests/_oracle_optimizers.py -> (History of loss / KL{f}, final flat parameters)"""
    n, F, E = x.shape[0], spec.number_features, spec.feature_embedding_dimension
    w = np.asarray(w0, dtype=np.float64).copy()
    st = rule.init(w.size, np.float64)
    hist, step = {}, 0
    for epoch in range(epochs):
        order = orc.epoch_permutation(shuffle_seed, epoch, n)
        loss_sum, nseen, kl_steps = 0.0, 0, []
        for s0 in range(0, n, bs):
            rows = order[s0:s0 + bs]
            p = flat_to_params(blocks, w, spec)
            c = orc.forward(spec, p, x[rows].astype(np.float64), orc.philox_normal_all(noise_seed, step, rows, F, E))
            task, grads, _ = orc.backward(spec, p, x[rows].astype(np.float64), y[rows], c, beta, "bce_logits")
            rule.step(w, params_to_flat(blocks, grads, w.size, dtype=np.float64), st, lr)
            loss_sum += (task + beta * float(c.kl.sum())) * len(rows)
            nseen += len(rows)
            kl_steps.append(c.kl.copy())
            step += 1
        hist.setdefault("loss", []).append(loss_sum / nseen)
        for f, v in enumerate(np.mean(kl_steps, axis=0)):
            hist.setdefault(f"KL{f}", []).append(float(v))
    return hist, w


@pytest.mark.parametrize("path", ["default", "grouped_gemm"])
def test_fit_with_rmsprop_matches_the_float64_oracle_fit(path):
    """compile(optimizer=RMSprop(centered, momentum)) + 6 fit steps at B = 16 on the small Boolean zoo entry, on the row-tile
    kernels and on the grouped-GEMM path; the tolerance form of test_fit_trajectory_matches_oracle_fit"""
    import dib_amd
    spec = SPECS["boolean4_32x32"]
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)
    x, y = np.tile(x, (3, 1)).astype(np.float32), np.tile(y, 3).astype(np.float32)   # 48 rows: 3 steps per epoch
    lr = 3e-3
    with dispatch_path(path):
        model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        opt = dib_amd.optimizers.RMSprop(learning_rate=lr, rho=0.9, momentum=0.5, centered=True)
        model.compile(optimizer=opt, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True))
        w0 = model.get_flat_weights()
        beta = float(model.beta.value())
        eng = model._ensure_engine()
        n0 = eng.lib.dib_launch_count()
        hist = model.fit(x, y, epochs=2, shuffle=True, batch_size=16, verbose=False)
        assert int(eng.t_dev.item()) == 6
        got_w = model.get_flat_weights()
    rule = oo.Rule("rmsprop", rho=0.9, momentum=0.5, centered=True)
    ref, w = _oracle_fit(spec, model.param_blocks(), w0, rule, lr, x, y, 2, 16, beta, 4, 6)
    for k in ref:
        got, want = np.array(hist.history[k]), np.array(ref[k])
        tol = 1e-3 if "KL" in k else 2e-3
        assert np.abs(got - want).max() < tol * (1 + np.abs(want).max()), (k, got, want)
    n_params = eng.n_params
    assert np.abs(got_w[:n_params] - w[:n_params]).max() < 2e-3 * (1 + np.abs(w).max())
    assert np.abs(w[:n_params] - w0[:n_params]).max() > 5 * 2e-3 * (1 + np.abs(w).max())   # the run moved them well beyond the bound
    assert eng.lib.dib_launch_count() - n0 > 0


def test_fit_infonce_with_nadam_matches_the_float64_loop_oracle():
    """fit_infonce(optimizer=Nadam()): 4 steps at B = 16; both networks step with the same t; variables of both against the
    float64 loop oracle with the float64 Nadam in the place of its Adam"""
    import dib_amd
    import infonce_loop_oracle as ilo
    from dib_amd import infonce
    from dib_amd.dense import DenseStack
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 8, feature_embedding_dimension=8)
    rng = np.random.default_rng(11)
    xt, yt = rng.standard_normal((32, 4)).astype(np.float32), rng.standard_normal((32, 3)).astype(np.float32)
    xv, yv = rng.standard_normal((16, 4)).astype(np.float32), rng.standard_normal((16, 3)).astype(np.float32)
    seed, lr = 3, 3e-3
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=5, init_seed=seed)
    eng = model._ensure_engine()
    yenc = DenseStack(eng, 3, [32], 8, "relu", True, 5, seed=seed + 1)
    L = len(yenc.dims)
    p0 = flat_to_params(model.param_blocks(), model.get_flat_weights(), spec)
    y0 = ([yenc.kernel(l).cpu().numpy().astype(np.float64) for l in range(L)],
          [yenc.bias(l).cpu().numpy().astype(np.float64) for l in range(L)])
    kw = dict(batch_size=16, number_pretraining_epochs=1, number_annealing_epochs=2, beta_start=1e-3, beta_end=1e-2)
    got = infonce.fit_infonce(model, xt, yt, xv, yv, learning_rate=lr, similarity="l2", temperature=1.0, seed=seed,
                              output_encoder=yenc, optimizer=dib_amd.optimizers.Nadam(), shared_dimensionality=8, **kw)
    assert int(eng.t_dev.item()) == int(yenc.t_dev.item()) == 4
    assert abs(float(eng.opt_scalar.item()) - float(yenc.opt_scalar.item())) == 0.0

    class NadamLoop(ilo.InfoNCELoopOracle):
        def _adam(self, grads):   # one optimizer over all variables (train.py:196,219): the float64 Nadam, one (t, P)
            if not hasattr(self, "_st"):
                self._rule = oo.Rule("nadam")
                self._st = [self._rule.init(v.numel(), np.float64) for v in self.vars]
            self.t += 1
            with torch.no_grad():
                for v, g, st in zip(self.vars, grads, self._st):
                    w = v.detach().numpy().reshape(-1)    # shares the variable's memory
                    self._rule.step(w, g.detach().numpy().reshape(-1), st, self.lr)

    o = NadamLoop(spec, p0, ilo.YEncoder(y0[0], y0[1], "relu", True, 5, dtype=torch.float64), "l2", 1.0, lr, noise_seed=5)
    want = o.fit(xt, yt, xv, yv, seed=seed, **kw)
    assert o.t == 4
    for k in ("kl", "kl_validation", "loss_infonce", "loss_infonce_validation"):
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        tol = 1e-3 if "kl" in k else 2e-3
        assert g.shape == w.shape and np.abs(g - w).max() < tol * (1 + np.abs(w).max()), (k, g, w)
    xs = [t for t in flat_to_params(model.param_blocks(), model.get_flat_weights(), spec).tensors()]
    yb = yenc.params.cpu().numpy()
    ys = []
    for l, (i, oo_) in enumerate(yenc.dims):
        ys += [yb[yenc.w_off[l]: yenc.w_off[l] + i * oo_].reshape(i, oo_), yb[yenc.b_off[l]: yenc.b_off[l] + oo_]]
    starts = list(p0.tensors()) + [a for pair in zip(y0[0], y0[1]) for a in pair]
    assert len(xs) + len(ys) == len(o.vars)
    moved = 0.0
    for a, b, s in zip(xs + ys, o.vars, starts):
        b = b.detach().numpy()
        assert np.abs(np.asarray(a).reshape(b.shape) - b).max() < 2e-3 * (1 + np.abs(b).max())
        moved = max(moved, float(np.abs(b - np.asarray(s).reshape(b.shape)).max()))
    assert moved > 5e-3   # 4 Nadam steps at lr 3e-3: about 1e-2


def test_train_script_runs_with_optimizer_adagrad(tmp_path):
    from dib_amd import train
    hist = train.main(["--dataset", "boolean_circuit", "--number_pretraining_epochs", "1", "--number_annealing_epochs", "1",
                       "--batch_size", "128", "--artifact_outdir", str(tmp_path), "--optimizer", "adagrad",
                       "--feature_encoder_architecture", "32", "32", "--integration_network_architecture", "64",
                       "--feature_embedding_dimension", "8"])
    assert len(hist.history["loss"]) == 2 and np.isfinite(hist.history["loss"]).all()
    assert hist.model.optimizer.name == "adagrad" and hist.model.optimizer.learning_rate == 3e-4
    eng = hist.model._ensure_engine()
    a = eng.adam_m[:eng.n_params]
    assert float(a.min().item()) >= 0.1 and float(a.max().item()) > 0.1   # Adagrad's accumulator: starts at 0.1, only grows


def test_adam_and_plain_sgd_keep_their_launches():
    """the family is additive: Adam and momentum-free SGD still end the step in the fused tail - the same launch count per step
    with the optimizer tuple as with none - and optimizer_step() of either is adam_step() / sgd_step() (2 launches / 1)"""
    from dib_amd import optimizers as O
    from dib_amd.engine import HipEngine
    spec = SPECS["boolean4_32x32"]
    eng = HipEngine(**spec_kwargs(spec), init_seed=0)
    rng = np.random.default_rng(0)
    B = 16
    x = eng.to_device(rng.standard_normal((B, 4)).astype(np.float32))
    y = eng.to_device((rng.random((B, 1)) > 0.5).astype(np.float32))

    def launches(optimizer):
        n0 = eng.lib.dib_launch_count()
        eng.train_step(x, y, None, 0, B, 1, 0, "bce_logits", optimizer=optimizer)
        return eng.lib.dib_launch_count() - n0

    launches(None)   # workspace set-up
    base = launches(None)
    assert launches(("adam", 0.9, 0.999, 1e-7)) == base and launches(("sgd",)) == base
    rms = O.RMSprop()
    eng.set_optimizer(rms)                                   # (binding a rule fills its state: one launch, not a step's)
    assert launches(rms) == base + 2                # the rule's launch and its advance
    n0 = eng.lib.dib_launch_count()
    eng.optimizer_step(O.Adam())
    assert eng.lib.dib_launch_count() - n0 == 2
    eng.optimizer_step(O.SGD())
    assert eng.lib.dib_launch_count() - n0 == 3
    torch.cuda.synchronize()


# ---- one state object, one encoding --------------------------------------------------------------------------------------
def _engine(seed=0):
    from dib_amd.engine import HipEngine
    return HipEngine(**spec_kwargs(SPECS["boolean4_32x32"]), init_seed=seed)


def _same_state(a, b, names=("params", "adam_m", "adam_v", "opt_s2", "opt_scalar", "t_dev")):
    torch.cuda.synchronize()
    for name in names:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb)), name


@pytest.mark.parametrize("legacy", [("adam", 0.9, 0.999, 1e-7), ("sgd",)], ids=["adam", "sgd"])
def test_legacy_tuple_and_object_are_one_optimizer(legacy):
    """train_step and optimizer_step_part take the legacy tuple or the Optimizer it stands for: the same launches, the same bits"""
    from dib_amd import optimizers as O
    obj = O.Adam() if legacy[0] == "adam" else O.SGD()
    a, b = _engine(3), _engine(3)
    rng = np.random.default_rng(0)
    B = 16
    x = rng.standard_normal((B, 4)).astype(np.float32)
    y = (rng.random((B, 1)) > 0.5).astype(np.float32)
    counts = []
    for eng, optimizer in ((a, legacy), (b, obj)):
        xd, yd = eng.to_device(x), eng.to_device(y)
        eng.train_step(xd, yd, None, 0, B, 1, 0, "bce_logits", optimizer=None)   # workspace set-up
        n0 = eng.lib.dib_launch_count()
        for step in range(2):
            eng.train_step(xd, yd, None, 0, B, 1, step, "bce_logits", optimizer=optimizer)
        counts.append(eng.lib.dib_launch_count() - n0)
    assert counts[0] == counts[1]
    _same_state(a, b)
    assert int(a.t_dev.item()) == (2 if legacy[0] == "adam" else 0)
    assert not torch.equal(a.params, torch.from_numpy(a.glorot_uniform(3)).to(a.params.device))
    g = torch.from_numpy((rng.standard_normal(a.params.numel()) * 1e-2).astype(np.float32))
    counts = []
    for eng, optimizer in ((a, legacy), (b, obj)):
        eng.grads.copy_(g)
        n0 = eng.lib.dib_launch_count()
        for k, part in enumerate((1, 2, 3)):
            eng.optimizer_step_part(B, part, optimizer, bump=k == 2)
        counts.append(eng.lib.dib_launch_count() - n0)
    assert counts[0] == counts[1] > 0
    _same_state(a, b)
    assert int(a.t_dev.item()) == (3 if legacy[0] == "adam" else 0)


def test_dense_stack_reinitialises_its_state_on_a_change_of_rule():
    """DenseStack binds rules as HipEngine does: RMSprop steps, then Adam, is Adam from scratch (zero moments, t = 0), and the
    same RMSprop again is RMSprop from scratch"""
    from dib_amd import optimizers as O
    from dib_amd.dense import DenseStack
    eng = _engine()
    make = lambda: DenseStack(eng, 3, [32], 8, "relu", True, 5, seed=1)
    a, b, c = make(), make(), make()
    p0 = a.params.clone()
    rng = np.random.default_rng(5)
    g = [torch.from_numpy((rng.standard_normal(a.n_params) * 1e-2).astype(np.float32)).to(a.device) for _ in range(2)]
    rms, lr = O.RMSprop(momentum=0.5, centered=True), 1e-2

    def steps(stack, opt):
        for k in range(2):
            stack.grads.copy_(g[k])
            stack.optimizer_step(opt, lr=lr)

    steps(a, rms)
    assert int(a.t_dev.item()) == 2 and a.opt_s2 is not None and float(a.adam_v.abs().max().item()) > 0.0
    a.params.copy_(p0)
    steps(a, O.Adam())
    steps(b, O.Adam())
    _same_state(a, b, ("params", "adam_m", "adam_v", "t_dev"))
    assert int(a.t_dev.item()) == int(b.t_dev.item()) == 2
    assert not torch.equal(a.params, p0)
    a.params.copy_(p0)
    steps(a, rms)                     # the SAME object as before: the Adam steps in between were a change of rule
    steps(c, rms)
    _same_state(a, c)
    assert int(a.t_dev.item()) == 2


def test_dense_stack_and_the_c_entries_agree_on_nadam():
    """3 Nadam steps of a DenseStack against the same steps through the C entries on buffers of the test's own (Flat)"""
    from dib_amd import optimizers as O
    from dib_amd.dense import DenseStack
    stack = DenseStack(_engine(), 3, [32], 8, "relu", True, 5, seed=1)
    n, opt, lr = stack.n_params, O.Nadam(), 1e-2
    assert n % 4 == 0
    f = Flat(n, opt, stack.params.cpu().numpy())
    f.lr.fill_(lr)
    rng = np.random.default_rng(9)
    for _ in range(3):
        g = torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32)).to("cuda")
        stack.grads.copy_(g)
        f.g[:n] = g
        stack.optimizer_step(opt, lr=lr)
        assert f.step() == 0 and f.advance() == 0
    torch.cuda.synchronize()
    assert torch.equal(stack.params, f.w[:n]) and torch.equal(stack.adam_m, f.slots[0][:n]) and torch.equal(stack.adam_v, f.slots[1][:n])
    assert int(stack.t_dev.item()) == int(f.t.item()) == 3
    assert torch.equal(stack.opt_scalar, f.P) and float(f.P.item()) != 1.0
    assert f.canaries_intact() and stack.opt_s2 is None


def test_capture_step_graph_refuses_an_optimizer_outside_the_tail():
    from dib_amd import optimizers as O
    eng = _engine()
    x, y = eng.to_device(np.zeros((16, 4), dtype=np.float32)), eng.to_device(np.zeros((16, 1), dtype=np.float32))
    eng.enable_step_counter(0)
    torch.cuda.synchronize()
    n0 = eng.lib.dib_launch_count()
    for opt in (O.RMSprop(), O.build(O.Adam, clipnorm=1.0)):
        with pytest.raises(ValueError):
            eng.capture_step_graph(x, y, 16, "bce_logits", 1.0 / 16, 0, True, optimizer=opt)
    assert eng.lib.dib_launch_count() == n0 and 16 not in eng._ws_pinned
