"""CPU: the Keras optimizer family's public surface (optimizers.get, the classes, their rejections), the host half of the C ABI
(include/dib_optimizers.h: slots, refusals - they return before any launch), the NumPy restatements of the rules
(tests/_oracle_optimizers.py) against torch's float64 optimizers where the two place epsilon alike, and the conditions that make
the GPU comparison of tests/test_gpu_optimizers.py mean something: its inputs move the parameters far beyond its bound, tell
RMSprop's two epsilon placements apart and tell every two rules apart."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _oracle_optimizers as oo
from dib_amd import _lib, optimizers


# ---- optimizers.get and the classes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,lr", [("adam", optimizers.Adam, 1e-3), ("sgd", optimizers.SGD, 0.01),
                                         ("rmsprop", optimizers.RMSprop, 1e-3), ("adagrad", optimizers.Adagrad, 1e-3),
                                         ("adadelta", optimizers.Adadelta, 1e-3), ("adamax", optimizers.Adamax, 1e-3),
                                         ("nadam", optimizers.Nadam, 1e-3)])
def test_get_knows_every_keras_name_in_any_case(name, cls, lr):
    for spelled in (name, name.upper(), name.capitalize()):
        opt = optimizers.get(spelled)
        assert type(opt) is cls and opt.name == name and opt.learning_rate == lr
    opt.learning_rate = 3e-4   # reference train.py:129
    assert opt.learning_rate == 3e-4
    assert optimizers.get(opt) is opt


def test_keras_defaults():
    r = optimizers.RMSprop()
    assert (r.rho, r.momentum, r.epsilon, r.centered) == (0.9, 0.0, 1e-7, False)
    a = optimizers.Adagrad()
    assert (a.initial_accumulator_value, a.epsilon) == (0.1, 1e-7)
    d = optimizers.Adadelta()
    assert (d.rho, d.epsilon) == (0.95, 1e-7)
    for o in (optimizers.Adamax(), optimizers.Nadam(), optimizers.Adam()):
        assert (o.beta_1, o.beta_2, o.epsilon) == (0.9, 0.999, 1e-7)
    s = optimizers.SGD()
    assert (s.momentum, s.nesterov) == (0.0, False)
    assert optimizers.Adam().amsgrad is False


def test_sgd_keeps_its_momentum_and_adam_its_amsgrad():
    s = optimizers.SGD(momentum=0.9, nesterov=True)
    assert s.momentum == 0.9 and s.nesterov is True and not s.native and s.slots() == 1
    assert s.hyper() == dict(momentum=0.9, nesterov=1)
    a = optimizers.Adam(amsgrad=True)
    assert a.amsgrad is True and not a.native and a.slots() == 3 and a.kind == optimizers.OPT_AMSGRAD
    # the plain forms stay on their own launches
    assert optimizers.SGD().native and optimizers.Adam().native and optimizers.SGD(momentum=0.0).native


def test_as_optimizer_maps_the_legacy_tuples_once_and_refuses_the_rest():
    a = optimizers.as_optimizer(("adam", 0.8, 0.99, 1e-6))
    assert type(a) is optimizers.Adam and (a.beta_1, a.beta_2, a.epsilon) == (0.8, 0.99, 1e-6) and a.rides_in_tail
    assert optimizers.as_optimizer(("adam", 0.8, 0.99, 1e-6)) is a            # an equal tuple: the identical object
    assert optimizers.as_optimizer(("adam", 0.9, 0.999, 1e-7)) is not a
    s = optimizers.as_optimizer(("sgd",))
    assert type(s) is optimizers.SGD and s.momentum == 0.0 and optimizers.as_optimizer(("sgd",)) is s
    for opt in (a, optimizers.RMSprop(), optimizers.build(optimizers.Adam, clipnorm=1.0)):
        assert optimizers.as_optimizer(opt) is opt
    for bad in (("opt", optimizers.RMSprop()), ("adam",), ("adam", 0.9, 0.999), ("adam", 0.9, 0.999, [1e-7]), ("sgd", 0.9), ("rmsprop",),
                (), "adam", None, 3, ["sgd"]):
        with pytest.raises(ValueError):
            optimizers.as_optimizer(bad)


def test_rides_in_tail_is_plain_adam_and_plain_sgd_without_a_clip():
    O = optimizers
    for opt in (O.SGD(momentum=0.9), O.Adam(amsgrad=True), O.RMSprop(), O.Adagrad(), O.Adadelta(), O.Adamax(), O.Nadam()):
        assert not opt.native and not opt.rides_in_tail
    for cls in (O.Adam, O.SGD):
        assert cls().rides_in_tail and cls(3e-4).rides_in_tail
        assert O.build(cls, decay=0.1).rides_in_tail                          # a learning-rate setting is not a clip
        for setting in ("clipnorm", "clipvalue", "global_clipnorm"):
            opt = O.build(cls, **{setting: 1.0})
            assert opt.native and not opt.rides_in_tail
            setattr(opt, setting, None)
            assert opt.rides_in_tail


@pytest.mark.parametrize("name", ["ftrl", "adamw", "adafactor", "lion", "", None, 3])
def test_unknown_names_are_refused_with_the_supported_set(name):
    with pytest.raises(ValueError) as e:
        optimizers.get(name)
    assert repr(name) in str(e.value) and "rmsprop" in str(e.value) and "nadam" in str(e.value)


@pytest.mark.parametrize("cls", [optimizers.Adam, optimizers.SGD, optimizers.RMSprop, optimizers.Adagrad, optimizers.Adadelta,
                                 optimizers.Adamax, optimizers.Nadam])
@pytest.mark.parametrize("arg", ["clipnorm", "clipvalue", "global_clipnorm", "decay", "weight_decay", "use_ema", "momentun"])
def test_arguments_that_would_change_the_update_are_refused_not_dropped(cls, arg):
    with pytest.raises(ValueError) as e:
        cls(**{arg: 0.5})
    assert arg in str(e.value) and "rmsprop" in str(e.value)


def test_python_slots_agree_with_the_library():
    lib = _lib.load_library()
    opts = [optimizers.SGD(momentum=0.5), optimizers.SGD(momentum=0.5, nesterov=True), optimizers.RMSprop(),
            optimizers.RMSprop(centered=True), optimizers.RMSprop(momentum=0.9), optimizers.RMSprop(centered=True, momentum=0.9),
            optimizers.Adagrad(), optimizers.Adadelta(), optimizers.Adamax(), optimizers.Nadam(), optimizers.Adam(amsgrad=True)]
    want = [1, 1, 1, 2, 2, 3, 1, 2, 2, 2, 3]
    for o, w in zip(opts, want):
        h = _lib.OptimizerHyper(**o.hyper())
        assert lib.dib_optimizer_slots(o.kind, ctypes.byref(h)) == w == o.slots(), o.name
    h = _lib.OptimizerHyper()
    assert lib.dib_optimizer_slots(optimizers.OPT_SGD_MOMENTUM, ctypes.byref(h)) == 0   # momentum 0: dib_sgd_step's case
    assert lib.dib_optimizer_slots(0, ctypes.byref(h)) == -1 and lib.dib_optimizer_slots(8, ctypes.byref(h)) == -1
    assert lib.dib_optimizer_slots(optimizers.OPT_NADAM, None) == -1


def test_refusals_return_before_any_launch():
    """DIB_E_ARG (-1) for an unknown kind, a missing slot, a misaligned pointer, n < 0 - on fake addresses, without a GPU"""
    lib = _lib.load_library()
    A = 1 << 20   # never dereferenced: every call below is refused on the host
    p = lambda v: ctypes.c_void_p(v)
    n0 = lib.dib_launch_count()
    h = _lib.OptimizerHyper(**optimizers.RMSprop(centered=True, momentum=0.9).hyper())
    step = lambda kind, hy, w, g, s0, s1, s2, n, lr=A, t=A, P=None: lib.dib_optimizer_step(
        kind, ctypes.byref(hy), p(w), p(g), p(s0), p(s1), p(s2), n, p(lr), p(t), p(P), 1.0, None)
    K = optimizers.OPT_RMSPROP
    assert step(0, h, A, A, A, A, A, 16) == -1 and step(99, h, A, A, A, A, A, 16) == -1
    assert step(K, h, A, A, A, A, None, 16) == -1        # centred + momentum needs three slots
    assert step(K, h, A, A, A, None, A, 16) == -1
    assert step(K, h, A, A, A, A, A, -1) == -1
    for bad in (A + 4, A + 8, A + 12):
        assert step(K, h, bad, A, A, A, A, 16) == -1 and step(K, h, A, bad, A, A, A, 16) == -1
        assert step(K, h, A, A, bad, A, A, 16) == -1 and step(K, h, A, A, A, A, bad, 16) == -1
    assert step(K, h, None, A, A, A, A, 16) == -1 and step(K, h, A, A, A, A, A, 16, lr=None) == -1
    assert step(K, h, A, A, A, A, A, 16, t=None) == -1
    hn = _lib.OptimizerHyper(**optimizers.Nadam().hyper())
    assert step(optimizers.OPT_NADAM, hn, A, A, A, A, None, 16, P=None) == -1      # Nadam without its P
    assert step(optimizers.OPT_NADAM, hn, A, A, A, A, None, 16, P=A + 4) == -1
    hs = _lib.OptimizerHyper()
    assert step(optimizers.OPT_SGD_MOMENTUM, hs, A, A, A, None, None, 16) == -1   # momentum 0 is dib_sgd_step
    assert lib.dib_optimizer_init(K, ctypes.byref(h), p(A), p(A), None, 16, None, None) == -1
    assert lib.dib_optimizer_init(K, ctypes.byref(h), p(A), p(A + 4), p(A), 16, None, None) == -1
    assert lib.dib_optimizer_advance(0, ctypes.byref(h), p(A), None, None) == -1
    assert lib.dib_optimizer_advance(K, ctypes.byref(h), None, None, None) == -1
    assert lib.dib_optimizer_advance(optimizers.OPT_NADAM, ctypes.byref(hn), p(A), None, None) == -1
    assert step(K, h, A, A, A, A, A, 0) == 0             # an empty range: nothing to do, nothing launched
    assert lib.dib_launch_count() == n0


# ---- the restatements against torch's float64 optimizers, at lr = 1e-3 (constant: torch folds it into SGD's buffer) ---------
LR = 1e-3


def _torch_run(make, n=4099, steps=8):
    w0, g, _, _ = oo.inputs(n)
    w = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = make([w])
    for k in range(steps):
        w.grad = torch.tensor(g[k], dtype=torch.float64)
        opt.step()
    return w.detach().numpy()


def _numpy_run(rule, lr, n=4099, steps=8):
    w0, g, _, _ = oo.inputs(n)
    w = w0.astype(np.float64)
    st = rule.init(n, np.float64)
    for k in range(steps):
        rule.step(w, g[k], st, lr)
    return w


@pytest.mark.parametrize("rule,lr,make", [
    (oo.Rule("nadam"), LR, lambda p: torch.optim.NAdam(p, lr=LR, betas=(0.9, 0.999), eps=1e-7, momentum_decay=0.004)),
    (oo.Rule("adagrad"), LR, lambda p: torch.optim.Adagrad(p, lr=LR, initial_accumulator_value=0.1, eps=1e-7)),
    (oo.Rule("adadelta"), LR, lambda p: torch.optim.Adadelta(p, lr=LR, rho=0.95, eps=1e-7)),
    (oo.Rule("sgd", momentum=0.9), LR, lambda p: torch.optim.SGD(p, lr=LR, momentum=0.9)),
    (oo.Rule("sgd", momentum=0.9, nesterov=True), LR, lambda p: torch.optim.SGD(p, lr=LR, momentum=0.9, nesterov=True)),
], ids=["nadam", "adagrad", "adadelta", "sgd_momentum", "sgd_nesterov"])
def test_restatements_agree_with_torch_float64(rule, lr, make):
    """2e-11 on parameters of unit scale that move a few 1e-3: float64 rounding of two orders of the same operations.  torch's
    NAdam keeps its running product mu_product in a FLOAT32 scalar whatever the parameters' dtype: half an ulp (3e-8) of
    P_1 = 0.45 and P_2 = 0.2 is 2.5e-8 and 0.8e-8 of the coefficient 1 / (1 - P_t), on steps of at most 3.2 lr = 3.2e-3 (later
    P_t are negligible): up to 1.1e-10, so Nadam is compared to 2e-10 (measured: 2.2e-11)."""
    err = np.abs(_numpy_run(rule, lr) - _torch_run(make)).max()
    print(f"{rule.name}: restatement vs torch float64: {err:.3g}")
    assert err < (2e-10 if rule.name == "nadam" else 2e-11)


# ---- what the GPU comparison's inputs can show ------------------------------------------------------------------------------
CASES = sorted(oo.cases())


@pytest.mark.parametrize("case", CASES)
def test_inputs_move_the_parameters_far_beyond_the_bound(case):
    w0, _, zero, _ = oo.inputs()
    w, _, _ = oo.reference(case)
    bound, slot_bounds = oo.bounds(case)
    err, slot_err = oo.format_error(case)
    print(f"{case}: float32 restatement vs float64: parameters {err:.3g}, slots {['%.3g' % e for e in slot_err]}")
    assert np.abs(w - w0).max() >= 1000 * bound, (np.abs(w - w0).max(), bound)
    # the format's cost, not a loose net: a few 1e-7 on unit-scale parameters; on v, 1.3e-5 - what 1 - beta_2 loses in float32
    assert bound < 1e-5 and all(b < 1e-4 for b in slot_bounds)
    assert np.array_equal(w[zero], w0[zero].astype(np.float64))   # exactly-zero gradients leave the parameter alone


@pytest.mark.parametrize("case", ["rmsprop", "rmsprop_centered", "rmsprop_momentum", "rmsprop_centered_momentum"])
def test_inputs_tell_rmsprops_two_epsilon_placements_apart(case):
    rule, lr = oo.cases()[case]
    _, _, _, small = oo.inputs()
    w, _, _ = oo.reference(case)
    w_sw, _, _ = oo.run(oo.Rule("rmsprop", eps_swapped=True, **rule.h), lr, np.float64)
    bound, _ = oo.bounds(case)
    assert np.abs(w_sw - w)[small].max() >= 100 * bound   # the block of 1e-4 gradients: den ~ 1e-9 is below epsilon = 1e-7
    assert np.abs(w_sw - w).max() >= 100 * bound


def test_inputs_tell_every_two_rules_apart():
    ref = {c: oo.reference(c)[0] for c in CASES}
    ref["adam"] = oo.run(oo.Rule("adam", **oo.cases()["amsgrad"][0].h), 1e-2, np.float64)[0]   # AMSGrad must not pass as Adam either
    worst = max(oo.bounds(c)[0] for c in CASES)
    for a, b in itertools.combinations(sorted(ref), 2):
        assert np.abs(ref[a] - ref[b]).max() >= 100 * worst, (a, b)
