"""CPU: the host half of include/dib_grad_transform.h (the variable table and its tile work-list, the argument checks), the
schedules and the optimizer objects' clip / decay settings, and what the inputs of tests/test_gpu_grad_transforms.py can tell apart.

Measured here (printed by the tests): the float32 restatement against the float64 one on the envelope inputs differs by about
1e-7 of the largest gradient per mode, so the asserted bounds are a few 1e-7 relative; the schedules differ by at most a few
float32 ulps of the initial rate.  The two algebraic orders of clipnorm, (g * c) / max(n, c) and g * (c / max(n, c)), are NOT
told apart at this tolerance (test_inputs_discriminate prints their distance in bounds)."""
import ctypes
import os
import re
from ctypes import byref, c_int, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import dib_oracle as orc
import _oracle_grad_transforms as og
from _helpers import SPECS
from dib_amd import _lib, optimizers, schedules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = orc.DIBSpec([1, 2, 1], [32, 32], [24], 1, feature_embedding_dimension=8)
ALL_SPECS = dict(SPECS, ragged_121=RAGGED)
CLASSES = [optimizers.Adam, optimizers.SGD, optimizers.RMSprop, optimizers.Adagrad, optimizers.Adadelta, optimizers.Adamax,
           optimizers.Nadam]


def _layout(lib, spec):
    ci = lambda xs: (c_int * max(1, len(xs)))(*xs)
    h = c_void_p()
    rc = lib.dib_layout_create(spec.number_features, ci(list(spec.feature_dimensionalities)),
                               len(spec.feature_encoder_architecture), ci(list(spec.feature_encoder_architecture)),
                               spec.feature_embedding_dimension, len(spec.integration_network_architecture),
                               ci(list(spec.integration_network_architecture)), spec.output_dimensionality,
                               int(spec.use_positional_encoding), spec.number_positional_encoding_frequencies,
                               _lib.ACTIVATIONS[spec.activation_fn], _lib.ACTIVATIONS[spec.output_activation_fn], byref(h))
    assert rc == 0
    return h


def _param_blocks(lib, h, spec):
    """HipEngine._query_blocks (what param_blocks() returns) without a GPU: (offset, count) in its order"""
    off, rows, cols = c_int64(), c_int(), c_int()
    out = []
    for net, nl in ((0, len(spec.feature_encoder_architecture) + 1), (1, len(spec.integration_network_architecture) + 1)):
        for layer in range(nl):
            for f in (range(spec.number_features) if net == 0 else [0]):
                for what in (0, 1):
                    assert lib.dib_layout_param_block(h, net, layer, f, what, byref(off), byref(rows), byref(cols)) == 0
                    out.append((off.value, rows.value * cols.value))
    return out


def test_the_header_and_the_binding_agree():
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "dib_grad_transform.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(dib_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == set(_lib.SIGNATURES_GRAD_TRANSFORM) and len(declared) == 6
    for name in declared:
        assert hasattr(lib, name)
    assert ctypes.sizeof(_lib.GradTile) == 16 and ctypes.sizeof(_lib.LrSchedule) == 144
    assert _lib.GRAD_TILE == og.TILE == int(re.search(r"#define DIB_GRAD_TILE (\d+)", hdr).group(1))


@pytest.mark.parametrize("name", sorted(ALL_SPECS))
def test_table_of_a_layout_is_param_blocks_and_buckets_are_whole_variables(name):
    lib = _lib.load_library()
    spec = ALL_SPECS[name]
    h = _layout(lib, spec)
    total = int(lib.dib_layout_param_count(h))
    blocks = _param_blocks(lib, h, spec)
    table = _lib.HostGradTable.from_layout(h, (total + 3) // 4 * 4)
    assert list(zip(table.offsets, table.counts)) == blocks
    assert sum(table.counts) == spec.num_params()
    # the tile work-list: every element of every segment in exactly one tile, no tile crosses a segment, the gaps are in none
    owner = np.full(total + 4, -1, dtype=np.int64)
    for k in range(table.n_tiles):
        t = table.tiles[k]
        o, c = table.offsets[t.segment], table.counts[t.segment]
        assert 1 <= t.count <= og.TILE and o <= t.start and t.start + t.count <= o + c
        assert (t.start - o) % og.TILE == 0 and (t.count == og.TILE or t.start + t.count == o + c)
        assert (owner[t.start:t.start + t.count] == -1).all()
        owner[t.start:t.start + t.count] = t.segment
        assert table.seg_tile0[t.segment] <= k < table.seg_tile0[t.segment + 1]
    assert int((owner >= 0).sum()) == spec.num_params()
    for s, (o, c) in enumerate(blocks):
        assert (owner[o:o + c] == s).all()
    assert table.seg_tile0[0] == 0 and table.seg_tile0[table.n_segments] == table.n_tiles
    # every gradient bucket of the data-parallel protocol is a run of whole variables, and 1 + 2 + 3 (1 + 0) cover all of them
    off, cnt = c_int64(), c_int64()
    ranges = {}
    for part in (0, 1, 2, 3):
        assert lib.dib_layout_part_range(h, part, byref(off), byref(cnt)) == 0
        first, n = table.segment_range(off.value, cnt.value)   # raises if a variable straddles an end of the bucket
        ranges[part] = set(range(first, first + n))
        inside = sum(table.counts[s] for s in ranges[part])
        assert inside <= cnt.value < inside + 4 * (len(ranges[part]) + 1)   # the rest of the bucket is alignment gaps
    everything = set(range(table.n_segments))
    assert ranges[1] | ranges[2] | ranges[3] == everything and ranges[2] | ranges[3] == ranges[0]
    assert not (ranges[1] & ranges[0]) and not (ranges[2] & ranges[3])
    lib.dib_layout_destroy(h)


def test_table_builder_refusals():
    lib = _lib.load_library()
    arr = lambda xs: (c_int64 * max(1, len(xs)))(*xs)
    tiles = lambda o, c, n: int(lib.dib_grad_table_tiles(arr(o), arr(c), len(o), n, None, 0, None))
    assert tiles([0, 8], [5, 4097], 8 + 4097) == 1 + 2
    assert tiles([], [], 10) == 0 and tiles([3], [0], 3) == 0
    assert tiles([0, 4], [5, 5], 100) == -1            # overlap
    assert tiles([8, 0], [5, 9], 100) == -1            # overlap, listed in the other order
    assert tiles([-1], [5], 100) == -1 and tiles([0], [-5], 100) == -1
    assert tiles([96], [5], 100) == -1                 # past the end of the buffer
    assert tiles([0], [1 << 62], (1 << 62) - 1) == -1
    buf, seg0 = (_lib.GradTile * 2)(), (c_int32 * 3)()
    assert lib.dib_grad_table_tiles(arr([0, 8]), arr([5, 4097]), 2, 8 + 4097, buf, 2, seg0) == -1   # capacity 2 < 3 tiles
    assert list(seg0) == [0, 0, 0]
    assert lib.dib_grad_table_tiles(arr([0]), arr([5]), 1, 5, buf, 2, None) == -1                     # tiles without seg_tile0
    assert lib.dib_grad_table_from_layout(None, None, None, 0) == -1
    h = _layout(lib, SPECS["boolean4_32x32"])
    n = lib.dib_grad_table_from_layout(h, None, None, 0)
    assert n == 2 * (3 * 4 + 3)
    assert lib.dib_grad_table_from_layout(h, arr([0] * n), arr([0] * n), n - 1) == -1
    lib.dib_layout_destroy(h)


def test_launch_entries_refuse_bad_arguments_before_touching_the_device():
    """every refusal below returns before a launch: this runs without a GPU (the pointers are never dereferenced)"""
    lib = _lib.load_library()
    host = _lib.HostGradTable([0, 8], [5, 4097], 8 + 4097)
    fake = 1 << 20   # a 16-byte aligned address nobody reads
    t = _lib.GradTable(host.n_segments, 0, host.n_tiles, ctypes.cast(host.seg_tile0, c_void_p), fake, fake)
    n0 = lib.dib_launch_count()
    sumsq = lambda tab=t, first=0, cnt=2, g=fake, cv=0.0, part=fake, ss=fake: lib.dib_grad_sumsq(
        byref(tab) if tab is not None else None, first, cnt, g, 1.0, cv, part, ss, None)
    assert sumsq(tab=None) == -1 and sumsq(first=-1) == -1 and sumsq(first=1, cnt=2) == -1 and sumsq(cnt=-1) == -1
    assert sumsq(g=None) == -1 and sumsq(g=fake + 4) == -1 and sumsq(part=None) == -1 and sumsq(ss=fake + 4) == -1
    assert sumsq(cv=-1.0) == -1 and sumsq(cv=float("inf")) == -1 and sumsq(cv=float("nan")) == -1
    assert sumsq(cnt=0) == 0                                        # nothing to do: DIB_OK without a launch
    apply = lambda tab=t, first=0, cnt=2, g=fake, cv=0.0, mode=1, c=1.0, ss=fake, ssa=fake, nss=2: lib.dib_grad_clip_apply(
        byref(tab) if tab is not None else None, first, cnt, g, 1.0, cv, mode, c, ss, ssa, nss, None)
    assert apply(tab=None) == -1 and apply(cnt=3) == -1 and apply(g=fake + 8) == -1 and apply(mode=3) == -1 and apply(mode=-1) == -1
    assert apply(mode=0, cv=0.0) == -1                              # no clip at all
    assert apply(c=0.0) == -1 and apply(c=-1.0) == -1 and apply(c=float("nan")) == -1 and apply(c=float("inf")) == -1
    assert apply(ss=None) == -1 and apply(mode=2, ssa=None) == -1 and apply(mode=2, nss=0) == -1
    assert apply(cnt=0) == 0
    bad = _lib.GradTable(host.n_segments, 0, host.n_tiles, None, fake, fake)
    assert sumsq(tab=bad) == -1 and apply(tab=bad) == -1
    nodev = _lib.GradTable(host.n_segments, 0, host.n_tiles, ctypes.cast(host.seg_tile0, c_void_p), None, None)
    assert sumsq(tab=nodev) == -1 and apply(tab=nodev) == -1
    good = _lib.LrSchedule.from_fields(dict(kind=schedules.LR_COSINE, initial=1e-3, decay_steps=10.0))
    assert lib.dib_lr_schedule_check(byref(good)) == 0
    assert lib.dib_lr_schedule_eval(byref(good), None, fake, None) == -1 and lib.dib_lr_schedule_eval(byref(good), fake, None, None) == -1
    assert lib.dib_lr_schedule_eval(None, fake, fake, None) == -1
    for d in (dict(kind=0), dict(kind=7), dict(kind=schedules.LR_COSINE, initial=1e-3, decay_steps=0.0),
              dict(kind=schedules.LR_EXPONENTIAL, initial=1e-3, decay_steps=10.0, rate=-0.5),
              dict(kind=schedules.LR_INVERSE_DECAY, initial=1e-3, rate=-1.0),
              dict(kind=schedules.LR_POLYNOMIAL, initial=1e-3, decay_steps=10.0, power=0.0),
              dict(kind=schedules.LR_PIECEWISE, boundaries=[], values=[1.0]),
              dict(kind=schedules.LR_PIECEWISE, boundaries=[5, 5], values=[1.0, 2.0, 3.0]),
              dict(kind=schedules.LR_EXPONENTIAL, initial=float("nan"), decay_steps=10.0, rate=0.5)):
        s = _lib.LrSchedule.from_fields(d)
        assert lib.dib_lr_schedule_check(byref(s)) == -1 and lib.dib_lr_schedule_eval(byref(s), fake, fake, None) == -1, d
    assert lib.dib_launch_count() == n0


# ---- schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(og.lr_cases()))
def test_schedules_in_float32_match_the_float64_restatement(case):
    want, got32, bound = og.lr_reference(case)
    sched = og.make_schedule(case)
    if isinstance(sched, dict):
        opt = optimizers.build(optimizers.SGD, learning_rate=sched["lr"], decay=sched["decay"])
        d = opt.lr_schedule()
        assert d["kind"] == schedules.LR_INVERSE_DECAY and opt.learning_rate == sched["lr"]
    else:
        opt = optimizers.Adam(learning_rate=sched)
        d = opt.lr_schedule()
        assert opt.learning_rate is sched and d == sched.descriptor()
    assert _lib.load_library().dib_lr_schedule_check(byref(_lib.LrSchedule.from_fields(d))) == 0
    got = np.array([schedules.evaluate(d, s) for s in og.LR_STEPS], dtype=np.float64)
    err = float(np.abs(got - want).max())
    print(f"{case}: steps {og.LR_STEPS} float64 {want}; max |package float32 - float64| {err:.3g}, "
          f"|restatement float32 - float64| {np.abs(got32 - want).max():.3g}, bound {bound:.3g}")
    assert err <= bound, (case, got, want)
    assert len(set(np.round(want, 12))) >= 3, "the steps must see the schedule move"


def test_schedule_landmarks():
    """known values of the float64 restatement itself: staircase edges, the cycle wrap, both sides of the piecewise boundaries,
    cosine and the clamped polynomial beyond their end"""
    c, i, ds = og.lr_cases(), np.float64(np.float32(3e-3)), og.DECAY_STEPS
    r07, r05 = np.float64(np.float32(0.7)), np.float64(np.float32(0.5))
    f = lambda case, s: float(og.lr(c[case], s))
    assert f("exponential_staircase", ds - 1) == i and f("exponential_staircase", ds) == i * r07 == f("exponential_staircase", ds + 1)
    assert abs(f("exponential_staircase", 3 * ds + 2) - i * r07 ** 3) < 1e-18
    assert f("exponential", 0) == i and abs(f("exponential", ds) - i * r07) < 1e-18 and f("exponential", 1) < i
    assert f("inverse_time_staircase", ds - 1) == i and abs(f("inverse_time_staircase", ds + 1) - i / (1 + r05)) < 1e-18
    end = np.float64(np.float32(1e-4))
    assert f("polynomial", ds) == end == f("polynomial", 3 * ds + 2) and f("polynomial", ds - 1) > end
    # cycle: at 3 * ds + 2 the period is 4 * ds, so the rate is back above its value at ds - 1 of the first period
    assert abs(f("polynomial_cycle", ds) - end) < 1e-18 and f("polynomial_cycle", ds + 1) > f("polynomial_cycle", ds - 1)
    assert abs(f("polynomial_cycle", 3 * ds + 2) - ((i - end) * (1 - 32 / 40) ** 0.5 + end)) < 1e-12
    v = [np.float64(np.float32(x)) for x in c["piecewise"]["values"]]
    assert [f("piecewise", s) for s in og.LR_STEPS] == [v[0], v[0], v[1], v[1], v[2], v[3]]
    a = np.float64(np.float32(0.1))
    assert abs(f("cosine", ds) - i * a) < 1e-12 and f("cosine", 3 * ds + 2) == f("cosine", ds) and f("cosine", 0) == i
    assert abs(f("decay", ds) - i / (1 + np.float64(np.float32(0.05)) * ds)) < 1e-18


# ---- the settings on the optimizer objects ---------------------------------------------------------------------------------------
# The constructors keep refusing clipnorm / clipvalue / global_clipnorm / decay as KEYWORDS (tests/test_optimizers_host.py pins
# that for every class); they are attributes, as optimizer_v2 has them too, with configure / optimizers.build / optimizers.get(name,
# ...) as the one-line forms.
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("arg", ["clipnorm", "clipvalue", "global_clipnorm", "decay"])
def test_transform_settings_are_accepted_by_every_class(cls, arg):
    plain = cls()
    assert plain.clip() is None and plain.lr_schedule() is None and getattr(plain, arg) in (None, 0.0)
    by_attr, by_conf, by_build, by_get = cls(), cls().configure(**{arg: 0.5}), optimizers.build(cls, **{arg: 0.5}), \
        optimizers.get(cls.name, **{arg: 0.5})
    setattr(by_attr, arg, 0.5)
    for opt in (by_attr, by_conf, by_build, by_get):
        assert type(opt) is cls and getattr(opt, arg) == 0.5
        if arg == "decay":
            assert opt.clip() is None and opt.lr_schedule() == dict(kind=schedules.LR_INVERSE_DECAY, initial=opt.learning_rate, rate=0.5)
        else:
            mode = dict(clipvalue=optimizers.CLIP_NONE, clipnorm=optimizers.CLIP_NORM, global_clipnorm=optimizers.CLIP_GLOBAL_NORM)[arg]
            assert opt.clip() == ((0.5, mode, 0.0) if arg == "clipvalue" else (0.0, mode, 0.5)) and opt.lr_schedule() is None
        assert opt.native == plain.native and opt.kind == plain.kind and opt.hyper() == plain.hyper()   # not a change of rule
    setattr(by_attr, arg, None)   # and off again
    assert by_attr.clip() is None and by_attr.lr_schedule() is None
    with pytest.raises(ValueError) as e:   # the keyword stays refused, and the message names the route that works
        cls(**{arg: 0.5})
    assert f"optimizer.{arg} = value" in str(e.value) and "optimizers.get" in str(e.value)


@pytest.mark.parametrize("cls", CLASSES)
def test_refusals_of_the_settings(cls):
    with pytest.raises(ValueError, match="Cannot accept both"):
        optimizers.build(cls, clipnorm=1.0, global_clipnorm=1.0)
    with pytest.raises(ValueError, match="Cannot accept both"):
        cls().configure(global_clipnorm=1.0).configure(clipnorm=1.0)
    for arg in ("clipnorm", "clipvalue", "global_clipnorm"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            opt = cls()
            with pytest.raises(ValueError, match=arg):
                setattr(opt, arg, bad)
            assert opt.clip() is None          # a refused assignment changes nothing
    with pytest.raises(ValueError, match="decay"):
        cls().decay = -0.1
    sched = schedules.ExponentialDecay(1e-3, 10, 0.5)
    with pytest.raises(ValueError, match="decay"):
        optimizers.build(cls, learning_rate=sched, decay=0.1)
    with pytest.raises(ValueError, match="decay"):
        optimizers.build(cls, decay=0.1).learning_rate = sched
    with pytest.raises(ValueError, match="unknown setting"):
        cls().configure(momentum=0.5)
    for arg in ("weight_decay", "use_ema"):
        with pytest.raises(ValueError, match="2.11"):
            cls(**{arg: 0.5})
        with pytest.raises(ValueError, match="2.11"):
            optimizers.get(cls.name, **{arg: 0.5})
    assert optimizers.UNSUPPORTED_ARGUMENTS == ("weight_decay", "use_ema")
    assert optimizers.build(cls, clipvalue=1.0, clipnorm=2.0).clip() == (1.0, optimizers.CLIP_NORM, 2.0)
    assert optimizers.build(cls, clipvalue=1.0, global_clipnorm=2.0).clip() == (1.0, optimizers.CLIP_GLOBAL_NORM, 2.0)
    # switching between the two norms: the first goes off before the second goes on
    opt = optimizers.build(cls, clipnorm=1.0)
    opt.clipnorm = None
    opt.global_clipnorm = 2.0
    assert opt.clip() == (0.0, optimizers.CLIP_GLOBAL_NORM, 2.0)


def test_a_float_replaces_a_schedule_and_schedules_validate():
    opt = optimizers.Adam(schedules.CosineDecay(3e-4, 1000))
    assert opt.lr_schedule()["kind"] == schedules.LR_COSINE
    opt.learning_rate = 3e-4                      # reference train.py:129
    assert opt.learning_rate == 3e-4 and opt.lr_schedule() is None
    assert optimizers.get("adam", clipnorm=1.0).clipnorm == 1.0
    assert optimizers.build(optimizers.SGD, 0.1, momentum=0.9, clipvalue=2.0).hyper() == dict(momentum=0.9, nesterov=0)
    with pytest.raises(ValueError):
        optimizers.get(opt, clipnorm=1.0)
    with pytest.raises(ValueError):
        schedules.PiecewiseConstantDecay([1, 2], [1.0, 2.0])
    with pytest.raises(ValueError):
        schedules.PiecewiseConstantDecay(list(range(9)), [1.0] * 10)
    with pytest.raises(ValueError):
        schedules.PiecewiseConstantDecay([3, 3], [1.0, 2.0, 3.0])
    for cls in (schedules.ExponentialDecay, schedules.InverseTimeDecay):
        with pytest.raises(ValueError):
            cls(1e-3, 0, 0.5)
    with pytest.raises(ValueError):
        schedules.CosineDecay(1e-3, -5)
    with pytest.raises(ValueError):
        schedules.PolynomialDecay(1e-3, 10, power=0.0)


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------
def test_inputs_discriminate():
    flat, segments, gaps = og.envelope()
    live = ~gaps
    assert {o % 4 for o, _ in segments} == {0, 1, 2, 3}
    assert [n for _, n in segments] == list(og.SIZES) and {og.TILE - 1, og.TILE, og.TILE + 1} <= set(og.SIZES)
    assert gaps.sum() >= 8 and (flat[gaps] == og.GAP_MARK).all()
    zero = [k for k, (o, n) in enumerate(segments) if not flat[o:o + n].any()]
    assert len(zero) >= 1
    for gs in (1.0, 1.0 / 3.0):
        none, ss = og.transform(flat, segments, gs)
        nrm = np.sqrt(ss)
        scaled = int((nrm > og.CLIPNORM).sum())
        assert scaled >= len(segments) / 4 and len(segments) - scaled >= len(segments) / 4, nrm
        assert np.sqrt(ss.sum()) > og.GLOBAL_CLIPNORM                       # the global clip is active
        clipped_elems = float((np.abs(none[live]) > og.CLIPVALUE).mean())
        assert 0.05 < clipped_elems < 0.95
        outs, worst = {"none": none}, 0.0
        for mode in og.MODES:
            w, ss_m, b = og.envelope_reference(mode, gs)
            g32, _ = og.transform(flat, segments, gs, dtype=np.float32, **og.MODES[mode])
            print(f"grad_scale {gs:.3g} {mode}: max |float32 - float64| {np.abs(g32[live] - w[live]).max():.3g}, bound {b:.3g}, "
                  f"largest |g| {np.abs(w[live]).max():.3g}")
            worst = max(worst, b)
            outs[mode] = w
            for k in zero:
                o, n = segments[k]
                assert not w[o:o + n].any() and not np.signbit(w[o:o + n]).any()
            assert (w[gaps] == og.GAP_MARK).all()
        names = sorted(outs)
        for i, a in enumerate(names):
            for b_ in names[i + 1:]:
                d = float(np.abs(outs[a][live] - outs[b_][live]).max())
                assert d > 100 * worst, (a, b_, d, worst)
        # a clipnorm whose norm ignored grad_scale (grad_scale 1: the same thing, so only the other scale can tell)
        w, _, b = og.envelope_reference("clipnorm", gs)
        wrong, _ = og.transform(flat, segments, gs, clipnorm=og.CLIPNORM, ignore_grad_scale_in_norm=True)
        d = float(np.abs(wrong[live] - w[live]).max())
        assert (d > 100 * b) if gs != 1.0 else d == 0.0, (gs, d, b)
        swapped, _ = og.transform(flat, segments, gs, clipnorm=og.CLIPNORM, dtype=np.float32, swapped_order=True)
        print(f"grad_scale {gs:.3g}: g * (c / max(n, c)) in float32 is {np.abs(swapped[live] - w[live]).max() / b:.2f} bounds from "
              f"the float64 (g * c) / max(n, c): not told apart")


def test_a_non_finite_norm_makes_every_gradient_nan():
    """tf.clip_by_global_norm's behaviour, on the restatement only (the device test does not provoke it)"""
    flat, segments, gaps = og.envelope()
    for poison in (np.inf, np.nan):
        bad = flat.copy()
        bad[segments[3][0]] = poison
        for dtype in (np.float64, np.float32):
            out, _ = og.transform(bad, segments, global_clipnorm=og.GLOBAL_CLIPNORM, dtype=dtype)
            assert np.isnan(out[~gaps]).all() and (out[gaps] == og.GAP_MARK).all()
    out, _ = og.transform(np.zeros(16, np.float32), [(0, 16)], global_clipnorm=1.0)
    assert not out.any()                                                    # N = 0: scale = c * min(inf, 1 / c) = 1
