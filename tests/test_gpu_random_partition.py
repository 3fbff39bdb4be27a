"""dib_partition_symbolize (include/dib_partition.h) through the C ABI, and dib_amd.RandomPartition / random_partition_survey,
against the float64 restatement of cell 7 (tests/_oracle_random_partition.py), across the kernel's envelope: in_dim 1-4,
1-3 hidden layers of widths 16 / 64 / 128 and a mixed stack, A in {2, 3, 4, 5, 16}, every accepted activation, fp32 and fp64
input with padded rows (ldx > in_dim, the padding NaN so a stray read shows), ragged point counts and more points than one
grid-stride pass.  Outputs carry guard regions with NaN / sentinel fill that must survive the launch.

Bounds.  Logits: |got - ref| <= 1e-5 x the same chain on |W|, |b|, |x| (the scale of fp32 rounding; worst case ~k eps for k
terms per layer).  Symbols: equal to the oracle's wherever the oracle's margin (largest minus second-largest |logit|) is at least
2 x that bound of the point's logits, where no rounding can change the argmax; below it they may differ, at most 1e-4 n points."""
import ctypes

import numpy as np
import pytest
import torch

import _oracle_random_partition as orp
from dib_amd import _lib, chaos_data
from dib_amd import random_partition as rp
from dib_amd.dense import _MlpDesc

pytestmark = pytest.mark.gpu

ACT = {"linear": 0, "relu": 1, "leaky_relu": 2, "tanh": 3}
GUARD = 17
SENT_U8 = 0xA5
SENT_I64 = -0x5A5A5A5A5A
DIB_E_ARG, DIB_E_UNSUPPORTED = -1, -4   # include/dib_hip.h
LOGIT_RTOL = 1e-5


def _lib_():
    return _lib.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _weights(d, widths, A, rng):
    """cell 7's distributions: hidden N(0.05, 0.5^2), glorot-uniform output kernel, zero output bias (made nonzero here, so the
    output bias is exercised)"""
    dims = [d] + list(widths)
    w = []
    for i, o in zip(dims[:-1], dims[1:]):
        w += [rng.normal(0.05, 0.5, (i, o)).astype(np.float32), rng.normal(0.05, 0.5, o).astype(np.float32)]
    lim = np.sqrt(6.0 / (dims[-1] + A))
    w += [rng.uniform(-lim, lim, (dims[-1], A)).astype(np.float32), (0.1 * rng.standard_normal(A)).astype(np.float32)]
    return w


def _flat(weights, d, act):
    """desc + device buffer with the layers at unaligned, interleaved offsets and NaN between them"""
    desc = _MlpDesc()
    L = len(weights) // 2
    flat, o = [np.full(3, np.nan, np.float32)], 3
    for l in range(L):
        w, b = weights[2 * l], weights[2 * l + 1]
        desc.w_off[l], desc.b_off[l], desc.width[l] = o, o + w.size + 1, w.shape[1]
        flat += [w.ravel(), np.full(1, np.nan, np.float32), b, np.full(2, np.nan, np.float32)]
        o += w.size + 1 + b.size + 2
    desc.n_hidden, desc.in_dim, desc.n_freq, desc.act = L - 1, d, 1, ACT[act]
    return desc, torch.from_numpy(np.concatenate(flat)).cuda()


def _points(n, d, ldx, rng, f64):
    """[n][ldx] with NaN padding columns; the kernel reads columns < d only"""
    x = np.full((n, ldx), np.nan)
    x[:, :d] = rng.uniform(-2.0, 2.0, (n, d))
    return x if f64 else x.astype(np.float32)


def _call(desc, params, x, A, counts0=None, num_cus=None, logits=True):
    """one dib_partition_symbolize launch on guarded outputs; returns host (sym, logits, counts)"""
    n, ldx = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    sym = torch.full((n + GUARD,), SENT_U8, dtype=torch.uint8, device="cuda")
    lg = torch.full(((n + GUARD) * A,), float("nan"), dtype=torch.float32, device="cuda")
    cnt = torch.full((A + GUARD,), SENT_I64, dtype=torch.int64, device="cuda")
    cnt[:A] = torch.as_tensor(np.zeros(A, np.int64) if counts0 is None else counts0)
    old = _lib.get_tuning("num_cus")
    try:
        if num_cus is not None:
            _lib.set_tuning("num_cus", num_cus)
        _lib.check(_lib_().dib_partition_symbolize(ctypes.byref(desc), ctypes.c_void_p(params.data_ptr()),
                                                   ctypes.c_void_p(xd.data_ptr()), int(x.dtype == np.float64), ldx, n,
                                                   ctypes.c_void_p(sym.data_ptr()), ctypes.c_void_p(lg.data_ptr()) if logits else None,
                                                   ctypes.c_void_p(cnt.data_ptr()), _stream()), "dib_partition_symbolize")
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning("num_cus", old)
    s, l, c = sym.cpu().numpy(), lg.cpu().numpy(), cnt.cpu().numpy()
    assert np.all(s[n:] == SENT_U8), "sym: guard region written"
    assert np.all(np.isnan(l[n * A:])), "logits: guard region written"
    assert np.all(c[A:] == SENT_I64), "counts: guard region written"
    if not logits:
        assert np.all(np.isnan(l)), "logits written although NULL was passed"
    return s[:n], l[: n * A].reshape(n, A), c[:A]


def _check_against_oracle(weights, act, x, d, sym, lg, what=""):
    ref = orp.forward(weights, x[:, :d], act)
    scale = orp.abs_forward(weights, x[:, :d], act)
    bound = LOGIT_RTOL * scale
    err = np.abs(lg.astype(np.float64) - ref)
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{what} logits: element {i} {lg[i]} vs {ref[i]} (bound {LOGIT_RTOL} x abs-chain {scale[i]})"
    near = orp.margin(ref) < 2 * bound.max(1)
    bad = np.flatnonzero(sym != orp.symbols(ref))
    assert np.all(near[bad]), f"{what}: symbols differ at points whose margin exceeds the rounding bound: {bad[~near[bad]][:5]}"
    assert bad.size <= 1e-4 * len(sym), f"{what}: {bad.size} symbol mismatches of {len(sym)}"
    assert np.all(sym < lg.shape[1]), f"{what}: symbol out of range"
    return ref


# ---- the envelope -----------------------------------------------------------------------------------------------------------
# (d, hidden widths, A, act, n, fp64, ldx): a cover of d {1..4}, depth {1, 2, 3}, widths {16, 64, 128, (32, 80, 16)},
# A {2, 3, 4, 5, 16}, every activation, fp32 / fp64, ldx = d or padded, n {1, 15, 16, 17, 1000, > one grid-stride pass}
CASES = {
    "d1_w16_a2_linear_n1_f32": (1, (16,), 2, "linear", 1, False, 1),
    "d2_w64_a3_relu_n15_f64_pad": (2, (64,), 3, "relu", 15, True, 3),
    "d3_w128_a4_leaky_n16_f32_pad": (3, (128,), 4, "leaky_relu", 16, False, 7),
    "d4_w16x16_a5_tanh_n17_f64": (4, (16, 16), 5, "tanh", 17, True, 4),
    "d2_w64x64_a16_tanh_n1000_f32_pad": (2, (64, 64), 16, "tanh", 1000, False, 5),
    "d1_w128x128_a2_leaky_n1000_f64": (1, (128, 128), 2, "leaky_relu", 1000, True, 1),
    "d3_w32x80x16_a5_relu_n1000_f32": (3, (32, 80, 16), 5, "relu", 1000, False, 3),
    "d4_w64x64x64_a4_linear_n17_f64_pad": (4, (64, 64, 64), 4, "linear", 17, True, 6),
    "d2_w128x128x128_a16_relu_n15_f32": (2, (128, 128, 128), 16, "relu", 15, False, 2),
    "d2_w16x16x16_a3_tanh_n1_f64_pad": (2, (16, 16, 16), 3, "tanh", 1, True, 4),
    "d1_w64_a16_tanh_n16_f32": (1, (64,), 16, "tanh", 16, False, 1),
    "d4_w32x80x16_a2_leaky_n15_f64_pad": (4, (32, 80, 16), 2, "leaky_relu", 15, True, 9),
    "d3_w64x64_a3_linear_n1000_f32_pad": (3, (64, 64), 3, "linear", 1000, False, 4),
    # more points than one grid-stride pass (256 CUs x 3 workgroups x 4 waves x 16 points = 49 152)
    "d2_w64x64x64_a4_tanh_n120003_f64": (2, (64, 64, 64), 4, "tanh", 120_003, True, 2),
    "d2_w64x64x64_a4_relu_n120003_f32_pad": (2, (64, 64, 64), 4, "relu", 120_003, False, 3),
}
for _k, _vals in [(0, {1, 2, 3, 4}), (2, {2, 3, 4, 5, 16}), (3, set(ACT)), (4, {1, 15, 16, 17, 1000}), (5, {True, False})]:
    assert {c[_k] for c in CASES.values()} >= _vals, (_k, _vals)
assert {len(c[1]) for c in CASES.values()} == {1, 2, 3}
assert {w for c in CASES.values() for w in c[1]} >= {16, 64, 128} and any(c[1] == (32, 80, 16) for c in CASES.values())


def _case(case):
    d, widths, A, act, n, f64, ldx = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    w = _weights(d, widths, A, rng)
    desc, params = _flat(w, d, act)
    x = _points(n, d, ldx, rng, f64)
    return w, desc, params, x, A, act, d


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_oracle_across_the_envelope(case):
    w, desc, params, x, A, act, d = _case(case)
    assert _lib_().dib_partition_supported(ctypes.byref(desc)) == 1
    c0 = np.arange(A, dtype=np.int64) * 1000 + 7
    sym, lg, cnt = _call(desc, params, x, A, counts0=c0)
    _check_against_oracle(w, act, x, d, sym, lg, case)
    assert np.array_equal(cnt - c0, np.bincount(sym, minlength=A)), "counts are added into the buffer: counts0 + bincount(sym)"
    # without logits: the same symbols and counts
    sym2, _, cnt2 = _call(desc, params, x, A, logits=False)
    assert np.array_equal(sym, sym2) and np.array_equal(cnt2, cnt - c0)


@pytest.mark.parametrize("case", ["d2_w64x64x64_a4_tanh_n120003_f64", "d4_w16x16_a5_tanh_n17_f64",
                                  "d2_w16x16x16_a3_tanh_n1_f64_pad", "d1_w128x128_a2_leaky_n1000_f64"])
def test_fp64_input_is_bit_identical_to_its_float32_cast(case):
    w, desc, params, x, A, act, d = _case(case)
    a = _call(desc, params, x, A)
    b = _call(desc, params, x.astype(np.float32), A)
    for u, v in zip(a, b):
        assert np.array_equal(u, v, equal_nan=True)


@pytest.mark.parametrize("case", ["d2_w64x64x64_a4_relu_n120003_f32_pad", "d2_w64x64x64_a4_tanh_n120003_f64"])
def test_runs_and_grids_are_bit_identical(case):
    """two runs, and dib_set_tuning("num_cus", 7) (many grid-stride passes per workgroup), give the same bits"""
    w, desc, params, x, A, act, d = _case(case)
    a = _call(desc, params, x, A)
    for b in (_call(desc, params, x, A), _call(desc, params, x, A, num_cus=7)):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_chunked_calls_equal_one_call_and_counts_accumulate():
    w, desc, params, x, A, act, d = _case("d2_w64x64x64_a4_tanh_n120003_f64")
    sym, lg, cnt = _call(desc, params, x, A)
    n, ldx = x.shape
    xd = torch.from_numpy(x).cuda()
    s2 = torch.full((n,), SENT_U8, dtype=torch.uint8, device="cuda")
    c2 = torch.zeros(A, dtype=torch.int64, device="cuda")
    lib, p = _lib_(), ctypes.c_void_p(params.data_ptr())
    edges = [0, 1, 17, 4113, 50_000, 50_001, 99_999, n]   # ragged chunk sizes, one of a single point
    for a, b in zip(edges[:-1], edges[1:]):
        _lib.check(lib.dib_partition_symbolize(ctypes.byref(desc), p, ctypes.c_void_p(xd[a:].data_ptr()), 1, ldx, b - a,
                                               ctypes.c_void_p(s2[a:].data_ptr()), None, ctypes.c_void_p(c2.data_ptr()),
                                               _stream()), "chunk")
    torch.cuda.synchronize()
    assert np.array_equal(s2.cpu().numpy(), sym)
    assert np.array_equal(c2.cpu().numpy(), cnt)
    # n == 0 launches nothing and changes nothing
    assert lib.dib_partition_symbolize(ctypes.byref(desc), p, ctypes.c_void_p(xd.data_ptr()), 1, ldx, 0,
                                       ctypes.c_void_p(s2.data_ptr()), None, ctypes.c_void_p(c2.data_ptr()), _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c2.cpu().numpy(), cnt)


# ---- ties, the magnitude rule, NaN ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,A,pairs", [("relu", 4, {3: 0, 2: 1}), ("tanh", 16, {5: 1, 14: 2, 10: 8, 13: 12, 7: 4})])
def test_duplicated_and_negated_columns_go_to_the_lower_index(act, A, pairs):
    """column c = column s (duplicate) or = -column s (|v| = |-v|), s < c, in other lane groups and the same one: exact ties
    that the first index must win"""
    rng = np.random.default_rng(A)
    for sign in (1.0, -1.0):
        w = _weights(2, (64, 64), A, rng)
        for c, s in pairs.items():
            w[-2][:, c], w[-1][c] = sign * w[-2][:, s], sign * w[-1][s]
        desc, params = _flat(w, 2, act)
        x = _points(20_000, 2, 2, rng, False)
        sym, lg, cnt = _call(desc, params, x, A)
        for c, s in pairs.items():
            assert np.array_equal(lg[:, c], sign * lg[:, s]), "the tied columns are bit-equal in magnitude"
        assert np.array_equal(sym, orp.symbols(lg)), "argmax |logit| of the kernel's own logits, the first index winning"
        assert not np.isin(sym, list(pairs)).any(), "a tie went to the later column"
        assert np.isin(sym, list(pairs.values())).any(), "no point chose a tied column: the case tests nothing"
        _check_against_oracle(w, act, x, 2, sym, lg, f"sign {sign}")


def test_all_zero_output_layer_gives_symbol_zero():
    rng = np.random.default_rng(3)
    w = _weights(3, (64,), 5, rng)
    w[-2][:], w[-1][:] = 0.0, 0.0
    desc, params = _flat(w, 3, "tanh")
    sym, lg, cnt = _call(desc, params, _points(1000, 3, 3, rng, True), 5)
    assert not lg.any() and not sym.any()
    assert cnt.tolist() == [1000, 0, 0, 0, 0]


def test_magnitude_not_sign_decides():
    """logits (-2 v, v, v / 2): the magnitude argmax is 0 everywhere, the signed one is 1 wherever v > 0"""
    rng = np.random.default_rng(4)
    w = _weights(2, (64, 64), 3, rng)
    v = w[-2][:, 1].copy()
    w[-2][:, 0], w[-2][:, 2], w[-1][:] = -2.0 * v, 0.5 * v, 0.0
    desc, params = _flat(w, 2, "relu")
    sym, lg, cnt = _call(desc, params, _points(5000, 2, 2, rng, False), 3)
    assert np.array_equal(lg[:, 0], -2.0 * lg[:, 1])
    assert (np.argmax(lg, 1) != 0).mean() > 0.05, "the signed argmax must differ somewhere for the case to mean anything"
    assert not sym.any(), "argmax of |logit|"


def test_nan_logits_never_win():
    rng = np.random.default_rng(5)
    w = _weights(2, (16,), 4, rng)
    w[-2][:, 0] = np.nan
    desc, params = _flat(w, 2, "leaky_relu")
    x = _points(3000, 2, 2, rng, False)
    sym, lg, cnt = _call(desc, params, x, 4)
    assert np.isnan(lg[:, 0]).all()
    assert np.array_equal(sym, 1 + orp.symbols(lg[:, 1:])), "NaN ranks below every magnitude"
    w[-2][:] = np.nan
    desc, params = _flat(w, 2, "leaky_relu")
    sym, lg, cnt = _call(desc, params, x, 4)
    assert not sym.any() and cnt.tolist() == [3000, 0, 0, 0], "all NaN -> symbol 0"


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _desc(in_dim=4, n_hidden=3, width=(128, 128, 128, 16), act=3, n_freq=1):
    d = _MlpDesc()
    for l in range(4):
        d.w_off[l], d.b_off[l], d.width[l] = 0, 0, width[l] if l < len(width) else 0
    d.n_hidden, d.in_dim, d.n_freq, d.act = n_hidden, in_dim, n_freq, act
    return d


OUTSIDE = {"in_dim0": dict(in_dim=0), "in_dim5": dict(in_dim=5), "n_freq2": dict(n_freq=2), "depth0": dict(n_hidden=0),
           "depth4": dict(n_hidden=4, width=(16, 16, 16, 16)), "width8": dict(width=(8, 128, 128, 16)),
           "width24": dict(width=(128, 24, 128, 16)), "width144": dict(width=(128, 128, 144, 16)), "A1": dict(width=(128, 128, 128, 1)),
           "A17": dict(width=(128, 128, 128, 17)), "sigmoid": dict(act=4), "leaky01": dict(act=7), "negative_act": dict(act=-1)}


def _refused(d, code, n=64, ldx=4, null=None):
    params = torch.zeros(200_000, device="cuda")
    x = torch.zeros(4096, device="cuda")
    sym = torch.full((4096,), SENT_U8, dtype=torch.uint8, device="cuda")
    lg = torch.full((1 << 16,), float("nan"), device="cuda")
    cnt = torch.full((32,), SENT_I64, dtype=torch.int64, device="cuda")
    ptr = {k: ctypes.c_void_p(t.data_ptr()) for k, t in dict(params=params, x=x, sym=sym, lg=lg, cnt=cnt).items()}
    if null:
        ptr[null] = None
    got = _lib_().dib_partition_symbolize(ctypes.byref(d), ptr["params"], ptr["x"], 0, ldx, n, ptr["sym"], ptr["lg"], ptr["cnt"],
                                          _stream())
    torch.cuda.synchronize()
    assert got == code, got
    assert bool((sym == SENT_U8).all()) and bool(torch.isnan(lg).all()) and bool((cnt == SENT_I64).all()), "a refused call wrote"


@pytest.mark.parametrize("name", list(OUTSIDE))
def test_shapes_outside_the_envelope_are_refused_without_a_launch(name):
    lib = _lib_()
    assert lib.dib_partition_supported(ctypes.byref(_desc())) == 1
    d = _desc(**OUTSIDE[name])
    assert lib.dib_partition_supported(ctypes.byref(d)) == 0
    _refused(d, DIB_E_UNSUPPORTED)


@pytest.mark.parametrize("what", ["n_negative", "ldx_below_in_dim", "params", "x", "sym"])
def test_bad_arguments_are_refused_without_a_launch(what):
    if what == "n_negative":
        _refused(_desc(), DIB_E_ARG, n=-1)
    elif what == "ldx_below_in_dim":
        _refused(_desc(), DIB_E_ARG, ldx=3)
    else:
        _refused(_desc(), DIB_E_ARG, null=what)


def test_model_refuses_outside_the_envelope():
    with pytest.raises(ValueError, match="envelope"):
        rp.RandomPartition(2, 4, 2, "sigmoid")
    with pytest.raises(ValueError, match="envelope"):
        rp.RandomPartition(2, 17, 2, "relu")
    with pytest.raises(ValueError, match="envelope"):
        rp.RandomPartition(5, 4, 2, "relu")


# ---- RandomPartition ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ikeda():
    return chaos_data.generate_data("ikeda", 200_000, 10_000, seed=0)


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_notebook_configurations_match_the_oracle(ikeda, A, N, act):
    part = rp.RandomPartition(2, A, N, act, seed=100 * A + 10 * N + len(act))
    w = part.get_weights()
    assert all(np.array_equal(u, v) for u, v in zip(w, rp.draw_weights(2, A, N, seed=100 * A + 10 * N + len(act))))
    sym, counts = part.symbolize(ikeda, chunk_size=70_001, return_counts=True)
    assert sym.dtype == np.uint8 and sym.shape == (len(ikeda),)
    lg = part.logits(ikeda)
    _check_against_oracle(w, act, ikeda, 2, sym, lg, f"A{A} N{N} {act}")
    assert np.array_equal(counts, np.bincount(sym, minlength=A))
    assert np.array_equal(part.symbolize(ikeda.astype(np.float32)), sym), "float32 input of the cast trajectory: same bits"
    assert np.array_equal(part.symbolize(torch.from_numpy(ikeda).cuda()), sym), "device input"


def test_set_weights_round_trip_and_one_dimensional_input():
    part = rp.RandomPartition(1, 2, 1, "linear", units_per_mlp_layer=16, weights=orp.generating_partition_weights())
    assert all(np.array_equal(u, v) for u, v in zip(part.get_weights(), orp.generating_partition_weights()))
    x = np.array([0.1, 0.49, 0.51, 0.9])
    assert part.symbolize(x).tolist() == [1, 1, 0, 0]


def test_logistic_generating_partition_known_answer():
    """the CPU known answer (tests/test_random_partition_oracle.py) through the kernel: symbols equal the oracle's except where
    |o0| and |o1| are within 1e-6 (x within ~5e-7 of 0.5), and the entropy rate is the notebook's 0.5203 within 0.003 bits"""
    x = orp.logistic_trajectory(2_000_000)
    w = orp.generating_partition_weights()
    part = rp.RandomPartition(1, 2, 1, "linear", units_per_mlp_layer=16, weights=w)
    sym, counts = part.symbolize(x, return_counts=True)
    ref = orp.forward(w, x, "linear")
    near = orp.margin(ref) < 1e-6
    assert near.sum() <= 10
    assert np.array_equal(sym[~near], orp.symbols(ref)[~near])
    ndp = np.logspace(np.log10(2000), np.log10(1_000_000), 15, dtype=np.int32)
    r = part.characterize(sym, number_data_points=ndp)
    assert r["entropy_single_timestep"] == orp.compute_entropy(sym)
    assert abs(r["entropy_rate"] - 0.5203) <= 0.003, r["entropy_rate"]
    r2 = part.characterize(x[:400_000], number_data_points=[2000, 8000, 30000, 100_000, 300_000], number_rand_draws=3)
    assert r2["entropy_single_timestep"] == orp.compute_entropy(sym[:400_000]), "H(U) from the kernel's counts"


def test_survey_on_a_short_trajectory(ikeda, tmp_path):
    """the skip rule, the records and the npz files of cell 7 through the kernel; every h <= H(U) + 0.02 + 3 err (the fit's
    error with slack for the short windows)"""
    ndp = [2000, 5000, 12_000, 30_000, 80_000, 190_000]
    recs = rp.random_partition_survey(ikeda, seed=3, number_data_points=ndp, number_rand_draws=3, out_dir=str(tmp_path))
    assert len(recs) == 12
    for r in recs:
        w = rp.draw_weights(2, r["alphabet_size"], r["number_mlp_layers"], seed=r["seed"])
        sym = rp.RandomPartition(2, r["alphabet_size"], r["number_mlp_layers"], r["activation"], weights=w).symbolize(ikeda)
        assert r["entropy_single_timestep"] == orp.compute_entropy(sym)
        assert r["skipped"] == (r["entropy_single_timestep"] < 0.1)
        if r["skipped"]:
            assert r["file"] is None and r["entropy_rate"] is None
            continue
        assert r["entropy_rate"] <= r["entropy_single_timestep"] + 0.02 + 3 * r["entropy_rate_err"], r
        z = np.load(r["file"])
        assert sorted(z.files) == ["entropy_rate", "entropy_rate_err", "entropy_rate_values", "entropy_single_timestep"]
        assert float(z["entropy_rate"]) == r["entropy_rate"]
    assert any(not r["skipped"] for r in recs)
    all_skipped = rp.random_partition_survey(ikeda[:20_000], alphabet_sizes=(2,), layer_counts=(1,), entropy_threshold=10.0,
                                             out_dir=str(tmp_path / "none"))
    assert [r["skipped"] for r in all_skipped] == [True, True]
    assert not list((tmp_path / "none").iterdir())
