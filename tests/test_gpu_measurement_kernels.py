"""The four measurement-partition kernels (include/dib_measure.h) called one by one through the C ABI on device buffers, without
MeasurementIB, against the float64 restatement of the header's contract (tests/_oracle_measurement.py measure_fwd,
measure_bwd, vq_logits, posenc_rows), across the envelope: both embedding tiles and partial noise groups (E), logits in
every lane group (A), all three hidden activations, every VQ width class, L from 1 to 32, ragged row tails and more rows
than one pass of the grid-stride loops.  Every output is allocated with a guard region past its last row, filled with a
NaN / sentinel pattern that must survive the launch, and the valid part is NaN-filled before it, so that a row or a feature
the kernel does not write shows up as a NaN."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _oracle_measurement as om
from dib_amd import _lib
from dib_amd._gemm_plan import _ptr
from dib_amd.measurement import MeasurementIB, _MeasureDesc

pytestmark = pytest.mark.gpu

ACT = {"linear": 0, "relu": 1, "leaky_relu": 2}
SLOPE = {0: 1.0, 1: 0.0, 2: 0.2}
GUARD_ROWS = 17
SENTINEL_I32 = -123456789
SENTINEL_U8 = 0xA5
SEED, STEP = 0x1234_5678_9ABC, 77
DIB_E_ARG, DIB_E_UNSUPPORTED = -1, -4   # include/dib_hip.h


def _lib_():
    return _lib.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _desc(E, A, H1, H2, L, act, in_dim=2, offs=None):
    d = _MeasureDesc()
    d.in_dim, d.E, d.H1, d.H2, d.A, d.L, d.act = in_dim, E, H1, H2, A, L, act
    for l in range(3):
        d.w_off[l], d.b_off[l] = offs[l] if offs else (0, 0)
    return d


def _vq(E, A, H1, H2, rng, dup=None):
    """random VQ weights [W1, b1, W2, b2, W3, b3] (float32, glorot-uniform kernels) and the flat parameter buffer with the
    layers at unaligned, interleaved offsets.  dup {copy: source}: logit column `copy` repeats column `source` exactly."""
    ws = []
    for i, o in [(E, H1), (H1, H2), (H2, A)]:
        lim = np.sqrt(6.0 / (i + o))
        ws += [rng.uniform(-lim, lim, (i, o)).astype(np.float32), (0.3 * rng.standard_normal(o)).astype(np.float32)]
    for c, s in (dup or {}).items():
        ws[4][:, c], ws[5][c] = ws[4][:, s], ws[5][s]
    offs, flat, o = [], [np.full(3, np.nan, np.float32)], 3
    for l in range(3):
        w, b = ws[2 * l], ws[2 * l + 1]
        offs.append((o, o + w.size + 1))
        flat += [w.ravel(), np.full(1, np.nan, np.float32), b, np.full(2, np.nan, np.float32)]
        o += w.size + 1 + b.size + 2
    return ws, torch.from_numpy(np.concatenate(flat)).cuda(), offs


def _enc(rows, E, rng):
    mu = 0.8 * rng.standard_normal((rows, E))
    lv = rng.uniform(-1.5, 0.5, (rows, E))
    return np.concatenate([mu, lv], 1).astype(np.float32)


def _guarded(rows, cols, dtype=torch.float32):
    """(buffer, view of its first rows): the whole buffer NaN / sentinel-filled, GUARD_ROWS rows of guard past the view"""
    fill = {torch.float32: float("nan"), torch.int32: SENTINEL_I32, torch.uint8: SENTINEL_U8}[dtype]
    buf = torch.full(((rows + GUARD_ROWS) * cols,), fill, dtype=dtype, device="cuda")
    return buf, buf[: rows * cols].view(rows, cols)


def _guard_intact(buf, rows, cols, what):
    g = buf[rows * cols:]
    ok = bool(torch.isnan(g).all()) if g.dtype == torch.float32 else bool((g == (SENTINEL_I32 if g.dtype == torch.int32
                                                                                   else SENTINEL_U8)).all())
    assert ok, f"{what}: the guard region past row {rows} was written"


def _no_nan(view, what):
    assert not bool(torch.isnan(view).any()), f"{what}: NaN in the output (an element left unwritten or computed as NaN)"


def _close(got, ref, what, rtol=1e-4, floor=1e-5):
    """per element: |got - ref| <= rtol |ref| + floor * max|ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = rtol * np.abs(ref) + floor * max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref)
    i = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{what}: element {i} {got[i]} vs {ref[i]} (bound {rtol} |ref| + {floor} max|ref|)"


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


# ---- training forward / backward ---------------------------------------------------------------------------------------
# (E, A, (H1, H2), act, L, B, kl exponent p, agg_width): a pairwise cover of E {1, 3, 5, 16, 17, 32}, A {2, 4, 5, 16}, VQ widths
# {16x16, 16x128, 112x48, 128x128}, act {linear, relu, leaky_relu}, L {1, 7, 32}, rows below 16 / ragged / more than one pass of
# the forward's 256 x 8 x 16 = 32 768-row grid, p {0.5, 1, 2} and aggregator widths {1, 37, 256}
CASES = {
    "e1_a2_h16x16_linear_l1_rows5": (1, 2, (16, 16), "linear", 1, 5, 0.5, 1),
    "e3_a4_h16x128_relu_l7_rows91": (3, 4, (16, 128), "relu", 7, 13, 1.0, 37),
    "e5_a5_h112x48_leaky_l32_rows224": (5, 5, (112, 48), "leaky_relu", 32, 7, 2.0, 256),
    "e16_a16_h128x128_linear_l7_rows35": (16, 16, (128, 128), "linear", 7, 5, 2.0, 37),
    "e17_a5_h16x16_relu_l1_rows1000": (17, 5, (16, 16), "relu", 1, 1000, 0.5, 256),
    "e32_a16_h112x48_relu_l32_rows96": (32, 16, (112, 48), "relu", 32, 3, 1.0, 1),
    "e32_a2_h128x128_leaky_l7_rows63": (32, 2, (128, 128), "leaky_relu", 7, 9, 0.5, 37),
    "e17_a4_h16x128_linear_l32_rows64": (17, 4, (16, 128), "linear", 32, 2, 2.0, 1),
    "e3_a16_h16x16_leaky_l1_rows1": (3, 16, (16, 16), "leaky_relu", 1, 1, 1.0, 256),
    "e5_a2_h128x128_relu_l7_rows119": (5, 2, (128, 128), "relu", 7, 17, 2.0, 1),
    "e1_a16_h112x48_linear_l32_rows32": (1, 16, (112, 48), "linear", 32, 1, 0.5, 37),
    "e16_a4_h16x16_relu_l32_rows480": (16, 4, (16, 16), "relu", 32, 15, 1.0, 256),
    # more rows than one pass of the forward's grid (and of the backward's: one workgroup per CU)
    "e5_a5_h16x16_leaky_l13_rows35503": (5, 5, (16, 16), "leaky_relu", 13, 2731, 2.0, 37),
    "e17_a16_h16x16_linear_l13_rows35503": (17, 16, (16, 16), "linear", 13, 2731, 0.5, 1),
}
for _k, _vals in enumerate([{1, 3, 5, 16, 17, 32}, {2, 4, 5, 16}, {(16, 16), (16, 128), (112, 48), (128, 128)},
                            set(ACT), {1, 7, 32}, None, {0.5, 1.0, 2.0}, {1, 37, 256}]):
    assert _vals is None or {c[_k] for c in CASES.values()} >= _vals, (_k, _vals)


def _fwd(case, num_cus=None):
    """run dib_measure_fwd on the case's inputs (deterministic per case); host copies of every output and the guard checks"""
    E, A, (H1, H2), act, L, B, p, _ = CASES[case]
    rows = B * L
    rng = np.random.default_rng(sum(map(ord, case)))
    ws, params, offs = _vq(E, A, H1, H2, rng)
    enc = _enc(rows, E, rng)
    d = _desc(E, A, H1, H2, L, ACT[act], offs=offs)
    lib = _lib_()
    assert lib.dib_measure_supported(ctypes.byref(d)) == 1
    outs = {k: _guarded(rows, c) for k, c in [("z", E), ("h1", H1), ("h2", H2), ("soft", A)]}
    out3 = _guarded(1, 3)
    ws_dev = torch.zeros(int(lib.dib_measure_workspace_bytes(ctypes.byref(d), rows)) // 4 + 1, dtype=torch.float32, device="cuda")
    enc_dev = torch.from_numpy(enc).cuda()
    beta = 0.37
    old = _lib.get_tuning("num_cus")
    try:
        if num_cus is not None:
            _lib.set_tuning("num_cus", num_cus)
        _lib.check(lib.dib_measure_fwd(ctypes.byref(d), _ptr(params), _ptr(enc_dev), rows, SEED, STEP, beta, p,
                                       *[_ptr(outs[k][1]) for k in ("z", "h1", "h2", "soft")], _ptr(out3[1]), _ptr(ws_dev),
                                       _stream()), "dib_measure_fwd")
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning("num_cus", old)
    for k, (buf, view) in list(outs.items()) + [("out3", out3)]:
        _guard_intact(buf, 1 if k == "out3" else rows, view.shape[1], f"fwd {k}")
        _no_nan(view, f"fwd {k}")
    res = {k: v[1].cpu().numpy() for k, v in outs.items()}
    res["out3"] = out3[1].cpu().numpy().ravel()
    return dict(ws=ws, params=params, offs=offs, enc=enc, d=d, beta=beta, res=res)


@functools.lru_cache(maxsize=None)
def _fwd_cached(case):
    return _fwd(case)


def _bwd(case, num_cus=None):
    E, A, (H1, H2), act, L, B, p, HA = CASES[case]
    rows = B * L
    f = _fwd_cached(case)
    rng = np.random.default_rng(sum(map(ord, case)) + 1)
    g_agg = rng.standard_normal((B, HA)).astype(np.float32)
    w_agg0 = (rng.standard_normal((L * A, HA)) / np.sqrt(HA)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    outs = {k: _guarded(rows, c) for k, c in [("g3", A), ("g2", H2), ("g1", H1), ("g_enc", 2 * E)]}
    lib = _lib_()
    old = _lib.get_tuning("num_cus")
    args = [dev(f["enc"]), dev(f["res"]["h1"]), dev(f["res"]["h2"]), dev(f["res"]["soft"]), dev(g_agg), dev(w_agg0),
            dev(f["res"]["out3"])]
    try:
        if num_cus is not None:
            _lib.set_tuning("num_cus", num_cus)
        _lib.check(lib.dib_measure_bwd(ctypes.byref(f["d"]), _ptr(f["params"]), _ptr(args[0]), rows, SEED, STEP, _ptr(args[1]),
                                       _ptr(args[2]), _ptr(args[3]), _ptr(args[4]), _ptr(args[5]), HA, _ptr(args[6]),
                                       *[_ptr(outs[k][1]) for k in ("g3", "g2", "g1", "g_enc")], _stream()), "dib_measure_bwd")
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning("num_cus", old)
    for k, (buf, view) in outs.items():
        _guard_intact(buf, rows, view.shape[1], f"bwd {k}")
        _no_nan(view, f"bwd {k}")
    return dict(f=f, g_agg=g_agg, w_agg0=w_agg0, res={k: v[1].cpu().numpy() for k, v in outs.items()})


@pytest.mark.parametrize("case", list(CASES))
def test_fwd_matches_oracle(case):
    E, A, _, act, L, B, p, _ = CASES[case]
    f = _fwd_cached(case)
    z, h1, h2, soft, out3 = om.measure_fwd(f["ws"], f["enc"], SEED, STEP, np.float32(f["beta"]), p, L, SLOPE[ACT[act]])
    r = f["res"]
    _close(r["z"], z, "z")
    _close(r["h1"], h1, "h1 (post-activation)")
    _close(r["h2"], h2, "h2 (post-activation)")
    _close(r["soft"], soft, "softmax")
    np.testing.assert_allclose(r["soft"].sum(1), 1.0, rtol=0, atol=1e-5, err_msg="softmax rows sum to 1 (bound 1e-5)")
    for i, what in enumerate(["kl", "beta L kl^p", "p beta L kl^(p-1) / rows"]):
        assert abs(r["out3"][i] - out3[i]) <= 1e-5 * abs(out3[i]), (what, r["out3"][i], out3[i], "bound 1e-5 relative")


@pytest.mark.parametrize("case", list(CASES))
def test_bwd_matches_oracle(case):
    E, A, _, act, L, B, p, _ = CASES[case]
    b = _bwd(case)
    f = b["f"]
    ref = om.measure_bwd(f["ws"], f["enc"], SEED, STEP, f["res"]["h1"], f["res"]["h2"], f["res"]["soft"], b["g_agg"],
                         b["w_agg0"], float(f["res"]["out3"][2]), L, SLOPE[ACT[act]])
    for k, rv in zip(["g3", "g2", "g1", "g_enc"], ref):
        assert np.linalg.norm(rv) > 0, (k, "degenerate case: the reference gradient is zero")
        assert _rel(b["res"][k], rv) <= 1e-4, (k, _rel(b["res"][k], rv), "bound 1e-4 norm-relative")


@pytest.mark.parametrize("case", ["e5_a5_h16x16_leaky_l13_rows35503", "e32_a16_h112x48_relu_l32_rows96",
                                  "e17_a5_h16x16_relu_l1_rows1000"])
def test_fwd_and_bwd_bits_do_not_depend_on_the_grid(case):
    """dib_set_tuning("num_cus", 7): the forward's grid (and its KL summation order) is a function of the row count alone; the
    backward's one workgroup per CU then loops many times over the row tiles - the same bits either way"""
    a, b = _fwd_cached(case), _fwd(case, num_cus=7)
    for k in a["res"]:
        assert np.array_equal(a["res"][k], b["res"][k]), ("fwd", k)
    x, y = _bwd(case), _bwd(case, num_cus=7)
    for k in x["res"]:
        assert np.array_equal(x["res"][k], y["res"][k]), ("bwd", k)


# ---- symbolisation ------------------------------------------------------------------------------------------------------
# (E, A, (H1, H2), act, n, K, dup): A {2, 3, 5, 16} x K {1, 7, 100}; dup {copy: source} makes logit column `copy` an exact
# copy of an earlier column, in another lane group (5 <- 1 ...) or the same one (10 <- 8): exact ties, which the first index wins
SYM_CASES = {
    "e8_a2_k100_h128x128_leaky_n1037": (8, 2, (128, 128), "leaky_relu", 1037, 100, {}),
    "e3_a3_k7_h16x128_relu_n5": (3, 3, (16, 128), "relu", 5, 7, {}),
    "e17_a5_k1_h112x48_linear_n4000": (17, 5, (112, 48), "linear", 4000, 1, {4: 0}),
    "e32_a16_k100_h112x48_relu_n523": (32, 16, (112, 48), "relu", 523, 100, {5: 1, 14: 2, 10: 8, 13: 12}),
    "e5_a5_k100_h128x128_leaky_n301": (5, 5, (128, 128), "leaky_relu", 301, 100, {4: 1}),
    "e16_a16_k7_h16x16_leaky_n40000": (16, 16, (16, 16), "leaky_relu", 40000, 7, {7: 3, 9: 0}),
    "e1_a3_k1_h16x16_linear_n33": (1, 3, (16, 16), "linear", 33, 1, {}),
    "e17_a2_k7_h112x48_relu_n2000": (17, 2, (112, 48), "relu", 2000, 7, {}),
}
for _k, _vals in [(1, {2, 3, 5, 16}), (5, {1, 7, 100})]:
    assert {c[_k] for c in SYM_CASES.values()} >= _vals


def _symbolize(case, num_cus=None):
    E, A, (H1, H2), act, n, K, dup = SYM_CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    ws, params, offs = _vq(E, A, H1, H2, rng, dup)
    enc = _enc(n, E, rng)
    noise = rng.standard_normal((K, E)).astype(np.float32)
    d = _desc(E, A, H1, H2, 12, ACT[act], offs=offs)
    sym = _guarded(n, 1, torch.uint8)
    counts = _guarded(n, A, torch.int32)
    lib = _lib_()
    enc_dev, noise_dev = torch.from_numpy(enc).cuda(), torch.from_numpy(noise).cuda()
    old = _lib.get_tuning("num_cus")
    try:
        if num_cus is not None:
            _lib.set_tuning("num_cus", num_cus)
        _lib.check(lib.dib_measure_symbolize(ctypes.byref(d), _ptr(params), _ptr(enc_dev), n, _ptr(noise_dev), K, _ptr(sym[1]),
                                             _ptr(counts[1]), _stream()), "dib_measure_symbolize")
        torch.cuda.synchronize()
    finally:
        _lib.set_tuning("num_cus", old)
    _guard_intact(sym[0], n, 1, "sym")
    _guard_intact(counts[0], n, A, "counts")
    s, c = sym[1].cpu().numpy().ravel(), counts[1].cpu().numpy()
    assert np.all(s <= 1), "sym: unwritten points"
    assert np.all(c >= 0), "counts: unwritten entries"
    return dict(ws=ws, enc=enc, noise=noise, sym=s, counts=c)


@pytest.mark.parametrize("case", list(SYM_CASES))
def test_symbolize_matches_oracle(case):
    E, A, _, act, n, K, dup = SYM_CASES[case]
    r = _symbolize(case)
    lg = om.vq_logits(r["ws"], r["enc"][:, :E], r["enc"][:, E:], r["noise"], SLOPE[ACT[act]])   # [K, n, A]
    # exact ties between a column and its copy go to the first index (NumPy argmax): the reference argmax runs over the
    # distinct columns, sources before their copies
    uniq = np.array([a for a in range(A) if a not in dup])
    lu = lg[..., uniq]
    am = uniq[np.argmax(lu, -1)]                                                   # [K, n]
    # near-ties between distinct columns (top two within 3e-6 of the draw's largest |logit|) are where fp32 and fp64 may disagree
    top2 = np.sort(lu, -1)[..., -2:]
    near = np.any(top2[..., 1] - top2[..., 0] < 3e-6 * np.abs(lg).max(-1), axis=0)
    assert near.mean() <= 1e-3, (near.mean(), "near-tie exclusions above 0.1 %")
    ref_counts = np.stack([(am == a).sum(0) for a in range(A)], 1)
    ref_sym = np.uint8(np.mean(am, 0) > 0.5)                                     # the reference rule for every A
    bad = np.flatnonzero(~near & np.any(r["counts"] != ref_counts, 1))
    assert bad.size == 0, (f"counts differ at {bad.size} points", bad[:5], r["counts"][bad[:3]], ref_counts[bad[:3]])
    assert np.array_equal(r["sym"][~near], ref_sym[~near]), "sym vs mean(argmax) > 0.5"
    assert r["counts"].sum(1).tolist() == [K] * n, "counts of a point sum to K"
    # sym restates the counts on every point, near-ties included
    assert np.array_equal(r["sym"], np.uint8(2 * (r["counts"] * np.arange(A)).sum(1) > K))
    if dup:   # the copies never win
        assert not r["counts"][:, list(dup)].any(), "a tie went to the later column"
        assert r["counts"][:, [dup[c] for c in dup]].any(), "no draw chose a duplicated column"


def test_symbolize_bits_do_not_depend_on_the_grid():
    case = "e16_a16_k7_h16x16_leaky_n40000"
    a, b = _symbolize(case), _symbolize(case, num_cus=7)
    assert np.array_equal(a["sym"], b["sym"]) and np.array_equal(a["counts"], b["counts"])


# ---- positional encoding of gathered rows -------------------------------------------------------------------------------
@pytest.mark.parametrize("first_exponent", [-2, 0, 1])
@pytest.mark.parametrize("n_freq", [1, 11])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_posenc_rows_matches_oracle(d, n_freq, first_exponent):
    rng = np.random.default_rng(100 * d + 10 * n_freq + first_exponent)
    ldx, nx, n = d + 3, 50, 77
    x = rng.uniform(-3, 3, (nx, ldx)).astype(np.float32)
    idx = rng.integers(0, nx, n).astype(np.int32)             # gathered, unsorted, repeated
    idx[:3] = [nx - 1, 0, nx - 1]
    out = _guarded(n, d * n_freq)
    xd, idd = torch.from_numpy(x).cuda(), torch.from_numpy(idx).cuda()
    _lib.check(_lib_().dib_measure_posenc_rows(_ptr(xd), ldx, _ptr(idd), n, d, n_freq, first_exponent, _ptr(out[1]), _stream()),
               "dib_measure_posenc_rows")
    torch.cuda.synchronize()
    _guard_intact(out[0], n, d * n_freq, "posenc")
    _no_nan(out[1], "posenc")
    ref = om.posenc_rows(x, idx, d, n_freq, first_exponent)
    got = out[1].cpu().numpy()
    assert np.array_equal(got[:, :d], x[idx, :d]), "block 0 is x itself"
    assert np.abs(got - ref).max() <= 1e-6, (np.abs(got - ref).max(), "bound 1e-6 absolute")


# ---- the envelope -------------------------------------------------------------------------------------------------------
INSIDE = dict(E=32, A=16, H1=128, H2=128, L=32, act=2, in_dim=4)
OUTSIDE = {"E33": dict(E=33), "A1": dict(A=1), "A17": dict(A=17), "L33": dict(L=33), "in_dim5": dict(in_dim=5),
           "H1_136": dict(H1=136), "H2_136": dict(H2=136), "H1_24": dict(H1=24), "H2_24": dict(H2=24), "tanh": dict(act=3)}


@pytest.mark.parametrize("name", list(OUTSIDE))
def test_shapes_outside_the_envelope_are_refused_without_a_launch(name):
    lib = _lib_()
    ok = _desc(**INSIDE)
    assert lib.dib_measure_supported(ctypes.byref(ok)) == 1
    d = _desc(**{**INSIDE, **OUTSIDE[name]})
    assert lib.dib_measure_supported(ctypes.byref(d)) == 0
    assert lib.dib_measure_workspace_bytes(ctypes.byref(d), 64) == DIB_E_UNSUPPORTED
    params = torch.zeros(200_000, device="cuda")
    buf = torch.full((1 << 16,), float("nan"), device="cuda")
    p, q = _ptr(params), _ptr(buf)
    st = _stream()
    assert lib.dib_measure_fwd(ctypes.byref(d), p, p, 32, 0, 0, 1.0, 2.0, q, q, q, q, q, q, st) == DIB_E_UNSUPPORTED
    assert lib.dib_measure_bwd(ctypes.byref(d), p, p, 32, 0, 0, p, p, p, p, p, 8, p, q, q, q, q, st) == DIB_E_UNSUPPORTED
    assert lib.dib_measure_symbolize(ctypes.byref(d), p, p, 32, p, 4, q, q, st) == DIB_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote its outputs"


def test_bwd_refuses_rows_not_a_multiple_of_L():
    lib = _lib_()
    d = _desc(E=4, A=3, H1=16, H2=16, L=7, act=2, offs=[(0, 64), (80, 336), (352, 400)])
    params = torch.zeros(512, device="cuda")
    buf = torch.full((1 << 14,), float("nan"), device="cuda")
    p, q = _ptr(params), _ptr(buf)
    assert lib.dib_measure_bwd(ctypes.byref(d), p, p, 50, 0, 0, p, p, p, p, p, 8, p, q, q, q, q, _stream()) == DIB_E_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote its outputs"


def test_model_refuses_an_activation_outside_the_envelope():
    with pytest.raises(ValueError, match="envelope"):
        MeasurementIB(2, activation_function="tanh")
