"""The batched entry points behind MeasurementEnsemble, called through the C ABI on device buffers: dib_measure_fwd_batched /
dib_measure_bwd_batched (include/dib_measure.h) and dib_infonce_fwd_bwd_batched (include/dib_hip.h).

Each computes R independent problems in the launches of one, the replica being a grid index.  Checked per shape:
  * every output of replica r equals, bit for bit, what the single entry point writes when called on that replica's slices
    (its parameters, its seed) - the batched kernels run the same body text on moved pointers;
  * the float64 restatements (tests/_oracle_measurement.py measure_fwd / measure_bwd; the float64 InfoNCE of oracle/) at the
    tolerances of tests/test_gpu_measurement_kernels.py and tests/test_gpu_parity.py::test_infonce_loss_and_grads_match_oracle;
  * NaN guard bands before and after every output block survive, and no element inside is left unwritten (the ABI makes the
    replicas' slices contiguous, so the band between two slices has no width: a write across it would break the bit-equality
    of the neighbour's slice);
  * refused arguments launch nothing (dib_launch_count unchanged)."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import _oracle_measurement as om
import dib_oracle as orc
import dib_torch_cpu as tc
import test_gpu_measurement_kernels as mk
from dib_amd import _lib
from dib_amd._gemm_plan import _ptr
from dib_amd._lib import SIMILARITIES

pytestmark = pytest.mark.gpu

GUARD = 67                      # floats of NaN before and after every output block
STEP, BETA, P, HA = 77, 0.37, 1.5, 37
DIB_E_ARG, DIB_E_UNSUPPORTED = -1, -4


def _lib_():
    return _lib.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seeds(R, base=0x1234_5678_9ABC):
    return [base + 0x1_0000_0001 * r * r + 17 * r for r in range(R)]


def _u64(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


class _Block:
    """[R][rows][cols] floats, NaN-filled, between two NaN guard bands"""

    def __init__(self, R, rows, cols):
        self.n = R * rows * cols
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.view = self.buf[GUARD: GUARD + self.n].view(R, rows, cols)

    def check(self, what):
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all()), \
            f"{what}: a guard band around the replicas' slices was written"
        assert not bool(torch.isnan(self.view).any()), f"{what}: NaN inside (an element left unwritten)"
        return self.view.cpu().numpy()


# (rows per replica as (B, L), E, (H1, H2), A, act): the full product of the small shapes, and the tile loop's second trip
SHAPES = {"rows15": (3, 5), "rows35": (7, 5), "rows272": (34, 8)}
CASES = {f"r{R}_{s}_e{E}_h{H[0]}x{H[1]}_a{A}_{act}": (R, SHAPES[s], E, H, A, act)
         for R, s, E, H, A, act in itertools.product([1, 3], SHAPES, [4, 17], [(16, 32), (48, 64)], [2, 5], ["leaky_relu", "relu"])}
CASES["r3_rows32784_e4_h16x16_a2_leaky_relu"] = (3, (4098, 8), 4, (16, 16), 2, "leaky_relu")


def _setup(case):
    R, (B, L), E, (H1, H2), A, act = CASES[case]
    rows = B * L
    rng = np.random.default_rng(sum(map(ord, case)))
    reps = [mk._vq(E, A, H1, H2, rng) for _ in range(R)]          # distinct parameters; the same (unaligned) layer offsets
    offs = reps[0][2]
    size = int(reps[0][1].numel())
    stride = (size + 3) // 4 * 4 + 8                              # a multiple of 4 floats that is not the packed size
    params = torch.full((R * stride + 4,), float("nan"), dtype=torch.float32, device="cuda")
    for r in range(R):
        params[r * stride: r * stride + size].copy_(reps[r][1])
    enc = np.stack([mk._enc(rows, E, rng) for _ in range(R)])
    d = mk._desc(E, A, H1, H2, L, mk.ACT[act], offs=offs)
    assert _lib_().dib_measure_supported(ctypes.byref(d)) == 1
    g_agg = rng.standard_normal((R, B, HA)).astype(np.float32)
    wstride = L * A * HA + 12
    w_agg0 = np.full((R, wstride), np.nan, np.float32)
    w_agg0[:, : L * A * HA] = (rng.standard_normal((R, L * A * HA)) / np.sqrt(HA)).astype(np.float32)
    return dict(R=R, B=B, L=L, rows=rows, E=E, H1=H1, H2=H2, A=A, slope=mk.SLOPE[mk.ACT[act]], ws=[r[0] for r in reps],
                params=params, stride=stride, enc=enc, d=d, seeds=_seeds(R), g_agg=g_agg, w_agg0=w_agg0, wstride=wstride)


def _run_batched(c):
    lib, d, R, rows = _lib_(), c["d"], c["R"], c["rows"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc = dev(c["enc"])
    fo = {k: _Block(R, rows, w) for k, w in [("z", c["E"]), ("h1", c["H1"]), ("h2", c["H2"]), ("soft", c["A"])]}
    fo["out3"] = _Block(R, 1, 3)
    nws = int(lib.dib_measure_batched_workspace_bytes(ctypes.byref(d), rows, R))
    assert nws > 0
    ws = torch.zeros(nws // 4 + 1, dtype=torch.float32, device="cuda")
    n0 = lib.dib_launch_count()
    for _ in range(2):   # twice on one workspace: the last arriver of every replica re-armed its counter
        _lib.check(lib.dib_measure_fwd_batched(ctypes.byref(d), _ptr(c["params"]), c["stride"], _ptr(enc), rows, R, _u64(c["seeds"]),
                                               STEP, BETA, P, *[_ptr(fo[k].view) for k in ("z", "h1", "h2", "soft", "out3")],
                                               _ptr(ws), _stream()), "dib_measure_fwd_batched")
    assert lib.dib_launch_count() - n0 == 2, "one launch per call"
    torch.cuda.synchronize()
    fwd = {k: v.check(f"fwd {k}") for k, v in fo.items()}
    bo = {k: _Block(R, rows, w) for k, w in [("g3", c["A"]), ("g2", c["H2"]), ("g1", c["H1"]), ("g_enc", 2 * c["E"])]}
    g_agg, w_agg0 = dev(c["g_agg"]), dev(c["w_agg0"])
    n0 = lib.dib_launch_count()
    _lib.check(lib.dib_measure_bwd_batched(ctypes.byref(d), _ptr(c["params"]), c["stride"], _ptr(enc), rows, R, _u64(c["seeds"]), STEP,
                                           _ptr(fo["h1"].view), _ptr(fo["h2"].view), _ptr(fo["soft"].view), _ptr(g_agg),
                                           _ptr(w_agg0), c["wstride"], HA, _ptr(fo["out3"].view),
                                           *[_ptr(bo[k].view) for k in ("g3", "g2", "g1", "g_enc")], _stream()),
               "dib_measure_bwd_batched")
    assert lib.dib_launch_count() - n0 == 1
    torch.cuda.synchronize()
    return fwd, {k: v.check(f"bwd {k}") for k, v in bo.items()}


def _run_single(c, r):
    """the single entry points on replica r's slices with seeds[r]"""
    lib, d, rows = _lib_(), c["d"], c["rows"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    enc = dev(c["enc"][r])
    par = c["params"][r * c["stride"]:]
    fo = {k: _Block(1, rows, w) for k, w in [("z", c["E"]), ("h1", c["H1"]), ("h2", c["H2"]), ("soft", c["A"])]}
    fo["out3"] = _Block(1, 1, 3)
    ws = torch.zeros(int(lib.dib_measure_workspace_bytes(ctypes.byref(d), rows)) // 4 + 1, dtype=torch.float32, device="cuda")
    _lib.check(lib.dib_measure_fwd(ctypes.byref(d), _ptr(par), _ptr(enc), rows, c["seeds"][r], STEP, BETA, P,
                                   *[_ptr(fo[k].view) for k in ("z", "h1", "h2", "soft", "out3")], _ptr(ws), _stream()),
               "dib_measure_fwd")
    bo = {k: _Block(1, rows, w) for k, w in [("g3", c["A"]), ("g2", c["H2"]), ("g1", c["H1"]), ("g_enc", 2 * c["E"])]}
    g_agg, w_agg0 = dev(c["g_agg"][r]), dev(c["w_agg0"][r])
    _lib.check(lib.dib_measure_bwd(ctypes.byref(d), _ptr(par), _ptr(enc), rows, c["seeds"][r], STEP, _ptr(fo["h1"].view),
                                   _ptr(fo["h2"].view), _ptr(fo["soft"].view), _ptr(g_agg), _ptr(w_agg0), HA, _ptr(fo["out3"].view),
                                   *[_ptr(bo[k].view) for k in ("g3", "g2", "g1", "g_enc")], _stream()), "dib_measure_bwd")
    torch.cuda.synchronize()
    return {k: v.check(f"single fwd {k}")[0] for k, v in fo.items()}, {k: v.check(f"single bwd {k}")[0] for k, v in bo.items()}


@pytest.mark.parametrize("case", list(CASES))
def test_measure_batched_equals_the_single_kernels_and_the_oracle(case):
    c = _setup(case)
    fwd, bwd = _run_batched(c)
    L, slope = c["L"], c["slope"]
    for r in range(c["R"]):
        sf, sb = _run_single(c, r)
        for k in sf:
            assert np.array_equal(fwd[k][r], sf[k]), (r, "fwd", k, "batched != dib_measure_fwd on the replica's slices")
        for k in sb:
            assert np.array_equal(bwd[k][r], sb[k]), (r, "bwd", k, "batched != dib_measure_bwd on the replica's slices")
        # the float64 restatement, at the bounds of tests/test_gpu_measurement_kernels.py
        z, h1, h2, soft, out3 = om.measure_fwd(c["ws"][r], c["enc"][r], c["seeds"][r], STEP, np.float32(BETA), P, L, slope)
        mk._close(fwd["z"][r], z, "z")
        mk._close(fwd["h1"][r], h1, "h1")
        mk._close(fwd["h2"][r], h2, "h2")
        mk._close(fwd["soft"][r], soft, "softmax")
        o3 = fwd["out3"][r].ravel()
        for i in range(3):
            assert abs(o3[i] - out3[i]) <= 1e-5 * abs(out3[i]), (r, i, o3[i], out3[i], "bound 1e-5 relative")
        ref = om.measure_bwd(c["ws"][r], c["enc"][r], c["seeds"][r], STEP, fwd["h1"][r], fwd["h2"][r], fwd["soft"][r], c["g_agg"][r],
                             c["w_agg0"][r][: L * c["A"] * HA].reshape(L * c["A"], HA), float(o3[2]), L, slope)
        for k, rv in zip(["g3", "g2", "g1", "g_enc"], ref):
            assert np.linalg.norm(rv) > 0, (k, "degenerate case")
            assert mk._rel(bwd[k][r], rv) <= 1e-4, (r, k, mk._rel(bwd[k][r], rv), "bound 1e-4 norm-relative")
    if c["R"] > 1:   # distinct seeds and parameters reach the replicas
        assert not np.array_equal(fwd["z"][0], fwd["z"][1]) and not np.array_equal(fwd["soft"][0], fwd["soft"][1])


def test_measure_batched_refuses_bad_arguments_without_a_launch():
    lib = _lib_()
    c = _setup("r3_rows35_e4_h16x32_a2_relu")
    d, R, rows = c["d"], c["R"], c["rows"]
    buf = torch.full((1 << 16,), float("nan"), device="cuda")
    p, q, st, sd = _ptr(c["params"]), _ptr(buf), _stream(), _u64(c["seeds"])
    bad = mk._desc(c["E"], 17, c["H1"], c["H2"], c["L"], 2, offs=[(0, 0)] * 3)
    fwd = lambda d_=d, par=p, stride=c["stride"], rows_=rows, R_=R, seeds=sd: lib.dib_measure_fwd_batched(
        ctypes.byref(d_), par, stride, q, rows_, R_, seeds, 0, 1.0, 2.0, q, q, q, q, q, q, st)
    bwd = lambda d_=d, stride=c["stride"], rows_=rows, R_=R, seeds=sd, ws_=c["wstride"], ha=HA: lib.dib_measure_bwd_batched(
        ctypes.byref(d_), p, stride, q, rows_, R_, seeds, 0, q, q, q, q, q, ws_, ha, q, q, q, q, q, st)
    n0 = lib.dib_launch_count()
    assert fwd(d_=bad) == DIB_E_UNSUPPORTED and bwd(d_=bad) == DIB_E_UNSUPPORTED
    assert lib.dib_measure_batched_workspace_bytes(ctypes.byref(bad), rows, R) == DIB_E_UNSUPPORTED
    assert lib.dib_measure_batched_workspace_bytes(ctypes.byref(d), rows, 0) == DIB_E_UNSUPPORTED
    for kw in [dict(stride=c["stride"] + 2), dict(stride=-4), dict(R_=0), dict(rows_=0), dict(seeds=None)]:
        assert fwd(**kw) == DIB_E_ARG, kw
        assert bwd(**kw) == DIB_E_ARG, kw
    assert fwd(par=None) == DIB_E_ARG
    assert bwd(rows_=rows + 1) == DIB_E_ARG, "rows not a multiple of L"
    assert bwd(ha=0) == DIB_E_ARG and bwd(ws_=-1) == DIB_E_ARG
    assert lib.dib_launch_count() == n0, "a refused call launched"
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote its outputs"


# ---- InfoNCE ------------------------------------------------------------------------------------------------------------
# B: tile edges (64 | 65), both sides of the one-launch limit (128 | 129), 260 = five 64-row tiles: more than one partner slice
# and the final kernel; D: below / at a multiple of 4, above one 64-wide accumulator and not a multiple of 4
INCE_CASES = list(itertools.product([5, 64, 65, 128, 129, 260], [8, 32, 65], ["l2sq", "l2", "cosine"]))
INCE_R = 3


@functools.lru_cache(maxsize=None)
def _ince_data(B, D):
    """[3][B][D] embedding pairs scaled so that squared distances are O(1): the softmax is not saturated at T = 0.5"""
    rng = np.random.default_rng(1000 * B + D)
    a = (rng.standard_normal((INCE_R, B, D)) / np.sqrt(D)).astype(np.float32)
    b = (a + 0.7 * rng.standard_normal((INCE_R, B, D)) / np.sqrt(D)).astype(np.float32)
    return a, b


@functools.lru_cache(maxsize=None)
def _ince_oracle(B, D, kind, temp, r):
    a, b = _ince_data(B, D)
    loss, ga, gb = tc.infonce_loss_and_grads(a[r], b[r], kind, temp)
    ref = orc.infonce_loss(a[r], b[r], kind, temp)     # the NumPy restatement the autograd version is pinned on
    assert abs(loss - ref) <= 1e-12 * (1 + abs(ref))
    return ref, ga, gb


def _ince_single(a, b, kind, temp, grads):
    lib = _lib_()
    B, D = a.shape
    x, y = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    gx, gy, lo = _Block(1, B, D), _Block(1, B, D), _Block(1, 1, 1)
    ws = torch.zeros(int(lib.dib_infonce_workspace_bytes(B)) // 4 + 1, dtype=torch.float32, device="cuda")
    n0 = lib.dib_launch_count()
    _lib.check(lib.dib_infonce_fwd_bwd(_ptr(x), _ptr(y), B, D, SIMILARITIES[kind], temp, _ptr(gx.view) if grads else None,
                                       _ptr(gy.view) if grads else None, _ptr(lo.view), _ptr(ws), _stream()), "dib_infonce_fwd_bwd")
    n = lib.dib_launch_count() - n0
    torch.cuda.synchronize()
    return (float(lo.check("loss").ravel()[0]), gx.check("g_x")[0] if grads else None, gy.check("g_y")[0] if grads else None, n)


@pytest.mark.parametrize("B,D,kind", INCE_CASES, ids=[f"b{B}_d{D}_{k}" for B, D, k in INCE_CASES])
def test_infonce_batched_equals_the_single_entry_point_and_the_oracle(B, D, kind):
    _ince_check(B, D, kind, itertools.product([1.0, 0.5], [True, False]))


# the gradient kernel's three- and four-accumulator instantiations (129 <= D <= 256), which the shapes above do not reach
@pytest.mark.parametrize("D", [130, 256])
@pytest.mark.parametrize("kind", ["l2sq", "l2", "cosine"])
def test_infonce_batched_wide_embeddings(kind, D):
    _ince_check(129, D, kind, [(0.5, True)])


def _ince_check(B, D, kind, combos):
    lib = _lib_()
    a, b = _ince_data(B, D)
    for temp, grads in combos:
        single = [_ince_single(a[r], b[r], kind, temp, grads) for r in range(INCE_R)]
        for R in (1, 3):
            x, y = torch.from_numpy(a[:R].copy()).cuda(), torch.from_numpy(b[:R].copy()).cuda()
            gx, gy, lo = _Block(R, B, D), _Block(R, B, D), _Block(1, 1, R)
            nws = int(lib.dib_infonce_batched_workspace_bytes(R, B))
            assert 0 < nws <= R * int(lib.dib_infonce_workspace_bytes(B)) and nws % (16 * R) == 0
            ws = torch.zeros(nws // 4 + 1, dtype=torch.float32, device="cuda")
            n0 = lib.dib_launch_count()
            _lib.check(lib.dib_infonce_fwd_bwd_batched(_ptr(x), _ptr(y), R, B, D, SIMILARITIES[kind], temp,
                                                       _ptr(gx.view) if grads else None, _ptr(gy.view) if grads else None,
                                                       _ptr(lo.view), _ptr(ws), _stream()), "dib_infonce_fwd_bwd_batched")
            n = lib.dib_launch_count() - n0
            torch.cuda.synchronize()
            loss = lo.check("loss").ravel()
            what = (R, temp, grads)
            assert n == single[0][3], (what, n, single[0][3], "as many launches as one problem")
            got_x, got_y = (gx.check("g_x"), gy.check("g_y")) if grads else (None, None)
            if not grads:
                assert bool(torch.isnan(gx.buf).all()) and bool(torch.isnan(gy.buf).all())
            for r in range(R):
                assert loss[r] == np.float32(single[r][0]), (what, r, loss[r], single[r][0])
                ref, g1, g2 = _ince_oracle(B, D, kind, temp, r)
                assert abs(float(loss[r]) - ref) < 2e-5 * (1 + abs(ref)), (what, r, loss[r], ref)
                if grads:
                    assert np.array_equal(got_x[r], single[r][1]) and np.array_equal(got_y[r], single[r][2]), (what, r)
                    assert np.abs(got_x[r] - g1).max() < 2e-4 * (1 + np.abs(g1).max()), (what, r)
                    assert np.abs(got_y[r] - g2).max() < 2e-4 * (1 + np.abs(g2).max()), (what, r)
            if grads:   # which route ran: one launch up to B = 128 (D <= 64), else sim + lse + grad (+ the final kernel from t64 = 5)
                assert n == (1 if B <= 128 and D <= 64 else 4 if B == 260 else 3), (what, n)


@pytest.mark.parametrize("kind", ["l1", "linf"])
def test_infonce_batched_refuses_l1_and_linf_without_a_launch(kind):
    lib = _lib_()
    buf = torch.full((1 << 14,), float("nan"), device="cuda")
    x = torch.zeros(3 * 12 * 8, device="cuda")
    ws = torch.zeros(int(lib.dib_infonce_batched_workspace_bytes(3, 12)) // 4 + 1, device="cuda")
    n0 = lib.dib_launch_count()
    q = _ptr(buf)
    assert lib.dib_infonce_fwd_bwd_batched(_ptr(x), _ptr(x), 3, 12, 8, SIMILARITIES[kind], 1.0, q, q, q, _ptr(ws), _stream()) \
        == DIB_E_UNSUPPORTED
    assert lib.dib_infonce_fwd_bwd_batched(_ptr(x), _ptr(x), 0, 12, 8, 0, 1.0, q, q, q, _ptr(ws), _stream()) == DIB_E_ARG
    assert lib.dib_infonce_fwd_bwd_batched(_ptr(x), _ptr(x), 3, 12, 8, 0, 0.0, q, q, q, _ptr(ws), _stream()) == DIB_E_ARG
    assert lib.dib_infonce_batched_workspace_bytes(0, 12) == DIB_E_ARG
    assert lib.dib_launch_count() == n0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
