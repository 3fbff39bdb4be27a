"""The batched entry points behind CircuitEnsemble, called through the C ABI on device buffers: dib_circuit_fwd_batched,
dib_circuit_bwd_batched, dib_circuit_mi_bounds_batched (include/dib_circuit.h) and dib_mlp_small_head_step_batched
(include/dib_hip.h).  Each computes R independent problems in one launch, the replica being a grid index.  Checked per shape:
  * every output of replica r equals, BIT FOR BIT, what the single entry point writes when called on that replica's slices
    (its table, G, seed, beta, parameters) - the batched kernels run the same body on moved pointers;
  * the float64 restatement (tests/_oracle_circuit.py; a float64 forward for the head) at the tolerances tests/test_gpu_circuit.py
    uses for the same quantities;
  * NaN sentinels around and between what a replica may write survive (kl beyond G_r + 1, grads outside the 2 G_r scalars,
    bounds rows g >= G_r, guard bands around every block);
  * an ensemble of 65 replicas (two launches of <= 64) has the bits of 65 single calls;
  * refused arguments return their error code, launch nothing (dib_launch_count unchanged) and write nothing."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _oracle_circuit as oc
from dib_amd import _lib, circuit
from dib_amd._gemm_plan import _ptr

pytestmark = pytest.mark.gpu

GUARD, LD, KLW = 67, 16, 17     # floats of NaN around every output block; u's pitch; a replica's kl row
STEP = 77
DIB_E_ARG, DIB_E_UNSUPPORTED = -1, -4
MIXED = (1, 3, 16)              # one gate, the pad columns, the full 16


def _lib_():
    return _lib.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _seeds(R, base=0x1234_5678_9ABC):
    return [base + 0x1_0000_0001 * r * r + 17 * r for r in range(R)]


class _Block:
    """`shape` elements, sentinel-filled (NaN; -7 for integers), between two guard bands"""

    def __init__(self, shape, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else -7
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD: GUARD + self.n].view(*shape)

    def _is_fill(self, t):
        return torch.isnan(t) if self.buf.dtype.is_floating_point else t == self.fill

    def untouched(self):
        return bool(self._is_fill(self.buf).all())

    def numpy(self, what):
        assert bool(self._is_fill(self.buf[:GUARD]).all()) and bool(self._is_fill(self.buf[GUARD + self.n:]).all()), \
            f"{what}: a guard band was written"
        return self.view.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _problem(Gs, B):
    """R replicas: random truth tables (3 spare words in front of each), scalars away from (1, -3), g_u; host arrays"""
    R = len(Gs)
    rng = np.random.default_rng(1000 * B + sum((i + 1) * g for i, g in enumerate(Gs)))
    words, offs, pos = [], [], 0
    for G in Gs:
        words.append(np.full(3, 0xFFFFFFFF, np.uint32)); pos += 3
        offs.append(pos)
        words.append(rng.integers(0, 1 << (G + 1), 1 << G, dtype=np.uint32)); pos += 1 << G
    words = np.concatenate(words)
    sc_off, stride = 128, 128 + 64 + 8                 # a replica's slice: [0, sc_off) unused, 2 G scalars, a tail
    params = np.full((R, stride), np.nan, np.float32)
    for r, G in enumerate(Gs):
        params[r, sc_off: sc_off + G] = rng.uniform(0.3, 1.5, G)
        params[r, sc_off + G: sc_off + 2 * G] = rng.uniform(-3.0, 0.5, G)
    return dict(Gs=Gs, R=R, B=B, words=words, offs=offs, sc_off=sc_off, stride=stride, params=params, seeds=_seeds(R),
                betas=[float(np.float32(0.37 + 0.5 * r)) for r in range(R)],
                row_idx=rng.integers(0, 1 << 20, (R, B)).astype(np.int32),
                g_u=(rng.standard_normal((R, B, LD)) / B).astype(np.float32))


def _table_bits(c, r):
    G = c["Gs"][r]
    w = c["words"][c["offs"][r]: c["offs"][r] + (1 << G)]
    return ((w[:, None] >> np.arange(G + 1, dtype=np.uint32)) & 1).astype(np.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_fwd_bwd(c, use_rows, expect_launches=1):
    """(batched outputs, per-replica single outputs) of the forward and the backward"""
    lib, R, B, Gs = _lib_(), c["R"], c["B"], c["Gs"]
    tables, params, g_u = _dev(c["words"].view(np.int32)), _dev(c["params"]), _dev(c["g_u"])
    ri = _dev(c["row_idx"]) if use_rows else None
    o = dict(rows=_Block((R, B), torch.int32), u=_Block((R, B, LD)), y=_Block((R, B)), kl=_Block((R, KLW)),
             grads=_Block((R, c["stride"])))
    head = (_ptr(tables), len(c["words"]), _arr(ctypes.c_int64, c["offs"]), _arr(ctypes.c_int, Gs), R, B, _ptr(params), c["stride"],
            c["sc_off"], _arr(ctypes.c_uint64, c["seeds"]), STEP, _arr(ctypes.c_float, c["betas"]))
    n0 = lib.dib_launch_count()
    _lib.check(lib.dib_circuit_fwd_batched(*head, _ptr(ri), _ptr(o["rows"].view), _ptr(o["u"].view), _ptr(o["y"].view),
                                           _ptr(o["kl"].view), _stream()), "dib_circuit_fwd_batched")
    _lib.check(lib.dib_circuit_bwd_batched(*head, _ptr(o["rows"].view), _ptr(g_u), _ptr(o["grads"].view), c["stride"], _stream()),
               "dib_circuit_bwd_batched")
    assert lib.dib_launch_count() - n0 == 2 * expect_launches
    torch.cuda.synchronize()
    bat = {k: v.numpy(k) for k, v in o.items()}
    single = []
    for r, G in enumerate(Gs):
        s = dict(rows=_Block((B,), torch.int32), u=_Block((B, LD)), y=_Block((B,)), kl=_Block((G + 1,)), g_sc=_Block((2 * G,)))
        tab, sc = _ptr(tables, c["offs"][r]), _ptr(params, r * c["stride"] + c["sc_off"])
        _lib.check(lib.dib_circuit_fwd(tab, G, B, sc, c["seeds"][r], STEP, c["betas"][r], _ptr(ri[r]) if use_rows else None,
                                       _ptr(s["rows"].view), _ptr(s["u"].view), _ptr(s["y"].view), _ptr(s["kl"].view), _stream()),
                   "dib_circuit_fwd")
        _lib.check(lib.dib_circuit_bwd(tab, G, B, sc, c["seeds"][r], STEP, c["betas"][r], _ptr(s["rows"].view), _ptr(g_u[r]),
                                       _ptr(s["g_sc"].view), _stream()), "dib_circuit_bwd")
        torch.cuda.synchronize()
        single.append({k: v.numpy(k) for k, v in s.items()})
    return bat, single


def _assert_fwd_bwd_equal_single(c, bat, single):
    so = c["sc_off"]
    for r, G in enumerate(c["Gs"]):
        s = single[r]
        for k in ("rows", "u", "y"):
            assert np.array_equal(bat[k][r], s[k]), (k, r)
        assert np.array_equal(bat["kl"][r, :G + 1], s["kl"]) and np.isnan(bat["kl"][r, G + 1:]).all(), ("kl", r)
        g = bat["grads"][r]
        assert np.array_equal(g[so: so + 2 * G], s["g_sc"]), ("g_sc", r)
        assert np.isnan(g[:so]).all() and np.isnan(g[so + 2 * G:]).all(), ("grads outside the replica's scalars were written", r)


@pytest.mark.parametrize("use_rows", [False, True], ids=["draw", "row_idx"])
@pytest.mark.parametrize("B", [1, 17, 512])
@pytest.mark.parametrize("Gs", [(1,), (3,), (16,), MIXED], ids=lambda g: "G" + "_".join(map(str, g)))
def test_fwd_and_bwd_batched_equal_the_single_kernels_and_the_oracle(Gs, B, use_rows):
    c = _problem(Gs, B)
    bat, single = _run_fwd_bwd(c, use_rows)
    _assert_fwd_bwd_equal_single(c, bat, single)
    for r, G in enumerate(Gs):                      # the float64 restatement, per replica
        seed, beta, bits = c["seeds"][r], c["betas"][r], _table_bits(c, r)
        s = c["params"][r, c["sc_off"]: c["sc_off"] + G].astype(np.float64)
        lv = c["params"][r, c["sc_off"] + G: c["sc_off"] + 2 * G].astype(np.float64)
        rows = (c["row_idx"][r].astype(np.int64) & ((1 << G) - 1)) if use_rows else oc.draw_rows(seed, STEP, B, G)
        assert np.array_equal(bat["rows"][r], rows), r
        e = oc.eps(seed, STEP, B, G)
        x = 2.0 * bits[rows, :G] - 1.0
        u = bat["u"][r].astype(np.float64)
        # tests/test_gpu_circuit.py's bound, which scales with the largest draw: the seeds of _problem are such that even the
        # B = 1 problems have a draw of at least one standard deviation
        assert np.abs(e).max() >= 1.0, ("the problem's seeds: largest |eps| below 1", r, np.abs(e).max())
        assert np.abs(u[:, :G] - (x * s + np.exp(lv / 2) * e)).max() < 2e-5 * np.abs(e).max(), r
        assert np.all(u[:, G:] == 0.0), "u's pad columns"
        assert np.array_equal(bat["y"][r], bits[rows, G].astype(np.float32))
        kl_ref = 0.5 * (s ** 2 + np.exp(lv) - lv - 1.0)
        kl = bat["kl"][r].astype(np.float64)
        np.testing.assert_allclose(kl[:G], kl_ref, rtol=1e-5, atol=1e-6)
        assert abs(kl[G] - beta * kl_ref.sum()) < 1e-5 * (1 + beta * kl_ref.sum())
        gu = c["g_u"][r, :, :G].astype(np.float64)
        ds = np.sum(gu * x, 0) + beta * s
        dlv = np.sum(gu * e, 0) * 0.5 * np.exp(lv / 2) + beta * 0.5 * (np.exp(lv) - 1.0)
        g = bat["grads"][r, c["sc_off"]: c["sc_off"] + 2 * G].astype(np.float64)
        for gd, gr in ((g[:G], ds), (g[G:], dlv)):
            assert np.abs(gd - gr).max() < 3e-4 * (np.abs(gr).max() + 1e-6), (r, gd, gr)


# ---- the row-tile head step ----------------------------------------------------------------------------------------------
def _head_desc(hidden, act="leaky_relu"):
    dims, w_off, b_off, sc_off, n_params = circuit._flat_layout(list(hidden))
    return circuit._predictor_desc(dims, w_off, b_off, act), dims, w_off, b_off, n_params


@functools.lru_cache(maxsize=None)
def _head_problem(R, B, hidden):
    d, dims, w_off, b_off, P = _head_desc(hidden)
    rng = np.random.default_rng(100 * R + B + sum(hidden))
    params = np.zeros((R, P), np.float32)
    for r in range(R):
        for (i, o), w, b in zip(dims, w_off, b_off):
            params[r, w: w + i * o] = (rng.standard_normal(i * o) * np.sqrt(2.0 / i)).astype(np.float32)
            params[r, b: b + o] = (0.1 * rng.standard_normal(o)).astype(np.float32)
    return dict(R=R, B=B, hidden=hidden, dims=dims, w_off=w_off, b_off=b_off, P=P, params=params,
                x=rng.standard_normal((R, B, LD)).astype(np.float32), y=rng.integers(0, 2, (R, B)).astype(np.float32))


def _head_outputs(R, B, hidden):
    o = dict(pred=_Block((R, B)), g_pred=_Block((R, B)), g_x=_Block((R, B, LD)), sums3=_Block((R, 3)))
    for l, w in enumerate(hidden):
        o[f"h{l}"], o[f"g{l}"] = _Block((R, B, w)), _Block((R, B, w))
    return o


def _ptr3(o, pre, nh, r=None):
    return (ctypes.c_void_p * 3)(*[_ptr(o[f"{pre}{l}"].view if r is None else o[f"{pre}{l}"].view[r]).value if l < nh else None
                                   for l in range(3)])


def _run_head(c, with_gx):
    lib, R, B, hidden, P = _lib_(), c["R"], c["B"], c["hidden"], c["P"]
    d, nh = _head_desc(hidden)[0], len(hidden)
    params, x, y = _dev(c["params"]), _dev(c["x"]), _dev(c["y"])
    bce = _lib.LOSS_KINDS["bce_logits"]
    assert lib.dib_mlp_small_head_batched_supported(ctypes.byref(d), B, R) == 1
    o, grads = _head_outputs(R, B, hidden), _Block((R, P))
    ws = torch.zeros(int(lib.dib_mlp_small_head_batched_workspace_bytes(ctypes.byref(d), B, R)) // 4, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):      # twice on one workspace: the last arriver of every replica re-armed its replica's word
        for b in list(o.values()) + [grads]:
            b.buf.fill_(float("nan"))
        n0 = lib.dib_launch_count()
        _lib.check(lib.dib_mlp_small_head_step_batched(ctypes.byref(d), _ptr(params), P, _ptr(x), B, R, _ptr(y), 1, bce, 1.0 / B,
                                                       _ptr3(o, "h", nh), _ptr3(o, "g", nh), _ptr(o["pred"].view),
                                                       _ptr(o["g_pred"].view), _ptr(o["g_x"].view) if with_gx else None,
                                                       _ptr(grads.view), P, _ptr(o["sums3"].view), _ptr(ws), _stream()),
                   "dib_mlp_small_head_step_batched")
        assert lib.dib_launch_count() - n0 == 1, "one launch whatever R"
        torch.cuda.synchronize()
        runs.append({**{k: v.numpy(k) for k, v in o.items()}, "grads": grads.numpy("grads")})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k], equal_nan=True), (k, "the second call on the same workspace")
    s, sg = _head_outputs(R, B, hidden), _Block((R, P))
    sws = torch.zeros(int(lib.dib_mlp_small_head_workspace_bytes(ctypes.byref(d), B)) // 4 + 4, dtype=torch.float32, device="cuda")
    for r in range(R):
        _lib.check(lib.dib_mlp_small_head_step(ctypes.byref(d), _ptr(params[r]), _ptr(x[r]), B, _ptr(y[r]), 1, bce, 1.0 / B,
                                               _ptr3(s, "h", nh, r), _ptr3(s, "g", nh, r), _ptr(s["pred"].view[r]),
                                               _ptr(s["g_pred"].view[r]), _ptr(s["g_x"].view[r]) if with_gx else None,
                                               _ptr(sg.view[r]), _ptr(s["sums3"].view[r]), _ptr(sws), _stream()),
                   "dib_mlp_small_head_step")
    torch.cuda.synchronize()
    return runs[0], {**{k: v.numpy(k) for k, v in s.items()}, "grads": sg.numpy("grads")}


@pytest.mark.parametrize("with_gx", [True, False], ids=["g_x", "no_g_x"])
@pytest.mark.parametrize("hidden", [(16,), (32, 16), (256, 256, 256)], ids=lambda h: "x".join(map(str, h)))
@pytest.mark.parametrize("B", [1, 16, 17, 512])
@pytest.mark.parametrize("R", [1, 2, 5])
def test_head_step_batched_equals_the_single_entry_and_a_float64_forward(R, B, hidden, with_gx):
    c = _head_problem(R, B, hidden)
    bat, single = _run_head(c, with_gx)
    for k in bat:     # pred, g_pred, every h / g, g_x, sums3, the output layer's gradient; NaN where neither entry writes
        assert np.array_equal(bat[k], single[k], equal_nan=True), k
    assert np.isnan(bat["g_x"]).all() != with_gx
    wo, bo, KL = c["w_off"][-1], c["b_off"][-1], hidden[-1]
    assert not np.isnan(bat["grads"][:, wo: wo + KL]).any() and not np.isnan(bat["grads"][:, bo]).any()
    assert np.isnan(bat["grads"][:, :wo]).all(), "only the output layer's gradient is this kernel's"
    for r in range(R):   # float64 forward: logits and the mean BCE (tests/test_gpu_circuit.py's tolerances)
        h = c["x"][r].astype(np.float64)
        for l, ((i, o), w, b) in enumerate(zip(c["dims"], c["w_off"], c["b_off"])):
            z = h @ c["params"][r, w: w + i * o].reshape(i, o).astype(np.float64) + c["params"][r, b: b + o]
            h = np.where(z > 0, z, oc.SLOPE * z) if l < len(hidden) else z
        logit, y = h[:, 0], c["y"][r].astype(np.float64)
        ref = float(np.mean(np.maximum(logit, 0) - logit * y + np.log1p(np.exp(-np.abs(logit)))))
        np.testing.assert_allclose(bat["pred"][r], logit, rtol=0, atol=2e-4 * (1 + np.abs(logit).max()))
        assert abs(float(bat["sums3"][r, 2]) - ref) < 2e-5 * (1 + ref), (r, bat["sums3"][r], ref)


# ---- the sandwich bounds ---------------------------------------------------------------------------------------------------
def _run_mi(c, n, nb, calls=2):
    lib, R, Gs = _lib_(), c["R"], c["Gs"]
    rng = np.random.default_rng(n + nb)
    x = np.float32([-1.0, 1.0])[rng.integers(0, 2, (R, nb, n))]
    params, xd = _dev(c["params"]), _dev(x)
    need = int(lib.dib_circuit_mi_batched_workspace_bytes(R, n, nb))
    assert need > 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    out = _Block((R, 16, nb, 2), torch.float64)
    res = []
    for _ in range(calls):   # the second call reuses the self-cleaning arrival counters
        out.buf.fill_(float("nan"))
        n0 = lib.dib_launch_count()
        _lib.check(lib.dib_circuit_mi_bounds_batched(_ptr(params), c["stride"], c["sc_off"], _arr(ctypes.c_int, Gs), R, _ptr(xd), n,
                                                     nb, _arr(ctypes.c_uint64, c["seeds"]), _ptr(out.view), _ptr(ws), _stream()),
                   "dib_circuit_mi_bounds_batched")
        assert lib.dib_launch_count() - n0 == (R + 63) // 64
        torch.cuda.synchronize()
        res.append(out.numpy("bounds"))
    assert all(np.array_equal(res[0], r, equal_nan=True) for r in res[1:])
    single = []
    for r, G in enumerate(Gs):
        sws = torch.zeros(int(lib.dib_circuit_mi_workspace_bytes(G, n, nb)) // 8 + 1, dtype=torch.float64, device="cuda")
        so = _Block((G, nb, 2), torch.float64)
        _lib.check(lib.dib_circuit_mi_bounds(_ptr(params, r * c["stride"] + c["sc_off"]), G, _ptr(xd[r]), n, nb, c["seeds"][r],
                                             _ptr(so.view), _ptr(sws), _stream()), "dib_circuit_mi_bounds")
        torch.cuda.synchronize()
        single.append(so.numpy("single bounds"))
    return res[0], single, x


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("n", [2, 65, 1024])
def test_mi_bounds_batched_equal_the_single_kernel_and_compute_batch(n, nb):
    c = _problem(MIXED, 17)
    bat, single, x = _run_mi(c, n, nb)
    for r, G in enumerate(MIXED):
        assert np.isfinite(single[r]).all()
        assert np.array_equal(bat[r, :G], single[r]), r
        assert np.isnan(bat[r, G:]).all(), ("rows g >= G_r were written", r)
    if n <= 65:   # the notebook's compute_batch in float64 on the device's own fp32 noise (as tests/test_gpu_circuit.py does)
        lib = _lib_()
        for r, G in enumerate(MIXED):
            eps = torch.empty((n, G, 1), dtype=torch.float32, device="cuda")
            for b in range(nb):
                assert lib.dib_philox_normal_fill(_ptr(eps), None, 0, n, G, 1, c["seeds"][r], b, None) == 0
                e = eps.cpu().numpy()[:, :, 0].astype(np.float64)
                for g in range(G):
                    lo, up = oc.mi_bounds_batch(c["params"][r, c["sc_off"] + g], c["params"][r, c["sc_off"] + G + g], x[r, b], e[:, g])
                    if np.isfinite(lo) and np.isfinite(up):
                        assert abs(bat[r, g, b, 0] - lo) < 1e-9 and abs(bat[r, g, b, 1] - up) < 1e-9, (r, g, b)


# ---- more replicas than one launch carries -----------------------------------------------------------------------------------
def test_65_replicas_in_two_launches_equal_65_single_calls():
    Gs = tuple((1, 3, 16, 2, 5)[r % 5] for r in range(65))
    c = _problem(Gs, 17)
    bat, single = _run_fwd_bwd(c, use_rows=False, expect_launches=2)
    _assert_fwd_bwd_equal_single(c, bat, single)
    mb, ms, _ = _run_mi(c, 65, 1, calls=1)
    for r, G in enumerate(Gs):
        assert np.array_equal(mb[r, :G], ms[r]) and np.isnan(mb[r, G:]).all(), r
    hb, hs = _run_head(_head_problem(65, 17, (16,)), True)     # (the head's grid carries any R: one launch)
    for k in hb:
        assert np.array_equal(hb[k], hs[k], equal_nan=True), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_launch_nothing_and_write_nothing():
    lib, c = _lib_(), _problem(MIXED, 17)
    R, B = 3, 17
    tables, params, g_u = _dev(c["words"].view(np.int32)), _dev(c["params"]), _dev(c["g_u"])
    o = dict(rows=_Block((R, B), torch.int32), u=_Block((R, B, LD)), y=_Block((R, B)), kl=_Block((R, KLW)),
             grads=_Block((R, c["stride"])), mi=_Block((R, 16, 1, 2), torch.float64))
    ws = torch.zeros(int(lib.dib_circuit_mi_batched_workspace_bytes(R, 65, 1)) // 8, dtype=torch.float64, device="cuda")
    rows_in = torch.zeros((R, B), dtype=torch.int32, device="cuda")

    def fwd_bwd(Gs=MIXED, R=R, B=B, tab=tables):
        head = (_ptr(tab), len(c["words"]), _arr(ctypes.c_int64, c["offs"]), _arr(ctypes.c_int, Gs), R, B, _ptr(params), c["stride"],
                c["sc_off"], _arr(ctypes.c_uint64, c["seeds"]), STEP, _arr(ctypes.c_float, c["betas"]))
        return (lib.dib_circuit_fwd_batched(*head, None, _ptr(o["rows"].view), _ptr(o["u"].view), _ptr(o["y"].view),
                                            _ptr(o["kl"].view), _stream()),
                lib.dib_circuit_bwd_batched(*head, _ptr(rows_in), _ptr(g_u), _ptr(o["grads"].view), c["stride"], _stream()))

    def mi(Gs=MIXED, R=R, n=65):
        return lib.dib_circuit_mi_bounds_batched(_ptr(params), c["stride"], c["sc_off"], _arr(ctypes.c_int, Gs), R, _ptr(rows_in), n, 1,
                                                 _arr(ctypes.c_uint64, c["seeds"]), _ptr(o["mi"].view), _ptr(ws), _stream())

    n0 = lib.dib_launch_count()
    for bad in ((1, 0, 16), (17, 3, 16), (1, 3, 17)):
        assert fwd_bwd(Gs=bad) == (DIB_E_UNSUPPORTED, DIB_E_UNSUPPORTED), bad
        assert mi(Gs=bad) == DIB_E_UNSUPPORTED, bad
    for bad in (0, 2049):
        assert fwd_bwd(B=bad) == (DIB_E_UNSUPPORTED, DIB_E_UNSUPPORTED), bad
    assert fwd_bwd(R=0) == (DIB_E_UNSUPPORTED, DIB_E_UNSUPPORTED) and mi(R=0) == DIB_E_UNSUPPORTED
    assert fwd_bwd(tab=None) == (DIB_E_ARG, DIB_E_ARG), "a NULL table"
    assert mi(n=1) == DIB_E_UNSUPPORTED
    # the head: R = 0, B = 0 and B beyond the row-tile envelope
    d, dims, w_off, b_off, P = _head_desc((16,))
    ho, hg = _head_outputs(R, B, (16,)), _Block((R, P))
    hws = torch.zeros(int(lib.dib_mlp_small_head_batched_workspace_bytes(ctypes.byref(d), B, R)) // 4, dtype=torch.float32, device="cuda")
    hp = torch.zeros((R, P), dtype=torch.float32, device="cuda")

    def head(R=R, B=B):
        return lib.dib_mlp_small_head_step_batched(ctypes.byref(d), _ptr(hp), P, _ptr(o["u"].view), B, R, _ptr(o["y"].view), 1,
                                                   _lib.LOSS_KINDS["bce_logits"], 1.0, _ptr3(ho, "h", 1), _ptr3(ho, "g", 1),
                                                   _ptr(ho["pred"].view), _ptr(ho["g_pred"].view), _ptr(ho["g_x"].view), _ptr(hg.view), P,
                                                   _ptr(ho["sums3"].view), _ptr(hws), _stream())

    assert head(R=0) == DIB_E_UNSUPPORTED and head(B=0) == DIB_E_ARG and head(B=1 << 20) == DIB_E_UNSUPPORTED
    assert lib.dib_launch_count() == n0, "a refusal launches nothing"
    torch.cuda.synchronize()
    for k, b in {**o, **ho, "head grads": hg}.items():
        assert b.untouched(), (k, "a refusal wrote to an output buffer")
    assert not bool(hws.any()) and not bool(ws.any())
