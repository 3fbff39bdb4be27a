"""The LDS-free forward / dgrad kernel (csrc/dib_gemm_stream.h) against the tiled one (csrc/dib_gemm.h, modes 0 and 1) it replaces
for large products in whole 128 x 128 x 32 tiles: the same entry (include/dib_hip.h dib_gemm), once with
dib_set_tuning("gemm_stream", 0) and once with 1, the row threshold ("gemm_stream_rows") at 128 and the fill rule
("gemm_stream_fill") off.  The contract is BIT equality of the whole output buffer - NaN guard rows and columns around it
included - plus the library's live profile saying which kernel ran (entries 20 / 21 of dib_profile_summary_n re-count the parts
of categories 3 / 7 that ran the new kernel).  Both arms are also held to the standard float32 bound against NumPy float64,
n 2^-24 / (1 - n 2^-24) |A| |B| with n = K, applied BEFORE the activation (mode 0: a run with the linear activation and no bias;
mode 1: the run without a mask).  One whole training step at the end: parameters, gradients and step outputs bit-equal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

KEYS = ("gemm_stream", "gemm_stream_rows", "gemm_stream_fill", "stream_rows")
LINEAR, RELU, LEAKY = 0, 1, 2      # include/dib_hip.h activation codes
N_PROF = 22
U = 2.0 ** -24


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _launches(lib, mode):
    """(launches timed in the 128 x 128 tiled kernel's category of this mode, how many of them were the new kernel)"""
    ms = (ctypes.c_double * N_PROF)()
    cnt = (ctypes.c_int * N_PROF)()
    assert lib.dib_profile_summary_n(ms, cnt, N_PROF) == 0
    return cnt[mode * 4 + 3], cnt[20 + mode]


def _operands(mode, M, N, K, pad, seed_extra=0):
    """A [M, lda] with many exact zeros (like the real activations), B ([K, N] mode 0, [N, K] mode 1), bias, aux with exact zeros,
    -0.0 and negatives.  pad: lda = K + 8, ldc = N + 8, ldaux = N + 4 (the extra columns hold NaN / are never read)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + 13 * mode + seed_extra)
    lda, ldc, ldaux = (K + 8, N + 8, N + 4) if pad else (K, N, N)
    A = np.full((M, lda), np.nan, dtype=np.float32)
    A[:, :K] = np.maximum(rng.standard_normal((M, K)), 0)
    Bm = rng.standard_normal((K, N) if mode == 0 else (N, K)).astype(np.float32)
    Bm[K // 3 if mode == 0 else N // 3] = 0.0                    # a zeroed row
    bias = rng.standard_normal(N).astype(np.float32)
    aux = np.full((M, ldaux), np.nan, dtype=np.float32)
    x = rng.standard_normal((M, N)).astype(np.float32)
    x[rng.random((M, N)) < 0.2] = 0.0
    x[rng.random((M, N)) < 0.1] = -0.0
    aux[:, :N] = x
    assert (x == 0).any() and np.signbit(x[x == 0]).any() and (x < 0).any()
    return A, Bm, bias, aux, lda, ldc, ldaux


def _run_both(mode, M, N, K, act, use_bias=False, use_aux=False, pad=False, stream_rows=None, ops=None):
    """Both arms on the same operands -> ([tiled, stream] whole C buffers as int32 [M + 2, ldc], launches per arm, operands)."""
    from dib_amd import _lib as L
    lib = L.load_library()
    A, Bm, bias, aux, lda, ldc, ldaux = ops if ops is not None else _operands(mode, M, N, K, pad)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(Bm).cuda()
    bd = torch.from_numpy(bias).cuda() if use_bias else None
    xd = torch.from_numpy(aux).cuda() if use_aux else None
    desc = torch.zeros(256, dtype=torch.uint8, device="cuda")
    old = [L.get_tuning(k) for k in KEYS]
    bufs, launches = [], []
    try:
        L.set_tuning("gemm_stream_rows", 128)
        L.set_tuning("gemm_stream_fill", 0)
        if stream_rows is not None:     # the kernels' non-temporal policy from this many rows up (default 8192)
            L.set_tuning("stream_rows", stream_rows)
        for arm in (0, 1):
            L.set_tuning("gemm_stream", arm)
            C = torch.full((M + 2, ldc), float("nan"), device="cuda")     # a guard row above and below, guard columns when ldc > N
            lib.dib_profile_enable(1)
            L.check(lib.dib_gemm(mode, M, N, K, _ptr(Ad), lda, _ptr(Bd), N if mode == 0 else K, _ptr(C[1]), ldc,
                                 _ptr(bd) if use_bias else None, _ptr(xd) if use_aux else None, ldaux if use_aux else 0, act,
                                 _ptr(desc), _stream()), "dib_gemm")
            torch.cuda.synchronize()
            launches.append(_launches(lib, mode))
            lib.dib_profile_enable(0)
            bufs.append(C.view(torch.int32).cpu().numpy())
    finally:
        lib.dib_profile_enable(0)
        for k, v in zip(KEYS, old):
            L.set_tuning(k, v)
    return bufs, launches, (A[:, :K], Bm, bias, aux[:, :N])


def _product(mode, A, Bm):
    a, b = A.astype(np.float64), (Bm if mode == 0 else Bm.T).astype(np.float64)
    return a @ b, np.abs(a) @ np.abs(b)


def _check_guards(buf_i32, M, N):
    buf = buf_i32.view(np.float32)
    assert np.isnan(buf[0]).all() and np.isnan(buf[M + 1]).all() and np.isnan(buf[:, N:]).all()
    assert not np.isnan(buf[1: M + 1, :N]).any()


def _check_preactivation(buf_i32, mode, M, N, K, A, Bm):
    got = buf_i32.view(np.float32)[1: M + 1, :N].astype(np.float64)
    ref, mag = _product(mode, A, Bm)
    assert np.all(np.abs(got - ref) <= K * U / (1 - K * U) * mag + 1e-30)


SHAPES = [(M, N, K) for M in (128, 384) for N in (128, 256) for K in (32, 96, 256, 2048)]   # K: shorter than the ring, a ragged trip
#                                                                                            # round it, the two real depths


@pytest.mark.parametrize("act,use_bias", [(RELU, True), (LINEAR, False), (LEAKY, True), (LINEAR, True), (RELU, False)])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_forward_is_the_tiled_kernels_bit_for_bit(M, N, K, act, use_bias):
    (tiled, stream), launches, (A, Bm, bias, _) = _run_both(0, M, N, K, act, use_bias=use_bias)
    assert launches[0] == (1, 0) and launches[1] == (1, 1), launches     # arm 0: the tiled kernel; arm 1: the new one
    _check_guards(tiled, M, N)
    _check_guards(stream, M, N)
    assert np.array_equal(tiled, stream)     # int32 views: NaNs compare by their bits
    if act == LINEAR and not use_bias:       # the pre-activation products, both arms
        _check_preactivation(tiled, 0, M, N, K, A, Bm)
        _check_preactivation(stream, 0, M, N, K, A, Bm)
    else:                                    # ... and the epilogue on top of them: float32 arithmetic on the float32 product
        (lin, _), _, _ = _run_both(0, M, N, K, LINEAR)
        z = lin.view(np.float32)[1: M + 1, :N] + (bias if use_bias else np.float32(0))
        want = np.maximum(z, 0) if act == RELU else (np.where(z > 0, z, np.float32(0.2) * z) if act == LEAKY else z)
        assert np.array_equal(stream.view(np.float32)[1: M + 1, :N], want.astype(np.float32))


@pytest.mark.parametrize("use_aux", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dgrad_is_the_tiled_kernels_bit_for_bit(M, N, K, use_aux):
    act = LEAKY if use_aux else LINEAR
    (tiled, stream), launches, (A, Bm, _, aux) = _run_both(1, M, N, K, act, use_aux=use_aux)
    assert launches[0] == (1, 0) and launches[1] == (1, 1), launches
    _check_guards(tiled, M, N)
    _check_guards(stream, M, N)
    assert np.array_equal(tiled, stream)
    if not use_aux:
        _check_preactivation(tiled, 1, M, N, K, A, Bm)
        _check_preactivation(stream, 1, M, N, K, A, Bm)
    else:                                    # the mask: one float32 multiplication of the float32 product
        (lin, _), _, _ = _run_both(1, M, N, K, LINEAR)
        want = lin.view(np.float32)[1: M + 1, :N] * np.where(aux > 0, np.float32(1), np.float32(0.2))
        assert np.array_equal(stream.view(np.float32)[1: M + 1, :N], want.astype(np.float32))


@pytest.mark.parametrize("M,N,K", [(384, 256, 256), (128, 128, 96)])
def test_relu_mask_values(M, N, K):
    """dib_gemm's tiled arm is the 32-deep kernel, whose relu shortcut writes +0 where the mask is off; the 128 x 128 x 64 kernel of
    the large launches - the one the new kernel reproduces - multiplies by 0 and keeps the product's sign on its zeros.  So here the
    arms are equal as float VALUES (+0 == -0), and the new kernel's bits are those of the multiplication."""
    (tiled, stream), launches, (A, Bm, _, aux) = _run_both(1, M, N, K, RELU, use_aux=True)
    assert launches[0] == (1, 0) and launches[1] == (1, 1), launches
    _check_guards(stream, M, N)
    t, s = tiled.view(np.float32)[1: M + 1, :N], stream.view(np.float32)[1: M + 1, :N]
    assert np.array_equal(t, s)
    (lin, _), _, _ = _run_both(1, M, N, K, LINEAR)
    want = lin.view(np.float32)[1: M + 1, :N] * np.where(aux > 0, np.float32(1), np.float32(0))
    assert np.array_equal(s.view(np.int32), want.astype(np.float32).view(np.int32))
    assert np.array_equal(tiled[0], stream[0]) and np.array_equal(tiled[M + 1], stream[M + 1])


@pytest.mark.parametrize("mode,act,use_bias,use_aux", [(0, RELU, True, False), (1, LEAKY, False, True)])
@pytest.mark.parametrize("stream_rows", [None, 64])     # 64: the tiled arm's non-temporal loads and both arms' row rule
def test_padded_leading_dimensions(mode, act, use_bias, use_aux, stream_rows):
    M, N, K = 384, 256, 96
    ops = _operands(mode, M, N, K, pad=True)
    (tiled, stream), launches, (A, Bm, _, _) = _run_both(mode, M, N, K, act, use_bias=use_bias, use_aux=use_aux, stream_rows=stream_rows,
                                                         ops=ops)
    assert launches[0] == (1, 0) and launches[1] == (1, 1), launches
    _check_guards(stream, M, N)
    assert np.array_equal(tiled, stream)
    (lt, ls), _, _ = _run_both(mode, M, N, K, LINEAR, stream_rows=stream_rows, ops=ops)
    assert np.array_equal(lt, ls)
    _check_preactivation(lt, mode, M, N, K, A, Bm)
    _check_preactivation(ls, mode, M, N, K, A, Bm)


def test_output_of_256_mb_is_stored_non_temporally_with_the_same_bits():
    """[32768, 2048] floats = 256 MB, at least "stream_rows" rows: the new kernel stores it non-temporally (the large dgrad's g_u
    is this case)."""
    from dib_amd import _lib as L
    lib = L.load_library()
    M, N, K = 32768, 2048, 32
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.relu(torch.randn((M, K), device="cuda", generator=g))
    Bm = torch.randn((N, K), device="cuda", generator=g)
    desc = torch.zeros(256, dtype=torch.uint8, device="cuda")
    old = [L.get_tuning(k) for k in KEYS]
    outs, launches = [], []
    try:
        L.set_tuning("gemm_stream_rows", 128)
        L.set_tuning("gemm_stream_fill", 0)
        for arm in (0, 1):
            L.set_tuning("gemm_stream", arm)
            C = torch.full((M + 2, N), float("nan"), device="cuda")
            lib.dib_profile_enable(1)
            L.check(lib.dib_gemm(1, M, N, K, _ptr(A), K, _ptr(Bm), K, _ptr(C[1]), N, None, None, 0, LINEAR, _ptr(desc), _stream()), "dib_gemm")
            torch.cuda.synchronize()
            launches.append(_launches(lib, 1))
            lib.dib_profile_enable(0)
            outs.append(C)
    finally:
        lib.dib_profile_enable(0)
        for k, v in zip(KEYS, old):
            L.set_tuning(k, v)
    assert launches[0] == (1, 0) and launches[1] == (1, 1), launches
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.isnan(outs[1][0]).all() and torch.isnan(outs[1][M + 1]).all() and not torch.isnan(outs[1][1: M + 1]).any()
    rows = torch.cat([torch.arange(0, 256), torch.arange(M - 256, M)]).cuda()     # the first and the last tiles' rows against float64
    a, b = A[rows].double(), Bm.double()
    bound = K * U / (1 - K * U) * (a.abs() @ b.abs().T) + 1e-30
    assert bool(((outs[1][1 + rows].double() - a @ b.T).abs() <= bound).all())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,N,K", [(200, 256, 96), (384, 200, 96), (384, 256, 40)])     # M, N = 192 + 8, K: no whole tiles
def test_ineligible_shapes_stay_on_the_tiled_kernel(mode, M, N, K):
    (tiled, stream), launches, (A, Bm, _, _) = _run_both(mode, M, N, K, LINEAR)
    assert launches[0] == (1, 0) and launches[1] == (1, 0), launches
    _check_guards(stream, M, N)
    _check_preactivation(stream, mode, M, N, K, A, Bm)
    assert np.array_equal(tiled, stream)


def test_thresholds_keep_small_products_on_the_tiled_kernel():
    """the defaults: 8192 rows and 85 % of the wave slots"""
    from dib_amd import _lib as L
    lib = L.load_library()
    M = N = K = 256
    A = torch.randn((M, K), device="cuda")
    Bm = torch.randn((K, N), device="cuda")
    C = torch.empty((M, N), device="cuda")
    desc = torch.zeros(256, dtype=torch.uint8, device="cuda")
    assert L.get_tuning("gemm_stream") == 1 and L.get_tuning("gemm_stream_rows") == 8192 and L.get_tuning("gemm_stream_fill") == 85
    try:
        lib.dib_profile_enable(1)
        L.check(lib.dib_gemm(0, M, N, K, _ptr(A), K, _ptr(Bm), N, _ptr(C), N, None, None, 0, LINEAR, _ptr(desc), _stream()), "dib_gemm")
        torch.cuda.synchronize()
        assert _launches(lib, 0) == (1, 0)
    finally:
        lib.dib_profile_enable(0)


# ---- one whole training step: the headline architecture with two features, B = 17 x 128 rows (above the row-tile regime) ----
def _step_arm(arm, B=2176):
    import dib_oracle as orc
    from _helpers import spec_kwargs
    from dib_amd import _lib as L
    from dib_amd.engine import HipEngine
    spec = orc.DIBSpec([1, 1], [128, 128], [256, 256], 1, activation_fn="relu", feature_embedding_dimension=32)
    lib = L.load_library()
    old = [L.get_tuning(k) for k in KEYS]
    try:
        L.set_tuning("gemm_stream_rows", 128)
        L.set_tuning("gemm_stream_fill", 0)
        L.set_tuning("gemm_stream", arm)
        eng = HipEngine(**spec_kwargs(spec), init_seed=4)
        eng.set_beta(0.05)
        eng.set_lr(3e-4)
        rng = np.random.default_rng(3)
        x = rng.standard_normal((B, 2)).astype(np.float32)
        y = (x[:, :1] * x[:, 1:2] > 0).astype(np.float32)
        xd, yd = eng.to_device(x), eng.to_device(y)
        lib.dib_profile_enable(1)
        for step in range(2):
            eng.train_step(xd, yd, None, 0, B, 5, step, "bce_logits")
            torch.cuda.synchronize()
            if step == 1:
                out = dict(grads=eng.grads.view(torch.int32).cpu().numpy().copy(),
                           step_out=eng.step_out(B).view(torch.int32).cpu().numpy().copy())
            eng.adam_step()
        torch.cuda.synchronize()
        ms = (ctypes.c_double * N_PROF)()
        cnt = (ctypes.c_int * N_PROF)()
        assert lib.dib_profile_summary_n(ms, cnt, N_PROF) == 0
        out["stream"] = (cnt[20], cnt[21])
        out["params"] = eng.params.view(torch.int32).cpu().numpy().copy()
        assert np.isfinite(eng.get_flat_grads()).all()
        return out
    finally:
        lib.dib_profile_enable(0)
        for k, v in zip(KEYS, old):
            L.set_tuning(k, v)


def test_whole_step_has_the_tiled_arms_bits():
    tiled, stream = _step_arm(0), _step_arm(1)
    assert tiled["stream"] == (0, 0), tiled["stream"]
    # two steps: both integration forwards (K = 64 and 256, N = 256) and the layer-2 dgrad (K = N = 256) each time; the layer-1
    # dgrad's 64 columns are no whole tile
    assert stream["stream"][0] >= 4 and stream["stream"][1] >= 2, stream["stream"]
    for k in ("params", "grads", "step_out"):
        assert np.array_equal(tiled[k], stream[k]), k
