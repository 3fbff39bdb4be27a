"""The LDS-free weight-gradient kernel (csrc/dib_wgrad_stream.h) against the tiled one (csrc/dib_gemm.h, mode 2) it replaces for
128-wide row-major operands: the same entry (include/dib_st.h dib_wgrad_grouped), the same forced split, once with
dib_set_tuning("wgrad_stream", 0) and once with 1, the row threshold ("wgrad_stream_rows") at 64 and the fill rule
("wgrad_stream_fill") off.  The contract is BIT equality
of the whole slab buffer - weight-gradient slabs, bias rows (the kernel hands its running column sums between the half-waves so
that the additions happen in the tiled kernel's order), and the NaNs of everything the launch does not write - plus the
library's live profile saying which kernel ran.  Both are also held to the standard float32 bound against NumPy float64."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_OFF = 64          # the first group's block does not start the buffer
CAT_STREAM = (17, 18)   # include/dib_hip.h dib_profile_summary_n: dib_wgrad_stream_kernel on 128- / 64-column tiles


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stream_launches(lib):
    ms = (ctypes.c_double * 19)()
    cnt = (ctypes.c_int * 19)()
    assert lib.dib_profile_summary_n(ms, cnt, 19) == 0
    return sum(cnt[c] for c in CAT_STREAM), sum(cnt[c] for c in range(8, 12))   # (8..11: dib_gemm_kernel<2, ...>)


def _run_both(M, N, K, rows, slabs, groups, ldb=None, nontemporal=False):
    """Both arms on the same operands.  Returns (buffers as int32 [2][slabs + 1][stride], descriptors, A, B, stride, launches)."""
    from dib_amd import _lib as L
    from dib_amd._gemm_plan import DESC
    lib = L.load_library()
    ldb = ldb or N
    rng = np.random.default_rng(M * 7 + N * 3 + K + slabs * 11 + groups)
    A = np.maximum(rng.standard_normal((groups, K, M)), 0).astype(np.float32)     # many exact zeros, like h1 / h2
    Bm = np.zeros((groups, K, ldb), dtype=np.float32)
    Bm[:, :, :N] = rng.standard_normal((groups, K, N))
    Bm[:, K // 3: K // 3 + 9, : N // 2] = 0.0                                      # a zeroed block, like a masked gradient
    per = (M * N + N + 3) // 4 * 4
    stride = C_OFF + groups * per
    desc = np.zeros(groups, dtype=DESC)
    for g in range(groups):
        # feature-major operands: offset = boff * batch; M / N by value, K = -1 = the batch
        desc[g] = (0, 0, C_OFF + g * per, -1 if (groups > 1 and g == 1) else C_OFF + g * per + M * N, 0,
                   g * M, g * ldb, 0, 0, M, N, -1, M, ldb, N, 0, 0)
    dev = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(Bm).cuda()
    keys = ("wgrad_stream", "wgrad_stream_rows", "wgrad_stream_fill", "stream_rows")
    old = [L.get_tuning(k) for k in keys]
    bufs, launches = [], []
    try:
        L.set_tuning("wgrad_stream_rows", 64)
        L.set_tuning("wgrad_stream_fill", 0)
        if nontemporal:     # both kernels load their operands non-temporally from "stream_rows" streamed rows up
            L.set_tuning("stream_rows", 64)
        for arm in (0, 1):
            L.set_tuning("wgrad_stream", arm)
            buf = torch.full(((slabs + 1) * stride,), float("nan"), device="cuda")   # one slab more than the launch writes
            lib.dib_profile_enable(1)
            L.check(lib.dib_wgrad_grouped(groups, _ptr(dev), desc.ctypes.data_as(ctypes.c_void_p), M, N, K, _ptr(Ad), _ptr(Bd),
                                          _ptr(buf), _ptr(buf), slabs, rows, stride, _stream()), "dib_wgrad_grouped")
            torch.cuda.synchronize()
            launches.append(_stream_launches(lib))
            lib.dib_profile_enable(0)
            bufs.append(buf.view(torch.int32).view(slabs + 1, stride).cpu().numpy())
    finally:
        lib.dib_profile_enable(0)
        for k, v in zip(keys, old):
            L.set_tuning(k, v)
    return bufs, desc, A, Bm[:, :, :N], stride, launches


def _check_against_float64(buf_i32, desc, A, Bm, rows, slabs, K):
    """Every written word against NumPy float64 within the standard bound of an n-term float32 sum, n 2^-24 sum |terms| (n = the
    slab's rows); everything else still NaN."""
    buf = buf_i32.view(np.float32)
    written = np.zeros(buf.shape, dtype=bool)
    u = 2.0 ** -24      # gamma_n = n u / (1 - n u)
    for g, d in enumerate(desc):
        M, N = int(d["M"]), int(d["N"])
        for s in range(slabs):
            a = A[g, s * rows: min(K, (s + 1) * rows)].astype(np.float64)
            b = Bm[g, s * rows: min(K, (s + 1) * rows)].astype(np.float64)
            n = max(a.shape[0], 1)
            got = buf[s, d["c_off"]: d["c_off"] + M * N].reshape(M, N)
            assert np.all(np.abs(got - a.T @ b) <= n * u / (1 - n * u) * (np.abs(a).T @ np.abs(b)) + 1e-30), (g, s)
            written[s, d["c_off"]: d["c_off"] + M * N] = True
            if d["bias_off"] >= 0:
                got_b = buf[s, d["bias_off"]: d["bias_off"] + N]
                assert np.all(np.abs(got_b - b.sum(0)) <= n * u / (1 - n * u) * np.abs(b).sum(0) + 1e-30), (g, s, "column sums")
                written[s, d["bias_off"]: d["bias_off"] + N] = True
    assert not np.isnan(buf[written]).any()
    assert np.isnan(buf[~written]).all()    # gaps, the bias row of a group without one, the slab beyond the launch's


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("slabs", [1, 3])
@pytest.mark.parametrize("rows", [64, 192, 576])     # fewer blocks than the prefetch ring holds ... several trips around it
@pytest.mark.parametrize("M,N", [(128, 128), (128, 64), (256, 256)])   # 16-byte / 8-byte B loads; 2 x 2 tiles, bias from tm == 0 only
def test_stream_kernel_slabs_are_the_tiled_kernels_bit_for_bit(M, N, rows, slabs, groups):
    K = rows * slabs
    (tiled, stream), desc, A, Bm, stride, launches = _run_both(M, N, K, rows, slabs, groups, nontemporal=slabs == 3)
    assert launches[0] == (0, 1) and launches[1] == (1, 0), launches     # arm 0: the tiled kernel; arm 1: the new one
    _check_against_float64(tiled, desc, A, Bm, rows, slabs, K)
    _check_against_float64(stream, desc, A, Bm, rows, slabs, K)
    assert np.array_equal(tiled, stream)     # int32 views: NaNs compare by their bits


@pytest.mark.parametrize("M,N,K,rows,slabs,ldb", [(200, 128, 192, 64, 3, None),    # M is no multiple of 128
                                                  (128, 70, 192, 64, 3, 72),        # N is neither 64 nor a multiple of 128
                                                  (128, 128, 160, 64, 3, None)])    # a ragged last slab (32 rows)
def test_ineligible_shapes_stay_on_the_tiled_kernel(M, N, K, rows, slabs, ldb):
    (tiled, stream), desc, A, Bm, stride, launches = _run_both(M, N, K, rows, slabs, 2, ldb=ldb)
    assert launches[0] == (0, 1) and launches[1] == (0, 1), launches
    _check_against_float64(stream, desc, A, Bm, rows, slabs, K)
    assert np.array_equal(tiled, stream)


@pytest.mark.parametrize("nontemporal", [False, True])
def test_bias_chains_of_the_128_column_tiled_kernel(nontemporal):
    """The cases above are so small that the tile rule puts the tiled arm on 64-column tiles (four bias chains per column, the
    form the new kernel then follows).  From 128 tiles of 64 x 128 up the tiled kernel runs 128-column tiles with two chains of 32
    rows per 64-row K-tile - the form of every large launch: 4 groups x 4 slabs of a 256 x 256 layer."""
    M = N = 256
    rows, slabs, groups = 128, 4, 4
    (tiled, stream), desc, A, Bm, stride, launches = _run_both(M, N, rows * slabs, rows, slabs, groups, nontemporal=nontemporal)
    assert launches[0] == (0, 1) and launches[1] == (1, 0), launches
    _check_against_float64(stream, desc, A, Bm, rows, slabs, rows * slabs)
    assert np.array_equal(tiled, stream)
