"""The exhaustive subset informations on the device (include/dib_subsets.h, csrc/dib_subsets.h, dib_amd.subset_information):
  - dib_subset_information against the float64 host backend (which tests/test_subset_information_host.py holds to the notebook's
    own numbers and to a brute-force restatement) across the envelope - key widths on both sides of the wave, the workgroup and
    the number of low bits a workgroup folds (8 / 7 / 6 for K <= 2 / <= 6 / <= 16), every class count that changes the LDS row,
    full cubes, one row, a sparse sample with duplicates, multi-bit features - and with the fold width forced through its tuning
    key: 1e-10 bits, the empty subset 0.0 exactly, guard bands untouched;
  - known answers by equality; chunked calls, a second placement and graph replay by equality of bits; refusals that write nothing;
  - the paper circuit against the notebook's numbers, and the ranks of the notebook's printed subset sequence.
Tolerance 1e-10 bits: a float64 sum of 2^13 terms totalling at most 12 bits errs by about 1e-11 in the worst case; 10x margin for
the last place of log2."""
import ctypes
import functools
import importlib.util
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dib_amd import circuit  # noqa: E402
from dib_amd import subset_information as si  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-10
GUARD = 64
SENTINEL = -777.25
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED
GOLDEN = os.path.join(ROOT, "tests", "golden", "subset_mi.npz")


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device(T, fb, mask0=0, n_masks=None, shift=0):
    """one dib_subset_information call on counts T [2^B, K] -> out [n_masks] float64.  counts and out sit `shift` elements into
    their buffers, out between guard bands that must come back untouched."""
    lib = _lib()
    B, K, F = int(T.shape[0]).bit_length() - 1, T.shape[1], len(fb)
    n_masks = (1 << F) - mask0 if n_masks is None else n_masks
    cbuf = torch.zeros(T.size + shift, dtype=torch.int32, device="cuda")
    cbuf[shift:] = torch.from_numpy(T.astype(np.int32).reshape(-1)).cuda()
    buf = torch.full((n_masks + 2 * GUARD + shift,), SENTINEL, dtype=torch.float64, device="cuda")
    out = buf[GUARD + shift:GUARD + shift + n_masks]
    nws = int(lib.dib_subset_information_workspace_bytes(B, K))
    assert nws >= 0
    ws = torch.zeros(max(nws, 8), dtype=torch.uint8, device="cuda")
    n0 = lib.dib_launch_count()
    rc = lib.dib_subset_information(_p(cbuf[shift:]), B, K, (ctypes.c_int * F)(*fb), F, mask0, n_masks, _p(out), _p(ws), _st())
    assert rc == 0, rc
    assert lib.dib_launch_count() == n0 + 1   # one launch per call
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:GUARD + shift] == SENTINEL).all() and (b[GUARD + shift + n_masks:] == SENTINEL).all()
    return b[GUARD + shift:GUARD + shift + n_masks].copy()


class _low_bits:
    """dib_set_tuning("subset_low_bits", L) for the block"""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        from dib_amd import _lib
        self.old = _lib.get_tuning("subset_low_bits")
        _lib.set_tuning("subset_low_bits", self.L)

    def __exit__(self, *exc):
        from dib_amd import _lib
        _lib.set_tuning("subset_low_bits", self.old)


@functools.lru_cache(maxsize=None)
def _case(fb, K, rows, seed=0):
    """(T, host bits) of a sample: rows "cube" = every key once, with a random class; an int = that many random rows (duplicates
    and missing patterns); class K - 1 always occurs, so the table has K columns"""
    fb = list(fb)
    B = sum(fb)
    rng = np.random.default_rng(1000 * B + 10 * K + seed)
    if rows == "cube":
        keys = np.arange(1 << B)
    else:
        keys = rng.integers(0, 1 << B, rows)
    y = rng.integers(0, K, len(keys))
    y[0] = K - 1
    off = np.cumsum([0] + fb[:-1])
    x = np.stack([(keys >> o) & ((1 << b) - 1) for o, b in zip(off, fb)], 1)
    T, fb2, K2 = si.joint_counts(x, y, fb)
    assert K2 == K and fb2 == fb
    want = si._host_bits(T, fb)
    want.setflags(write=False)
    return T, want


def _check(fb, K, rows, **kw):
    T, want = _case(tuple(fb), K, rows)
    got = _device(T, fb, **kw)
    err = float(np.abs(got - want).max())
    print(f"B {sum(fb)} F {len(fb)} K {K} rows {rows}: max |device - host| = {err:.3e} bits")
    assert got[0] == 0.0 and err <= TOL, (fb, K, rows, err)
    return got


# B: 1, 2 (less than a wave of low subsets), 5 / 6 / 7 (32, 64, 128 low subsets: the wave boundary), 8 (one lane per low subset,
# still one workgroup at K = 2), 9 / 10 / 12 (2 / 4 / 16 workgroups at K = 2; 64 at K = 16).  The fold takes 8 low bits at K = 2,
# 7 at K = 3 and 5, 6 at K = 16: B = 6 / 7 / 8 / 9 are the last one-workgroup and the first many-workgroup sizes of each.
@pytest.mark.parametrize("B", [1, 2, 5, 6, 7, 8, 9, 10, 12])
def test_device_matches_the_host_backend_across_the_envelope(B):
    for K in (2, 3, 5, 16):
        for rows in ("cube", 1, 37) + ((5000,) if B == 10 else ()):
            _check([1] * B, K, rows)


@pytest.mark.parametrize("fb", [[2, 1, 3], [3, 3, 3, 1], [1, 9], [9, 1, 1], [4, 4, 4]])
def test_multi_bit_features(fb):
    """F < B: bit fields inside the low bits, inside the high bits and across the boundary between them (with 8 low bits:
    [3, 3, 3, 1] cuts the third field, [1, 9] and [9, 1, 1] the wide one, [4, 4, 4] none)"""
    for K in (2, 5):
        _check(fb, K, 300)
    with _low_bits(2):
        _check(fb, 2, 300)


@pytest.mark.parametrize("L", [1, 2, 3, 5, 7])
def test_every_fold_width_forced_through_its_tuning_key(L):
    """the one kernel at every number of low bits the default rule can pick, and below: L low bits leave 2^(B - L) workgroups"""
    from dib_amd import _lib
    with _low_bits(L):
        assert _lib.get_tuning("subset_low_bits") == L
        for B, K in ((7, 2), (9, 3), (8, 16)):
            _check([1] * B, K, "cube")
            _check([1] * B, K, 37)
    assert _lib.get_tuning("subset_low_bits") == 0


def _cube(n):
    return (np.arange(1 << n)[:, None] >> np.arange(n)) & 1


@pytest.mark.parametrize("n", [6, 10])
def test_known_answers_are_exact(n):
    """parity of k of n inputs: exactly 0 on every S missing one of the k, 1 otherwise; y = x_j: 1 iff j in S; constant y: zeros"""
    x = _cube(n)
    masks = np.arange(1 << n)
    for inputs in (list(range(n)), [1, 4], [0, 2, n - 1]):
        need = sum(1 << i for i in inputs)
        T, _, _ = si.joint_counts(x, x[:, inputs].sum(1) & 1)
        for L in (0, 3):
            with _low_bits(L):
                got = _device(T, [1] * n)
            assert np.array_equal(got, ((masks & need) == need).astype(np.float64)), (inputs, L)
    for j in (0, n - 1):
        T, _, _ = si.joint_counts(x, x[:, j])
        assert np.array_equal(_device(T, [1] * n), ((masks >> j) & 1).astype(np.float64))
    T, _, _ = si.joint_counts(x, np.zeros(1 << n, dtype=np.int64))
    assert T.shape[1] == 1 and np.array_equal(_device(T, [1] * n), np.zeros(1 << n))


@pytest.mark.parametrize("fb,K", [([1] * 10, 2), ([1] * 9, 5), ([2, 1, 3, 1, 1, 1, 1], 3)])
def test_chunks_and_placement_do_not_change_the_bits(fb, K):
    T, _ = _case(tuple(fb), K, 300)
    F = len(fb)
    whole = _check(fb, K, 300)
    assert np.array_equal(_device(T, fb, shift=3), whole)   # a second placement of counts and out
    for n in (1, 3, 64):
        for mask0 in (1, 7, (1 << F) - n - (1 - n % 2)):   # odd starts
            assert mask0 % 2 == 1
            assert np.array_equal(_device(T, fb, mask0=mask0, n_masks=n), whole[mask0:mask0 + n]), (mask0, n)
    parts = [_device(T, fb, mask0=m, n_masks=min(64, (1 << F) - m)) for m in range(0, 1 << F, 64)]
    assert np.array_equal(np.concatenate(parts), whole)


def test_graph_replay_has_the_eager_bits():
    lib = _lib()
    fb = [1] * 10
    T, _ = _case(tuple(fb), 3, 300)
    T2, _ = _case(tuple(fb), 3, 37)
    eager, eager2 = _device(T, fb), _device(T2, fb)
    counts = torch.from_numpy(T.astype(np.int32)).cuda()
    out = torch.zeros(1024, dtype=torch.float64, device="cuda")
    widths = (ctypes.c_int * 10)(*fb)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # the call neither allocates nor synchronises: it can be captured
        rc = lib.dib_subset_information(_p(counts), 10, 3, widths, 10, 0, 1024, _p(out), None, _st())
    assert rc == 0
    for _ in range(2):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager)
    counts.copy_(torch.from_numpy(T2.astype(np.int32)))   # a replay reads the buffers as they are now
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), eager2)


def test_refused_calls_launch_nothing_and_write_nothing():
    lib = _lib()
    counts = torch.ones((1 << 10) * 16, dtype=torch.int32, device="cuda")
    out = torch.full((1 << 10,), SENTINEL, dtype=torch.float64, device="cuda")
    ones = [1] * 21
    n0 = lib.dib_launch_count()

    def call(counts_=counts, B=10, K=2, fb=None, F=10, mask0=0, n=1 << 10, out_=out, no_fb=False):
        widths = None if no_fb else (ctypes.c_int * len(fb or ones))(*(fb or ones))
        return lib.dib_subset_information(_p(counts_), B, K, widths, F, mask0, n, _p(out_), None, _st())

    assert call(B=21, F=21) == UNSUPPORTED and call(K=17) == UNSUPPORTED and call(F=11) == UNSUPPORTED
    assert call(counts_=None) == ARG and call(out_=None) == ARG and call(no_fb=True) == ARG
    assert call(B=0) == ARG and call(K=0) == ARG and call(F=0) == ARG
    assert call(fb=[1] * 9 + [2]) == ARG and call(fb=[1] * 9 + [0]) == ARG and call(F=9) == ARG   # sum feature_bits != B
    assert call(mask0=-1) == ARG and call(n=0) == ARG and call(mask0=1) == ARG and call(n=(1 << 10) + 1) == ARG
    assert lib.dib_subset_information_supported(20, 20, 16) == 1 and lib.dib_subset_information_supported(21, 21, 2) == 0
    assert lib.dib_subset_information_supported(10, 11, 2) == 0 and lib.dib_subset_information_supported(10, 10, 17) == 0
    assert lib.dib_subset_information_workspace_bytes(21, 2) == -1 and lib.dib_subset_information_workspace_bytes(10, 17) == -1
    torch.cuda.synchronize()
    assert lib.dib_launch_count() == n0
    assert (out.cpu().numpy() == SENTINEL).all()
    # the Python surface refuses before anything is uploaded
    with pytest.raises(ValueError, match="20 bits"):
        si.subset_information(np.zeros((4, 21)), np.zeros(4))
    assert lib.dib_launch_count() == n0


def test_paper_circuit_matches_the_notebook_and_ranks_its_printed_sequence():
    fx = np.load(GOLDEN)
    tt = fx["truth_table"]
    dev = si.subset_information(tt[:, :10], tt[:, 10])
    host = si.subset_information(tt[:, :10], tt[:, 10], backend="host")
    err = float(np.abs(dev.bits[si.subset_masks(fx["all_on_off_combos"])] - fx["all_mis_bits"]).max())
    print(f"paper circuit: max |device - notebook| = {err:.3e} bits")
    assert err <= TOL and dev.bits[0] == 0.0 and abs(dev.entropy_y_bits - float(fx["entropy_y_bits"])) <= 1e-12
    spec = importlib.util.spec_from_file_location("circuit_run", os.path.join(ROOT, "tools", "circuit_run.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ranks = [dev.rank(s) for s in mod.NOTEBOOK_FIG1_SEQUENCE]
    print("ranks of the notebook's printed sequence among the subsets of their size:", ranks)
    assert ranks == [host.rank(s) for s in mod.NOTEBOOK_FIG1_SEQUENCE]
    assert ranks[-1] == 0 and ranks[-2] == host.by_size(1)[0].tolist().index(1 << 2)
    assert np.abs(dev.shapley_values() - host.shapley_values()).max() <= TOL
    # circuit.subset_comparison on curves that walk the notebook's sequence
    seq = [list(range(10))] + mod.NOTEBOOK_FIG1_SEQUENCE
    parts = np.array([[1.0 if g in s else 0.0 for g in range(10)] for s in seq])
    rows = circuit.subset_comparison(parts, tt)
    assert [r["gates"] for r in rows[:-1]] == mod.NOTEBOOK_FIG1_SEQUENCE and [r["rank"] for r in rows[:-1]] == ranks
    assert all(abs(r["information_bits"] - host.bits[r["mask"]]) <= TOL for r in rows)


def test_random_circuit_of_14_gates():
    """the largest case: a random 14-input circuit (data.random_circuit, the generator of `--boolean_random_circuit True`), device against host.  The host
    backend took 0.22 s at 14 bits beside the MI355X and 0.6 s on a slower CPU, so the case is not skipped."""
    import dib_amd
    table = dib_amd.data.truth_table(dib_amd.data.random_circuit(14, np.random.default_rng(3)), 14)
    x, y = table[:, :14], table[:, -1]
    assert x.shape == (1 << 14, 14)
    t0 = time.perf_counter()
    host = si.subset_information(x, y, backend="host")
    t_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev = si.subset_information(x, y)
    t_dev = time.perf_counter() - t0
    err = float(np.abs(dev.bits - host.bits).max())
    print(f"14 gates: host {t_host:.3f} s, device call {t_dev:.3f} s, max |device - host| = {err:.3e} bits")
    assert err <= TOL and dev.bits[0] == 0.0
    assert abs(dev.bits[-1] - host.entropy_y_bits) <= TOL   # a deterministic circuit: all inputs carry all of H(Y)
