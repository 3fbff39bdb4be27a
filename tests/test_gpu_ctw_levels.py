"""The CTW entropy-rate estimator built level by level on the device (include/dib_ctw_device.h, csrc/dib_ctw_levels.h,
dib_amd.ctw.estimate_entropy_windows) against the order-free restatement tests/_oracle_ctw_levels.py (float64 NumPy) and the
host estimator csrc/dib_ctw.cpp.

Bounds.  The depth guard, the node counts and the statuses are integers: equality.  The rate is the host's float32 value or
one of its two float32 neighbours (the mixture's log2 / exp2 are the device's).  The unrounded code length against the oracle's
float64: CODE_LENGTH_BOUND below, 16 x the largest relative difference measured over the grid (profiles/ctw_device_bench.json,
"grid_max_relative_code_length_difference"), never above 2^-24, beyond which the rounded rate could move by more than a float32
step."""
import ctypes

import numpy as np
import pytest

import _oracle_ctw_levels as lv

pytestmark = pytest.mark.gpu

MEASURED_GRID_DIFFERENCE = 3.464262089524407e-16   # profiles/ctw_device_bench.json; 284 of the 288 cases are bit-equal
CODE_LENGTH_BOUND = min(16 * MEASURED_GRID_DIFFERENCE, 2.0 ** -24)


def _f32_steps(a, b):
    """distance in float32 steps between two arrays of (positive or NaN) rates"""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.fixture(scope="module")
def ctw():
    import torch
    assert torch.cuda.is_available()
    from dib_amd import ctw
    return ctw


@pytest.fixture(scope="module")
def grid(ctw):
    """per alphabet: the sequences laid end to end, their windows, the oracle's results and the host's rates / node counts -
    computed once, read by the tests below"""
    out = {}
    for A in lv.GRID_ALPHABETS:
        seqs = [s for a, s in lv.grid_cases() if a == A]
        lengths = np.array([len(s) for s in seqs], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        orc = [lv.ctw_levels(s, A) for s in seqs]
        out[A] = dict(flat=np.concatenate(seqs), starts=starts, lengths=lengths, seqs=seqs,
                      deep=np.array([o["deep"] for o in orc]), bits=np.array([o["code_length_bits"] for o in orc]),
                      host_rate=ctw.estimate_entropy_batch(seqs, A, threads=4),
                      host_nodes=np.array([ctw.node_count(s, A) for s in seqs]))
    assert sum(len(g["seqs"]) for g in out.values()) == 288
    return out


@pytest.fixture(scope="module")
def grid_device(ctw, grid):
    """the 288 cases through the device path, one call per alphabet"""
    return {A: ctw.estimate_entropy_windows(g["flat"], g["starts"], g["lengths"], A, return_details=True) for A, g in grid.items()}


def test_grid_status_node_counts_and_rates(ctw, grid, grid_device):
    for A, g in grid.items():
        rates, det = grid_device[A]
        deep = (det["status"] & ctw.STATUS_DEEP) != 0
        assert np.array_equal(deep, g["deep"]), (A, np.where(deep != g["deep"])[0])
        assert np.array_equal(det["status"][~deep], np.zeros((~deep).sum(), np.int32))
        assert np.array_equal(det["nodes"][~deep], g["host_nodes"][~deep]), A
        steps = _f32_steps(rates, g["host_rate"])
        print(f"A={A}: {int(deep.sum())} deep of {len(deep)}, rates off by one float32 step: {int((steps == 1).sum())}")
        assert steps.max() <= 1, (A, steps.max())
        assert np.array_equal(det["fallback"], deep)
        assert 1 <= det["chunks"] <= 1 + deep.sum()      # a window that fills the shared node capacity is run again alone
        assert np.array_equal(rates[deep], g["host_rate"][deep])          # recomputed on the host: its value exactly
        assert (det["nodes"][deep] == -1).all() and np.isnan(det["code_length_bits"][deep]).all()


def test_grid_unrounded_code_length(grid, grid_device):
    worst = 0.0
    for A, g in grid.items():
        _, det = grid_device[A]
        ok = ~g["deep"]
        rel = np.abs(det["code_length_bits"][ok] - g["bits"][ok]) / g["bits"][ok]
        worst = max(worst, float(rel.max()))
        print(f"A={A}: largest relative difference of the unrounded code length {rel.max():.3e}, bit-equal {int((rel == 0).sum())} of {int(ok.sum())}")
    print(f"grid_max_relative_code_length_difference {worst:.6e}  (bound {CODE_LENGTH_BOUND:.6e})")
    assert worst <= CODE_LENGTH_BOUND


def test_edges_short_windows_single_symbol_alphabet_and_sixteen_symbols(ctw):
    seq = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    starts, lengths = [0, 0, 1, 2, 4, 6, 7], [0, 1, 2, 3, 3, 1, 0]    # a window ends at the last symbol; one starts past it, empty
    rates, det = ctw.estimate_entropy_windows(seq, starts, lengths, 2, return_details=True)
    assert np.isnan(rates[0]) and np.isnan(rates[6]) and not det["fallback"].any()
    assert det["nodes"][0] == 1 and det["code_length_bits"][0] == 0.0
    for w in range(1, 6):
        s = seq[starts[w]: starts[w] + lengths[w]]
        o = lv.ctw_levels(s, 2)
        assert det["nodes"][w] == o["nodes"] == ctw.node_count(s, 2)
        assert _f32_steps(rates[w], ctw.estimate_entropy(s, 2)) <= 1
        assert abs(det["code_length_bits"][w] - o["code_length_bits"]) <= CODE_LENGTH_BOUND * o["code_length_bits"]
    # A = 1: 513 symbols reach the last level exactly, 514 pass it
    zeros = np.zeros(514, dtype=np.uint8)
    rates, det = ctw.estimate_entropy_windows(zeros, [0, 0], [513, 514], 1, return_details=True)
    assert det["status"].tolist() == [0, ctw.STATUS_DEEP] and det["fallback"].tolist() == [False, True]
    assert det["nodes"][0] == 513 and det["levels"] == 513
    assert rates[0] == 0.0 and rates[1] == ctw.estimate_entropy(zeros, 1)
    # A = 16, lengths on both sides of the 1024-element tile, several workgroups
    rng = np.random.default_rng(3)
    s16 = rng.integers(0, 16, size=6000).astype(np.uint8)
    s16[rng.random(6000) < 0.5] = 15
    st, ln = [0, 1000, 1000, 0, 4976], [1023, 1025, 1025, 6000, 1024]    # identical windows, overlapping windows, the array's end
    rates, det = ctw.estimate_entropy_windows(s16, st, ln, 16, return_details=True)
    assert not det["fallback"].any()
    assert rates[1] == rates[2] and det["code_length_bits"][1] == det["code_length_bits"][2] and det["nodes"][1] == det["nodes"][2]
    for w in range(5):
        s = s16[st[w]: st[w] + ln[w]]
        o = lv.ctw_levels(s, 16)
        assert det["nodes"][w] == o["nodes"] == ctw.node_count(s, 16)
        assert _f32_steps(rates[w], ctw.estimate_entropy(s, 16)) <= 1
        assert abs(det["code_length_bits"][w] - o["code_length_bits"]) <= CODE_LENGTH_BOUND * o["code_length_bits"]


@pytest.fixture(scope="module")
def logistic_windows(ctw):
    """75 windows of 200 to 5000 symbols of one logistic-map sequence (window 40 is the one of 5000), the sequence on the
    device, and the unchunked device result"""
    import torch
    seq = lv.logistic_symbols(20_000)
    rng = np.random.default_rng(11)
    lengths = rng.integers(200, 2001, size=75).astype(np.int64)
    lengths[40] = 5000
    starts = np.array([rng.integers(0, len(seq) - n + 1) for n in lengths], dtype=np.int64)
    starts[7], lengths[7] = len(seq) - 900, 900      # ends at the last symbol of the array
    dev = torch.from_numpy(seq).to("cuda")
    rates, det = ctw.estimate_entropy_windows(dev, starts, lengths, 2, return_details=True)
    return seq, dev, starts, lengths, rates, det


def test_75_logistic_windows_in_one_call_against_the_host_batch(ctw, logistic_windows):
    seq, dev, starts, lengths, rates, det = logistic_windows
    assert det["chunks"] == 1 and det["symbols_on_device"] and not det["fallback"].any()
    host = ctw.estimate_entropy_batch([seq[s: s + n] for s, n in zip(starts, lengths)], 2, threads=4)
    assert _f32_steps(rates, host).max() <= 1
    assert np.array_equal(det["nodes"], [ctw.node_count(seq[s: s + n], 2) for s, n in zip(starts, lengths)])
    assert det["element_steps"] > lengths.sum() and det["levels"] > 10
    batch = ctw.estimate_entropy_batch([seq[s: s + n] for s, n in zip(starts[:5], lengths[:5])], 2, backend="device")
    assert np.array_equal(batch, rates[:5])      # the batch form lays the windows end to end: other calls, the same bits


def test_chunks_do_not_change_the_bits_and_an_overflowing_window_goes_to_the_host(ctw, logistic_windows, monkeypatch):
    from dib_amd import _lib
    seq, dev, starts, lengths, rates, det = logistic_windows
    lib = _lib.load_library()
    # without the floor of the node capacity, room for any window of up to 2000 symbols at 4 nodes per symbol (a logistic window
    # takes 1.5); the window of 5000 gets what the budget leaves it, about 4500 nodes where it needs 7300
    monkeypatch.setattr(ctw, "MIN_NODE_CAPACITY", 1024)
    budget = int(lib.dib_ctw_device_workspace_bytes(2000, 1, 2, ctw._node_capacity(2000, 1)))
    r2, d2 = ctw.estimate_entropy_windows(dev, starts, lengths, 2, return_details=True, workspace_budget=budget)
    assert d2["chunks"] >= 3
    assert d2["fallback"].sum() == 1 and d2["fallback"][40] and d2["status"][40] == ctw.STATUS_OVERFLOW
    assert r2[40] == ctw.estimate_entropy(seq[starts[40]: starts[40] + 5000], 2)
    keep = np.arange(75) != 40
    assert np.array_equal(r2[keep], rates[keep])
    assert np.array_equal(d2["code_length_bits"][keep], det["code_length_bits"][keep])
    assert np.array_equal(d2["nodes"][keep], det["nodes"][keep])
    monkeypatch.undo()
    # the same call twice
    r3, d3 = ctw.estimate_entropy_windows(dev, starts, lengths, 2, return_details=True)
    assert np.array_equal(r3, rates) and np.array_equal(d3["code_length_bits"], det["code_length_bits"])
    assert np.array_equal(d3["nodes"], det["nodes"])


def test_refusals_launch_nothing_and_write_nothing(ctw):
    import torch
    from dib_amd import _lib
    lib = _lib.load_library()
    sym = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((3, 2), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n_symbols, starts, lengths, A, cap=4096, ws_bytes=1 << 22):
        s, l = np.array(starts, dtype=np.int64), np.array(lengths, dtype=np.int64)
        return lib.dib_ctw_device_estimate(ctypes.c_void_p(sym.data_ptr()), n_symbols, s.ctypes.data, l.ctypes.data, len(s), A, cap,
                                           ctypes.c_void_p(out[0].data_ptr()), ctypes.c_void_p(out[1].data_ptr()),
                                           ctypes.c_void_p(out[2].data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                           ctypes.c_void_p(ws.data_ptr()), ws_bytes, None, stream)

    n0 = lib.dib_launch_count()
    assert call(64, [0, 8], [32, 32], 17) == -4                                   # DIB_E_UNSUPPORTED: the alphabet
    assert call(2 ** 30, [0, 0], [2 ** 30, 2 ** 30], 2) == -4                     # the total: 2^31 symbols (never touched)
    assert call(64, [0, 40], [32, 32], 2) == -1                                   # DIB_E_ARG: a window leaves the array
    assert call(64, [0, 8], [32, 32], 2, cap=1) == -1                             # fewer nodes than roots
    assert call(64, [0, 8], [32, 32], 2, ws_bytes=1024) == -3                     # DIB_E_WORKSPACE
    torch.cuda.synchronize()
    assert lib.dib_launch_count() == n0
    assert torch.isnan(out).all() and (st == -7).all()
    assert lib.dib_ctw_device_supported(17, 64, 2) == 0 and lib.dib_ctw_device_supported(16, 64, 2) == 1
    assert call(64, [0, 8], [32, 32], 2) == 0                                     # and the same buffers serve a good call
    torch.cuda.synchronize()
    assert lib.dib_launch_count() > n0 and (st == 0).all() and not torch.isnan(out[:2]).any()


def test_a_symbol_outside_the_alphabet_raises(ctw):
    import torch
    seq = lv.logistic_symbols(600)
    bad = seq.copy()
    bad[411] = 2
    with pytest.raises(ValueError, match=r"symbols must lie in \[0, 2\)"):
        ctw.estimate_entropy_windows(bad, [0, 300], [300, 300], 2)                # found on the host before the upload
    with pytest.raises(ValueError, match=r"symbols must lie in \[0, 2\)"):
        ctw.estimate_entropy_windows(torch.from_numpy(bad).to("cuda"), [0, 300], [300, 300], 2)   # found by the kernel
    with pytest.raises(ValueError):
        ctw.estimate_entropy_windows(seq, [0], [300], 17)


def test_entropy_rate_fit_on_the_device_backend():
    from dib_amd import measurement
    seq = lv.logistic_symbols(20_000)
    kw = dict(number_data_points=[200, 500, 1000], number_rand_draws=3, threads=4)
    host = measurement.entropy_rate_fit(seq, 2, **kw)
    dev = measurement.entropy_rate_fit(seq, 2, ctw_backend="device", **kw)
    assert _f32_steps(dev["entropy_rate_values"], host["entropy_rate_values"]).max() <= 1
    assert not dev["ctw_details"]["fallback"].any() and dev["ctw_details"]["chunks"] == 1
    # the fitted rate agrees to the precision the fit has: the host backend's own error estimate.  Three lengths determine the
    # three parameters of the ansatz exactly, so curve_fit reports no finite error at the sizes above; five lengths do.
    print("fit, 3 lengths:", host["entropy_rate"], dev["entropy_rate"], "err", host["entropy_rate_err"])
    assert abs(dev["entropy_rate"] - host["entropy_rate"]) <= host["entropy_rate_err"]
    kw["number_data_points"] = [200, 350, 500, 700, 1000]
    host5 = measurement.entropy_rate_fit(seq, 2, **kw)
    dev5 = measurement.entropy_rate_fit(seq, 2, ctw_backend="device", **kw)
    print("fit, 5 lengths:", host5["entropy_rate"], dev5["entropy_rate"], "err", host5["entropy_rate_err"])
    assert np.isfinite(host5["entropy_rate_err"])
    assert abs(dev5["entropy_rate"] - host5["entropy_rate"]) <= host5["entropy_rate_err"]


def test_random_partition_characterize_keeps_the_symbols_on_the_device():
    import torch
    import _oracle_random_partition as orp
    from dib_amd import random_partition as rp
    x = orp.logistic_trajectory(20_000)
    part = rp.RandomPartition(1, 2, 1, "linear", units_per_mlp_layer=16, weights=orp.generating_partition_weights())
    kw = dict(number_data_points=[200, 500, 1000], number_rand_draws=3, threads=4)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    dev = part.characterize(xd, ctw_backend="device", **kw)
    host = part.characterize(x, **kw)
    det = dev["ctw_details"]
    assert det["symbols_on_device"] and det["chunks"] == 1 and not det["fallback"].any() and (det["status"] == 0).all()
    assert det["element_steps"] > 0 and (det["nodes"] > 0).all()
    assert dev["entropy_single_timestep"] == host["entropy_single_timestep"]
    assert _f32_steps(dev["entropy_rate_values"], host["entropy_rate_values"]).max() <= 1
    sym = part.symbolize_device(xd)
    again = part.characterize(sym, ctw_backend="device", **kw)      # uint8 symbols already on the device
    assert np.array_equal(again["entropy_rate_values"], dev["entropy_rate_values"]) and again["ctw_details"]["symbols_on_device"]
