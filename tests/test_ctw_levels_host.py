"""CPU: the order-free statement of the CTW tree (tests/_oracle_ctw_levels.py, the checker of the device level build in
csrc/dib_ctw_levels.h) against the host estimator csrc/dib_ctw.cpp, the depth-512 guard, and the surface of the device
backend that needs no GPU (keywords, declarations, the host-only entry points of include/dib_ctw_device.h)."""
import inspect
import os
import re

import numpy as np
import pytest

import _oracle_ctw_levels as lv
from dib_amd import ctw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_as_host(seq, A):
    r = lv.ctw_levels(seq, A)
    assert not r["deep"]
    host = ctw.estimate_entropy(seq, A)
    assert r["rate"] == host or (np.isnan(r["rate"]) and np.isnan(host)), (A, len(seq), r["rate"], host)
    assert r["nodes"] == ctw.node_count(seq, A), (A, len(seq))
    return r


def test_restatement_equals_the_host_estimator_on_the_random_grid():
    cases = lv.grid_cases()
    assert len(cases) == 288
    compared = 0
    for A, seq in cases:
        if lv.ctw_levels(seq, A)["deep"]:
            continue
        _same_as_host(seq, A)
        compared += 1
    assert compared >= 250   # the guard fires on a few of the 0.99-zeros sequences only


@pytest.mark.parametrize("n", [512, 513])
def test_zeros_up_to_the_last_level_are_equal(n):
    r = _same_as_host(np.zeros(n, dtype=np.uint8), 2)
    assert r["nodes"] == n and len(r["level_nodes"]) == n


def test_period_three_below_the_last_level():
    assert _same_as_host(np.array([0, 1, 1] * 100, dtype=np.uint8), 2)["nodes"] == 888


def test_logistic_map_20000_symbols():
    r = _same_as_host(lv.logistic_symbols(20_000), 2)
    assert r["nodes"] == 48_734
    assert r["level_moving"][0] == 19_999 and r["level_moving"][-1] == 0


@pytest.mark.parametrize("name", ["zeros514", "zeros515", "period3x300", "block512", "block513"])
def test_guard_fires(name):
    seq = {"zeros514": np.zeros(514, np.uint8), "zeros515": np.zeros(515, np.uint8),
           "period3x300": np.array([0, 1, 1] * 300, np.uint8), "block512": lv.repeated_block(512),
           "block513": lv.repeated_block(513)}[name]
    r = lv.ctw_levels(seq, 2)
    assert r["deep"] and len(r["level_nodes"]) == lv.MAX_LEVEL + 1
    if name == "period3x300":   # why the guard is needed: the host's tree goes on below level 512
        assert r["nodes"] == 1536 and ctw.node_count(seq, 2) == 1539


def test_single_symbol_alphabet_and_empty_window():
    assert not lv.ctw_levels(np.zeros(513, np.uint8), 1)["deep"]
    assert lv.ctw_levels(np.zeros(514, np.uint8), 1)["deep"]
    r = lv.ctw_levels(np.zeros(0, np.uint8), 2)
    assert np.isnan(r["rate"]) and r["nodes"] == 1 and r["code_length_bits"] == 0.0


def test_backend_keywords_exist_and_default_to_host():
    from dib_amd import measurement, random_partition
    assert inspect.signature(ctw.estimate_entropy_batch).parameters["backend"].default == "host"
    assert inspect.signature(ctw.estimate_entropy_windows).parameters["backend"].default == "device"
    for fn in (measurement.entropy_rate_fit, measurement.characterize_partition, random_partition.RandomPartition.characterize,
               random_partition.random_partition_survey):
        assert inspect.signature(fn).parameters["ctw_backend"].default == "host", fn
    for tool in ("partition_run.py", "measurement_run.py"):
        assert "--ctw_backend" in open(os.path.join(ROOT, "tools", tool)).read()
    with pytest.raises(ValueError):
        ctw.estimate_entropy_batch([np.zeros(4, np.uint8)], 2, backend="gpu")


def test_host_backend_of_the_windows_function_equals_the_batch():
    seq = lv.logistic_symbols(3000)
    starts, lengths = [0, 100, 100, 2990], [500, 700, 700, 10]
    rates, det = ctw.estimate_entropy_windows(seq, starts, lengths, 2, backend="host", return_details=True)
    want = ctw.estimate_entropy_batch([seq[s: s + n] for s, n in zip(starts, lengths)], 2)
    assert np.array_equal(rates, want) and det["fallback"].all()
    with pytest.raises(ValueError):
        ctw.estimate_entropy_windows(seq, [2990], [11], 2, backend="host")


def test_entropy_rate_fit_default_is_unchanged_by_the_keyword():
    from dib_amd import measurement
    seq = lv.logistic_symbols(4000)
    a = measurement.entropy_rate_fit(seq, 2, number_data_points=[200, 500, 1000], number_rand_draws=3, threads=2)
    b = measurement.entropy_rate_fit(seq, 2, number_data_points=[200, 500, 1000], number_rand_draws=3, threads=2, ctw_backend="host")
    assert np.array_equal(a["entropy_rate_values"], b["entropy_rate_values"]) and a["entropy_rate"] == b["entropy_rate"]
    assert "ctw_details" not in a


def test_header_functions_are_declared_exported_and_included():
    from dib_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dib_ctw_device.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t)\s+(dib_ctw_device_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == set(_lib.SIGNATURES_CTW_DEVICE) and len(declared) == 3
    assert '#include "dib_ctw_device.h"' in open(os.path.join(ROOT, "include", "dib_hip.h")).read()
    lib = _lib.load_library()
    assert lib.dib_abi_version() == 7
    for name in declared:
        assert hasattr(lib, name)


def test_envelope_and_workspace_query_without_a_gpu():
    from dib_amd import _lib
    lib = _lib.load_library()
    assert lib.dib_ctw_device_supported(1, 0, 0) == 1 and lib.dib_ctw_device_supported(16, 2 ** 31 - 1, 75) == 1
    assert lib.dib_ctw_device_supported(17, 100, 1) == 0 and lib.dib_ctw_device_supported(0, 100, 1) == 0
    assert lib.dib_ctw_device_supported(2, 2 ** 31, 1) == 0
    assert lib.dib_ctw_device_workspace_bytes(100, 1, 17, 1000) == -1
    assert lib.dib_ctw_device_workspace_bytes(2 ** 31, 1, 2, 1000) == -1
    assert lib.dib_ctw_device_workspace_bytes(100, 4, 2, 3) == -1          # fewer nodes than roots
    small, more_nodes, more_symbols = (lib.dib_ctw_device_workspace_bytes(*a) for a in
                                       ((1000, 3, 2, 5000), (1000, 3, 2, 50_000), (100_000, 3, 2, 5000)))
    assert 0 < small < more_nodes and small < more_symbols
    assert lib.dib_ctw_device_workspace_bytes(1000, 3, 16, 5000) > small    # the key arrays grow with the alphabet


def test_chunk_plan_covers_every_window_once_and_respects_the_budget(monkeypatch):
    from dib_amd import _lib
    lib = _lib.load_library()
    monkeypatch.setattr(ctw, "MIN_NODE_CAPACITY", 1024)
    lengths = np.array([200, 5000, 300, 0, 4000, 1200, 700], dtype=np.int64)
    whole = ctw._plan_chunks(lib, lengths, 2, ctw.DEFAULT_WORKSPACE_BUDGET)
    assert whole == [(0, 7, ctw._node_capacity(int(lengths.sum()), 7))]
    budget = int(lib.dib_ctw_device_workspace_bytes(4000, 1, 2, ctw._node_capacity(4000, 1)))
    plan = ctw._plan_chunks(lib, lengths, 2, budget)
    assert [a for a, _, _ in plan] == [0] + [b for _, b, _ in plan[:-1]] and plan[-1][1] == 7 and len(plan) >= 3
    for a, b, cap in plan:
        assert lib.dib_ctw_device_workspace_bytes(int(lengths[a:b].sum()), b - a, 2, cap) <= budget
    (_, _, cap5000), = [c for c in plan if c[0] == 1]
    assert cap5000 < ctw._node_capacity(5000, 1)   # the window that does not fit gets what the budget leaves
