"""CPU: everything CircuitIB, CircuitEnsemble, MeasurementIB and MeasurementEnsemble send to the C ABI - every entry point, in
order, with its arguments - against tests/golden/step_call_trace.json, the trace of the commit BEFORE the ensembles and the
single models came to share their host code.  That fixture was written on that commit by running `_record(case)` of this
module, as it stands here, for every case below and dumping the dict with json.dump(..., indent=0, sort_keys=True); the code
under test never regenerates it.

The models are built on host memory (device="cpu") behind three patches, undone after each test: _lib.load_library returns a
recorder around the real library (host queries - *_supported, *_bytes - are answered by the library, every other call is
recorded and not launched), torch.cuda.is_available says yes, and torch.cuda.current_stream gives stream 0.  A fourth makes
torch.empty return zeros: MeasurementEnsemble.fit retires a replica on the VALUE of a bound that no kernel computes here, and
zeros retire every replica at the first evaluation, which reaches the snapshot path.

What the trace holds, so that it depends on behaviour and not on attribute names:
  pointers     label+byte offset.  params, grads, adam_m, adam_v, t_dev, lr_dev of the model carry those names; every other
               tensor is buf<k> in order of first use in the call stream.  A tensor is found by walking the model (attributes,
               dicts, lists, launch records, the template model and stacks an ensemble holds) and the locals of the frames that
               lead to the call (the step's temporaries; they are kept alive, so that no address is used twice).  Of the tensors
               that hold an address the outermost RANGE names it - not the storage: params | grads | m | v of an ensemble are
               views of one allocation today and need not stay so.  A pointer nothing holds is "?", and fails the test.
  tables       the device descriptor table of a grouped GEMM is recorded as the sha1 of its bytes: the descriptors themselves
  arrays       ctypes arrays element by element, floats as floats
  structures   the bytes of a descriptor passed by reference, hex
Torch-side work between the calls (torch.mul(out=), zero_() of gradients or of slab 0, copy_) is not recorded: the GPU suite
checks it."""
import ctypes
import hashlib
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from _st_host_recorder import RecordingLib
from dib_amd import _lib, circuit, measurement
from dib_amd._gemm_plan import _Gemm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_call_trace.json")
NAMED = ("params", "grads", "adam_m", "adam_v", "t_dev", "lr_dev")


def _walk(roots, found, tables, seen):
    """every tensor reachable from `roots` into found (id -> tensor); the .dev of every launch record into tables (ids)"""
    stack = list(roots)
    while stack:
        o = stack.pop()
        if o is None or isinstance(o, (int, float, str, bytes, bool, np.ndarray, np.generic, types.ModuleType, type,
                                       ctypes.Array, ctypes.Structure, RecordingLib)) or id(o) in seen:
            continue
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            found[id(o)] = o
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif isinstance(o, types.FunctionType):
            stack.extend(c.cell_contents for c in (o.__closure__ or ()) if _filled(c))
        elif isinstance(o, types.MethodType):
            stack.append(o.__self__)
        elif type(o).__module__.startswith("dib_amd"):
            if isinstance(o, _Gemm) and o.dev is not None:
                tables.add(id(o.dev))
            stack.extend(vars(o).values())


def _filled(cell) -> bool:
    try:
        cell.cell_contents
        return True
    except ValueError:
        return False


class TraceLib(RecordingLib):
    """RecordingLib with the labels, tables and arrays of this module's docstring; `lines` holds one string per call"""

    def __init__(self, real):
        super().__init__(real)
        self.lines, self.model, self._named, self._bufs, self._tables = [], None, [], [], set()

    def watch(self, model) -> None:
        self.model = model
        self._named = [(k, getattr(model, k)) for k in NAMED]

    @staticmethod
    def _holds(t, p) -> bool:
        lo = t.data_ptr()
        return lo <= p < lo + max(1, t.numel() * t.element_size())

    def _label(self, t, name, p):
        if id(t) in self._tables:
            return f"table:{hashlib.sha1(t.numpy().tobytes()).hexdigest()}+{p - t.data_ptr()}"
        return f"{name}+{p - t.data_ptr()}"

    def name_pointer(self, p):
        if not p:
            return None
        for name, t in self._named + self._bufs:
            if self._holds(t, p):
                return self._label(t, name, p)
        found, seen = {}, set()
        _walk([self.model], found, self._tables, seen)
        f = sys._getframe(1)
        while f is not None:   # the package's frames and this module's (the caller's inputs), not the test runner's
            if f.f_globals is globals() or f.f_globals.get("__name__", "").startswith("dib_amd"):
                _walk(f.f_locals.values(), found, self._tables, seen)
            f = f.f_back
        holders = [t for t in found.values() if self._holds(t, p)]
        if not holders:
            return "?"
        t = min(holders, key=lambda t: (t.data_ptr(), -t.numel() * t.element_size()))
        self._bufs.append((f"buf{len(self._bufs)}", t))
        return self._label(t, self._bufs[-1][0], p)

    def _arg(self, a):
        if isinstance(a, ctypes.c_void_p):
            return self.name_pointer(a.value)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [self.name_pointer(v) for v in a]
            return [float(v) if a._type_ in (ctypes.c_float, ctypes.c_double) else int(v) for v in a]
        if isinstance(a, float):
            return repr(a)
        return super()._arg(a)

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if fn.__name__ != "record":
            return fn

        def record(*args):
            self.lines.append(f"{name}({', '.join(str(self._arg(a)) for a in args)})".replace("'", ""))
            return 0

        return record


@pytest.fixture
def host_lib(monkeypatch):
    """the patches of the module docstring; gives the recorder every model built in the test sends its calls to"""
    lib = TraceLib(_lib.load_library())
    monkeypatch.setattr(_lib, "load_library", lambda *a, **k: lib)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch, "empty", torch.zeros)
    return lib


# ---- the cases -----------------------------------------------------------------------------------------------------------------
TABLES = [circuit.truth_table(c) for c in circuit.SI_CIRCUITS]
ENSEMBLE_TABLES = {1: [TABLES[3]], 3: [TABLES[0], TABLES[3], TABLES[5]]}


def _rows(shape, rows, seed):
    return np.random.default_rng(seed).integers(0, rows, shape).astype(np.int32)


def _circuit_single(lib):
    m = circuit.CircuitIB(4, (32, 32), device="cpu")
    lib.watch(m)
    t = TABLES[3]
    for B in (17, 17, 160, 160):
        m.train_step(t, 0.25, B)
    m.train_step(t, 0.25, row_idx=_rows(24, 16, 1))
    m.estimate_channel_mi_bounds(21, 64, 2)
    m.fit(t, number_training_steps=6, batch_size=64, evaluate_mutual_info_freq=3, seed=5)


def _circuit_ensemble(lib, R):
    tables = ENSEMBLE_TABLES[R]
    e = circuit.CircuitEnsemble(tables, (32, 32), device="cpu")
    lib.watch(e)
    beta = [0.25, 0.5, 1.0][:R]
    for B in (17, 17, 160, 160):
        e.train_step(beta, B)
    e.train_step(beta, row_idx=np.stack([_rows(24, t.shape[0], 1 + r) for r, t in enumerate(tables)]))
    e.estimate_channel_mi_bounds([21 + r for r in range(R)], 64, 2)
    e.fit(number_training_steps=6, batch_size=64, beta_start=[1e-3, 2e-3, 4e-3][:R], beta_end=5.0, evaluate_mutual_info_freq=3,
          seeds=[5 + r for r in range(R)])
    r = min(1, R - 1)
    m = e.to_model(r)
    lib.lines.append(f"# to_model({r})")
    lib.watch(m)
    m.train_step(tables[r], 0.25, 17)


MEASUREMENT = dict(input_dimensionality=2, number_states=3, alphabet_size=3, info_bott_encoder_arch_spec=(32, 32),
                   vector_quant_arch_spec=(32, 32), measurement_aggregator_arch_spec=(32, 32),
                   reference_state_encoder_arch_spec=(32, 32))


def _traj(n=200, seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 2)).astype(np.float32)


def _measurement_single(lib):
    m = measurement.MeasurementIB(device="cpu", **MEASUREMENT)
    lib.watch(m)
    traj = torch.from_numpy(_traj())
    starts = _rows(96, 197, 2)
    m.match_batch_from_starts(traj, starts, True)
    m.match_batch_from_starts(traj, starts, False)
    m.symbolize(_traj(50, 4), noise_vector=np.random.default_rng(6).standard_normal((5, m.E)), chunk_size=32)
    m.fit(_traj(), number_training_steps=4, batch_size=96)


def _measurement_ensemble(lib, R, similarity):
    e = measurement.MeasurementEnsemble(R, device="cpu", infonce_similarity=similarity, **MEASUREMENT)
    lib.watch(e)
    traj = torch.from_numpy(_traj())
    starts = _rows((R, 96), 197, 2)
    e.match_batch_from_starts(traj, starts, True)
    e.match_batch_from_starts(traj, starts, False)
    e._info_bounds(_traj(64, 7), 16, 2, 9)
    r = min(1, R - 1)
    noise = np.random.default_rng(6).standard_normal((5, e.E))
    e.symbolize(r, _traj(50, 4), noise_vector=noise, chunk_size=32)
    h = e.fit(_traj(), number_training_steps=4, batch_size=96, info_eval_data=_traj(64, 7), evaluate_info_every=2,
              info_evaluation_batch_size=16, info_evaluation_number_batches=2, info_stopping_point=0.0)
    assert [k["steps"] for k in h] == [2] * R and sorted(e.snapshots) == list(range(R))   # every replica retired
    e.symbolize(r, _traj(50, 4), noise_vector=noise, chunk_size=32)                       # ... and is read from its snapshot
    m = e.to_model(r)
    lib.lines.append(f"# to_model({r})")
    lib.watch(m)
    m.match_batch_from_starts(traj, starts[r], True)


CASES = {"CircuitIB": _circuit_single,
         "CircuitEnsemble-R1": lambda lib: _circuit_ensemble(lib, 1),
         "CircuitEnsemble-R3": lambda lib: _circuit_ensemble(lib, 3),
         "MeasurementIB": _measurement_single,
         **{f"MeasurementEnsemble-R{R}-{s}": (lambda lib, R=R, s=s: _measurement_ensemble(lib, R, s))
            for R in (1, 3) for s in ("l2sq", "l1")}}


def _record(case, lib):
    CASES[case](lib)
    return list(lib.lines)


@pytest.mark.parametrize("case", list(CASES))
def test_calls_to_the_c_abi_match_the_recorded_trace(case, host_lib):
    got = _record(case, host_lib)
    assert not any("?" in line for line in got), [line for line in got if "?" in line][:3]
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (case, k, a, b)


def test_the_expected_launch_sequences(host_lib):
    m = circuit.CircuitIB(4, (32, 32), device="cpu")
    host_lib.watch(m)
    m.train_step(TABLES[3], 0.25, 17)
    assert [line.split("(")[0] for line in host_lib.lines] == ["dib_circuit_fwd", "dib_mlp_small_head_step", "dib_gemm_grouped",
                                                               "dib_circuit_bwd", "dib_reduce_adam_step"]
    del host_lib.lines[:]
    e = measurement.MeasurementEnsemble(3, device="cpu", **MEASUREMENT)
    host_lib.watch(e)
    e.match_batch_from_starts(torch.from_numpy(_traj()), _rows((3, 96), 197, 2), True)
    assert len(host_lib.lines) == 26


@pytest.mark.parametrize("family", ["circuit", "measurement"])
def test_to_model_takes_the_learning_rate_behind_the_host_cache(family, host_lib):
    """set_lr skips the device fill when the value equals its host cache; a model leaving an ensemble gets its learning rate by
    a device copy, so that cache must be void afterwards: the next set_lr of the default value has to reach the device"""
    ens = circuit.CircuitEnsemble(ENSEMBLE_TABLES[3], (32, 32), device="cpu") if family == "circuit" \
        else measurement.MeasurementEnsemble(2, device="cpu", **MEASUREMENT)
    default = float(ens.lr_dev)
    ens.set_lr(5e-4)
    m = ens.to_model(0)
    assert float(m.lr_dev) == float(np.float32(5e-4))
    m.set_lr(default)
    assert float(m.lr_dev) == default
    m.set_lr(1e-3)
    assert float(m.lr_dev) == float(np.float32(1e-3))
