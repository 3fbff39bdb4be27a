"""CPU: the engine-call trace of DistributedIBNet.fit / evaluate - every engine method called, in order, with its arguments -
against tests/golden/fit_protocol_trace.json, the trace of the commit before fit's step protocols, evaluation pass and input
handling moved to dib_amd/_fit.py.  That fixture was written by running `_trace(case, engine)` of this module, as it stands
here, for every (case, engine) below on that commit and dumping the dict with json.dump(..., indent=0, sort_keys=True).

Two engines: the checker engine as it is (no set_optimizer, apply_lr, step_dev or capture_step_graph: fit's probes all miss)
and, for the branches behind those probes, a subclass of it with recording no-op set_optimizer / apply_lr / set_step_counter
and a device step counter.  Graph capture stays a GPU matter (tests/test_gpu_parity.py)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import dib_oracle as orc
from _helpers import spec_kwargs
from _oracle_engine import OracleEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_protocol_trace.json")


class ProbedEngine(OracleEngine):
    """the checker engine with what fit probes for: an optimizer binding, a device-side learning rate and a device step counter
    (all no-ops here: the arithmetic stays the checker's), and a stand-in for the information evaluation of a tracked fit"""
    step_dev = torch.zeros(1, dtype=torch.int32)

    def set_optimizer(self, optimizer): pass
    def apply_lr(self, optimizer): pass
    def set_step_counter(self, value): pass


def _feature_information(self, x, rows, batch, n_batches, seed, step):
    return np.zeros((self.F, n_batches, 2))


class RecordingProxy:
    """Stands in front of an engine: attribute reads pass through (so do fit's hasattr / getattr probes), every method call is
    logged as one line, `name(parameter=value, ...)`, with the arguments bound to the method's signature and those that equal
    their default left out - the call as the engine receives it, however the caller spelled it.  A tensor is logged as
    buffer+offset[shape]: the buffer it lives in and its element offset into it, which gives a row-index or gradient slice by its
    bounds.  The buffers are named in the order the engine handed them out (to_device: dev0, dev1, ... - kept alive here, so
    that no address is ever used twice) or by the engine attribute that owns them."""

    def __init__(self, engine):
        self._eng, self.log = engine, []
        self._buffers = [(name, getattr(engine, name)) for name in ("params", "grads", "metrics_acc", "metrics_acc_val")]

    def _value(self, v):
        if isinstance(v, torch.Tensor):
            base = v.untyped_storage().data_ptr()
            label = next((n for n, t in self._buffers if t.untyped_storage().data_ptr() == base), "?")
            return f"{label}+{v.storage_offset()}{list(v.shape)}"
        if isinstance(v, np.ndarray):
            weighted = float(v.reshape(-1).astype(np.float64) @ np.arange(1, v.size + 1))   # tells one permutation from another
            return f"ndarray{list(v.shape)}:{v.dtype}:{weighted!r}"
        if inspect.isfunction(v) or inspect.ismethod(v):
            return "<callable>"
        if v is None or isinstance(v, (bool, int, float, str, torch.dtype)):
            return repr(v)
        return f"<{type(v).__name__} {getattr(v, 'name', getattr(v, 'kind', ''))}>"

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not inspect.ismethod(attr):
            return attr
        parameters = inspect.signature(attr).parameters

        def call(*args, **kwargs):
            given = inspect.signature(attr).bind(*args, **kwargs).arguments
            shown = [f"{k}={self._value(v)}" for k, v in given.items() if v is not parameters[k].default]
            self.log.append(f"{name}({', '.join(shown)})")
            out = attr(*args, **kwargs)
            if name == "to_device":
                self._buffers.append((f"dev{sum(n.startswith('dev') for n, _ in self._buffers)}", out))
            return out
        return call


def _model(engine_cls, optimizer):
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [8], [8], 1, feature_embedding_dimension=4)
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=1, shuffle_seed=2, init_seed=3)
    model._make_engine = lambda: RecordingProxy(engine_cls(**model._spec_kwargs(), init_seed=model.init_seed))
    model.compile(optimizer=optimizer, loss=dib_amd.losses.BinaryCrossentropy(from_logits=True), metrics=["accuracy"])
    return model


def _optimizer(decay):
    import dib_amd
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = 5e-3
    if decay:
        opt.decay = 0.25
    return opt


CASES = ("fit_validation_one_by_one", "fit_validation_merged", "fit_tracked_every_2", "fit_two_syncs_per_epoch", "evaluate")
ENGINES = {"checker": (OracleEngine, False), "probed": (ProbedEngine, False), "probed_decay": (ProbedEngine, True)}


def _trace(case, engine):
    """5 rows at batch 2 (two full batches and a 1-row tail), 2 epochs, 3 validation rows: the engine calls of one case"""
    engine_cls, decay = ENGINES[engine]
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)
    x, y = x[:5].astype(np.float32), y[:5].astype(np.float32)
    model = _model(engine_cls, _optimizer(decay))
    if case == "evaluate":
        model.evaluate(x, y, batch_size=2)
        return model._engine.log
    kw = {}
    if case == "fit_validation_one_by_one":
        model.validation_merge_rows = 0
    elif case == "fit_tracked_every_2":
        inner = model._ensure_engine()._eng
        inner.feature_information = _feature_information.__get__(inner)
        kw["track_information"] = {"every": 2}
    elif case == "fit_two_syncs_per_epoch":
        model.syncs_per_epoch = 2
    model.fit(x, y, epochs=2, batch_size=2, verbose=False, validation_data=(x[:3].copy(), y[:3].copy()), **kw)
    return model._engine.log


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("case", CASES)
def test_engine_call_trace_is_the_recorded_one(golden, case, engine):
    got, want = _trace(case, engine), golden[f"{case}/{engine}"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    assert len(got) == len(want)


def _names(log):
    return [line.split("(")[0] for line in log]


def test_decayed_learning_rate_is_applied_once_per_step_ahead_of_it():
    names = _names(_trace("fit_validation_merged", "probed_decay"))
    steps = [i for i, n in enumerate(names) if n == "train_step"]
    assert len(steps) == 2 * 3 and names.count("apply_lr") == len(steps) and "set_lr" not in names
    assert all(names[i - 1] == "apply_lr" for i in steps)


def test_step_counter_follows_every_eager_step_and_brackets_the_validation_pass():
    """the device step counter of an engine that has one: the fit's first step at the start, the next step after every eager
    step, the validation key (1 << 31) + epoch ahead of the validation pass and the training step again behind it"""
    log = _trace("fit_validation_merged", "probed")
    names = _names(log)
    assert [line for line in log if line.startswith("set_step_counter")] == [
        f"set_step_counter(value={v})" for v in (0, 1, 2, 3, (1 << 31) + 0, 3, 4, 5, 6, (1 << 31) + 1, 6)]
    assert all(names[i + 1] == "set_step_counter" for i, n in enumerate(names) if n == "train_step")
    first_eval = names.index("eval_step")   # 3 validation rows at batch 2: two launch sets
    assert names[first_eval - 1] == "set_step_counter" and names[first_eval + 2] == "set_step_counter"
