"""TEST-ONLY host recorder for dib_amd.SetTransformerDIB: a subclass that keeps its buffers in host memory and a proxy of the
library that forwards the HOST queries (`*_supported`, `*_bytes`, tuning) to the real libdib_hip.so and RECORDS every other
C-ABI call - name and arguments, device pointers rewritten as (buffer name, byte offset) - instead of launching it.  With it
the plan of a (batch, particles) shape and the call sequence of a step can be inspected, and compared between two versions of
the host code, on a machine without a GPU.  Lives in tests/; the product package never imports it and has no hook for it.
The recorder must never be pointed at a real GPU stream: nothing it records is launched."""
import ctypes
from ctypes import c_void_p

import numpy as np
import torch

import dib_amd
from dib_amd import _lib

HOST_CALLS = ("dib_version", "dib_abi_version", "dib_error_string", "dib_set_tuning", "dib_get_tuning", "dib_launch_count")


def _is_host_query(name: str) -> bool:
    return name in HOST_CALLS or name.endswith("_supported") or name.endswith("_bytes")


class RecordingLib:
    """forwards host queries to `real`, records every other entry point in `calls` as (name, [arguments]) and returns DIB_OK"""

    def __init__(self, real):
        self._real, self.calls, self._regions = real, [], []

    def register(self, name: str, t) -> None:
        if t is not None and not any(t is r[1] for r in self._regions):
            self._regions.append((name, t, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))

    def name_pointer(self, p):
        if not p:
            return None
        for name, _t, lo, hi in self._regions:
            if lo <= p < hi or (p == lo == hi):
                return [name, p - lo]
        return ["?", int(p)]

    def _arg(self, a):
        if a is None or isinstance(a, (int, float, str)):
            return a
        if isinstance(a, np.integer):
            return int(a)
        if isinstance(a, c_void_p):
            return self.name_pointer(a.value)
        if isinstance(a, ctypes.Array):
            if a._type_ is c_void_p:
                return [self.name_pointer(v) for v in a]
            return [int(v) for v in a]
        if hasattr(a, "_obj"):   # ctypes.byref(structure)
            return bytes(a._obj).hex()
        raise TypeError(f"unrecorded argument type {type(a)}")

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        fn = getattr(self._real, name)   # AttributeError for an entry point the library does not export
        if _is_host_query(name):
            return fn

        def record(*args):
            self.calls.append((name, [self._arg(a) for a in args]))
            return 0

        return record


def real_library():
    return _lib.load_library()


def make_model(switches=None, **kw):
    """A SetTransformerDIB on host memory whose library is a RecordingLib.  `switches`: attributes set after construction
    and before the first plan (the A/B switches, skinny_k_min_tokens)."""
    proxy = RecordingLib(real_library())

    class HostRecordedSetTransformerDIB(dib_amd.SetTransformerDIB):
        def _acquire_device(self, device):
            self.lib, self.device = proxy, torch.device("cpu")

        def _stream(self):
            return c_void_p(0)

    kw.setdefault("attention_score_stash_bytes", 0)   # (the stash policy asks the device for its free memory)
    kw.setdefault("use_graphs", False)
    m = HostRecordedSetTransformerDIB(**kw)
    for k, v in (switches or {}).items():
        setattr(m, k, v)
    for name in ("params", "grads", "adam_m", "adam_v", "beta_dev", "lr_dev", "t_dev", "step_dev"):
        proxy.register(name, getattr(m, name))
    return m


def tables(pl):
    """(name, launch record) of every table of a plan; a split-K record counts with the grouped launch inside it"""
    return [(k, getattr(t, "gemm", t)) for k, t in pl["g"].items()] if isinstance(pl["g"], dict) else \
        [(f"enc{l}_fwd", t) for l, t in enumerate(pl["g"])]


def register_plan(m, pl) -> None:
    reg = m.lib.register
    reg("ws", pl["ws"])
    reg("slabs", pl.get("slabs"))
    if pl.get("head_mlp") is not None:
        reg("head_ws", pl["head_mlp"]["ws"])
    for k, t in tables(pl):
        reg(f"table:{k}", t.dev)


def _labels(m, B):
    y = (torch.arange(B, dtype=torch.float32) % 2).reshape(B, 1).repeat(1, m.output_dimensionality).contiguous()
    m.lib.register("labels", y)
    return y


def _inputs(m, B, P):
    g = torch.Generator().manual_seed(B * 1000 + P)
    return torch.randn(B, P, m.particle_feature_dimensions, generator=g)


def record_train_step(m, B, P):
    """the calls of forward(_skip_head=True) -> loss_and_backward(reduce=False) -> adam_step(fused_reduce=True)"""
    pl = m._plan(B, P)
    register_plan(m, pl)
    y = _labels(m, B)
    m.lib.calls.clear()
    m.forward(_inputs(m, B, P), _skip_head=True)
    m.loss_and_backward(y, reduce=False)
    if m._sync is None:   # (allocated by the first optimizer step: name it before the call is recorded)
        m._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32)
    m.lib.register("sync", m._sync)
    m.adam_step(fused_reduce=True)
    return list(m.lib.calls)


def record_eval_step(m, B, P):
    """the calls of forward(for_backward=False) -> _loss_only"""
    pl = m._plan(B, P)
    register_plan(m, pl)
    y = _labels(m, B)
    m.lib.calls.clear()
    m.forward(_inputs(m, B, P), for_backward=False)
    m._loss_only(y)
    return list(m.lib.calls)


def record_encoder(m, T):
    """the encoder-only plan behind particle_encoder and its calls"""
    x = torch.zeros(T, m.particle_feature_dimensions)
    m.particle_encoder(x)   # builds the plan
    pl = m._plans[("enc", T)]
    m.lib.register(f"enc_ws{T}", pl["ws"])
    for k, t in tables(pl):
        m.lib.register(f"enc{T}_table:{k}", t.dev)
    m.lib.calls.clear()
    m.particle_encoder(x)
    return dict(off=dict(pl["off"]), ws_size=pl["ws"].numel(),
                g=[dict(descs=t.host.tobytes().hex(), mode=t.mode, act=t.act) for _k, t in tables(pl)], calls=list(m.lib.calls))


def call_counts(calls) -> dict:
    out = {}
    for name, _a in calls:
        out[name] = out.get(name, 0) + 1
    return out
