"""The LDS admission gates of the row-tile kernels, asked of the real libdib_hip.so without a GPU (host queries only, nothing
launched): dib_mlp_small_supported, dib_mlp_small_head_supported, dib_st_chain_supported and dib_layout_create's admission of the
integration network.  Each sweeps the last hidden width in steps of 16 across the limit and must flip exactly where the Python
restatement of the kernel's LDS size - the envelope tests' own (_mlp_lds, _int_lds, st_chain_*_lds), imported, not rewritten -
crosses 150 KB.  The kernels carve their LDS from one map per kernel (csrc/dib_small.h, csrc/dib_st_chain.h) and the host sizes
and admits launches from the same map: this pins where the gates lay before that map existed."""
import ctypes
import os
import shutil

import pytest

from dib_amd import _lib
from dib_amd._st_plan import _BlockDesc
from dib_amd.dense import _mlp_desc

from test_gpu_small_envelope import _int_lds, _mlp_lds
from test_gpu_st_envelope import LDS_GATE, st_chain_bwd_lds, st_chain_fwd_lds, st_chain_supported

# the skip rule of test_st_plan_host.py
if not os.path.exists(_lib.LIB_PATH) and not any(c and os.path.exists(c) for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc")):
    pytest.skip("no prebuilt libdib_hip.so and no hipcc to build it", allow_module_level=True)
try:
    LIB = _lib.load_library()
except OSError as e:   # dlopen: no HIP runtime on this machine
    pytest.skip(f"libdib_hip.so cannot be loaded here: {e}", allow_module_level=True)

WIDTHS = range(16, 1024 + 1, 16)
RELU, TANH = _lib.ACTIVATIONS["relu"], _lib.ACTIVATIONS["tanh"]


def _flips_with(answers, sizes):
    """answers / sizes by swept width: admitted exactly while the restated size is within the gate, and the sweep crosses it"""
    for w in WIDTHS:
        assert answers[w] == (sizes[w] <= LDS_GATE), (w, answers[w], sizes[w])
    assert {sizes[w] <= LDS_GATE for w in WIDTHS} == {True, False}, "the sweep does not cross the gate"


def _desc(in_dim, widths, n_freq=1):
    return _mlp_desc([0] * len(widths), [0] * len(widths), widths, in_dim, n_freq, RELU)


# (input columns, frequencies, hidden widths in front of the swept one, output width)
@pytest.mark.parametrize("in_dim,n_freq,front,out", [(64, 1, [], 16), (6, 5, [384], 64), (128, 1, [256, 256], 16), (512, 1, [], 512)])
def test_mlp_small_supported_flips_at_the_gate(in_dim, n_freq, front, out):
    got = {w: LIB.dib_mlp_small_supported(ctypes.byref(_desc(in_dim, front + [w, out], n_freq)), 128) == 1 for w in WIDTHS}
    _flips_with(got, {w: _mlp_lds(in_dim * n_freq, front + [w], out) for w in WIDTHS})


# the 1-unit head adds its scratch, 9 (KL + 1) + 32 floats: _int_lds with out = 1 is the whole launch
@pytest.mark.parametrize("in_dim,front", [(64, []), (32, [384]), (128, [256, 256]), (1024, [])])
def test_mlp_small_head_supported_flips_at_the_gate(in_dim, front):
    got = {w: LIB.dib_mlp_small_head_supported(ctypes.byref(_desc(in_dim, front + [w, 1])), 128) == 1 for w in WIDTHS}
    _flips_with(got, {w: _int_lds(in_dim, front + [w], 1) for w in WIDTHS})


# feed-forward [.., w, D]: the backward's size crosses first with a narrow context, the forward's with a wide one
@pytest.mark.parametrize("D,HK,front", [(32, 128, []), (64, 16, []), (128, 128, []), (32, 1536, [256]), (128, 1536, [])])
def test_st_chain_supported_flips_at_the_gate(D, HK, front):
    def ask(w):
        d = _BlockDesc()
        ff = front + [w, D]
        d.n_ff, d.D, d.HK, d.eps, d.act = len(ff), D, HK, 1e-3, RELU
        for i, u in enumerate(ff):
            d.ff_width[i] = u
        return LIB.dib_st_chain_supported(ctypes.byref(d), 200) == 1
    got = {w: ask(w) for w in WIDTHS}
    size = {w: max(st_chain_fwd_lds(D, HK, front + [w, D]), st_chain_bwd_lds(D, HK, front + [w, D])) for w in WIDTHS}
    _flips_with(got, size)
    assert all(got[w] == st_chain_supported(D, HK, front + [w, D], RELU, 200) for w in WIDTHS)


def _workspace_bytes(dims, enc, E, units, out, act, batch=128):
    ci = lambda xs: (ctypes.c_int * max(1, len(xs)))(*xs)   # noqa: E731
    h = ctypes.c_void_p()
    _lib.check(LIB.dib_layout_create(len(dims), ci(dims), len(enc), ci(enc), E, len(units), ci(units), out, 0, 1, act, 0,
                                     ctypes.byref(h)), "dib_layout_create")
    try:
        return int(LIB.dib_workspace_bytes(h, batch))
    finally:
        LIB.dib_layout_destroy(h)


# A layout admitted to the row-tile integration kernel carries the cluster mode's counters and exchange buffers in its workspace
# (dib_workspace_bytes, a host query); one whose activation is not piecewise-linear never does.  With a 16-column feature the
# row-tile ENCODERS admit neither (inputs <= 15), so the two workspaces differ exactly when the integration network was admitted.
@pytest.mark.parametrize("F,E,front,out", [(1, 64, [], 16), (2, 64, [384], 1), (4, 32, [256, 256], 64), (2, 512, [], 16)])
def test_layout_admits_the_integration_network_up_to_the_gate(F, E, front, out):
    got = {w: _workspace_bytes([16] * F, [48, 48], E, front + [w], out, RELU) != _workspace_bytes([16] * F, [48, 48], E, front + [w], out, TANH)
           for w in WIDTHS}
    _flips_with(got, {w: _int_lds(F * E, front + [w], out) for w in WIDTHS})
