"""The encoder layer-2 weight gradient that recomputes h1 in registers (csrc/dib_wgrad_recompute.h) against the one that streams the
stashed h1 (csrc/dib_wgrad_stream.h): the same seeded training step on two fresh engines, once with
dib_set_tuning("wgrad_recompute_h1", 0) and once with 1, the stream path opened to small batches ("small_batch" 0,
"wgrad_stream_rows" 64, "wgrad_stream_fill" 0).  The contract is BIT equality of the flat gradients, of the parameters after Adam
and of the step's scalars; the h1 region of the workspace, filled with NaN before the step, says whether the forward wrote it
(arm 0: every word) or nobody touched it (arm 1: still all NaN - had the weight gradient read it, its gradients would be NaN);
entry 19 of the library's live profile counts the new kernel's launches.  Arm 1 is also held to the float64 oracle."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dib_oracle as orc  # noqa: E402
from _helpers import flat_to_params, params_to_flat, spec_kwargs  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("small_batch", "wgrad_stream", "wgrad_stream_rows", "wgrad_stream_fill", "wgrad_max_splits", "wgrad_recompute_h1",
        "stream_rows")
BETA, SEED, STEP = 0.05, 5, 3


def _spec(dims, act):
    return orc.DIBSpec(list(dims), [128, 128], [256, 256], 1, activation_fn=act, feature_embedding_dimension=32)


def _h1_launches(lib):
    ms = (ctypes.c_double * 20)()
    cnt = (ctypes.c_int * 20)()
    assert lib.dib_profile_summary_n(ms, cnt, 20) == 0
    assert cnt[19] <= cnt[17]     # entry 19 re-counts the part of category 17 that ran dib_wgrad_h1_kernel
    return cnt[19]


def _data(spec, B):
    rng = np.random.default_rng(B + 7 * len(spec.feature_dimensionalities))
    x = rng.standard_normal((B, sum(spec.feature_dimensionalities))).astype(np.float32)
    y = (x[:, :1] * x[:, 1:2] > 0).astype(np.float32)
    return x, y


def _run(spec, B, arm, max_splits, mode="train_step", flip=None, stream=1, nontemporal=False):
    """One seeded step on a fresh engine -> dict of int32 views (+ bookkeeping).  mode: "train_step" (the engine's own step),
    "single" / "staged" (the step's entry points one by one, the encoder-bank backward in one call or as stage 1 then stage 2);
    flip: the value "wgrad_recompute_h1" takes between forward and backward; nontemporal: the kernels' non-temporal operand loads
    ("stream_rows" 64; default: from 8192 streamed rows up)."""
    from dib_amd import _lib as L
    from dib_amd.engine import HipEngine, _ptr
    old = {k: L.get_tuning(k) for k in KEYS}
    lib = L.load_library()
    try:
        L.set_tuning("small_batch", 0)
        L.set_tuning("wgrad_stream", stream)
        L.set_tuning("wgrad_stream_rows", 64)
        L.set_tuning("wgrad_stream_fill", 0)
        L.set_tuning("wgrad_max_splits", max_splits)     # read when the workspace is sized
        L.set_tuning("wgrad_recompute_h1", arm)
        if nontemporal:
            L.set_tuning("stream_rows", 64)
        eng = HipEngine(**spec_kwargs(spec), init_seed=4)
        flat = eng.get_flat_params()
        rng = np.random.default_rng(11)
        for b in eng.blocks:     # non-zero biases: b1 is the recompute's C operand
            if b["what"] == 1:
                flat[b["offset"]: b["offset"] + b["cols"]] = 0.05 * rng.standard_normal(b["cols"])
        eng.set_flat_params(flat)
        params0 = eng.get_flat_params().copy()
        eng.set_beta(BETA)
        eng.set_lr(3e-4)
        x, y = _data(spec, B)
        xd, yd = eng.to_device(x), eng.to_device(y)
        h1 = eng.ws_view(B, L.WS_ENC_H0, B * eng.F * 128)     # the raw region (eng.enc_h would fill it on demand)
        h1.fill_(float("nan"))
        lib.dib_profile_enable(1)
        if mode == "train_step":
            eng.train_step(xd, yd, None, 0, B, SEED, STEP, "bce_logits")
        else:
            inv, ws, st = 1.0 / B, eng.workspace(B), eng._stream()
            eng.forward(xd, None, 0, B, SEED, STEP, defer_sums=True)
            eng.loss("bce_logits", yd, None, 0, B, inv, defer_sums=True)
            if flip is not None:
                L.set_tuning("wgrad_recompute_h1", flip)
            L.check(lib.dib_integration_bwd(eng.layout, B, _ptr(eng.params), _ptr(eng.grads), _ptr(ws), st), "dib_integration_bwd")
            for stage in ((1, 2) if mode == "staged" else (None,)):
                if stage is None:
                    L.check(lib.dib_encoder_bank_bwd(eng.layout, B, _ptr(eng.params), _ptr(eng.grads), _ptr(eng.beta_dev), inv,
                                                     _ptr(ws), st), "dib_encoder_bank_bwd")
                else:
                    L.check(lib.dib_encoder_bank_bwd_stage(eng.layout, B, _ptr(eng.params), _ptr(eng.grads), _ptr(eng.beta_dev), inv,
                                                           stage, _ptr(ws), st), "dib_encoder_bank_bwd_stage")
            eng.step_tail(B, -1, L.TAIL_FINALIZE | L.TAIL_KL | L.TAIL_LOSS, inv)
        torch.cuda.synchronize()
        launches = _h1_launches(lib)
        lib.dib_profile_enable(0)
        out = dict(grads=eng.grads.view(torch.int32).cpu().numpy().copy(), gflat=eng.get_flat_grads().astype(np.float64),
                   step_out=eng.step_out(B).view(torch.int32).cpu().numpy().copy(),
                   h1_nan=torch.isnan(h1).sum().item(), h1_words=h1.numel(), launches=launches,
                   slabs=int(lib.dib_layout_wgrad_splits(eng.layout, B)), params0=params0, blocks=eng.blocks,
                   n_alloc=eng.params.numel(), x=x, y=y)
        eng.adam_step()
        torch.cuda.synchronize()
        out["params"] = eng.params.view(torch.int32).cpu().numpy().copy()
        return out
    finally:
        lib.dib_profile_enable(0)
        for k, v in old.items():
            L.set_tuning(k, v)


def _same_bits(a, b):
    for k in ("grads", "params", "step_out"):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["gflat"]).all()


def _check_oracle(spec, r, B):
    """every gradient block within the parity tests' bound (tests/test_gpu_parity.py: 3e-4 of the block's largest entry)"""
    p = flat_to_params(r["blocks"], r["params0"], spec)
    F, E = spec.number_features, spec.feature_embedding_dimension
    c = orc.forward(spec, p, r["x"].astype(np.float64), orc.philox_normal_all(SEED, STEP, np.arange(B), F, E))
    _, grads, _ = orc.backward(spec, p, r["x"].astype(np.float64), r["y"], c, BETA, "bce_logits")
    gref = params_to_flat(r["blocks"], grads, r["n_alloc"]).astype(np.float64)
    worst = 0.0
    for b in r["blocks"]:
        sl = slice(b["offset"], b["offset"] + b["rows"] * b["cols"])
        err = np.abs(r["gflat"][sl] - gref[sl]).max()
        worst = max(worst, err / (np.abs(gref[sl]).max() + 1e-3))
        print("block", b["net"], b["layer"], b["feature"], b["what"], "err", err, "scale", np.abs(gref[sl]).max())
        assert err <= 3e-4 * (np.abs(gref[sl]).max() + 1e-3), (b, err)
    return worst


# (batch, most slabs) -> slabs x rows of the layer-2 weight gradient: 1 x 64 (fewer blocks than the ring holds), 1 x 192 (one and a
# half trips of 32-row tiles per 64-row K-tile pair ...), 3 x 192, 1 x 576, 3 x 576 (several trips around the ring)
SHAPES = [(64, 1, 1), (192, 1, 1), (576, 3, 3), (576, 1, 1), (1728, 3, 3)]


@pytest.mark.parametrize("B,max_splits,slabs", SHAPES)
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("act", ["relu", "leaky_relu", None])
def test_recompute_arm_has_the_stash_arms_bits(act, F, B, max_splits, slabs):
    spec = _spec([1] * F, act)
    nt = slabs == 3     # (as tests/test_gpu_wgrad_stream.py: the non-temporal instantiations on the 3-slab cases)
    stash, rec = _run(spec, B, 0, max_splits, nontemporal=nt), _run(spec, B, 1, max_splits, nontemporal=nt)
    assert stash["slabs"] == slabs and rec["slabs"] == slabs
    assert stash["launches"] == 0 and rec["launches"] == 1, (stash["launches"], rec["launches"])
    assert stash["h1_nan"] == 0                      # arm 0: the forward wrote every word of the region
    assert rec["h1_nan"] == rec["h1_words"]          # arm 1: nobody wrote it - and nobody read it: the gradients are finite
    _same_bits(stash, rec)
    if F == 2 and B in (64, 1728):
        _check_oracle(spec, rec, B)


@pytest.mark.parametrize("nontemporal", [False, True])
@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_two_bias_chains_of_the_large_launches(act, nontemporal):
    """The cases above are so small that the tile rule gives the launch the 64-column tiles' four bias chains.  8 features x 8
    slabs of 128 rows = 128 tiles of 64 x 128: the 128-column tiles' two chains, the form of every large launch (the headline's)."""
    spec = _spec([1] * 8, act)
    stash, rec = _run(spec, 1024, 0, 32, nontemporal=nontemporal), _run(spec, 1024, 1, 32, nontemporal=nontemporal)
    assert stash["slabs"] == 8 and rec["slabs"] == 8
    assert stash["launches"] == 0 and rec["launches"] == 1
    assert stash["h1_nan"] == 0 and rec["h1_nan"] == rec["h1_words"]
    _same_bits(stash, rec)
    if act == "relu" and not nontemporal:
        _check_oracle(spec, rec, 1024)


@pytest.mark.parametrize("what", ["in_dim_10", "ragged_slab", "stream_off"])
def test_gates_keep_the_stash_path(what):
    """a 2-dimensional feature (encoder input 10 wide), a batch that is no whole number of 64-row K-tiles, the LDS-free kernel
    switched off: both arms stash h1 and stream it"""
    spec = _spec([2, 1] if what == "in_dim_10" else [1, 1], "relu")
    B = 160 if what == "ragged_slab" else 192
    a = _run(spec, B, 0, 1, stream=0 if what == "stream_off" else 1)
    b = _run(spec, B, 1, 1, stream=0 if what == "stream_off" else 1)
    assert a["launches"] == 0 and b["launches"] == 0
    assert a["h1_nan"] == 0 and b["h1_nan"] == 0
    _same_bits(a, b)


def test_staged_backward_equals_the_single_call():
    spec = _spec([1, 1], "relu")
    single, staged = _run(spec, 576, 1, 3, mode="single"), _run(spec, 576, 1, 3, mode="staged")
    stash = _run(spec, 576, 0, 3, mode="staged")
    assert single["launches"] == 1 and staged["launches"] == 1 and stash["launches"] == 0
    assert staged["h1_nan"] == staged["h1_words"]
    _same_bits(single, staged)
    _same_bits(stash, staged)


@pytest.mark.parametrize("fwd,bwd", [(1, 0), (0, 1)])
def test_the_backward_follows_the_forwards_record(fwd, bwd):
    """the key flipped between forward and backward: the weight gradient does what the forward prepared"""
    spec = _spec([1, 1], "leaky_relu")
    stash = _run(spec, 576, 0, 3, mode="single")
    flipped = _run(spec, 576, fwd, 3, mode="single", flip=bwd)
    assert flipped["launches"] == fwd
    assert flipped["h1_nan"] == (flipped["h1_words"] if fwd else 0)
    _same_bits(stash, flipped)


def test_enc_h_view_is_filled_on_demand():
    """HipEngine.enc_h(batch, 0) after a forward that did not stash the layer: recomputed into the region, not stale memory"""
    from dib_amd import _lib as L
    from dib_amd.engine import HipEngine
    spec = _spec([1, 1], "relu")
    old = {k: L.get_tuning(k) for k in KEYS}
    try:
        L.set_tuning("small_batch", 0)
        L.set_tuning("wgrad_stream_rows", 64)
        L.set_tuning("wgrad_stream_fill", 0)
        views = []
        for arm in (0, 1):
            L.set_tuning("wgrad_recompute_h1", arm)
            eng = HipEngine(**spec_kwargs(spec), init_seed=4)
            x, y = _data(spec, 192)
            eng.ws_view(192, L.WS_ENC_H0, 192 * 2 * 128).fill_(float("nan"))
            eng.train_step(eng.to_device(x), eng.to_device(y), None, 0, 192, SEED, STEP, "bce_logits")
            assert int(eng.lib.dib_workspace_h1_stashed(eng.layout, ctypes.c_void_p(eng.workspace(192).data_ptr()))) == 1 - arm
            views.append(eng.enc_h(192, 0).cpu().numpy().astype(np.float64))
        assert np.isfinite(views[1]).all()
        # the fused forward's values and the grouped GEMM's: two float32 evaluations of b1 + a 5-term sum, each within gamma_6
        # (u = 2^-24) of the exact value relative to the sum of the terms' magnitudes, which |b1| + 5 max|P| max|W1| bounds
        # (an encoder input is x or a sine / cosine of it: max|P| <= max(|x|, 1))
        wmax = float(np.abs(eng.get_flat_params()).max())
        smax = wmax + 5.0 * max(float(np.abs(x).max()), 1.0) * wmax
        assert np.abs(views[0] - views[1]).max() <= 2 * 6 * 2.0 ** -24 / (1 - 6 * 2.0 ** -24) * smax
    finally:
        for k, v in old.items():
            L.set_tuning(k, v)
