"""dL/dx of DistributedIBNet on the GPU (dib_encoder_bank_input_grad, csrc/dib_input_grad.h) against the float64 oracle
(tests/_oracle_input_grad.py), through every dispatch path, and the autograd bridge / DistributedIBModule built on it.

Tolerance: max|dx - dx64| <= TOL * max|dx64| per feature block.  The same oracle code in float32 arithmetic on the CPU, over the
oracle cases below, is at most RATIO32 = 5.2e-7 of the block's largest entry away from float64 (measured 5.10e-7, tabular8_default
at B = 40; tests/test_input_grad_oracle.py re-measures it); dx is one contraction deeper than dW1 plus a multiply, so TOL = 8 x
that = 4.16e-6 (the GPU's largest figure over all cases and paths: 6.4e-7).  The bound tests/test_gpu_parity.py applies to the first encoder layer's weight gradient, 3e-4, is 72 x looser and
never reached.

Rows: a row may be left out only where the float64 oracle has a hidden pre-activation with |z| < 1e-5 (a relu / leaky_relu mask on
a knife edge), at most 0.1 % of a case's rows - none at B = 40, two at B = 2100.  With this zoo a row has 200 - 1300 hidden units,
so 1 - 3 % of the rows lie within 1e-5 of an edge; what float32 rounding can flip is |z| < ~1e-7.  The parameter seeds are the ones
for which the oracle has no more rows within 1e-6 (ten times that) than the case may exclude: zlib.crc32(name) % 1000 as in
tests/test_gpu_parity.py for every B = 40 case, the first seed after it that qualifies for the two B = 2100 cases
(tests/test_input_grad_oracle.py checks the criterion on the CPU).  The two grid-stride cases (STRIDE) have smooth activations."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as orc
import _oracle_input_grad as og
from _helpers import SPECS, dispatch_path, flat_to_params, params_to_flat, spec_kwargs

pytestmark = pytest.mark.gpu

RATIO32 = 5.2e-7
TOL = 8 * RATIO32
PARITY_BOUND = 3e-4
MAX_EXCLUDED_SHARE = 1e-3
PATHS = ("default", "large_batch", "grouped_gemm")
LARGE = {"boolean4_32x32": 555, "fused_128_leaky": 602}    # parameter seeds of the B = 2100 cases (see above)
# the smallest shape tests/test_gpu_wgrad_recompute.py arms the h1 recompute with: 2 features, B = 64, one slab
RECOMPUTE = ("recompute_h1", 64, 13)
RECOMPUTE_KEYS = {"small_batch": 0, "wgrad_stream": 1, "wgrad_stream_rows": 64, "wgrad_stream_fill": 0, "wgrad_max_splits": 1}
_EXTRA = {"recompute_h1": orc.DIBSpec([1, 1], [128, 128], [256, 256], 1, activation_fn="relu", feature_embedding_dimension=32)}
# the kernel's own envelope beyond the zoo (whose positional encodings have 1, 3, 4 and 5 blocks, inputs at most 10 columns per
# feature and first layers that fit one LDS packing): every instantiation (2, 6, 7, 8 blocks), two groups of blocks (11), two
# chunks of 16 x columns (a 19-wide feature), a first layer walked in two LDS chunks (13 k tiles: 9 fit with 7 blocks, 8 with 8)
# with rows of G that are 16-byte aligned (200) and not (203)
ENVELOPE = {
    "blocks2_wide19": orc.DIBSpec([19, 2], [24], [12], 1, activation_fn="tanh", feature_embedding_dimension=4,
                                  number_positional_encoding_frequencies=2),
    "blocks6": orc.DIBSpec([2, 1], [20], [8], 1, feature_embedding_dimension=4, number_positional_encoding_frequencies=6),
    "blocks7_h203": orc.DIBSpec([1, 3], [203], [8], 1, activation_fn="elu", feature_embedding_dimension=4,
                                number_positional_encoding_frequencies=7),
    "blocks8_h200": orc.DIBSpec([2], [200, 16], [8], 1, feature_embedding_dimension=4, number_positional_encoding_frequencies=8),
    "blocks11": orc.DIBSpec([1, 2], [16], [8], 1, activation_fn="leaky_relu", feature_embedding_dimension=4,
                            number_positional_encoding_frequencies=11),
}
_EXTRA.update(ENVELOPE)
# The kernel's grid stride: a feature's row tiles go to min(ceil(tiles / 4), ceil(2048 / F)) workgroups of 4 waves, so a second
# round of the tile loop needs B > 64 ceil(2048 / F) - more (feature, row) pairs than any case above has.  Two cases with two
# rounds and a ragged second one:
#   stride_f64_linear    F = 64: 32 workgroups x 4 waves = 128 tiles per round; B = 2100 is 132 tiles, the second round has 4 (the
#                        last a tail of 4 rows) and 124 idle waves; one packing of W1, reused by the second round; the fused
#                        large-batch kernels in front (B > 2048)
#   stride_f40_blocks11  F = 40, 11 blocks: 52 workgroups = 208 tiles per round; B = 3400 is 213 tiles, the second round has 5 (the
#                        last a tail of 8 rows); two groups of blocks, so W1 is repacked at every step of both rounds
# Their activations are linear / tanh: with 131 072 (feature, row) pairs x the hidden units of a relu encoder, some ten rows of
# the float64 oracle lie within 1e-6 of a knife edge whatever the seed, more than the 0.1 % a case may exclude - and the kernel
# never sees the activation, which enters only through G.
STRIDE = {
    "stride_f64_linear": (orc.DIBSpec([1] * 64, [32, 32], [32], 1, activation_fn=None, feature_embedding_dimension=32), 2100),
    "stride_f40_blocks11": (orc.DIBSpec([1, 2] * 20, [16], [8], 1, activation_fn="tanh", feature_embedding_dimension=4,
                                        number_positional_encoding_frequencies=11), 3400),
}
_EXTRA.update({k: v[0] for k, v in STRIDE.items()})


def spec_of(name):
    return SPECS.get(name) or _EXTRA[name]


def oracle_cases():
    """(name, B, parameter seed or None) of every case whose rows are the first B of the noise table"""
    return [(n, 40, None) for n in list(SPECS) + list(ENVELOPE)] + [(n, 2100, s) for n, s in LARGE.items()] + [RECOMPUTE] \
        + [(n, b, None) for n, (_, b) in STRIDE.items()]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _engine(spec, p32):
    from dib_amd.engine import HipEngine
    eng = HipEngine(**spec_kwargs(spec), init_seed=0)
    eng.set_flat_params(params_to_flat(eng.blocks, p32, eng.params.numel()))
    eng.set_beta(og.BETA)
    return eng


_REF = {}


def _reference(key, spec, p32, x, y, kind, eps):
    """the float64 dx of a case, computed once and shared by the dispatch paths (their noise is the same table)"""
    if key not in _REF:
        dx64, edge = og.reference(spec, p32, x, y, kind, eps)
        dx64.setflags(write=False)
        _REF[key] = (dx64, edge, eps.copy())
    dx64, edge, eps0 = _REF[key]
    assert np.array_equal(eps, eps0)
    return dx64, edge


def _check(spec, dx, dx64, edge, what):
    dx = np.asarray(dx, dtype=np.float64)
    assert dx.shape == dx64.shape and np.isfinite(dx).all(), what
    B = dx.shape[0]
    bad = np.zeros(B, dtype=bool)
    c0 = 0
    for f, d in enumerate(spec.feature_dimensionalities):
        scale = np.abs(dx64[:, c0: c0 + d]).max()
        err = np.abs(dx[:, c0: c0 + d] - dx64[:, c0: c0 + d]).max(axis=1)
        print(what, "feature", f, "max err / scale", err.max() / scale, "scale", scale, "edge rows", int(edge.sum()))
        bad |= err > TOL * scale
        c0 += d
    assert not (bad & ~edge).any(), (what, np.nonzero(bad & ~edge)[0][:8])
    assert bad.sum() <= int(MAX_EXCLUDED_SHARE * B), (what, int(bad.sum()))


def _step_and_dx(name, B, seed):
    spec = spec_of(name)
    p32, x, y, kind = og.make_case(name, spec, B, param_seed=seed)
    eng = _engine(spec, p32)
    xd, yd = eng.to_device(x), eng.to_device(y)
    eng.train_step(xd, yd, None, 0, B, og.SEED, og.STEP, kind)
    dx = eng.input_grad(xd, None, 0, B)
    eps = eng.eps(None, 0, B, og.SEED, og.STEP).cpu().numpy()
    torch.cuda.synchronize()
    dx64, edge = _reference((name, B, seed), spec, p32, x, y, kind, eps)
    return eng, spec, dx.cpu().numpy(), dx64, edge


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(SPECS))
def test_zoo_parity(name, path):
    """B = 40: two full 16-row tiles and a tail of 8, a partial 64-row tile"""
    with dispatch_path(path):
        _, spec, dx, dx64, edge = _step_and_dx(name, 40, None)
    _check(spec, dx, dx64, edge, f"{name}/{path}")


@pytest.mark.parametrize("name", list(ENVELOPE))
def test_kernel_envelope(name):
    _, spec, dx, dx64, edge = _step_and_dx(name, 40, None)
    _check(spec, dx, dx64, edge, name)


@pytest.mark.parametrize("name", list(STRIDE))
def test_grid_stride_rounds(name):
    """two rounds of the kernel's tile loop, the second ragged (see STRIDE): the tile index of a later round, the packed weights
    reused / repacked across rounds, idle waves that still reach the barriers, a tail tile in the last round"""
    spec, B = STRIDE[name]
    F, tiles = spec.number_features, -(-B // 16)
    per_round = 4 * min(-(-tiles // 4), -(-2048 // F))      # csrc/host/input_grad.h: gx workgroups of 4 waves
    assert per_round < tiles <= 2 * per_round and tiles % per_round != 0 and B % 16 != 0
    _, spec, dx, dx64, edge = _step_and_dx(name, B, None)
    _check(spec, dx, dx64, edge, name)


@pytest.mark.parametrize("name", list(LARGE))
def test_multi_tile_large_batch(name):
    """B = 2100 on the default path: past the row-tile regime (2048 rows), so the fused large-batch kernels with their own grid
    stride and tail tile in front of the new kernel - which here still has one round: 132 row tiles on 33 workgroups x 4 waves
    per feature, the last a tail of 4 rows (its second round: test_grid_stride_rounds)"""
    _, spec, dx, dx64, edge = _step_and_dx(name, 2100, LARGE[name])
    _check(spec, dx, dx64, edge, f"{name}/B2100")


def test_h1_not_stashed():
    """the forward left h1 to the weight gradient's recompute: the entry materialises it before the layer-1 dgrad GEMM"""
    from dib_amd import _lib as L
    name, B, seed = RECOMPUTE
    old = {k: L.get_tuning(k) for k in list(RECOMPUTE_KEYS) + ["wgrad_recompute_h1"]}
    try:
        for k, v in RECOMPUTE_KEYS.items():
            L.set_tuning(k, v)
        out = []
        for arm in (1, 0):
            L.set_tuning("wgrad_recompute_h1", arm)
            eng, spec, dx, dx64, edge = _step_and_dx(name, B, seed)
            assert int(eng.lib.dib_workspace_h1_stashed(eng.layout, _ptr(eng.workspace(B)))) == 1 - arm
            _check(spec, dx, dx64, edge, f"{name}/arm{arm}")
            out.append(dx)
        # relu: h1 enters dx only through the sign of its entries, and the materialised h1 differs from the fused forward's in a
        # last bit at most - no sign of a unit with |z| >= 1e-6 (the seed's criterion) can differ
        assert np.array_equal(out[0], out[1])
    finally:
        for k, v in old.items():
            L.set_tuning(k, v)


@pytest.mark.parametrize("mode", ["row_idx_duplicates", "row0"])
@pytest.mark.parametrize("path", PATHS)
def test_addressing_and_guard_bands(path, mode):
    """ldx > sum_d, lddx > sum_d, a row_idx that repeats rows, row0 > 0; NaN all around dx stays NaN"""
    name, B = "pendulum_ragged", 40
    spec = SPECS[name]
    sum_d = sum(spec.feature_dimensionalities)
    p32, x, y, kind = og.make_case(name, spec, B + 13)
    if mode == "row_idx_duplicates":
        rows = np.random.default_rng(2).integers(0, B + 13, B).astype(np.int32)
        rows[5] = rows[4] = rows[0]
        row0 = 0
    else:
        rows, row0 = None, 7
    ids = rows if rows is not None else np.arange(row0, row0 + B)
    with dispatch_path(path):
        eng = _engine(spec, p32)
        wide = torch.full((B + 13, sum_d + 3), float("nan"), device=eng.device)
        wide[:, :sum_d] = eng.to_device(x)
        xd = wide[:, :sum_d]                      # ldx = sum_d + 3
        yd = eng.to_device(y)
        idx = None if rows is None else eng.to_device(rows, dtype=torch.int32)
        eng.train_step(xd, yd, idx, row0, B, og.SEED, og.STEP, kind)
        lddx = sum_d + 5
        buf = torch.full((B + 4, lddx), float("nan"), device=eng.device)
        dxv = buf[2: 2 + B]
        rc = eng.lib.dib_encoder_bank_input_grad(eng.layout, _ptr(xd), xd.stride(0), _ptr(idx), row0, B, _ptr(eng.params),
                                                 _ptr(eng.workspace(B)), _ptr(dxv), lddx, eng._stream())
        assert rc == 0
        eps = eng.eps(idx, row0, B, og.SEED, og.STEP).cpu().numpy()
        got = buf.cpu().numpy()
    assert np.isnan(got[:2]).all() and np.isnan(got[2 + B:]).all() and np.isnan(got[2: 2 + B, sum_d:]).all()
    dx64, edge = _reference((name, mode), spec, p32, x[ids], y[ids], kind, eps)
    _check(spec, got[2: 2 + B, :sum_d], dx64, edge, f"{name}/{path}/{mode}")
    if rows is not None:   # the same dataset row at three batch positions: the noise is keyed by the row id, so the same gradient
        assert np.array_equal(got[2 + 0, :sum_d], got[2 + 4, :sum_d]) and np.array_equal(got[2 + 0, :sum_d], got[2 + 5, :sum_d])
        assert not np.array_equal(got[2 + 0, :sum_d], got[2 + 1, :sum_d])


@pytest.mark.parametrize("path", PATHS)
def test_refusals_write_nothing(path):
    name, B = "boolean4_32x32", 40
    spec = SPECS[name]
    p32, x, y, kind = og.make_case(name, spec, B)
    with dispatch_path(path):
        eng = _engine(spec, p32)
        xd, yd = eng.to_device(x), eng.to_device(y)
        dx = torch.full((B, 4), float("nan"), device=eng.device)
        ws = eng.workspace(B)
        call = lambda l=eng.layout, x_=xd, b=B, p=eng.params, w=ws, d=dx, ld=4: eng.lib.dib_encoder_bank_input_grad(
            l, _ptr(x_), 4, None, 0, b, _ptr(p), _ptr(w), _ptr(d), ld, eng._stream())
        assert call() == -3                                     # no forward since dib_workspace_init
        eng.train_step(xd, yd, None, 0, B, og.SEED, og.STEP, kind)
        for kw in (dict(l=None), dict(x_=None), dict(p=None), dict(w=None), dict(d=None), dict(b=0), dict(ld=3)):
            assert call(**kw) == -1, kw
        eng.forward(xd, None, 0, B, og.SEED, og.STEP, inference=True)
        assert call() == -3                                     # the last forward wrote no stashes
        torch.cuda.synchronize()
        assert torch.isnan(dx).all()
        eng.train_step(xd, yd, None, 0, B, og.SEED, og.STEP, kind)
        assert call() == 0
        torch.cuda.synchronize()
        assert torch.isfinite(dx).all()


def _model(dims=(1, 1, 2)):
    import dib_amd
    return dib_amd.DistributedIBNet(list(dims), [32, 32], [16], 1, noise_seed=3, init_seed=1)


def _bridge_step(model, x, y, row_ids=None):
    model._step = 0      # the same noise for every call
    leaf = model.flat_parameters
    leaf.grad = None
    pred, kl = model.forward_autograd(x, row_ids=row_ids)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, y) + kl
    loss.backward()
    return leaf.grad.clone()


def test_bridge_returns_dx_and_leaves_the_parameter_gradients_alone():
    model = _model()
    eng = model._ensure_engine()
    B = 40
    rng = np.random.default_rng(0)
    x0 = eng.to_device(rng.standard_normal((B, 4)).astype(np.float32))
    y = eng.to_device(rng.integers(0, 2, (B, 1)).astype(np.float32))
    n0 = eng.lib.dib_launch_count()
    g_plain = _bridge_step(model, x0, y)
    n_plain = eng.lib.dib_launch_count() - n0
    assert x0.grad is None
    x = x0.clone().requires_grad_()
    n0 = eng.lib.dib_launch_count()
    g_dx = _bridge_step(model, x, y)
    n_dx = eng.lib.dib_launch_count() - n0
    assert x.grad is not None and x.grad.shape == x.shape
    assert torch.equal(x.grad, eng.input_grad(x.detach(), None, 0, B))
    assert torch.equal(g_plain, g_dx)                       # bit-identical parameter gradients
    assert 1 <= n_dx - n_plain <= 3                         # the new kernel (+ the layer-1 dgrad GEMM): only when x asks
    first = x.grad.clone()
    x.grad = None
    g_again = _bridge_step(model, x, y)
    assert torch.equal(x.grad, first) and torch.equal(g_again, g_dx)
    # row_ids: the forward gathers x[row_ids], so x.grad sums the batch positions of each row
    ids = torch.arange(B, dtype=torch.int32, device=eng.device)
    ids[4] = ids[5] = 0
    ids[9] = 3
    xr = x0.clone().requires_grad_()
    model._step = 0
    pred, kl = model.forward_autograd(xr, row_ids=ids)
    (torch.nn.functional.binary_cross_entropy_with_logits(pred, y) + kl).backward()
    per_pos = eng.input_grad(xr.detach(), ids, 0, B).double().cpu()
    want = torch.zeros(B, 4, dtype=torch.float64).index_add_(0, ids.long().cpu(), per_pos)
    assert torch.allclose(xr.grad.double().cpu(), want, rtol=1e-6, atol=1e-9)
    assert (xr.grad[[4, 5, 9]] == 0).all() and (xr.grad[0] != per_pos[0].float().to(eng.device)).any()


def test_double_backward_raises():
    model = _model()
    eng = model._ensure_engine()
    x = torch.randn(8, 4, device=eng.device).requires_grad_()
    pred, kl = model.forward_autograd(x)
    gx, = torch.autograd.grad(pred.sum() + kl, x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_composition_upstream_module_gets_the_float64_gradient():
    """torch.nn.Linear(6, 4) + tanh on the device -> DistributedIBModule([1, 1, 2]) -> BCE + KL: the Linear's weight and bias
    gradients against the float64 chain rule from the oracle's dx at the activations the device produced.
    Bound per entry: every dz[b, j] = dx[b, j] (1 - a^2) carries at most TOL max|dx64| (the dx tolerance; tanh' adds two roundings)
    and the float32 sum over B rows gamma_B: (TOL + (B + 4) 2^-24) * sum_b max|dx64| |raw[b, i]|."""
    import dib_amd
    torch.manual_seed(0)
    B = 16
    net = _model()
    dib = dib_amd.DistributedIBModule(net)
    eng = net._ensure_engine()
    assert [n for n, _ in dib.named_parameters()] == ["flat_parameters"]
    assert dib.flat_parameters.data_ptr() == eng.params.data_ptr()
    lin = torch.nn.Linear(6, 4).to(eng.device)
    raw = torch.randn(B, 6, device=eng.device)
    y = (torch.rand(B, 1, device=eng.device) > 0.5).float()
    act = torch.tanh(lin(raw))
    pred, kl = dib(act)
    (torch.nn.functional.binary_cross_entropy_with_logits(pred, y) + kl).backward()
    assert lin.weight.grad is not None and lin.bias.grad is not None and dib.flat_parameters.grad is not None
    spec = orc.DIBSpec([1, 1, 2], [32, 32], [16], 1)
    p32 = flat_to_params(eng.blocks, eng.get_flat_params(), spec, dtype=np.float32)
    a = act.detach().cpu().numpy()
    eps = eng.eps(None, 0, B, net.noise_seed, 0).cpu().numpy()
    dx64, edge = og.reference(spec, p32, a, y.cpu().numpy(), "bce_logits", eps, beta=float(net.beta.value()))
    assert not edge.any(), "pick another torch seed: a relu unit of the float64 oracle sits on a knife edge"
    a64, raw64 = a.astype(np.float64), raw.cpu().numpy().astype(np.float64)
    dz = dx64 * (1.0 - a64 * a64)
    bound = (TOL + (B + 4) * 2.0 ** -24) * np.abs(dx64).max()
    errw = np.abs(lin.weight.grad.cpu().numpy() - dz.T @ raw64)
    errb = np.abs(lin.bias.grad.cpu().numpy() - dz.sum(0))
    print("weight err", errw.max(), "bound", (bound * np.abs(raw64).sum(0)).min(), "bias err", errb.max(), "bound", bound * B)
    assert (errw <= bound * np.abs(raw64).sum(0)[None, :]).all()
    assert (errb <= bound * B).all()
    # three lines: subnetwork -> DIB -> torch optimizer
    opt = torch.optim.Adam(list(lin.parameters()) + list(dib.parameters()), lr=1e-3)
    before = eng.get_flat_params().copy()
    opt.step()
    assert not np.array_equal(eng.get_flat_params(), before)     # the optimizer wrote the buffer the kernels read
    # a Parameter that no longer aliases the engine's buffer would get no gradient: refused, not silent
    dib.flat_parameters.data = dib.flat_parameters.data.clone()
    with pytest.raises(RuntimeError, match="no longer shares memory"):
        dib(act.detach())
