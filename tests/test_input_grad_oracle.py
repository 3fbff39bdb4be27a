"""CPU: the float64 oracle of dL/dx (tests/_oracle_input_grad.py) against central differences of the oracle's own loss, the new
entry point's declaration / binding / export, DistributedIBModule's refusal to exist without a GPU, and the numbers the GPU
test's tolerance and seeds rest on (tests/test_gpu_input_grad.py), re-measured here."""
import os
import re

import numpy as np
import pytest

import dib_oracle as orc
import _oracle_input_grad as og
from _helpers import SPECS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FD_SPECS = {
    "ragged_posenc": orc.DIBSpec([3, 5, 1], [17, 9], [13], 3, activation_fn="tanh", feature_embedding_dimension=6,
                                 number_positional_encoding_frequencies=3),
    "no_posenc": orc.DIBSpec([4, 2], [24], [20, 12], 2, use_positional_encoding=False, activation_fn="elu",
                             feature_embedding_dimension=8),
    "no_hidden": orc.DIBSpec([1, 2], [], [], 1, feature_embedding_dimension=4),
}


@pytest.mark.parametrize("name", list(FD_SPECS))
def test_oracle_dx_matches_central_differences_of_its_own_loss(name):
    """smooth activations, so the loss is differentiable everywhere: h = 1e-6, central differences of a float64 loss of O(1) carry
    ~1e-16 / 1e-6 = 1e-10 of round-off and O(h^2) = 1e-12 of truncation times the third derivative (<= 16^3 from the sinusoids)"""
    spec = FD_SPECS[name]
    B = 5
    rng = np.random.default_rng(3)
    p = og.as_dtype(og.make_case(name, spec, B, param_seed=7)[0], np.float64)
    x = rng.standard_normal((B, sum(spec.feature_dimensionalities)))
    kind = og.loss_kind_of(name, spec)
    y = rng.integers(0, spec.output_dimensionality, (B, 1)).astype(np.float64) if kind == "sparse_cce_logits" \
        else rng.integers(0, 2, (B, 1)).astype(np.float64)
    eps = rng.standard_normal((B, spec.number_features, spec.feature_embedding_dimension))
    beta = 0.37
    dx = og.input_grad(spec, p, x, y, orc.forward(spec, p, x, eps), beta, kind)
    assert dx.shape == x.shape
    h = 1e-6
    fd = np.zeros_like(x)
    for b in range(B):
        for c in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[b, c] += h
            xm[b, c] -= h
            fd[b, c] = (og.loss_value(spec, p, xp, y, eps, beta, kind) - og.loss_value(spec, p, xm, y, eps, beta, kind)) / (2 * h)
    assert np.abs(dx).max() > 1e-4
    assert np.abs(dx - fd).max() <= 1e-8 + 1e-7 * np.abs(dx).max(), (np.abs(dx - fd).max(), np.abs(dx).max())


def test_entry_point_is_declared_bound_and_exported():
    from dib_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dib_hip.h")).read()
    assert re.search(r"^int\s+dib_encoder_bank_input_grad\s*\(", hdr, re.M)
    assert re.search(r"#define DIB_ABI_VERSION 7\b", hdr)
    assert "dib_encoder_bank_input_grad" in _lib.SIGNATURES and len(_lib.SIGNATURES["dib_encoder_bank_input_grad"][1]) == 11
    lib = _lib.load_library()
    assert hasattr(lib, "dib_encoder_bank_input_grad")
    # host-side refusals need no device: null arguments
    assert lib.dib_encoder_bank_input_grad(None, None, 0, None, 0, 0, None, None, None, 0, None) == -1


def test_module_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import dib_amd
    assert issubclass(dib_amd.DistributedIBModule, torch.nn.Module)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dib_amd.DistributedIBModule(dib_amd.DistributedIBNet([1, 1], [8], [8], 1))


def test_gpu_test_tolerance_and_seeds_are_what_float32_arithmetic_gives():
    """The GPU test's numbers, re-derived: over its cases the float32 restatement of the oracle stays within RATIO32 of the float64
    one on every row, and no case has more rows with a hidden pre-activation within 1e-6 of zero (ten times what float32 rounding
    moves one) than it may exclude."""
    import test_gpu_input_grad as t
    worst = 0.0
    for name, B, seed in t.oracle_cases():
        spec = t.spec_of(name)
        p32, x, y, kind = og.make_case(name, spec, B, param_seed=seed)
        eps = orc.philox_normal_all(og.SEED, og.STEP, np.arange(B), spec.number_features,
                                    spec.feature_embedding_dimension).astype(np.float32)
        dx64, edge = og.reference(spec, p32, x, y, kind, eps)
        p64 = og.as_dtype(p32, np.float64)
        c = orc.forward(spec, p64, x.astype(np.float64), eps.astype(np.float64))
        near = og.knife_edge_rows(spec, p64, x.astype(np.float64), c, thresh=1e-6)
        assert near.sum() <= int(t.MAX_EXCLUDED_SHARE * B), (name, B, seed, int(near.sum()))
        dx32 = og.restatement_float32(spec, p32, x, y, kind, eps)
        worst = max(worst, max(og.block_errors(spec, dx32, dx64, keep=~near)))
    assert worst <= t.RATIO32, worst
    assert t.TOL == 8 * t.RATIO32 and t.TOL <= t.PARITY_BOUND
