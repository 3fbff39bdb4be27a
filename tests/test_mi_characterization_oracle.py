"""MI-bound characterization without a device: the float64 oracle of the Monte-Carlo estimate (tests/
_oracle_mi_characterization.py) against the notebook's literal formula, against closed forms and against a known answer; the
C-ABI binding of the new entry points; the figure."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle_mi_characterization as omc  # noqa: E402
import dib_oracle as orc  # noqa: E402


def test_lse_term_equals_the_literal_raw_exp_formula():
    """small enough not to underflow: 6 dimensions, separation 1.5, unit variances"""
    rng = np.random.default_rng(0)
    mus = np.concatenate([rng.integers(0, 2, (48, 3)) * 2 - 1.0, np.zeros((48, 3))], -1) * 1.5
    src = rng.integers(0, 48, 500)
    u = omc.sample_u(mus, np.zeros_like(mus), src, seed=3, step=1)
    a, b = omc.mc_terms_lse(mus, np.zeros_like(mus), u, src), omc.mc_terms_literal(mus, u, src)
    assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max()


def test_closed_form_anchors_at_separation_zero():
    """all conditionals equal: every Monte-Carlo term is 0, the InfoNCE bound is 0 and the leave-one-out bound log(n / (n - 1))"""
    rng = np.random.default_rng(1)
    n, E = 64, 8
    mus, lvs = np.zeros((n, E)), np.zeros((n, E))
    src = rng.integers(0, n, 300)
    u = omc.sample_u(mus, lvs, src, seed=5, step=0)
    assert np.abs(omc.mc_terms_lse(mus, lvs, u, src)).max() <= 1e-12
    for b in range(3):
        lo, up = orc.mi_sandwich_bounds_batch(mus, lvs, orc.mi_sandwich_sample_u(mus, lvs, 5, b, 0))
        assert abs(lo) <= 1e-12 and abs(up - np.log(n / (n - 1.0))) <= 1e-12


KNOWN = [(1, 1.0, 0.48594), (2, 1.0, 0.97189), (4, 1.5, 3.03992), (6, 3.0, 5.96668), (6, 0.75, 1.91449)]


@pytest.mark.parametrize("k,d,bits", KNOWN)
def test_known_answer_k_independent_bits(k, d, bits):
    """balanced {+-1}^k dataset, unit variances: I(U;X) = k I_1(d) (one-dimensional quadrature).  The oracle on 20 000 Philox
    samples over 1 024 rows lies within 5 standard errors (of its own per-sample terms) of it; the 5 sigma are a cap on chance
    (about 6e-7 per case), the seeds are fixed."""
    truth = k * omc.one_bit_information(d)
    assert abs(truth - bits) < 1e-5
    mus = omc.balanced_signs(k, 1024) * d
    lvs = np.zeros_like(mus)
    src = np.random.default_rng([7, k]).integers(0, 1024, 20000)
    u = omc.sample_u(mus, lvs, src, seed=11, step=k)
    terms = omc.mc_terms_lse(mus, lvs, u, src) / np.log(2.0)
    se = terms.std(ddof=1) / np.sqrt(len(terms))
    z = (terms.mean() - truth) / se
    print(f"k={k} d={d}: truth {truth:.5f} oracle {terms.mean():.5f} se {se:.5f} z {z:+.2f}")
    assert abs(z) <= 5.0


def test_binding_header_and_abi_version():
    from dib_amd import _lib
    for name in ("dib_mi_monte_carlo_workspace_bytes", "dib_mi_monte_carlo"):
        assert name in _lib.SIGNATURES_MI_CHANNEL
    assert len(_lib.SIGNATURES_MI_CHANNEL["dib_mi_monte_carlo"][1]) == 15
    header = open(os.path.join(ROOT, "include", "dib_mi_channel.h")).read()
    assert "int dib_mi_monte_carlo(" in header and "int64_t dib_mi_monte_carlo_workspace_bytes(" in header
    assert re.search(r"#define DIB_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "dib_hip.h")).read())
    assert _lib.ABI_VERSION == 7
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load_library(build_if_missing=False)
        assert lib.dib_mi_monte_carlo.argtypes == _lib.SIGNATURES_MI_CHANNEL["dib_mi_monte_carlo"][1]
        assert lib.dib_abi_version() == 7
    import dib_amd
    assert dib_amd.mi_characterization.VARIABLES[3].sample(np.random.default_rng(0), 5).shape == (5, 6)
    assert callable(dib_amd.utils.estimate_mi_sandwich_bounds_from_parameters)


def test_gaussian_channel_and_variables():
    from dib_amd import mi_characterization as mic
    x = np.array([[1, -1], [-1, -1], [1, 1]])
    mus, lvs = mic.gaussian_channel(x, 2.5, embedding_dimension=5, logvar=0.25)
    assert mus.shape == lvs.shape == (3, 5)
    assert (mus[:, :2] == x * 2.5).all() and (mus[:, 2:] == 0).all() and (lvs == 0.25).all()
    assert [v.name for v in mic.VARIABLES] == ["bits1", "bits2", "bits4", "bits6", "uniform"]
    for v in mic.VARIABLES:
        a, b = v.sample(np.random.default_rng(4), 100), v.sample(np.random.default_rng(4), 100)
        assert (a == b).all() and len(v.separation_scales) == 25 and v.separation_scales[0] == 0.0
    assert set(np.unique(mic.VARIABLES[2].sample(np.random.default_rng(0), 200))) == {-1, 1}
    u = mic.VARIABLES[4].sample(np.random.default_rng(0), 200)
    assert u.shape == (200, 1) and u.min() >= -0.5 and u.max() <= 0.5


def test_save_figure_draws_the_curve_the_bounds_and_their_residuals(tmp_path):
    pytest.importorskip("matplotlib")
    from dib_amd import mi_characterization as mic
    rng = np.random.default_rng(2)
    S, bss = 7, [64, 256, 1024]
    scales = np.linspace(0, 3, S)
    mc = 1.0 - np.exp(-scales)
    stats = np.empty((3, S, 4))
    for k in range(3):
        stats[k, :, 0] = mc - 0.03 / (k + 1)
        stats[k, :, 2] = mc + 0.04 / (k + 1)
        stats[k, :, 1] = stats[k, :, 3] = 0.01
    result = {"monte_carlo": mc, "info_bound_stats": stats, "separation_scales": scales, "evaluation_batch_sizes": bss,
              "info_bound_estimates": rng.standard_normal((3, S, 4, 2))}
    path = str(tmp_path / "fig.png")
    fig = mic.save_figure(result, path, label="synthetic", info_plot_lims=(0, 1.2))
    assert os.path.getsize(path) > 1000
    top, bottom = fig.axes
    lines = {l.get_label(): l for l in top.get_lines()}
    assert np.allclose(lines["Monte Carlo"].get_ydata(), mc)
    for k, bs in enumerate(bss):
        assert np.allclose(lines[f"lower, batch {bs}"].get_ydata(), stats[k, :, 0])
        assert np.allclose(lines[f"upper, batch {bs}"].get_ydata(), stats[k, :, 2])
    res = {l.get_label(): l for l in bottom.get_lines()}
    for k, bs in enumerate(bss):
        assert np.allclose(res[f"lower residual, batch {bs}"].get_ydata(), stats[k, :, 0] - mc)
        assert np.allclose(res[f"upper residual, batch {bs}"].get_ydata(), stats[k, :, 2] - mc)
    assert tuple(bottom.get_ylim()) == (-0.1, 0.1)
    assert mic.largest_residuals(result)[1024] == pytest.approx((0.01, 0.04 / 3))
