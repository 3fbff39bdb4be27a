"""The checker of tests/test_gpu_st_information.py (tests/_oracle_st_information.py) and the package's information-plane tail,
pinned on the set-transformer notebook's own statements executed on the NumPy TF stand-in
(tests/golden/make_golden_st_information.py -> tests/golden/st_information.npz): cell 5's compute_infos_mus_logvars and
cell 8's information plane.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import _oracle_st_information as osi  # noqa: E402
import dib_oracle as orc  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "st_information.npz")


def test_sandwich_oracle_matches_compute_infos_mus_logvars():
    g = np.load(GOLD)
    for k in range(3):
        mus, lv, eps = g[f"mus{k}"], g[f"logvars{k}"], g[f"eps{k}"]
        u = mus + np.exp(lv / 2.0) * eps
        lit = osi.sandwich_bounds(mus, lv, u, form="literal")
        lse = osi.sandwich_bounds(mus, lv, u, form="lse")
        ref = (float(g[f"lower{k}"]), float(g[f"upper{k}"]))
        assert np.allclose(lit, ref, rtol=1e-12, atol=1e-12), (k, lit, ref)
        assert np.allclose(lse, ref, rtol=1e-11, atol=1e-11), (k, lse, ref)
        # the package's other restatement of the same estimator (utils.py's compute_batch)
        assert np.allclose(orc.mi_sandwich_bounds_batch(mus, lv, u), ref, rtol=1e-12, atol=1e-12)
        n = mus.shape[0]
        assert ref[0] <= np.log(n) + 1e-12 and ref[0] <= ref[1]


def test_lse_forms_survive_where_the_literal_form_underflows():
    rng = np.random.default_rng(0)
    mus = rng.standard_normal((12, 8)) * 60.0
    lv = rng.standard_normal((12, 8)) * 0.3 - 3.0
    u = mus + np.exp(lv / 2.0) * rng.standard_normal((12, 8))
    lo_l, up_l = osi.sandwich_rows_literal(mus, lv, u)
    lo, up = osi.sandwich_rows_lse(mus, lv, u)
    assert not np.isfinite(up_l).all() and np.isfinite(up).all() and np.isfinite(lo).all()
    assert np.allclose(lo, np.log(12), atol=1e-9)   # every other Gaussian is far away: the lower bound saturates at log n
    p_lo, p_up = osi.probe_rows_lse(mus[:3], lv[:3], u[:3], mus[3:], lv[3:])
    assert np.isfinite(p_up).all() and np.allclose(p_lo, np.log(10), atol=1e-9)


def test_probe_oracle_lse_form_equals_the_literal_restatement():
    import set_transformer_oracle as sto
    g = np.load(os.path.join(ROOT, "tests", "golden", "probe_grid_bounds.npz"))
    u = g["mus_probes"] + np.exp(g["logvars_probes"] / 2.0) * g["eps"]
    lo, up = osi.probe_rows_lse(g["mus_probes"], g["logvars_probes"], u, g["mus_data"], g["logvars_data"])
    assert np.abs(lo - g["infonce_per"]).max() < 1e-11 and np.abs(up - g["loo_per"]).max() < 1e-10
    rlo, rup = sto.probe_info_bounds(g["mus_probes"], g["logvars_probes"], u, g["mus_data"], g["logvars_data"])
    assert np.abs(lo - rlo).max() < 1e-11 and np.abs(up - rup).max() < 1e-10


def test_information_plane_matches_the_notebook_tail():
    from dib_amd.set_transformer import information_plane
    g = np.load(GOLD)
    info_in, info_out, acc = osi.information_plane(g["hist_bce"], g["hist_acc"], g["hist_info_bounds"])
    assert np.allclose(info_in, g["info_in"], rtol=1e-6) and np.allclose(info_out, g["info_out"], rtol=1e-6)
    assert np.allclose(acc, g["acc_plot"], rtol=1e-6)
    ip = information_plane(dict(bce_series_val=list(g["hist_bce"]), acc_series_val=list(g["hist_acc"]),
                                info_bounds=list(g["hist_info_bounds"])))
    assert np.allclose(ip["info_in"], g["info_in"], rtol=1e-6) and np.allclose(ip["info_out"], g["info_out"], rtol=1e-6)
    assert np.allclose(ip["acc"], g["acc_plot"], rtol=1e-6) and ip["info_out"].shape == (21,)


def test_notebook_probe_grid():
    from dib_amd.set_transformer import notebook_probe_grid
    p = notebook_probe_grid()
    assert p.shape == (10000, 2) and p.dtype == np.float32
    assert p[0].tolist() == [-3.0, -3.0] and p[1, 0] > p[0, 0] and p[100, 1] > p[0, 1] and p[-1].tolist() == [3.0, 3.0]
