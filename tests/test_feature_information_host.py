"""Every feature's information bounds in one evaluation, without a device: the draw rule of the evaluation batches
(utils.evaluation_batch_rows) against the three lines the per-feature loop has always drawn them with, the host-only envelope
calls of include/dib_mi_features.h (dib_mi_features_supported / dib_mi_features_workspace_bytes) at the envelope's corners and
just outside them, the binding, and the figure."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -4   # include/dib_hip.h DIB_E_ARG, DIB_E_UNSUPPORTED


@pytest.mark.parametrize("n,bs,nb,seed", [(300, 100, 3, 0), (1024, 1024, 8, 7), (60, 100, 2, 5), (1, 4, 2, 3), (5000, 1024, 8, 11)])
def test_evaluation_batch_rows_is_the_draw_of_the_per_feature_loop(n, bs, nb, seed):
    from dib_amd import utils
    rng = np.random.default_rng(seed)
    want = []
    for b in range(nb):
        rows = rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs)
        want.append(rows)
    got = utils.evaluation_batch_rows(n, bs, nb, seed)
    assert got.shape == (nb, bs) and got.dtype == np.int64
    assert np.array_equal(got, np.stack(want))
    assert got.min() >= 0 and got.max() < n
    if n >= bs:
        assert all(len(set(r)) == bs for r in got)   # without replacement


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


@pytest.mark.parametrize("E", [1, 3, 64, 68, 256])
@pytest.mark.parametrize("n", [2, 16384])
def test_envelope_corners_are_accepted(E, n):
    lib = _lib()
    for F, nb in ((65535, 1), (1, 65535), (257, 255), (1, 1)):
        assert lib.dib_mi_features_supported(F, E, n, nb) == 1, (F, nb)
        need = lib.dib_mi_features_workspace_bytes(F, E, n, nb)
        # at least the folded table (16 E + 8 bytes per row) and one (max, sum) partial and one own log-density per row
        assert need >= F * nb * n * (16 * E + 8 + 24), (F, nb, need)


@pytest.mark.parametrize("F,E,n,nb,code", [(1, 65, 64, 1, UNSUPPORTED), (1, 260, 64, 1, UNSUPPORTED), (1, 32, 1, 1, UNSUPPORTED),
                                           (65536, 32, 64, 1, UNSUPPORTED), (256, 32, 64, 256, UNSUPPORTED),
                                           (1, 66, 64, 1, UNSUPPORTED), (1, 32, 16385, 1, UNSUPPORTED),
                                           (0, 32, 64, 1, ARG), (1, 0, 64, 1, ARG), (1, 32, 0, 1, ARG), (1, 32, 64, 0, ARG),
                                           (-1, 32, 64, 1, ARG), (1, 32, 64, -3, ARG)])
def test_outside_the_envelope_is_refused_with_the_documented_code(F, E, n, nb, code):
    lib = _lib()
    assert lib.dib_mi_features_supported(F, E, n, nb) == 0
    assert lib.dib_mi_features_workspace_bytes(F, E, n, nb) == code


def test_workspace_does_not_depend_on_how_the_groups_split_into_features_and_batches():
    """the split count is a function of n alone: F x nb groups need the same workspace however they factor"""
    lib = _lib()
    for E, n in ((32, 1024), (5, 300), (128, 70), (8, 5000)):
        sizes = {lib.dib_mi_features_workspace_bytes(F, E, n, nb) for F, nb in ((64, 8), (8, 64), (512, 1), (1, 512))}
        assert len(sizes) == 1 and min(sizes) > 0, (E, n, sizes)


def test_binding_and_header():
    from dib_amd import _lib
    header = open(os.path.join(ROOT, "include", "dib_mi_features.h")).read()
    for name, (_, args) in _lib.SIGNATURES_MI_FEATURES.items():
        decl = header[header.index(name + "("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == len(args), name
    lib = _lib.load_library()
    assert lib.dib_mi_features_bounds.argtypes == _lib.SIGNATURES_MI_FEATURES["dib_mi_features_bounds"][1]
    assert lib.dib_abi_version() == 7 == _lib.ABI_VERSION
    import dib_amd
    assert callable(dib_amd.DistributedIBNet.information_per_feature)
    from dib_amd import train
    assert train.get_args([]).info_bounds_frequency == 0
    assert train.get_args(["--info_bounds_frequency", "5"]).info_bounds_frequency == 5


def test_info_plane_in_mutual_information_bounds_writes_a_file(tmp_path):
    from dib_amd import visualization
    rng = np.random.default_rng(0)
    lower = np.abs(rng.standard_normal((6, 3)))
    bounds = np.stack([lower, lower + 0.2], -1)
    bounds[0, 1, 1] = np.inf   # the upper bound of a channel whose encodings are far apart
    info = {"epochs": [0, 2, 4, 6, 8, 10], "beta": list(np.geomspace(1e-3, 1, 6)), "bounds": bounds}
    for k, loss in enumerate((np.linspace(1.0, 0.3, 11), np.linspace(1.0, 0.3, 6))):   # one value per epoch / per evaluation
        out = visualization.save_distributed_info_plane_mi(info, loss, str(tmp_path / f"p{k}"), entropy_y=1.0)
        assert os.path.basename(out) == "distributed_info_plane_mi.png" and os.path.getsize(out) > 1000
    single = {"epochs": [3], "beta": [0.1], "bounds": bounds[:1, :1]}
    assert os.path.getsize(visualization.save_distributed_info_plane_mi(single, [0.5] * 4, str(tmp_path / "one"))) > 1000
    with pytest.raises(ValueError):
        visualization.save_distributed_info_plane_mi({"epochs": [0], "bounds": bounds}, [0.5], str(tmp_path / "bad"))
