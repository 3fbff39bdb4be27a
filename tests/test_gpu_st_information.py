"""Information tracking of the set-transformer notebook on the device (csrc/dib_st_info.h through include/dib_st.h and
SetTransformerDIB.information_bounds / information_maps / fit(track_information=True)):
  - dib_mi_sandwich_batched and dib_mi_probe_map against the float64 oracle (tests/_oracle_st_information.py) on the device's own
    samples, and the samples against the Philox reference, across the envelope (E, particles, batches, tiles, duplicates, offsets,
    far-apart Gaussians, the notebook's 25 600 data rows per batch);
  - equality with the paths they replace: the per-batch loop of dib_mi_sandwich_rows and the per-(chunk, batch) loop of
    dib_mi_probe_bounds on shared encodings, information_maps against information_map;
  - bit-identical replay and refusals; fit with tracking = fit without it; the tracked schedule and its files."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle_st_information as osi  # noqa: E402
import dib_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(rng, n_val, P, E, spread=1.0):
    """synthetic encoder outputs [n_val * P, 2E] (mu | raw logvar) on the device"""
    mu = rng.standard_normal((n_val * P, E)) * spread
    lv = rng.standard_normal((n_val * P, E)) * 0.4 + 1.0
    return torch.tensor(np.concatenate([mu, lv], 1), dtype=torch.float32, device="cuda")


def _sandwich(lib, enc, n_val, P, E, idx, off, seed, step, rows=True):
    nb, nn = idx.shape
    ws = torch.empty(int(lib.dib_mi_sandwich_batched_workspace_bytes(n_val, P, E, nb, nn)) // 8 + 2, dtype=torch.float64, device="cuda")
    out = torch.empty((2, nb), dtype=torch.float64, device="cuda")
    r = torch.empty((2, nb, nn * P), dtype=torch.float64, device="cuda")
    u = torch.empty((nb, nn * P, E), dtype=torch.float64, device="cuda")
    idx_d = torch.tensor(idx, dtype=torch.int32, device="cuda")
    rc = lib.dib_mi_sandwich_batched(_p(enc), n_val, P, E, _p(idx_d), nb, nn, off, seed, step, _p(out[0]), _p(out[1]),
                                     _p(r[0]) if rows else None, _p(r[1]) if rows else None, _p(u), _p(ws), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), r.cpu().numpy(), u.cpu().numpy()


def _probe_map(lib, ep, enc, n_val, P, E, idx, steps, C, off, seed):
    n_chunks, nb, nn = idx.shape
    M = ep.shape[0]
    ws = torch.empty(int(lib.dib_mi_probe_map_workspace_bytes(M, C, n_val, P, E, nb, nn)) // 8 + 2, dtype=torch.float64, device="cuda")
    out = torch.empty((2, M), dtype=torch.float64, device="cuda")
    u = torch.empty((n_chunks, nb, C, E), dtype=torch.float64, device="cuda")
    idx_d = torch.tensor(idx, dtype=torch.int32, device="cuda")
    st_d = torch.tensor(np.asarray(steps, dtype=np.uint32).view(np.int32), device="cuda")
    rc = lib.dib_mi_probe_map(_p(ep), M, C, _p(enc), n_val, P, E, _p(idx_d), nb, nn, off, seed, _p(st_d), _p(out[0]), _p(out[1]),
                              _p(u), _p(ws), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), u.cpu().numpy()


def _rows(enc_np, P, nbhds):
    return np.concatenate([enc_np[k * P:(k + 1) * P] for k in nbhds], 0)


def _eps(seed, step, n, E):
    return orc.philox_normal_all(seed, step, np.arange(n, dtype=np.uint32), 1, E)[:, 0, :]


SANDWICH_CASES = [  # E, P, nb, n_nbhd, offset, n_val
    (4, 13, 3, 5, -3.0, 9), (32, 50, 16, 2, -3.0, 7), (36, 1, 3, 2, 0.0, 4), (256, 13, 1, 3, -3.0, 5), (32, 1, 16, 70, 0.0, 90),
    (32, 50, 3, 32, -3.0, 40)]


@pytest.mark.parametrize("E,P,nb,nn,off,n_val", SANDWICH_CASES)
def test_batched_sandwich_bounds_match_oracle(E, P, nb, nn, off, n_val):
    """per-row and per-batch bounds against the log-sum-exp restatement on the device's samples; samples = mu + sigma * Philox
    (seed, step + batch, row, 0); duplicated neighbourhoods stay separate rows"""
    lib = _lib()
    rng = np.random.default_rng(E * 1000 + P)
    enc = _table(rng, n_val, P, E)
    idx = rng.integers(0, n_val, (nb, nn))
    idx[0, :] = idx[0, 0]   # one batch made of a single neighbourhood repeated
    seed, step = 77, 5
    out, rows, u = _sandwich(lib, enc, n_val, P, E, idx, off, seed, step)
    e = enc.cpu().numpy().astype(np.float64)
    for b in range(nb):
        x = _rows(e, P, idx[b])
        mus, lvs = x[:, :E], x[:, E:] + off
        ref_u = mus + np.exp(lvs / 2.0) * _eps(seed, step + b, nn * P, E)
        assert np.abs(u[b] - ref_u).max() < 1e-5 * (1 + np.abs(ref_u).max())
        lo, up = osi.sandwich_rows_lse(mus, lvs, u[b])
        tol = 1e-8 * (1 + max(np.abs(lo).max(), np.abs(up).max()))
        assert np.abs(rows[0, b] - lo).max() < tol and np.abs(rows[1, b] - up).max() < tol, b
        assert abs(out[0, b] - lo.mean()) < tol and abs(out[1, b] - up.mean()) < tol
        assert (rows[0, b] <= np.log(nn * P) + 1e-9).all()


def test_batched_sandwich_equals_the_per_batch_rows_loop():
    """offset 0 (dib_mi_sandwich_rows has none): the batched launch against one dib_mi_sandwich_rows per batch on the gathered rows"""
    lib = _lib()
    rng = np.random.default_rng(3)
    E, P, nb, nn, n_val = 32, 50, 4, 6, 20
    enc = _table(rng, n_val, P, E)
    idx = rng.integers(0, n_val, (nb, nn))
    seed, step = 11, 100
    out, rows, _ = _sandwich(lib, enc, n_val, P, E, idx, 0.0, seed, step)
    n = nn * P
    ws = torch.empty(int(lib.dib_mi_workspace_bytes(n, E)) // 8 + 2, dtype=torch.float64, device="cuda")
    for b in range(nb):
        eb = torch.cat([enc[k * P:(k + 1) * P] for k in idx[b]]).contiguous()
        r = torch.empty((2, n), dtype=torch.float64, device="cuda")
        assert lib.dib_mi_sandwich_rows(_p(eb), n, E, seed, step + b, 0, _p(r[0]), _p(r[1]), _p(ws), _st()) == 0
        r = r.cpu().numpy()
        scale = 1 + np.abs(r).max()
        assert np.abs(rows[0, b] - r[0]).max() <= 1e-12 * scale and np.abs(rows[1, b] - r[1]).max() <= 1e-12 * scale


PROBE_CASES = [  # E, P, nb, n_nbhd, M, C, offset
    (4, 13, 3, 4, 70, 30, -3.0), (32, 50, 3, 6, 130, 100, -3.0), (36, 1, 1, 40, 65, 64, 0.0), (256, 13, 3, 2, 20, 7, -3.0),
    (32, 50, 16, 2, 33, 33, -3.0)]


@pytest.mark.parametrize("E,P,nb,nn,M,C,off", PROBE_CASES)
def test_probe_map_matches_oracle(E, P, nb, nn, M, C, off):
    """per probe: mean over the batches of the LSE-form bounds on the device's samples; samples keyed (seed, steps[c][b],
    row in chunk, 0); chunks and probes that are not multiples of the 64-probe tile"""
    lib = _lib()
    rng = np.random.default_rng(E + 7 * P + M)
    n_val = 11
    enc = _table(rng, n_val, P, E)
    ep = _table(rng, M, 1, E)
    n_chunks = -(-M // C)
    idx = rng.integers(0, n_val, (n_chunks, nb, nn))
    steps = rng.integers(0, 2 ** 32, (n_chunks, nb), dtype=np.uint64)
    seed = 2 ** 40 + 9
    out, u = _probe_map(lib, ep, enc, n_val, P, E, idx, steps, C, off, seed)
    e, pe = enc.cpu().numpy().astype(np.float64), ep.cpu().numpy().astype(np.float64)
    ref = np.zeros((2, M))
    for c in range(n_chunks):
        sl = slice(c * C, min(M, c * C + C))
        m = sl.stop - sl.start
        mus, lvs = pe[sl, :E], pe[sl, E:] + off
        for b in range(nb):
            ref_u = mus + np.exp(lvs / 2.0) * _eps(seed, int(steps[c, b]), m, E)
            assert np.abs(u[c, b, :m] - ref_u).max() < 1e-5 * (1 + np.abs(ref_u).max())
            x = _rows(e, P, idx[c, b])
            lo, up = osi.probe_rows_lse(mus, lvs, u[c, b, :m], x[:, :E], x[:, E:] + off)
            ref[0, sl] += lo
            ref[1, sl] += up
    ref /= nb
    assert np.abs(out - ref).max() < 1e-8 * (1 + np.abs(ref).max())
    assert (out[0] <= np.log(nn * P + 1) + 1e-9).all() and (out[0] <= out[1] + 1e-9).all()


def test_probe_map_equals_the_probe_bounds_loop():
    """the one-launch map against the loop it replaces: dib_mi_probe_bounds per (chunk, batch) on the gathered rows, averaged"""
    lib = _lib()
    rng = np.random.default_rng(5)
    E, P, nb, nn, M, C, n_val, off, seed = 32, 50, 3, 8, 90, 40, 25, -3.0, 4
    enc, ep = _table(rng, n_val, P, E), _table(rng, M, 1, E)
    n_chunks = -(-M // C)
    idx = rng.integers(0, n_val, (n_chunks, nb, nn))
    steps = np.array([[c * C * 131 + b for b in range(nb)] for c in range(n_chunks)], dtype=np.uint64)
    out, _ = _probe_map(lib, ep, enc, n_val, P, E, idx, steps, C, off, seed)
    acc = np.zeros((2, M))
    for c in range(n_chunks):
        sl = slice(c * C, min(M, c * C + C))
        m = sl.stop - sl.start
        for b in range(nb):
            ed = torch.cat([enc[k * P:(k + 1) * P] for k in idx[c, b]]).contiguous()
            ws = torch.empty(int(lib.dib_mi_probe_workspace_bytes(m, nn * P, E)) // 8 + 2, dtype=torch.float64, device="cuda")
            r = torch.empty((2, m), dtype=torch.float64, device="cuda")
            assert lib.dib_mi_probe_bounds(_p(ep[sl].contiguous()), m, _p(ed), nn * P, E, off, seed, int(steps[c, b]), 0, _p(r[0]),
                                           _p(r[1]), None, _p(ws), _st()) == 0
            acc[:, sl] += r.cpu().numpy()
    acc /= nb
    assert np.abs(out - acc).max() <= 1e-12 * (1 + np.abs(acc).max())


def test_far_apart_gaussians_stay_finite():
    """well separated Gaussians: the literal exp-then-log form gives +-inf / nan, the kernels' log-sum-exp stays finite and
    equal to the LSE restatement"""
    lib = _lib()
    rng = np.random.default_rng(8)
    E, P, n_val = 32, 13, 6
    enc = _table(rng, n_val, P, E, spread=40.0)
    idx = np.array([[0, 1, 2], [3, 4, 5]])
    out, rows, u = _sandwich(lib, enc, n_val, P, E, idx, -3.0, 1, 0)
    e = enc.cpu().numpy().astype(np.float64)
    x = _rows(e, P, idx[0])
    lit = osi.sandwich_rows_literal(x[:, :E], x[:, E:] - 3.0, u[0])
    assert not np.isfinite(lit[1]).all()
    lo, up = osi.sandwich_rows_lse(x[:, :E], x[:, E:] - 3.0, u[0])
    assert np.isfinite(rows).all() and np.abs(rows[1, 0] - up).max() < 1e-8 * (1 + np.abs(up).max())
    ep = _table(rng, 10, 1, E, spread=40.0)
    pm, _ = _probe_map(lib, ep, enc, n_val, P, E, idx[None], np.zeros((1, 2), np.uint64), 10, -3.0, 3)
    assert np.isfinite(pm).all()


def test_notebook_batch_size_on_a_subset_of_probes():
    """512 neighbourhoods x 50 particles = 25 600 data rows per batch (the notebook's probe-grid batch), 24 probes, 2 batches"""
    lib = _lib()
    rng = np.random.default_rng(12)
    E, P, nb, nn, M, n_val = 32, 50, 2, 512, 24, 600
    enc, ep = _table(rng, n_val, P, E), _table(rng, M, 1, E)
    idx = rng.integers(0, n_val, (1, nb, nn))
    steps = np.array([[17, 18]], dtype=np.uint64)
    out, u = _probe_map(lib, ep, enc, n_val, P, E, idx, steps, M, -3.0, 6)
    e, pe = enc.cpu().numpy().astype(np.float64), ep.cpu().numpy().astype(np.float64)
    ref = np.zeros((2, M))
    for b in range(nb):
        x = _rows(e, P, idx[0, b])
        for s in range(0, M, 8):   # 8 probes at a time: 8 x 25 600 x 32 float64 terms
            lo, up = osi.probe_rows_lse(pe[s:s + 8, :E], pe[s:s + 8, E:] - 3.0, u[0, b, s:s + 8], x[:, :E], x[:, E:] - 3.0)
            ref[0, s:s + 8] += lo
            ref[1, s:s + 8] += up
    ref /= nb
    assert np.abs(out - ref).max() < 1e-8 * (1 + np.abs(ref).max())


def test_replay_is_bit_identical_and_bad_arguments_are_refused():
    lib = _lib()
    rng = np.random.default_rng(2)
    E, P, n_val = 32, 50, 30
    enc, ep = _table(rng, n_val, P, E), _table(rng, 150, 1, E)
    idx = rng.integers(0, n_val, (16, 32))
    a = _sandwich(lib, enc, n_val, P, E, idx, -3.0, 9, 3)
    b = _sandwich(lib, enc, n_val, P, E, idx, -3.0, 9, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    pidx = rng.integers(0, n_val, (2, 3, 40))
    steps = np.arange(6, dtype=np.uint64).reshape(2, 3)
    p1 = _probe_map(lib, ep, enc, n_val, P, E, pidx, steps, 100, -3.0, 1)
    p2 = _probe_map(lib, ep, enc, n_val, P, E, pidx, steps, 100, -3.0, 1)
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])
    # envelope and argument checks (no launch)
    assert lib.dib_mi_sandwich_batched_workspace_bytes(n_val, P, 30, 1, 2) < 0          # E % 4 != 0
    assert lib.dib_mi_sandwich_batched_workspace_bytes(n_val, P, 260, 1, 2) < 0         # E > 256
    assert lib.dib_mi_sandwich_batched_workspace_bytes(n_val, 1, 32, 1, 1) < 0          # one row: no leave-one-out
    assert lib.dib_mi_probe_map_workspace_bytes(0, 100, n_val, P, E, 1, 1) < 0
    assert lib.dib_mi_probe_map_workspace_bytes(10 ** 6, 1, n_val, P, E, 16, 1) < 0     # more than 65 535 (chunk, batch) groups
    z = ctypes.c_void_p(0)
    assert lib.dib_mi_sandwich_batched(z, n_val, P, E, z, 1, 2, -3.0, 0, 0, z, z, z, z, z, z, _st()) < 0
    assert lib.dib_mi_probe_map(z, 10, 10, z, n_val, P, E, z, 1, 1, -3.0, 0, z, z, z, z, z, _st()) < 0


def _model(E=32, seed=0):
    import dib_amd
    m = dib_amd.SetTransformerDIB(bottleneck_dimension=E, ff_arch_per_block=(64, E), number_attention_blocks=1,
                                  number_heads_per_mha=2, init_seed=seed, noise_seed=3)
    return m


def _val(rng, n, P):
    from dib_amd.set_transformer import convert_to_per_particle_feature_set
    return np.stack([convert_to_per_particle_feature_set(rng.standard_normal((P + 3, 2)) * 1.3, rng.integers(1, 3, P + 3), P)
                     for _ in range(n)]).astype(np.float32)


def test_model_methods_refuse_bad_input():
    m = _model()
    rng = np.random.default_rng(0)
    xv = _val(rng, 6, 10)
    with pytest.raises(ValueError):
        m.information_bounds(xv[:, :, :5])
    with pytest.raises(ValueError):
        m.sandwich_bounds_batched(m._val_table(xv), np.array([[0, 6]]))
    with pytest.raises(ValueError):
        m.information_maps(np.zeros((4, 2)), xv, number_probes_to_eval_at_a_time=0)
    with pytest.raises(ValueError):
        m.fit(xv, np.zeros(6), number_training_steps=2, track_information=True)


def test_encodings_do_not_depend_on_how_many_particles_are_encoded_with_them():
    """the encoder GEMM picks its tile shape by row count: a particle's encoding is the same bits alone, in a chunk of 100 and
    among 25 600 - which is what lets information_maps (probes and validation set encoded once) match information_map
    (probes per chunk, data per batch) to 1e-10"""
    m = _model()
    rng = np.random.default_rng(1)
    x = _val(rng, 512, 50).reshape(-1, 12)
    full = m.particle_encoder(x).cpu().numpy()
    for n in (1, 7, 100, 1000):
        assert np.array_equal(m.particle_encoder(x[:n]).cpu().numpy(), full[:n]), n


def test_information_maps_equal_information_map():
    m = _model(seed=4)
    rng = np.random.default_rng(4)
    xv = _val(rng, 30, 10)
    from dib_amd.set_transformer import notebook_probe_grid
    pos = notebook_probe_grid(3.0, 9)
    kw = dict(num_eval_batches=3, eval_batch_size_probe_grid=8, number_probes_to_eval_at_a_time=20, seed=7)
    grids = m.information_maps(pos, xv, (0, 1), **kw)
    assert grids.shape == (2, 81, 2)
    for t in (0, 1):
        ref = m.information_map(pos, t, xv, **kw)
        assert np.abs(grids[t] - ref).max() <= 1e-10 * (1 + np.abs(ref).max()), t
    assert (grids[..., 0] <= np.log(8 * 10 + 1) + 1e-9).all()


def test_information_bounds_match_the_oracle_on_the_model_encodings():
    m = _model(seed=5)
    rng = np.random.default_rng(5)
    xv = _val(rng, 20, 10)
    lo, up = m.information_bounds(xv, eval_batch_size=4, num_eval_batches=3, seed=21, step=2)
    enc = m.particle_encoder(xv.reshape(-1, 12)).cpu().numpy().astype(np.float64)
    draw = np.random.default_rng(21)
    idx = np.stack([draw.choice(20, size=4) for _ in range(3)])
    ref = []
    for b in range(3):
        x = _rows(enc, 10, idx[b])
        mus, lvs = x[:, :32], x[:, 32:] - 3.0
        u = mus + np.exp(lvs / 2.0) * _eps(21, 2 + b, 40, 32)
        ref.append(osi.sandwich_bounds(mus, lvs, u))
    ref = np.mean(ref, 0)
    assert abs(lo - ref[0]) < 1e-4 and abs(up - ref[1]) < 1e-4   # u from float32 noise: the oracle's u differs by ~1e-7
    assert lo <= up + 1e-12 and lo <= np.log(40) + 1e-9


def _fit_args(rng):
    xtr = _val(rng, 40, 10)
    ytr = (xtr[:, :, 0].mean(1) > 0).astype(np.float32)
    return xtr, ytr


def test_tracked_fit_trains_exactly_like_the_untracked_fit():
    rng = np.random.default_rng(9)
    xtr, ytr = _fit_args(rng)
    kw = dict(number_training_steps=24, learning_rate=1e-3, batch_size=8, particle_features_val=xtr[:12], loci_val=ytr[:12],
              eval_every=4)
    a, b = _model(seed=1), _model(seed=1)
    ha = a.fit(xtr, ytr, **kw)
    hb = b.fit(xtr, ytr, track_information=True, eval_start=0, eval_grid_mi_every=8, particle_positions_probe=np.zeros((5, 2)),
               num_eval_batches=2, eval_batch_size=4, eval_batch_size_probe_grid=6, **kw)
    assert torch.equal(a.params, b.params) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.t_dev, b.t_dev)
    for k in ("bce_series_val", "acc_series_val", "bce_series_train", "eval_steps"):
        assert ha[k] == hb[k], k
    assert "info_bounds" not in ha and len(hb["info_bounds"]) == 6


def test_tracked_schedule_and_outdir_files(tmp_path):
    rng = np.random.default_rng(10)
    xtr, ytr = _fit_args(rng)
    m = _model(seed=2)
    from dib_amd.set_transformer import information_plane, notebook_probe_grid, save_information_map, save_information_plane
    pos = notebook_probe_grid(3.0, 6)
    h = m.fit(xtr, ytr, number_training_steps=40, learning_rate=1e-3, batch_size=8, particle_features_val=xtr[:12],
              loci_val=ytr[:12], eval_every=4, track_information=True, eval_start=10, eval_grid_mi_every=8,
              particle_positions_probe=pos, num_eval_batches=2, eval_batch_size=4, eval_batch_size_probe_grid=6, info_seed=3,
              outdir=str(tmp_path))
    assert h["info_eval_steps"] == [12, 16, 20, 24, 28, 32, 36]
    assert sorted(h["information_maps"]) == [16, 24, 32]
    ib = np.asarray(h["info_bounds"])
    assert ib.shape == (7, 2) and (ib[:, 0] <= ib[:, 1] + 1e-9).all() and (ib[:, 0] <= 10 * np.log(4 * 10) + 1e-6).all()
    for step, g in h["information_maps"].items():
        assert g.shape == (2, 36, 2) and (g[..., 0] <= np.log(6 * 10 + 1) + 1e-9).all() and (g[..., 0] <= g[..., 1] + 1e-9).all()
        for t in (0, 1):
            f = np.load(tmp_path / f"info_bounds_grid_{step}_type{t}.npy")
            assert f.shape == (6, 6, 2) and np.array_equal(f, g[t].reshape(6, 6, 2))
    hist = np.load(tmp_path / "history.npz")
    assert np.array_equal(hist["info_bounds"], np.float32(h["info_bounds"]) / np.log(2))
    assert np.array_equal(hist["validation_bce"], np.float32(h["bce_series_val"]) / np.log(2))
    ip = information_plane(h)
    assert ip["info_in"].shape == (7,) and ip["info_out"].shape == (7,) and ip["acc"].shape == (7,)
    save_information_plane(h, str(tmp_path / "infoplane.png"))
    save_information_map(h["information_maps"][16], str(tmp_path / "infomap_16.svg"))
    assert (tmp_path / "infoplane.png").stat().st_size > 0 and (tmp_path / "infomap_16.svg").stat().st_size > 0
