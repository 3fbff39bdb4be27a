"""MI-bound characterization on the device (include/dib_mi_channel.h, csrc/dib_mi_channel.h, dib_amd.mi_characterization,
utils.estimate_mi_sandwich_bounds_from_parameters):
  - dib_mi_monte_carlo against the float64 oracle (tests/_oracle_mi_characterization.py) on the device's own samples, and the
    samples against the Philox reference, across the envelope (E, rows, sample tiles, tables, groups, logvars, duplicates, row
    splits), with guard regions around every output; far-apart Gaussians; replay, split calls and refusals;
  - the parameter form of the sandwich bounds against the dib_mi_sandwich_rows loop, the oracle and the closed-form anchors;
  - the Monte-Carlo terms of src_idx = arange(N) against the lower rows of the batched sandwich launch (one shared arithmetic);
  - a known answer (k independent bits through unit Gaussian noise) within 5 standard errors of the ORACLE's terms;
  - characterize: stacked launch = per-scale calls, launch count independent of scales and runs, the notebook's layout."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle_mi_characterization as omc  # noqa: E402
import _oracle_st_information as osi  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 37   # doubles of sentinel before and after every output


def _lib():
    from dib_amd import _lib
    return _lib.load_library()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n):
    """(whole buffer, the n payload doubles inside it): NaN payload between sentinel guards"""
    buf = torch.full((n + 2 * GUARD,), -777.25, dtype=torch.float64, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:GUARD] == -777.25).all() and (b[GUARD + n:] == -777.25).all()


def _mc(lib, tables, group_table, src, seed, step0, want_terms=True, want_u=True):
    """one dib_mi_monte_carlo call on host arrays -> (means [G], terms [G, ns], u [G, ns, E]) with the guards checked"""
    T, N, E2 = tables.shape
    E = E2 // 2
    G, ns = src.shape
    need = int(lib.dib_mi_monte_carlo_workspace_bytes(T, N, E, G, ns))
    assert need > 0, need
    ws = torch.empty(need // 8 + 2, dtype=torch.float64, device="cuda")
    tab_d = torch.tensor(tables, dtype=torch.float32, device="cuda")
    gt_d = torch.tensor(np.asarray(group_table), dtype=torch.int32, device="cuda")
    src_d = torch.tensor(src, dtype=torch.int32, device="cuda")
    mb, means = _guarded(G)
    tb, terms = _guarded(G * ns)
    ub, u = _guarded(G * ns * E)
    rc = lib.dib_mi_monte_carlo(_p(tab_d), T, N, E, _p(gt_d), _p(src_d), G, ns, seed, step0, _p(means),
                                _p(terms) if want_terms else None, _p(u) if want_u else None, _p(ws), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _guards_intact(mb, G) and _guards_intact(tb, G * ns) and _guards_intact(ub, G * ns * E)
    if not want_terms:
        assert torch.isnan(terms).all()
    if not want_u:
        assert torch.isnan(u).all()
    return means.cpu().numpy(), terms.cpu().numpy().reshape(G, ns), u.cpu().numpy().reshape(G, ns, E)


def _random_tables(rng, T, N, E, spread=1.5):
    """[T, N, 2E] float32 (mu | logvar) with random per-row logvars and a few repeated rows"""
    mu = rng.standard_normal((T, N, E)) * spread
    lv = rng.standard_normal((T, N, E)) * 0.4 - 0.3
    tab = np.concatenate([mu, lv], -1).astype(np.float32)
    tab[:, N - 1] = tab[:, 0]            # the last row repeats the first
    if N > 8:
        tab[:, 5] = tab[:, 3]
        tab[:, 6] = tab[:, 3]
    return tab


ENVELOPE_CASES = [  # E, n_rows, n_samples, n_tables, n_groups      (samples x rows x E <= 1e9 in total)
    (1, 2, 70, 2, 3), (2, 63, 130, 2, 4), (8, 64, 65, 3, 5), (32, 1000, 333, 2, 4), (33, 1024, 200, 2, 3), (64, 1500, 150, 2, 3),
    (32, 1500, 100, 1, 2), (64, 64, 129, 2, 4), (1, 1024, 257, 1, 2), (8, 2, 1, 1, 1)]


@pytest.mark.parametrize("E,N,ns,T,G", ENVELOPE_CASES)
def test_kernel_matches_oracle_across_the_envelope(E, N, ns, T, G):
    """samples = mu_r + sigma_r Philox(seed, step0 + g, sample, 0); per-sample terms and group means against the log-sum-exp
    restatement on the device's samples; sample counts that are not multiples of the 64-sample tile, several tables, several
    groups per table, random logvars, repeated rows; 1 000+ rows with few samples take the row-split path"""
    lib = _lib()
    rng = np.random.default_rng(1000 * E + N)
    tables = _random_tables(rng, T, N, E)
    group_table = rng.integers(0, T, G)
    group_table[0] = T - 1
    src = rng.integers(0, N, (G, ns))
    src[0, : min(ns, 3)] = N - 1          # samples drawn from a repeated row
    seed, step0 = 2 ** 41 + 5, 2 ** 32 - 2   # the step wraps inside the call
    means, terms, u = _mc(lib, tables, group_table, src, seed, step0)
    t64 = tables.astype(np.float64)
    for g in range(G):
        mus, lvs = t64[group_table[g], :, :E], t64[group_table[g], :, E:]
        ref_u = omc.sample_u(mus, lvs, src[g], seed, (step0 + g) & 0xFFFFFFFF)
        assert np.abs(u[g] - ref_u).max() < 1e-5 * (1 + np.abs(ref_u).max())
        ref = omc.mc_terms_lse(mus, lvs, u[g], src[g])
        tol = 1e-8 * (1 + np.abs(ref).max())
        assert np.abs(terms[g] - ref).max() < tol, g
        assert abs(means[g] - ref.mean()) < tol, g
        assert (terms[g] <= np.log(N) + 1e-9).all()
    m2, t2, u2 = _mc(lib, tables, group_table, src, seed, step0, want_terms=False, want_u=False)
    assert (m2 == means).all()


def test_far_apart_gaussians_stay_finite():
    """centres 1e3 apart: the raw-exp form underflows to 0 / 0; here every term is log(n_rows / multiplicity of the source row)"""
    lib = _lib()
    E, N, ns = 8, 70, 500
    centre = np.arange(N)
    centre[10:20] = centre[0:10]          # rows 0..9 are in the table twice, 20..29 three times
    centre[30:40] = centre[20:30]
    centre[40:50] = centre[20:30]
    mult = np.array([(centre == c).sum() for c in centre])
    mus = np.zeros((N, E))
    mus[:, 0] = centre * 1000.0
    mus[:, 3] = -centre * 2000.0
    tables = np.concatenate([mus, np.zeros((N, E))], -1)[None].astype(np.float32)
    src = np.random.default_rng(0).integers(0, N, (2, ns))
    means, terms, _ = _mc(lib, tables, [0, 0], src, 9, 0)
    for g in range(2):
        ref = np.log(N / mult[src[g]])
        assert np.isfinite(terms[g]).all() and np.abs(terms[g] - ref).max() <= 1e-9
        assert abs(means[g] - ref.mean()) <= 1e-9


def test_replay_split_calls_and_refusals():
    lib = _lib()
    rng = np.random.default_rng(12)
    E, N, ns, T, G = 32, 600, 90, 2, 5
    tables = _random_tables(rng, T, N, E)
    gt = rng.integers(0, T, G)
    src = rng.integers(0, N, (G, ns))
    seed, step0 = 31, 1000
    a = _mc(lib, tables, gt, src, seed, step0)
    b = _mc(lib, tables, gt, src, seed, step0)
    for x, y in zip(a, b):
        assert (x == y).all()
    # the groups over two calls, step0 advanced by the groups already done: the same bits
    c0 = _mc(lib, tables, gt[:2], src[:2], seed, step0)
    c1 = _mc(lib, tables, gt[2:], src[2:], seed, step0 + 2)
    for x, y0, y1 in zip(a, c0, c1):
        assert (x == np.concatenate([y0, y1])).all()
    # an index outside the tables is not dereferenced: NaN for what it touches, the other groups unchanged
    bad_src = src.copy()
    bad_src[1, 7] = N
    bad_gt = gt.copy()
    bad_gt[3] = T
    d = _mc(lib, tables, bad_gt, bad_src, seed, step0)
    assert np.isnan(d[1][1, 7]) and np.isnan(d[0][1]) and np.isnan(d[0][3]) and np.isnan(d[1][3]).all()
    assert (d[0][[0, 2, 4]] == a[0][[0, 2, 4]]).all() and (np.delete(d[1][1], 7) == np.delete(a[1][1], 7)).all()
    # refusals: the code, and nothing launched
    ws = torch.empty(int(lib.dib_mi_monte_carlo_workspace_bytes(T, N, E, G, ns)) // 8 + 4, dtype=torch.float64, device="cuda")
    tab_d = torch.tensor(tables, device="cuda")
    gt_d = torch.tensor(gt, dtype=torch.int32, device="cuda")
    src_d = torch.tensor(src, dtype=torch.int32, device="cuda")
    out = torch.zeros(G, dtype=torch.float64, device="cuda")
    n0 = lib.dib_launch_count()

    def call(T=T, N=N, E=E, G=G, ns=ns, tab=tab_d, gtp=gt_d, srcp=src_d, outp=out, wsp=_p(ws)):
        return lib.dib_mi_monte_carlo(_p(tab), T, N, E, _p(gtp), _p(srcp), G, ns, seed, step0, _p(outp), None, None, wsp, _st())
    ARG, UNSUPPORTED = -1, -4
    for kw in (dict(E=0), dict(N=0), dict(G=0), dict(ns=0), dict(T=0), dict(ns=-3), dict(tab=None), dict(gtp=None), dict(srcp=None),
               dict(outp=None), dict(wsp=ctypes.c_void_p(0)), dict(wsp=ctypes.c_void_p(ws.data_ptr() + 8))):
        assert call(**kw) == ARG, kw
    for kw in (dict(E=65), dict(N=1), dict(N=65537), dict(ns=2 ** 20 + 1), dict(G=65536), dict(T=65537)):
        assert call(**kw) == UNSUPPORTED, kw
        args = dict(T=T, N=N, E=E, G=G, ns=ns)
        args.update(kw)
        assert lib.dib_mi_monte_carlo_workspace_bytes(args["T"], args["N"], args["E"], args["G"], args["ns"]) == UNSUPPORTED
    assert lib.dib_mi_monte_carlo_workspace_bytes(T, N, 0, G, ns) == ARG
    assert lib.dib_launch_count() == n0
    assert lib.dib_mi_monte_carlo_workspace_bytes(1, 65536, 64, 1, 2 ** 20) > 0
    assert call() == 0 and lib.dib_launch_count() == n0 + 3
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == a[0]).all()


def test_bounds_from_parameters_equal_the_rows_loop_and_the_oracle():
    from dib_amd import utils
    lib = _lib()
    rng = np.random.default_rng(21)
    N, E, bs, nb, seed = 300, 32, 128, 5, 17
    mus = (rng.standard_normal((N, E)) * 1.2).astype(np.float32)
    lvs = (rng.standard_normal((N, E)) * 0.3 - 0.2).astype(np.float32)
    est = utils.estimate_mi_sandwich_bounds_from_parameters(mus, lvs, evaluation_batch_size=bs, number_evaluation_batches=nb, seed=seed)
    assert est.shape == (nb, 2) and (est[:, 0] <= est[:, 1]).all()
    rows = np.random.default_rng(seed).integers(0, N, (nb, bs))     # the documented draw
    table = torch.tensor(np.concatenate([mus, lvs], -1), device="cuda")
    ws = torch.empty(int(lib.dib_mi_workspace_bytes(bs, E)) // 8 + 2, dtype=torch.float64, device="cuda")
    # the samples the batched kernel draws, for the oracle
    wsb = torch.empty(int(lib.dib_mi_sandwich_batched_workspace_bytes(N, 1, E, nb, bs)) // 8 + 2, dtype=torch.float64, device="cuda")
    ob = torch.empty((2, nb), dtype=torch.float64, device="cuda")
    u = torch.empty((nb, bs, E), dtype=torch.float64, device="cuda")
    idx_d = torch.tensor(rows, dtype=torch.int32, device="cuda")
    assert lib.dib_mi_sandwich_batched(_p(table), N, 1, E, _p(idx_d), nb, bs, 0.0, seed, 0, _p(ob[0]), _p(ob[1]), None, None, _p(u),
                                       _p(wsb), _st()) == 0
    assert (ob.cpu().numpy().T / np.log(2.0) == est).all()
    u = u.cpu().numpy()
    for b in range(nb):
        eb = table[torch.tensor(rows[b], device="cuda")].contiguous()
        r = torch.empty((2, bs), dtype=torch.float64, device="cuda")
        assert lib.dib_mi_sandwich_rows(_p(eb), bs, E, seed, b, 0, _p(r[0]), _p(r[1]), _p(ws), _st()) == 0
        loop = r.cpu().numpy().mean(axis=1) / np.log(2.0)
        assert np.abs(est[b] - loop).max() <= 1e-12 * (1 + np.abs(loop).max())
        lo, up = osi.sandwich_rows_lse(mus[rows[b]].astype(np.float64), lvs[rows[b]].astype(np.float64), u[b])
        ref = np.array([lo.mean(), up.mean()]) / np.log(2.0)
        assert np.abs(est[b] - ref).max() < 1e-8 * (1 + np.abs(ref).max())


def test_monte_carlo_terms_are_the_sandwich_lower_rows():
    """The identity that makes the tiled families one family (csrc/dib_gauss_lse.h): with src_idx = arange(N) and one group,
    dib_mi_monte_carlo's sample i is drawn from row i with the noise of dib_mi_sandwich_batched's batch arange(N) (P = 1, offset
    0, same seed and step), so u_out is bit-equal and term_i = l_ii - (LSE_j l_ij - log N) = lower_i.
    One table of N = 70 rows: the E <= 32 instantiations, a padded block of dimensions in the Monte-Carlo kernel (it stages 8)
    and two staged blocks of rows (64 + 6: waves 0, 1 take a pair, waves 2, 3 the odd tail row).  E = 4, not 5:
    dib_mi_sandwich_batched takes multiples of 4 only (asserted below), and 4 is the nearest size both entry points accept.
    Tolerance (derived, not measured): the two sides differ in the float64 rounding of a 70-term log-sum-exp (the own term inside
    or beside the streaming sum) and of l_ii (folded FMAs or (u - mu) / sigma) - a few ulp of values below 20, < 1e-13; the
    assertion leaves two decades above that.  Observed on an MI355X: 2.7e-15 (profiles/mi_lse_equivalence.txt (C))."""
    lib = _lib()
    N, E, seed, step0 = 70, 4, 31, 9
    assert lib.dib_mi_sandwich_batched_workspace_bytes(N, 1, 5, 1, N) < 0
    rng = np.random.default_rng(70)
    mu = 1.5 * rng.standard_normal((N, E))
    lv = rng.uniform(-1.0, 0.5, (N, E))
    table = np.concatenate([mu, lv], -1).astype(np.float32)
    idx = np.arange(N)
    _, terms, u_mc = _mc(lib, table[None], [0], idx[None], seed, step0)
    tab_d = torch.tensor(table, device="cuda")
    idx_d = torch.tensor(idx, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.dib_mi_sandwich_batched_workspace_bytes(N, 1, E, 1, N)) // 8 + 2, dtype=torch.float64, device="cuda")
    ob = torch.empty((2, 1), dtype=torch.float64, device="cuda")
    rows = torch.empty((2, N), dtype=torch.float64, device="cuda")
    u_sb = torch.empty((N, E), dtype=torch.float64, device="cuda")
    assert lib.dib_mi_sandwich_batched(_p(tab_d), N, 1, E, _p(idx_d), 1, N, 0.0, seed, step0, _p(ob[0]), _p(ob[1]), _p(rows[0]),
                                       _p(rows[1]), _p(u_sb), _p(ws), _st()) == 0
    assert np.array_equal(u_sb.cpu().numpy(), u_mc[0])
    diff = np.abs(rows[0].cpu().numpy() - terms[0]).max()
    print(f"Monte-Carlo terms vs sandwich lower rows, N = {N}, E = {E}: max |difference| = {diff:.3e} nats")
    assert diff <= 1e-11


def test_bounds_from_parameters_reproduce_the_separation_zero_anchors():
    """all conditionals equal: lower = 0 and upper = log2(n / (n - 1)) in every batch; and the Monte-Carlo value is 0"""
    from dib_amd import mi_characterization as mic
    from dib_amd import utils
    x = mic.VARIABLES[2].sample(np.random.default_rng(0), 256)
    mus, lvs = mic.gaussian_channel(x, 0.0, embedding_dimension=32)
    for bs in (64, 256):
        est = utils.estimate_mi_sandwich_bounds_from_parameters(mus, lvs, evaluation_batch_size=bs, number_evaluation_batches=6, seed=1)
        assert np.abs(est[:, 0]).max() <= 1e-12 and np.abs(est[:, 1] - np.log2(bs / (bs - 1.0))).max() <= 1e-12
    mean, runs = mic.monte_carlo_information(mus, lvs, mc_sample_size=1000, number_monte_carlo_runs=3, seed=2)
    assert abs(mean) <= 1e-12 and np.abs(runs).max() <= 1e-12


@pytest.mark.parametrize("k,d", [(1, 1.0), (2, 1.0), (6, 3.0), (6, 0.75)])
def test_known_answer_on_the_device(k, d):
    """balanced 64-row {+-1}^k dataset at separation d, unit variances, 200 000 samples in one launch: the device's mean within 5
    standard errors of k I_1(d), the standard error from the ORACLE's per-sample terms on the same samples"""
    lib = _lib()
    E, N, ns = 8, 64, 200_000
    mus = np.concatenate([omc.balanced_signs(k, N) * d, np.zeros((N, E - k))], -1)
    tables = np.concatenate([mus, np.zeros((N, E))], -1)[None]
    src = np.random.default_rng([5, k]).integers(0, N, (1, ns))
    means, _, u = _mc(lib, tables, [0], src, 23, k, want_terms=False)
    ref = omc.mc_terms_lse(mus, np.zeros((N, E)), u[0], src[0]) / np.log(2.0)
    truth = k * omc.one_bit_information(d)
    se = ref.std(ddof=1) / np.sqrt(ns)
    value = means[0] / np.log(2.0)
    print(f"k={k} d={d}: truth {truth:.6f} device {value:.6f} oracle {ref.mean():.6f} se {se:.6f} z {(value - truth) / se:+.2f}")
    assert abs(value - ref.mean()) < 1e-8 * (1 + np.abs(ref).max())
    assert abs(value - truth) <= 5.0 * se


def test_characterize_on_a_small_sweep():
    from dib_amd import mi_characterization as mic
    lib = _lib()
    rng = np.random.default_rng(3)
    x = mic.VARIABLES[1].sample(rng, 128)
    scales = np.linspace(0.0, 2.0, 5)
    kw = dict(evaluation_batch_sizes=(16, 64), number_evaluation_batches=6, embedding_dimension=8, mc_sample_size=300, seed=4)
    n0 = lib.dib_launch_count()
    res = mic.characterize(x, scales, number_monte_carlo_runs=8, **kw)
    big = lib.dib_launch_count() - n0
    n0 = lib.dib_launch_count()
    one = mic.characterize(x, scales[3:4], number_monte_carlo_runs=1, **kw)
    small = lib.dib_launch_count() - n0
    assert big == small == 3 + 2 * 3      # Monte Carlo: prep, terms, combine; per batch size: prep, bounds, combine
    assert res["monte_carlo"].shape == (5,) and res["monte_carlo_runs"].shape == (5, 8)
    assert res["info_bound_estimates"].shape == (2, 5, 6, 2) and res["info_bound_stats"].shape == (2, 5, 4)
    assert one["info_bound_estimates"].shape == (2, 1, 6, 2)
    e = res["info_bound_estimates"]
    assert np.array_equal(res["info_bound_stats"], np.stack([e[..., 0].mean(-1), e[..., 0].std(-1), e[..., 1].mean(-1),
                                                             e[..., 1].std(-1)], -1))
    # the stacked launch against one call per scale, bit for bit
    for s, scale in enumerate(scales):
        mus, lvs = mic.gaussian_channel(x, scale, 8)
        mean, runs = mic.monte_carlo_information(mus, lvs, 300, 8, seed=4, group_offset=s * 8)
        assert (runs == res["monte_carlo_runs"][s]).all() and abs(mean - res["monte_carlo"][s]) <= 1e-15 * (1 + abs(mean))
    # the estimate and its bounds behave: 0 at separation 0, rising, below H(X) = 2 bits, lower <= Monte Carlo <= upper on average
    assert abs(res["monte_carlo"][0]) < 1e-12 and (np.diff(res["monte_carlo"]) > 0).all() and res["monte_carlo"][-1] < 2.0
    assert (res["info_bound_stats"][1, :, 0] <= res["info_bound_stats"][1, :, 2]).all()
