"""The kernels of include/dib_ensemble.h alone, R = 3 replicas with a seed and a beta each, F = 3 features: against a float64
restatement at the tolerances tests/test_gpu_parity.py applies to the same quantities on its grouped_gemm path (u 2e-4 (1 + max),
KL 1e-3 nats, task loss 2e-4 (1 + |task|), accuracy 1e-6; dL/dpred is an element-wise function of the prediction and takes the
activation tolerance, dL/d(enc) the gradient tolerance 3e-4 (1 + max) of g_u), replica r of the R = 3 launch against an R = 1
launch bit for bit, a second launch bit for bit, the forward against a single engine's u bit for bit, sentinels behind every
output, and every refusal.  rows are distinct dataset rows with gaps, in no order: a kernel that keyed the noise or gathered
the labels by batch position fails."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as orc
from _helpers import dispatch_path, spec_kwargs

pytestmark = pytest.mark.gpu

R, F, NROWS = 3, 3, 5000
SEEDS = [11, 0x1234567890ABCDEF, 7]
BETAS = [0.37, 1e-3, 2.5]
STEP = 5
SENT = 1234.5
PAD = 64
UNSUPPORTED, E_ARG = -4, -1


def _lib():
    from dib_amd import _lib as L
    return L.load_library()


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else ctypes.c_void_p(0)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda:0", dtype=dtype)


def _out(n):
    """an output of n floats, sentinel-filled, with PAD sentinel floats behind it"""
    return torch.full((n + PAD,), SENT, dtype=torch.float32, device="cuda:0")


def _untouched(t, n):
    return bool((t[n:] == SENT).all())


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(NROWS // 3)[:n] * 3 + r for r in range(R)]).astype(np.int32)   # gaps, a row set per replica


def _ws(lib, r, E, n):
    need = lib.dib_ens_workspace_bytes(r, F, E, n)
    assert need > 0 and need % 4 == 0
    return torch.zeros(need // 4, dtype=torch.float32, device="cuda:0")


def _seeds_dev(seeds):
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device="cuda:0")


def _fwd(lib, enc, rows, seeds, E, n, deterministic=0):
    r = enc.shape[0]
    u, kl, sd, ws = _out(r * n * F * E), _out(r * F), _seeds_dev(seeds), _ws(lib, r, E, n)   # (alive until the synchronize)
    rc = lib.dib_ens_reparam_kl_fwd(_p(enc), _p(rows), _p(sd), STEP, deterministic, r, F, E, n, _p(u), _p(kl), _p(ws), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return u, kl


def _bwd(lib, enc, gu, u, betas, inv_b, E, n):
    r = enc.shape[0]
    d, bd = _out(r * F * n * 2 * E), _dev(np.float32(betas))
    rc = lib.dib_ens_reparam_kl_bwd(_p(enc), _p(gu), _p(u), _p(bd), inv_b, r, F, E, n, _p(d), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("n", [1, 17, 130])
@pytest.mark.parametrize("E", [8, 6, 32])
def test_reparam_forward_and_backward(E, n):
    """E = 8: 128 rows per workgroup (130 crosses it), E = 32: 32 rows (130 leaves a ragged last workgroup), E = 6: the scalar
    tail of the last quad"""
    lib = _lib()
    rng = np.random.default_rng(100 * E + n)
    mu = np.clip(rng.standard_normal((R, F, n, E)), -3, 3)
    lv = rng.uniform(-2.0, 0.0, (R, F, n, E))
    enc_h = np.concatenate([mu, lv], -1).astype(np.float32)
    rows_h = _rows(n, n)
    enc, rows = _dev(enc_h), _dev(rows_h, torch.int32)
    u, kl = _fwd(lib, enc, rows, SEEDS, E, n)
    nu = R * n * F * E
    assert _untouched(u, nu) and _untouched(kl, R * F), "wrote behind an output"
    uh = u[:nu].cpu().numpy().reshape(R, n, F, E).astype(np.float64)
    klh = kl[:R * F].cpu().numpy().reshape(R, F)
    mu64, lv64 = enc_h[..., :E].astype(np.float64), enc_h[..., E:].astype(np.float64)   # [R, F, n, E]
    for r in range(R):
        eps = orc.philox_normal_all(SEEDS[r], STEP, rows_h[r], F, E)                     # [n, F, E], the replica's own key
        m, l = mu64[r].transpose(1, 0, 2), lv64[r].transpose(1, 0, 2)                    # [n, F, E]
        # the noise the sample implies.  |mu| <= 3 and |eps| < 5.5 bound |u| < 8.5, so the rounding of u = fl(mu + fl(sigma eps))
        # is below 2^-24 * 8.5 * 1.1 = 5.6e-7; sigma >= exp(-1) turns it into 1.6e-6 of eps, on top of the 1e-5 the device's
        # float32 Box-Muller is held to (test_eps_matches_oracle_and_host_ref)
        implied = (uh[r] - m) * np.exp(-l / 2.0)
        assert np.abs(implied - eps).max() < 1e-5 + 1.6e-6, (r, np.abs(implied - eps).max())
        ref_u = m + np.exp(l / 2.0) * eps
        assert np.abs(uh[r] - ref_u).max() <= 2e-4 * (1.0 + np.abs(ref_u).max())
        ref_kl = np.sum(0.5 * (m * m + np.exp(l) - l - 1.0), axis=(0, 2))                # [F] sums over the batch
        assert np.abs(klh[r] / n - ref_kl / n).max() < 1e-3, (r, klh[r] / n, ref_kl / n)
    # a second identical launch, and an R = 1 launch of every replica: the same bits
    u2, kl2 = _fwd(lib, enc, rows, SEEDS, E, n)
    assert torch.equal(u, u2) and torch.equal(kl, kl2)
    for r in range(R):
        u1, kl1 = _fwd(lib, enc[r:r + 1].contiguous(), rows[r:r + 1].contiguous(), SEEDS[r:r + 1], E, n)
        assert torch.equal(u1[:n * F * E], u[r * n * F * E:(r + 1) * n * F * E]), r
        assert torch.equal(kl1[:F], kl[r * F:(r + 1) * F]), r
    # deterministic: u = mu
    ud, _ = _fwd(lib, enc, rows, SEEDS, E, n, deterministic=1)
    assert np.array_equal(ud[:nu].cpu().numpy().reshape(R, n, F, E), enc_h[..., :E].transpose(0, 2, 1, 3))

    # ---- backward ----
    inv_b = 1.0 / (n + 3)
    gu_h = (rng.standard_normal((R, n, F * E)) / n).astype(np.float32)
    gu = _dev(gu_h)
    d = _bwd(lib, enc, gu, u, BETAS, inv_b, E, n)
    nd = R * F * n * 2 * E
    assert _untouched(d, nd)
    dh = d[:nd].cpu().numpy().reshape(R, F, n, 2 * E).astype(np.float64)
    for r in range(R):
        eps = orc.philox_normal_all(SEEDS[r], STEP, rows_h[r], F, E).transpose(1, 0, 2)  # [F, n, E]
        g = gu_h[r].astype(np.float64).reshape(n, F, E).transpose(1, 0, 2)
        dmu = g + BETAS[r] * mu64[r] * inv_b                                             # oracle.backward's two lines
        dlv = g * eps * 0.5 * np.exp(lv64[r] / 2.0) + BETAS[r] * 0.5 * (np.exp(lv64[r]) - 1.0) * inv_b
        ref = np.concatenate([dmu, dlv], -1)
        assert np.abs(dh[r] - ref).max() <= 3e-4 * (1.0 + np.abs(ref).max()), (r, np.abs(dh[r] - ref).max())
    assert torch.equal(d, _bwd(lib, enc, gu, u, BETAS, inv_b, E, n))
    for r in range(R):
        sl = slice(r * n * F * E, (r + 1) * n * F * E)
        d1 = _bwd(lib, enc[r:r + 1].contiguous(), gu[r:r + 1].contiguous(), u[sl].contiguous(), BETAS[r:r + 1], inv_b, E, n)
        assert torch.equal(d1[:F * n * 2 * E], d[r * F * n * 2 * E:(r + 1) * F * n * 2 * E]), r


def _loss(lib, kind_id, pred, y, rows, betas, kl, inv_b, n, out_dim, acc0):
    r = pred.shape[0]
    g = _out(r * n * out_dim)
    acc = torch.full((r * (F + 3) + PAD,), SENT, dtype=torch.float32, device="cuda:0")
    acc[:r * (F + 3)] = acc0
    bd, ws = _dev(np.float32(betas)), _ws(lib, r, 8, n)
    rc = lib.dib_ens_loss(kind_id, _p(pred), out_dim, _p(y), y.stride(0), _p(rows), r, F, n, inv_b, 0, _p(bd), _p(kl), _p(g), _p(acc),
                          _p(ws), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return g, acc


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("out_dim", [1, 3])
@pytest.mark.parametrize("kind", ["bce_logits", "sparse_cce_logits", "mse"])
def test_loss_and_history_sums(kind, out_dim, n):
    """one thread per row, 256 per workgroup: n = 300 is two workgroups per replica, the second ragged"""
    from dib_amd._lib import LOSS_KINDS
    lib = _lib()
    rng = np.random.default_rng(n + out_dim)
    pred_h = rng.standard_normal((R, n, out_dim)).astype(np.float32) * 2
    if kind == "sparse_cce_logits":
        y_h = rng.integers(0, out_dim, (NROWS, 1)).astype(np.float32)
    elif kind == "bce_logits":
        y_h = rng.integers(0, 2, (NROWS, out_dim)).astype(np.float32)
    else:
        y_h = rng.standard_normal((NROWS, out_dim)).astype(np.float32)
    rows_h = _rows(n, 3 * n)
    kl_h = rng.uniform(0.1, 5.0, (R, F)).astype(np.float32) * n
    acc0 = 0.25      # the sums are ADDED to what the accumulator holds
    inv_b = 1.0 / n
    pred, y, rows, kl = _dev(pred_h), _dev(y_h), _dev(rows_h, torch.int32), _dev(kl_h)
    g, acc = _loss(lib, LOSS_KINDS[kind], pred, y, rows, BETAS, kl, inv_b, n, out_dim, acc0)
    ng, na = R * n * out_dim, R * (F + 3)
    assert _untouched(g, ng) and _untouched(acc, na)
    gh, ah = g[:ng].cpu().numpy().reshape(R, n, out_dim), acc[:na].cpu().numpy().reshape(R, F + 3).astype(np.float64) - acc0
    for r in range(R):
        yb = y_h[rows_h[r]]
        task, gref = orc.loss_and_grad(kind, yb, pred_h[r].astype(np.float64))
        assert np.abs(gh[r] - gref).max() <= 2e-4 * (1.0 + np.abs(gref).max()), (r, "dL/dpred")
        kls = kl_h[r].astype(np.float64)
        assert np.abs(ah[r, :F] - kls * inv_b).max() < 1e-3, "KL per feature (nats)"
        total = task + BETAS[r] * kls.sum() / n          # per row: task + beta sum_f KL_f
        assert abs(ah[r, F] / n - total) < 2e-4 * (1 + abs(total)), (r, ah[r, F] / n, total)
        assert ah[r, F + 2] == n
        if kind != "mse":
            assert abs(ah[r, F + 1] / n - orc.accuracy(kind, yb, pred_h[r].astype(np.float64))) < 1e-6
    g2, acc2 = _loss(lib, LOSS_KINDS[kind], pred, y, rows, BETAS, kl, inv_b, n, out_dim, acc0)
    assert torch.equal(g, g2) and torch.equal(acc, acc2)
    for r in range(R):
        g1, a1 = _loss(lib, LOSS_KINDS[kind], pred[r:r + 1].contiguous(), y, rows[r:r + 1].contiguous(), BETAS[r:r + 1],
                       kl[r:r + 1].contiguous(), inv_b, n, out_dim, acc0)
        assert torch.equal(g1[:n * out_dim], g[r * n * out_dim:(r + 1) * n * out_dim]), r
        assert torch.equal(a1[:F + 3], acc[r * (F + 3):(r + 1) * (F + 3)]), r


@pytest.mark.parametrize("d,n_blocks,n", [(1, 5, 17), (2, 3, 130), (30, 1, 33)])
def test_posenc_rows_gathers_every_replica_and_feature(d, n_blocks, n):
    """F d = 3, 6 and 90 input columns (the last: two 64-column tiles, the second ragged); n = 17 and 130 leave a ragged row tile"""
    lib = _lib()
    rng = np.random.default_rng(d + n)
    ld = F * d + 3                                   # a row pitch wider than the matrix
    x_h = rng.standard_normal((NROWS, ld)).astype(np.float32) * 3
    rows_h = _rows(n, d)
    x, rows = _dev(x_h), _dev(rows_h, torch.int32)
    pw = d * n_blocks

    def run(r0, r1):
        out, rr = _out((r1 - r0) * F * n * pw), rows[r0:r1].contiguous()
        assert lib.dib_ens_posenc_rows(_p(x), ld, _p(rr), r1 - r0, F, d, n_blocks, n, _p(out), _st()) == 0
        torch.cuda.synchronize()
        return out

    out = run(0, R)
    tot = R * F * n * pw
    assert _untouched(out, tot)
    got = out[:tot].cpu().numpy().reshape(R, F, n, n_blocks, d)
    for r in range(R):
        v = x_h[rows_h[r], :F * d].reshape(n, F, d).transpose(1, 0, 2).astype(np.float64)      # [F, n, d]
        ref = np.stack([v] + [np.sin(2.0 ** j * v) for j in range(1, n_blocks)], axis=2)       # models.py:22-23, blockwise
        assert np.array_equal(got[r, :, :, 0], v.astype(np.float32)), "the gather is a copy"
        assert np.abs(got[r] - ref).max() < 2e-4 * (1 + np.abs(ref).max())
        assert torch.equal(run(r, r + 1)[:F * n * pw], out[r * F * n * pw:(r + 1) * F * n * pw]), r
    assert torch.equal(out, run(0, R))


def test_forward_reproduces_a_single_engines_u_bit_for_bit():
    """fed a HipEngine's own encoder outputs under the grouped_gemm dispatch with the same seed, step and rows, the ensemble
    forward gives that engine's u and KL sums: they share the body"""
    from dib_amd.engine import HipEngine
    lib = _lib()
    spec = orc.DIBSpec([1, 1, 1], [32, 32], [64], 1, feature_embedding_dimension=8)
    E, B = 8, 130
    rng = np.random.default_rng(0)
    x = rng.standard_normal((NROWS, 3)).astype(np.float32)
    rows_h = _rows(B, 9)[:1]
    with dispatch_path("grouped_gemm"):
        eng = HipEngine(**spec_kwargs(spec), init_seed=3)
        idx = eng.to_device(rows_h[0], dtype=torch.int32)
        eng.forward(eng.to_device(x), idx, 0, B, SEEDS[1], STEP)
        torch.cuda.synchronize()
        enc = eng.enc_out(B).permute(1, 0, 2).contiguous().view(1, F, B, 2 * E)   # [F][B][2E] as the device holds it
        want_u, want_kl = eng.u(B).clone(), eng.step_out(B)[:F].clone()
    u, kl = _fwd(lib, enc, _dev(rows_h, torch.int32), SEEDS[1:2], E, B)
    assert torch.equal(u[:B * F * E].view(B, F * E), want_u)
    # (130 rows are two workgroup partials per feature; the engine adds them in a tree, the ensemble in order: a few ulp at most)
    assert np.abs((kl[:F] - want_kl).cpu().numpy()).max() <= 4 * 2.0 ** -24 * float(want_kl.abs().max())


def test_refusals_launch_nothing_and_write_nothing():
    lib = _lib()
    assert lib.dib_ens_supported(64, 1023, 1024, 2048, 16, 3) == 1 and lib.dib_ens_supported(1, 1, 1, 1, 1, 0) == 1
    t = torch.full((4096,), SENT, dtype=torch.float32, device="cuda:0")
    i = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    s = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    n0 = lib.dib_launch_count()
    bad = [(0, 3, 8, 16, 1, 0), (3, 0, 8, 16, 1, 0), (64, 1024, 8, 16, 1, 0), (3, 3, 0, 16, 1, 0), (3, 3, 1025, 16, 1, 0),
           (3, 3, 8, 0, 1, 0), (3, 3, 8, 2049, 1, 0), (3, 3, 8, 16, 0, 0), (3, 3, 8, 16, 17, 0), (3, 3, 8, 16, 1, 1), (3, 3, 8, 16, 1, 4)]
    for (r, f, e, n, o, k) in bad:
        assert lib.dib_ens_supported(r, f, e, n, o, k) == 0, (r, f, e, n, o, k)
        if (o, k) == (1, 0):   # a shape refusal: every entry answers it
            assert lib.dib_ens_workspace_bytes(r, f, e, n) == UNSUPPORTED
            assert lib.dib_ens_reparam_kl_fwd(_p(t), _p(i), _p(s), 0, 0, r, f, e, n, _p(t), _p(t), _p(t), _st()) == UNSUPPORTED
            assert lib.dib_ens_reparam_kl_bwd(_p(t), _p(t), _p(t), _p(t), 1.0, r, f, e, n, _p(t), _st()) == UNSUPPORTED
            if 1 <= e <= 1024:
                assert lib.dib_ens_posenc_rows(_p(t), 8, _p(i), r, f, 1, 5, n, _p(t), _st()) == UNSUPPORTED
        if 1 <= e <= 1024:
            assert lib.dib_ens_loss(k, _p(t), o, _p(t), 16, _p(i), r, f, n, 1.0, 0, _p(t), _p(t), _p(t), _p(t), _p(t), _st()) == UNSUPPORTED
    assert lib.dib_ens_posenc_rows(_p(t), 8, _p(i), 3, 3, 0, 5, 16, _p(t), _st()) == UNSUPPORTED
    assert lib.dib_ens_posenc_rows(_p(t), 8, _p(i), 3, 3, 1, 33, 16, _p(t), _st()) == UNSUPPORTED
    # bad pointers and sizes
    assert lib.dib_ens_reparam_kl_fwd(None, _p(i), _p(s), 0, 0, 3, 3, 8, 16, _p(t), _p(t), _p(t), _st()) == E_ARG
    assert lib.dib_ens_reparam_kl_fwd(_p(t), _p(i), _p(s), 0, 0, 3, 3, 8, 16, _p(t), _p(t), None, _st()) == E_ARG
    assert lib.dib_ens_reparam_kl_bwd(_p(t), _p(t), _p(t), None, 1.0, 3, 3, 8, 16, _p(t), _st()) == E_ARG
    assert lib.dib_ens_loss(0, _p(t), 3, _p(t), 2, _p(i), 3, 3, 16, 1.0, 0, _p(t), _p(t), _p(t), _p(t), _p(t), _st()) == E_ARG   # ldy < out_dim
    assert lib.dib_ens_loss(0, _p(t), 1, _p(t), 1, _p(i), 3, 3, 16, 1.0, 99, _p(t), _p(t), _p(t), _p(t), _p(t), _st()) == E_ARG  # activation
    assert lib.dib_ens_posenc_rows(_p(t), 2, _p(i), 3, 3, 1, 5, 16, _p(t), _st()) == E_ARG                                      # ldx < F d
    assert lib.dib_ens_posenc_rows(_p(t), 8, None, 3, 3, 1, 5, 16, _p(t), _st()) == E_ARG
    torch.cuda.synchronize()
    assert lib.dib_launch_count() == n0, "a refusal launched something"
    assert bool((t == SENT).all()), "a refusal wrote something"
