"""GPU: the Keras loss and metric family (include/dib_losses.h, csrc/dib_losses.h) from the C ABI up to compile / fit / evaluate.

The float64 comparison.  The reference is tests/_oracle_losses.py in float64 (values by the listed formulas, gradients by
torch.autograd).  The tolerance is NOT taken from the device: the same functions evaluated in float32 on the same inputs measure
what the number format costs, and the device gets FACTOR = 4 times that (fused multiply-add contraction, the device's exp / log /
rsqrt), never less than one float32 ulp of the compared value:
    gradients   bound = max(4 eps_g inv_bg, ulp32(max |g64|)); eps_g = the worst |g32 - g64| / inv_bg over every input of the
                (kind, out_dim) case, g32 scaled by inv_bg and act' in float32 like the kernel does
    partials    a block's sum of <= 256 row values: E = max(sum_rows |l32 - l64|, eps_l) + the worst deviation of a float32 sum
                of the block's l32 from their float64 sum over eleven summation orders; eps_l = the worst |l32 - l64| of a row
                over every input of the case; bound = max(4 E, ulp32(|partial64|))
Counted metrics (0 / 1 per element) are compared through the integer count, which must be exact; the inputs keep an arg-max margin
and a distance from the 0.5 threshold of at least 1e-3, asserted below.  Every case prints device error / bound."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as orc
import _oracle_losses as ol
from _helpers import SPECS, dispatch_path, flat_to_params, params_to_flat, random_params, spec_kwargs

pytestmark = pytest.mark.gpu

FACTOR = 4.0
PAD = 64
F32 = np.float32
NATURAL_METRIC = {"bce_logits": "binary_accuracy", "bce": "binary_accuracy", "mse": "mae", "mae": "mse", "mape": "mae",
                  "msle": "mse", "huber": "mae", "log_cosh": "mse", "poisson": "mse", "kl_divergence": "categorical_accuracy",
                  "cosine_similarity": "mae", "cce_logits": "categorical_accuracy", "cce": "categorical_accuracy",
                  "sparse_cce": "sparse_categorical_accuracy"}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _lib():
    from dib_amd import _lib as L
    return L, L.load_library()


def _desc(kind, metric=None, param=None):
    from dib_amd import losses
    L, _ = _lib()
    return L.LossDesc(losses.KIND_IDS[kind], losses.METRIC_IDS[metric], float(ol.PARAM.get(kind, 0.0) if param is None else param))


def _guarded(n):
    """n floats between two bands of PAD NaNs"""
    return torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device="cuda")


def _bands_intact(buf, n):
    return bool(torch.isnan(buf[:PAD]).all().item()) and bool(torch.isnan(buf[PAD + n:]).all().item())


def _call(desc, p, Y, B, C, inv_bg, act, row_idx=None, row0=0):
    """dib_loss_rows_ex on guarded buffers -> (rc, g [B, C], partial [blocks, 2], guards intact)"""
    _, lib = _lib()
    nblk = (B + 255) // 256
    g, part = _guarded(B * C), _guarded(2 * nblk)
    pd = torch.from_numpy(np.ascontiguousarray(p)).cuda()
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    idx = None if row_idx is None else torch.from_numpy(row_idx.astype(np.int32)).cuda()
    rc = lib.dib_loss_rows_ex(ctypes.byref(desc), _ptr(pd), C, _ptr(Yd), Y.shape[1], _ptr(idx), int(row0), B, float(inv_bg),
                              int(act), _ptr(g[PAD:]), _ptr(part[PAD:]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ok = _bands_intact(g, B * C) and _bands_intact(part, 2 * nblk)
    return rc, g[PAD:PAD + B * C].cpu().numpy().reshape(B, C), part[PAD:PAD + 2 * nblk].cpu().numpy().reshape(nblk, 2), ok


def _ulp(v):
    return float(np.spacing(F32(abs(v)))) if v != 0 else float(np.spacing(F32(0)))


def _sum_rounding(v32):
    """float32's own summation rounding on these values: the worst deviation from their float64 sum over the serial sum forwards,
    backwards, NumPy's pairwise sum and eight seeded orders (np.cumsum accumulates serially in float32)"""
    v = v32.astype(F32)
    exact = float(v.astype(np.float64).sum())
    rng = np.random.default_rng(len(v))
    orders = [v, v[::-1]] + [v[rng.permutation(len(v))] for _ in range(8)]
    sums = [float(np.cumsum(o, dtype=F32)[-1]) for o in orders] + [float(v.sum(dtype=F32))]
    return max(abs(t - exact) for t in sums)


def _block_bound(v32, v64, eps_row):
    """see the module docstring: (float64 partial, bound) of one block's row values"""
    E = max(float(np.abs(v32 - v64).sum()), eps_row) + _sum_rounding(v32)
    tot = float(v64.sum())
    return tot, max(FACTOR * E, _ulp(tot))


def _reference(kind, metric, p, Y, rows, C, inv_bg, act):
    """float64 and float32 evaluations of one call's inputs"""
    param = ol.PARAM.get(kind, 0.0)
    y = Y[rows][:, :1 if kind == "sparse_cce" else C]
    assert ol.margins_ok(metric, p, Y, rows, C), "the inputs must make the counted metric unambiguous"
    l64, g64 = ol.rows_and_grad(kind, y, p, param, torch.float64)
    l32, g32 = ol.rows_and_grad(kind, y, p, param, torch.float32)
    gref = g64 * inv_bg * ol.act_grad_from_output(act, p)
    g32s = (g32.astype(F32) * F32(inv_bg) * ol.act_grad_from_output(act, p, F32)).astype(np.float64)
    return dict(l64=l64, l32=l32, gref=gref, g32s=g32s, m64=ol.metric_rows(metric, y, p),
                m32=ol.metric_rows(metric, y, p, F32).astype(np.float64), inv_bg=inv_bg)


def _check(kind, metric, B, C, act, r, eps, g, part):
    """device results of one call against its reference r under the case's measured roundings eps; the worst error / bound"""
    bound_g = max(FACTOR * eps["g"] * r["inv_bg"], _ulp(float(np.abs(r["gref"]).max())))
    err_g = float(np.abs(g.astype(np.float64) - r["gref"]).max())
    worst = err_g / bound_g
    assert np.isfinite(g).all() and err_g <= bound_g, (kind, B, C, act, "g_pred", err_g, bound_g)
    counted = metric in ("binary_accuracy", "categorical_accuracy", "sparse_categorical_accuracy")
    for blk in range((B + 255) // 256):
        sl = slice(256 * blk, min(256 * blk + 256, B))
        tot, bound = _block_bound(r["l32"][sl], r["l64"][sl], eps["l"])
        err = abs(float(part[blk, 0]) - tot)
        worst = max(worst, err / bound)
        assert err <= bound, (kind, B, C, "loss partial", blk, err, bound)
        if counted:
            scale = C if metric == "binary_accuracy" else 1
            count = int(round(float(r["m64"][sl].sum()) * scale))
            assert abs(float(part[blk, 1]) * scale - count) < 0.25 and int(round(float(part[blk, 1]) * scale)) == count, \
                (kind, metric, blk, float(part[blk, 1]), count)
        elif metric is not None:
            mtot, mbound = _block_bound(r["m32"][sl], r["m64"][sl], eps["m"])
            merr = abs(float(part[blk, 1]) - mtot)
            worst = max(worst, merr / mbound)
            assert merr <= mbound, (kind, metric, blk, float(part[blk, 1]), mtot, mbound)
        else:
            assert float(part[blk, 1]) == 0.0
    return worst


# batch sizes on both sides of the 256-row block; out_dim on both sides of every LANES threshold (1 | 4 | 16 | 64) and of a
# multiple of 64, and wider than one 64-lane pass many times over (1000)
BATCHES = (1, 255, 256, 257, 700)
CASES = [(k, C) for k in ol.CLASS_AXIS for C in (1, 2, 3, 5, 63, 64, 65, 257, 1000)] + \
        [(k, C) for k in ol.ELEMENTWISE for C in (1, 3, 9, 65)]   # 9: the 16-lane instantiation of the element-wise kinds


@pytest.mark.parametrize("kind,C", CASES, ids=[f"{k}-{c}" for k, c in CASES])
def test_envelope_matches_the_float64_helper(kind, C):
    """Every batch size x both addressings of a (kind, out_dim), the output activations in turn.  float32's own rounding is
    measured over ALL of the case's inputs (its worst deviation from float64, the gradients' relative to inv_bg): one row or
    one block is too small a sample of a number format - a single draw can land within a quarter ulp by chance."""
    metric = NATURAL_METRIC[kind]
    desc = _desc(kind, metric)
    calls, n = [], 0
    for B in BATCHES:
        for addressing in ("row_idx", "row0"):
            act = n % 8          # every output activation of include/dib_hip.h (7: dib_st.h's LeakyReLU(0.1))
            n += 1
            nrows = B + 11
            p, Y = ol.draw(kind, B, C, (1 if kind == "sparse_cce" else C) + 3, nrows, seed=n, metric=metric)
            rows = np.random.default_rng(n).permutation(nrows)[:B] if addressing == "row_idx" else np.arange(7, 7 + B)
            inv_bg = 1.0 / (B + 3)
            calls.append((B, addressing, act, p, Y, rows, inv_bg, _reference(kind, metric, p, Y, rows, C, inv_bg, act)))
    eps = dict(l=max(float(np.abs(c[7]["l32"] - c[7]["l64"]).max()) for c in calls),
               m=max(float(np.abs(c[7]["m32"] - c[7]["m64"]).max()) for c in calls),
               g=max(float(np.abs(c[7]["g32s"] - c[7]["gref"]).max()) / c[6] for c in calls))
    worst = 0.0
    for B, addressing, act, p, Y, rows, inv_bg, ref in calls:
        rc, g, part, intact = _call(desc, p, Y, B, C, inv_bg, act, rows if addressing == "row_idx" else None, 7)
        assert rc == 0 and intact, (rc, intact)
        worst = max(worst, _check(kind, metric, B, C, act, ref, eps, g, part))
    print(f"{kind} C={C}: worst device error / bound = {worst:.3f} (bound = {FACTOR:g} x float32's own rounding)")


def _one_row(kind, p, y, param=None, metric=None):
    p, y = np.atleast_2d(np.asarray(p, F32)), np.atleast_2d(np.asarray(y, F32))
    rc, g, part, ok = _call(_desc(kind, metric, param), p, y, p.shape[0], p.shape[1], 1.0, 0)
    assert rc == 0 and ok
    return g, part


def test_edges_stay_finite_and_gradients_vanish_where_the_contract_says():
    g, part = _one_row("mae", [[1.5, -2.0, 0.25]], [[1.5, 0.0, 0.25]])
    assert g[0, 0] == 0 and g[0, 2] == 0 and g[0, 1] == -(F32(1) / F32(3))      # e = 0: no gradient
    g, part = _one_row("huber", [[2.0, -1.0, 0.5, 5.0]], [[1.0, 0.0, 0.0, 0.0]], param=1.0)   # |e| = delta exactly: the quadratic branch
    assert np.allclose(g, np.array([[1.0, -1.0, 0.5, 1.0]]) / 4, rtol=1e-6)
    assert np.isclose(part[0, 0], (0.5 + 0.5 + 0.125 + 4.5) / 4, rtol=1e-6)
    g, part = _one_row("log_cosh", [[1e4, -1e4]], [[0.0, 0.0]])
    assert np.isfinite(g).all() and np.isfinite(part).all() and np.allclose(g, [[0.5, -0.5]])
    assert np.isclose(part[0, 0], 1e4 - np.log(2.0), rtol=1e-6)
    for kind, big in (("cce_logits", 80.0), ("cce_logits", 1e4), ("bce_logits", 80.0), ("bce_logits", 1e4)):
        # (the third logit is not 0: the helper's max(z, 0) has its own kink there, where autograd picks a one-sided slope)
        g, part = _one_row(kind, [[big, -big, 0.5]], [[0.0, 1.0, 0.0]], param=0.0)
        assert np.isfinite(g).all() and np.isfinite(part).all(), (kind, big)
        l64, g64 = ol.rows_and_grad(kind, np.array([[0.0, 1.0, 0.0]]), np.array([[big, -big, 0.5]]))
        assert np.allclose(g, g64, atol=1e-6) and np.isclose(part[0, 0], l64[0], rtol=1e-6), (kind, big)
    for kind in ("bce", "kl_divergence", "sparse_cce", "cce"):   # probabilities exactly 0 and 1: clipped, no gradient there
        y = [[2.0]] if kind == "sparse_cce" else [[0.0, 1.0, 0.0]] if kind != "kl_divergence" else [[0.2, 0.3, 0.5]]
        g, part = _one_row(kind, [[1.0, 0.0, 0.0]], y, param=0.0)
        assert np.isfinite(g).all() and np.isfinite(part).all(), kind
        if kind == "kl_divergence":
            assert g[0, 1] == 0 and g[0, 2] == 0 and g[0, 0] != 0    # p = 1 is inside [eps, 1]; p = 0 is outside
        else:
            assert not g.any(), (kind, g)
    g, part = _one_row("msle", [[5e-8, 0.0, 2.0]], [[1.0, 1.0, 1.0]])     # p < eps: no gradient
    assert g[0, 0] == 0 and g[0, 1] == 0 and g[0, 2] != 0 and np.isfinite(part).all()
    p = np.array([[2.0, 6.0, 12.0]])                                     # unnormalised probabilities: q = p / 20
    g, part = _one_row("cce", p, [[0.0, 1.0, 0.0]], param=0.0)
    l64, g64 = ol.rows_and_grad("cce", np.array([[0.0, 1.0, 0.0]]), p)
    assert np.isclose(part[0, 0], -np.log(0.3), rtol=1e-6) and np.allclose(g, g64, rtol=1e-5, atol=1e-8)
    for p, y in (([[0.0, 0.0, 0.0]], [[1.0, 2.0, 3.0]]), ([[1.0, 2.0, 3.0]], [[0.0, 0.0, 0.0]]), ([[0.0, 0.0]], [[0.0, 0.0]])):
        g, part = _one_row("cosine_similarity", p, y)                    # all-zero rows: the 1e-12 clamp keeps them finite
        assert np.isfinite(g).all() and np.isfinite(part).all() and part[0, 0] == 0


@pytest.mark.parametrize("kind,C", [("mae", 1), ("huber", 3), ("cce_logits", 10), ("cosine_similarity", 65), ("cce", 257)])
def test_bits_do_not_depend_on_the_call_or_the_block(kind, C):
    B = 600
    metric = NATURAL_METRIC[kind]
    desc = _desc(kind, metric)
    p, Y = ol.draw(kind, B, C, C, B, seed=5, metric=metric)
    _, g1, part1, _ = _call(desc, p, Y, B, C, 1.0 / B, 3)
    _, g2, part2, _ = _call(desc, p, Y, B, C, 1.0 / B, 3)
    assert g1.tobytes() == g2.tobytes() and part1.tobytes() == part2.tobytes()
    rc, g3, part3, ok = _call(desc, p[256:], Y, B - 256, C, 1.0 / B, 3, row0=256)   # the same rows, one block further on
    assert rc == 0 and ok
    assert g3.tobytes() == g1[256:].tobytes() and part3.tobytes() == part1[1:].tobytes()


def test_refused_calls_launch_nothing_and_write_nothing():
    L, lib = _lib()
    B, C = 300, 5
    p, Y = ol.draw("mae", B, C, C, B, seed=1)
    n0 = lib.dib_launch_count()
    bad = [(_desc("mae", param=0.3), 0), (_desc("huber", param=0.0), 0), (_desc("huber", param=float("nan")), 0),
           (_desc("cce", param=1.5), 0), (_desc("mae", "sparse_categorical_accuracy"), 0), (_desc("sparse_cce", "mae"), 0),
           (L.LossDesc(2, 0, 0.0), 0), (L.LossDesc(99, 0, 0.0), 0), (L.LossDesc(4, 9, 0.0), 0), (_desc("mae"), 99)]
    for desc, act in bad:
        rc, g, part, ok = _call(desc, p, Y, B, C, 1.0, act)
        assert rc in (-1, -4) and ok and np.isnan(g).all() and np.isnan(part).all(), (desc.kind, desc.metric, desc.param, rc)
    st = ctypes.c_void_p(0)
    g, part = _guarded(B * C), _guarded(4)
    pd, Yd = torch.from_numpy(p).cuda(), torch.from_numpy(Y).cuda()
    d = _desc("mae")
    args = lambda **k: [k.get("desc", ctypes.byref(d)), k.get("p", _ptr(pd)), k.get("C", C), k.get("y", _ptr(Yd)), k.get("ldy", C),
                        None, 0, k.get("B", B), ctypes.c_float(1.0), 0, k.get("g", _ptr(g[PAD:])), k.get("part", _ptr(part[PAD:])), st]
    for k in (dict(desc=None), dict(p=None), dict(y=None), dict(g=None), dict(part=None), dict(B=0), dict(B=-3), dict(C=0),
              dict(ldy=C - 1)):
        assert lib.dib_loss_rows_ex(*args(**k)) == -1, k
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all().item()) and bool(torch.isnan(part).all().item())
    assert lib.dib_launch_count() == n0
    assert lib.dib_loss_ex_supported(ctypes.byref(_desc("sparse_cce", "sparse_categorical_accuracy")), 7) == 1
    assert [lib.dib_loss_ex_lanes(c) for c in (1, 2, 4, 5, 16, 17, 1000)] == [1, 4, 4, 16, 16, 64, 64]


# ---- step level ---------------------------------------------------------------------------------------------------------------
PROB_SPEC = orc.DIBSpec([2, 1], [16], [12], 3, output_activation_fn="sigmoid", feature_embedding_dimension=4)


def _engine(spec, seed=0):
    from dib_amd.engine import HipEngine
    eng = HipEngine(**spec_kwargs(spec), init_seed=seed)
    p = random_params(spec, seed)
    eng.set_flat_params(params_to_flat(eng.blocks, p, eng.params.numel()))
    return eng, flat_to_params(eng.blocks, eng.get_flat_params(), spec)


def _patch_oracle(monkeypatch):
    monkeypatch.setattr(orc, "loss_and_grad", ol.loss_and_grad)
    monkeypatch.setattr(orc, "accuracy", ol.accuracy)


@pytest.mark.parametrize("path", ["default", "grouped_gemm"])
@pytest.mark.parametrize("kind", ol.KINDS)
def test_one_training_step_matches_the_oracle_backward(kind, path, monkeypatch):
    """loss, metric, KL and every gradient block of one step against oracle.backward with the helper's loss swapped in"""
    from dib_amd import losses
    _patch_oracle(monkeypatch)
    spec = PROB_SPEC if kind in ol.PROBABILITY_KINDS + ol.POSITIVE_KINDS else SPECS["odd_shapes_tanh"]
    C, B = spec.output_dimensionality, 300
    metric = NATURAL_METRIC[kind]
    case = ol.Case(kind, ol.PARAM.get(kind, 0.0), metric)
    with dispatch_path(path):
        eng, p = _engine(spec, seed=7)
        rng = np.random.default_rng(3)
        n = B + 11
        x = rng.standard_normal((n, sum(spec.feature_dimensionalities))).astype(np.float32)
        _, y = ol.draw(kind, 1, C, 1 if kind == "sparse_cce" else C, n, seed=2)
        rows = rng.permutation(n)[:B].astype(np.int32)
        xd, yd = eng.to_device(x), eng.to_device(y)
        idx = eng.to_device(rows, dtype=torch.int32)
        beta, seed, step = 0.37, 11, 5
        eng.set_beta(beta)
        d = losses.LossDescriptor(kind, losses.KIND_IDS[kind], losses.METRIC_IDS[metric], case.param)
        eng.train_step(xd, yd, idx, 0, B, seed, step, d)
        torch.cuda.synchronize()
        F, E = spec.number_features, spec.feature_embedding_dimension
        eps = orc.philox_normal_all(seed, step, rows, F, E)
        c = orc.forward(spec, p, x[rows].astype(np.float64), eps)
        task, grads, g_u = orc.backward(spec, p, x[rows].astype(np.float64), y[rows], c, beta, case)
        so = eng.step_out(B).cpu().numpy()
        assert np.abs(so[:F] / B - c.kl).max() < 1e-3, "KL per feature (nats)"
        assert abs(so[F] / B - task) < 2e-4 * (1 + abs(task)), ("task loss", so[F] / B, task)
        want = orc.accuracy(case, y[rows], c.pred)
        assert abs(so[F + 1] / B - want) < (1e-6 if "accuracy" in metric else 2e-4 * (1 + abs(want))), (so[F + 1] / B, want)
        assert so[F + 2] == B
        gflat = eng.get_flat_grads()
        gref = params_to_flat(eng.blocks, grads, eng.params.numel()).astype(np.float64)
        for b in eng.blocks:
            sl = slice(b["offset"], b["offset"] + b["rows"] * b["cols"])
            err = np.abs(gflat[sl] - gref[sl]).max()
            assert err <= 3e-4 * (np.abs(gref[sl]).max() + 1e-3), (b, err, np.abs(gref[sl]).max())


# ---- fit level ----------------------------------------------------------------------------------------------------------------
def _circuit(copies=8):
    x, y = orc.boolean_circuit_truth_table([0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]], 4)
    return np.tile(x, (copies, 1)).astype(np.float32), np.tile(y, copies).astype(np.float32)


def _fit_against_oracle(monkeypatch, spec, loss, metric_name, case, x, y):
    """30 steps (10 epochs of 2 full batches and a ragged one) with validation against oracle.fit; returns the model"""
    import dib_amd
    _patch_oracle(monkeypatch)
    model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
    opt = dib_amd.optimizers.get("adam")
    opt.learning_rate = 3e-3
    model.compile(optimizer=opt, loss=loss, metrics=[metric_name])
    cb = dib_amd.InfoBottleneckAnnealingCallback(1e-3, 1.0, 2, 6)
    p = flat_to_params(model.param_blocks(), model.get_flat_weights(), spec)
    epochs, bs = 10, 48
    hist = model.fit(x, y, epochs=epochs, shuffle=True, batch_size=bs, callbacks=[cb], verbose=False, validation_data=(x[:40], y[:40]))
    ref = orc.fit(spec, p, x, y, epochs=epochs, batch_size=bs, loss_kind=case, beta_fn=lambda e: orc.beta_schedule(e, 1e-3, 1.0, 2, 6),
                  lr=3e-3, shuffle=True, validation_data=(x[:40], y[:40]), noise_seed=4, shuffle_seed=6, metrics=["accuracy"])
    ref = {k.replace("accuracy", metric_name): v for k, v in ref.items()}
    assert set(ref) == set(hist.history) and metric_name in ref and "val_" + metric_name in ref
    for k in ref:
        got, want = np.array(hist.history[k]), np.array(ref[k])
        tol = 1e-3 if "KL" in k else 2e-3
        assert np.abs(got - want).max() < tol * (1 + np.abs(want).max()), (k, got, want)
    logs = model.evaluate(x[:40], y[:40], batch_size=bs)
    assert set(logs) == {k for k in hist.history if not k.startswith("val_")}
    return model


def test_fit_under_huber_with_mae_matches_the_oracle_fit(monkeypatch):
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
    x, y = _circuit()
    y = (2.5 * y + 0.3 * x[:, 0] - 0.2).astype(np.float32)   # a regression target with residuals on both sides of delta
    _fit_against_oracle(monkeypatch, spec, dib_amd.losses.Huber(delta=0.5), "mae", ol.Case("huber", 0.5, "mae"), x, y)


def test_fit_on_one_hot_labels_with_smoothing_and_accuracy_matches_the_oracle_fit(monkeypatch):
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64], 3, feature_embedding_dimension=8)
    x, y = _circuit()
    labels = (y + x[:, 0] * (1 - y) * 2).astype(np.int64)    # three classes
    onehot = np.eye(3, dtype=np.float32)[labels]
    loss = dib_amd.losses.CategoricalCrossentropy(from_logits=True, label_smoothing=0.1)
    model = _fit_against_oracle(monkeypatch, spec, loss, "accuracy", ol.Case("cce_logits", 0.1, "categorical_accuracy"), x, onehot)
    with pytest.raises(ValueError, match="sum to 1"):
        model.fit(x, onehot * 2, epochs=1, batch_size=48, verbose=False)
    with pytest.raises(ValueError, match="sample_weight"):
        model.fit(x, onehot, epochs=1, batch_size=48, verbose=False, sample_weight=np.ones(len(x)))


def test_root_mean_squared_error_takes_the_root_at_the_end_of_the_epoch():
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
    x, y = _circuit()
    logs = {}
    for name in ("mse", "root_mean_squared_error"):
        model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        model.compile(optimizer="adam", loss="mae", metrics=[name])
        logs[name] = model.evaluate(x, y, batch_size=48)[name]
    assert logs["root_mean_squared_error"] == pytest.approx(np.sqrt(logs["mse"]), rel=1e-6)


# ---- what must not change -----------------------------------------------------------------------------------------------------
def test_the_reference_kinds_keep_their_route_and_their_launch_counts():
    """bce_logits and mse with metrics=['accuracy'] go to the engine by NAME: dib_loss_fwd_bwd / the fused one-unit head, the
    launches of the untouched entry points.  BCE-from-logits with label smoothing is a descriptor and never takes the head."""
    import dib_amd
    from dib_amd import _lib as L
    lib = L.load_library()
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
    x, y = _circuit()
    B = 48
    counts = {}
    for name, loss in (("bce_logits", dib_amd.losses.BinaryCrossentropy(from_logits=True)), ("mse", "mse"),
                       ("smoothed", dib_amd.losses.BinaryCrossentropy(from_logits=True, label_smoothing=0.1))):
        model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        model.compile(optimizer="adam", loss=loss, metrics=["accuracy"])
        arg = model._loss_arg()
        eng = model._ensure_engine()
        xd, yd = eng.to_device(x), eng.to_device(y[:, None])
        eng.train_step(xd, yd, None, 0, B, 1, 0, arg)   # (module loads)
        n0 = lib.dib_launch_count()
        eng.train_step(xd, yd, None, 0, B, 1, 1, arg)
        counts[name] = lib.dib_launch_count() - n0
        if name == "smoothed":
            assert not isinstance(arg, str) and arg.param == pytest.approx(0.1) and not eng._head_fused(arg)
            loss_sm = eng.step_out(B).cpu().numpy()[4]
        else:
            assert arg == name and eng._head_fused(L.LOSS_KINDS[name])
            n0 = lib.dib_launch_count()
            eng.train_step(xd, yd, None, 0, B, 1, 1, name)
            assert lib.dib_launch_count() - n0 == counts[name]
            if name == "bce_logits":
                loss_plain = eng.step_out(B).cpu().numpy()[4]
    torch.cuda.synchronize()
    assert counts["bce_logits"] == counts["mse"] < counts["smoothed"], counts
    assert loss_sm != loss_plain   # the smoothing reached the kernel


def test_fit_under_graph_replay_has_the_eager_bits_for_a_new_kind(monkeypatch):
    """DIB_ENABLE_GRAPHS=1: the step of a descriptor loss is captured like the reference kinds' (dib_loss_fwd_bwd_ex is one
    capturable launch) and its replay gives the bits of the eager launch sequence"""
    import dib_amd
    spec = orc.DIBSpec([1, 1, 1, 1], [32, 32], [64, 64], 1, feature_embedding_dimension=8)
    x, y = _circuit(33)
    x, y = x[:520], (2.5 * y[:520] - 0.2).astype(np.float32)

    def run():
        model = dib_amd.DistributedIBNet(**spec_kwargs(spec), noise_seed=4, shuffle_seed=6, init_seed=2)
        model.compile(optimizer="adam", loss=dib_amd.losses.Huber(delta=0.5), metrics=["mae"])
        h = model.fit(x, y, epochs=9, shuffle=True, batch_size=64, verbose=False, validation_data=(x[:100], y[:100]))
        return h.history, model.get_flat_weights(), model

    monkeypatch.setenv("DIB_ENABLE_GRAPHS", "1")
    hist_g, w_g, model_g = run()
    assert getattr(model_g._engine, "step_dev", None) is not None, "graph path was not taken"
    monkeypatch.setenv("DIB_ENABLE_GRAPHS", "0")
    hist_e, w_e, model_e = run()
    assert getattr(model_e._engine, "step_dev", None) is None
    for k in hist_e:
        assert hist_g[k] == hist_e[k], k
    assert np.array_equal(w_g, w_e)
