"""NumPy oracle of the encoder bank ALONE (checker of dib_fused_encoder_fwd_kernel / dib_fused_encoder_bwd_kernel, csrc/dib_fused.h;
calls nothing of the library), and the cases of tests/test_gpu_fused_envelope.py, built without the library so that the float32
restatement of tests/test_fused_encoder_oracle.py can run anywhere.

Per feature f (reference models.py:101-112):  P = positional_encoding(x_f) ; h1 = act(P W1 + b1) ; h2 = act(h1 W2 + b2) ;
(mu | logvar) = h2 W3 + b3 ; u = mu + exp(logvar / 2) eps ; KL_f = sum_rows sum_e (mu^2 + exp(logvar) - logvar - 1) / 2.
Given dL/du = g_u, beta and inv_bg (the backward's arguments):
    dmu = g_u + beta inv_bg mu ;  dlogvar = g_u (u - mu) / 2 + beta inv_bg (exp(logvar) - 1) / 2 ;  dout = (dmu | dlogvar)
    dW3 = h2^T dout ; dh2 = (dout W3^T) act'(h2) ; dW2 = h1^T dh2 ; dh1 = (dh2 W2^T) act'(h1) ; dW1 = P^T dh1 ; db = column sums
with act' taken from the activation OUTPUT as dib_oracle._act_grad_from_output does (relu' = [h > 0], leaky' = 1 if h > 0 else 0.2).
Everything runs in the dtype of its arguments: float64 for the reference, float32 for the restatement that measures what float32
arithmetic alone costs."""
import zlib
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

import dib_oracle as orc


@dataclass
class EncoderForward:
    P: List[np.ndarray]       # [F] of [B, in_dim_f]
    z1: List[np.ndarray]      # [F] of [B, H1] pre-activations
    z2: List[np.ndarray]
    h1: List[np.ndarray]
    h2: List[np.ndarray]
    mu: np.ndarray            # [B, F, E]
    logvar: np.ndarray
    u: np.ndarray
    kl: np.ndarray            # [F] summed over rows (what ws[STEP_OUT][:F] holds)
    u_slack: Optional[np.ndarray] = None     # [B, F, E] sigma x noise_float32_slack (reference() fills it)


def encoder_forward(spec: orc.DIBSpec, p: orc.DIBParams, x: np.ndarray, eps: np.ndarray) -> EncoderForward:
    F, E = spec.number_features, spec.feature_embedding_dimension
    dt = x.dtype
    xs = orc.split_features(x, spec.feature_dimensionalities)
    freqs = spec.frequencies.astype(dt)
    Ps, z1s, z2s, h1s, h2s, mus, lvs = [], [], [], [], [], [], []
    for f in range(F):
        P = orc.positional_encoding(xs[f], freqs) if spec.use_positional_encoding else xs[f]
        W, b = p.enc_W[f], p.enc_b[f]
        assert len(W) == 3 and W[0].dtype == dt
        z1 = P @ W[0] + b[0]
        h1 = orc._act(spec.activation_fn, z1)
        z2 = h1 @ W[1] + b[1]
        h2 = orc._act(spec.activation_fn, z2)
        out = h2 @ W[2] + b[2]
        Ps.append(P); z1s.append(z1); z2s.append(z2); h1s.append(h1); h2s.append(h2)
        mus.append(out[:, :E]); lvs.append(out[:, E:])
    mu, lv = np.stack(mus, 1), np.stack(lvs, 1)
    eps = np.asarray(eps, dtype=dt)
    u = mu + np.exp(lv / dt.type(2.0)) * eps
    kl = (dt.type(0.5) * (mu * mu + np.exp(lv) - lv - dt.type(1.0))).sum(axis=(0, 2))
    return EncoderForward(Ps, z1s, z2s, h1s, h2s, mu, lv, u, kl)


def encoder_backward(spec: orc.DIBSpec, p: orc.DIBParams, fw: EncoderForward, g_u: np.ndarray, beta: float, inv_bg: float):
    """the six gradient blocks per feature, as a DIBParams whose integration blocks are zero"""
    F, E = spec.number_features, spec.feature_embedding_dimension
    dt = fw.mu.dtype
    B = fw.mu.shape[0]
    gu = np.asarray(g_u, dtype=dt).reshape(B, F, E)
    kb = dt.type(beta) * dt.type(inv_bg)
    half = dt.type(0.5)
    dmu = gu + kb * fw.mu
    dlv = gu * (fw.u - fw.mu) * half + kb * (np.exp(fw.logvar) - dt.type(1.0)) * half
    grads = p.zeros_like()
    for f in range(F):
        W = p.enc_W[f]
        dout = np.concatenate([dmu[:, f], dlv[:, f]], axis=-1)
        grads.enc_W[f][2] = fw.h2[f].T @ dout
        grads.enc_b[f][2] = dout.sum(0)
        dh2 = (dout @ W[2].T) * orc._act_grad_from_output(spec.activation_fn, fw.h2[f])
        grads.enc_W[f][1] = fw.h1[f].T @ dh2
        grads.enc_b[f][1] = dh2.sum(0)
        dh1 = (dh2 @ W[1].T) * orc._act_grad_from_output(spec.activation_fn, fw.h1[f])
        grads.enc_W[f][0] = fw.P[f].T @ dh1
        grads.enc_b[f][0] = dh1.sum(0)
    return grads


# ---- the cases of tests/test_gpu_fused_envelope.py ---------------------------------------------------------------------------------
BETA, SEED, STEP = 0.37, 11, 5
PAD_ROWS = 11                 # every case's x has B + 11 rows: row_idx gathers into them, row0 = 7 shifts into them
ROW0 = 7
# A float32 act' can differ from the float64 one only where 0 < |z| < GUARD: 8 x the largest |z32 - z64| over the cases' hidden
# pre-activations, 9.7e-7 (tests/test_fused_encoder_oracle.py re-measures it).  The builder leaves no such pre-activation.
GUARD = 8 * 9.7e-7
MAX_REDRAW_ROUNDS = 4         # the largest observed: 2
_INT = ([8], 1)               # the integration network is never run; it only has to exist


def _cyc(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


@dataclass
class Case:
    spec: orc.DIBSpec
    B: int
    dead: bool = False            # units {0, 31, H - 1} of both hidden layers of the first and last feature exactly dead
    backward: bool = True         # the instantiation has a fused backward
    path: str = "default"         # tests/_helpers.py dispatch_path
    modes: tuple = ("plain",)


def _spec(dims, arch, E, act, **kw):
    return orc.DIBSpec(list(dims), list(arch), _INT[0], _INT[1], activation_fn=act, feature_embedding_dimension=E, **kw)


CASES = {
    "trips_f64_h32_relu": Case(_spec([1] * 64, (32, 32), 32, "relu"), 1300, dead=True,
                               modes=("plain", "gather", "row0", "numerics")),
    "trips_f64_h128_relu": Case(_spec([1] * 64, (128, 128), 32, "relu"), 1100, dead=True),
    "trips_f128_h128_leaky_ragged": Case(_spec(_cyc([1, 2, 3], 128), (128, 128), 32, "leaky_relu"), 1000, dead=True),
    "trips_f100_h32_leaky_in15": Case(_spec(_cyc([1, 3, 5], 100), (32, 32), 32, "leaky_relu",
                                            number_positional_encoding_frequencies=3), 800),
    "trips_f50_e16_relu": Case(_spec(_cyc([1, 7, 8, 9, 16], 50), (64, 64), 16, "relu", use_positional_encoding=False), 1537,
                               backward=False),
    "trips_f300_e8_linear": Case(_spec([1] * 300, (32, 32), 8, None), 600, backward=False),
}
for _b in (32, 33, 256, 257):
    CASES[f"edges_single_trip_b{_b}"] = Case(_spec([1, 2, 3], (32, 32), 32, "relu"), _b, path="large_batch")
TRIPS = [n for n in CASES if n.startswith("trips_")]
VARIANTS = [(n, m) for n, c in CASES.items() for m in c.modes]


def fused_gx(F, B):
    """csrc/host/encoder.h fused_gx: workgroups per feature of the persistent grid"""
    return max(1, min(-(-B // 256), max(1, 256 // F)))


def in_row_tile_regime(F, B):
    """csrc/host/encoder.h small_regime with the default tuning"""
    return B <= 2048 and -(-B // 16) * F <= 512


def probe_rows(F, B):
    """rows 0, 31, 32, 255, 256, the first and last row of the first tile a workgroup sees on its second trip, the first row of
    the tail tile, B - 1: those that exist, each once, ascending"""
    gx, n_tiles = fused_gx(F, B), -(-B // 256)
    cand = [0, 31, 32, 255, 256, gx * 256, min(gx * 256 + 255, B - 1), (n_tiles - 1) * 256, B - 1]
    return sorted({r for r in cand if 0 <= r < B})


def _case_seed(name):
    return zlib.crc32(name.encode()) % 1000


def _kill(p, f, layer, unit, bias=0.0):
    p.enc_W[f][layer][:, unit] = 0.0
    p.enc_b[f][layer][unit] = bias


def _near_edge(spec, p64, x64):
    """[(row, feature)] whose float64 hidden pre-activations have an entry with 0 < |z| < GUARD (exact zeros: the dead units)"""
    fw = encoder_forward(spec, p64, x64, np.zeros((x64.shape[0], spec.number_features, spec.feature_embedding_dimension)))
    bad = []
    for f in range(spec.number_features):
        near = np.zeros(x64.shape[0], dtype=bool)
        for z in (fw.z1[f], fw.z2[f]):
            a = np.abs(z)
            near |= ((a > 0) & (a < GUARD)).any(axis=1)
        bad += [(int(r), f) for r in np.nonzero(near)[0]]
    return bad


@dataclass
class BuiltCase:
    name: str
    case: Case
    p32: orc.DIBParams
    x: np.ndarray                 # [B + PAD_ROWS, sum_d] float32
    redraw_rounds: int
    refs: dict = field(default_factory=dict)


_BUILT = {}


def build(name) -> BuiltCase:
    """float32 parameters (glorot kernels, N(0, 0.1^2) biases, the dead units) and N(0, 1) inputs with the knife edges redrawn"""
    if name in _BUILT:
        return _BUILT[name]
    from _helpers import random_params
    case = CASES[name]
    spec = case.spec
    seed = _case_seed(name)
    p32 = random_params(spec, seed).astype(np.float32)
    if case.dead:
        H = spec.feature_encoder_architecture[0]
        for f in (0, spec.number_features - 1):
            for layer in (0, 1):
                for unit in (0, 31, H - 1):
                    _kill(p32, f, layer, unit)
        p32.enc_b[0][0][31] = np.float32(-0.0)
        p32.enc_b[spec.number_features - 1][1][0] = np.float32(-0.0)
    n = case.B + PAD_ROWS
    x = np.random.default_rng(case.B + seed).standard_normal((n, sum(spec.feature_dimensionalities))).astype(np.float32)
    rounds = 0
    if spec.activation_fn in ("relu", "leaky_relu"):
        p64 = p32.astype(np.float64)
        col = np.concatenate([[0], np.cumsum(spec.feature_dimensionalities)])
        bad = _near_edge(spec, p64, x.astype(np.float64))
        while bad:
            rounds += 1
            assert rounds <= MAX_REDRAW_ROUNDS, (name, len(bad))
            rng = np.random.default_rng([seed, 1000 + rounds])
            for r, f in bad:
                x[r, col[f]: col[f + 1]] = rng.standard_normal(col[f + 1] - col[f]).astype(np.float32)
            # only the redrawn rows can have a new edge (and only in the redrawn feature, which the re-check covers)
            rows = sorted({r for r, _ in bad})
            again = _near_edge(spec, p64, x[rows].astype(np.float64))
            bad = [(rows[i], f) for i, f in again]
    x.setflags(write=False)
    _BUILT[name] = BuiltCase(name, case, p32, x, rounds)
    return _BUILT[name]


def numerics_params(bc: BuiltCase) -> orc.DIBParams:
    """the last layer shrunk, its logvar biases spread from -30 to +8 across the E dims, its mu biases +-4: sigma from 3e-7 to 55"""
    p = bc.p32.copy()
    E = bc.case.spec.feature_embedding_dimension
    for f in range(bc.case.spec.number_features):
        p.enc_W[f][2] *= np.float32(0.05)
        p.enc_b[f][2][:E] = np.where(np.arange(E) % 2 == 0, 4.0, -4.0).astype(np.float32)
        p.enc_b[f][2][E:] = np.linspace(-30.0, 8.0, E).astype(np.float32)
    return p


def batch_ids(bc: BuiltCase, mode):
    """dataset rows of the batch: what keys the noise"""
    B = bc.case.B
    if mode == "gather":
        return np.random.default_rng(B).permutation(B + PAD_ROWS)[:B].astype(np.int32)
    return np.arange(B, dtype=np.int32) + (ROW0 if mode == "row0" else 0)


def g_u_of(bc: BuiltCase, kind):
    """dL/du [B, F E] float32: "dense" N(0, 1) / B everywhere; "probe" N(0, 1) on the probe rows and exactly 0 elsewhere;
    "complement" exactly 0 on the probe rows and N(0, 1) / B elsewhere"""
    spec, B = bc.case.spec, bc.case.B
    FE = spec.number_features * spec.feature_embedding_dimension
    rng = np.random.default_rng([_case_seed(bc.name), {"dense": 1, "probe": 2, "complement": 3}[kind]])
    g = rng.standard_normal((B, FE)).astype(np.float32)
    rows = probe_rows(spec.number_features, B)
    if kind == "probe":
        keep = np.zeros(B, dtype=bool)
        keep[rows] = True
        g[~keep] = 0.0
        return g
    g = (g / np.float32(B)).astype(np.float32)
    if kind == "complement":
        g[rows] = 0.0
    return g


def run(bc: BuiltCase, mode, dtype, want=("dense", "probe", "complement")):
    """(parameters, EncoderForward, {kind: gradients}) of one variant in `dtype` arithmetic.  dense: beta = BETA; the probes: beta = 0."""
    spec, B = bc.case.spec, bc.case.B
    p = (numerics_params(bc) if mode == "numerics" else bc.p32).astype(dtype)
    ids = batch_ids(bc, mode)
    eps = orc.philox_normal_all(SEED, STEP, ids, spec.number_features, spec.feature_embedding_dimension)
    fw = encoder_forward(spec, p, bc.x[ids].astype(dtype), eps.astype(dtype))
    grads = {}
    if bc.case.backward:
        for kind in want:
            grads[kind] = encoder_backward(spec, p, fw, g_u_of(bc, kind), BETA if kind == "dense" else 0.0, 1.0 / B)
    return p, fw, grads


def _radius_uniforms(ids, F, E):
    """the uniform behind the Box-Muller radius of every eps[b, f, e] (dib_oracle.philox_normal's u0 for e % 4 < 2, u2 otherwise)"""
    rows = np.asarray(ids, dtype=np.uint32).reshape(-1, 1)
    nblk = (E + 3) // 4
    blk = np.arange(nblk, dtype=np.uint32).reshape(1, -1)
    out = np.empty((len(rows), F, nblk * 4))
    for f in range(F):
        x = orc.philox4x32_10(rows, np.uint32(f), blk, np.uint32(STEP), SEED & 0xFFFFFFFF, (SEED >> 32) & 0xFFFFFFFF)
        u = [((xi >> np.uint32(8)).astype(np.float64) + 0.5) * (1.0 / 16777216.0) for xi in (x[0], x[2])]
        out[:, f] = np.stack([u[0], u[0], u[1], u[1]], axis=-1).reshape(len(rows), nblk * 4)
    return out[:, :, :E]


def noise_float32_slack(ids, F, E, eps64):
    """What ANY float32 evaluation of the noise spec (csrc/dib_common.h dib_eps4, host or device) may differ from the float64 one
    by, beyond ordinary rounding: the radius uniform u0 = (k + 0.5) 2^-24 is not a float32 once k >= 2^23 (25 significant bits), so
    it carries up to 2^-25 of absolute error, and r = sqrt(-2 ln u0) has dr/du0 = -1 / (u0 r): |d eps| <= 2^-25 |eps| / (u0 r^2).
    Negligible but where u0 -> 1 (r -> 0, |eps| <= r small): 2^-25 / r there, up to 1.2e-4 at the last uniform."""
    u0 = _radius_uniforms(ids, F, E)
    return 2.0 ** -25 * np.abs(eps64) / (u0 * (-2.0 * np.log(u0)))


def reference(name, mode):
    """the float64 reference of a variant: computed once, shared by every test that needs it, read-only"""
    bc = build(name)
    if mode not in bc.refs:
        _, fw, grads = run(bc, mode, np.float64)
        for a in fw.h1 + fw.h2 + [fw.mu, fw.logvar, fw.u, fw.kl] + [t for g in grads.values() for t in g.tensors()]:
            a.setflags(write=False)
        fw.P, fw.z1, fw.z2 = None, None, None      # (not compared; a third of the memory)
        spec, ids = bc.case.spec, batch_ids(bc, mode)
        F, E = spec.number_features, spec.feature_embedding_dimension
        fw.u_slack = np.exp(fw.logvar / 2.0) * noise_float32_slack(ids, F, E, orc.philox_normal_all(SEED, STEP, ids, F, E))
        fw.u_slack.setflags(write=False)
        bc.refs[mode] = (fw, grads)
    return bc.refs[mode]


# ---- error figures: max|got - ref| / max|ref| ----------------------------------------------------------------------------------------
def rel_err(got, ref):
    scale = float(np.abs(ref).max())
    assert scale > 0
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max()) / scale


def forward_errors(spec, got, ref):
    """got / ref: dicts of h1, h2 [F][B, H] and mu, logvar, u [B, F, E] -> {(tensor, feature): figure}"""
    out = {}
    for f in range(spec.number_features):
        for k in ("h1", "h2"):
            out[(k, f)] = rel_err(got[k][f], ref[k][f])
        for k in ("mu", "logvar", "u"):
            out[(k, f)] = rel_err(got[k][:, f], ref[k][:, f])
    return out


def grad_errors(spec, got: orc.DIBParams, ref: orc.DIBParams):
    """{(block, feature): figure} over the six encoder blocks of every feature, and over the dlogvar halves of dW3 / db3 on their
    own scale (next to the dmu halves they may be small)"""
    out = {}
    E = spec.feature_embedding_dimension
    for f in range(spec.number_features):
        for l in range(3):
            out[(f"dW{l + 1}", f)] = rel_err(got.enc_W[f][l], ref.enc_W[f][l])
            out[(f"db{l + 1}", f)] = rel_err(got.enc_b[f][l], ref.enc_b[f][l])
        out[("dW3_logvar", f)] = rel_err(got.enc_W[f][2][:, E:], ref.enc_W[f][2][:, E:])
        out[("db3_logvar", f)] = rel_err(got.enc_b[f][2][E:], ref.enc_b[f][2][E:])
    return out


def worst(errs):
    k = max(errs, key=errs.get)
    return errs[k], k
