"""The row-tile kernels (csrc/dib_small.h) across the envelope dib_layout_create admits, against the float64 oracle.

Every case is one training step through HipEngine (Philox noise, a gathered batch): mu / logvar, u, pred, per-feature KL, the task
loss, dL/du and every gradient block against oracle/dib_oracle.py at the tolerances of test_gpu_parity.py, then a validation step
(eval_step, no stashes) at a later noise step against the oracle forward of that step.  Cases marked `custom` also run the
custom-loss entry (forward + backward_from_pred_grad, the InfoNCE loop's contract) against tests/_oracle_pred_grad.py.

Each case states the branch of the kernels' width-dependent code it is there for and the path it must take, as launches per
step of the categories the library's live profile counts (dib_profile_summary): mode-0 / mode-1 / mode-2 GEMMs and the fused
encoder-bank kernels.  The row-tile kernels themselves are "other" (not counted), so a step entirely on row tiles shows exactly
one launch: the merged weight-gradient GEMM (mode 2) of dib_backward.  A silent fall-back shows up as extra GEMM launches.

The counts come from the dispatch code (csrc/host/step.h and csrc/host/encoder.h, n = integration hidden layers):
  ROW     encoders + integration on row tiles, 1-unit head or out_dim % 16 == 0: merged wgrad only       train {g2: 1}, eval {}
  SKINNY  ... out_dim <= 8, not the head: output layer on the skinny kernels, every integration layer's backward (and so its
          dgrad) on GEMMs (integration_bwd_impl: no row-tile dgrad chain without a row-tile output layer), encoder wgrads 2, 3
                                                                                               train {g1: n, g2: n + 2}, eval {}
  OUTGEMM ... 8 < out_dim, out_dim % 16 != 0: as SKINNY, the output layer a GEMM too   train {g0: 1, g1: n + 1, g2: n + 3}, eval {g0: 1}
  ENCGEMM encoders outside the envelope on the grouped GEMMs (3 fwd, 3 wgrad, 2 dgrad), integration on row tiles with the head:
          its hidden wgrads run per layer                                            train {g0: 3, g1: 2, g2: n + 3}, eval {g0: 3}
  INTGEMM integration outside (head), encoders on row tiles: hidden fwd / dgrad / wgrad per layer, encoder wgrads 2, 3
                                                                                   train {g0: n, g1: n, g2: n + 2}, eval {g0: n}
  LARGE   the batch is outside the row-tile regime (non-fused widths, head): everything on GEMMs
                                                                           train {g0: n + 3, g1: n + 2, g2: n + 3}, eval {g0: n + 3}
"""
import collections
import zlib

import numpy as np
import pytest
import torch

import dib_oracle as orc
from _helpers import flat_to_params, params_to_flat, random_params, spec_kwargs
from _oracle_pred_grad import backward_from_pred_grad

# ---- the kernels' width-dependent selections (csrc/dib_small.h), restated ONLY to check that the case table reaches each ----


def _pick_nt(n):   # dib_small_pick_nt -> which return statement
    t = n // 16
    if n % 64 == 0 and (n // 64) % 4 == 0:
        return "nt4:T%16"
    if n % 32 == 0 and (n // 32) % 4 == 0:
        return "nt2:T%8"
    if t % 4 == 0:
        return "nt1:T%4"
    if n % 32 == 0:
        return "nt2:T%2"
    return "nt1:odd"


def _pick_nt_bwd(kin):   # dib_small_pick_nt_bwd -> which return statement
    t = kin // 16
    for m, name in ((20, "nt5:T%20"), (16, "nt4:T%16"), (8, "nt2:T%8"), (4, "nt1:T%4"), (5, "nt5:T%5"), (2, "nt2:T%2")):
        if t % m == 0:
            return name
    return "nt1:odd"


def _fwd_cols(K, ncols):   # dib_small_fwd_cols: (nt, kways, ub)
    nt = 4 if ncols % 64 == 0 else (2 if ncols % 32 == 0 else 1)
    ng = ncols // (16 * nt)
    kw = 8 if ng <= 1 else (4 if ng == 2 else 2)
    per_share = ((K + 3) // 4 + kw - 1) // kw
    return nt, kw, 8 if per_share <= 8 else (10 if per_share <= 10 else 16)


def _bwd_cols(N, kcols):   # dib_small_bwd_cols: G, ub (G = 0: dib_small_bwd's pick_nt_bwd class instead)
    t = kcols // 16
    G = 1 if t <= 5 else (2 if t <= 10 and t % 2 == 0 else 0)
    if G == 0:
        return 0, _pick_nt_bwd(kcols)
    kmax = 8 // G
    return G, 1 if N <= 16 * kmax else (2 if N <= 256 else 4)


def _slices(width, cl):   # dib_small_cluster_slice: 16-column tiles of each workgroup of a cluster
    T = width // 16
    return [(c + 1) * T // cl - c * T // cl for c in range(cl)]


def _branches(case):
    """Branch labels the case's row-tile launches take (encoder kernels, single-workgroup or cluster integration kernel)."""
    s, hit = case.spec, set()
    F, E = s.number_features, s.feature_embedding_dimension
    if case.enc == "rt":
        H1, H2 = s.feature_encoder_architecture
        hit.add("enc.l1." + _pick_nt(H1))
        for K, N in ((H1, H2), (H2, 2 * E)):
            nt, kw, ub = _fwd_cols(K, N)
            hit |= {f"enc.fwdcols.nt{nt}", f"enc.fwdcols.kw{kw}", f"enc.fwdcols.ub{ub}"}
        for N, k in ((2 * E, H2), (H2, H1)):
            G, ub = _bwd_cols(N, k)
            hit |= {f"enc.bwdcols.G{G}"} | ({f"enc.bwdcols.ub{ub}"} if G else {"bwd." + ub})
    units, out = list(s.integration_network_architecture), s.output_dimensionality
    head = out == 1 and case.kind in ("bce_logits", "mse")
    out_rt = out % 16 == 0 and not head
    K0 = F * E
    ins = [K0] + units[:-1]
    if case.int == "wg":
        hit |= {"int.fwd." + _pick_nt(w) for w in units} | ({"int.fwd." + _pick_nt(out)} if out_rt else set())
        hit |= {"bwd." + _pick_nt_bwd(k) for k in ins} | ({"bwd." + _pick_nt_bwd(units[-1])} if out_rt else set())
    elif case.int == "cl":
        cl = case.tune["int_cluster"]
        fw = [(k, w) for k, w in zip(ins, units)] + ([(units[-1], out)] if out_rt else [])
        bw = [(units[l], units[l - 1]) for l in range(1, len(units))] + [(units[0], K0)] + ([(out, units[-1])] if out_rt else [])
        for K, w in fw:
            for t in _slices(w, cl):
                hit.add("cl.empty" if t == 0 else f"cl.fwdcols.ub{_fwd_cols(K, 16 * t)[2]}")
        for N, k in bw:
            for t in _slices(k, cl):
                if t:
                    G, ub = _bwd_cols(N, 16 * t)
                    hit.add(f"cl.bwdcols.G{G}:{t}")
    return hit


# ---- the case table ----------------------------------------------------------------------------------------------------

def _S(dims, enc, integ, out, E, pe=True, nf=5, act="relu", out_act=None):
    return orc.DIBSpec(dims, enc, integ, out, use_positional_encoding=pe, number_positional_encoding_frequencies=nf,
                       activation_fn=act, feature_embedding_dimension=E, output_activation_fn=out_act)


def _L(g0=0, g1=0, g2=0, fused=0):
    return {"g0": g0, "g1": g1, "g2": g2, "fused": fused}


ROW = (_L(g2=1), _L())
WG = {"int_cluster": 1}   # the single-workgroup integration kernel whatever the network's size
Case = collections.namedtuple("Case", "spec B kind expect enc int tune custom")


def _C(spec, B, kind, expect=ROW, enc="rt", int="wg", tune=WG, custom=False):
    return Case(spec, B, kind, expect, enc, int, tune, custom)


CASES = {
    # ---- encoder bank: layer 1 on dib_small_fwd (pick_nt of H1), layers 2 / 3 forward on dib_small_fwd_cols (whole-layer slice: nt
    # from the width, kways from its groups, ub from K), layers 3 / 2 backward on dib_small_bwd_cols (G from H2 / H1 tiles, ub from
    # N = 2E / H2; G = 0: dib_small_bwd and pick_nt_bwd)
    # H1 = 256: pick_nt T % 16; layer 2 nt 1 x 5 groups ub 16; layer-3 backward G = 1 (H2 = 80: 5 tiles) ub 1, layer 2 G = 0 T % 16
    "enc_256_80_e8": _C(_S([1, 1], [256, 80], [32], 1, 8), 17, "bce_logits"),
    # E = 40 (2E = 80); H1 = 128: pick_nt T % 8; layer 2 nt 2 (3 groups); backwards G = 2 (H2 = 96: 6 tiles, H1 = 128: 8) ub 2
    "enc_128_96_e40": _C(_S([2, 1], [128, 96], [32], 1, 40), 16, "bce_logits"),
    # the widest square encoder that fits (162 304 B for the backward): pick_nt T % 4, nt 4 x 7 groups, G = 0 (28 tiles: T % 4)
    "enc_448_448_e32": _C(_S([1], [448, 448], [64], 16, 32), 15, "mse", custom=True),
    # leaky_relu; H1 = 160: pick_nt T % 2; layer-3 backward G = 0 (H2 = 176: 11 tiles, pick_nt_bwd odd), layer 2 G = 2 (10 tiles)
    "enc_160_176_leaky": _C(_S([3, 1], [160, 176], [32], 1, 8, act="leaky_relu"), 1, "bce_logits"),
    # E = 512 with narrow encoders, F = 2 (K0 = 1024); H1 = 48: pick_nt odd; layer-3 backward G = 2 (H2 = 160) ub 4 (N = 1024),
    # layer 2 G = 1 ub 2
    "enc_48_160_e512": _C(_S([1, 2], [48, 160], [64], 1, 512), 37, "bce_logits"),
    # layer-3 forward ub 10 (K = 320 on one group); layer-3 backward G = 0 (20 tiles: pick_nt_bwd T % 20); layer 2 G = 1 ub 4
    "enc_64_320_e32": _C(_S([1, 1], [64, 320], [32], 1, 32), 64, "bce_logits"),
    # 15 input columns = d 3 x 5 frequencies; E = 64: layers 2 / 3 forward on 2 groups (kways 4)
    "enc_96_128_e64_in15_posenc": _C(_S([3], [96, 128], [32], 1, 64), 33, "bce_logits"),
    # 15 input columns without positional encoding; linear activation; layer-3 backward G = 2 ub 1 (N = 64), layer 2 G = 1 ub 1
    "enc_32_96_linear_in15": _C(_S([15], [32, 96], [16], 1, 32, pe=False, act=None), 100, "bce_logits"),
    # the widest first layer inside (154 112 B): pick_nt T % 16 at H1 = 768, layer-2 backward G = 0 (48 tiles)
    "enc_768_64": _C(_S([1], [768, 64], [32], 1, 16), 16, "bce_logits"),
    # ---- outside the encoder envelope: the grouped-GEMM path (no fused instantiation of these widths)
    # [512, 512] at E = 32: backward 178 688 B > 160 KB
    "enc_512_512_outside": _C(_S([1], [512, 512], [32], 1, 32), 16, "bce_logits", (_L(g0=3, g1=2, g2=4), _L(g0=3)), enc="gemm"),
    # [1024, 16]: forward 116 736 B fits, backward 186 880 B does not
    "enc_1024_16_outside": _C(_S([1, 1], [1024, 16], [32], 1, 8), 2, "bce_logits", (_L(g0=3, g1=2, g2=4), _L(g0=3)), enc="gemm"),
    # 16 encoder-input columns: the d(W1|b1) tile's 16th row is the bias
    "enc_in16_outside": _C(_S([16], [64, 48], [32], 1, 16, pe=False), 20, "bce_logits", (_L(g0=3, g1=2, g2=4), _L(g0=3)), enc="gemm"),
    # ---- integration network, single-workgroup kernel: pick_nt / pick_nt_bwd classes by tile count
    # 3 layers of 1 / 3 / 5 tiles (pick_nt odd), dgrads into 48 / 16 (odd) and K0 = 64 (T % 4); ragged B = 1000
    "int_16_48_80": _C(_S([1, 1, 1, 1], [16, 16], [16, 48, 80], 1, 16), 1000, "bce_logits"),
    # 7 / 10 / 20 tiles (odd, T % 2, T % 4); output layer 16 on row tiles: its dgrad into 320 (T % 20), then 160 (T % 5),
    # 112 (odd), K0 = 32 (T % 2); B = 2048
    "int_112_160_320_out16": _C(_S([1, 1], [16, 16], [112, 160, 320], 16, 16), 2048, "mse", custom=True),
    # 16 / 8 / 24 tiles (T % 16, T % 8); out_dim 48 (sparse CCE): dgrads into 384 / 128 (T % 8), 256 (T % 16)
    "int_256_128_384_out48": _C(_S([1, 1, 1, 1], [16, 16], [256, 128, 384], 48, 8), 15, "sparse_cce_logits"),
    # the widest single layer inside the 150 KB rule at K0 = 64: 704 (145 316 B; T % 4)
    "int_704_widest": _C(_S([1, 1, 1, 1], [16, 16], [704], 16, 16), 64, "mse", custom=True),
    # ... and just outside it: 720 (154 084 B) - the integration network on GEMMs, the encoders stay on row tiles
    "int_720_outside": _C(_S([1, 1, 1, 1], [16, 16], [720], 16, 16), 64, "mse", (_L(g0=2, g1=2, g2=4), _L(g0=2)), int="gemm"),
    # K0 = F E = 2048 (F = 64, E = 32): 177 828 B with a 128-wide layer - integration on GEMMs, 512 encoder workgroups on row tiles
    "int_k0_2048_outside": _C(_S([1] * 64, [16, 16], [128], 1, 32), 128, "bce_logits", (_L(g0=1, g1=1, g2=3), _L(g0=1)), int="gemm"),
    # K0 = 512; row tiles x F = 32 x 16 = 512, the last batch of the regime at the default small_wgs ...
    "regime_edge_512": _C(_S([1] * 16, [16, 16], [64], 1, 32), 512, "bce_logits"),
    # ... and B = 513: 33 x 16 = 528 workgroups, the large-batch path
    "regime_edge_513": _C(_S([1] * 16, [16, 16], [64], 1, 32), 513, "bce_logits", (_L(g0=4, g1=3, g2=4), _L(g0=4)), enc="gemm", int="gemm"),
    # small_wgs raised to 1024: 64 x 16 = 1024 (tile, feature) pairs = kSmallMaxEncWgs, the d(W1|b1) workspace at its maximum ...
    "wgs1024_clamp_1024": _C(_S([1] * 16, [16, 16], [32], 1, 8), 1024, "bce_logits", tune={"int_cluster": 1, "small_wgs": 1024}),
    # ... and 65 x 16 = 1040 pairs: beyond the clamp whatever small_wgs says
    "wgs1024_clamp_1040": _C(_S([1] * 16, [16, 16], [32], 1, 8), 1025, "bce_logits", (_L(g0=4, g1=3, g2=4), _L(g0=4)), enc="gemm",
                             int="gemm", tune={"int_cluster": 1, "small_wgs": 1024}),
    # ---- outputs
    # out_dim 2 (mse) / 5 (sparse CCE): the skinny output kernels
    "out_2_skinny": _C(_S([1, 2], [32, 32], [64], 2, 16), 16, "mse", (_L(g1=1, g2=3), _L())),
    "out_5_skinny": _C(_S([2, 2, 2], [48, 32], [80, 48], 5, 16), 1, "sparse_cce_logits", (_L(g1=2, g2=4), _L())),
    # out_dim 17: a GEMM output layer after row-tile hidden layers
    "out_17_gemm": _C(_S([1, 1], [32, 64], [96], 17, 8), 1000, "mse", (_L(g0=1, g1=2, g2=4), _L(g0=1))),
    # bce with a sigmoid output: not a piecewise-linear output activation - neither half is admitted, everything on GEMMs
    "bce_sigmoid_outside": _C(_S([1, 1], [32, 32], [32], 1, 16, out_act="sigmoid"), 17, "bce", (_L(g0=4, g1=3, g2=4), _L(g0=4)),
                              enc="gemm", int="gemm"),
    # ---- the package's default models at library defaults (they cluster): row tiles throughout
    # reference default (train.py: 10 x 1 features, [128, 128] / [256, 256], E = 32, B = 128)
    "default_reference": _C(_S([1] * 10, [128, 128], [256, 256], 1, 32), 128, "bce_logits", int="default", tune={}),
    # the pendulum layout of the InfoNCE loop (64-wide output)
    "default_pendulum": _C(_S([2, 1, 2, 1], [128, 128], [256, 256], 64, 32), 128, "mse", int="default", tune={}, custom=True),
    # the 10-input Boolean circuit with the notebook's leaky_relu and batch 512
    "default_circuit": _C(_S([1] * 10, [128, 128], [256, 256], 1, 32, act="leaky_relu"), 512, "bce_logits", int="default", tune={}),
    # ---- cluster mode against the oracle directly (int_cluster_min_weights 0)
    # cl 2: slices of 6 (192) and 10 (320) tiles -> G = 2; K0 = 224 -> 7 tiles a slice -> G = 0; out 16 -> an empty slice, ub 10
    "cl2_192_320": _C(_S([1] * 7, [16, 16], [192, 320], 16, 32), 37, "mse", int="cl",
                      tune={"int_cluster": 2, "int_cluster_min_weights": 0}, custom=True),
    # cl 4: 48 and K0 = 32 have fewer tiles than workgroups (empty slices), ub 8
    "cl4_48_64": _C(_S([1, 1, 1, 1], [16, 16], [48, 64], 64, 8), 16, "mse", int="cl", tune={"int_cluster": 4, "int_cluster_min_weights": 0}),
    # cl 8: 384 -> 3 tiles a slice, the 128-wide layer's forward (K = 384) ub 16; K0 = 64 -> empty slices; the 1-unit head
    "cl8_384_128": _C(_S([1, 1], [16, 16], [384, 128], 1, 32), 100, "bce_logits", int="cl",
                      tune={"int_cluster": 8, "int_cluster_min_weights": 0}),
    # cl 4 on the agent-scope exchange: 576 -> 9 tiles a slice: the output layer's dgrad G = 0
    "cl4_576_agent_scope": _C(_S([1] * 8, [16, 16], [576], 16, 8), 37, "mse", int="cl",
                              tune={"int_cluster": 4, "int_cluster_min_weights": 0, "int_cluster_short_exchange": 0}, custom=True),
    # cl 4: K0 = 512 -> 8 tiles a slice: the dgrad into u G = 2
    "cl4_k0_512": _C(_S([1] * 8, [16, 16], [64], 16, 64), 16, "sparse_cce_logits", int="cl",
                     tune={"int_cluster": 4, "int_cluster_min_weights": 0}),
}

# what the table must reach (unreachable returns of pick_nt / pick_nt_bwd excluded)
REQUIRED = ({"enc.l1." + c for c in ("nt4:T%16", "nt2:T%8", "nt1:T%4", "nt2:T%2", "nt1:odd")}
            | {f"enc.fwdcols.{k}" for k in ("nt1", "nt2", "nt4", "kw2", "kw4", "kw8", "ub8", "ub10", "ub16")}
            | {f"enc.bwdcols.{k}" for k in ("G0", "G1", "G2", "ub1", "ub2", "ub4")}
            | {"int.fwd." + c for c in ("nt4:T%16", "nt2:T%8", "nt1:T%4", "nt2:T%2", "nt1:odd")}
            | {"bwd." + c for c in ("nt5:T%20", "nt4:T%16", "nt2:T%8", "nt1:T%4", "nt5:T%5", "nt2:T%2", "nt1:odd")}
            | {"cl.empty", "cl.fwdcols.ub8", "cl.fwdcols.ub10", "cl.fwdcols.ub16"}
            | {f"cl.bwdcols.G2:{t}" for t in (6, 8, 10)} | {"cl.bwdcols.G0:7", "cl.bwdcols.G0:9"})


def _int_lds(K0, units, out):   # csrc/host/layout.h sb_int_lds (bytes) of the single-workgroup integration kernel
    pitch = lambda w: (w + 63) // 64 * 64 + 4   # noqa: E731 (dib_small_pitch)
    fl = 16 * pitch(K0) + sum(2 * 16 * pitch(w) for w in units) + 16 * pitch(out) + 4 * 5 * 64 * 4 + 9 * (units[-1] + 1) + 32
    return 4 * fl


def test_case_table_reaches_every_branch():
    hit = set().union(*(_branches(c) for c in CASES.values()))
    assert REQUIRED <= hit, sorted(REQUIRED - hit)
    # cluster mode is not visible in the launch counts: its cases must leave room for the 20 KB wider exchange buffer
    for name, c in CASES.items():
        if c.int == "cl":
            s = c.spec
            lds = _int_lds(s.number_features * s.feature_embedding_dimension, list(s.integration_network_architecture),
                           s.output_dimensionality)
            assert lds + 20480 <= 160 * 1024, (name, lds)


# ---- running a case ----------------------------------------------------------------------------------------------------

def _close(got, ref, tol=2e-4):
    got = np.asarray(got, dtype=np.float64)
    return np.abs(got - ref).max() <= tol * (1.0 + np.abs(ref).max())


def _grads_close(eng, gflat, grads, tol=3e-4):
    gref = params_to_flat(eng.blocks, grads, eng.params.numel()).astype(np.float64)
    for b in eng.blocks:
        sl = slice(b["offset"], b["offset"] + b["rows"] * b["cols"])
        err = np.abs(gflat[sl] - gref[sl]).max()
        assert err <= tol * (np.abs(gref[sl]).max() + 1e-3), (b, err, np.abs(gref[sl]).max())


def _counts(eng):
    """launches per category since profile_enable(True), then re-armed"""
    got = _L()
    for name, (_, n) in eng.profile_summary().items():
        if name.startswith("dib_gemm_kernel<"):
            got["g" + name[len("dib_gemm_kernel<")]] += n
        elif name.startswith("dib_fused_encoder_"):
            got["fused"] += n
    eng.profile_enable(True)
    return got


@pytest.fixture
def tuning():
    from dib_amd import _lib
    saved = {}

    def set_(kv):
        for k, v in kv.items():
            saved.setdefault(k, _lib.get_tuning(k))
            _lib.set_tuning(k, v)
    yield set_
    for k, v in saved.items():
        _lib.set_tuning(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_row_tile_envelope_step_matches_oracle(name, tuning):
    from dib_amd.engine import HipEngine
    case = CASES[name]
    spec, B, kind = case.spec, case.B, case.kind
    tuning(case.tune)   # before the engine: the layout reads its switches when it is created
    seed = zlib.crc32(name.encode()) % 1000
    eng = HipEngine(**spec_kwargs(spec), init_seed=seed)
    eng.set_flat_params(params_to_flat(eng.blocks, random_params(spec, seed), eng.params.numel()))
    p = flat_to_params(eng.blocks, eng.get_flat_params(), spec)
    if name.startswith(("enc_96_128", "enc_32_96")):   # the encoder input is exactly 15 columns wide
        assert all(b["rows"] == 15 for b in eng.blocks if b["net"] == 0 and b["layer"] == 0 and b["what"] == 0)
    F, E = spec.number_features, spec.feature_embedding_dimension
    rng = np.random.default_rng(B + seed)
    n = B + 7
    x = rng.standard_normal((n, sum(spec.feature_dimensionalities))).astype(np.float32)
    if kind in ("bce_logits", "bce"):
        y = rng.integers(0, 2, (n, 1)).astype(np.float32)
    elif kind == "mse":
        y = rng.standard_normal((n, spec.output_dimensionality)).astype(np.float32)
    else:
        y = rng.integers(0, spec.output_dimensionality, (n, 1)).astype(np.float32)
    rows = rng.permutation(n)[:B].astype(np.int32)
    xd, yd, idx = eng.to_device(x), eng.to_device(y), eng.to_device(rows, dtype=torch.int32)
    beta, step = 0.29, 4
    eng.set_beta(beta)
    train_exp, eval_exp = case.expect
    eng.profile_enable(True)
    try:
        eng.train_step(xd, yd, idx, 0, B, 11, step, kind)
        torch.cuda.synchronize()
        got = _counts(eng)
        assert got == train_exp, ("train path", got)
        rec = dict(enc_out=eng.enc_out(B).cpu().numpy(), u=eng.u(B).cpu().numpy(), pred=eng.pred(B).cpu().numpy(),
                   so=eng.step_out(B).cpu().numpy(), g_u=eng.g_u(B).cpu().numpy(), grads=eng.get_flat_grads())
        if case.int == "cl" or case.tune == {}:   # a clustered step again: the same bits (self-cleaning counters, fixed sum order)
            eng.train_step(xd, yd, idx, 0, B, 11, step, kind)
            torch.cuda.synchronize()
            _counts(eng)
            again = dict(enc_out=eng.enc_out(B).cpu().numpy(), u=eng.u(B).cpu().numpy(), pred=eng.pred(B).cpu().numpy(),
                         so=eng.step_out(B).cpu().numpy(), g_u=eng.g_u(B).cpu().numpy(), grads=eng.get_flat_grads())
            for k in rec:
                assert np.array_equal(rec[k], again[k]), ("replay", k)
        # validation step at its own noise step
        eng.eval_step(xd, yd, idx, 0, B, 11, step + 3, kind)
        torch.cuda.synchronize()
        ev = _counts(eng)
        val_pred = eng.pred(B).cpu().numpy()
        if case.custom:   # the custom-loss entry: dL/dpred given
            gp = (np.sin(np.arange(B * spec.output_dimensionality)).reshape(B, -1) / B).astype(np.float32)
            eng.forward(xd, idx, 0, B, 11, step + 5)
            eng.backward_from_pred_grad(eng.to_device(gp), idx, 0, B, 11, step + 5)
            torch.cuda.synchronize()
            cu = _counts(eng)
            custom = dict(pred=eng.pred(B).cpu().numpy(), g_u=eng.g_u(B).cpu().numpy(), grads=eng.get_flat_grads())
    finally:
        eng.profile_enable(False)
    assert ev == eval_exp, ("eval path", ev)

    xr = x[rows].astype(np.float64)
    c = orc.forward(spec, p, xr, orc.philox_normal_all(11, step, rows, F, E))
    task, grads, g_u = orc.backward(spec, p, xr, y[rows], c, beta, kind)
    assert _close(rec["enc_out"][:, :, :E], c.mu), "mu"
    assert _close(rec["enc_out"][:, :, E:], c.logvar), "logvar"
    assert _close(rec["u"], c.u), "u"
    assert _close(rec["pred"], c.pred), "pred"
    so = rec["so"]
    assert np.abs(so[:F] / B - c.kl).max() < 1e-3, "KL per feature (nats)"
    assert abs(so[F] / B - task) < 2e-4 * (1 + abs(task)), "task loss"
    assert so[F + 2] == B
    assert _close(rec["g_u"], g_u, 3e-4), "g_u"
    _grads_close(eng, rec["grads"], grads)

    cv = orc.forward(spec, p, xr, orc.philox_normal_all(11, step + 3, rows, F, E))
    assert _close(val_pred, cv.pred), "validation pred"

    if case.custom:
        assert cu == train_exp, ("custom-loss path", cu)
        cc = orc.forward(spec, p, xr, orc.philox_normal_all(11, step + 5, rows, F, E))
        grads_c, g_u_c = backward_from_pred_grad(spec, p, cc, gp.astype(np.float64), beta, 1.0 / B)
        assert _close(custom["pred"], cc.pred), "custom pred"
        assert _close(custom["g_u"], g_u_c, 3e-4), "custom g_u"
        _grads_close(eng, custom["grads"], grads_c)


def _mlp_lds(K0, units, out):   # csrc/host/small.h mlp_small_lds_floats (bytes): dib_mlp_small_fwd launches the same kernel
    pitch = lambda w: (w + 63) // 64 * 64 + 4   # noqa: E731 (dib_small_pitch)
    return 4 * (16 * pitch(K0) + sum(2 * 16 * pitch(w) for w in units) + 16 * pitch(out) + 4 * 5 * 64 * 4)


@pytest.mark.gpu
def test_one_kernel_launched_with_two_lds_sizes_keeps_the_larger_limit(tuning):
    """The dynamic-LDS limit above 64 KB is an attribute of the KERNEL FUNCTION (csrc/host/common.h launch_lds), and
    dib_small_integration_kernel is launched from three places: the layout's integration network, dib_mlp_small_fwd / _bwd and
    dib_mlp_small_head_step.  In one process: a layout step that needs 146 596 B, then a plain MLP that needs 95 744 B - more than
    64 KB, less than the layout - then the layout step again.  A cache per call site would have the second call "raise" the limit to
    its own, smaller size while the first site still believed in its own; with one high-water mark per kernel the limit only goes up.
    Every call returns DIB_OK (check() raises otherwise: a refused launch is an error code) and the two layout steps give the same
    bits."""
    import ctypes
    from dib_amd.dense import DenseStack
    from dib_amd.engine import HipEngine
    spec, B, mlp_units, mlp_out = _S([1, 1, 1, 1], [16, 16], [384, 384], 1, 32), 32, [256, 256], 16
    int_lds = _int_lds(4 * 32, [384, 384], 1)
    mlp_lds = _mlp_lds(2, mlp_units, mlp_out)
    assert 64 * 1024 < mlp_lds < int_lds <= 150 * 1024, (mlp_lds, int_lds)
    tuning({"int_cluster": 0})   # the plain dib_small_integration_kernel, not its cluster variant (a kernel of its own)
    eng = HipEngine(**spec_kwargs(spec), init_seed=5)
    eng.set_flat_params(params_to_flat(eng.blocks, random_params(spec, 5), eng.params.numel()))
    eng.set_beta(0.29)
    rng = np.random.default_rng(5)
    xd = eng.to_device(rng.standard_normal((B, 4)).astype(np.float32))
    yd = eng.to_device(rng.integers(0, 2, (B, 1)).astype(np.float32))

    def layout_step():
        eng.profile_enable(True)
        try:
            eng.train_step(xd, yd, None, 0, B, 11, 4, "bce_logits")
            torch.cuda.synchronize()
            assert _counts(eng) == ROW[0]   # integration network and head on the row-tile kernel: the merged wgrad is the only GEMM
        finally:
            eng.profile_enable(False)
        return dict(pred=eng.pred(B).clone(), so=eng.step_out(B).clone(), g_u=eng.g_u(B).clone(), grads=eng.grads.clone())

    first = layout_step()
    stack = DenseStack(eng, 2, mlp_units, mlp_out, activation="relu", use_positional_encoding=False, seed=3)
    assert eng.lib.dib_mlp_small_supported(ctypes.byref(stack._desc), B) == 1
    out = stack.forward(eng.to_device(rng.standard_normal((B, 2)).astype(np.float32)))   # dib_mlp_small_fwd, checked
    torch.cuda.synchronize()
    assert stack._last["small"] and out.shape == (B, mlp_out) and torch.isfinite(out).all()
    again = layout_step()
    for k in first:
        assert torch.equal(first[k], again[k]), k
    assert torch.isfinite(first["grads"]).all()


# ---- the paired grid (dib_integration_fwd_and_mlp_fwd / dib_backward_and_mlp_bwd) against the oracle ------------------------
PAIRS = {
    # X model below int_cluster_min_weights next to a small output encoder: the plain paired kernel (one workgroup per tile)
    "plain_pair": (orc.DIBSpec([4, 2], [32, 64], [64], 16, use_positional_encoding=False, feature_embedding_dimension=16),
                   [128, 128], 37),
    # the pendulum X model clusters, so does a [256, 256] output encoder: the cluster paired kernel
    "cluster_pair": (orc.DIBSpec([2, 1, 2, 1], [128, 128], [256, 256], 64, feature_embedding_dimension=32), [256, 256], 128),
    # ... next to a [384, 384, 128] output encoder of 145 408 B (<= 150 KB on its own): with the 20 KB cluster exchange buffer the
    # paired grid would need 165 888 B - over the 160 KB a workgroup may have: both networks one workgroup per tile instead
    "wide_companion": (orc.DIBSpec([2, 1, 2, 1], [128, 128], [256, 256], 64, feature_embedding_dimension=32), [384, 384, 128], 128),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PAIRS))
def test_paired_grid_matches_oracle(name):
    from dib_amd.dense import DenseStack
    from dib_amd.engine import HipEngine
    spec, units, B = PAIRS[name]
    eng = HipEngine(**spec_kwargs(spec), init_seed=3)
    eng.set_flat_params(params_to_flat(eng.blocks, random_params(spec, 3), eng.params.numel()))
    p = flat_to_params(eng.blocks, eng.get_flat_params(), spec)
    beta = 0.05
    eng.set_beta(beta)
    D = spec.output_dimensionality
    ds = DenseStack(eng, 6, units, D, "relu", True, 5, seed=9)
    L = len(units) + 1
    rng = np.random.default_rng(B)
    for l in range(L):
        ds.bias(l).copy_(torch.tensor(rng.standard_normal(ds.dims[l][1]) * 0.1, dtype=torch.float32))
    nin = sum(spec.feature_dimensionalities)
    x = rng.standard_normal((B + 5, nin)).astype(np.float32)
    ytab = rng.standard_normal((B + 5, 6)).astype(np.float32)
    rows = rng.permutation(B + 5)[:B].astype(np.int32)
    gp = (rng.standard_normal((B, D)) / B).astype(np.float32)
    gy = (rng.standard_normal((B, D)) / B).astype(np.float32)
    xd, yd, idx = eng.to_device(x), eng.to_device(ytab), eng.to_device(rows, dtype=torch.int32)
    eng.profile_enable(True)
    try:
        comp = ds.companion_forward(yd, rows=idx)
        assert comp is not None, "the output encoder takes the row-tile kernels"
        eng.forward(xd, idx, 0, B, 7, 3, companion=comp)
        emb_y = ds.companion_output().cpu().numpy()
        pred = eng.pred(B).cpu().numpy()
        compb = ds.companion_backward(eng.to_device(gy))
        eng.backward_from_pred_grad(eng.to_device(gp), idx, 0, B, 7, 3, inv_global_batch=1.0 / B, companion=compb)
        ds.backward(eng.to_device(gy), dgrad_done=True)
        torch.cuda.synchronize()
        cnt = _counts(eng)
    finally:
        eng.profile_enable(False)
    xg, yg, g_u = eng.get_flat_grads(), ds.grads.cpu().numpy(), eng.g_u(B).cpu().numpy()
    # X model: float64 oracle from the given dL/dpred
    xr = x[rows].astype(np.float64)
    c = orc.forward(spec, p, xr, orc.philox_normal_all(7, 3, rows, spec.number_features, spec.feature_embedding_dimension))
    grads, g_u_ref = backward_from_pred_grad(spec, p, c, gp.astype(np.float64), beta, 1.0 / B)
    assert _close(pred, c.pred), "pred"
    assert _close(g_u, g_u_ref, 3e-4), "g_u"
    _grads_close(eng, xg, grads)
    # output encoder: float64 NumPy (the restatement of test_dense_stack_row_tile_kernels)
    h = orc.positional_encoding(ytab[rows].astype(np.float64), [2 ** k for k in range(1, 5)])
    Ws = [ds.kernel(l).cpu().numpy().astype(np.float64) for l in range(L)]
    bs = [ds.bias(l).cpu().numpy().astype(np.float64) for l in range(L)]
    hs = [h]
    for l in range(L):
        z = hs[-1] @ Ws[l] + bs[l]
        hs.append(np.maximum(z, 0) if l < L - 1 else z)
    ref_g = np.zeros(ds.n_params)
    gg = gy.astype(np.float64)
    for l in reversed(range(L)):
        i, o_ = ds.dims[l]
        ref_g[ds.w_off[l]: ds.w_off[l] + i * o_] = (hs[l].T @ gg).reshape(-1)
        ref_g[ds.b_off[l]: ds.b_off[l] + o_] = gg.sum(0)
        if l > 0:
            gg = (gg @ Ws[l].T) * (hs[l] > 0)
    assert np.abs(emb_y - hs[-1]).max() < 2e-5 * (1 + np.abs(hs[-1]).max()), "output encoder forward"
    assert np.abs(yg - ref_g).max() < 2e-4 * (1 + np.abs(ref_g).max()), "output encoder gradients"
    # the X model on row tiles throughout (the output encoder's weight gradients are its own grouped GEMMs)
    assert cnt["g0"] == cnt["g1"] == cnt["fused"] == 0, cnt
