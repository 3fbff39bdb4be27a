"""The set-transformer kernels (include/dib_st.h over csrc/dib_attn.h, csrc/dib_attn_small.h, csrc/dib_st_chain.h) across the
envelope their entry points admit, against float64 computed from the same float32 inputs.

A. dib_attention_fwd / _bwd: particle counts on both sides of the 64-particle single-workgroup path, the 32-key tiles, the
   128-key dQ blocks and the 256-query 8-wave forward; 1 / 3 / 12 heads, 1 / 3 neighbourhoods; a padded leading dimension;
   three softmax scales; five score regimes (below); every switch that applies (score stash / recompute, attn_fwd_waves 8 / 4,
   attn_small_bwd_waves 8 / 4).  Memory: NaN in the inputs' padding columns and guard rows, sentinels in the outputs' padding
   columns and guard regions, a NaN-filled workspace and stash, and two identical calls bit-identical.
B. dib_attention_fwd_proj / _bwd_proj: a padded x (NaN padding), distinct non-zero weight / bias offsets, dx slabs further apart
   than B P 32 with sentinels between them, slab 0 untouched; a rising regime reached through the scale of W_q / W_k.
C. dib_st_chain_fwd / _bwd against tests/_oracle_st_chain.py: model widths 32 .. 256, 1 - 3 feed-forward layers whose widths
   reach every dib_small_pick_nt / pick_nt_bwd class, the three activations, 1 .. 4096 tokens, 1 - 13 gradient slabs, the
   admitted LDS-gate edge; host-side refusals (nothing is launched).
D. SetTransformerDIB against oracle/set_transformer_oracle.py at architectures other than the notebook's, each asserting the
   plan branch it is there for.

Score regimes of A (scores = scale q.k):
  diffuse      q, k ~ 0.5 N(0, 1): the inputs of the older tests (score std 0.25 at scale 1/sqrt(128)).
  rising       score(p, j) ~ a_p 7 min(j / 32, 6), a_p in [1, 1.5]: every query's maximum jumps by more than 6 on each of the
               first six key tiles, so the flash forward's lazy rescale (kLazy = 6) runs on later tiles.
  sharp        q, k ~ N(0, s^2) with score std 15: each query's maximum lies in a random tile, most probabilities underflow.
  late_onehot  the last key (in the last, usually partial, tile) beats every other key by >= 30 for three queries in four; the
               fourth query stays diffuse (so dq / dk keep a scale of their own).
  mixed        even queries rising, odd queries falling: lanes of one wave disagree on `moved`.

Tolerances (eps = 2^-24, the float32 unit round-off).  A float32 score s = scale sum_d q_d k_d of 128 terms is off by at most a
few sqrt(128) eps of Smag = max_{p,j} scale sum_d |q_pd k_jd| (the largest sum of absolute terms the kernel adds); each
probability then carries a relative error of that size (plus its own exp round-off), and o, lse, dq, dk, dv are sums weighted by
those probabilities.  So every output is compared at  rel = min(1e-3, 256 eps (1 + Smag))  of its reference's max-abs (256: the
sqrt(128) of the dot products with a margin of 20 for the exponentials, the rescales and the fp32 sums over up to 2049 keys).
Two outputs are exact cancellations and are compared against the round-off that decides them instead:
  - dq / dk of a one-particle neighbourhood (the gradient of a softmax over one key, identically 0): the round-off of
    1 - exp(s - lse), 256 eps (1 + Smag) scale max|k| max|dP|;
  - late_onehot, dk of the dominant key: every saturated query adds scale q_p p*(dP* - delta_p) with p* = 1 - e^-30 in exact
    arithmetic, but p* = exp(s - lse) carries the round-off of lse (|lse| ~ 48: a few eps (1 + Smag)), so the row is
    bounded by 16 eps (1 + Smag) scale max|dP| max_neighbourhood sum_p max_d |q_pd|; the other keys' rows keep the rel rule.
The chain and the model have their tolerances in the docstrings of their tests.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

EPS32 = 2.0 ** -24
SENT = -12345.5                      # sentinel of output padding / guard regions (exact in float32)
GUARD = 64                           # guard floats behind every buffer
S128 = 1.0 / math.sqrt(128.0)
D_ATT = 128

# ---- the dispatch rules, restated ONLY to check that the case tables reach each branch --------------------------------------


def attn_fwd_path(P, fwd_waves=8):
    """csrc/host/st.h dib_attention_fwd"""
    if P <= 64:
        return "small"
    return "flash8" if fwd_waves == 8 and P >= 256 else "flash4"


def attn_bwd_path(P, small_waves=8):
    """csrc/host/st.h dib_attention_bwd: the single-workgroup kernel (8 or 4 waves) or the flash kernel (+ dQ reduce)"""
    if P <= 64:
        return "small8" if small_waves >= 8 else "small4"
    return "flash_dq_reduce" if (P + 127) // 128 > 1 else "flash_one_key_block"


def pick_nt(n):   # dib_small_pick_nt (its fourth return is unreachable)
    if n % 64 == 0 and (n // 64) % 4 == 0:
        return "nt4:T%16"
    if n % 32 == 0 and (n // 32) % 4 == 0:
        return "nt2:T%8"
    if (n // 16) % 4 == 0:
        return "nt1:T%4"
    if n % 32 == 0:
        return "nt2:T%2"
    return "nt1:odd"


def pick_nt_bwd(kin):   # dib_small_pick_nt_bwd
    t = kin // 16
    for m, name in ((20, "nt5:T%20"), (16, "nt4:T%16"), (8, "nt2:T%8"), (4, "nt1:T%4"), (5, "nt5:T%5"), (2, "nt2:T%2")):
        if t % m == 0:
            return name
    return "nt1:odd"


PICK_NT = {"nt4:T%16", "nt2:T%8", "nt1:T%4", "nt2:T%2", "nt1:odd"}
PICK_NT_BWD = {"nt5:T%20", "nt4:T%16", "nt2:T%8", "nt1:T%4", "nt5:T%5", "nt2:T%2", "nt1:odd"}


def _pitch(w):   # dib_small_pitch
    return (w + 63) // 64 * 64 + 4


XCH = 4 * 5 * 64 * 4   # DIB_SMALL_XCH_FLOATS
LDS_GATE = 150 * 1024


def st_chain_fwd_lds(D, HK, ff):
    return 4 * (16 * (_pitch(HK) + 2 * _pitch(D)) + XCH + sum(16 * _pitch(w) for w in ff))


def st_chain_bwd_lds(D, HK, ff):
    return 4 * (16 * (4 * _pitch(D) + 2 * D) + XCH + sum(2 * 16 * _pitch(w) for w in ff))


def st_chain_supported(D, HK, ff, act, T, small_batch=1):
    """csrc/host/st.h dib_st_chain_supported"""
    if T <= 0 or not small_batch:
        return False
    if D <= 0 or D % 32 or D > 256 or HK <= 0 or HK % 16 or not 1 <= len(ff) <= 3:
        return False
    if not 0 <= act <= 2 or any(w <= 0 or w % 16 or w > 1024 for w in ff) or ff[-1] != D or T > 4096:
        return False
    return st_chain_fwd_lds(D, HK, ff) <= LDS_GATE and st_chain_bwd_lds(D, HK, ff) <= LDS_GATE


def chain_branches(D, HK, ff):
    """the width-dependent code of csrc/dib_st_chain.h a shape runs: pick_nt of every forward product (output projection N = D,
    layer l N = ff[l]), pick_nt_bwd of every dgrad (Kin = ff[l - 1], D, HK), LayerNorm columns per lane, combine chunks"""
    fwd = {pick_nt(n) for n in [D] + list(ff)}
    bwd = {pick_nt_bwd(k) for k in list(ff[:-1]) + [D, HK]}
    return fwd, bwd, (D + 31) // 32, max(1, 512 // (4 * D))


# ---- A. attention case table -----------------------------------------------------------------------------------------------
# (B, P, H, pad, scale, regime)
ATTN = [
    (1, 1, 1, 0, S128, "diffuse"),
    (3, 2, 3, 4, 1.0, "sharp"),
    (2, 31, 12, 128, 0.02, "diffuse"),
    (1, 32, 3, 4, S128, "late_onehot"),
    (3, 33, 1, 0, S128, "sharp"),
    (2, 63, 3, 128, 1.0, "mixed"),
    (3, 64, 12, 4, S128, "rising"),
    (2, 65, 3, 4, S128, "rising"),
    (1, 65, 1, 0, 0.02, "late_onehot"),
    (1, 127, 1, 128, 0.02, "late_onehot"),
    (3, 128, 3, 0, 1.0, "mixed"),
    (1, 129, 12, 4, S128, "sharp"),
    (2, 129, 1, 0, S128, "diffuse"),
    (2, 255, 1, 128, S128, "rising"),
    (1, 256, 3, 4, 0.02, "mixed"),
    (3, 257, 1, 0, S128, "late_onehot"),
    (2, 300, 3, 128, 1.0, "diffuse"),
    (1, 300, 1, 4, S128, "sharp"),
    (1, 1100, 3, 4, S128, "mixed"),
    (1, 1100, 1, 0, 0.02, "rising"),
    (1, 2049, 1, 128, S128, "late_onehot"),
    (1, 2049, 1, 4, 1.0, "rising"),
    (1, 2049, 1, 0, S128, "sharp"),
    (1, 2049, 1, 4, 0.02, "mixed"),
]
ATTN_IDS = [f"B{b}_P{p}_H{h}_pad{pd}_s{s:.3g}_{r}" for b, p, h, pd, s, r in ATTN]


def attn_configs(P):
    """(stash, attn_fwd_waves, attn_small_bwd_waves) runs of one case: every switch that changes the code that runs"""
    if P <= 64:
        return [(False, 8, 8), (False, 8, 4)]
    if P >= 256:
        return [(True, 8, 8), (False, 8, 8), (True, 4, 8), (False, 4, 8)]
    return [(True, 8, 8), (False, 8, 8)]


# ---- C. token-chain case table ---------------------------------------------------------------------------------------------
# name: (D, HK, ff widths, act, T, g_out slabs)
CHAIN = {
    "d32_hk16_ff32_linear_t1": (32, 16, [32], 0, 1, 1),
    "d32_hk1536_notebook_t4096_13slabs": (32, 1536, [128, 32], 1, 4096, 13),
    "d32_hk384_ff3_leaky_t15": (32, 384, [48, 320, 32], 2, 15, 2),
    "d64_hk128_leaky_t200_13slabs": (64, 128, [128, 64], 2, 200, 13),
    "d64_hk384_ff3_relu_t17": (64, 384, [80, 192, 64], 1, 17, 5),
    "d96_hk384_ff1_leaky_t16": (96, 384, [96], 2, 16, 5),
    "d96_hk16_linear_t200": (96, 16, [320, 96], 0, 200, 1),
    "d128_hk1536_ff1_relu_t200": (128, 1536, [128], 1, 200, 2),
    "d128_hk128_w256_leaky_t17": (128, 128, [256, 128], 2, 17, 13),
    "d128_hk16_linear_t4096": (128, 16, [512, 128], 0, 4096, 5),
    "d256_hk128_gate_edge_relu_t200": (256, 128, [256], 1, 200, 13),
    "d256_hk16_leaky_t1": (256, 16, [256], 2, 1, 2),
    "d256_hk384_linear_t4096": (256, 384, [256], 0, 4096, 1),
    "d64_hk1536_relu_t16": (64, 1536, [64], 1, 16, 2),
    "d32_hk128_w400_leaky_t15": (32, 128, [400, 32], 2, 15, 1),
    "d64_hk16_w768_gate_exact_leaky_t17": (64, 16, [768, 64], 2, 17, 2),   # 153 600 B: exactly the gate
}

# refused shapes: (name, D, HK, ff, act, T, kwargs of the call) - every one rejected before a launch
REFUSALS = [
    ("t4097", 32, 128, [128, 32], 1, 4097, {}),
    ("d48", 48, 128, [48], 1, 16, {}),
    ("d288", 288, 128, [288], 1, 16, {}),
    ("hk24", 32, 24, [32], 1, 16, {}),
    ("width1040", 32, 128, [1040, 32], 1, 16, {}),
    ("act3", 32, 128, [32], 3, 16, {}),
    ("nff0", 32, 128, [], 1, 16, {}),
    ("nff4", 32, 128, [32, 32, 32, 32], 1, 16, {}),
    ("last_width_not_d", 32, 128, [128, 64], 1, 16, {}),
    ("lds_over_gate_bwd", 32, 128, [784, 32], 1, 16, {}),
    ("lds_over_gate_fwd", 256, 1296, [256], 1, 16, {}),
    ("small_batch_0", 32, 128, [128, 32], 1, 16, {"small_batch": 0}),
    ("slab_stride_below_td", 32, 128, [128, 32], 1, 16, {"slabs": 2, "stride": 16 * 32 - 4}),
    ("misaligned_g_out", 32, 128, [128, 32], 1, 16, {"g_off": 1}),
]


def test_case_tables_reach_every_branch():
    """The case tables of A and C against the dispatch rules above: every attention path for every regime, both sides of
    every particle-count limit, every chain dimension value, every pick_nt / pick_nt_bwd class, LayerNorm tiles with several
    columns per lane and the one-chunk combine, the admitted gate edge, and every refusal refused by the rules."""
    paths = {}
    for B, P, H, pad, scale, regime in ATTN:
        for stash, fw, bw in attn_configs(P):
            paths.setdefault(regime, set()).update({attn_fwd_path(P, fw), attn_bwd_path(P, bw)})
    for regime, got in paths.items():
        assert {"small", "flash4"} <= got, (regime, got)
    assert all(any(p in got for got in paths.values()) for p in
               ("small", "flash4", "flash8", "small8", "small4", "flash_dq_reduce", "flash_one_key_block"))
    for reg in ("rising", "sharp", "late_onehot", "mixed", "diffuse"):
        assert "flash8" in paths[reg] or reg == "diffuse", reg
    Ps = {c[1] for c in ATTN}
    assert {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 1100, 2049} <= Ps
    assert {c[2] for c in ATTN} == {1, 3, 12} and {1, 3} <= {c[0] for c in ATTN}
    assert {c[3] for c in ATTN} == {0, 4, 128} and {round(c[4], 6) for c in ATTN} == {round(S128, 6), 1.0, 0.02}
    for pad in (0, 4, 128):   # a padded leading dimension on both kernels families
        assert {attn_fwd_path(c[1]) == "small" for c in ATTN if c[3] == pad} == {True, False}, pad
    fwd, bwd, cols, nch, edge, exact = set(), set(), set(), set(), 0, 0
    for name, (D, HK, ff, act, T, slabs) in CHAIN.items():
        assert st_chain_supported(D, HK, ff, act, T), name
        f, b, c, n = chain_branches(D, HK, ff)
        fwd |= f; bwd |= b; cols.add(c); nch.add(n)
        edge += st_chain_bwd_lds(D, HK, ff) > 149 * 1024
        exact += st_chain_bwd_lds(D, HK, ff) == LDS_GATE
    assert fwd == PICK_NT and bwd == PICK_NT_BWD, (PICK_NT - fwd, PICK_NT_BWD - bwd)
    assert {1, 2, 8} <= cols and nch == {1, 2, 4} and edge >= 2 and exact >= 1
    vals = list(zip(*CHAIN.values()))
    assert set(vals[0]) == {32, 64, 96, 128, 256} and set(vals[1]) == {16, 128, 384, 1536}
    assert {len(f) for f in vals[2]} == {1, 2, 3} and set(vals[3]) == {0, 1, 2}
    assert set(vals[4]) == {1, 15, 16, 17, 200, 4096} and set(vals[5]) == {1, 2, 5, 13}
    # the documented gate-edge numbers
    assert st_chain_bwd_lds(256, 128, [256]) == 153088 and st_chain_fwd_lds(256, 1536, [256]) == 168960
    for name, D, HK, ff, act, T, kw in REFUSALS:
        refused = not st_chain_supported(D, HK, ff, act, T, kw.get("small_batch", 1))
        assert refused or set(kw) & {"slabs", "g_off"}, name
    over = [r for r in REFUSALS if r[0].startswith("lds_over")]
    assert st_chain_bwd_lds(*over[0][1:4]) > LDS_GATE >= st_chain_fwd_lds(*over[0][1:4])
    assert st_chain_fwd_lds(*over[1][1:4]) > LDS_GATE >= st_chain_bwd_lds(*over[1][1:4])
    assert st_chain_bwd_lds(*over[0][1:4]) - LDS_GATE <= 4096 and st_chain_fwd_lds(*over[1][1:4]) - LDS_GATE <= 4096   # just over


# ---- shared GPU helpers ----------------------------------------------------------------------------------------------------


def _lib():
    from dib_amd._lib import load_library
    return load_library()


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(code, what):
    from dib_amd._lib import check
    check(code, what)


def _guarded(n, fill, dev):
    """a flat float32 buffer of n floats + GUARD guard floats, all `fill`"""
    return torch.full((n + GUARD,), fill, dtype=torch.float32, device=dev)


def _guard_ok(buf, n):
    return bool((buf[n:] == SENT).all())


def _regime(regime, B, P, H, scale, g):
    """q, k, v, dO [B, P, H, 128] float32 (CPU) of a score regime (module docstring)"""
    shp = (B, P, H, D_ATT)
    rn = lambda s=1.0: torch.randn(shp, generator=g) * s
    v, do = rn(0.5), rn(0.5)
    j = torch.arange(P, dtype=torch.float64)
    ramp = 7.0 * torch.clamp(j / 32.0, max=6.0)                 # + 7 per key tile for six tiles, then flat
    rs = 1.0 / math.sqrt(scale)
    if regime == "diffuse":
        q, k = rn(0.5), rn(0.5)
    elif regime in ("rising", "mixed"):
        q, k = rn(0.1), rn(0.1)
        a = 1.0 + 0.5 * torch.rand((B, P, H), generator=g)
        if regime == "mixed":
            a = a * (1.0 - 2.0 * (torch.arange(P) % 2)).view(1, P, 1)     # odd queries: falling scores
        q[..., 0] = (a * rs).float()
        k[..., 0] = (ramp * rs).float().view(1, P, 1)
    elif regime == "sharp":
        s = math.sqrt(15.0 / (scale * math.sqrt(D_ATT)))
        q, k = rn(s), rn(s)
    elif regime == "late_onehot":
        q, k = rn(0.5), rn(0.5)
        q[..., 0] = 0.0
        k[..., 0] = 0.0
        big = math.sqrt(48.0 / scale)
        hot = (torch.arange(P) % 4 != 3).view(1, P, 1)
        q[..., 0] = torch.where(hot, torch.tensor(big), torch.tensor(0.0)).float().expand(B, P, H)
        k[:, P - 1, :, 0] = big
    else:
        raise ValueError(regime)
    return q.float().contiguous(), k.float().contiguous(), v.contiguous(), do.contiguous()


def _attn_ref(q, k, v, do, scale):
    """float64 autograd (on the device, in double) of o = softmax(scale q k^T) v: o, lse, dq, dk, dv, P, dP, Smag"""
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    dod = do.double()
    s = torch.einsum("bphd,bqhd->bhpq", qd, kd) * scale
    lse = torch.logsumexp(s, -1)
    att = torch.softmax(s, -1)
    o = torch.einsum("bhpq,bqhd->bphd", att, vd)
    gq, gk, gv = torch.autograd.grad((o * dod).sum(), [qd, kd, vd])
    smag = float((torch.einsum("bphd,bqhd->bhpq", q.double().abs(), k.double().abs()) * scale).max())
    dp = torch.einsum("bphd,bqhd->bhpq", dod, vd.detach())
    return dict(o=o.detach(), lse=lse.detach(), dq=gq, dk=gk, dv=gv, smag=smag, dpmax=float(dp.abs().max()))


def _pad_rows(x, T, ld, fill):
    """[B, P, H, 128] -> flat [(T + 2) * ld] with `fill` in the padding columns and the two guard rows"""
    H = x.shape[2]
    buf = torch.full((T + 2, ld), fill, dtype=torch.float32, device=x.device)
    buf[:T, : H * D_ATT] = x.reshape(T, H * D_ATT)
    return buf.reshape(-1)


def _unpad(buf, B, P, H, ld):
    T = B * P
    return buf[: T * ld].view(T, ld)[:, : H * D_ATT].reshape(B, P, H, D_ATT)


def _pad_ok(buf, T, H, ld):
    """output padding columns and guard rows still hold the sentinel"""
    m = buf.view(T + 2, ld)
    return bool((m[:, H * D_ATT:] == SENT).all()) and bool((m[T:] == SENT).all())


def _attn_device(lib, q, k, v, do, B, P, H, ld, scale, stash_mode):
    """one forward + backward on padded, guarded buffers; returns the output buffers"""
    dev = q.device
    T = B * P
    qb, kb, vb, dob = (_pad_rows(t, T, ld, float("nan")) for t in (q, k, v, do))
    o, dq, dk, dv = (torch.full(((T + 2) * ld,), SENT, device=dev) for _ in range(4))
    lse = _guarded(B * H * P, SENT, dev)
    nws = int(lib.dib_attention_bwd_workspace_bytes(B, P, H)) // 4
    ws = _guarded(nws, float("nan"), dev)
    ws[nws:] = SENT
    nst = int(lib.dib_attention_stash_bytes(B, P, H)) // 4
    stash = None
    if stash_mode:
        stash = _guarded(nst, float("nan"), dev)
        stash[nst:] = SENT
    sp = _p(stash) if stash is not None else ctypes.c_void_p(0)
    st = _stream()
    _check(lib.dib_attention_fwd(_p(qb), _p(kb), _p(vb), B, P, H, D_ATT, ld, scale, _p(o), _p(lse), sp, st), "fwd")
    _check(lib.dib_attention_bwd(_p(qb), _p(kb), _p(vb), _p(o), _p(dob), _p(lse), sp, B, P, H, D_ATT, ld, scale, _p(dq), _p(dk),
                                 _p(dv), _p(ws), st), "bwd")
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, ws=ws, nws=nws, stash=stash, nst=nst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ATTN, ids=ATTN_IDS)
def test_attention_envelope_matches_float64(case):
    """dib_attention_fwd / _bwd at one (B, P, H, ld, scale, regime) in every switch setting that applies, against float64
    autograd at rel = min(1e-3, 256 eps (1 + Smag)) of each reference's max-abs (module docstring); padding / guard / workspace
    checks and a bit-identical second call in every setting."""
    from dib_amd import _lib as L
    B, P, H, pad, scale, regime = case
    lib, dev = _lib(), torch.device("cuda:0")
    T, ld = B * P, H * D_ATT + pad
    g = torch.Generator(device="cpu").manual_seed(B * 100003 + P * 101 + H * 7 + pad)
    q, k, v, do = (t.to(dev) for t in _regime(regime, B, P, H, scale, g))
    ref = _attn_ref(q, k, v, do, scale)
    rel = min(1e-3, 256 * EPS32 * (1.0 + ref["smag"]))
    defaults = {key: L.get_tuning(key) for key in ("attn_fwd_waves", "attn_small_bwd_waves")}
    worst = {}
    try:
        for stash_mode, fw, bw in attn_configs(P):
            L.set_tuning("attn_fwd_waves", fw)
            L.set_tuning("attn_small_bwd_waves", bw)
            runs = [_attn_device(lib, q, k, v, do, B, P, H, ld, scale, stash_mode) for _ in range(2)]
            r = runs[0]
            tag = (stash_mode, fw, bw)
            for name in ("o", "lse", "dq", "dk", "dv"):
                assert torch.equal(r[name], runs[1][name]), (tag, name, "second call differs")
            for name in ("o", "dq", "dk", "dv"):
                assert _pad_ok(r[name], T, H, ld), (tag, name, "padding column or guard row written")
            assert _guard_ok(r["lse"], B * H * P), (tag, "lse guard written")
            assert _guard_ok(r["ws"], r["nws"]), (tag, "workspace guard written")
            if r["stash"] is not None:
                assert _guard_ok(r["stash"], r["nst"]), (tag, "stash guard written")
            got = {n: _unpad(r[n], B, P, H, ld) for n in ("o", "dq", "dk", "dv")}
            got["lse"] = r["lse"][: B * H * P].view(B, H, P)
            for name, a in got.items():
                assert torch.isfinite(a).all(), (tag, name, "non-finite output (NaN padding read?)")
                b = ref[name]
                err = float((a.double() - b).abs().max())
                if P == 1 and name in ("dq", "dk"):   # exactly 0 in exact arithmetic (module docstring)
                    other = k if name == "dq" else q
                    tol = 256 * EPS32 * (1.0 + ref["smag"]) * scale * float(other.abs().max()) * ref["dpmax"]
                elif regime == "late_onehot" and name == "dk" and P > 1:   # the dominant key's row (module docstring)
                    hot = float((a[:, P - 1].double() - b[:, P - 1]).abs().max())
                    tol_hot = 16 * EPS32 * (1.0 + ref["smag"]) * scale * ref["dpmax"] * float(q.abs().amax(-1).sum(1).max())
                    assert hot <= tol_hot, (tag, "dk of the dominant key", hot, tol_hot)
                    a, b = a[:, : P - 1], b[:, : P - 1]
                    err = float((a.double() - b).abs().max())
                    tol = rel * float(b.abs().max())
                else:
                    tol = rel * float(b.abs().max())
                worst[(tag, name)] = err / tol
                assert err <= tol, (tag, name, err, tol, float(b.abs().max()))
    finally:
        for key, val in defaults.items():
            L.set_tuning(key, val)
    print("Smag", ref["smag"], "rel", rel, "worst err / tol", max(worst.values()), max(worst, key=worst.get))


# ---- B. attention with the q / k / v projections ---------------------------------------------------------------------------
PROJ = [   # (B, P, H, ldx, regime)
    (2, 50, 12, 36, "diffuse"),
    (3, 64, 3, 40, "rising"),
    (2, 1, 2, 36, "diffuse"),
    (1, 33, 1, 48, "rising"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PROJ, ids=[f"B{c[0]}_P{c[1]}_H{c[2]}_ldx{c[3]}_{c[4]}" for c in PROJ])
def test_attention_with_projections_matches_float64(case):
    """dib_attention_fwd_proj / _bwd_proj (model width 32, ld = H 128): q, k, v = x W_i + b_i with W / b at distinct non-zero
    offsets of a parameter buffer whose other entries are NaN, x [T, ldx > 32] with NaN padding; the backward's dx slabs
    slab_stride > B P 32 floats apart with sentinels between them and in slab 0.  Against float64: q, k, v and o, lse, dq, dk,
    dv (the forward from x, the backward from the device's own q, k, v) at the attention rule of the module docstring, and each
    head's dx_h = dq_h Wq_h^T + dk_h Wk_h^T + dv_h Wv_h^T at the same rel (its 3 x 128-term sums are of the size of the dq
    products).  "rising": W_q / W_k scaled so that scores grow along the key axis (x[:, 0] = particle index / 8)."""
    B, P, H, ldx, regime = case
    lib, dev = _lib(), torch.device("cuda:0")
    T, HK, M = B * P, H * D_ATT, 32
    ld = HK
    scale = S128
    g = torch.Generator(device="cpu").manual_seed(B * 7919 + P * 31 + H)
    x = torch.randn((T, M), generator=g)
    if regime == "rising":
        x[:, 0] = (torch.arange(T) % P).float() / 8.0
    W = [torch.randn((M, HK), generator=g) * 0.2 for _ in range(3)]
    if regime == "rising":   # score(p, j) ~ 0.011 p j + O(1): up to ~40 along the key axis
        for i in (0, 1):
            W[i][0] = 0.25
    bvec = [torch.randn((HK,), generator=g) * 0.1 for _ in range(3)]
    # parameter buffer: NaN everywhere but W_q, W_k, W_v, b_q, b_k, b_v at distinct non-zero (multiple of 4) offsets
    w_off = [12, 12 + M * HK + 4, 12 + 2 * (M * HK + 4)]
    b_off = [w_off[2] + M * HK + 8, w_off[2] + M * HK + 8 + HK + 4, w_off[2] + M * HK + 8 + 2 * (HK + 4)]
    params = torch.full((b_off[2] + HK + 16,), float("nan"))
    for i in range(3):
        params[w_off[i]: w_off[i] + M * HK] = W[i].reshape(-1)
        params[b_off[i]: b_off[i] + HK] = bvec[i]
    params = params.to(dev)
    xb = torch.full((T + 2, ldx), float("nan"))
    xb[:T, :M] = x
    xb = xb.reshape(-1).to(dev)
    qo, ko, vo, o = (_guarded(T * ld, SENT, dev) for _ in range(4))
    lse = _guarded(B * H * P, SENT, dev)
    W64 = [w.double().to(dev) for w in W]
    b64 = [b.double().to(dev) for b in bvec]
    x64 = x.double().to(dev)
    wo = (ctypes.c_int64 * 3)(*w_off)
    bo = (ctypes.c_int64 * 3)(*b_off)
    st = _stream()
    assert lib.dib_attention_fwd_proj_supported(P, D_ATT, M) == 1
    _check(lib.dib_attention_fwd_proj(_p(xb), ldx, _p(params), wo, bo, B, P, H, D_ATT, M, ld, scale, _p(qo), _p(ko), _p(vo),
                                      _p(o), _p(lse), st), "fwd_proj")
    torch.cuda.synchronize()
    for name, buf in (("q", qo), ("k", ko), ("v", vo), ("o", o)):
        assert _guard_ok(buf, T * ld), (name, "guard written")
    assert _guard_ok(lse, B * H * P)
    # q, k, v: 32-term products (float32 sums of |x| |W| bounded by 64 eps of their sum of absolute terms)
    for i, (name, buf) in enumerate((("q", qo), ("k", ko), ("v", vo))):
        ref = x64 @ W64[i] + b64[i]
        tol = 64 * EPS32 * float(((x64.abs() @ W64[i].abs()) + b64[i].abs()).max())
        assert float((buf[: T * ld].view(T, ld).double() - ref).abs().max()) <= tol, name
    q, k, v = (buf[: T * ld].view(B, P, H, D_ATT).clone() for buf in (qo, ko, vo))
    ref = _attn_ref((x64 @ W64[0] + b64[0]).view(B, P, H, D_ATT).float(), (x64 @ W64[1] + b64[1]).view(B, P, H, D_ATT).float(),
                    (x64 @ W64[2] + b64[2]).view(B, P, H, D_ATT).float(), torch.zeros_like(q), scale)
    rel = min(1e-3, 256 * EPS32 * (1.0 + ref["smag"]))
    for name, a, b in (("o", o[: T * ld].view(B, P, H, D_ATT), ref["o"]), ("lse", lse[: B * H * P].view(B, H, P), ref["lse"])):
        assert float((a.double() - b).abs().max()) <= rel * float(b.abs().max()), name
    # backward from the device's q, k, v
    do = (torch.randn((B, P, H, D_ATT), generator=g) * 0.5).to(dev)
    ref = _attn_ref(q, k, v, do, scale)
    rel = min(1e-3, 256 * EPS32 * (1.0 + ref["smag"]))
    stride = T * M + 36   # > B P 32, % 4 == 0
    dx = torch.full(((H + 1) * stride + GUARD,), SENT, device=dev)
    dqb, dkb, dvb = (_guarded(T * ld, SENT, dev) for _ in range(3))
    lse_in = lse.clone()
    for rep in range(2):
        _check(lib.dib_attention_bwd_proj(_p(qo), _p(ko), _p(vo), _p(do.reshape(-1)), _p(lse_in), B, P, H, D_ATT, M, ld, scale,
                                          _p(dqb), _p(dkb), _p(dvb), _p(params), wo, _p(dx), stride, st), "bwd_proj")
        torch.cuda.synchronize()
        if rep == 0:
            first = [t.clone() for t in (dqb, dkb, dvb, dx)]
    for a, b in zip(first, (dqb, dkb, dvb, dx)):
        assert torch.equal(a, b), "second call differs"
    for name, buf in (("dq", dqb), ("dk", dkb), ("dv", dvb)):
        assert _guard_ok(buf, T * ld), (name, "guard written")
        a = buf[: T * ld].view(B, P, H, D_ATT)
        b = ref[name]
        tol = rel * float(b.abs().max()) if P > 1 or name == "dv" else \
            256 * EPS32 * (1.0 + ref["smag"]) * scale * float((k if name == "dq" else q).abs().max()) * ref["dpmax"]
        assert float((a.double() - b).abs().max()) <= tol, name
    assert bool((dx[:stride] == SENT).all()), "slab 0 written"
    assert bool((dx[(H + 1) * stride:] == SENT).all()), "guard after the last slab written"
    dxs = dx[: (H + 1) * stride].view(H + 1, stride)
    assert bool((dxs[1:, T * M:] == SENT).all()), "gap between slabs written"
    gmax = 0.0
    refs = []
    for h in range(H):
        cols = slice(h * D_ATT, (h + 1) * D_ATT)
        r = sum(ref[n][:, :, h].reshape(T, D_ATT) @ W64[i][:, cols].T for i, n in enumerate(("dq", "dk", "dv")))
        refs.append(r)
        gmax = max(gmax, float(r.abs().max()))
    for h in range(H):
        a = dxs[1 + h, : T * M].view(T, M).double()
        assert torch.isfinite(a).all(), h
        assert float((a - refs[h]).abs().max()) <= rel * gmax, (h, float((a - refs[h]).abs().max()), rel * gmax)


# ---- C. the token chain ----------------------------------------------------------------------------------------------------


def _chain_params(D, HK, ff, g):
    """float64 parameters of one block (Glorot-scale weights, non-trivial biases / LayerNorm parameters) and their element
    offsets in a flat buffer whose gaps and head are NaN-free sentinels"""
    shapes = [("o_w", (HK, D)), ("o_b", (D,)), ("ln1_g", (D,)), ("ln1_b", (D,))]
    kin = D
    for l, w in enumerate(ff):
        shapes += [(f"ff{l}_w", (kin, w)), (f"ff{l}_b", (w,))]
        kin = w
    shapes += [("ln2_g", (D,)), ("ln2_b", (D,))]
    p, off, o = {}, {}, 8
    for name, shp in shapes:
        if name.endswith("_w"):
            a = g.standard_normal(shp) * math.sqrt(2.0 / (shp[0] + shp[1])) * 1.5
        elif name.endswith("_g"):
            a = 1.0 + 0.1 * g.standard_normal(shp)
        else:
            a = 0.1 * g.standard_normal(shp)
        p[name] = a.astype(np.float32).astype(np.float64)
        off[name] = o
        o += (int(np.prod(shp)) + 3) // 4 * 4 + 4   # a 4..7-float gap behind every block
    return p, off, o + 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHAIN))
def test_token_chain_envelope_matches_float64(name):
    """dib_st_chain_fwd / _bwd on one shape of the envelope against tests/_oracle_st_chain.py (float64 from the same float32
    inputs, under the device's act' choices; those choices may differ from float64's `z > 0` only at pre-activations within
    the rounding tolerance below, and only for a handful of units).

    Tolerance: every output is a chain of at most n_ff + 2 dependent float32 contractions (output projection, the feed-forward
    layers, the LayerNorm sums; the parameter gradients add one sum over T tokens), each of at most K terms - K the largest of
    HK, D, the widths (and T for the parameter gradients).  A K-term float32 sum is within a few sqrt(K) eps of its sum of
    absolute terms; with a margin of 64 for the ratio of absolute terms to the result and LayerNorm's rstd (the inputs are O(1)),
    rel = min(1e-3, 64 eps sqrt(K) (n_ff + 2)) of each reference's max-abs.
    Memory: every output has a sentinel guard behind it, g_out's slabs are g_out_stride > T D apart with NaN in the gaps, the
    gradient buffer keeps its sentinels outside the four LayerNorm ranges, the arrival counter is back to 0 after the launch,
    and a second backward on the same workspace reproduces the first bit for bit."""
    import _oracle_st_chain as oc
    from dib_amd.set_transformer import _BlockDesc
    D, HK, ff, act, T, slabs = CHAIN[name]
    lib, dev = _lib(), torch.device("cuda:0")
    g = np.random.default_rng(D * 1000 + HK + T + slabs)
    p, off, n_par = _chain_params(D, HK, ff, g)
    flat = np.full(n_par, SENT, np.float32)
    for k_, a in p.items():
        flat[off[k_]: off[k_] + a.size] = a.ravel()
    params = torch.from_numpy(flat).to(dev)
    dsc = _BlockDesc()
    dsc.o_w, dsc.o_b, dsc.ln1_g, dsc.ln1_b, dsc.ln2_g, dsc.ln2_b = (off[k_] for k_ in ("o_w", "o_b", "ln1_g", "ln1_b", "ln2_g", "ln2_b"))
    for l, w in enumerate(ff):
        dsc.ff_w[l], dsc.ff_b[l], dsc.ff_width[l] = off[f"ff{l}_w"], off[f"ff{l}_b"], w
    dsc.n_ff, dsc.D, dsc.HK, dsc.eps, dsc.act = len(ff), D, HK, 1e-3, act
    assert lib.dib_st_chain_supported(ctypes.byref(dsc), T) == 1 and st_chain_supported(D, HK, ff, act, T)
    ctx = (g.standard_normal((T, HK)) * 0.5).astype(np.float32)
    x_in = g.standard_normal((T, D)).astype(np.float32)
    ctx_d = torch.from_numpy(ctx).to(dev)
    x_d = torch.from_numpy(x_in).to(dev)
    outs = {k_: _guarded(n, SENT, dev) for k_, n in (("h", T * D), ("xhat1", T * D), ("rstd1", T), ("x_out", T * D),
                                                     ("xhat2", T * D), ("rstd2", T))}
    ffb = [_guarded(T * w, SENT, dev) for w in ff]
    ffp = (ctypes.c_void_p * 3)(*[_p(b).value for b in ffb])
    st = _stream()
    n0 = lib.dib_launch_count()
    _check(lib.dib_st_chain_fwd(ctypes.byref(dsc), T, _p(params), _p(ctx_d), _p(x_d), _p(outs["h"]), _p(outs["xhat1"]),
                                _p(outs["rstd1"]), ffp, _p(outs["x_out"]), _p(outs["xhat2"]), _p(outs["rstd2"]), st), "chain fwd")
    torch.cuda.synchronize()
    assert lib.dib_launch_count() - n0 == 1
    for k_, b in list(outs.items()) + [(f"ff{l}", b) for l, b in enumerate(ffb)]:
        n = b.numel() - GUARD
        assert _guard_ok(b, n), (k_, "guard written")
    masks = [(b[: T * w].view(T, w) > 0).cpu().numpy() for b, w in zip(ffb, ff)]
    boundary = {}
    po = {k_: p[k_] for k_ in ("o_w", "o_b", "ln1_g", "ln1_b", "ln2_g", "ln2_b")}
    po["ff_w"], po["ff_b"] = [p[f"ff{l}_w"] for l in range(len(ff))], [p[f"ff{l}_b"] for l in range(len(ff))]
    ref = oc.chain_forward(po, ctx.astype(np.float64), x_in.astype(np.float64), 1e-3, act, masks=masks, boundary=boundary)
    K = max([HK, D] + list(ff))
    rel = min(1e-3, 64 * EPS32 * math.sqrt(K) * (len(ff) + 2))
    rel_ln = min(1e-3, 64 * EPS32 * math.sqrt(max(K, T)) * (len(ff) + 3))
    if act != 0:
        for l, (cnt, worst) in boundary.items():
            zmax = float(np.abs(ref["ff"][l]).max())
            assert cnt <= 2e-5 * masks[l].size + 2 and worst <= rel * max(zmax, 1.0), (l, cnt, worst)

    def cmp(tag, a, b, r):
        a = np.asarray(a, np.float64)
        assert np.isfinite(a).all(), tag
        err, tol = float(np.abs(a - b).max()), r * float(np.abs(b).max())
        assert err <= tol, (tag, err, tol)
        return err / tol

    worst = {}
    for k_, shp in (("h", (T, D)), ("xhat1", (T, D)), ("rstd1", (T,)), ("x_out", (T, D)), ("xhat2", (T, D)), ("rstd2", (T,))):
        worst[k_] = cmp(k_, outs[k_][: int(np.prod(shp))].view(*shp).cpu().numpy(), ref[k_], rel)
    for l, w in enumerate(ff):
        worst[f"ff{l}"] = cmp(f"ff{l}", ffb[l][: T * w].view(T, w).cpu().numpy(), ref["ff"][l], rel)
    # ---- backward ----
    gsl = [(g.standard_normal((T, D)) * (1.0 if s == 0 else 0.3)).astype(np.float32) for s in range(slabs)]
    stride = T * D + 4 * (1 + slabs % 3)            # > T D, % 4 == 0
    gout = torch.full((slabs * stride + GUARD,), float("nan"), device=dev)
    for s, a in enumerate(gsl):
        gout[s * stride: s * stride + T * D] = torch.from_numpy(a.ravel()).to(dev)
    g_ref = sum(a.astype(np.float64) for a in gsl)
    bw = oc.chain_backward(po, ref, g_ref, act)
    gff = [_guarded(T * w, SENT, dev) for w in ff]
    gfp = (ctypes.c_void_p * 3)(*[_p(b).value for b in gff])
    g_in, g_ctx = _guarded(T * D, SENT, dev), _guarded(T * HK, SENT, dev)
    grads = torch.full((n_par,), SENT, device=dev)
    nws = int(lib.dib_st_chain_workspace_bytes(T, D)) // 4
    ws = torch.zeros(nws + GUARD, device=dev)
    ws[nws:] = SENT
    tiles = (T + 15) // 16
    res = []
    for rep in range(2):
        _check(lib.dib_st_chain_bwd(ctypes.byref(dsc), T, _p(params), _p(gout), slabs, stride, _p(outs["xhat2"]), _p(outs["rstd2"]),
                                    ffp, _p(outs["xhat1"]), _p(outs["rstd1"]), gfp, _p(g_in), _p(g_ctx), _p(grads), _p(ws), st),
               "chain bwd")
        torch.cuda.synchronize()
        assert int(ws[tiles * 4 * D: tiles * 4 * D + 1].view(torch.int32).item()) == 0, "arrival counter not reset"
        res.append([t.clone() for t in gff + [g_in, g_ctx, grads]])
    for a, b in zip(*res):
        assert torch.equal(a, b), "second backward on the same workspace differs"
    assert _guard_ok(ws, nws), "workspace guard written"
    for k_, b, n in [("g_in", g_in, T * D), ("g_ctx", g_ctx, T * HK)] + [(f"g_ff{l}", b, T * w) for l, (b, w) in enumerate(zip(gff, ff))]:
        assert _guard_ok(b, n), (k_, "guard written")
    worst["g_in"] = cmp("g_in", g_in[: T * D].view(T, D).cpu().numpy(), bw["g_in"], rel)
    worst["g_ctx"] = cmp("g_ctx", g_ctx[: T * HK].view(T, HK).cpu().numpy(), bw["g_ctx"], rel)
    for l, w in enumerate(ff):
        worst[f"g_ff{l}"] = cmp(f"g_ff{l}", gff[l][: T * w].view(T, w).cpu().numpy(), bw["g_ff"][l], rel)
    gr = grads.cpu().numpy()
    untouched = np.ones(n_par, bool)
    for k_ in ("ln1_g", "ln1_b", "ln2_g", "ln2_b"):
        worst[k_] = cmp(k_, gr[off[k_]: off[k_] + D], bw[k_], rel_ln)
        untouched[off[k_]: off[k_] + D] = False
    assert (gr[untouched] == SENT).all(), "gradient entries outside the four LayerNorm ranges written"
    print(name, "rel", rel, "worst err / tol", max(worst.values()), max(worst, key=worst.get))


@pytest.mark.gpu
@pytest.mark.parametrize("refusal", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_token_chain_refuses_outside_the_envelope(refusal):
    """Shapes outside the envelope are refused by the host before any launch (the launch counter does not move): the
    library's dib_st_chain_supported agrees with the rules restated above, and both entries return an error code.  Every
    buffer is sized for the refused shape anyway, so that a launch by mistake could not write outside it."""
    from dib_amd import _lib as L
    from dib_amd.set_transformer import _BlockDesc
    name, D, HK, ff, act, T, kw = refusal
    lib, dev = _lib(), torch.device("cuda:0")
    dsc = _BlockDesc()
    wmax = max([D, HK] + list(ff) + [1])
    base = 16
    for l, w in enumerate(ff[:3]):
        dsc.ff_w[l], dsc.ff_b[l], dsc.ff_width[l] = base, base, w
    dsc.o_w, dsc.o_b, dsc.ln1_g, dsc.ln1_b, dsc.ln2_g, dsc.ln2_b = base, base, base, base, base, base
    dsc.n_ff, dsc.D, dsc.HK, dsc.eps, dsc.act = len(ff), D, HK, 1e-3, act
    n_par = base + 4 * wmax * wmax + 64
    slabs = kw.get("slabs", 1)
    stride = kw.get("stride", 0)
    Tb = max(T, 16)
    big = Tb * max(wmax, 1024) * max(slabs, 1) + 64
    arena = torch.zeros(24 * big + n_par + 64, device=dev)
    bufs = [_p(arena, 4 + i * big) for i in range(24)]
    params = _p(arena, 24 * big)
    ptrs3 = (ctypes.c_void_p * 3)(*[b.value for b in bufs[0:3]])
    gptrs3 = (ctypes.c_void_p * 3)(*[b.value for b in bufs[3:6]])
    default_sb = L.get_tuning("small_batch")
    try:
        if "small_batch" in kw:
            L.set_tuning("small_batch", kw["small_batch"])
        expect = st_chain_supported(D, HK, ff, act, T, kw.get("small_batch", 1))
        assert lib.dib_st_chain_supported(ctypes.byref(dsc), T) == int(expect), name
        n0 = lib.dib_launch_count()
        if not expect:
            rc = lib.dib_st_chain_fwd(ctypes.byref(dsc), T, params, bufs[6], bufs[7], bufs[8], bufs[9], bufs[10], ptrs3, bufs[11],
                                      bufs[12], bufs[13], _stream())
            assert rc != 0, name
        g_out = ctypes.c_void_p(bufs[14].value + 4 * kw.get("g_off", 0))
        rc = lib.dib_st_chain_bwd(ctypes.byref(dsc), T, params, g_out, slabs, stride, bufs[15], bufs[16], ptrs3, bufs[17], bufs[18],
                                  gptrs3, bufs[19], bufs[20], bufs[21], bufs[22], _stream())
        assert rc != 0, name
        torch.cuda.synchronize()
        assert lib.dib_launch_count() == n0, (name, "a refused call launched")
    finally:
        L.set_tuning("small_batch", default_sb)


# ---- D. the model at other architectures -----------------------------------------------------------------------------------


def _spec(**kw):
    import set_transformer_oracle as sto
    return sto.SetTransformerSpec(**kw)


# name: (spec kwargs, B, P, expected plan: impl, chain, attn_proj, attn_bwd_proj, deferred, ksplit[, skinny])
MODEL = {
    "d64_ff128_64_h2_p50": (dict(bottleneck_dimension=64, ff_arch_per_block=[128, 64], number_heads_per_mha=2,
                                 number_attention_blocks=2), 4, 50, ("flash", True, False, False, True, 4)),
    "d256_ff256_h1_gate_edge": (dict(bottleneck_dimension=256, ff_arch_per_block=[256], number_heads_per_mha=1,
                                     number_attention_blocks=2), 2, 50, ("flash", True, False, False, True, 2)),
    "d32_ff64_48_32": (dict(ff_arch_per_block=[64, 48, 32], number_attention_blocks=2), 3, 50, ("flash", True, True, True, True, 8)),
    "d32_ff32": (dict(ff_arch_per_block=[32], number_attention_blocks=2), 3, 50, ("flash", True, True, True, True, 8)),
    "key16_h2_gemm_chain": (dict(key_dim=16, number_heads_per_mha=2, number_attention_blocks=2), 3, 50,
                            ("gemm", True, False, False, False, 1)),
    "p65_h2": (dict(number_heads_per_mha=2, number_attention_blocks=2), 2, 65, ("flash", True, False, False, True, 4)),
    "p129_h2": (dict(number_heads_per_mha=2, number_attention_blocks=1), 2, 129, ("flash", True, False, False, True, 4)),
    "p257_h2": (dict(number_heads_per_mha=2, number_attention_blocks=1), 1, 257, ("flash", True, False, False, True, 4)),
    "t4500_p50_two_blocks": (dict(number_attention_blocks=2), 90, 50, ("flash", False, True, False, False, 8, True)),
}


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", list(MODEL))
def test_model_plan_branches_match_oracle(name):
    """SetTransformerDIB (forward, KL, BCE, every gradient block) against oracle/set_transformer_oracle.py through
    tests/test_gpu_set_transformer.py's _masked_parity (3e-4 of each gradient block's max-abs under the device's act' choices,
    2e-4 on the activations), at an architecture that sends the plan down a branch the notebook's never takes; the branch is
    asserted from the plan: attention implementation, token chain, projections inside the attention forward / backward,
    deferred weight gradients and the split-K count (the chain backward then sums 1 + 3 ksplit gradient slabs), and for more
    than 4096 tokens the skinny-K projection launches."""
    from test_gpu_set_transformer import _masked_parity
    kw, B, P, exp = MODEL[name]
    spec = _spec(**kw)
    m = _masked_parity(spec, B, P, seed=sum(map(ord, name)) % 89, attention="auto")
    pl = m.last["plan"]
    impl, chain, proj, bproj, deferred, ksplit = exp[:6]
    got = (pl["impl"], bool(pl["chain"]), pl["attn_proj"], pl["attn_bwd_proj"], bool(pl["deferred_wgrads"]), pl["ksplit"])
    assert got == exp[:6], (name, got)
    if chain:
        D = spec.bottleneck_dimension
        HK = spec.number_heads_per_mha * spec.key_dim
        assert st_chain_supported(D, HK, spec.ff_arch_per_block, 1, B * P)
    if len(exp) > 6:
        assert B * P > 4096 and type(pl["g"]["b0_qkv_fwd"]).__name__ == "_SkinnyKGemm"
        assert type(pl["g"]["b0_o_dgrad"]).__name__ == "_SkinnyKGemm"
