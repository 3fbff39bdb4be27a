"""The step plan of SetTransformerDIB for one (batch, particles) shape, in four steps that only hand values forward:

    decide(m, B, P)            what the shape runs on: every dispatch decision and every size the library is asked for
    layout(d)                  where every buffer lives: name -> element offset in the fp32 workspace (pure integers)
    *_tables(d, off, po)       which grouped-GEMM launches exist, per stage: named _Gemm / _SkinnyKGemm / _SplitKGemm records
    build_step_plan(m, B, P)   chains them and allocates - the only step that touches the device: workspace, gradient slabs,
                               table upload

Nothing after `decide` decides anything: where a builder picks a record type (`_SkinnyKGemm.fits`: decide's `skinny` AND the
kernel's own shape rule for these descriptors) or an operand's geometry (`_attn_product`: score buffers are the ones named
`*_S`), it applies a fixed rule to what it was handed.  The ORDER of the `take` calls in `layout` fixes every workspace offset.  The set of
tables does not depend on the path the step takes: the ones a path never launches are built too (evaluation-only calls and
the A/B switches find them).  SetTransformerDIB keeps the cache of plans."""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Dict, List, Tuple

import torch

from . import _lib
from ._gemm_plan import _Gemm, _SkinnyKGemm, _SplitKGemm, _d, _ptr_array3
from .dense import _mlp_desc

ACT_NONE, ACT_RELU, ACT_LEAKY01 = 0, 1, _lib.ACT_LEAKY_RELU_01


class _BlockDesc(ctypes.Structure):
    """include/dib_st.h dib_st_block_desc: element offsets of one attention block's token-wise chain in the flat parameter buffer"""
    _fields_ = [("o_w", ctypes.c_int64), ("o_b", ctypes.c_int64), ("ln1_g", ctypes.c_int64), ("ln1_b", ctypes.c_int64),
                ("ln2_g", ctypes.c_int64), ("ln2_b", ctypes.c_int64), ("ff_w", ctypes.c_int64 * 3), ("ff_b", ctypes.c_int64 * 3),
                ("n_ff", ctypes.c_int32), ("ff_width", ctypes.c_int32 * 3), ("D", ctypes.c_int32), ("HK", ctypes.c_int32),
                ("eps", ctypes.c_float), ("act", ctypes.c_int32)]


assert ctypes.sizeof(_BlockDesc) == 128


def _align4(n: int) -> int:
    return (n + 3) // 4 * 4


def block_grad_names(blocks: int, b: int) -> Tuple[str, str]:
    """(buffer holding dL/d(output of block b), buffer receiving dL/d(input of block b)): "g_x" and "g_s" alternate from
    block to block in backward order, so a block's result is the next block's input without a copy."""
    return ("g_x", "g_s") if (blocks - 1 - b) % 2 == 0 else ("g_s", "g_x")


# ---- 1. decisions -------------------------------------------------------------------------------------------------------------
class Decisions(namedtuple("Decisions", "B P T D H K HK F0 pe_w enc_units ff fin out_dim blocks n_alloc impl ldS ksplit chain defer "
                                        "nsplit rps skinny enc_mlp head_mlp attn_proj attn_bwd_proj target_wgs stash_block_bytes sizes")):
    """Everything a (batch, particles) shape runs on.
    Sizes: B neighbourhoods x P particles = T tokens of width D; H heads of key_dim K (HK = H * K); F0 input features, pe_w =
    F0 x frequencies; widths of the encoder / feed-forward / head layers; n_alloc elements of the flat parameter buffer.
    impl             attention: "flash" (dib_attention_*) or "gemm" (grouped products, probabilities in HBM, row pitch ldS)
    ksplit           split-K factor of the skinny [T, HK] x [HK, D] products (1: none)
    chain            one _BlockDesc per block: the token-wise half of a block as one launch per direction, or []
    defer            all blocks' weight gradients at the end of the backward, one grouped launch per shape class, each
                     aiming at target_wgs workgroups
    nsplit, rps      row slabs of the weight gradients' contraction over the tokens, and the rows of one slab
    skinny           projections out of the D-wide residual stream as streaming launches (dib_gemm_skinny_k)
    enc_mlp          dib_mlp_desc of the particle encoder on the row-tile kernels, or None
    head_mlp         dib_mlp_desc of the head as one launch (dib_mlp_small_head_step), or None
    attn_proj        q / k / v projections inside the attention forward (<= 64 particles)
    attn_bwd_proj    ... and their input gradient inside the attention backward
    stash_block_bytes  flash attention's score stash of one block (0: gemm attention)
    sizes            workspace regions whose size the library states, in elements"""
    __slots__ = ()

    def gn(self, b: int, nm: str) -> str:
        """buffer of block b's gradient `nm` (g_z, g_ff{l}, g_q, g_k, g_v): its own when deferred, else shared by all blocks"""
        return f"b{b}_{nm}" if self.defer else nm


def _split_k(T: int, HK: int) -> int:
    """few row tiles (< 128 of 64 tokens): cut the contraction of the skinny [T, HK] x [HK, D] products (_SplitKGemm)"""
    if (T + 63) // 64 < 128:
        for cand in (8, 4, 2):
            if HK % (cand * 32) == 0 and HK // cand >= 64:
                return cand
    return 1


def _chain_descs(m, T: int, D: int, HK: int, ff: List[int]) -> list:
    """csrc/dib_st_chain.h: output projection -> Add + LN -> feed-forward -> Add + LN of every block, if all are supported"""
    descs = []
    for b in range(m.number_attention_blocks):
        po, pre = m.offsets, f"blk{b}_"
        dsc = _BlockDesc()
        dsc.o_w, dsc.o_b = po[pre + "o_w"], po[pre + "o_b"]
        dsc.ln1_g, dsc.ln1_b = po[pre + "ln1_g"], po[pre + "ln1_b"]
        dsc.ln2_g, dsc.ln2_b = po[pre + "ln2_g"], po[pre + "ln2_b"]
        for l, u in enumerate(ff):
            dsc.ff_w[l], dsc.ff_b[l], dsc.ff_width[l] = po[pre + f"ff{l}_w"], po[pre + f"ff{l}_b"], u
        dsc.n_ff, dsc.D, dsc.HK, dsc.eps, dsc.act = len(ff), D, HK, m.layer_norm_epsilon, ACT_RELU
        descs.append(dsc)
    return descs if descs and all(m.lib.dib_st_chain_supported(ctypes.byref(dsc), T) for dsc in descs) else []


def decide(m, B: int, P: int) -> Decisions:
    """Every dispatch decision of the shape, from the model's configuration, its declared switches (SetTransformerDIB.__init__)
    and the library's *_supported / *_bytes / tuning answers.  In dependency order: chain needs T; defer needs chain and
    ksplit; nsplit needs defer; attn_bwd_proj needs defer."""
    lib, po = m.lib, m.offsets
    D, H, K = m.bottleneck_dimension, m.number_heads_per_mha, m.key_dim
    HK, T = H * K, B * P
    F0, nfreq = m.particle_feature_dimensions, m.number_positional_encoding_frequencies
    enc_units, ff, fin = m.particle_encoder_arch_spec + [2 * D], m.ff_arch_per_block, m.final_processing_arch
    impl = m.attention_impl   # fixed by the constructor: flash for key_dim == 128 unless attention="gemm"
    ksplit = _split_k(T, HK)
    chain = _chain_descs(m, T, D, HK, ff) if m.use_chain and len(ff) <= 3 else []
    # Deferred weight gradients: on the chain path every block keeps the operands of its weight gradients in buffers of its
    # own and ALL blocks' weight gradients run at the end of the backward as one grouped launch per shape class instead of 3
    # launches per block: at the notebook's size 18 launches of 7-18 us on a few dozen workgroups each become 3 that fill the chip.
    defer = bool(chain) and ksplit > 1 and bool(m.defer_wgrads)
    # Weight gradients contract over the T tokens in row slabs summed in a fixed order: 64-row slabs, at most 32 (with one slab
    # the q/k/v and output-projection wgrads of 1600 tokens ran on 12-36 workgroups looping over all rows, 110-137 us each).
    # Deferred: many groups per launch fill the chip with FEW splits, and every slab costs the optimizer's launch a pass over
    # the whole gradient buffer - 25 slabs x 5.2 MB were 33 us of a 1.29 ms step (`deferred_max_slabs`).
    nsplit = max(1, min(int(m.deferred_max_slabs) if defer else 32, T // 64))
    rps = ((T + nsplit - 1) // nsplit + 31) // 32 * 32
    nsplit = (T + rps - 1) // rps
    # the particle encoder on the row-tile MLP kernels (up to 2048 tokens): one launch forward (encoding included), one for
    # the dgrad chain, instead of 4 + 2
    enc_mlp = None
    if m.encoder_row_tiles and 2 <= len(enc_units) <= 4:
        dsc = _mlp_desc([po[f"enc{l}_w"] for l in range(len(enc_units))], [po[f"enc{l}_b"] for l in range(len(enc_units))],
                        enc_units, F0, nfreq, ACT_LEAKY01)
        enc_mlp = dsc if lib.dib_mlp_small_supported(ctypes.byref(dsc), T) else None
    # the head's whole share of a training step as ONE launch (dib_mlp_small_head_step): forward, loss, gradient of the logit,
    # dgrad chain, the output layer's gradient
    head_mlp = None
    if m.head_row_tiles and m.output_dimensionality == 1 and 1 <= len(fin) <= 3:
        dsc = _mlp_desc([po[f"fin{l}_w"] for l in range(len(fin))] + [po["out_w"]],
                        [po[f"fin{l}_b"] for l in range(len(fin))] + [po["out_b"]], fin + [1], D, 1, ACT_LEAKY01)
        head_mlp = dsc if lib.dib_mlp_small_head_supported(ctypes.byref(dsc), B) else None
    # <= 64 particles: the q / k / v projections inside the attention forward, and their input gradient inside the attention
    # backward (one slab per head behind the LN1-addend gradient: needs the deferred mode's per-block dx regions and the
    # 8-wave kernel)
    attn_proj = bool(impl == "flash" and m.attention_proj and lib.dib_attention_fwd_proj_supported(P, K, D))
    attn_bwd_proj = bool(defer and impl == "flash" and m.attention_bwd_proj and lib.dib_attention_fwd_proj_supported(P, K, D)
                         and _lib.get_tuning("attn_small_bwd_waves") >= 8)
    sizes = dict(ln_ws=int(lib.dib_add_layernorm_bwd_workspace_bytes(T, D)) // 4,
                 kl_ws=int(lib.dib_token_kl_workspace_bytes(T, D)) // 4 + 4,
                 loss_ws=int(lib.dib_loss_rows_workspace_bytes(B)) // 4 + 4)
    if impl == "flash":
        sizes["attn_delta"] = int(lib.dib_attention_bwd_workspace_bytes(B, P, H)) // 4   # delta + dQ key-block partials
    if chain:
        sizes["chain_ws"] = int(lib.dib_st_chain_workspace_bytes(T, D)) // 4
    if head_mlp is not None:
        sizes["head_ws"] = int(lib.dib_mlp_small_head_workspace_bytes(ctypes.byref(head_mlp), B)) // 4 + 4
    return Decisions(B=B, P=P, T=T, D=D, H=H, K=K, HK=HK, F0=F0, pe_w=F0 * nfreq, enc_units=enc_units, ff=ff, fin=fin,
                     out_dim=m.output_dimensionality, blocks=m.number_attention_blocks, n_alloc=m.n_alloc, impl=impl,
                     ldS=_align4(P), ksplit=ksplit, chain=chain, defer=defer, nsplit=nsplit, rps=rps,
                     skinny=T >= m.skinny_k_min_tokens, enc_mlp=enc_mlp, head_mlp=head_mlp, attn_proj=attn_proj,
                     attn_bwd_proj=attn_bwd_proj, target_wgs=int(m.deferred_wgrad_target_wgs),
                     stash_block_bytes=int(lib.dib_attention_stash_bytes(B, P, H)) if impl == "flash" else 0, sizes=sizes)


# ---- 2. layout ----------------------------------------------------------------------------------------------------------------
class _Taker:
    """hands out 16-byte aligned regions of the workspace in call order"""

    def __init__(self):
        self.off: Dict[str, int] = {}
        self.size = 0

    def __call__(self, name: str, n: int) -> None:
        self.off[name] = self.size
        self.size = _align4(self.size + int(n))


def _encoder_layout(take: _Taker, T: int, F0: int, pe_w: int, enc_units: List[int]) -> None:
    take("feats", T * F0)
    take("pe", T * pe_w)
    for l, u in enumerate(enc_units):
        take(f"enc_h{l}", T * u)                # last one = enc_out (mu | raw logvar)


def layout(d: Decisions) -> Tuple[Dict[str, int], int]:
    """name -> element offset of every workspace buffer, and the workspace's size.  Activations first (the backward reads
    them), then the backward's scratch."""
    take = _Taker()
    B, P, T, D, H, HK = d.B, d.P, d.T, d.D, d.H, d.HK
    _encoder_layout(take, T, d.F0, d.pe_w, d.enc_units)
    take("x0", T * D)                           # u = sampled embeddings
    for b in range(d.blocks):
        for nm in ("q", "k", "v", "ctx"):
            take(f"b{b}_{nm}", T * HK)
        if d.impl == "gemm":
            take(f"b{b}_S", B * H * P * d.ldS)  # attention probabilities (stashed for the backward)
        else:
            take(f"b{b}_lse", B * H * P)        # per-query log-sum-exp (the flash backward recomputes the rest)
        take(f"b{b}_mha", T * D)
        take(f"b{b}_xhat1", T * D); take(f"b{b}_rstd1", T); take(f"b{b}_h", T * D)
        for l, u in enumerate(d.ff):
            take(f"b{b}_ff{l}", T * u)
        take(f"b{b}_xhat2", T * D); take(f"b{b}_rstd2", T); take(f"b{b}_x", T * D)
    take("pool", B * D)
    for l, u in enumerate(d.fin):
        take(f"fin{l}", B * u)
    take("pred", B * d.out_dim)
    take("g_pred", B * d.out_dim)
    take("out3", 4)
    take("kl_sum", 4)
    # backward scratch (reused by every block)
    for l, u in enumerate(d.fin):
        take(f"g_fin{l}", B * u)
    take("g_pool", B * D)
    # g_x / g_s: gradient w.r.t. a block's output / input, ping-ponging from block to block (no copy); g_a: both addends
    # of LN2; g_z: feed-forward pre-activation; g_h: the feed-forward branch's gradient w.r.t. h
    take("g_x", T * D); take("g_s", T * D); take("g_a", T * D); take("g_z", T * D); take("g_h", T * D)
    for l, u in enumerate(d.ff[:-1]):
        take(f"g_ff{l}", T * u)
    for nm in ("q", "k", "v", "ctx"):
        take(f"g_{nm}", T * HK)
    if d.impl == "gemm":
        take("g_S", B * H * P * d.ldS)
    else:
        take("attn_delta", d.sizes["attn_delta"])
    for nm in ("q", "k", "v"):
        take(f"g_x{nm}", T * D)
    if d.ksplit > 1:
        take("ksplit_ws", 3 * d.ksplit * T * D)   # the partial slabs of the split-K products
    for l, u in enumerate(d.enc_units):
        take(f"g_enc_h{l}", T * u)
    take("ln_ws", d.sizes["ln_ws"])
    take("kl_ws", d.sizes["kl_ws"])
    if d.chain:
        take("chain_ws", d.sizes["chain_ws"])
    if d.defer:
        # per block: dL/d(feed-forward pre-activations), dL/dq|k|v, and b{b}_dx = [slot 0: the gradient of LN1's addends |
        # slots 1..: the split-K slabs of the q/k/v input gradient, or one slab per head (attn_bwd_proj)], so that ONE
        # fixed-order sum over the slots is the gradient handed to the next block and slot 0 stays what the output
        # projection's weight gradient contracts with
        for b in range(d.blocks):
            take(f"b{b}_g_z", T * D)
            for l, u in enumerate(d.ff[:-1]):
                take(f"b{b}_g_ff{l}", T * u)
            for nm in "qkv":
                take(f"b{b}_g_{nm}", T * HK)
            take(f"b{b}_dx", (1 + max(3 * d.ksplit, H)) * T * D)
            take.off[f"b{b}_gln1"] = take.off[f"b{b}_dx"]   # slot 0 (the one alias of the workspace)
    take("loss_ws", d.sizes["loss_ws"])
    return take.off, take.size


# ---- 3. tables ----------------------------------------------------------------------------------------------------------------
# Base tensors are given by name ("ws" the workspace, "params", "gt" the weight gradients' target: the slabs or the gradient
# buffer); build_*_plan binds them.
def _wgrads(d: Decisions, descs, M=None) -> _Gemm:
    """weight (and bias) gradients of `descs` in one grouped launch: in the step's row slabs over the tokens, or (M given)
    as one slab of M rows"""
    ns, r = (d.nsplit, d.rps) if M is None else (1, max(M, 1))
    return _Gemm(2, descs, "ws", "ws", "gt", bias_out="gt", nsplit=ns, rows_per_split=r, split_stride=d.n_alloc)


def _wdesc(off, po, x, kin, dy, kout, w, b, M) -> dict:
    return _d(off[x], kin, off[dy], kout, po[w], kout, kin, kout, M, bias_off=po[b])


def _descs(t: _Gemm) -> List[dict]:
    """the descriptors of a table, to regroup them in another launch"""
    return [dict(zip(t.host.dtype.names, row)) for row in t.host.tolist()]


# one Dense layer of a chain: name of its tables, name of its parameters, output buffer, buffer of the output's gradient
_Layer = namedtuple("_Layer", "table param out grad width act")


def _mlp_fwd_tables(off, po, x, kin, layers, M) -> Dict[str, _Gemm]:
    """forward of a Dense chain (a list of _Layer) on buffer x [M, kin]"""
    g = {}
    for L in layers:
        g[f"{L.table}_fwd"] = _Gemm(0, [_d(off[x], kin, po[L.param + "_w"], L.width, off[L.out], L.width, M, L.width, kin,
                                           bias_off=po[L.param + "_b"])], "ws", "params", "ws", bias="params", act=L.act)
        x, kin = L.out, L.width
    return g


def _mlp_bwd_tables(d: Decisions, off, po, x, kin, gx, layers, M, token_slabs=True) -> Dict[str, _Gemm]:
    """Backward of the same chain: per layer the weight gradient, and the gradient handed to the layer below, dy @ W^T times
    that layer's act'(its output); the chain's input takes it plain, into buffer gx, or (None) not at all."""
    g, below = {}, None
    for L in layers:
        g[f"{L.table}_wgrad"] = _wgrads(d, [_wdesc(off, po, x, kin, L.grad, L.width, L.param + "_w", L.param + "_b", M)],
                                        M=None if token_slabs else M)
        if below:     # x is the output of the layer below: aux
            g[f"{L.table}_dgrad"] = _Gemm(1, [_d(off[L.grad], L.width, po[L.param + "_w"], L.width, off[below.grad], kin, M, kin,
                                                 L.width, aux_off=off[x], ldaux=kin)], "ws", "params", "ws", aux="ws", act=below.act)
        elif gx:
            g[f"{L.table}_dgrad"] = _Gemm(1, [_d(off[L.grad], L.width, po[L.param + "_w"], L.width, off[gx], kin, M, kin, L.width,
                                                 ldaux=kin)], "ws", "params", "ws")
        x, kin, below = L.out, L.width, L
    return g


def _encoder_layers(enc_units: List[int]) -> list:
    """particle encoder (shared by all particles): [T, pe_w] -> Dense(LeakyReLU(0.1))* -> Dense"""
    return [_Layer(f"enc{l}", f"enc{l}", f"enc_h{l}", f"g_enc_h{l}", u, ACT_LEAKY01 if l < len(enc_units) - 1 else ACT_NONE)
            for l, u in enumerate(enc_units)]


def _ff_layers(d: Decisions, b: int) -> list:
    """feed-forward of block b on h (per-layer tables: the path without the chain kernels); g_z = dL/d(pre-activation of the
    last layer)"""
    n = len(d.ff)
    return [_Layer(f"b{b}_ff{l}", f"blk{b}_ff{l}", f"b{b}_ff{l}", "g_z" if l == n - 1 else f"g_ff{l}", u, ACT_RELU)
            for l, u in enumerate(d.ff)]


def encoder_tables(d: Decisions, off, po) -> Dict[str, _Gemm]:
    """particle encoder, forward and backward (its input has no gradient)"""
    layers = _encoder_layers(d.enc_units)
    return {**_mlp_fwd_tables(off, po, "pe", d.pe_w, layers, d.T), **_mlp_bwd_tables(d, off, po, "pe", d.pe_w, None, layers, d.T)}


def _attn_product(d: Decisions, off, mode, a, b, c, M, N, Kc, **kw) -> _Gemm:
    """One product of the gemm attention for every (neighbourhood, head).  An operand is a [T, HK] buffer, of which the pair
    owns the P rows of the neighbourhood and the K columns of the head, or (names ending in "_S") the [B, H, P, ldS] scores."""
    def at(name, bi, hi):
        return off[name] + ((bi * d.H + hi) * d.P * d.ldS if name.endswith("_S") else bi * d.P * d.HK + hi * d.K)
    ld = lambda name: d.ldS if name.endswith("_S") else d.HK
    return _Gemm(mode, [_d(at(a, bi, hi), ld(a), at(b, bi, hi), ld(b), at(c, bi, hi), ld(c), M, N, Kc)
                        for bi in range(d.B) for hi in range(d.H)], "ws", "ws", "ws", **kw)


def block_fwd_tables(d: Decisions, off, po, b: int) -> Dict[str, object]:
    """forward of attention block b: q/k/v projections, (gemm attention: scores, context), output projection, feed-forward"""
    T, D, HK, P, K = d.T, d.D, d.HK, d.P, d.K
    xin, pre, g = "x0" if b == 0 else f"b{b - 1}_x", f"blk{b}_", {}
    qkv = [_d(off[xin], D, po[pre + nm + "_w"], HK, off[f"b{b}_{nm}"], HK, T, HK, D, bias_off=po[pre + nm + "_b"]) for nm in "qkv"]
    mk = _SkinnyKGemm if d.skinny and _SkinnyKGemm.fits(0, qkv) else _Gemm
    g[f"b{b}_qkv_fwd"] = mk(0, qkv, "ws", "params", "ws", bias="params")
    if d.impl == "gemm":
        g[f"b{b}_qk"] = _attn_product(d, off, 1, f"b{b}_q", f"b{b}_k", f"b{b}_S", P, P, K)   # S = Q K^T (scale: in the softmax)
        g[f"b{b}_pv"] = _attn_product(d, off, 0, f"b{b}_S", f"b{b}_v", f"b{b}_ctx", P, K, P)  # ctx = P V
    if d.ksplit > 1:   # one partial slab per chunk of the contraction; LN1 sums the slabs (mode "defer")
        ck = HK // d.ksplit
        g[f"b{b}_o_fwd"] = _SplitKGemm(
            _Gemm(0, [_d(off[f"b{b}_ctx"] + s * ck, HK, po[pre + "o_w"] + s * ck * D, D, off["ksplit_ws"] + s * T * D, D,
                         T, D, ck, bias_off=po[pre + "o_b"] if s == 0 else -1) for s in range(d.ksplit)],
                  "ws", "params", "ws", bias="params"),
            "ws", off["ksplit_ws"], T * D, d.ksplit, "ws", off[f"b{b}_mha"], mode="defer")
    else:
        g[f"b{b}_o_fwd"] = _Gemm(0, [_d(off[f"b{b}_ctx"], HK, po[pre + "o_w"], D, off[f"b{b}_mha"], D, T, D, HK, bias_off=po[pre + "o_b"])],
                                 "ws", "params", "ws", bias="params", act=ACT_NONE)
    g.update(_mlp_fwd_tables(off, po, f"b{b}_h", D, _ff_layers(d, b), T))
    return g


def _qkv_dgrad_split_k(d: Decisions, off, po, b: int, region: str, slot0: int, nslabs: int, out: str, mode: str) -> _SplitKGemm:
    """The q/k/v projections' input gradient as 3 x ksplit partial products, one slab each from slot `slot0` of `region` on;
    `mode` says who sums the `nslabs` slots of the region into `out` (_SplitKGemm)."""
    T, D, HK, ks = d.T, d.D, d.HK, d.ksplit
    ck = HK // ks
    return _SplitKGemm(
        _Gemm(1, [_d(off[d.gn(b, f"g_{nm}")] + s * ck, HK, po[f"blk{b}_{nm}_w"] + s * ck, HK,
                     off[region] + (slot0 + i * ks + s) * T * D, D, T, D, ck) for i, nm in enumerate("qkv") for s in range(ks)],
              "ws", "params", "ws"),
        "ws", off[region], T * D, nslabs, "ws", off[out], mode=mode)


def block_bwd_tables(d: Decisions, off, po, b: int) -> Dict[str, object]:
    """backward of attention block b: feed-forward, output projection, (gemm attention: its four products), q/k/v"""
    T, D, HK, P, K, ff, nff = d.T, d.D, d.HK, d.P, d.K, d.ff, len(d.ff)
    xin, pre, g = "x0" if b == 0 else f"b{b - 1}_x", f"blk{b}_", {}
    gout = block_grad_names(d.blocks, b)[1]   # gradient w.r.t. the block's input x (= gradient of LN1's two addends)
    g.update(_mlp_bwd_tables(d, off, po, f"b{b}_h", D, "g_h", _ff_layers(d, b), T))
    # attention output projection (deferred: its dy is slot 0 of the block's dx region)
    g[f"b{b}_o_wgrad"] = _wgrads(d, [_wdesc(off, po, f"b{b}_ctx", HK, f"b{b}_gln1" if d.defer else gout, D,
                                            pre + "o_w", pre + "o_b", T)])
    o_dgrad = [_d(off[gout], D, po[pre + "o_w"], D, off["g_ctx"], HK, T, HK, D)]
    mk = _SkinnyKGemm if d.skinny and _SkinnyKGemm.fits(1, o_dgrad) else _Gemm
    g[f"b{b}_o_dgrad"] = mk(1, o_dgrad, "ws", "params", "ws")
    if d.impl == "gemm":
        one = dict(nsplit=1, rows_per_split=max(P, 1))
        g[f"b{b}_dv"] = _attn_product(d, off, 2, f"b{b}_S", "g_ctx", d.gn(b, "g_v"), P, K, P, **one)
        g[f"b{b}_dp"] = _attn_product(d, off, 1, "g_ctx", f"b{b}_v", "g_S", P, P, K)
        g[f"b{b}_dq"] = _attn_product(d, off, 0, "g_S", f"b{b}_k", d.gn(b, "g_q"), P, K, P)
        g[f"b{b}_dk"] = _attn_product(d, off, 2, "g_S", f"b{b}_q", d.gn(b, "g_k"), P, K, P, **one)
    g[f"b{b}_qkv_wgrad"] = _wgrads(d, [_wdesc(off, po, xin, D, d.gn(b, f"g_{nm}"), HK, pre + nm + "_w", pre + nm + "_b", T)
                                       for nm in "qkv"])
    if d.chain:
        # the feed-forward layers' weight gradients in one grouped launch (dy = the chain backward's g_ff); the output
        # projection's and q / k / v's keep their own launches.  (One launch for ALL of them was tried: a grouped launch's
        # grid is max-shape tiles x groups, and [1536, 32] next to [32, 1536] made it 21 600 mostly empty workgroups - 48 us.)
        g[f"b{b}_ff_wgrad"] = _wgrads(d, [
            _wdesc(off, po, f"b{b}_h" if l == 0 else f"b{b}_ff{l - 1}", D if l == 0 else ff[l - 1],
                   d.gn(b, "g_z" if l == nff - 1 else f"g_ff{l}"), ff[l], pre + f"ff{l}_w", pre + f"ff{l}_b", T) for l in range(nff)])
    if d.defer:
        # the slabs land behind the LN1-addend gradient in the block's own region; the sum over all slots is taken by the
        # consumer: the previous block's chain launch sums them as it loads its tile (dib_st_chain_bwd g_out_slabs), block
        # 0's go through one reduce launch into the buffer the bottleneck's backward reads
        g[f"b{b}_qkv_dgrad"] = _qkv_dgrad_split_k(d, off, po, b, f"b{b}_dx", 1, 1 + 3 * d.ksplit, gout, "store" if b == 0 else "defer")
    elif d.ksplit > 1:   # 3 * ksplit slabs, summed straight into gout (= the residual's gradient + g_xq + g_xk + g_xv)
        g[f"b{b}_qkv_dgrad"] = _qkv_dgrad_split_k(d, off, po, b, "ksplit_ws", 0, 3 * d.ksplit, gout, "add")
    else:
        g[f"b{b}_qkv_dgrad"] = _Gemm(1, [_d(off[f"g_{nm}"], HK, po[pre + nm + "_w"], HK, off[f"g_x{nm}"], D, T, D, HK)
                                         for nm in "qkv"], "ws", "params", "ws")
    return g


def head_tables(d: Decisions, off, po) -> Dict[str, _Gemm]:
    """head: pooled [B, D] -> Dense(LeakyReLU(0.1))* -> Dense(out), forward and backward (contraction over the B neighbourhoods)"""
    layers = [_Layer(f"fin{l}", f"fin{l}", f"fin{l}", f"g_fin{l}", u, ACT_LEAKY01) for l, u in enumerate(d.fin)] \
        + [_Layer("out", "out", "pred", "g_pred", d.out_dim, ACT_NONE)]
    return {**_mlp_fwd_tables(off, po, "pool", d.D, layers, d.B),
            **_mlp_bwd_tables(d, off, po, "pool", d.D, "g_pool", layers, d.B, token_slabs=False)}


def deferred_wgrad_tables(d: Decisions, g: Dict[str, object]) -> Dict[str, _Gemm]:
    """The deferred mode's launches, regrouped from the per-layer tables `g`: the head's weight gradients as one launch, and
    one launch per shape class for all blocks' - q/k/v ([D, HK]), output projection ([HK, D]), feed-forward, which the
    particle encoder's join (same T tokens, fit the class's tiles)."""
    blocks, T = range(d.blocks), d.T
    out = {"head_wgrads": _wgrads(d, [dsc for k in ([] if d.head_mlp is not None else ["out_wgrad"])
                                      + [f"fin{l}_wgrad" for l in range(len(d.fin))] for dsc in _descs(g[k])], M=d.B)}
    classes = (("dw_qkv", [f"b{b}_qkv_wgrad" for b in blocks], (64, 128)), ("dw_o", [f"b{b}_o_wgrad" for b in blocks], (128, 64)),
               ("dw_ff", [f"b{b}_ff_wgrad" for b in blocks] + [f"enc{l}_wgrad" for l in range(len(d.enc_units))], (128, 128)))
    # A grouped launch's grid is (splits, tiles of the LARGEST group shape, groups): the split count of each class is chosen so
    # that its workgroups make about `deferred_wgrad_target_wgs` - many groups need few, long splits (1536: the best of 384 /
    # 512 / 768 / 1024 / 1536 at the notebook's size, profiles/r06b_set_transformer_deferred_wgrads_ab.txt; 2048 and 3072 no
    # better, r06c); slabs beyond a launch's count are never written and stay zero (the slab buffer is zero-initialised and
    # every launch always writes the same slabs)
    for name, members, (tm, tn) in classes:
        descs = [dsc for k in members for dsc in _descs(g[k])]
        mm, nn = max(x["M"] for x in descs), max(x["N"] for x in descs)
        tiles = len(descs) * ((mm + tm - 1) // tm) * ((nn + tn - 1) // tn)
        ns = max(1, min(d.nsplit, int(round(d.target_wgs / tiles))))
        r = ((T + ns - 1) // ns + 63) // 64 * 64
        out[name] = _Gemm(2, descs, "ws", "ws", "gt", bias_out="gt", nsplit=(T + r - 1) // r, rows_per_split=r, split_stride=d.n_alloc)
    return out


def step_tables(d: Decisions, off, po) -> Dict[str, object]:
    """every table of the shape, by name"""
    g = encoder_tables(d, off, po)
    for b in range(d.blocks):
        g.update(block_fwd_tables(d, off, po, b))
        g.update(block_bwd_tables(d, off, po, b))
    g.update(head_tables(d, off, po))
    if d.defer:
        g.update(deferred_wgrad_tables(d, g))
    return g


# ---- 4. allocation ------------------------------------------------------------------------------------------------------------
def _upload(g, bases, device) -> None:
    for t in g.values():
        t.bind(bases)
        t.upload(device)


def build_step_plan(m, B: int, P: int) -> dict:
    """The plan of a training / evaluation step of shape (B, P): SetTransformerDIB._plan caches it."""
    d = decide(m, B, P)
    off, size = layout(d)
    po = m.offsets
    g = step_tables(d, off, po)
    ws = torch.zeros(size, dtype=torch.float32, device=m.device)
    slabs = torch.zeros(d.nsplit * m.n_alloc, dtype=torch.float32, device=m.device) if d.nsplit > 1 else None
    gt = slabs if d.nsplit > 1 else m.grads
    _upload(g, dict(ws=ws, params=m.params, gt=gt), m.device)
    rows = lambda pre, n: _ptr_array3(ws, [off[f"{pre}{l}"] for l in range(n)])   # the hidden layers' rows of a row-tile MLP
    nh = len(d.enc_units) - 1
    enc_mlp = None if d.enc_mlp is None else dict(desc=d.enc_mlp, h=rows("enc_h", nh), g=rows("g_enc_h", nh))
    head_mlp = None if d.head_mlp is None else dict(desc=d.head_mlp, h=rows("fin", len(d.fin)), g=rows("g_fin", len(d.fin)),
                                                    ws=torch.zeros(d.sizes["head_ws"], dtype=torch.float32, device=m.device))
    # stash: flash attention's score tiles, one buffer per block, outside the fp32-indexed workspace (3.2 GB per block at
    # 4 x 4096); None = recompute mode.  Allocated LAZILY by the first forward that a backward will follow
    # (SetTransformerDIB._ensure_stash): evaluation-only shapes never own one.
    return dict(impl=d.impl, B=B, P=P, T=d.T, ldS=d.ldS, off=off, ws=ws, g=g, nsplit=d.nsplit, slabs=slabs, gt=gt, pe_w=d.pe_w,
                enc_units=d.enc_units, stash=None, stash_block_bytes=d.stash_block_bytes, stash_denied=None, ksplit=d.ksplit,
                chain=d.chain, deferred_wgrads=["dw_qkv", "dw_o", "dw_ff"] if d.defer else [], enc_mlp=enc_mlp,
                head_mlp=head_mlp, attn_proj=d.attn_proj, attn_bwd_proj=d.attn_bwd_proj,
                qkv_off=[((ctypes.c_int64 * 3)(*[po[f"blk{b}_{nm}_w"] for nm in "qkv"]),
                          (ctypes.c_int64 * 3)(*[po[f"blk{b}_{nm}_b"] for nm in "qkv"])) for b in range(d.blocks)],
                # per block: the buffers of its feed-forward layers' pre-activation gradients and of dq, dk, dv
                grad_names=[dict(ff=[d.gn(b, "g_z" if l == len(d.ff) - 1 else f"g_ff{l}") for l in range(len(d.ff))],
                                 qkv=[d.gn(b, f"g_{nm}") for nm in "qkv"]) for b in range(d.blocks)])


def build_encoder_plan(m, T: int) -> dict:
    """Encoder-only workspace + forward tables for `particle_encoder` on T particles (no attention buffers)."""
    F0 = m.particle_feature_dimensions
    pe_w, units = F0 * m.number_positional_encoding_frequencies, m.particle_encoder_arch_spec + [2 * m.bottleneck_dimension]
    take = _Taker()
    _encoder_layout(take, T, F0, pe_w, units)
    g = _mlp_fwd_tables(take.off, m.offsets, "pe", pe_w, _encoder_layers(units), T)
    ws = torch.zeros(take.size, dtype=torch.float32, device=m.device)
    _upload(g, dict(ws=ws, params=m.params), m.device)
    return dict(ws=ws, off=take.off, g=list(g.values()))
