"""Host side of SetTransformerDIB's step plans without a GPU (tests/_st_host_recorder.py: the model on host memory, the library's
host queries answered by the real libdib_hip.so, every launch recorded instead of issued): which entry points a step calls
per dispatch path, that every descriptor stays inside the buffer it indexes, that the workspace map has no overlap, and that
the A/B switches are declared attributes."""
import bisect
import os
import shutil

import numpy as np
import pytest

import _st_host_recorder as R
from dib_amd import _lib, _st_plan

# Skipped only where the library can neither be found nor built, decided from the environment before anything runs; a failing
# import, compile, ABI or symbol check of the code under test fails the module.
if not os.path.exists(_lib.LIB_PATH) and not any(c and os.path.exists(c) for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc")):
    pytest.skip("no prebuilt libdib_hip.so and no hipcc to build it", allow_module_level=True)
try:
    R.real_library()
except OSError as e:   # dlopen: no HIP runtime on this machine
    pytest.skip(f"libdib_hip.so cannot be loaded here: {e}", allow_module_level=True)

SMALL = dict(number_heads_per_mha=4)
_TRAIN = {"dib_mean_pool_bwd": 1, "dib_mean_pool_fwd": 1, "dib_mlp_small_bwd": 1, "dib_mlp_small_fwd": 1, "dib_reduce_adam_step": 1,
          "dib_token_reparam_kl_bwd": 1, "dib_token_reparam_kl_fwd": 1}
_EVAL = {"dib_loss_rows": 1, "dib_mean_pool_fwd": 1, "dib_mlp_small_fwd": 1, "dib_token_reparam_kl_fwd": 1}
_CHAIN = {"dib_st_chain_bwd": 6, "dib_st_chain_fwd": 6}
# (name, constructor arguments, switches, B, P, calls of a training step, calls of an evaluation step) - the counts by entry
# point recorded before the plan builder was split into decide / layout / tables (the parent of that change)
MATRIX = [
    ("proj_4x50", SMALL, {}, 4, 50,
     dict(_TRAIN, **_CHAIN, dib_attention_bwd_proj=6, dib_attention_fwd_proj=6, dib_gemm_grouped=4, dib_mlp_small_head_step=1,
          dib_reduce_splits=1),
     dict(_EVAL, dib_attention_fwd_proj=6, dib_gemm_grouped=2, dib_st_chain_fwd=6)),
    ("flash_2x100", SMALL, {}, 2, 100,
     dict(_TRAIN, **_CHAIN, dib_attention_bwd=6, dib_attention_fwd=6, dib_gemm_grouped=16, dib_mlp_small_head_step=1,
          dib_reduce_splits=1),
     dict(_EVAL, dib_attention_fwd=6, dib_gemm_grouped=8, dib_st_chain_fwd=6)),
    ("no_chain_4x50", SMALL, dict(use_chain=False), 4, 50,
     dict(_TRAIN, dib_add_layernorm_bwd_fused=12, dib_add_layernorm_fwd=12, dib_attention_bwd=6, dib_attention_fwd_proj=6,
          dib_gemm_grouped=70, dib_mlp_small_head_step=1, dib_reduce_splits_add=6),
     dict(_EVAL, dib_add_layernorm_fwd=12, dib_attention_fwd_proj=6, dib_gemm_grouped=20)),
    ("no_defer_4x50", SMALL, dict(defer_wgrads=False), 4, 50,
     dict(_TRAIN, **_CHAIN, dib_attention_bwd=6, dib_attention_fwd_proj=6, dib_gemm_grouped=28, dib_mlp_small_head_step=1,
          dib_reduce_splits_add=6),
     dict(_EVAL, dib_attention_fwd_proj=6, dib_gemm_grouped=2, dib_st_chain_fwd=6)),
    ("gemm_4x20", dict(SMALL, attention="gemm"), {}, 4, 20,
     dict(_TRAIN, **_CHAIN, dib_gemm_grouped=52, dib_mlp_small_head_step=1, dib_reduce_splits=1, dib_softmax_rows_bwd=6,
          dib_softmax_rows_fwd=6),
     dict(_EVAL, dib_gemm_grouped=20, dib_softmax_rows_fwd=6, dib_st_chain_fwd=6)),
    ("skinny_2x100", SMALL, dict(skinny_k_min_tokens=128), 2, 100,
     dict(_TRAIN, **_CHAIN, dib_attention_bwd=6, dib_attention_fwd=6, dib_gemm_grouped=10, dib_gemm_skinny_k=6,
          dib_mlp_small_head_step=1, dib_reduce_splits=1),
     dict(_EVAL, dib_attention_fwd=6, dib_gemm_grouped=2, dib_gemm_skinny_k=6, dib_st_chain_fwd=6)),
    ("out2_4x50", dict(SMALL, output_dimensionality=2), {}, 4, 50,
     dict(_TRAIN, **_CHAIN, dib_attention_bwd_proj=6, dib_attention_fwd_proj=6, dib_gemm_grouped=8, dib_loss_rows=1,
          dib_reduce_splits=1),
     dict(_EVAL, dib_attention_fwd_proj=6, dib_gemm_grouped=2, dib_st_chain_fwd=6)),
    ("one_head_key64_4x20", dict(number_heads_per_mha=1, key_dim=64), {}, 4, 20,
     dict(_TRAIN, **_CHAIN, dib_add_inplace=18, dib_gemm_grouped=70, dib_mlp_small_head_step=1, dib_softmax_rows_bwd=6,
          dib_softmax_rows_fwd=6),
     dict(_EVAL, dib_gemm_grouped=20, dib_softmax_rows_fwd=6, dib_st_chain_fwd=6)),
]
SWITCHES = dict(use_chain=True, defer_wgrads=True, deferred_max_slabs=8, deferred_wgrad_target_wgs=1536, encoder_row_tiles=True,
                head_row_tiles=True, attention_proj=True, attention_bwd_proj=True)


def _unnamed(calls):
    return [(n, a) for n, args in calls for a in args
            if isinstance(a, list) and (a[:1] == ["?"] or any(isinstance(x, list) and x[:1] == ["?"] for x in a))]


@pytest.mark.parametrize("name,kw,sw,B,P,train,evaluate", MATRIX, ids=[c[0] for c in MATRIX])
def test_calls_per_step_by_entry_point(name, kw, sw, B, P, train, evaluate):
    m = R.make_model(sw, **kw)
    calls = R.record_train_step(m, B, P)
    assert R.call_counts(calls) == train
    assert not _unnamed(calls), "a launch was handed a pointer outside every buffer of the model and its plan"
    calls = R.record_eval_step(m, B, P)
    assert R.call_counts(calls) == evaluate
    assert not _unnamed(calls)


def test_switches_are_declared_attributes():
    """a misspelt switch must not be silently ignored: the eight exist, with their defaults, on a fresh object - and the class
    reads them (here: each of two changes the step)"""
    m = R.make_model(**SMALL)
    assert {k: getattr(m, k) for k in SWITCHES} == SWITCHES
    assert m.skinny_k_min_tokens == 1024 and R.make_model(skinny_k_min_tokens=7, **SMALL).skinny_k_min_tokens == 7
    assert m._unreduced is None and m._sync is None and m._info_ws is None
    base = R.call_counts(R.record_train_step(m, 4, 50))
    for k in ("use_chain", "attention_bwd_proj"):
        assert R.call_counts(R.record_train_step(R.make_model({k: False}, **SMALL), 4, 50)) != base, k


def _regions(pl):
    """sorted (offset, name) of the workspace map; b{b}_gln1 is slot 0 of b{b}_dx, the one declared alias"""
    off = pl["off"]
    alias = {k for k in off if k.endswith("_gln1")}
    for k in alias:
        assert off[k] == off[k.replace("_gln1", "_dx")]
    return sorted((o, k) for k, o in off.items() if k not in alias)


def _needed(m, B, P, pl):
    """name pattern -> elements its users touch, stated from the kernels' side (not from the layout's own numbers): [rows,
    width] activations, the sizes the library itself asks for, and for b{b}_dx slot 0 + the larger of the split-K slabs
    (3 * ksplit) and one slab per head (attention backward with the projections inside)."""
    lib = R.real_library()
    T, D, H, out = B * P, m.bottleneck_dimension, m.number_heads_per_mha, m.output_dimensionality
    HK, F0, ks = H * m.key_dim, m.particle_feature_dimensions, pl["ksplit"]
    S = B * H * P * pl["ldS"]
    need = {"feats": T * F0, "pe": T * pl["pe_w"], "x0": T * D, "pool": B * D, "g_pool": B * D, "pred": B * out, "g_pred": B * out,
            "out3": 3, "kl_sum": 1, "g_S": S, "ksplit_ws": 3 * ks * T * D,
            "attn_delta": -(-lib.dib_attention_bwd_workspace_bytes(B, P, H) // 4),
            "ln_ws": -(-lib.dib_add_layernorm_bwd_workspace_bytes(T, D) // 4), "kl_ws": -(-lib.dib_token_kl_workspace_bytes(T, D) // 4),
            "chain_ws": -(-lib.dib_st_chain_workspace_bytes(T, D) // 4), "loss_ws": -(-lib.dib_loss_rows_workspace_bytes(B) // 4)}
    need.update({nm: T * D for nm in ("g_x", "g_s", "g_a", "g_z", "g_h", "g_xq", "g_xk", "g_xv")})
    need.update({f"g_{nm}": T * HK for nm in ("q", "k", "v", "ctx")})
    for l, u in enumerate(pl["enc_units"]):
        need[f"enc_h{l}"] = need[f"g_enc_h{l}"] = T * u
    for l, u in enumerate(m.final_processing_arch):
        need[f"fin{l}"] = need[f"g_fin{l}"] = B * u
    for l, u in enumerate(m.ff_arch_per_block[:-1]):
        need[f"g_ff{l}"] = T * u
    for b in range(m.number_attention_blocks):
        need.update({f"b{b}_{nm}": T * HK for nm in ("q", "k", "v", "ctx", "g_q", "g_k", "g_v")})
        need.update({f"b{b}_{nm}": T * D for nm in ("mha", "h", "x", "xhat1", "xhat2", "g_z")})
        need.update({f"b{b}_rstd1": T, f"b{b}_rstd2": T, f"b{b}_S": S, f"b{b}_lse": B * H * P, f"b{b}_dx": (1 + max(3 * ks, H)) * T * D})
        for l, u in enumerate(m.ff_arch_per_block):
            need[f"b{b}_ff{l}"] = need[f"b{b}_g_ff{l}"] = T * u
    return need


@pytest.mark.parametrize("name,kw,sw,B,P", [c[:5] for c in MATRIX], ids=[c[0] for c in MATRIX])
def test_workspace_regions_do_not_overlap(name, kw, sw, B, P):
    """every named region is as large as its users need and ends before the next begins"""
    m = R.make_model(sw, **kw)
    pl = m._plan(B, P)
    reg = _regions(pl)
    offs = [o for o, _k in reg]
    assert len(set(offs)) == len(offs), "two named regions share an offset"
    assert all(o % 4 == 0 for o in offs) and offs[0] == 0
    need = _needed(m, B, P, pl)
    for (o, k), end in zip(reg, offs[1:] + [pl["ws"].numel()]):
        assert k in need, f"region {k}: the test does not know its size"
        assert need[k] > 0 and o + need[k] <= end, (k, o, need[k], end)
    # the layout's own statement of the same: offsets, and a workspace that ends with the last region
    d = _st_plan.decide(m, B, P)
    off, size = _st_plan.layout(d)
    assert off == pl["off"] and size == pl["ws"].numel() and d.sizes["loss_ws"] >= need["loss_ws"]


def _extent(rows, cols, ld):
    assert ld >= cols > 0 and rows > 0
    return (rows - 1) * ld + cols


@pytest.mark.parametrize("name,kw,sw,B,P", [c[:5] for c in MATRIX], ids=[c[0] for c in MATRIX])
def test_descriptors_stay_inside_their_buffers(name, kw, sw, B, P):
    """Every operand of every group of every table (include/dib_st.h dib_gemm_grouped: mode 0 C[M,N] = A[M,K] B[K,N] + bias[N];
    mode 1 C[M,N] = A[M,K] B[N,K]^T * act'(aux[M,N]); mode 2 C[M,N] = A[K,M]^T B[K,N] in nsplit slabs split_stride apart,
    bias_out[N]) lies inside its base tensor; inside ONE named region when the base is the workspace, inside ONE parameter
    when it is the parameter / gradient buffer; and the slabs of a mode-2 launch cover its contraction."""
    m = R.make_model(sw, **kw)
    pl = m._plan(B, P)
    reg = _regions(pl)
    ws_starts = [o for o, _k in reg] + [pl["ws"].numel()]
    par = sorted((o, o + int(np.prod(m.shapes[k]))) for k, o in m.offsets.items())
    par_starts = [lo for lo, _hi in par]

    def inside(t, lo, n, what, stride=0, copies=1):
        assert t is not None, what
        assert 0 <= lo and lo + (copies - 1) * stride + n <= t.numel(), what
        if t is pl["ws"]:
            i = bisect.bisect_right(ws_starts, lo) - 1
            assert lo + n <= ws_starts[i + 1], (what, reg[i][1])
        else:   # parameters, gradients or their slabs
            i = bisect.bisect_right(par_starts, lo) - 1
            assert lo + n <= par[i][1], what

    n_tables = 0
    for key, g in R.tables(pl):
        assert g.n == len(g.host) > 0 and g.dev is not None and g.dev.numel() == g.host.nbytes
        assert g.max_m == max(int(d["M"]) for d in g.host) and g.max_n == max(int(d["N"]) for d in g.host)
        for i, d in enumerate(g.host):
            M, N, K = int(d["M"]), int(d["N"]), int(d["K"])
            what = f"{key}[{i}]"
            a_shape, b_shape = {0: ((M, K), (K, N)), 1: ((M, K), (N, K)), 2: ((K, M), (K, N))}[g.mode]
            inside(g.A, int(d["a_off"]), _extent(*a_shape, int(d["lda"])), what + " A")
            inside(g.B, int(d["b_off"]), _extent(*b_shape, int(d["ldb"])), what + " B")
            splits = g.nsplit if g.mode == 2 else 1
            inside(g.C, int(d["c_off"]), _extent(M, N, int(d["ldc"])), what + " C", g.stride, splits)
            if g.mode == 2:
                assert g.nsplit >= 1 and g.nsplit * g.rps >= K, what + ": the slabs do not cover the contraction"
                assert g.nsplit == 1 or (g.stride == m.n_alloc and g.nsplit <= pl["nsplit"] and g.C is pl["slabs"]), what
                if int(d["bias_off"]) >= 0:
                    inside(g.bias_out, int(d["bias_off"]), N, what + " bias_out", g.stride, splits)
            elif g.mode == 0 and int(d["bias_off"]) >= 0:
                inside(g.bias, int(d["bias_off"]), N, what + " bias")
            if g.mode == 1 and g.aux is not None:
                inside(g.aux, int(d["aux_off"]), _extent(M, N, int(d["ldaux"])), what + " aux")
        n_tables += 1
    assert n_tables == len(pl["g"]) >= 30
    for key, t in pl["g"].items():   # split-K records: the slots the reduce sums lie in one region, as does its result
        if hasattr(t, "gemm"):
            inside(t.partial, t.partial_off, t.n * t.nslabs, key + " slabs")
            inside(t.out, t.out_off, t.n, key + " out")
            assert all(t.partial_off <= int(d["c_off"]) < t.partial_off + t.n * t.nslabs for d in t.gemm.host), key


def test_encoder_plan_shares_the_step_plans_encoder():
    """particle_encoder's own plan (cache key ("enc", T)) lays out and describes the encoder as the step plan of T tokens does"""
    m = R.make_model(**SMALL)
    rec = R.record_encoder(m, 200)
    pl = m._plan(4, 50)
    assert rec["off"] == {k: pl["off"][k] for k in rec["off"]}
    assert [g["descs"] for g in rec["g"]] == [pl["g"][f"enc{l}_fwd"].host.tobytes().hex() for l in range(len(rec["g"]))]
    assert R.call_counts(rec["calls"]) == {"dib_positional_encoding": 1, "dib_gemm_grouped": 3}
    assert ("enc", 200) in m._plans and (4, 50) in m._plans
