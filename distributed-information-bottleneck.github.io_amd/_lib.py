"""ctypes binding of libdib_hip.so (C ABI declared in include/dib_hip.h) + in-tree build helper.

The library is built IN-TREE with hipcc for gfx950 (`build_library`) so the .so travels with the
repo snapshot to the GPU box.  There is no CPU fallback: if the library cannot be loaded the
product path raises.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_HERE, "libdib_hip.so")
# Kernel A/B experiments (tools/ab_bench.sh) point DIB_LIB_PATH at a variant build (exp/lib_TAG.so); the product artefact is
# never overwritten.  A set-but-missing path is an error, not a silent return to the product library.
LIB_OVERRIDE = os.environ.get("DIB_LIB_PATH") or None
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")


def _sources() -> list:
    """Every file the one translation unit (csrc/dib_api.hip) can include: it, the kernel headers and the host fragments under
    csrc/, and the public headers.  Read from the directories, so a new header needs no registration here.  (csrc/dib_ctw.cpp is
    ctw.py's own build.)"""
    out = []
    for root, _, names in os.walk(CSRC):
        out += [os.path.join(root, n) for n in names if n.endswith((".h", ".hip"))]
    out += [os.path.join(INCLUDE_DIR, n) for n in os.listdir(INCLUDE_DIR) if n.endswith(".h")]
    return sorted(out)


# error codes (include/dib_hip.h)
DIB_OK = 0
ABI_VERSION = 7   # include/dib_hip.h DIB_ABI_VERSION this binding's SIGNATURES were written against
ACTIVATIONS = {None: 0, "linear": 0, "None": 0, "relu": 1, "leaky_relu": 2, "tanh": 3, "sigmoid": 4, "elu": 5,
               "softplus": 6}
ACT_LEAKY_RELU_01 = 7  # tf.keras.layers.LeakyReLU(0.1) (include/dib_st.h)
LOSS_KINDS = {"bce_logits": 0, "bce": 1, "sparse_cce_logits": 2, "mse": 3}
WS_U, WS_PRED, WS_ENC_OUT, WS_G_U, WS_STEP_OUT, WS_G_PRED = range(6)
WS_ENC_H0, WS_INT_H0 = 16, 32
# include/dib_hip.h flag bits
SYNC_WORDS = 1056   # DIB_SYNC_WORDS
FWD_DETERMINISTIC, FWD_INFERENCE, FWD_DEFER_SUMS = 1, 2, 4
HEAD_DEFER_SUMS, HEAD_NO_GRAD, HEAD_DEFER_WGRAD = 1, 2, 4
BWD_INTEGRATION_DONE = 1
TAIL_FINALIZE, TAIL_KL, TAIL_LOSS, TAIL_ADAM, TAIL_BUMP, TAIL_METRICS, TAIL_SGD, TAIL_HEAD_WGRAD, TAIL_LOSS_HEAD = \
    1, 2, 4, 8, 16, 32, 64, 128, 256
SIMILARITIES = {"l2sq": 0, "l2": 1, "l1": 2, "linf": 3, "cosine": 4}


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libdib_hip.so")


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(p) > t for p in _sources())


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    if not force and not _stale():
        return LIB_PATH
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
           os.path.join(CSRC, "dib_api.hip"), "-o", LIB_PATH + f".tmp{os.getpid()}"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
    os.replace(LIB_PATH + f".tmp{os.getpid()}", LIB_PATH)  # per-process temp name: concurrent ranks cannot clobber each other
    return LIB_PATH


_lib = None

# name -> (restype, argtypes); must list every symbol declared in include/dib_hip.h
SIGNATURES = {
    "dib_version": (c_char_p, []),
    "dib_abi_version": (c_int, []),
    "dib_error_string": (c_char_p, [c_int]),
    "dib_layout_create": (c_int, [c_int, POINTER(c_int), c_int, POINTER(c_int), c_int, c_int, POINTER(c_int), c_int,
                                  c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "dib_layout_destroy": (None, [c_void_p]),
    "dib_layout_param_count": (c_int64, [c_void_p]),
    "dib_layout_param_block": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int),
                                       POINTER(c_int)]),
    "dib_layout_table_bytes": (c_int64, [c_void_p]),
    "dib_layout_upload_tables": (c_int, [c_void_p, c_void_p, c_void_p]),
    "dib_layout_set_step_counter": (c_int, [c_void_p, c_void_p]),
    "dib_workspace_bytes": (c_int64, [c_void_p, c_int]),
    "dib_workspace_init": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "dib_workspace_offset": (c_int64, [c_void_p, c_int, c_int]),
    "dib_layout_wgrad_splits": (c_int, [c_void_p, c_int]),
    "dib_workspace_h1_stashed": (c_int, [c_void_p, c_void_p]),
    "dib_workspace_h1_materialize": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_encoder_bank_fwd": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_uint64,
                                     c_uint32, c_int, c_void_p, c_void_p]),
    "dib_integration_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_loss_fwd_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_int, c_void_p,
                                 c_void_p]),
    "dib_integration_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_output_head_fused_supported": (c_int, [c_void_p, c_int]),
    "dib_integration_fwd_hidden": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_output_head_fused": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "dib_integration_head_step": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    "dib_integration_bwd_hidden": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_backward": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]),
    "dib_encoder_bank_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "dib_encoder_bank_input_grad": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_void_p]),
    "dib_encoder_bank_bwd_stage": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]),
    "dib_grads_finalize": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_grads_finalize_part": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_layout_part_range": (c_int, [c_void_p, c_int, POINTER(c_int64), POINTER(c_int64)]),
    "dib_metrics_accumulate": (c_int, [c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dib_step_tail": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                              c_float, c_float, c_float, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dib_set_tuning": (c_int, [c_char_p, c_int]),
    "dib_get_tuning": (c_int, [c_char_p, POINTER(c_int)]),
    "dib_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_float,
                              c_float, c_float, c_void_p]),
    "dib_sgd_step": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_float, c_void_p]),
    "dib_encode_deterministic": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_bhattacharyya": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dib_infonce_workspace_bytes": (c_int64, [c_int]),
    "dib_infonce_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "dib_infonce_batched_workspace_bytes": (c_int64, [c_int, c_int]),
    "dib_infonce_fwd_bwd_batched": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    "dib_positional_encoding": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dib_positional_encoding_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dib_mlp_small_supported": (c_int, [c_void_p, c_int]),
    "dib_mlp_small_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_mlp_small_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "dib_mlp_small_head_supported": (c_int, [c_void_p, c_int]),
    "dib_mlp_small_head_workspace_bytes": (c_int64, [c_void_p, c_int]),
    "dib_mlp_small_head_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_integration_fwd_and_mlp_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                                c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_backward_and_mlp_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "dib_reduce_adam_step": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                     c_float, c_float, c_float, c_float, c_void_p, c_void_p]),
    "dib_mi_workspace_bytes": (c_int64, [c_int, c_int]),
    "dib_mi_sandwich_rows": (c_int, [c_void_p, c_int, c_int, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "dib_philox_normal_fill": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_uint64, c_uint32,
                                       c_void_p]),
    "dib_philox_normal_ref": (c_float, [c_uint64, c_uint32, c_uint32, c_uint32, c_uint32]),
    "dib_mlp_small_head_batched_supported": (c_int, [c_void_p, c_int, c_int]),
    "dib_mlp_small_head_batched_workspace_bytes": (c_int64, [c_void_p, c_int, c_int]),
    "dib_mlp_small_head_step_batched": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_float,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                                c_void_p, c_void_p]),
    "dib_launch_count": (c_int64, []),
    "dib_profile_enable": (c_int, [c_int]),
    "dib_profile_summary": (c_int, [POINTER(ctypes.c_double), POINTER(c_int)]),
    "dib_profile_summary_n": (c_int, [POINTER(ctypes.c_double), POINTER(c_int), c_int]),
    "dib_gemm": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                         c_void_p, c_int, c_int, c_void_p, c_void_p]),
}

# include/dib_st.h: building blocks of the per-particle set transformer
SIGNATURES_ST = {
    "dib_gemm_grouped": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int, c_int, c_int, c_int64, c_void_p]),
    "dib_wgrad_grouped": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_int, c_int64, c_void_p]),
    "dib_reduce_splits": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "dib_reduce_splits_add": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "dib_gemm_skinny_k": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_softmax_rows_fwd": (c_int, [c_void_p, c_int64, c_int, c_int, c_float, c_void_p]),
    "dib_softmax_rows_bwd": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_void_p]),
    "dib_attention_stash_bytes": (c_int64, [c_int, c_int, c_int]),
    "dib_attention_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64, c_float, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "dib_attention_fwd_proj_supported": (c_int, [c_int, c_int, c_int]),
    "dib_attention_fwd_proj": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_float,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_attention_bwd_proj": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_float,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dib_attention_bwd_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "dib_attention_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_add_layernorm_fwd": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int, c_void_p, c_void_p, c_float, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "dib_add_layernorm_bwd_workspace_bytes": (c_int64, [c_int64, c_int]),
    "dib_add_layernorm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "dib_add_layernorm_bwd_fused": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                            c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_st_chain_supported": (c_int, [c_void_p, c_int64]),
    "dib_st_chain_workspace_bytes": (c_int64, [c_int64, c_int]),
    "dib_st_chain_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "dib_st_chain_bwd": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_mean_pool_fwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dib_mean_pool_bwd": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dib_add_inplace": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "dib_act_grad_mul": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "dib_token_kl_workspace_bytes": (c_int64, [c_int64, c_int]),
    "dib_token_reparam_kl_fwd": (c_int, [c_void_p, c_int64, c_int, c_float, c_uint64, c_uint32, c_void_p, c_int64, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p]),
    "dib_token_reparam_kl_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_float, c_void_p,
                                         c_void_p]),
    "dib_mi_probe_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "dib_mi_probe_bounds": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_float, c_uint64, c_uint32, c_uint32, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_loss_rows_workspace_bytes": (c_int64, [c_int]),
    "dib_loss_rows": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "dib_mi_probe_map_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "dib_mi_probe_map": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_uint64,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_mi_sandwich_batched_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "dib_mi_sandwich_batched": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_float, c_uint64, c_uint32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/dib_measure.h: the chaos notebook's measurement-partition model
SIGNATURES_MEASURE = {
    "dib_measure_supported": (c_int, [c_void_p]),
    "dib_measure_workspace_bytes": (c_int64, [c_void_p, c_int]),
    "dib_measure_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_uint64, c_uint32, c_float, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_measure_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_measure_batched_workspace_bytes": (c_int64, [c_void_p, c_int, c_int]),
    "dib_measure_fwd_batched": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_uint32, c_float, c_float,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_measure_bwd_batched": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_uint32, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "dib_measure_symbolize": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dib_measure_posenc_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}

# include/dib_circuit.h: the Boolean-circuit notebook's scalar-channel model
SIGNATURES_CIRCUIT = {
    "dib_circuit_supported": (c_int, [c_int, c_int]),
    "dib_circuit_fwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_uint64, c_uint32, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "dib_circuit_bwd": (c_int, [c_void_p, c_int, c_int, c_void_p, c_uint64, c_uint32, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "dib_circuit_mi_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "dib_circuit_mi_bounds": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_uint64, c_void_p, c_void_p, c_void_p]),
    "dib_circuit_batched_supported": (c_int, [c_void_p, c_int, c_int]),
    "dib_circuit_fwd_batched": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p,
                                        c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_circuit_bwd_batched": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p,
                                        c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "dib_circuit_mi_batched_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "dib_circuit_mi_bounds_batched": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
}

# include/dib_ensemble.h: the lockstep DistributedIBNet ensemble's kernels
SIGNATURES_ENSEMBLE = {
    "dib_ens_supported": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "dib_ens_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "dib_ens_posenc_rows": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "dib_ens_reparam_kl_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "dib_ens_loss": (c_int, [c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dib_ens_reparam_kl_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_int, c_void_p,
                                       c_void_p]),
}

# include/dib_partition.h: the chaos notebook's random-MLP partitions
SIGNATURES_PARTITION = {
    "dib_partition_supported": (c_int, [c_void_p]),
    "dib_partition_symbolize": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
}

# include/dib_mi_channel.h: Monte-Carlo I(U;X) of a known Gaussian channel (the MI-bound characterization notebook)
SIGNATURES_MI_CHANNEL = {
    "dib_mi_monte_carlo_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "dib_mi_monte_carlo": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_uint64, c_uint32, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/dib_mi_features.h: the sandwich bounds of every feature of a DistributedIBNet in one evaluation
SIGNATURES_MI_FEATURES = {
    "dib_mi_features_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "dib_mi_features_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
    "dib_mi_features_bounds": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_int, c_uint64, c_uint32, c_uint32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

# include/dib_compression.h: the compression-scheme matrices of every feature of a DistributedIBNet in one evaluation
SIGNATURES_COMPRESSION = {
    "dib_compression_supported": (c_int, [c_int, c_int, c_int]),
    "dib_compression_gather": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "dib_compression_matrices": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
}


# include/dib_optimizers.h: the Keras optimizer family beyond Adam and momentum-free SGD on a flat buffer
class OptimizerHyper(ctypes.Structure):
    """dib_optimizer_hyper"""
    _fields_ = [("rho", c_float), ("beta_2", c_float), ("epsilon", c_float), ("momentum", c_float),
                ("initial_accumulator", c_float), ("nesterov", c_int32), ("centered", c_int32), ("reserved", c_int32)]


SIGNATURES_OPTIMIZERS = {
    "dib_optimizer_slots": (c_int, [c_int, POINTER(OptimizerHyper)]),
    "dib_optimizer_init": (c_int, [c_int, POINTER(OptimizerHyper), c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "dib_optimizer_step": (c_int, [c_int, POINTER(OptimizerHyper), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_float, c_void_p]),
    "dib_optimizer_advance": (c_int, [c_int, POINTER(OptimizerHyper), c_void_p, c_void_p, c_void_p]),
}


# include/dib_losses.h: the Keras loss and metric family beyond dib_loss_fwd_bwd's four kinds
class LossDesc(ctypes.Structure):
    """dib_loss_desc"""
    _fields_ = [("kind", c_int32), ("metric", c_int32), ("param", c_float)]


SIGNATURES_LOSSES = {
    "dib_loss_ex_supported": (c_int, [POINTER(LossDesc), c_int]),
    "dib_loss_ex_lanes": (c_int, [c_int]),
    "dib_loss_rows_ex": (c_int, [POINTER(LossDesc), c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_int,
                                 c_void_p, c_void_p, c_void_p]),
    "dib_loss_fwd_bwd_ex": (c_int, [c_void_p, POINTER(LossDesc), c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_int,
                                    c_void_p, c_void_p]),
}


# include/dib_grad_transform.h: gradient clipping over the variables of a flat buffer, learning-rate schedules on the device
GRAD_TILE = 4096
CLIP_NONE, CLIP_NORM, CLIP_GLOBAL_NORM = 0, 1, 2
LR_MAX_BOUNDARIES = 8


class GradTile(ctypes.Structure):
    """dib_grad_tile"""
    _fields_ = [("start", c_int64), ("count", c_int32), ("segment", c_int32)]


class GradTable(ctypes.Structure):
    """dib_grad_table"""
    _fields_ = [("n_segments", c_int32), ("reserved", c_int32), ("n_tiles", c_int64), ("seg_tile0", c_void_p),
                ("tiles_dev", c_void_p), ("seg_tile0_dev", c_void_p)]


class LrSchedule(ctypes.Structure):
    """dib_lr_schedule"""
    _fields_ = [("kind", c_int32), ("flags", c_int32), ("initial", c_float), ("decay_steps", c_float), ("rate", c_float),
                ("end", c_float), ("power", c_float), ("alpha", c_float), ("n_boundaries", c_int32), ("reserved", c_int32),
                ("boundaries", c_int64 * LR_MAX_BOUNDARIES), ("values", c_float * (LR_MAX_BOUNDARIES + 1)), ("reserved2", c_float)]

    @classmethod
    def from_fields(cls, d: dict) -> "LrSchedule":
        """from optimizers.Optimizer.lr_schedule() / schedules.LearningRateSchedule.descriptor()"""
        s = cls()
        for k in ("kind", "flags"):
            setattr(s, k, int(d.get(k, 0)))
        for k in ("initial", "decay_steps", "rate", "end", "power", "alpha"):
            setattr(s, k, float(d.get(k, 0.0)))
        b, v = d.get("boundaries", ()), d.get("values", ())
        if len(b) > LR_MAX_BOUNDARIES or len(v) > LR_MAX_BOUNDARIES + 1:
            raise ValueError(f"a schedule has at most {LR_MAX_BOUNDARIES} boundaries")
        s.n_boundaries = len(b)
        for i, x in enumerate(b):
            s.boundaries[i] = int(x)
        for i, x in enumerate(v):
            s.values[i] = float(x)
        return s


SIGNATURES_GRAD_TRANSFORM = {
    "dib_grad_table_from_layout": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64), c_int]),
    "dib_grad_table_tiles": (c_int64, [POINTER(c_int64), POINTER(c_int64), c_int, c_int64, POINTER(GradTile), c_int64,
                                       POINTER(c_int32)]),
    "dib_grad_sumsq": (c_int, [POINTER(GradTable), c_int, c_int, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "dib_grad_clip_apply": (c_int, [POINTER(GradTable), c_int, c_int, c_void_p, c_float, c_float, c_int, c_float, c_void_p, c_void_p,
                                    c_int, c_void_p]),
    "dib_lr_schedule_check": (c_int, [POINTER(LrSchedule)]),
    "dib_lr_schedule_eval": (c_int, [POINTER(LrSchedule), c_void_p, c_void_p, c_void_p]),
}


# include/dib_tabular.h: the tabular front end's quantile transform
TABULAR_MIN_QUANTILES, TABULAR_MAX_QUANTILES, TABULAR_MAX_COLS = 2, 10000, 65535
TABULAR_DISTRIBUTIONS = {"normal": 0, "uniform": 1}
SIGNATURES_TABULAR = {
    "dib_quantile_supported": (c_int, [c_int, c_int, c_int]),
    "dib_quantile_transform": (c_int, [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64,
                                       c_void_p, c_void_p]),
}


# include/dib_subsets.h: I(X_S;Y) of every subset of the features of a small discrete table
SUBSET_MAX_BITS, SUBSET_MAX_CLASSES = 20, 16
SIGNATURES_SUBSETS = {
    "dib_subset_information_supported": (c_int, [c_int, c_int, c_int]),
    "dib_subset_information_workspace_bytes": (c_int64, [c_int, c_int]),
    "dib_subset_information": (c_int, [c_void_p, c_int, c_int, POINTER(c_int), c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
}


# include/dib_ctw_device.h: the CTW entropy-rate estimator built level by level on the device
CTW_DEVICE_MAX_ALPHABET, CTW_DEVICE_MAX_SYMBOLS = 16, 2 ** 31 - 1
CTW_DEVICE_DEEP, CTW_DEVICE_OVERFLOW, CTW_DEVICE_BAD_SYMBOL = 1, 2, 4


class CtwDeviceInfo(ctypes.Structure):
    """dib_ctw_device_info"""
    _fields_ = [("levels", c_int32), ("reserved", c_int32), ("element_steps", c_int64), ("big_nodes", c_int64),
                ("level_seconds", ctypes.c_double), ("mix_seconds", ctypes.c_double)]


SIGNATURES_CTW_DEVICE = {
    "dib_ctw_device_supported": (c_int, [c_int, c_int64, c_int]),
    "dib_ctw_device_workspace_bytes": (c_int64, [c_int64, c_int, c_int, c_int64]),
    "dib_ctw_device_estimate": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_int64, POINTER(CtwDeviceInfo), c_void_p]),
}


class HostGradTable:
    """The host half of a variable table (include/dib_grad_transform.h): segments, the tile work-list, seg_tile0.  No GPU needed;
    `upload(device)` makes the dib_grad_table the launches take (engine.py, dense.py)."""

    def __init__(self, offsets, counts, buffer_elems: int):
        lib = load_library()
        n = len(offsets)
        self.offsets, self.counts = [int(o) for o in offsets], [int(c) for c in counts]
        self.n_segments = n
        off, cnt = (c_int64 * max(1, n))(*self.offsets), (c_int64 * max(1, n))(*self.counts)
        nt = int(lib.dib_grad_table_tiles(off, cnt, n, int(buffer_elems), None, 0, None))
        if nt < 0:
            raise ValueError(f"dib_grad_table_tiles -> {nt}: the segments are not disjoint pieces of a buffer of {buffer_elems} floats")
        self.n_tiles = nt
        self.tiles = (GradTile * max(1, nt))()
        self.seg_tile0 = (c_int32 * (n + 1))()
        got = int(lib.dib_grad_table_tiles(off, cnt, n, int(buffer_elems), self.tiles, nt, self.seg_tile0))
        assert got == nt, (got, nt)

    @classmethod
    def from_layout(cls, layout, buffer_elems: int) -> "HostGradTable":
        lib = load_library()
        n = int(lib.dib_grad_table_from_layout(layout, None, None, 0))
        if n < 0:
            raise DibError(f"dib_grad_table_from_layout -> {n}")
        off, cnt = (c_int64 * n)(), (c_int64 * n)()
        if int(lib.dib_grad_table_from_layout(layout, off, cnt, n)) != n:
            raise DibError("dib_grad_table_from_layout refused its own count")
        return cls(list(off), list(cnt), buffer_elems)

    def segment_range(self, offset: int, count: int):
        """(first, number) of the segments inside [offset, offset + count) - they must be consecutive in the table and none may
        straddle an end of the range (a gradient bucket is a union of whole variables)"""
        inside = [s for s in range(self.n_segments) if offset <= self.offsets[s] and self.offsets[s] + self.counts[s] <= offset + count]
        cut = [s for s in range(self.n_segments) if s not in inside and self.counts[s] > 0
               and self.offsets[s] < offset + count and offset < self.offsets[s] + self.counts[s]]
        if cut or (inside and inside != list(range(inside[0], inside[-1] + 1))):
            raise ValueError(f"[{offset}, {offset + count}) is not a run of whole variables of the table")
        return (inside[0], len(inside)) if inside else (0, 0)

    def upload(self, device):
        """(GradTable, the tensors it points into): tiles and seg_tile0 on `device`"""
        import numpy as np
        import torch
        tiles = np.frombuffer(self.tiles, dtype=np.uint8, count=16 * self.n_tiles).copy()
        tiles_dev = torch.from_numpy(tiles if self.n_tiles else np.zeros(16, np.uint8)).to(device)
        seg_dev = torch.from_numpy(np.frombuffer(self.seg_tile0, dtype=np.int32).copy()).to(device)
        t = GradTable(self.n_segments, 0, self.n_tiles, ctypes.cast(self.seg_tile0, c_void_p), tiles_dev.data_ptr(), seg_dev.data_ptr())
        return t, (tiles_dev, seg_dev, self)


def load_library(build_if_missing: bool = True):
    """dlopen libdib_hip.so and attach signatures.  Raises (no fallback) if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if LIB_OVERRIDE is not None:
        if not os.path.exists(LIB_OVERRIDE):
            raise RuntimeError(f"DIB_LIB_PATH={LIB_OVERRIDE} does not exist")
        return _attach(ctypes.CDLL(os.path.abspath(LIB_OVERRIDE)))
    if build_if_missing and _stale():
        try:
            build_library()
        except Exception:
            if not os.path.exists(LIB_PATH):
                raise
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return _attach(ctypes.CDLL(LIB_PATH))


def _attach(lib):
    global _lib
    try:
        lib.dib_abi_version.restype = c_int
        have = int(lib.dib_abi_version())
    except AttributeError:
        have = None
    # A library of another ABI revision is refused outright: a stale variant build called with shifted arguments would corrupt
    # memory silently.  (Rounds 4-5 had a lenient mode, DIB_LIB_ABI_CHECK=0, that bound only the entry points unchanged since
    # ABI 3 for same-box A/Bs against an older round's library; since ABI 5 every step goes through entry points that
    # did not exist then, so the mode could no longer run a step and was removed - tools/runs/r04g.sh is a historical record.)
    if have != ABI_VERSION:
        raise RuntimeError(f"libdib_hip ABI version {have} != {ABI_VERSION} expected by this binding ({getattr(lib, '_name', '?')}): "
                           "rebuild it (python -c 'import __graft_entry__ as g; g.build()' / tools/build_variant.sh)")
    for name, (res, args) in list(SIGNATURES.items()) + list(SIGNATURES_ST.items()) + list(SIGNATURES_MEASURE.items()) \
            + list(SIGNATURES_CIRCUIT.items()) + list(SIGNATURES_ENSEMBLE.items()) + list(SIGNATURES_PARTITION.items()) + list(SIGNATURES_MI_CHANNEL.items()) + list(SIGNATURES_MI_FEATURES.items()) \
            + list(SIGNATURES_COMPRESSION.items()) + list(SIGNATURES_OPTIMIZERS.items()) + list(SIGNATURES_LOSSES.items()) \
            + list(SIGNATURES_GRAD_TRANSFORM.items()) + list(SIGNATURES_TABULAR.items()) + list(SIGNATURES_SUBSETS.items()) \
            + list(SIGNATURES_CTW_DEVICE.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def set_tuning(key: str, value: int) -> None:
    """include/dib_hip.h dib_set_tuning: the library's only hidden inputs (it reads no environment variable).  The keys are
    listed there; e.g. "wgrad_stream", "gemm_stream", "gemm_stream_rows", "gemm_stream_fill", "wgrad_recompute_h1" (read by the
    forward: set it before the step it is meant for)."""
    check(load_library().dib_set_tuning(key.encode(), int(value)), f"dib_set_tuning({key})")


def get_tuning(key: str) -> int:
    v = c_int()
    check(load_library().dib_get_tuning(key.encode(), ctypes.byref(v)), f"dib_get_tuning({key})")
    return int(v.value)


class DibError(RuntimeError):
    pass


def check(code: int, what: str = "") -> None:
    if code != DIB_OK:
        msg = load_library().dib_error_string(int(code)).decode()
        raise DibError(f"libdib_hip {what} failed: {msg} (code {code})")
