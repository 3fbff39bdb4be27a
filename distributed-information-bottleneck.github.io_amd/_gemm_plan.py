"""Grouped-GEMM launch records shared by the host classes that drive `dib_gemm_grouped` (include/dib_st.h) directly:
SetTransformerDIB (its plans: _st_plan.py) and DenseStack (dense.py).  A `_Gemm` is one launch: a device-resident descriptor
table (one `dib_gemm_desc` per group: element offsets into the base tensors, leading dimensions, M/N/K) plus the base
tensors; the tables are built and uploaded once per batch shape, so a step is a sequence of C-ABI calls with no per-call
descriptor traffic."""
from __future__ import annotations

from ctypes import c_void_p
from typing import Optional

import numpy as np
import torch

from ._lib import check

DESC = np.dtype([("a_off", "<i8"), ("b_off", "<i8"), ("c_off", "<i8"), ("bias_off", "<i8"), ("aux_off", "<i8"),
                 ("a_boff", "<i8"), ("b_boff", "<i8"), ("c_boff", "<i8"), ("aux_boff", "<i8"),
                 ("M", "<i4"), ("N", "<i4"), ("K", "<i4"), ("lda", "<i4"), ("ldb", "<i4"), ("ldc", "<i4"), ("ldaux", "<i4"),
                 ("flags", "<i4")])
assert DESC.itemsize == 104  # include/dib_st.h: dib_gemm_desc


def _ptr(t: Optional[torch.Tensor], off: int = 0):
    return c_void_p(t.data_ptr() + 4 * off) if t is not None else c_void_p(0)


def _ptr8(t: Optional[torch.Tensor]):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def _ptr_array3(t: torch.Tensor, offs):
    """void*[3] of up to three regions of `t` (element offsets), NULL beyond: the per-layer row buffers of dib_mlp_small_*"""
    return (c_void_p * 3)(*([_ptr(t, o).value for o in offs] + [None] * (3 - len(offs))))


def slab_rule(n: int):
    """(nsplit, rows_per_split) of a weight gradient contracted over n batch rows: slabs of >= 64 rows (a multiple of 32), at
    most 32 of them, summed in a fixed order afterwards"""
    nsplit = max(1, min(32, n // 64))
    rps = ((n + nsplit - 1) // nsplit + 31) // 32 * 32
    return (n + rps - 1) // rps, rps


class _Gemm:
    """One grouped-GEMM launch: a device descriptor table + base tensors.  A base tensor may be given by NAME when the table
    is built before its memory exists; `bind` resolves the names."""

    def __init__(self, mode, descs, A, B, C, bias=None, aux=None, bias_out=None, act=0, nsplit=1, rows_per_split=0,
                 split_stride=0):
        self.mode, self.n = mode, len(descs)
        self.max_m = int(max(d["M"] for d in descs))
        self.max_n = int(max(d["N"] for d in descs))
        arr = np.zeros(len(descs), dtype=DESC)
        for k in descs[0]:   # (all descriptors of a table come from the same constructor: same fields)
            arr[k] = [d[k] for d in descs]
        self.host = arr
        self.dev = None
        self.A, self.B, self.C, self.bias, self.aux, self.bias_out = A, B, C, bias, aux, bias_out
        self.act, self.nsplit, self.rps, self.stride = act, nsplit, rows_per_split, split_stride

    def bind(self, bases):
        for k in ("A", "B", "C", "bias", "aux", "bias_out"):
            if isinstance(getattr(self, k), str):
                setattr(self, k, bases[getattr(self, k)])

    def upload(self, device):
        self.dev = torch.from_numpy(self.host.view(np.uint8).copy()).to(device)

    def run(self, lib, stream):
        check(lib.dib_gemm_grouped(self.mode, self.n, _ptr(self.dev), self.max_m, self.max_n, _ptr(self.A), _ptr(self.B),
                                   _ptr(self.C), _ptr(self.bias), _ptr(self.aux), _ptr(self.bias_out), self.act, self.nsplit,
                                   self.rps, self.stride, stream), "dib_gemm_grouped")


class _SkinnyKGemm(_Gemm):
    """The same launch record for `dib_gemm_skinny_k` (include/dib_st.h): mode 0 / 1 products whose contraction is at most
    32 wide and whose output is large - a streaming kernel bound by its output stores.  All groups share M, N, K."""

    @staticmethod
    def fits(mode, descs, act=0, aux=None) -> bool:
        d0 = descs[0]
        return (mode in (0, 1) and act == 0 and aux is None and 0 < d0["K"] <= 32 and d0["K"] % 4 == 0 and d0["N"] % 32 == 0
                and all((d["M"], d["N"], d["K"]) == (d0["M"], d0["N"], d0["K"]) for d in descs))

    def run(self, lib, stream):
        d0 = self.host[0]
        check(lib.dib_gemm_skinny_k(self.mode, self.n, _ptr(self.dev), int(d0["M"]), int(d0["N"]), int(d0["K"]), _ptr(self.A),
                                    _ptr(self.B), _ptr(self.C), _ptr(self.bias), stream), "dib_gemm_skinny_k")


def _d(a_off, lda, b_off, ldb, c_off, ldc, M, N, K, bias_off=-1, aux_off=0, ldaux=0):
    return dict(a_off=a_off, b_off=b_off, c_off=c_off, bias_off=bias_off, aux_off=aux_off, M=M, N=N, K=K, lda=lda, ldb=ldb,
                ldc=ldc, ldaux=ldaux)


class _SplitKGemm:
    """A skinny product C[M, N] = A[M, K] @ W (N = the model width, 32; K = heads * key_dim = 1536) with FEW row tiles: the
    output has ceil(M / 64) workgroups' worth of tiles and each would walk all of K with one tile of prefetch - at the
    notebook's size (1600 tokens) 25 workgroups x 48 dependent k-tiles = 84 us for 0.16 GFLOP, the two slowest launches of
    the whole step.  Here the contraction is cut into `ksplit` chunks that run as extra GROUPS of the same grouped launch
    (one partial slab each), summed in a fixed order by dib_reduce_splits: deterministic, no new kernel."""

    def __init__(self, gemm: _Gemm, partial, partial_off, n, nslabs, out, out_off, mode: str = "store"):
        """mode: "store" out = sum of the slabs; "add" out += sum (a residual branch's gradient joins the one already there:
        one launch instead of reduce + add); "defer" no reduce here - the consumer sums the slabs itself
        (dib_add_layernorm_fwd's b_slabs)."""
        self.gemm, self.partial, self.partial_off, self.n, self.nslabs, self.out, self.out_off, self.mode = \
            gemm, partial, partial_off, n, nslabs, out, out_off, mode

    def bind(self, bases):
        self.gemm.bind(bases)
        self.partial, self.out = bases[self.partial], bases[self.out]

    def upload(self, device):
        self.gemm.upload(device)

    def run(self, lib, stream):
        self.gemm.run(lib, stream)
        if self.mode == "defer":
            return
        fn = lib.dib_reduce_splits_add if self.mode == "add" else lib.dib_reduce_splits
        check(fn(_ptr(self.partial, self.partial_off), self.n, self.nslabs, self.n, _ptr(self.out, self.out_off), stream),
              "dib_reduce_splits")
