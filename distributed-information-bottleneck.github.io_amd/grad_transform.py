"""Launch sequencing of include/dib_grad_transform.h for ONE flat gradient buffer: the variable table (made and uploaded once),
the tile partials and the float64 sums of squares.  HipEngine and DenseStack each own one; fit_infonce binds both to one `ss`
array so that global_clipnorm takes its norm over the X model and the Y encoder together (reference train.py:196-219: one
optimizer, one gradient list).

`clip` below is optimizers.Optimizer.clip(): (clipvalue or 0.0, DIB_CLIP_* mode, norm threshold).
Launches per buffer and step: clipvalue alone 1 (apply); clipnorm / global_clipnorm 3 (tile sums, segment sums, apply)."""
from __future__ import annotations

import ctypes
from ctypes import c_void_p

import torch

from . import _lib
from ._lib import check


def _ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class GradTransform:
    def __init__(self, lib, host_table: "_lib.HostGradTable", grads: torch.Tensor, stream):
        self.lib, self.host, self.grads, self._stream = lib, host_table, grads, stream
        self.table, self._keep = host_table.upload(grads.device)
        self.partials = torch.zeros(max(1, host_table.n_tiles), dtype=torch.float64, device=grads.device)
        self.bind_ss(torch.zeros(max(1, host_table.n_segments), dtype=torch.float64, device=grads.device), 0)

    @property
    def n_segments(self) -> int:
        return self.host.n_segments

    def bind_ss(self, ss_all: torch.Tensor, first: int) -> None:
        """this buffer's sums of squares live at ss_all[first : first + n_segments]; the global norm is taken over all of ss_all"""
        assert ss_all.dtype == torch.float64 and first + self.n_segments <= ss_all.numel()
        self.ss_all, self.ss = ss_all, ss_all[first: first + max(1, self.n_segments)]

    def unbind_ss(self) -> None:
        """back to an ss array of this buffer alone"""
        self.bind_ss(torch.zeros(max(1, self.n_segments), dtype=torch.float64, device=self.grads.device), 0)

    def _range(self, seg_range):
        return (0, self.n_segments) if seg_range is None else seg_range

    def sumsq(self, clip, seg_range=None, grad_scale: float = 1.0) -> None:
        """ss[s] of the segments of the range (two launches)"""
        first, count = self._range(seg_range)
        check(self.lib.dib_grad_sumsq(ctypes.byref(self.table), first, count, _ptr(self.grads), float(grad_scale), float(clip[0]),
                                      _ptr(self.partials), _ptr(self.ss), self._stream()), "dib_grad_sumsq")

    def apply(self, clip, seg_range=None, grad_scale: float = 1.0) -> None:
        """grads <- the transformed gradient on the segments of the range (one launch); a norm mode reads what sumsq wrote"""
        first, count = self._range(seg_range)
        check(self.lib.dib_grad_clip_apply(ctypes.byref(self.table), first, count, _ptr(self.grads), float(grad_scale),
                                           float(clip[0]), int(clip[1]), float(clip[2]), _ptr(self.ss), _ptr(self.ss_all),
                                           int(self.ss_all.numel()), self._stream()), "dib_grad_clip_apply")

    def transform(self, clip, seg_range=None, grad_scale: float = 1.0) -> None:
        """the whole transform of one buffer that stands alone (its ss array holds no other buffer's variables)"""
        if clip[1] != _lib.CLIP_NONE:
            self.sumsq(clip, seg_range, grad_scale)
        self.apply(clip, seg_range, grad_scale)


def eval_lr(lib, descriptor: dict, t_dev: torch.Tensor, lr_dev: torch.Tensor, stream) -> None:
    """lr_dev <- schedule(t_dev) on the device (one thread): before the step's first launch that reads lr_dev"""
    s = _lib.LrSchedule.from_fields(descriptor)
    check(lib.dib_lr_schedule_eval(ctypes.byref(s), _ptr(t_dev), _ptr(lr_dev), stream), "dib_lr_schedule_eval")
