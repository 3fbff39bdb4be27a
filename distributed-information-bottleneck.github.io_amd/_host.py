"""Host-side pieces the product modules share around the C ABI: the launch stream as the library takes it, the (library,
device, stream) handle DenseStack and the model classes launch through, and the carver of a flat workspace."""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def stream_ptr(device) -> ctypes.c_void_p:
    """the device's current torch stream as the hipStream_t argument of an entry point"""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class LibHandle:
    """what DenseStack needs of an engine: the library, the device and the launch stream"""

    def __init__(self, device):
        self.lib = _lib.load_library()
        self.device = torch.device(device)

    def _stream(self):   # (stream_ptr spelled out: DenseStack asks several times per step)
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class Carver:
    """Element offsets of named regions carved one after another out of ONE flat workspace, each starting on a multiple of
    `align` elements: take(name, count) gives the region's offset (kept in `off`), `size` is the workspace's length."""

    def __init__(self, align: int):
        self.align, self.off, self.size = int(align), {}, 0

    def take(self, name: str, count: int) -> int:
        o = self.off[name] = self.size
        self.size = (o + int(count) + self.align - 1) // self.align * self.align
        return o
