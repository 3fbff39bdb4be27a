"""Context-tree-weighting entropy-rate estimator: Python surface of csrc/dib_ctw.cpp (include/dib_ctw.h).

Mirrors the reference's Cython module `ctw` (reference chaos/ctw.pyx:2, chaos/README.MD usage):

    from dib_amd.ctw import estimate_entropy
    estimate_entropy(seq, alphabet_size)          # bits per symbol, same value as the reference build

plus `estimate_entropy_batch` for the notebook's "75 sequences per partition" pattern (host threads).  The host library is
built in-tree with g++ on first use and needs no GPU.

`estimate_entropy_windows` estimates many windows of ONE symbol sequence; its default backend builds the same tree level by
level on the device (include/dib_ctw_device.h, csrc/dib_ctw_levels.h: the final tree does not depend on the order in which the
positions were inserted, up to depth 512), and recomputes on the host the windows the device build does not cover.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_int, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "dib_ctw.cpp")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "dib_ctw.h")
LIB_PATH = os.path.join(_HERE, "libdib_ctw.so")

SIGNATURES = {
    "dib_ctw_version": (c_char_p, []),
    "dib_ctw_estimate_entropy": (c_int, [c_void_p, c_int64, c_int, POINTER(c_double)]),
    "dib_ctw_estimate_entropy_batch": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "dib_ctw_node_count": (c_int, [c_void_p, c_int64, c_int, POINTER(c_int64)]),
}
_ERRORS = {-1: "invalid argument (empty pointer, alphabet outside [1,127] or symbol outside [0, alphabet))",
           -2: "out of memory while building the context tree"}
_lib = None


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.exists(p) and os.path.getmtime(p) > t for p in (SRC, HEADER))


def build_library(force: bool = False, verbose: bool = False) -> str:
    """g++ -O2 (no fast-math: results must stay bit-identical to the reference arithmetic)."""
    if not force and not _stale():
        return LIB_PATH
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        raise RuntimeError("g++ not found: cannot build libdib_ctw.so")
    cmd = [cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", SRC, "-o", LIB_PATH + f".tmp{os.getpid()}"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed:\n" + res.stdout + res.stderr)
    os.replace(LIB_PATH + f".tmp{os.getpid()}", LIB_PATH)  # per-process temp name: concurrent ranks cannot clobber each other
    return LIB_PATH


def load_library():
    global _lib
    if _lib is None:
        if _stale():
            try:
                build_library()
            except Exception:
                if not os.path.exists(LIB_PATH):
                    raise
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _symbols(seq, alphabet_size: int) -> np.ndarray:
    a = np.asarray(seq)
    if a.ndim != 1:
        a = a.reshape(-1)
    if a.size and (a.min() < 0 or a.max() >= alphabet_size):
        raise ValueError(f"symbols must lie in [0, {alphabet_size})")
    return np.ascontiguousarray(a, dtype=np.int8)


def _check(rc: int) -> None:
    if rc != 0:
        raise ValueError("dib_ctw: " + _ERRORS.get(rc, f"error {rc}"))


def estimate_entropy(seq, alphabet_size: int) -> float:
    """Entropy rate (bits/symbol) of a symbol sequence - drop-in for reference chaos/ctw.pyx:2."""
    alphabet_size = int(alphabet_size)
    if not 1 <= alphabet_size <= 127:
        raise ValueError("alphabet_size must be in [1, 127]")
    s = _symbols(seq, alphabet_size)
    out = c_double()
    _check(load_library().dib_ctw_estimate_entropy(s.ctypes.data, s.size, alphabet_size, ctypes.byref(out)))
    return out.value


def estimate_entropy_batch(seqs, alphabet_size: int, threads: int = 0, backend: str = "host") -> np.ndarray:
    """Entropy rates of many sequences (list of 1-D arrays, or a 2-D array of equal-length rows), computed on
    `threads` host threads (0 = all).  backend "device": the sequences are laid end to end, uploaded once and estimated as
    windows (estimate_entropy_windows); rates then agree with the host's to one float32 step."""
    if backend not in ("host", "device"):
        raise ValueError(f"backend is 'host' or 'device'; got {backend!r}")
    alphabet_size = int(alphabet_size)
    if not 1 <= alphabet_size <= 127:
        raise ValueError("alphabet_size must be in [1, 127]")
    parts = [_symbols(s, alphabet_size) for s in seqs]
    if backend == "device":
        lengths = np.array([p.size for p in parts], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if parts else np.zeros(0, np.int64)
        flat = np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, dtype=np.uint8)
        return estimate_entropy_windows(flat, starts, lengths, alphabet_size, backend="device", threads=threads)
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    if parts:
        offsets[1:] = np.cumsum([p.size for p in parts])
    flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int8)
    out = np.empty(len(parts), dtype=np.float64)
    _check(load_library().dib_ctw_estimate_entropy_batch(flat.ctypes.data, offsets.ctypes.data, len(parts), alphabet_size,
                                                        int(threads), out.ctypes.data))
    return out


def node_count(seq, alphabet_size: int) -> int:
    """Size of the suffix tree built for `seq` (memory: 8*alphabet_size + 8 bytes per node)."""
    s = _symbols(seq, int(alphabet_size))
    out = c_int64()
    _check(load_library().dib_ctw_node_count(s.ctypes.data, s.size, int(alphabet_size), ctypes.byref(out)))
    return out.value


# ---- windows of one sequence, on the device --------------------------------------------------------------------------------
STATUS_OK, STATUS_DEEP, STATUS_OVERFLOW, STATUS_BAD_SYMBOL = 0, 1, 2, 4   # include/dib_ctw_device.h
DEFAULT_WORKSPACE_BUDGET = 8 << 30
NODES_PER_SYMBOL = 4   # node capacity asked for per window symbol: about 1.5 are used on a chaotic sequence
# ... and a floor for short windows with long repeats: a window that goes down to level 512 can fill up to length / 2 nodes on
# every level (the near-constant sequences of 2000 symbols in the tests take 1.1e5), which no multiple of its length covers
MIN_NODE_CAPACITY = 1 << 18


def _node_capacity(total: int, windows: int) -> int:
    return NODES_PER_SYMBOL * total + windows + MIN_NODE_CAPACITY


def _plan_chunks(lib, lengths: np.ndarray, alphabet_size: int, budget: int):
    """[(first, last + 1, node_capacity)]: consecutive windows whose workspace (sized from the sum of their lengths) fits the
    budget.  A window that does not fit on its own gets the node capacity the budget leaves it (None: not even the minimum)."""
    from ._lib import CTW_DEVICE_MAX_SYMBOLS
    need = lambda total, count, cap: int(lib.dib_ctw_device_workspace_bytes(int(total), int(count), alphabet_size, int(cap)))
    chunks, first, total = [], 0, 0
    for w, n in enumerate(lengths.tolist()):
        if w > first:
            t = total + n
            if t > CTW_DEVICE_MAX_SYMBOLS or need(t, w + 1 - first, _node_capacity(t, w + 1 - first)) > budget:
                chunks.append((first, w, _node_capacity(total, w - first)))
                first, total = w, 0
        total += n
    if len(lengths) > first:
        chunks.append((first, len(lengths), _node_capacity(total, len(lengths) - first)))
    out = []
    for a, b, cap in chunks:
        total = int(lengths[a:b].sum())
        if b - a == 1 and (total > CTW_DEVICE_MAX_SYMBOLS or need(total, 1, cap) > budget):
            lo, hi = 1, cap    # the largest capacity that fits (the workspace grows with it)
            if total > CTW_DEVICE_MAX_SYMBOLS or need(total, 1, lo) > budget:
                out.append((a, b, None))
                continue
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if need(total, 1, mid) <= budget else (lo, mid - 1)
            cap = lo
        out.append((a, b, cap))
    return out


def estimate_entropy_windows(symbols, starts, lengths, alphabet_size: int, backend: str = "device", return_details: bool = False,
                             threads: int = 0, workspace_budget: int = DEFAULT_WORKSPACE_BUDGET):
    """Entropy rates (bits / symbol, float64 [n_windows]) of the windows symbols[starts[w] : starts[w] + lengths[w]] of one symbol
    sequence.  symbols: a NumPy array, or a CUDA uint8 tensor, which the device backend uses where it lies.

    backend "device" (libdib_hip; no device, no result): the windows are estimated in chunks whose workspace, sized from the sum
    of the chunk's lengths, fits `workspace_budget` bytes.  A window the level build marks deep (a context longer than 512
    symbols repeats), one that overflows the node capacity even in a call of its own, and one too large for the budget are
    recomputed with the host estimator on `threads` threads; every other rate is the device's, the host's float32 value or one
    of its neighbours.  A symbol outside [0, alphabet_size) raises as on the host.  backend "host": estimate_entropy_batch of the
    windows.

    return_details: (rates, details) with per window `status` (the device's: 0 ok, 1 deep, 2 overflow; -1 not run),
    `nodes` (tree size, -1 where the host recomputed), `code_length_bits` (unrounded L_w(root), NaN where the host
    recomputed), `fallback` (True where the host recomputed), and per call `chunks`, `levels`, `element_steps`, `level_seconds`,
    `mix_seconds`, `readback_seconds`, `symbols_on_device` (the sequence was a device tensor and was not copied)."""
    if backend not in ("host", "device"):
        raise ValueError(f"backend is 'host' or 'device'; got {backend!r}")
    alphabet_size = int(alphabet_size)
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
    lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    W = int(starts.size)
    if lengths.size != W:
        raise ValueError(f"{W} starts, {lengths.size} lengths")
    is_tensor = hasattr(symbols, "data_ptr")
    n_symbols = int(symbols.numel()) if is_tensor else int(np.asarray(symbols).size)
    if W and (starts.min() < 0 or lengths.min() < 0 or (starts + lengths).max() > n_symbols):
        raise ValueError(f"a window leaves the sequence of {n_symbols} symbols")

    def host_rates(which):
        host = symbols.detach().cpu().numpy().reshape(-1) if is_tensor else np.asarray(symbols).reshape(-1)
        return estimate_entropy_batch([host[starts[w]: starts[w] + lengths[w]] for w in which], alphabet_size, threads=threads)

    if backend == "host":
        rates = host_rates(range(W))
        if not return_details:
            return rates
        return rates, {"status": np.full(W, -1, np.int32), "nodes": np.full(W, -1, np.int64), "code_length_bits": np.full(W, np.nan),
                       "fallback": np.ones(W, dtype=bool), "chunks": 0, "levels": 0, "element_steps": 0, "level_seconds": 0.0,
                       "mix_seconds": 0.0, "readback_seconds": 0.0, "symbols_on_device": False}

    import time
    import torch
    from . import _lib
    from ._host import stream_ptr
    if not 1 <= alphabet_size <= _lib.CTW_DEVICE_MAX_ALPHABET:
        raise ValueError(f"alphabet_size {alphabet_size} outside the device estimator's envelope [1, {_lib.CTW_DEVICE_MAX_ALPHABET}]")
    if not torch.cuda.is_available():
        raise RuntimeError("estimate_entropy_windows(backend='device') runs on the GPU (libdib_hip); no device is available - "
                           "backend='host' is the host estimator")
    lib = _lib.load_library()
    on_device = bool(is_tensor and symbols.is_cuda and symbols.dtype == torch.uint8 and symbols.dim() == 1 and symbols.is_contiguous())
    if on_device:
        sym = symbols
    elif is_tensor:
        sym = symbols.reshape(-1).to(device="cuda", dtype=torch.uint8).contiguous()
    else:
        a = np.asarray(symbols).reshape(-1)
        if a.size and (a.min() < 0 or a.max() >= alphabet_size):
            raise ValueError(f"symbols must lie in [0, {alphabet_size})")
        sym = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to("cuda")
    dev = sym.device
    rates = np.full(W, np.nan)
    details = {"status": np.full(W, -1, np.int32), "nodes": np.full(W, -1, np.int64), "code_length_bits": np.full(W, np.nan),
               "fallback": np.zeros(W, dtype=bool), "chunks": 0, "levels": 0, "element_steps": 0, "level_seconds": 0.0,
               "mix_seconds": 0.0, "readback_seconds": 0.0, "symbols_on_device": on_device}

    def run(which: np.ndarray, cap: int) -> None:
        n, total = int(which.size), int(lengths[which].sum())
        nws = int(lib.dib_ctw_device_workspace_bytes(total, n, alphabet_size, cap))
        ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=dev)
        out = torch.empty((3, n), dtype=torch.float64, device=dev)   # code bits, rates, nodes (int64 bits)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        info = _lib.CtwDeviceInfo()
        s_, l_ = np.ascontiguousarray(starts[which]), np.ascontiguousarray(lengths[which])
        with torch.cuda.device(dev):
            _lib.check(lib.dib_ctw_device_estimate(c_void_p(sym.data_ptr()), n_symbols, s_.ctypes.data, l_.ctypes.data, n,
                                                   alphabet_size, cap, c_void_p(out[0].data_ptr()), c_void_p(out[1].data_ptr()),
                                                   c_void_p(out[2].data_ptr()), c_void_p(st.data_ptr()), c_void_p(ws.data_ptr()), nws,
                                                   ctypes.byref(info), stream_ptr(dev)),
                       "dib_ctw_device_estimate")
        t0 = time.perf_counter()
        o, s = out.cpu().numpy(), st.cpu().numpy()
        details["readback_seconds"] += time.perf_counter() - t0
        rates[which], details["code_length_bits"][which], details["nodes"][which] = o[1], o[0], o[2].view(np.int64)
        details["status"][which] = s
        details["chunks"] += 1
        details["levels"] = max(details["levels"], int(info.levels))
        details["element_steps"] += int(info.element_steps)
        details["level_seconds"] += float(info.level_seconds)
        details["mix_seconds"] += float(info.mix_seconds)

    for a, b, cap in _plan_chunks(lib, lengths, alphabet_size, int(workspace_budget)):
        which = np.arange(a, b)
        if cap is None:
            details["status"][which] = STATUS_OVERFLOW
            continue
        run(which, cap)
        if b - a > 1:   # the capacity is shared: a window that overflowed among others gets a call of its own
            for w in which[(details["status"][which] & STATUS_OVERFLOW) != 0]:
                (_, _, own), = _plan_chunks(lib, lengths[w: w + 1], alphabet_size, int(workspace_budget))
                if own is not None:
                    run(np.array([w]), own)
    if W and np.any((details["status"] > 0) & ((details["status"] & STATUS_BAD_SYMBOL) != 0)):
        raise ValueError(f"symbols must lie in [0, {alphabet_size})")
    again = np.where(details["status"] != STATUS_OK)[0]
    if again.size:
        rates[again] = host_rates(again)
        details["fallback"][again] = True
        details["nodes"][again] = -1
        details["code_length_bits"][again] = np.nan
    return (rates, details) if return_details else rates
