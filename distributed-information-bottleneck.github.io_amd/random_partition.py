"""Random-MLP partitions of the chaos paper's Fig. 1 (reference chaos/Chaos_experiments.ipynb cell 7): a random MLP
[d] -> N x Dense(64, act) -> Dense(A) partitions the state space by the index of its output of largest magnitude; the
evaluation trajectory is symbolised through it and the symbol sequence characterised by H(U) and its CTW entropy rate.

Device path: one dib_partition_symbolize launch per chunk (include/dib_partition.h, csrc/dib_partition.h) reads the points
(fp32 or fp64), runs the whole MLP, the argmax of |output| and the symbol histogram, and writes one byte per point.  The
characterisation after it is the CTW estimator (dib_amd.ctw: host C++ by default, ctw_backend="device" for the level build of
csrc/dib_ctw_levels.h) and the Schurmann-Grassberger fit of measurement.characterize_partition.
There is no CPU fallback: a network outside dib_partition_supported raises."""
from __future__ import annotations

import ctypes
import math
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, measurement
from ._gemm_plan import _ptr
from ._host import stream_ptr
from ._lib import ACTIVATIONS, check
from .dense import _MlpDesc

PARTITION_ACTIVATIONS = ("linear", "relu", "leaky_relu", "tanh")
MAX_CTW_THREADS = 16


def ctw_threads() -> int:
    """CTW host threads for the characterisation: OMP_NUM_THREADS if set, else the CPUs this process may run on, at most 16"""
    n = 0
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "") or 0)
    except ValueError:
        n = 0
    if n <= 0:
        try:
            n = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            n = os.cpu_count() or 1
    return max(1, min(MAX_CTW_THREADS, n))


def draw_weights(input_dimension: int, alphabet_size: int, number_mlp_layers: int, units_per_mlp_layer: int = 64,
                 weight_mean: float = 0.05, weight_std: float = 0.5, seed=None) -> List[np.ndarray]:
    """Cell 7's random network in Keras layout [W0, b0, ..., W_out, b_out] (float32): hidden kernels and biases from
    N(weight_mean, weight_std^2) (random_normal(mean=0.05, stddev=0.5)), the output kernel glorot-uniform with limit
    sqrt(6 / (fan_in + A)) and a zero output bias (Keras's Dense defaults).  Host NumPy.

    The distributions are the notebook's; the draws are not: TensorFlow's initializer stream cannot be reproduced here, so a
    seed gives a reproducible network of this package, not the network of a TensorFlow run (load that with set_weights)."""
    rng = np.random.default_rng(seed)
    dims = [int(input_dimension)] + [int(units_per_mlp_layer)] * int(number_mlp_layers)
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        out += [rng.normal(weight_mean, weight_std, (i, o)).astype(np.float32),
                rng.normal(weight_mean, weight_std, o).astype(np.float32)]
    A = int(alphabet_size)
    lim = math.sqrt(6.0 / (dims[-1] + A))
    out += [rng.uniform(-lim, lim, (dims[-1], A)).astype(np.float32), np.zeros(A, dtype=np.float32)]
    return out


def entropy_from_counts(counts) -> float:
    """H(U) in bits from a symbol histogram: the same value as utils.compute_entropy of the sequence it counts"""
    c = np.asarray(counts, dtype=np.int64)
    c = c[c > 0]
    p = c / np.sum(c)
    return float(-np.sum(p * np.log2(p)))


class RandomPartition:
    """One random partition: MLP [input_dimension] -> number_mlp_layers x Dense(units, activation) -> Dense(alphabet_size),
    symbol = argmax |output| (the first index wins ties).  Weights: `weights` (Keras layout) if given, else draw_weights(seed)."""

    def __init__(self, input_dimension: int, alphabet_size: int, number_mlp_layers: int, activation: str,
                 units_per_mlp_layer: int = 64, seed=None, weights: Optional[Sequence[np.ndarray]] = None, device="cuda:0"):
        if activation not in PARTITION_ACTIVATIONS:
            raise ValueError(f"activation {activation!r} outside the kernel's envelope: one of {PARTITION_ACTIVATIONS}")
        self.d, self.A, self.N = int(input_dimension), int(alphabet_size), int(number_mlp_layers)
        self.units, self.activation = int(units_per_mlp_layer), activation
        dims = [self.d] + [self.units] * self.N + [self.A]
        self.dims = list(zip(dims[:-1], dims[1:]))
        d = self._desc = _MlpDesc()
        off = 0
        for l, (i, o) in enumerate(self.dims):   # DenseStack's flat layout: kernel, then bias, each padded to 4 floats
            d.w_off[l] = off; off += (i * o + 3) // 4 * 4
            d.b_off[l] = off; off += (o + 3) // 4 * 4
            d.width[l] = o
        d.n_hidden, d.in_dim, d.n_freq, d.act = self.N, self.d, 1, ACTIVATIONS[activation]
        self.n_params = off
        self.lib = _lib.load_library()
        if not self.lib.dib_partition_supported(ctypes.byref(d)):
            raise ValueError(f"random partition outside the kernel's envelope (dib_partition_supported): d={self.d}, "
                             f"{self.N} hidden layers of {self.units}, A={self.A}: 1 <= d <= 4, 1 to 3 hidden layers, widths "
                             "multiples of 16 up to 128, 2 <= A <= 16")
        if not torch.cuda.is_available():
            raise RuntimeError("RandomPartition runs on the GPU (libdib_hip); no device is available")
        self.device = torch.device(device)
        self.params = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.set_weights(weights if weights is not None else
                         draw_weights(self.d, self.A, self.N, self.units, seed=seed))

    # ---- weights (Keras layout) ---------------------------------------------------------------------------------------------
    def get_weights(self) -> List[np.ndarray]:
        flat = self.params.cpu().numpy()
        out = []
        for l, (i, o) in enumerate(self.dims):
            out += [flat[self._desc.w_off[l]: self._desc.w_off[l] + i * o].reshape(i, o).copy(),
                    flat[self._desc.b_off[l]: self._desc.b_off[l] + o].copy()]
        return out

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        if len(weights) != 2 * len(self.dims):
            raise ValueError(f"expected {2 * len(self.dims)} arrays [kernel, bias] per layer, got {len(weights)}")
        flat = np.zeros(self.n_params, dtype=np.float32)
        for l, (i, o) in enumerate(self.dims):
            w, b = np.asarray(weights[2 * l], dtype=np.float32), np.asarray(weights[2 * l + 1], dtype=np.float32)
            if w.shape != (i, o) or b.shape != (o,):
                raise ValueError(f"layer {l}: kernel {w.shape} / bias {b.shape}, expected ({i}, {o}) / ({o},)")
            flat[self._desc.w_off[l]: self._desc.w_off[l] + i * o] = w.ravel()
            flat[self._desc.b_off[l]: self._desc.b_off[l] + o] = b
        self.params.copy_(torch.from_numpy(flat))

    # ---- symbolisation ------------------------------------------------------------------------------------------------------
    def _input(self, data) -> torch.Tensor:
        """[n, d] float32 / float64 on the device (a 1-D array is d = 1); rows may be strided, features contiguous"""
        x = data if torch.is_tensor(data) else torch.from_numpy(np.asarray(data))
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float32)
        if x.dim() == 1:
            x = x[:, None]
        if x.dim() != 2 or x.shape[1] != self.d:
            raise ValueError(f"data of shape {tuple(x.shape)}: expected [n, {self.d}]")
        if x.stride(1) != 1 or x.stride(0) < self.d:
            x = x.contiguous()
        return x.to(self.device)

    def _launch(self, x: torch.Tensor, sym: torch.Tensor, logits: Optional[torch.Tensor], counts: Optional[torch.Tensor]) -> None:
        st = stream_ptr(self.device)
        check(self.lib.dib_partition_symbolize(ctypes.byref(self._desc), _ptr(self.params), ctypes.c_void_p(x.data_ptr()),
                                               int(x.dtype == torch.float64), x.stride(0), int(x.shape[0]),
                                               ctypes.c_void_p(sym.data_ptr()), _ptr(logits),
                                               ctypes.c_void_p(counts.data_ptr()) if counts is not None else None, st),
              "dib_partition_symbolize")

    def symbolize_device(self, data, chunk_size: int = 1 << 22, return_counts: bool = False):
        """symbolize, the results left on the device: uint8 [n] tensor (and the int64 [A] histogram tensor)"""
        n = int(data.shape[0])
        sym = torch.empty(n, dtype=torch.uint8, device=self.device)
        counts = torch.zeros(self.A, dtype=torch.int64, device=self.device) if return_counts else None
        for c0 in range(0, n, int(chunk_size)):
            c1 = min(n, c0 + int(chunk_size))
            self._launch(self._input(data[c0:c1]), sym[c0:c1], None, counts)
        return (sym, counts) if return_counts else sym

    def symbolize(self, data, chunk_size: int = 1 << 22, return_counts: bool = False):
        """uint8 [n] symbols of the points data [n, d] (float32 or float64), and with return_counts the int64 [A] histogram.
        Host arrays are copied to the device one chunk at a time; one launch per chunk, the counts accumulate on the device."""
        out = self.symbolize_device(data, chunk_size, return_counts)
        return (out[0].cpu().numpy(), out[1].cpu().numpy()) if return_counts else out.cpu().numpy()

    def logits(self, data) -> np.ndarray:
        """float32 [n, A] outputs of the network (for inspection and tests)"""
        x = self._input(data)
        n = int(x.shape[0])
        sym = torch.empty(n, dtype=torch.uint8, device=self.device)
        out = torch.empty((n, self.A), dtype=torch.float32, device=self.device)
        self._launch(x, sym, out, None)
        return out.cpu().numpy()

    def characterize(self, data_or_symbols, number_data_points=None, number_rand_draws: int = 5, seed: int = 0,
                     threads: Optional[int] = None, ctw_backend: str = "host") -> dict:
        """H(U) from the kernel's symbol histogram (or of the given uint8 symbols) and the entropy rate from the CTW windows and
        Schurmann-Grassberger fit of measurement.characterize_partition; threads: CTW host threads (default ctw_threads()).
        ctw_backend "device": the symbols stay on the device between the symbolise kernel and the CTW level build (uint8
        symbols given as a CUDA tensor are used where they lie); the result gains "ctw_details"."""
        arr = data_or_symbols
        if isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and arr.ndim == 1:
            sym, counts = arr, np.bincount(arr, minlength=self.A)
        elif ctw_backend == "device" and torch.is_tensor(arr) and arr.dtype == torch.uint8 and arr.dim() == 1:
            sym = arr.to(self.device)
            counts = torch.bincount(sym.to(torch.int64), minlength=self.A).cpu().numpy()
        elif ctw_backend == "device":
            sym, counts = self.symbolize_device(arr, return_counts=True)
            counts = counts.cpu().numpy()
        else:
            sym, counts = self.symbolize(arr, return_counts=True)
        out = measurement.entropy_rate_fit(sym, self.A, number_data_points, number_rand_draws, seed,
                                           threads=ctw_threads() if threads is None else threads, ctw_backend=ctw_backend)
        out["entropy_single_timestep"] = entropy_from_counts(counts)
        return out


# ---- cell 7 ---------------------------------------------------------------------------------------------------------------
def _symbolize_partition(weights, activation: str, trajectory, cache: dict, on_device: bool = False):
    """(symbols, counts) of the trajectory through one network; the trajectory is copied to the device once per survey.
    on_device: the symbols stay a device tensor (the counts come to the host either way)"""
    if "x" not in cache:
        cache["x"] = torch.from_numpy(np.ascontiguousarray(trajectory)).to("cuda")
    x = cache["x"]
    rp = RandomPartition(x.shape[1], weights[-1].shape[0], len(weights) // 2 - 1, activation, weights[0].shape[1],
                         weights=weights)
    if on_device:
        sym, counts = rp.symbolize_device(x, chunk_size=max(1, int(x.shape[0])), return_counts=True)
        return sym, counts.cpu().numpy()
    return rp.symbolize(x, chunk_size=max(1, int(x.shape[0])), return_counts=True)


def partition_seed(seed: int, rand_iter: int, alphabet_size: int, number_mlp_layers: int, activation: str) -> int:
    """the seed of one partition's weights (and of its CTW windows): a function of the survey seed and the configuration"""
    ss = np.random.SeedSequence([int(seed), int(rand_iter), int(alphabet_size), int(number_mlp_layers),
                                 PARTITION_ACTIVATIONS.index(activation)])
    return int(ss.generate_state(1, np.uint32)[0])


def partition_file_name(number_mlp_layers: int, activation: str, alphabet_size: int, rand_iter: int) -> str:
    return f"{number_mlp_layers}layers_{activation}_{alphabet_size}alphabet_{rand_iter}.npz"


def random_partition_survey(trajectory, alphabet_sizes=(2, 4), layer_counts=(1, 2, 3), activations=("tanh", "relu"),
                            number_random_repeats: int = 1, seed: int = 0, entropy_threshold: float = 0.1,
                            number_data_points=None, number_rand_draws: int = 5, out_dir: Optional[str] = None,
                            save_point_assignments: bool = False, threads: Optional[int] = None,
                            units_per_mlp_layer: int = 64, ctw_backend: str = "host") -> List[Dict]:
    """Cell 7: for rand_iter, then A, then N, then the activation (the notebook's loop order), a random network of
    draw_weights(seed=partition_seed(...)) symbolises the whole trajectory; a partition with H(U) < entropy_threshold bits is
    skipped (no entropy rate, no file); otherwise its entropy rate comes from CTW windows (number_data_points: the 15 log-spaced
    lengths 2e3 .. 2e6 by default, number_rand_draws each) and the fit.  With out_dir, writes
    {N}layers_{act}_{A}alphabet_{iter}.npz with cell 7's keys (and the first 64 000 points and symbols with
    save_point_assignments), which cell 8 reads back.  Returns one record per partition, skipped ones included.
    ctw_backend "device": the symbols go from the symbolise kernel to the CTW level build without leaving the device
    (measurement.entropy_rate_fit); the same windows are drawn."""
    if ctw_backend not in ("host", "device"):
        raise ValueError(f"ctw_backend is 'host' or 'device'; got {ctw_backend!r}")
    traj = np.asarray(trajectory)
    if traj.ndim == 1:
        traj = traj[:, None]
    d = traj.shape[1]
    th = ctw_threads() if threads is None else int(threads)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    cache: dict = {}
    records = []
    for rand_iter in range(int(number_random_repeats)):
        for A in alphabet_sizes:
            for N in layer_counts:
                for act in activations:
                    ps = partition_seed(seed, rand_iter, A, N, act)
                    rec = {"rand_iter": rand_iter, "alphabet_size": int(A), "number_mlp_layers": int(N), "activation": act,
                           "seed": ps}
                    t0 = time.perf_counter()
                    w = draw_weights(d, A, N, units_per_mlp_layer, seed=ps)
                    if ctw_backend == "device":
                        sym, counts = _symbolize_partition(w, act, traj, cache, on_device=True)
                    else:
                        sym, counts = _symbolize_partition(w, act, traj, cache)
                    t1 = time.perf_counter()
                    h_u = entropy_from_counts(counts)
                    rec.update(entropy_single_timestep=h_u, counts=np.asarray(counts).tolist(), symbolize_s=t1 - t0)
                    if h_u < entropy_threshold:   # ~the whole attractor is one symbol
                        rec.update(skipped=True, entropy_rate=None, entropy_rate_err=None, file=None)
                        records.append(rec)
                        continue
                    fit = measurement.entropy_rate_fit(sym, A, number_data_points, number_rand_draws, ps, threads=th,
                                                       ctw_backend=ctw_backend)
                    rec.update(skipped=False, entropy_rate=fit["entropy_rate"], entropy_rate_err=fit["entropy_rate_err"],
                               entropy_rate_values=fit["entropy_rate_values"], characterize_s=time.perf_counter() - t1,
                               file=None)
                    if out_dir is not None:
                        f = os.path.join(out_dir, partition_file_name(N, act, A, rand_iter))
                        arrs = dict(entropy_rate_values=fit["entropy_rate_values"], entropy_single_timestep=h_u,
                                    entropy_rate=fit["entropy_rate"], entropy_rate_err=fit["entropy_rate_err"])
                        if save_point_assignments:
                            arrs["raw_data_points"] = traj[:64_000]
                            arrs["symbolic_sequence"] = np.asarray(sym[:64_000].cpu() if torch.is_tensor(sym) else sym[:64_000])
                        np.savez(f, **arrs)
                        rec["file"] = f
                    records.append(rec)
    return records
