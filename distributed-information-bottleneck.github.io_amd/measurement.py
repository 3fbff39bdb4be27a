"""Measurement-partition optimisation of the chaos paper (reference chaos/Chaos_experiments.ipynb cells 3 and 10): a
distributed-IB encoder of one state, a soft vector quantiser (the partition), an aggregator of L soft symbols and a
reference-state encoder, matched with a symmetric InfoNCE loss; then the trained partition symbolises a trajectory and the
symbol sequence is characterised by its entropy and its CTW entropy rate.

Device path of one training step (include/dib_measure.h, csrc/dib_measure.h; the rest are existing library kernels):
    IB encoder forward of traj[start_b + l]      DenseStack (gather + PositionalEncoding + GEMMs)
    dib_measure_fwd                              KL partials, reparameterisation, VQ chain, softmax -> aggregator input
    aggregator / reference-state encoder         DenseStack (the reference input through dib_measure_posenc_rows, 2^0..)
    dib_infonce_fwd_bwd                          symmetric InfoNCE ('l2sq', temperature 1)
    aggregator / reference backward              DenseStack
    dib_measure_bwd                              d soft symbols, softmax and VQ dgrad chain, d(mu | logvar) with the KL term
    VQ weight gradients, IB encoder backward     grouped GEMMs on the stashes
    dib_adam_step                                Keras Adam over ONE flat buffer holding all four networks
There is no CPU fallback: a shape outside dib_measure_supported raises."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ctw, utils
from ._gemm_plan import _ptr
from ._lib import ACTIVATIONS, SIMILARITIES, check
from .dense import DenseStack


class _MeasureDesc(ctypes.Structure):
    """include/dib_measure.h dib_measure_desc"""
    _fields_ = [("w_off", ctypes.c_int64 * 3), ("b_off", ctypes.c_int64 * 3), ("in_dim", ctypes.c_int32), ("E", ctypes.c_int32),
                ("H1", ctypes.c_int32), ("H2", ctypes.c_int32), ("A", ctypes.c_int32), ("L", ctypes.c_int32),
                ("act", ctypes.c_int32), ("pad_", ctypes.c_int32)]


assert ctypes.sizeof(_MeasureDesc) == 80


class _Eng:
    """what DenseStack needs of an engine: the library, the device and the launch stream"""

    def __init__(self, device):
        self.lib = _lib.load_library()
        self.device = torch.device(device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class _Network:
    """One of the four networks: Keras-ordered get_weights / set_weights ([kernel, bias] per layer, NumPy)."""

    def __init__(self, stack: DenseStack, owner, encoder: bool = False):
        self.stack, self._measurement, self._encoder = stack, owner, encoder

    def get_weights(self) -> List[np.ndarray]:
        out = []
        for l in range(len(self.stack.dims)):
            out += [self.stack.kernel(l).detach().cpu().numpy().copy(), self.stack.bias(l).detach().cpu().numpy().copy()]
        return out

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        assert len(weights) == 2 * len(self.stack.dims)
        for l in range(len(self.stack.dims)):
            self.stack.kernel(l).copy_(torch.as_tensor(np.asarray(weights[2 * l], dtype=np.float32)))
            self.stack.bias(l).copy_(torch.as_tensor(np.asarray(weights[2 * l + 1], dtype=np.float32)))

    def __call__(self, x) -> torch.Tensor:
        """forward of a [n, in] array (a copy; the IB encoder gives [n, 2E] = mu | logvar)"""
        return self.stack.forward(torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x,
                                                  device=self.stack.device)).clone()


def beta_schedule(step_num: int, number_training_steps: int, beta_start: float, beta_end: float) -> float:
    """cell 10: exp(log b0 + min(step / n, 1) (log b1 - log b0)), assigned to a float32 variable"""
    return float(np.float32(np.exp(np.log(beta_start) + min(float(step_num) / number_training_steps, 1.)
                                   * (np.log(beta_end) - np.log(beta_start)))))


def sequence_indices(starts, number_states: int) -> np.ndarray:
    """cell 10: batch_inds[b, l] = start_b + l"""
    starts = np.asarray(starts)
    return np.stack([starts + offset for offset in range(number_states)], -1)


def majority_symbols(assignments) -> np.ndarray:
    """cell 10: uint8(mean over draws of argmax > 0.5) of assignments [K, N] - the reference's rule for every alphabet size
    (for A > 2 it is a quirk: symbols >= 1 all vote towards 1)"""
    return np.uint8(np.mean(np.asarray(assignments), axis=0) > 0.5)


class MeasurementIB:
    """The chaos notebook's measurement-optimisation model on the gfx950 kernels (cell 10 hyperparameter names)."""

    def __init__(self, input_dimensionality: int, number_states: int = 12, alphabet_size: int = 2,
                 information_bottleneck_embedding_dimension: int = 8, kl_loss_exponent: float = 2,
                 number_positional_encoding_frequencies: int = 10, info_bott_encoder_arch_spec=(128, 128),
                 vector_quant_arch_spec=(128, 128), measurement_aggregator_arch_spec=(256, 256),
                 reference_state_encoder_arch_spec=(256, 256), reference_timestep: int = 0, infonce_embedding_dimension: int = 32,
                 infonce_similarity: str = "l2sq", infonce_temperature: float = 1., activation_function: str = "leaky_relu",
                 noise_seed: int = 0, init_seed: int = 0, device="cuda:0"):
        # the reference state is states_batch[:, reference_timestep] (NumPy indexing: -1 is the last state); any other value
        # would read a state of the next sequence, or past the trajectory
        L = int(number_states)
        if not -L <= int(reference_timestep) < L:
            raise ValueError(f"reference_timestep {reference_timestep} outside the sequence: -{L} <= reference_timestep < {L}")
        reference_timestep = int(reference_timestep) % L
        if not torch.cuda.is_available():
            raise RuntimeError("MeasurementIB runs on the GPU (libdib_hip); no device is available")
        self.d, self.L, self.A = int(input_dimensionality), int(number_states), int(alphabet_size)
        self.E, self.p = int(information_bottleneck_embedding_dimension), float(kl_loss_exponent)
        self.n_freq = int(number_positional_encoding_frequencies) + 1   # x and its sines
        self.reference_timestep, self.D = reference_timestep, int(infonce_embedding_dimension)
        self.similarity, self.temperature = SIMILARITIES[infonce_similarity], float(infonce_temperature)
        self.noise_seed = int(noise_seed)
        self.eng = _Eng(device)
        self.lib, self.device = self.eng.lib, self.eng.device
        act = activation_function
        vq = list(vector_quant_arch_spec)
        if len(vq) != 2:
            raise ValueError("the VQ network has two hidden layers (the notebook's [128] * 2)")
        self._desc = d = _MeasureDesc()
        d.in_dim, d.E, d.H1, d.H2, d.A, d.L, d.act = self.d, self.E, vq[0], vq[1], self.A, self.L, ACTIVATIONS[act]
        if not self.lib.dib_measure_supported(ctypes.byref(d)):
            raise ValueError(f"measurement model outside the kernels' envelope (dib_measure_supported): d={self.d}, E={self.E}, "
                             f"VQ widths {vq}, A={self.A}, L={self.L}, activation {act}: d <= 4, E <= 32, 2 <= A <= 16, L <= 32, "
                             "VQ widths multiples of 16 up to 128")
        self.ib = DenseStack(self.eng, self.d, info_bott_encoder_arch_spec, 2 * self.E, act, True, self.n_freq, seed=init_seed)
        self.vq = DenseStack(self.eng, self.E, vq, self.A, act, False, seed=init_seed + 1)
        self.agg = DenseStack(self.eng, self.L * self.A, measurement_aggregator_arch_spec, self.D, act, False, seed=init_seed + 2)
        self.ref = DenseStack(self.eng, self.d * self.n_freq, reference_state_encoder_arch_spec, self.D, act, False,
                              seed=init_seed + 3)
        self._stacks = [self.ib, self.vq, self.agg, self.ref]
        # one flat buffer (params | grads | Adam m | Adam v) for all four networks: one optimizer launch per step
        offs, o = [], 0
        for s in self._stacks:
            offs.append(o)
            o += (s.n_params + 63) // 64 * 64
        self.n_params = o
        z = lambda: torch.zeros(o, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.adam_m, self.adam_v = z(), z(), z(), z()
        for s, off in zip(self._stacks, offs):
            self.params[off: off + s.n_params].copy_(s.params)
            s.params = self.params[off: off + s.n_params]
            s.grads = self.grads[off: off + s.n_params]
            s.adam_m = self.adam_m[off: off + s.n_params]
            s.adam_v = self.adam_v[off: off + s.n_params]
        for l in range(3):
            d.w_off[l], d.b_off[l] = self.vq.w_off[l], self.vq.b_off[l]
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.lr_dev = torch.full((1,), 3e-4, dtype=torch.float32, device=self.device)
        self.info_bott_encoder = _Network(self.ib, self, encoder=True)
        self.vector_quantization_network = _Network(self.vq, self)
        self.measurement_aggregator_network = _Network(self.agg, self)
        self.reference_state_encoder = _Network(self.ref, self)
        self.step = 0             # the noise key's step of the next training batch
        self.beta = 10.0          # the notebook's beta_var (initialised to beta_start); fit() assigns it every step
        self._bufs: Dict[int, dict] = {}

    # ---- one step ----------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        bf = self._bufs.get(B)
        if bf is None:
            R, f = B * self.L, lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
            bf = dict(soft=f(R * self.A), out3=f(3), lp=f(1), gx=f(B, self.D), gy=f(B, self.D), ref_in=f(B, self.d * self.n_freq),
                      ws=torch.zeros(int(self.lib.dib_measure_workspace_bytes(ctypes.byref(self._desc), R)) // 4 + 1,
                                     dtype=torch.float32, device=self.device),
                      nce_ws=torch.empty(int(self.lib.dib_infonce_workspace_bytes(B)) // 4 + 1, dtype=torch.float32,
                                         device=self.device),
                      offs=torch.arange(self.L, dtype=torch.int32, device=self.device))
            self._bufs[B] = bf
        return bf

    def _step(self, traj: torch.Tensor, starts: torch.Tensor, beta: float, training: bool) -> dict:
        lib, st = self.lib, self.eng._stream()
        B, L, A, E = int(starts.shape[0]), self.L, self.A, self.E
        R = B * L
        bf = self._buffers(B)
        rows = (starts.view(B, 1) + bf["offs"].view(1, L)).view(-1)
        enc = self.ib.forward(traj, rows=rows)                                  # [R, 2E] = mu | logvar
        vpl = self.vq._plan(R)
        vw = lambda name, cols: self.vq._view(vpl, name, R, cols)
        check(lib.dib_measure_fwd(ctypes.byref(self._desc), _ptr(self.vq.params), _ptr(enc), R, self.noise_seed,
                                  self.step & 0xFFFFFFFF, float(beta), self.p, _ptr(vw("a0", E)), _ptr(vw("a1", self._desc.H1)),
                                  _ptr(vw("a2", self._desc.H2)), _ptr(bf["soft"]), _ptr(bf["out3"]), _ptr(bf["ws"]), st),
              "dib_measure_fwd")
        seq = self.agg.forward(bf["soft"].view(B, L * A))
        ref_rows = starts + self.reference_timestep
        check(lib.dib_measure_posenc_rows(_ptr(traj), traj.stride(0), _ptr(ref_rows), B, self.d, self.n_freq, 0, _ptr(bf["ref_in"]),
                                          st), "dib_measure_posenc_rows")
        remb = self.ref.forward(bf["ref_in"])
        check(lib.dib_infonce_fwd_bwd(_ptr(seq), _ptr(remb), B, self.D, self.similarity, self.temperature,
                                      _ptr(bf["gx"]) if training else None, _ptr(bf["gy"]) if training else None, _ptr(bf["lp"]),
                                      _ptr(bf["nce_ws"]), st), "dib_infonce_fwd_bwd")
        if training:
            # the library's InfoNCE is the sum of both directions; the notebook halves it
            torch.mul(bf["gx"], 0.5, out=self.agg.output_grad_buffer())
            self.agg.backward(self.agg.output_grad_buffer())
            torch.mul(bf["gy"], 0.5, out=self.ref.output_grad_buffer())
            self.ref.backward(self.ref.output_grad_buffer())
            apl = self.agg._last
            g_agg = self.agg._view(apl, "g1", B, self.agg.dims[0][1])
            g_enc = self.ib.output_grad_buffer()
            check(lib.dib_measure_bwd(ctypes.byref(self._desc), _ptr(self.vq.params), _ptr(enc), R, self.noise_seed,
                                      self.step & 0xFFFFFFFF, _ptr(vw("a1", self._desc.H1)), _ptr(vw("a2", self._desc.H2)),
                                      _ptr(bf["soft"]), _ptr(g_agg), _ptr(self.agg.kernel(0)), self.agg.dims[0][1], _ptr(bf["out3"]),
                                      _ptr(vw("g3", A)), _ptr(vw("g2", self._desc.H2)), _ptr(vw("g1", self._desc.H1)), _ptr(g_enc),
                                      st), "dib_measure_bwd")
            # VQ weight gradients: one grouped launch on (z, h1, h2) x (g1, g2, g3)
            if vpl["nsplit"] == 1:
                self.vq.grads.zero_()
            vpl["g"]["wgrad_all"].run(lib, st)
            if vpl["nsplit"] > 1:
                check(lib.dib_reduce_splits(_ptr(vpl["slabs"]), self.vq.n_params, vpl["nsplit"], self.vq.n_params,
                                            _ptr(self.vq.grads), st), "dib_reduce_splits")
            self.ib.backward(g_enc)
            check(lib.dib_adam_step(_ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v), self.n_params,
                                    _ptr(self.lr_dev), _ptr(self.t_dev), 0.9, 0.999, 1e-7, 1.0, st), "dib_adam_step")
            self.step += 1
        return bf

    def match_batch_from_starts(self, traj_dev: torch.Tensor, starts, training: bool = True, beta: Optional[float] = None):
        """One batch of the sequences traj[start_b .. start_b + L) gathered on the device; returns fresh device scalars
        (loss, loss_prediction, kl) without synchronising.  beta: None = the model's `beta` (the notebook's beta_var)."""
        starts = torch.as_tensor(starts).to(device=self.device, dtype=torch.int32)
        bf = self._step(traj_dev, starts, self.beta if beta is None else beta, training)
        kl, lkl, lp = bf["out3"][0].clone(), bf["out3"][1], bf["lp"][0] * 0.5
        return lkl + lp, lp, kl

    def match_batch(self, states_batch, training: bool = True, beta: Optional[float] = None):
        """cell 10 match_batch(states_batch, training) on a host batch [B, L, d] at the model's `beta` (or the one given):
        returns (loss, loss_prediction, kl) as floats."""
        x = np.ascontiguousarray(np.asarray(states_batch, dtype=np.float32))
        B, L, d = x.shape
        assert L == self.L and d == self.d
        traj = torch.from_numpy(x.reshape(B * L, d)).to(self.device)
        starts = torch.arange(0, B * L, L, dtype=torch.int32, device=self.device)
        return tuple(float(v) for v in self.match_batch_from_starts(traj, starts, training, beta))

    # ---- training loop -----------------------------------------------------------------------
    def fit(self, train_trajectory, number_training_steps: int = 20_000, batch_size: int = 2048, learning_rate: float = 3e-4,
            beta_start: float = 10., beta_end: float = 1e-4, info_eval_data=None, evaluate_info_every: Optional[int] = None,
            info_evaluation_batch_size: int = 1024, info_evaluation_number_batches: int = 8, info_stopping_point: float = 1.0,
            seed: int = 0) -> dict:
        """cell 10's loop: per-step log-linear beta annealing, uniformly drawn start indices (seeded NumPy generator), and
        every `evaluate_info_every` steps the sandwich bounds of I(U~; X) in bits (the loop stops once their mean reaches
        `info_stopping_point`).  The trajectory stays on the device; the host synchronises only at information evaluations."""
        traj = torch.as_tensor(np.ascontiguousarray(np.asarray(train_trajectory, dtype=np.float32))).to(self.device)
        if traj.dim() == 1:
            traj = traj[:, None].contiguous()
        n_starts = traj.shape[0] - self.L
        rng = np.random.default_rng(seed)
        self.lr_dev.fill_(float(learning_rate))
        every = evaluate_info_every if evaluate_info_every is not None else max(1, number_training_steps // 100)
        hist = torch.zeros((number_training_steps, 2), dtype=torch.float32, device=self.device)
        out = {"loss": [], "info_in": [], "info_out": [], "beta": []}
        done = 0
        for step_num in range(number_training_steps):
            self.beta = beta = beta_schedule(step_num, number_training_steps, beta_start, beta_end)
            out["beta"].append(beta)
            starts = torch.from_numpy(rng.choice(n_starts, size=batch_size).astype(np.int32)).to(self.device, non_blocking=True)
            loss, lp, _ = self.match_batch_from_starts(traj, starts, True)
            hist[step_num, 0].copy_(loss)
            hist[step_num, 1].copy_(lp)
            done = step_num + 1
            if info_eval_data is not None and (step_num + 1) % every == 0:
                info = np.float32(utils.estimate_mi_sandwich_bounds(self.info_bott_encoder, info_eval_data,
                                                                    info_evaluation_batch_size, info_evaluation_number_batches,
                                                                    seed=step_num)) / np.log(2)
                out["info_in"].append(info)
                lpv = float(hist[step_num, 1])
                out["info_out"].append((np.log2(batch_size) - lpv / np.log(2)) / self.L)
                if np.mean(info) >= info_stopping_point:
                    break
        out["loss"] = hist[:done, 0].cpu().numpy().tolist()
        out["steps"] = done
        return out

    # ---- partition ---------------------------------------------------------------------------
    def symbolize(self, data, number_averaging_logits: int = 100, noise_vector=None, seed: int = 0, chunk_size: int = 1 << 18,
                  return_counts: bool = False):
        """cell 10's symbolisation: a fixed noise table [K, E] (given, or drawn from a seeded NumPy generator) shared by every
        point; sym = uint8(mean_k argmax VQ(mu + noise_k sigma) > 0.5).  One dib_measure_symbolize launch per chunk."""
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(data, dtype=np.float32))).to(self.device)
        if x.dim() == 1:
            x = x[:, None].contiguous()
        if noise_vector is None:
            noise_vector = np.random.default_rng(seed).standard_normal((int(number_averaging_logits), self.E))
        noise = torch.as_tensor(np.asarray(noise_vector, dtype=np.float32).reshape(-1, self.E)).to(self.device).contiguous()
        K, n = int(noise.shape[0]), int(x.shape[0])
        sym = torch.empty(n, dtype=torch.uint8, device=self.device)
        counts = torch.empty((n, self.A), dtype=torch.int32, device=self.device) if return_counts else None
        st = self.eng._stream()
        for c0 in range(0, n, int(chunk_size)):
            c1 = min(n, c0 + int(chunk_size))
            enc = self.ib.forward(x[c0:c1])
            check(self.lib.dib_measure_symbolize(ctypes.byref(self._desc), _ptr(self.vq.params), _ptr(enc), c1 - c0, _ptr(noise), K,
                                                 _ptr(sym[c0:c1]), _ptr(counts[c0:c1]) if counts is not None else None, st),
                  "dib_measure_symbolize")
        s = sym.cpu().numpy()
        return (s, counts.cpu().numpy()) if return_counts else s

    def encode(self, x) -> torch.Tensor:
        """IB encoder output [n, 2E] (mu | logvar) on the device"""
        return self.info_bott_encoder(x)


def entropy_rate_fit(symbolic_sequence, alphabet_size: int, number_data_points=None, number_rand_draws: int = 5, seed: int = 0,
                     threads: int = 0, ctw_backend: str = "host") -> dict:
    """CTW entropy rates of `number_rand_draws` random windows of each length (15 log-spaced lengths 2e3 .. 2e6 by default),
    on `threads` host threads (0 = all), and the Schurmann-Grassberger fit h(N) = h + log2 N / N^g / |c|.

    ctw_backend "device": the same windows (the same rng.choice calls) are estimated by ctw.estimate_entropy_windows on the GPU;
    symbolic_sequence may then be a CUDA uint8 tensor, which is used where it lies.  The result gains "ctw_details"."""
    from scipy import optimize
    if ctw_backend not in ("host", "device"):
        raise ValueError(f"ctw_backend is 'host' or 'device'; got {ctw_backend!r}")
    on_device = ctw_backend == "device" and torch.is_tensor(symbolic_sequence)
    seq = symbolic_sequence.reshape(-1) if on_device else np.asarray(symbolic_sequence)
    if number_data_points is None:
        number_data_points = np.logspace(np.log10(2000), np.log10(2_000_000), 15, dtype=np.int32)
    number_data_points = np.asarray(number_data_points)
    rng = np.random.default_rng(seed)
    windows, starts, lengths = [], [], []
    for n in number_data_points:
        for _ in range(number_rand_draws):
            s = rng.choice(len(seq) - int(n))
            if ctw_backend == "host":
                windows.append(seq[s: s + int(n)])
            starts.append(int(s))
            lengths.append(int(n))
    extra = {}
    if ctw_backend == "host":
        rates = ctw.estimate_entropy_batch(windows, alphabet_size, threads=threads)
    else:
        rates, extra["ctw_details"] = ctw.estimate_entropy_windows(seq, starts, lengths, alphabet_size, backend="device",
                                                                   return_details=True, threads=threads)
    rates = np.asarray(rates, dtype=np.float64).reshape(-1, number_rand_draws)
    mean, err = rates.mean(1), rates.std(1)
    fit_vals, pcov = optimize.curve_fit(utils.entropy_rate_scaling_ansatz, number_data_points, mean, p0=[1, 0.5, 1], sigma=err)
    return {"number_data_points": number_data_points, "entropy_rate_values": rates, "entropy_rate": float(fit_vals[0]),
            "entropy_rate_err": float(np.sqrt(np.diag(pcov))[0]), **extra}


def characterize_partition(symbolic_sequence, alphabet_size: int, number_data_points=None, number_rand_draws: int = 5,
                           seed: int = 0, threads: Optional[int] = None, ctw_backend: str = "host") -> dict:
    """cell 10 after the symbolisation: H(U) of one symbol and entropy_rate_fit of the sequence.  threads: CTW host threads
    (None or 0 = all hardware threads).  ctw_backend: entropy_rate_fit's; a CUDA tensor of symbols stays on the device for the
    windows (H(U) is taken from its histogram)."""
    if ctw_backend == "device" and torch.is_tensor(symbolic_sequence):
        seq = symbolic_sequence.reshape(-1)
        c = torch.bincount(seq.to(torch.int64)).cpu().numpy()
        c = c[c > 0]
        h_u = float(-np.sum(c / c.sum() * np.log2(c / c.sum())))
    else:
        seq = np.asarray(symbolic_sequence)
        h_u = float(utils.compute_entropy(seq))
    fit = entropy_rate_fit(seq, alphabet_size, number_data_points, number_rand_draws, seed, threads=int(threads or 0),
                           ctw_backend=ctw_backend)
    return {"entropy_single_timestep": h_u, **fit}
