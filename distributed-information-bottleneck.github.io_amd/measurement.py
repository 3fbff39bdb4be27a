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
There is no CPU fallback: a shape outside dib_measure_supported raises.

MeasurementEnsemble trains R such models of one architecture in lockstep (the notebook's 20 repeats per number_states): the same
step with the replica as the group of every grouped GEMM and as a grid index of dib_measure_fwd_batched / _bwd_batched and
dib_infonce_fwd_bwd_batched, so that the number of launches of a step does not depend on R.  What the two classes do alike above
the C ABI is written once: the layer-chain plan (dense.chain_plan), the optimizer state (FlatOptimizer), symbolize, and the
preparation of fit; the two fit loops stay apart (other information kernels, and one retires replicas)."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ctw, utils
from ._flat_optimizer import FlatOptimizer, HoldsFlatOptimizer
from ._gemm_plan import _Gemm, _ptr, slab_rule
from ._host import Carver, LibHandle as _Eng
from ._lib import ACTIVATIONS, SIMILARITIES, check
from .dense import DenseStack, chain_plan


class _MeasureDesc(ctypes.Structure):
    """include/dib_measure.h dib_measure_desc"""
    _fields_ = [("w_off", ctypes.c_int64 * 3), ("b_off", ctypes.c_int64 * 3), ("in_dim", ctypes.c_int32), ("E", ctypes.c_int32),
                ("H1", ctypes.c_int32), ("H2", ctypes.c_int32), ("A", ctypes.c_int32), ("L", ctypes.c_int32),
                ("act", ctypes.c_int32), ("pad_", ctypes.c_int32)]


assert ctypes.sizeof(_MeasureDesc) == 80


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


def _fit_setup(model, train_trajectory, learning_rate: float, evaluate_info_every: Optional[int], number_training_steps: int):
    """what both fit loops begin with: the trajectory [n, d] on the device, the number of start indices it holds, the learning
    rate set, and the evaluation period (default: a hundred evaluations per fit)"""
    traj = torch.as_tensor(np.ascontiguousarray(np.asarray(train_trajectory, dtype=np.float32))).to(model.device)
    if traj.dim() == 1:
        traj = traj[:, None].contiguous()
    model.set_lr(learning_rate)
    every = evaluate_info_every if evaluate_info_every is not None else max(1, number_training_steps // 100)
    return traj, traj.shape[0] - model.L, every


def _info_out(batch_size: int, loss_prediction: float, L: int) -> float:
    """cell 10: the InfoNCE bound on the predictive information in bits, per state of the sequence"""
    return (np.log2(batch_size) - loss_prediction / np.log(2)) / L


def _symbolize(model, enc_stack: DenseStack, vq_params: torch.Tensor, vq_off: int, data, number_averaging_logits, noise_vector,
               seed, chunk_size, return_counts):
    """cell 10's symbolisation with the IB encoder `enc_stack` and the packed VQ parameters at vq_params[vq_off:]: a fixed
    noise table [K, E] (given, or drawn from a seeded NumPy generator) shared by every point; sym = uint8(mean_k argmax
    VQ(mu + noise_k sigma) > 0.5).  One dib_measure_symbolize launch per chunk."""
    x = torch.as_tensor(np.ascontiguousarray(np.asarray(data, dtype=np.float32))).to(model.device)
    if x.dim() == 1:
        x = x[:, None].contiguous()
    if noise_vector is None:
        noise_vector = np.random.default_rng(seed).standard_normal((int(number_averaging_logits), model.E))
    noise = torch.as_tensor(np.asarray(noise_vector, dtype=np.float32).reshape(-1, model.E)).to(model.device).contiguous()
    K, n = int(noise.shape[0]), int(x.shape[0])
    sym = torch.empty(n, dtype=torch.uint8, device=model.device)
    counts = torch.empty((n, model.A), dtype=torch.int32, device=model.device) if return_counts else None
    st = model.eng._stream()
    for c0 in range(0, n, int(chunk_size)):
        c1 = min(n, c0 + int(chunk_size))
        enc = enc_stack.forward(x[c0:c1])
        check(model.lib.dib_measure_symbolize(ctypes.byref(model._desc), _ptr(vq_params, vq_off), _ptr(enc), c1 - c0, _ptr(noise), K,
                                              _ptr(sym[c0:c1]), _ptr(counts[c0:c1]) if counts is not None else None, st),
              "dib_measure_symbolize")
    s = sym.cpu().numpy()
    return (s, counts.cpu().numpy()) if return_counts else s


class MeasurementIB(HoldsFlatOptimizer):
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
        self.params, self.grads = (torch.zeros(o, dtype=torch.float32, device=self.device) for _ in range(2))
        self.opt_state = FlatOptimizer(self.lib, self.eng._stream, o, self.device, learning_rate=3e-4)
        for s, off in zip(self._stacks, offs):
            self.params[off: off + s.n_params].copy_(s.params)
            s.params = self.params[off: off + s.n_params]
            s.grads = self.grads[off: off + s.n_params]
            s.adam_m = self.adam_m[off: off + s.n_params]
            s.adam_v = self.adam_v[off: off + s.n_params]
        for l in range(3):
            d.w_off[l], d.b_off[l] = self.vq.w_off[l], self.vq.b_off[l]
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
            self.opt_state.adam(self.params, self.grads, self.n_params, stream=st)
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
        traj, n_starts, every = _fit_setup(self, train_trajectory, learning_rate, evaluate_info_every, number_training_steps)
        rng = np.random.default_rng(seed)
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
                out["info_out"].append(_info_out(batch_size, float(hist[step_num, 1]), self.L))
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
        return _symbolize(self, self.ib, self.vq.params, 0, data, number_averaging_logits, noise_vector, seed, chunk_size,
                          return_counts)

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


# ---- R models in lockstep ---------------------------------------------------------------------------------------------------
class _EnsembleStack:
    """One of the four networks of every replica: a DenseStack's layer chain with the replica as the GROUP of each grouped
    launch (include/dib_st.h dib_gemm_grouped: R descriptors per layer).  Row buffers are [R][n][width] contiguous - what the
    batched measurement and InfoNCE kernels read and write; the weights of replica r sit at r * stride + base in the ensemble's
    flat buffer, laid out as the template DenseStack lays them out."""

    def __init__(self, owner, template: DenseStack, base: int):
        self.o, self.t, self.base = owner, template, int(base)
        self.dims, self.w_off, self.b_off, self.act, self.n_params = template.dims, template.w_off, template.b_off, template.act, \
            template.n_params
        self._plans: Dict[int, dict] = {}

    def plan(self, n: int) -> dict:
        pl = self._plans.get(n)
        if pl is not None:
            return pl
        o, c = self.o, Carver(4)
        ws, g, wgrad_descs = chain_plan(self.dims, self.w_off, self.b_off, self.act, n, o.params, o.device, c, o.R, o.n_params,
                                        self.base)
        nsplit, rps = slab_rule(n)
        if len(self._plans) >= 4:
            self._plans.pop(next(iter(self._plans)))
        pl = self._plans[n] = dict(n=n, ws=ws, off=c.off, g=g, nsplit=nsplit, rps=rps, wgrad={}, wgrad_descs=wgrad_descs)
        return pl

    def wgrad(self, pl: dict, target: torch.Tensor, split_stride: int) -> _Gemm:
        """every replica's and every layer's weight gradient of this network in ONE grouped launch, into `target` (the gradient
        buffer itself, or the ensemble's slabs `split_stride` floats apart)"""
        key = (target.data_ptr(), split_stride)
        gg = pl["wgrad"].get(key)
        if gg is None:
            gg = _Gemm(2, pl["wgrad_descs"], pl["ws"], pl["ws"], target, bias_out=target, nsplit=pl["nsplit"],
                       rows_per_split=pl["rps"], split_stride=split_stride)
            gg.upload(self.o.device)
            pl["wgrad"] = {key: gg}
        return gg

    def view(self, pl, name, width):
        o = pl["off"][name]
        return pl["ws"][o: o + self.o.R * pl["n"] * width].view(self.o.R, pl["n"], width)

    def forward(self, pl, st):
        for l in range(len(self.dims)):
            pl["g"][f"fwd{l}"].run(self.o.lib, st)

    def dgrad(self, pl, st):
        for l in reversed(range(1, len(self.dims))):
            pl["g"][f"dgrad{l}"].run(self.o.lib, st)


class MeasurementEnsemble(HoldsFlatOptimizer):
    """`replicas` MeasurementIB models of ONE architecture trained in lockstep - the notebook's "20 repeats per number_states":
    they differ in their initial weights, their noise seeds and the batches they draw, and share every launch of a step.

    Replica r starts from the weights of MeasurementIB(init_seed=init_seeds[r], noise_seed=noise_seeds[r], ...) (defaults:
    init_seed + 4 r - a model seeds its four networks init_seed .. init_seed + 3 - and noise_seed + r).  One flat buffer
    params | grads | m | v, replica-major, each replica laid out like MeasurementIB's; one dib_adam_step per step with a shared
    learning rate, step count and beta.  Per step: one gather + positional encoding of all R B L rows, every Dense layer as one
    grouped launch of R descriptors, dib_measure_fwd_batched / _bwd_batched, dib_infonce_fwd_bwd_batched (l1 / linf: the single
    entry point per replica) - for the dot-product similarities the number of launches does not depend on R."""

    def __init__(self, replicas: int, init_seeds: Optional[Sequence[int]] = None, noise_seeds: Optional[Sequence[int]] = None,
                 **kwargs):
        R = int(replicas)
        if R < 1:
            raise ValueError("replicas >= 1")
        init_seed, noise_seed = int(kwargs.pop("init_seed", 0)), int(kwargs.pop("noise_seed", 0))
        self.init_seeds = [int(s) for s in init_seeds] if init_seeds is not None else [init_seed + 4 * r for r in range(R)]
        self.noise_seeds = [int(s) for s in noise_seeds] if noise_seeds is not None else [noise_seed + r for r in range(R)]
        if len(self.init_seeds) != R or len(self.noise_seeds) != R:
            raise ValueError(f"init_seeds and noise_seeds take one seed per replica ({R})")
        self.R, self._kwargs = R, dict(kwargs)
        # replica 0 as a MeasurementIB: validates the arguments (before any launch), fixes the layout, and is the template
        m0 = self._template = MeasurementIB(init_seed=self.init_seeds[0], noise_seed=self.noise_seeds[0], **kwargs)
        for k in ("d", "L", "A", "E", "p", "n_freq", "reference_timestep", "D", "similarity", "temperature", "eng", "lib", "device",
                  "_desc", "n_params"):
            setattr(self, k, getattr(m0, k))
        P = self.n_params
        flat = torch.zeros(4 * R * P, dtype=torch.float32, device=self.device)
        self.params, self.grads, m, v = (flat[i * R * P: (i + 1) * R * P] for i in range(4))
        self.opt_state = FlatOptimizer(self.lib, self.eng._stream, R * P, self.device, learning_rate=3e-4, m=m, v=v)
        self._flat = flat
        bases = [int((s.params.data_ptr() - m0.params.data_ptr()) // 4) for s in m0._stacks]
        self.params[:P].copy_(m0.params)
        act = kwargs.get("activation_function", "leaky_relu")
        for r in range(1, R):   # the other replicas' initial weights: the DenseStack initialiser with their seeds
            for k, (s, b) in enumerate(zip(m0._stacks, bases)):
                init = DenseStack(self.eng, s.input_dim, [o for _, o in s.dims[:-1]], s.dims[-1][1], act, s.n_freq > 1, s.n_freq,
                                  seed=self.init_seeds[r] + k)
                assert init.n_params == s.n_params
                self.params[r * P + b: r * P + b + s.n_params].copy_(init.params)
        self.ib, self.vq, self.agg, self.ref = (_EnsembleStack(self, s, b) for s, b in zip(m0._stacks, bases))
        self._nets = {"ib": self.ib, "vq": self.vq, "agg": self.agg, "ref": self.ref}
        self._seeds_c = (ctypes.c_uint64 * R)(*[s & (2 ** 64 - 1) for s in self.noise_seeds])
        self.step, self.beta = 0, 10.0
        self.snapshots: Dict[int, torch.Tensor] = {}    # parameters of retired replicas (fit)
        self._bufs: Dict[int, dict] = {}

    # ---- one step ----------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        bf = self._bufs.get(B)
        if bf is None:
            R, lib, f = self.R, self.lib, lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
            pls = dict(ib=self.ib.plan(B * self.L), vq=self.vq.plan(B * self.L), agg=self.agg.plan(B), ref=self.ref.plan(B))
            nmax = max(pl["nsplit"] for pl in pls.values())
            bf = dict(pl=pls, out3=f(R, 3), lp=f(R), gx=f(R, B, self.D), gy=f(R, B, self.D), nsplit=nmax,
                      slabs=f(nmax * R * self.n_params) if nmax > 1 else None,
                      ws=torch.zeros(int(lib.dib_measure_batched_workspace_bytes(ctypes.byref(self._desc), B * self.L, R)) // 4 + 1,
                                     dtype=torch.float32, device=self.device),
                      # (l1 / linf: the single entry point's workspace, used by one replica after the other)
                      nce_ws=torch.empty(int(lib.dib_infonce_batched_workspace_bytes(R, B) if self.similarity in (0, 1, 4)
                                             else lib.dib_infonce_workspace_bytes(B)) // 4 + 1, dtype=torch.float32,
                                         device=self.device),
                      offs=torch.arange(self.L, dtype=torch.int32, device=self.device))
            # networks whose own rule gives one slab accumulate into slab 0 next to the others': it is cleared every step
            bf["clear_slab0"] = nmax > 1 and any(pl["nsplit"] == 1 for pl in pls.values())
            if len(self._bufs) >= 2:
                self._bufs.pop(next(iter(self._bufs)))
            self._bufs[B] = bf
        return bf

    def _step(self, traj: torch.Tensor, starts: torch.Tensor, beta: float, training: bool) -> dict:
        lib, st, R, P = self.lib, self.eng._stream(), self.R, self.n_params
        B, L, A, E, d = int(starts.shape[1]), self.L, self.A, self.E, self._desc
        n = B * L
        bf = self._buffers(B)
        ib, vq, agg, ref = (bf["pl"][k] for k in ("ib", "vq", "agg", "ref"))
        rows = (starts.view(R, B, 1) + bf["offs"].view(1, 1, L)).reshape(-1)
        check(lib.dib_positional_encoding_rows(_ptr(traj), traj.stride(0), _ptr(rows), R * n, self.d, self.n_freq,
                                               _ptr(ib["ws"], ib["off"]["a0"]), st), "dib_positional_encoding_rows")
        self.ib.forward(ib, st)
        enc = self.ib.view(ib, f"a{len(self.ib.dims)}", 2 * E)                   # [R, n, 2E] = mu | logvar
        vw = lambda name: _ptr(vq["ws"], vq["off"][name])
        soft = _ptr(agg["ws"], agg["off"]["a0"])                                 # [R][n][A] = the aggregator's input [R][B][L A]
        vqp = _ptr(self.params, self.vq.base)
        check(lib.dib_measure_fwd_batched(ctypes.byref(d), vqp, P, _ptr(enc), n, R, self._seeds_c, self.step & 0xFFFFFFFF, float(beta),
                                          self.p, vw("a0"), vw("a1"), vw("a2"), soft, _ptr(bf["out3"]), _ptr(bf["ws"]), st),
              "dib_measure_fwd_batched")
        self.agg.forward(agg, st)
        ref_rows = (starts + self.reference_timestep).reshape(-1)
        check(lib.dib_measure_posenc_rows(_ptr(traj), traj.stride(0), _ptr(ref_rows), R * B, self.d, self.n_freq, 0,
                                          _ptr(ref["ws"], ref["off"]["a0"]), st), "dib_measure_posenc_rows")
        self.ref.forward(ref, st)
        seq = self.agg.view(agg, f"a{len(self.agg.dims)}", self.D)
        remb = self.ref.view(ref, f"a{len(self.ref.dims)}", self.D)
        gx, gy = (bf["gx"], bf["gy"]) if training else (None, None)
        if self.similarity in (0, 1, 4):
            check(lib.dib_infonce_fwd_bwd_batched(_ptr(seq), _ptr(remb), R, B, self.D, self.similarity, self.temperature, _ptr(gx),
                                                  _ptr(gy), _ptr(bf["lp"]), _ptr(bf["nce_ws"]), st), "dib_infonce_fwd_bwd_batched")
        else:   # l1 / linf: no batched kernel - the single entry point, replica by replica
            for r in range(R):
                check(lib.dib_infonce_fwd_bwd(_ptr(seq[r]), _ptr(remb[r]), B, self.D, self.similarity, self.temperature,
                                              _ptr(gx[r]) if training else None, _ptr(gy[r]) if training else None,
                                              _ptr(bf["lp"][r:]), _ptr(bf["nce_ws"]), st), "dib_infonce_fwd_bwd")
        if training:
            slabs, stride = bf["slabs"], R * P
            target = slabs if slabs is not None else self.grads
            if slabs is None:
                self.grads.zero_()
            elif bf["clear_slab0"]:
                slabs[:stride].zero_()
            # the library's InfoNCE is the sum of both directions; the notebook halves it
            torch.mul(gx, 0.5, out=self.agg.view(agg, f"g{len(self.agg.dims)}", self.D))
            self.agg.dgrad(agg, st)
            self.agg.wgrad(agg, target, stride).run(lib, st)
            torch.mul(gy, 0.5, out=self.ref.view(ref, f"g{len(self.ref.dims)}", self.D))
            self.ref.dgrad(ref, st)
            self.ref.wgrad(ref, target, stride).run(lib, st)
            HA = self.agg.dims[0][1]
            check(lib.dib_measure_bwd_batched(ctypes.byref(d), vqp, P, _ptr(enc), n, R, self._seeds_c, self.step & 0xFFFFFFFF,
                                              vw("a1"), vw("a2"), soft, _ptr(agg["ws"], agg["off"]["g1"]),
                                              _ptr(self.params, self.agg.base + self.agg.w_off[0]), P, HA, _ptr(bf["out3"]),
                                              vw("g3"), vw("g2"), vw("g1"), _ptr(ib["ws"], ib["off"][f"g{len(self.ib.dims)}"]), st),
                  "dib_measure_bwd_batched")
            self.vq.wgrad(vq, target, stride).run(lib, st)
            self.ib.dgrad(ib, st)
            self.ib.wgrad(ib, target, stride).run(lib, st)
            if slabs is not None:
                check(lib.dib_reduce_splits(_ptr(slabs), stride, bf["nsplit"], stride, _ptr(self.grads), st), "dib_reduce_splits")
            self.opt_state.adam(self.params, self.grads, stride, stream=st)
            self.step += 1
        return bf

    def match_batch_from_starts(self, traj_dev: torch.Tensor, starts, training: bool = True, beta: Optional[float] = None):
        """One step of every replica on its own sequences traj[starts[r, b] .. + L): starts [R, B].  Returns fresh device
        vectors [R] (loss, loss_prediction, kl) without synchronising."""
        starts = torch.as_tensor(starts).to(device=self.device, dtype=torch.int32)
        if starts.dim() != 2 or starts.shape[0] != self.R:
            raise ValueError(f"starts must be [replicas = {self.R}, batch]")
        bf = self._step(traj_dev, starts.contiguous(), self.beta if beta is None else beta, training)
        kl, lkl, lp = bf["out3"][:, 0].clone(), bf["out3"][:, 1], bf["lp"] * 0.5
        return lkl + lp, lp, kl

    def match_batch(self, states_batch, training: bool = True, beta: Optional[float] = None):
        """host batches [R, B, L, d], one per replica: (loss, loss_prediction, kl) as NumPy vectors [R]"""
        x = np.ascontiguousarray(np.asarray(states_batch, dtype=np.float32))
        R, B, L, d = x.shape
        assert R == self.R and L == self.L and d == self.d
        traj = torch.from_numpy(x.reshape(R * B * L, d)).to(self.device)
        starts = torch.arange(0, R * B * L, L, dtype=torch.int32, device=self.device).view(R, B)
        return tuple(v.cpu().numpy() for v in self.match_batch_from_starts(traj, starts, training, beta))

    # ---- training loop -----------------------------------------------------------------------
    def _info_bounds(self, x: np.ndarray, bs: int, nb: int, seed: int) -> np.ndarray:
        """[R, 2] sandwich bounds of I(U~; X) in nats at the current weights: the batches utils.estimate_mi_sandwich_bounds draws
        for `seed` (the same rows for every replica), ONE grouped forward of every replica's IB encoder on them, and one
        dib_mi_sandwich_batched over the R nb batches (batch b of replica r keyed (seed, r nb + b, position, 0)); where that
        kernel does not take the shape (E not a multiple of 4), dib_mi_sandwich_rows batch by batch."""
        lib, st, R, E = self.lib, self.eng._stream(), self.R, self.E
        rng, n = np.random.default_rng(seed), x.shape[0]
        rows = np.concatenate([rng.permutation(n)[:bs] if n >= bs else rng.integers(0, n, bs) for _ in range(nb)])
        xb = torch.from_numpy(x[rows]).to(self.device)
        m = nb * bs
        pl = self.ib.plan(m)
        idx = torch.arange(m, dtype=torch.int32, device=self.device).repeat(R)
        check(lib.dib_positional_encoding_rows(_ptr(xb), xb.stride(0), _ptr(idx), R * m, self.d, self.n_freq,
                                               _ptr(pl["ws"], pl["off"]["a0"]), st), "dib_positional_encoding_rows")
        self.ib.forward(pl, st)
        enc = self.ib.view(pl, f"a{len(self.ib.dims)}", 2 * E)
        need = int(lib.dib_mi_sandwich_batched_workspace_bytes(R * m, 1, E, R * nb, bs))
        if need < 0:
            out = [[utils.mi_sandwich_rows(lib, self.device, enc[r, b * bs: (b + 1) * bs], seed, b, 0).mean(dim=1).cpu().numpy()
                    for b in range(nb)] for r in range(R)]
            return np.mean(np.asarray(out), 1)
        ws = torch.empty(need // 8 + 2, dtype=torch.float64, device=self.device)
        out = torch.empty((2, R * nb), dtype=torch.float64, device=self.device)
        bidx = torch.arange(R * m, dtype=torch.int32, device=self.device)
        check(lib.dib_mi_sandwich_batched(_ptr(enc), R * m, 1, E, _ptr(bidx), R * nb, bs, 0.0, int(seed) & (2 ** 64 - 1), 0,
                                          _ptr(out[0]), _ptr(out[1]), None, None, None, _ptr(ws), st), "dib_mi_sandwich_batched")
        return out.view(2, R, nb).mean(dim=2).cpu().numpy().T.copy()

    def fit(self, train_trajectory, number_training_steps: int = 20_000, batch_size: int = 2048, learning_rate: float = 3e-4,
            beta_start: float = 10., beta_end: float = 1e-4, info_eval_data=None, evaluate_info_every: Optional[int] = None,
            info_evaluation_batch_size: int = 1024, info_evaluation_number_batches: int = 8, info_stopping_point=1.0,
            seeds: Optional[Sequence[int]] = None) -> List[dict]:
        """MeasurementIB.fit for every replica at once.  Replica r draws its start indices from np.random.default_rng(seeds[r])
        (default r) - the stream a single fit(seed=seeds[r]) draws; one [R, B] upload per step.  Every `evaluate_info_every`
        steps the sandwich bounds of every replica are evaluated; a replica whose mean bound reaches its `info_stopping_point`
        (a scalar, or one per replica) is RETIRED: its parameters are copied to `snapshots[r]` and its history ends there,
        while the lockstep step goes on computing it so that nothing the others see changes.  Ends when every replica is
        retired or the steps run out.  Returns one history per replica with the keys of MeasurementIB.fit."""
        R = self.R
        seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
        thr = np.broadcast_to(np.asarray(info_stopping_point, dtype=np.float64), (R,)) if np.ndim(info_stopping_point) == 0 \
            else np.asarray(info_stopping_point, dtype=np.float64)
        if len(seeds) != R or thr.shape != (R,):
            raise ValueError(f"seeds and info_stopping_point take one entry per replica ({R})")
        traj, n_starts, every = _fit_setup(self, train_trajectory, learning_rate, evaluate_info_every, number_training_steps)
        rngs = [np.random.default_rng(s) for s in seeds]
        ev = None
        if info_eval_data is not None:
            ev = np.asarray(info_eval_data, dtype=np.float32)
            ev = ev[:, None] if ev.ndim == 1 else ev
        hist = torch.zeros((number_training_steps, 2, R), dtype=torch.float32, device=self.device)
        out = [{"loss": [], "info_in": [], "info_out": [], "beta": []} for _ in range(R)]
        done = [None] * R                                    # steps taken when the replica retired
        betas, taken = [], 0
        self.snapshots = {}
        for step_num in range(number_training_steps):
            self.beta = beta = beta_schedule(step_num, number_training_steps, beta_start, beta_end)
            betas.append(beta)
            starts = np.stack([g.choice(n_starts, size=batch_size) for g in rngs]).astype(np.int32)
            loss, lp, _ = self.match_batch_from_starts(traj, torch.from_numpy(starts).to(self.device, non_blocking=True), True)
            hist[step_num, 0].copy_(loss)
            hist[step_num, 1].copy_(lp)
            taken = step_num + 1
            if ev is not None and taken % every == 0:
                info = np.float32(self._info_bounds(ev, int(info_evaluation_batch_size), int(info_evaluation_number_batches),
                                                    step_num)) / np.log(2)
                lpv = hist[step_num, 1].cpu().numpy()
                for r in range(R):
                    if done[r] is not None:
                        continue
                    out[r]["info_in"].append(info[r])
                    out[r]["info_out"].append(_info_out(batch_size, float(lpv[r]), self.L))
                    if np.mean(info[r]) >= thr[r]:
                        done[r] = taken
                        self.snapshots[r] = self.params[r * self.n_params: (r + 1) * self.n_params].clone()
                if all(s is not None for s in done):
                    break
        losses = hist[:taken, 0].cpu().numpy()
        for r in range(R):
            k = taken if done[r] is None else done[r]
            out[r]["loss"] = losses[:k, r].tolist()
            out[r]["beta"] = betas[:k]
            out[r]["steps"] = k
        return out

    # ---- access to replicas ------------------------------------------------------------------
    def _replica_params(self, r: int) -> torch.Tensor:
        """replica r's parameters [n_params]: its snapshot if fit retired it, else its slice of the live buffer"""
        if not 0 <= int(r) < self.R:
            raise IndexError(f"replica {r} of {self.R}")
        snap = self.snapshots.get(int(r))
        return snap if snap is not None else self.params[r * self.n_params: (r + 1) * self.n_params]

    def get_weights(self, r: int) -> Dict[str, List[np.ndarray]]:
        """{"ib", "vq", "agg", "ref"} -> Keras-ordered [kernel, bias] per layer (of the snapshot if replica r is retired)"""
        p = self._replica_params(r).cpu().numpy()
        return {k: sum(([p[s.base + w: s.base + w + i * o].reshape(i, o).copy(), p[s.base + b: s.base + b + o].copy()]
                        for (i, o), w, b in zip(s.dims, s.w_off, s.b_off)), []) for k, s in self._nets.items()}

    def set_weights(self, r: int, weights: Dict[str, Sequence[np.ndarray]]) -> None:
        """the live parameters of replica r (a snapshot fit left for it is dropped)"""
        self._replica_params(r)
        live = self.params[r * self.n_params: (r + 1) * self.n_params]
        for k, ws in weights.items():
            s = self._nets[k]
            assert len(ws) == 2 * len(s.dims)
            for l, ((i, o), w, b) in enumerate(zip(s.dims, s.w_off, s.b_off)):
                live[s.base + w: s.base + w + i * o].copy_(torch.as_tensor(np.asarray(ws[2 * l], dtype=np.float32).reshape(-1)))
                live[s.base + b: s.base + b + o].copy_(torch.as_tensor(np.asarray(ws[2 * l + 1], dtype=np.float32).reshape(-1)))
        self.snapshots.pop(int(r), None)

    def to_model(self, r: int) -> MeasurementIB:
        """a MeasurementIB carrying replica r's weights (the snapshot if retired), noise seed and step: symbolize,
        characterize_partition and the CTW back ends apply to it unchanged.  A live replica also hands over its optimizer state
        (Adam moments, step count, learning rate); a retired one does not - the moments went on moving after its snapshot -
        and its model starts from a fresh one"""
        p = self._replica_params(r)
        m = MeasurementIB(init_seed=self.init_seeds[r], noise_seed=self.noise_seeds[r], **self._kwargs)
        m.params.copy_(p)
        if int(r) not in self.snapshots:
            m.opt_state.take_state(self.opt_state, slice(r * self.n_params, (r + 1) * self.n_params))
        m.step, m.beta = self.step, self.beta
        return m

    def symbolize(self, r: int, data, number_averaging_logits: int = 100, noise_vector=None, seed: int = 0,
                  chunk_size: int = 1 << 18, return_counts: bool = False):
        """MeasurementIB.symbolize for replica r: its IB encoder on a DenseStack, dib_measure_symbolize on ITS packed VQ
        parameters where they lie in the ensemble's buffer (in its snapshot if retired)"""
        p = self._replica_params(r)
        enc_stack = self._template.ib                         # the template's encoder stack, loaded with replica r's weights
        enc_stack.params.copy_(p[self.ib.base: self.ib.base + self.ib.n_params])
        return _symbolize(self, enc_stack, p, self.vq.base, data, number_averaging_logits, noise_vector, seed, chunk_size,
                          return_counts)
