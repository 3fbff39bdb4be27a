"""The Boolean-circuit notebook's distributed IB (reference complex_systems/InfoDecomp_Boolean_circuits.ipynb cells 4-7; the
paper's Fig. 1 and Fig. S1): one SimpleEncoder per input gate with two trainable scalars, x in {-1, +1} -> N(x s_g, e^{lv_g}),
and a predictor Dense(256, leaky_relu) x3 -> Dense(1) over the G sampled embeddings, trained with BCE from logits plus
beta * sum_g KL_g on batches drawn uniformly, with replacement, from the 2^G-row truth table.

Device path of one training step (include/dib_circuit.h, csrc/dib_circuit.h; the rest are existing library kernels):
    dib_circuit_fwd              row draw, gather, 0/1 -> -+1, reparameterisation, u [B, 16] (zero pad), y, KL [G] and beta sum KL
    dib_mlp_small_head_step      predictor forward, mean BCE, dL/dlogit, dgrad chain, output layer's gradient, g_u = dL/du
    dib_gemm_grouped             the hidden layers' weight gradients on the stashes (batch-split into gradient slabs)
    dib_circuit_bwd              d(s_g, lv_g) incl. the KL term, straight into the (first slab of the) flat gradient buffer
    dib_reduce_adam_step         slab sum, Keras Adam over ONE flat buffer (the predictor and the 2G scalars), step count
The sandwich bounds of all G channels over all evaluation batches are one dib_circuit_mi_bounds launch.  There is no CPU
fallback: shapes outside the kernels' envelope raise ValueError before anything is launched."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._gemm_plan import _Gemm, _d, _ptr
from ._lib import ACTIVATIONS, check
from .dense import _MlpDesc

MAX_GATES, MAX_BATCH, U_LD = 16, 2048, 16   # include/dib_circuit.h envelope and u's row pitch

# cell 5: [gate_id, input1, input2] per intermediate output (gates: and, or, xor); the last one is y
PAPER_CIRCUIT = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, [1, 0, 1], [2, 8, 7], [0, 4, 3], [1, 11, 5], [2, 6, 12], [2, 13, 9], [1, 14, 10],
                 [0, 15, 2], [0, 17, 16]]
# cell 10: the six circuits of Fig. S1 (a-f)
SI_CIRCUITS = [
    [0, 1, 2, [2, 1, 2], [2, 0, 3]],
    [0, 1, 2, [0, 1, 0], [2, 2, 3]],
    [0, 1, 2, 3, [0, 2, 0], [2, 4, 3], [0, 5, 1]],
    [0, 1, 2, 3, [1, 1, 3], [0, 4, 0], [2, 2, 5]],
    [0, 1, 2, 3, 4, [0, 1, 4], [2, 3, 5], [0, 6, 2], [1, 0, 7]],
    [0, 1, 2, 3, 4, 5, [2, 5, 4], [2, 0, 3], [0, 1, 2], [2, 8, 6], [2, 9, 7]],
]
_GATES = [np.logical_and, np.logical_or, np.logical_xor]


def number_input_gates(circuit_specification) -> int:
    """cell 10: the integer entries of a specification are its inputs"""
    return int(sum(1 for v in circuit_specification if isinstance(v, (int, np.integer))))


def truth_table(circuit_specification) -> np.ndarray:
    """cell 5 (apply_gates): [2^G, G + 1] int32 rows of the inputs (meshgrid 'xy' order) and y"""
    G = number_input_gates(circuit_specification)
    inputs = np.reshape(np.stack(np.meshgrid(*[[0, 1]] * G), -1), [-1, G])
    inter = inputs
    for gate, a, b in circuit_specification[G:]:
        inter = np.concatenate([inter, np.int32(_GATES[gate](inter[:, a], inter[:, b]))[:, None]], -1)
    return np.concatenate([inter[:, :G], inter[:, -1:]], -1).astype(np.int32)


def entropy_bits(vals) -> float:
    """cell 5 compute_entropy: entropy (bits) of a 0/1 column, or of the rows of several columns, of a truth table"""
    vals = np.asarray(vals)
    if vals.ndim == 2:
        vals = np.int32([int("".join(str(int(v)) for v in row), 2) for row in vals])
    p = np.bincount(vals) / float(vals.shape[0])
    p = p[p > 0]
    return float(-np.sum(p * np.log2(p)))


def beta_schedule(step: int, number_training_steps: int, beta_start: float, beta_end: float) -> float:
    """cell 6: beta_var.assign(exp(log b0 + step / n (log b1 - log b0))) - a float32 variable"""
    return float(np.float32(np.exp(np.log(beta_start) + float(step) / number_training_steps
                                   * (np.log(beta_end) - np.log(beta_start)))))


def evaluation_seed(seed: int, step: int) -> int:
    """the seed of fit(seed=...)'s information evaluation at `step`: the NumPy draw of the evaluation inputs and the Philox key
    of their noise (estimate_channel_mi_bounds / utils.estimate_mi_sandwich_bounds with this seed give the same bounds)"""
    return (int(seed) << 32) + int(step)


def information_plane(history: dict, entropy_y: float) -> Dict[str, np.ndarray]:
    """cell 6's post-processing of a fit() history: info_in_parts [n_eval, G] (bits per channel, Gaussian sigma 1.5 over
    evaluations), info_in_full [n_eval] (their sum, sigma 0.5) and predictive_information_out [n_eval] (H(Y) - BCE in bits,
    sigma 25 over steps, sampled at the evaluation steps)"""
    from scipy import ndimage
    freq = int(history["evaluate_mutual_info_freq"])
    transmitted = np.mean(np.asarray(history["mutual_information_bounds"]), axis=-1)
    out = entropy_y - np.float32(history["bce_loss_series"]) / np.log(2)
    return {"info_in_parts": ndimage.gaussian_filter1d(transmitted, 1.5, axis=0),
            "info_in_full": ndimage.gaussian_filter1d(np.sum(transmitted, axis=-1), 0.5),
            "predictive_information_out": ndimage.gaussian_filter(out, 25)[::freq]}


def selected_subsets(info_in_parts, threshold: float = 0.1) -> list:
    """cell 7: the gates above `threshold` bits, cumulatively (a gate once below stays out), at every evaluation where the set
    shrinks - then the notebook's trailing range(G) (the full set)"""
    info_in_parts = np.asarray(info_in_parts)
    above = np.cumprod(info_in_parts > threshold, axis=0)
    sum_active = np.sum(above, axis=-1)
    change = np.where((sum_active[1:] - sum_active[:-1]) < 0)[0]
    subsets = [np.where(above[i + 1])[0] for i in change]
    subsets.append(range(info_in_parts.shape[-1]))
    return subsets


def subset_comparison(info_in_parts, table, threshold: float = 0.1, backend: str = "device") -> list:
    """cell 7's check of the subsets the DIB selected against the exhaustive ground truth: for every subset of
    selected_subsets(info_in_parts, threshold), in that order, a dict with its gates, mask, size, information_bits = I(X_S;Y) on
    the truth table ([rows, G + 1] 0/1, y last), rank among the subsets of its size (0 = the most informative: the colour
    index) and best_bits_of_size.  One exhaustive evaluation (subset_information.subset_information) serves all of them."""
    from . import subset_information as si
    t = np.asarray(table)
    info = si.subset_information(t[:, :-1], t[:, -1], backend=backend)
    rows = []
    for s in selected_subsets(info_in_parts, threshold):
        gates = [int(g) for g in s]
        mask = sum(1 << g for g in gates)
        rows.append({"gates": gates, "mask": mask, "size": len(gates), "information_bits": float(info.bits[mask]),
                     "rank": info.rank(mask), "best_bits_of_size": float(info.by_size(len(gates))[1][0])})
    return rows


def pack_truth_table(table) -> np.ndarray:
    """[2^G, G + 1] 0/1 rows -> uint32 words (bit g = input g, bit G = y); ValueError for any other table"""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] < 2:
        raise ValueError(f"a truth table is [2^G, G + 1]; got shape {t.shape}")
    G = t.shape[1] - 1
    if not 1 <= G <= MAX_GATES:
        raise ValueError(f"{G} input gates outside the kernels' envelope 1 <= G <= {MAX_GATES}")
    if t.shape[0] != 1 << G:
        raise ValueError(f"a truth table of {G} inputs has {1 << G} rows; got {t.shape[0]}")
    if not np.isin(t, (0, 1)).all():
        raise ValueError("truth table entries are 0 or 1")
    return (t.astype(np.uint32) << np.arange(G + 1, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)


class _Eng:
    def __init__(self, device):
        self.lib = _lib.load_library()
        self.device = torch.device(device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class _FeatureEncoder:
    """cell 4 SimpleEncoder of gate `index`: get_weights / set_weights = [mu_scaling (1, 1), logvar (1, 1)]; called on x [n, 1]
    it returns [n, 2] = concat(x * mu_scaling, logvar) (a device tensor)"""

    def __init__(self, model: "CircuitIB", index: int):
        self._circuit, self.index = model, int(index)

    def _views(self):
        m = self._circuit
        return m.scalars[self.index: self.index + 1], m.scalars[m.G + self.index: m.G + self.index + 1]

    def get_weights(self) -> List[np.ndarray]:
        s, lv = self._views()
        return [s.detach().cpu().numpy().reshape(1, 1).copy(), lv.detach().cpu().numpy().reshape(1, 1).copy()]

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        s, lv = self._views()
        s.copy_(torch.as_tensor(np.asarray(weights[0], dtype=np.float32).reshape(1)))
        lv.copy_(torch.as_tensor(np.asarray(weights[1], dtype=np.float32).reshape(1)))

    def __call__(self, x) -> torch.Tensor:
        s, lv = self._views()
        x = torch.as_tensor(np.asarray(x, dtype=np.float32) if not torch.is_tensor(x) else x).to(self._circuit.device,
                                                                                                  torch.float32)
        x = x.reshape(-1, 1)
        return torch.cat([x * s, torch.ones_like(x) * lv], -1)


class _Predictor:
    """cell 6 predictive_model: Keras-ordered get_weights / set_weights ([kernel, bias] per layer; the first kernel is [G, 256] -
    its 16 - G zero pad rows of the device layout are not part of it)"""

    def __init__(self, model: "CircuitIB"):
        self._m = model

    def get_weights(self) -> List[np.ndarray]:
        m, out = self._m, []
        for l in range(len(m.dims)):
            k = m.kernel(l).detach().cpu().numpy()
            out += [(k[:m.G] if l == 0 else k).copy(), m.bias(l).detach().cpu().numpy().copy()]
        return out

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        m = self._m
        assert len(weights) == 2 * len(m.dims)
        for l in range(len(m.dims)):
            k = np.asarray(weights[2 * l], dtype=np.float32)
            if l == 0:
                k = np.concatenate([k, np.zeros((U_LD - m.G, k.shape[1]), np.float32)], 0)
            m.kernel(l).copy_(torch.as_tensor(k))
            m.bias(l).copy_(torch.as_tensor(np.asarray(weights[2 * l + 1], dtype=np.float32)))


class CircuitIB:
    """The Boolean-circuit notebook's model on the gfx950 kernels (cell 6 names)."""

    def __init__(self, number_input_gates: int, predictive_arch_spec=(256, 256, 256), activation_function: str = "leaky_relu",
                 noise_seed: int = 0, init_seed: int = 0, device="cuda:0"):
        G = int(number_input_gates)
        if not 1 <= G <= MAX_GATES:
            raise ValueError(f"number_input_gates {G} outside the kernels' envelope 1 <= G <= {MAX_GATES}")
        if not torch.cuda.is_available():
            raise RuntimeError("CircuitIB runs on the GPU (libdib_hip); no device is available")
        self.G, self.noise_seed = G, int(noise_seed)
        self.eng = _Eng(device)
        self.lib, self.device = self.eng.lib, self.eng.device
        units = [int(u) for u in predictive_arch_spec]
        if activation_function not in ACTIVATIONS:
            raise ValueError(f"unknown activation {activation_function!r}")
        # flat buffer: the predictor (DenseStack layout, input padded to 16 columns), then s[0..G), lv[0..G)
        dims = [U_LD] + units + [1]
        self.dims = list(zip(dims[:-1], dims[1:]))
        off, self.w_off, self.b_off = 0, [], []
        for i, o in self.dims:
            self.w_off.append(off); off += (i * o + 3) // 4 * 4
            self.b_off.append(off); off += (o + 3) // 4 * 4
        self.sc_off = (off + 63) // 64 * 64
        self.n_params = (self.sc_off + 2 * G + 63) // 64 * 64
        self._desc = d = _MlpDesc()
        nh = len(units)
        for l in range(len(self.dims)):
            d.w_off[l], d.b_off[l], d.width[l] = self.w_off[l], self.b_off[l], self.dims[l][1]
        d.n_hidden, d.in_dim, d.n_freq, d.act = nh, U_LD, 1, ACTIVATIONS[activation_function]
        if not 1 <= nh <= 3 or not self.lib.dib_mlp_small_head_supported(ctypes.byref(d), 1):
            raise ValueError(f"predictor {units} / {activation_function} outside the row-tile head kernel's envelope "
                             "(dib_mlp_small_head_supported): 1-3 hidden layers of widths multiple of 16 up to 1024, a "
                             "piecewise-linear activation")
        # Keras glorot-uniform kernels with the TRUE fan-in G of the first layer (its pad rows stay 0 under Adam: zero gradient)
        rng = np.random.default_rng(init_seed)
        flat = np.zeros(self.n_params, dtype=np.float32)
        for l, ((i, o), w) in enumerate(zip(self.dims, self.w_off)):
            fan_in = G if l == 0 else i
            lim = math.sqrt(6.0 / (fan_in + o))
            k = np.zeros((i, o), np.float32)
            k[:fan_in] = rng.uniform(-lim, lim, (fan_in, o)).astype(np.float32)
            flat[w: w + i * o] = k.reshape(-1)
        flat[self.sc_off: self.sc_off + G] = 1.0          # mu_scaling
        flat[self.sc_off + G: self.sc_off + 2 * G] = -3.0  # logvar
        self.params = torch.from_numpy(flat).to(self.device)
        z = lambda: torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.grads, self.adam_m, self.adam_v = z(), z(), z()
        self.scalars = self.params[self.sc_off: self.sc_off + 2 * G]
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.lr_dev = torch.full((1,), 1e-3, dtype=torch.float32, device=self.device)
        self._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32, device=self.device)
        self.feature_encoders = [_FeatureEncoder(self, g) for g in range(G)]
        self.predictive_model = _Predictor(self)
        self.step = 0                 # the noise key's step of the next training batch
        self._bufs: Dict[int, dict] = {}
        self._mi_ws: Dict[tuple, torch.Tensor] = {}
        self._table_key, self._table_dev = None, None

    # views
    def kernel(self, l):
        i, o = self.dims[l]
        return self.params[self.w_off[l]: self.w_off[l] + i * o].view(i, o)

    def bias(self, l):
        return self.params[self.b_off[l]: self.b_off[l] + self.dims[l][1]]

    # ---- one step ----------------------------------------------------------------------------
    def _table(self, table) -> torch.Tensor:
        words = pack_truth_table(table)
        if words.shape[0] != 1 << self.G:
            raise ValueError(f"the model has {self.G} input gates; the truth table has {words.shape[0]} rows")
        key = words.tobytes()
        if key != self._table_key:
            self._table_dev = torch.from_numpy(words.view(np.int32)).to(self.device)
            self._table_key = key
        return self._table_dev

    def _buffers(self, B: int) -> dict:
        bf = self._bufs.get(B)
        if bf is not None:
            return bf
        off, o = {}, 0

        def take(name, cnt):
            nonlocal o
            off[name] = o
            o = (o + int(cnt) + 63) // 64 * 64

        nh = len(self.dims) - 1
        take("u", B * U_LD)
        take("g_u", B * U_LD)
        for l in range(nh):
            take(f"h{l}", B * self.dims[l][1])
            take(f"g{l}", B * self.dims[l][1])
        for name in ("y", "pred", "g_pred"):
            take(name, B)
        take("kl", self.G + 1)
        take("sums3", 4)
        ws = torch.zeros(o, dtype=torch.float32, device=self.device)
        # hidden layers' weight gradients: dW_l = a_l^T g_l (a_0 = u), the DenseStack split rule over the batch.  Split: every
        # slab is a whole gradient buffer; slab 0 also takes the output layer's gradient (head kernel) and the scalars'
        # (dib_circuit_bwd), the other slabs' regions of those stay zero - the optimizer's launch sums the slabs in order
        nsplit = max(1, min(32, B // 64))
        rps = ((B + nsplit - 1) // nsplit + 31) // 32 * 32
        nsplit = (B + rps - 1) // rps
        slabs = torch.zeros(nsplit * self.n_params, dtype=torch.float32, device=self.device) if nsplit > 1 else None
        gt = slabs if nsplit > 1 else self.grads
        descs = [_d(off["u" if l == 0 else f"h{l - 1}"], self.dims[l][0], off[f"g{l}"], self.dims[l][1], self.w_off[l],
                    self.dims[l][1], self.dims[l][0], self.dims[l][1], B, bias_off=self.b_off[l]) for l in range(nh)]
        wgrad = _Gemm(2, descs, ws, ws, gt, bias_out=gt, nsplit=nsplit, rows_per_split=rps, split_stride=self.n_params)
        wgrad.upload(self.device)
        ptrs = lambda pre: (ctypes.c_void_p * 3)(*[_ptr(ws, off[f"{pre}{l}"]).value if l < nh else None for l in range(3)])
        head_ws = torch.zeros(int(self.lib.dib_mlp_small_head_workspace_bytes(ctypes.byref(self._desc), B)) // 4 + 4,
                              dtype=torch.float32, device=self.device)
        bf = dict(ws=ws, off=off, rows=torch.zeros(B, dtype=torch.int32, device=self.device), wgrad=wgrad, nsplit=nsplit,
                  slabs=slabs, gt=gt, h=ptrs("h"), g=ptrs("g"), head_ws=head_ws)
        self._bufs[B] = bf
        return bf

    def _view(self, bf, name, n):
        o = bf["off"][name]
        return bf["ws"][o: o + n]

    def _check_batch(self, B: int) -> None:
        if not self.lib.dib_circuit_supported(self.G, int(B)) or not self.lib.dib_mlp_small_head_supported(ctypes.byref(self._desc),
                                                                                                          int(B)):
            raise ValueError(f"batch size {B} outside the kernels' envelope 1 <= B <= {MAX_BATCH}")

    def _step(self, table_dev: torch.Tensor, B: int, beta: float, row_idx: Optional[torch.Tensor] = None) -> dict:
        lib, st, G = self.lib, self.eng._stream(), self.G
        bf = self._buffers(B)
        ws, off = bf["ws"], bf["off"]
        sc = _ptr(self.params, self.sc_off)
        seed, step = self.noise_seed, self.step & 0xFFFFFFFF
        check(lib.dib_circuit_fwd(_ptr(table_dev), G, B, sc, seed, step, float(beta), _ptr(row_idx) if row_idx is not None else None,
                                  _ptr(bf["rows"]), _ptr(ws, off["u"]), _ptr(ws, off["y"]), _ptr(ws, off["kl"]), st), "dib_circuit_fwd")
        check(lib.dib_mlp_small_head_step(ctypes.byref(self._desc), _ptr(self.params), _ptr(ws, off["u"]), B, _ptr(ws, off["y"]), 1,
                                          _lib.LOSS_KINDS["bce_logits"], 1.0 / B, bf["h"], bf["g"], _ptr(ws, off["pred"]),
                                          _ptr(ws, off["g_pred"]), _ptr(ws, off["g_u"]), _ptr(bf["gt"]), _ptr(ws, off["sums3"]),
                                          _ptr(bf["head_ws"]), st), "dib_mlp_small_head_step")
        bf["wgrad"].run(lib, st)
        check(lib.dib_circuit_bwd(_ptr(table_dev), G, B, sc, seed, step, float(beta), _ptr(bf["rows"]), _ptr(ws, off["g_u"]),
                                  _ptr(bf["gt"], self.sc_off), st), "dib_circuit_bwd")
        # grads = the fixed-order sum of the slabs (as given when unsplit), Keras Adam and the step count: one launch
        split = bf["nsplit"] > 1
        check(lib.dib_reduce_adam_step(_ptr(bf["slabs"]) if split else None, bf["nsplit"] if split else 0, self.n_params,
                                       _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v), self.n_params,
                                       _ptr(self.lr_dev), _ptr(self.t_dev), 0.9, 0.999, 1e-7, 1.0, _ptr(self._sync), st),
              "dib_reduce_adam_step")
        self.step += 1
        return bf

    def train_step(self, truth_table, beta: float, batch_size: int = 512, row_idx=None) -> torch.Tensor:
        """cell 6 train_step: one batch drawn from the truth table ([2^G, G + 1] 0/1 rows), BCE + beta sum_g KL_g, Keras Adam.
        Returns the batch's mean BCE (nats) as a fresh device scalar, without synchronising.  row_idx ([B] ints): use these
        rows instead of the device draw."""
        B = int(batch_size) if row_idx is None else int(len(row_idx))
        self._check_batch(B)
        table = self._table(truth_table)
        ri = None
        if row_idx is not None:
            ri = torch.as_tensor(np.asarray(row_idx) if not torch.is_tensor(row_idx) else row_idx).to(self.device, torch.int32)
            ri = ri.contiguous()
        bf = self._step(table, B, beta, ri)
        o = bf["off"]["sums3"]
        return bf["ws"][o + 2: o + 3].clone()[0]

    def last_step(self, batch_size: int) -> dict:
        """device views of the last step at this batch size: rows [B], u [B, 16], y [B], pred [B] (logits), g_u [B, 16], kl [G + 1]"""
        bf, B = self._bufs[int(batch_size)], int(batch_size)
        v = lambda name, n: self._view(bf, name, n)
        return {"rows": bf["rows"], "u": v("u", B * U_LD).view(B, U_LD), "y": v("y", B), "pred": v("pred", B),
                "g_u": v("g_u", B * U_LD).view(B, U_LD), "kl": v("kl", self.G + 1), "bce": v("sums3", 3)[2]}

    def set_lr(self, learning_rate: float) -> None:
        self.lr_dev.fill_(float(learning_rate))

    # ---- information of the channels ---------------------------------------------------------------
    def estimate_channel_mi_bounds(self, seed: int = 0, evaluation_batch_size: int = 1024, number_evaluation_batches: int = 8,
                                   per_batch: bool = False) -> np.ndarray:
        """cell 6's estimate_mi_sandwich_bounds(feature_encoder, [[-1.], [1]]) for every gate at once: [G, 2] (lower, upper) in
        nats, the mean over the batches ([G, nb, 2] with per_batch).  The inputs of each batch are drawn by the seeded NumPy rule
        of utils.estimate_mi_sandwich_bounds for a 2-row dataset; one dib_circuit_mi_bounds launch."""
        n, nb = int(evaluation_batch_size), int(number_evaluation_batches)
        if self.lib.dib_circuit_mi_workspace_bytes(self.G, n, nb) < 0:
            raise ValueError(f"evaluation of {nb} batches of {n} points outside the kernel's envelope (n >= 2, 1 <= nb <= 65535)")
        rng = np.random.default_rng(seed)
        data = np.array([-1.0, 1.0], dtype=np.float32)
        x = np.stack([data[rng.integers(0, 2, n)] for _ in range(nb)], 0)
        key = (n, nb)
        ws = self._mi_ws.get(key)
        if ws is None:
            ws = self._mi_ws[key] = torch.zeros(int(self.lib.dib_circuit_mi_workspace_bytes(self.G, n, nb)) // 8 + 1,
                                                dtype=torch.float64, device=self.device)
        xd = torch.from_numpy(x).to(self.device)
        out = torch.empty((self.G, nb, 2), dtype=torch.float64, device=self.device)
        check(self.lib.dib_circuit_mi_bounds(_ptr(self.params, self.sc_off), self.G, _ptr(xd), n, nb, int(seed) & (2 ** 64 - 1),
                                             _ptr(out), _ptr(ws), self.eng._stream()), "dib_circuit_mi_bounds")
        r = out.cpu().numpy()
        return r if per_batch else np.mean(r, axis=1)

    # ---- training loop -----------------------------------------------------------------------
    def fit(self, truth_table, number_training_steps: int = 50_000, batch_size: int = 512, learning_rate: float = 1e-3,
            beta_start: float = 1e-3, beta_end: float = 5.0, evaluate_mutual_info_freq: Optional[int] = None,
            seed: int = 0) -> dict:
        """cell 6's loop: for every step assign beta (log-linear ramp), train one batch, and where step % freq == 0 (step 0
        included) estimate every channel's sandwich bounds (seed evaluation_seed(seed, step)).  Returns bce_loss_series [n]
        (nats), beta [n], mutual_information_bounds [n_eval, G, 2] (bits) and evaluation_steps.  The host synchronises only at
        evaluations."""
        n = int(number_training_steps)
        B = int(batch_size)
        self._check_batch(B)
        table = self._table(truth_table)
        freq = int(evaluate_mutual_info_freq) if evaluate_mutual_info_freq is not None else max(1, n // 200)
        self.set_lr(learning_rate)
        hist = torch.zeros(n, dtype=torch.float32, device=self.device)
        betas, bounds, steps = [], [], []
        for step in range(n):
            beta = beta_schedule(step, n, beta_start, beta_end)
            betas.append(beta)
            bf = self._step(table, B, beta)
            o = bf["off"]["sums3"]
            hist[step: step + 1].copy_(bf["ws"][o + 2: o + 3])
            if step % freq == 0:
                bounds.append(self.estimate_channel_mi_bounds(evaluation_seed(seed, step)) / np.log(2))
                steps.append(step)
        return {"bce_loss_series": hist.cpu().numpy(), "beta": np.asarray(betas, dtype=np.float64),
                "mutual_information_bounds": np.asarray(bounds).reshape(-1, self.G, 2), "evaluation_steps": np.asarray(steps),
                "evaluate_mutual_info_freq": freq}
