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
fallback: shapes outside the kernels' envelope raise ValueError before anything is launched.
CircuitEnsemble trains R such models (other circuits, seeds, beta ramps) in lockstep on the batched twins of these entry points,
the replica being a grid index: the same five launches per step whatever R."""
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


def _flat_layout(units):
    """the flat parameter buffer of a model with hidden widths `units`: the predictor (DenseStack layout, input padded to 16
    columns), then s[0..G), lv[0..G) at sc_off.  Returns (dims, w_off, b_off, sc_off, n_params); none depends on G (2 G <= 32
    scalars fit the 64-float tail), so models of different circuits share it."""
    dims = [U_LD] + [int(u) for u in units] + [1]
    dims = list(zip(dims[:-1], dims[1:]))
    off, w_off, b_off = 0, [], []
    for i, o in dims:
        w_off.append(off); off += (i * o + 3) // 4 * 4
        b_off.append(off); off += (o + 3) // 4 * 4
    sc_off = (off + 63) // 64 * 64
    return dims, w_off, b_off, sc_off, (sc_off + 2 * MAX_GATES + 63) // 64 * 64


def _predictor_desc(dims, w_off, b_off, activation_function) -> _MlpDesc:
    d = _MlpDesc()
    for l in range(len(dims)):
        d.w_off[l], d.b_off[l], d.width[l] = w_off[l], b_off[l], dims[l][1]
    d.n_hidden, d.in_dim, d.n_freq, d.act = len(dims) - 1, U_LD, 1, ACTIVATIONS[activation_function]
    return d


def _initial_parameters(G, dims, w_off, sc_off, n_params, init_seed) -> np.ndarray:
    """Keras glorot-uniform kernels with the TRUE fan-in G of the first layer (its pad rows stay 0 under Adam: zero gradient),
    zero biases, mu_scaling 1 and logvar -3"""
    rng = np.random.default_rng(init_seed)
    flat = np.zeros(n_params, dtype=np.float32)
    for l, ((i, o), w) in enumerate(zip(dims, w_off)):
        fan_in = G if l == 0 else i
        lim = math.sqrt(6.0 / (fan_in + o))
        k = np.zeros((i, o), np.float32)
        k[:fan_in] = rng.uniform(-lim, lim, (fan_in, o)).astype(np.float32)
        flat[w: w + i * o] = k.reshape(-1)
    flat[sc_off: sc_off + G] = 1.0          # mu_scaling
    flat[sc_off + G: sc_off + 2 * G] = -3.0  # logvar
    return flat


def _split_rule(B: int):
    """the DenseStack split rule of the hidden layers' weight gradients over the batch: (nsplit, rows_per_split)"""
    nsplit = max(1, min(32, B // 64))
    rps = ((B + nsplit - 1) // nsplit + 31) // 32 * 32
    return (B + rps - 1) // rps, rps


def _evaluation_inputs(seed: int, n: int, nb: int) -> np.ndarray:
    """x [nb, n] = +-1: the seeded NumPy draw of utils.estimate_mi_sandwich_bounds for the 2-row dataset [[-1.], [1.]]"""
    rng = np.random.default_rng(seed)
    data = np.array([-1.0, 1.0], dtype=np.float32)
    return np.stack([data[rng.integers(0, 2, n)] for _ in range(nb)], 0)


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
        self.dims, self.w_off, self.b_off, self.sc_off, self.n_params = _flat_layout(units)
        self._desc = d = _predictor_desc(self.dims, self.w_off, self.b_off, activation_function)
        nh = len(units)
        if not 1 <= nh <= 3 or not self.lib.dib_mlp_small_head_supported(ctypes.byref(d), 1):
            raise ValueError(f"predictor {units} / {activation_function} outside the row-tile head kernel's envelope "
                             "(dib_mlp_small_head_supported): 1-3 hidden layers of widths multiple of 16 up to 1024, a "
                             "piecewise-linear activation")
        flat = _initial_parameters(G, self.dims, self.w_off, self.sc_off, self.n_params, init_seed)
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
        nsplit, rps = _split_rule(B)
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
        x = _evaluation_inputs(seed, n, nb)
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


def _per_replica(value, R: int, what: str) -> List[float]:
    """a scalar for every replica, or one entry per replica"""
    if np.ndim(value) == 0:
        return [float(value)] * R
    vals = [float(v) for v in value]
    if len(vals) != R:
        raise ValueError(f"{what} takes a scalar or one value per replica ({R}); got {len(vals)}")
    return vals


class CircuitEnsemble:
    """R CircuitIB models trained in lockstep: the six circuits of Fig. S1, or one circuit over seeds.  The model's shapes do not
    depend on the circuit (u is 16 columns wide for every G), so the replicas may differ in circuit, truth table, number of
    gates, seeds and beta ramp and still share every launch of a step:
        dib_circuit_fwd_batched           every replica's row draw, gather, reparameterisation, KL          grid (tiles, R)
        dib_mlp_small_head_step_batched   every predictor's forward, BCE, dgrad chain, output-layer gradient  grid (row tiles, R)
        dib_gemm_grouped                  the hidden layers' weight gradients, 3 R descriptors (CircuitIB's slab rule)
        dib_circuit_bwd_batched           the 2 G_r scalars' gradients                                        grid (gate, R)
        dib_reduce_adam_step              slab sum and Keras Adam over the R * n_params flat buffer
    and every replica's sandwich bounds are one dib_circuit_mi_bounds_batched launch.  Replica r starts from the parameters of
    CircuitIB(G_r, ..., init_seed=init_seeds[r], noise_seed=noise_seeds[r]) and draws that model's rows and noise at the same
    step number; one learning rate and one Adam step count are shared.  params | grads | m | v are replica-major, each replica
    laid out like CircuitIB's flat buffer."""

    def __init__(self, truth_tables, predictive_arch_spec=(256, 256, 256), activation_function: str = "leaky_relu",
                 init_seeds: Optional[Sequence[int]] = None, noise_seeds: Optional[Sequence[int]] = None, device="cuda:0"):
        tables = [np.asarray(t) for t in truth_tables]
        R = len(tables)
        if R < 1:
            raise ValueError("a CircuitEnsemble takes at least one truth table (R >= 1)")
        self.init_seeds = [int(s) for s in init_seeds] if init_seeds is not None else list(range(R))
        self.noise_seeds = [int(s) for s in noise_seeds] if noise_seeds is not None else list(range(R))
        if len(self.init_seeds) != R or len(self.noise_seeds) != R:
            raise ValueError(f"init_seeds and noise_seeds take one seed per replica ({R})")
        words = [pack_truth_table(t) for t in tables]          # ValueError unless [2^G, G + 1] 0/1 rows, 1 <= G <= 16
        self.G = [t.shape[1] - 1 for t in tables]
        self.units = [int(u) for u in predictive_arch_spec]
        if activation_function not in ACTIVATIONS:
            raise ValueError(f"unknown activation {activation_function!r}")
        if not 1 <= len(self.units) <= 3:
            raise ValueError(f"predictor {self.units}: 1-3 hidden layers")
        if not torch.cuda.is_available():
            raise RuntimeError("CircuitEnsemble runs on the GPU (libdib_hip); no device is available")
        self.R, self.activation_function = R, activation_function
        self.tables = tables
        self.eng = _Eng(device)
        self.lib, self.device = self.eng.lib, self.eng.device
        self.dims, self.w_off, self.b_off, self.sc_off, self.n_params = _flat_layout(self.units)
        self._desc = d = _predictor_desc(self.dims, self.w_off, self.b_off, activation_function)
        if not self.lib.dib_mlp_small_head_batched_supported(ctypes.byref(d), 1, R):
            raise ValueError(f"predictor {self.units} / {activation_function} x {R} replicas outside the row-tile head kernel's "
                             "envelope (dib_mlp_small_head_batched_supported)")
        P = self.n_params
        flat = np.concatenate([_initial_parameters(G, self.dims, self.w_off, self.sc_off, P, s)
                               for G, s in zip(self.G, self.init_seeds)])
        self._flat = torch.zeros(4 * R * P, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.adam_m, self.adam_v = (self._flat[i * R * P: (i + 1) * R * P] for i in range(4))
        self.params.copy_(torch.from_numpy(flat))
        offs = np.concatenate([[0], np.cumsum([w.shape[0] for w in words])])
        self._tables_dev = torch.from_numpy(np.concatenate(words).view(np.int32)).to(self.device)
        self._table_words = int(offs[-1])
        self._table_off_c = (ctypes.c_int64 * R)(*[int(o) for o in offs[:-1]])
        self._G_c = (ctypes.c_int * R)(*self.G)
        self._seeds_c = (ctypes.c_uint64 * R)(*[s & (2 ** 64 - 1) for s in self.noise_seeds])
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.lr_dev = torch.full((1,), 1e-3, dtype=torch.float32, device=self.device)
        self._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32, device=self.device)
        self.step = 0                 # the noise key's step of the next training batch (every replica's)
        self._bufs: Dict[int, dict] = {}
        self._mi_ws: Dict[tuple, torch.Tensor] = {}

    # ---- one step ----------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        bf = self._bufs.get(B)
        if bf is not None:
            return bf
        R, P, off, o = self.R, self.n_params, {}, 0

        def take(name, cnt):
            nonlocal o
            off[name] = o
            o = (o + int(cnt) + 63) // 64 * 64

        nh = len(self.dims) - 1
        take("u", R * B * U_LD)
        take("g_u", R * B * U_LD)
        for l in range(nh):
            take(f"h{l}", R * B * self.dims[l][1])
            take(f"g{l}", R * B * self.dims[l][1])
        for name in ("y", "pred", "g_pred"):
            take(name, R * B)
        take("kl", R * (MAX_GATES + 1))
        take("sums3", R * 3)
        ws = torch.zeros(o, dtype=torch.float32, device=self.device)
        # CircuitIB's slab rule per replica: a slab is a whole R * n_params gradient buffer; slab 0 also takes the output
        # layers' gradients (head kernel) and the scalars' (dib_circuit_bwd_batched)
        nsplit, rps = _split_rule(B)
        slabs = torch.zeros(nsplit * R * P, dtype=torch.float32, device=self.device) if nsplit > 1 else None
        gt = slabs if nsplit > 1 else self.grads
        descs = [_d(off["u" if l == 0 else f"h{l - 1}"] + r * B * self.dims[l][0], self.dims[l][0],
                    off[f"g{l}"] + r * B * self.dims[l][1], self.dims[l][1], r * P + self.w_off[l], self.dims[l][1],
                    self.dims[l][0], self.dims[l][1], B, bias_off=r * P + self.b_off[l]) for r in range(R) for l in range(nh)]
        wgrad = _Gemm(2, descs, ws, ws, gt, bias_out=gt, nsplit=nsplit, rows_per_split=rps, split_stride=R * P)
        wgrad.upload(self.device)
        ptrs = lambda pre: (ctypes.c_void_p * 3)(*[_ptr(ws, off[f"{pre}{l}"]).value if l < nh else None for l in range(3)])
        head_ws = torch.zeros(int(self.lib.dib_mlp_small_head_batched_workspace_bytes(ctypes.byref(self._desc), B, R)) // 4 + 4,
                              dtype=torch.float32, device=self.device)
        bf = dict(ws=ws, off=off, rows=torch.zeros((R, B), dtype=torch.int32, device=self.device), wgrad=wgrad, nsplit=nsplit,
                  slabs=slabs, gt=gt, h=ptrs("h"), g=ptrs("g"), head_ws=head_ws)
        self._bufs[B] = bf
        return bf

    def _check_batch(self, B: int) -> None:
        if not self.lib.dib_circuit_batched_supported(self._G_c, self.R, int(B)) or \
                not self.lib.dib_mlp_small_head_batched_supported(ctypes.byref(self._desc), int(B), self.R):
            raise ValueError(f"batch size {B} outside the kernels' envelope 1 <= B <= {MAX_BATCH}")

    def _step(self, B: int, betas: Sequence[float], row_idx: Optional[torch.Tensor] = None) -> dict:
        lib, st, R, P = self.lib, self.eng._stream(), self.R, self.n_params
        bf = self._buffers(B)
        ws, off = bf["ws"], bf["off"]
        beta_c = (ctypes.c_float * R)(*betas)
        step = self.step & 0xFFFFFFFF
        tab = (_ptr(self._tables_dev), self._table_words, self._table_off_c, self._G_c, R, B, _ptr(self.params), P, self.sc_off,
               self._seeds_c, step, beta_c)
        check(lib.dib_circuit_fwd_batched(*tab, _ptr(row_idx) if row_idx is not None else None, _ptr(bf["rows"]), _ptr(ws, off["u"]),
                                          _ptr(ws, off["y"]), _ptr(ws, off["kl"]), st), "dib_circuit_fwd_batched")
        check(lib.dib_mlp_small_head_step_batched(ctypes.byref(self._desc), _ptr(self.params), P, _ptr(ws, off["u"]), B, R,
                                                  _ptr(ws, off["y"]), 1, _lib.LOSS_KINDS["bce_logits"], 1.0 / B, bf["h"], bf["g"],
                                                  _ptr(ws, off["pred"]), _ptr(ws, off["g_pred"]), _ptr(ws, off["g_u"]),
                                                  _ptr(bf["gt"]), P, _ptr(ws, off["sums3"]), _ptr(bf["head_ws"]), st),
              "dib_mlp_small_head_step_batched")
        bf["wgrad"].run(lib, st)
        check(lib.dib_circuit_bwd_batched(*tab, _ptr(bf["rows"]), _ptr(ws, off["g_u"]), _ptr(bf["gt"]), P, st),
              "dib_circuit_bwd_batched")
        split = bf["nsplit"] > 1
        check(lib.dib_reduce_adam_step(_ptr(bf["slabs"]) if split else None, bf["nsplit"] if split else 0, R * P,
                                       _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v), R * P,
                                       _ptr(self.lr_dev), _ptr(self.t_dev), 0.9, 0.999, 1e-7, 1.0, _ptr(self._sync), st),
              "dib_reduce_adam_step")
        self.step += 1
        return bf

    def _bce(self, bf) -> torch.Tensor:
        o = bf["off"]["sums3"]
        return bf["ws"][o: o + 3 * self.R].view(self.R, 3)[:, 2]

    def train_step(self, beta, batch_size: int = 512, row_idx=None) -> torch.Tensor:
        """One step of every replica on a batch drawn from its own truth table.  beta: a float or R floats; row_idx ([R, B]
        ints): use these rows instead of the device draws.  Returns the R mean BCEs (nats) as a fresh device vector, without
        synchronising."""
        betas = _per_replica(beta, self.R, "beta")
        ri, B = None, int(batch_size)
        if row_idx is not None:
            ri = np.asarray(row_idx) if not torch.is_tensor(row_idx) else row_idx
            if ri.ndim != 2 or ri.shape[0] != self.R:
                raise ValueError(f"row_idx must be [replicas = {self.R}, batch]")
            B = int(ri.shape[1])
        self._check_batch(B)
        if ri is not None:
            ri = torch.as_tensor(ri).to(self.device, torch.int32).contiguous()
        return self._bce(self._step(B, betas, ri)).clone()

    def last_step(self, r: int, batch_size: int) -> dict:
        """device views of replica r's last step at this batch size, with the keys of CircuitIB.last_step"""
        r = self._replica(r)
        bf, B, G = self._bufs[int(batch_size)], int(batch_size), self.G[r]

        def v(name, n):
            o = bf["off"][name] + r * n
            return bf["ws"][o: o + n]

        return {"rows": bf["rows"][r], "u": v("u", B * U_LD).view(B, U_LD), "y": v("y", B), "pred": v("pred", B),
                "g_u": v("g_u", B * U_LD).view(B, U_LD), "kl": v("kl", MAX_GATES + 1)[:G + 1], "bce": v("sums3", 3)[2]}

    def set_lr(self, learning_rate: float) -> None:
        self.lr_dev.fill_(float(learning_rate))

    # ---- information of the channels ---------------------------------------------------------------
    def estimate_channel_mi_bounds(self, seeds: Optional[Sequence[int]] = None, evaluation_batch_size: int = 1024,
                                   number_evaluation_batches: int = 8, per_batch: bool = False) -> List[np.ndarray]:
        """CircuitIB.estimate_channel_mi_bounds(seeds[r], ...) of every replica (default seeds 0..R-1) in ONE
        dib_circuit_mi_bounds_batched launch and one read-back: a list of [G_r, 2] arrays (nats; [G_r, nb, 2] with per_batch)"""
        R, n, nb = self.R, int(evaluation_batch_size), int(number_evaluation_batches)
        seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != R:
            raise ValueError(f"seeds takes one seed per replica ({R})")
        need = int(self.lib.dib_circuit_mi_batched_workspace_bytes(R, n, nb))
        if need < 0:
            raise ValueError(f"evaluation of {nb} batches of {n} points outside the kernel's envelope (n >= 2, 1 <= nb <= 65535)")
        x = np.stack([_evaluation_inputs(s, n, nb) for s in seeds], 0)
        ws = self._mi_ws.get((n, nb))
        if ws is None:
            ws = self._mi_ws[(n, nb)] = torch.zeros(need // 8 + 1, dtype=torch.float64, device=self.device)
        xd = torch.from_numpy(x).to(self.device)
        out = torch.empty((R, MAX_GATES, nb, 2), dtype=torch.float64, device=self.device)
        seeds_c = (ctypes.c_uint64 * R)(*[s & (2 ** 64 - 1) for s in seeds])
        check(self.lib.dib_circuit_mi_bounds_batched(_ptr(self.params), self.n_params, self.sc_off, self._G_c, R, _ptr(xd), n, nb,
                                                     seeds_c, _ptr(out), _ptr(ws), self.eng._stream()),
              "dib_circuit_mi_bounds_batched")
        res = out.cpu().numpy()
        return [res[r, :G].copy() if per_batch else np.mean(res[r, :G], axis=1) for r, G in enumerate(self.G)]

    # ---- training loop -----------------------------------------------------------------------
    def fit(self, number_training_steps: int = 50_000, batch_size: int = 512, learning_rate: float = 1e-3, beta_start=1e-3,
            beta_end=5.0, evaluate_mutual_info_freq: Optional[int] = None, seeds: Optional[Sequence[int]] = None) -> List[dict]:
        """CircuitIB.fit for every replica at once: each replica ramps beta on beta_schedule between its own beta_start and
        beta_end (scalars, or one per replica), and where step % freq == 0 all replicas' bounds come from one launch, replica r
        with the inputs and noise key of CircuitIB.fit(seed=seeds[r]) (default seeds 0..R-1).  Returns one history per replica
        with the keys of CircuitIB.fit.  The host synchronises only at evaluations."""
        R, n, B = self.R, int(number_training_steps), int(batch_size)
        b0, b1 = _per_replica(beta_start, R, "beta_start"), _per_replica(beta_end, R, "beta_end")
        seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != R:
            raise ValueError(f"seeds takes one seed per replica ({R})")
        self._check_batch(B)
        freq = int(evaluate_mutual_info_freq) if evaluate_mutual_info_freq is not None else max(1, n // 200)
        self.set_lr(learning_rate)
        hist = torch.zeros((n, R), dtype=torch.float32, device=self.device)
        betas, bounds, steps = [], [[] for _ in range(R)], []
        for step in range(n):
            beta = [beta_schedule(step, n, b0[r], b1[r]) for r in range(R)]
            betas.append(beta)
            hist[step].copy_(self._bce(self._step(B, beta)))
            if step % freq == 0:
                ev = self.estimate_channel_mi_bounds([evaluation_seed(s, step) for s in seeds])
                for r in range(R):
                    bounds[r].append(ev[r] / np.log(2))
                steps.append(step)
        losses, betas = hist.cpu().numpy(), np.asarray(betas, dtype=np.float64).reshape(n, R)
        return [{"bce_loss_series": losses[:, r].copy(), "beta": betas[:, r].copy(),
                 "mutual_information_bounds": np.asarray(bounds[r]).reshape(-1, self.G[r], 2), "evaluation_steps": np.asarray(steps),
                 "evaluate_mutual_info_freq": freq} for r in range(R)]

    # ---- access to replicas ------------------------------------------------------------------
    def _replica(self, r: int) -> int:
        if not 0 <= int(r) < self.R:
            raise IndexError(f"replica {r} of {self.R}")
        return int(r)

    def replica_params(self, r: int) -> torch.Tensor:
        """replica r's slice [n_params] of the live parameter buffer (CircuitIB's layout)"""
        r = self._replica(r)
        return self.params[r * self.n_params: (r + 1) * self.n_params]

    def get_weights(self, r: int) -> dict:
        """replica r: {"predictive_model": Keras-ordered [kernel, bias] per layer (the first kernel [G_r, width]),
        "mu_scaling": [G_r], "logvar": [G_r]}"""
        p, G = self.replica_params(r).cpu().numpy(), self.G[self._replica(r)]
        w = []
        for l, ((i, o), wo, bo) in enumerate(zip(self.dims, self.w_off, self.b_off)):
            k = p[wo: wo + i * o].reshape(i, o)
            w += [(k[:G] if l == 0 else k).copy(), p[bo: bo + o].copy()]
        return {"predictive_model": w, "mu_scaling": p[self.sc_off: self.sc_off + G].copy(),
                "logvar": p[self.sc_off + G: self.sc_off + 2 * G].copy()}

    def set_weights(self, r: int, weights: dict) -> None:
        """the counterpart of get_weights: any subset of its keys"""
        live, G = self.replica_params(r), self.G[self._replica(r)]
        put = lambda o, a: live[o: o + a.size].copy_(torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)))
        if "predictive_model" in weights:
            ws = weights["predictive_model"]
            assert len(ws) == 2 * len(self.dims)
            for l, ((i, o), wo, bo) in enumerate(zip(self.dims, self.w_off, self.b_off)):
                k = np.asarray(ws[2 * l], dtype=np.float32)
                if l == 0:
                    k = np.concatenate([k.reshape(G, o), np.zeros((U_LD - G, o), np.float32)], 0)
                put(wo, k.reshape(i, o))
                put(bo, np.asarray(ws[2 * l + 1], dtype=np.float32).reshape(o))
        if "mu_scaling" in weights:
            put(self.sc_off, np.asarray(weights["mu_scaling"], dtype=np.float32).reshape(G))
        if "logvar" in weights:
            put(self.sc_off + G, np.asarray(weights["logvar"], dtype=np.float32).reshape(G))

    def to_model(self, r: int) -> CircuitIB:
        """a CircuitIB holding replica r's parameters and Adam state (moments, step count, learning rate) at the current step:
        trained on with the same beta and rows it takes the ensemble's replica r's next step, bit for bit"""
        r = self._replica(r)
        m = CircuitIB(self.G[r], self.units, self.activation_function, noise_seed=self.noise_seeds[r], init_seed=self.init_seeds[r],
                      device=self.device)
        sl = slice(r * self.n_params, (r + 1) * self.n_params)
        m.params.copy_(self.params[sl]); m.grads.copy_(self.grads[sl])
        m.adam_m.copy_(self.adam_m[sl]); m.adam_v.copy_(self.adam_v[sl])
        m.t_dev.copy_(self.t_dev); m.lr_dev.copy_(self.lr_dev)
        m.step = self.step
        return m
