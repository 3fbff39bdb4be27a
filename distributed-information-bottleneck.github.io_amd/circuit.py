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
the replica being a grid index: the same five launches per step whatever R.  Both classes are faces of _CircuitCore, which
holds the state and everything around the C calls once; CircuitIB launches through the single entry points."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._flat_optimizer import FlatOptimizer, HoldsFlatOptimizer
from ._gemm_plan import _Gemm, _d, _ptr, _ptr_array3, slab_rule
from ._host import Carver, LibHandle
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


def _evaluation_inputs(seed: int, n: int, nb: int) -> np.ndarray:
    """x [nb, n] = +-1: the seeded NumPy draw of utils.estimate_mi_sandwich_bounds for the 2-row dataset [[-1.], [1.]]"""
    rng = np.random.default_rng(seed)
    data = np.array([-1.0, 1.0], dtype=np.float32)
    return np.stack([data[rng.integers(0, 2, n)] for _ in range(nb)], 0)


def _per_replica(value, R: int, what: str) -> List[float]:
    """a scalar for every replica, or one entry per replica"""
    if np.ndim(value) == 0:
        return [float(value)] * R
    vals = [float(v) for v in value]
    if len(vals) != R:
        raise ValueError(f"{what} takes a scalar or one value per replica ({R}); got {len(vals)}")
    return vals


def _replica_seeds(seeds, R: int) -> List[int]:
    """one evaluation seed per replica (default 0..R-1)"""
    seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
    if len(seeds) != R:
        raise ValueError(f"seeds takes one seed per replica ({R})")
    return seeds


class _CircuitCore(HoldsFlatOptimizer):
    """What CircuitIB and CircuitEnsemble are faces of: R replicas' gate counts, the flat layout and the predictor descriptor they
    share, the flat state (params | grads and the optimizer's m | v, replica-major, n_params each) and, written once, the
    workspace map of a batch size, the step, the evaluation of the channels' bounds, the fit loop and the access to a replica's
    weights.  `batched` says which entry points launch them: the batched ones (the replica a grid index, any R), or - only for
    R = 1 - the single ones, which are 1.6 us per step faster there (profiles/HISTORY.md).  The two differ only where a C call
    is made; the faces translate their signatures (a truth table per call against tables at construction, scalars against
    per-replica lists, one history against a list) into the core's."""

    def _setup(self, gates, predictive_arch_spec, activation_function, init_seeds, noise_seeds, device, batched: bool) -> None:
        self.gates, self.R, self.batched = [int(G) for G in gates], len(gates), bool(batched)
        assert batched or self.R == 1
        self.init_seeds, self.noise_seeds = init_seeds, noise_seeds
        self.units, self.activation_function = [int(u) for u in predictive_arch_spec], activation_function
        if activation_function not in ACTIVATIONS:
            raise ValueError(f"unknown activation {activation_function!r}")
        if not 1 <= len(self.units) <= 3:
            raise ValueError(f"predictor {self.units}: 1-3 hidden layers")
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} runs on the GPU (libdib_hip); no device is available")
        self.eng = LibHandle(device)
        lib, self.device = self.eng.lib, self.eng.device
        self.lib, R = lib, self.R
        self.dims, self.w_off, self.b_off, self.sc_off, self.n_params = _flat_layout(self.units)
        self._desc = d = _predictor_desc(self.dims, self.w_off, self.b_off, activation_function)
        if not (lib.dib_mlp_small_head_batched_supported(ctypes.byref(d), 1, R) if batched
                else lib.dib_mlp_small_head_supported(ctypes.byref(d), 1)):
            raise ValueError(f"predictor {self.units} / {activation_function}{f' x {R} replicas' if batched else ''} outside the "
                             f"row-tile head kernel's envelope (dib_mlp_small_head{'_batched' if batched else ''}_supported): 1-3 "
                             "hidden layers of widths multiple of 16 up to 1024, a piecewise-linear activation")
        P = self.n_params
        flat = np.concatenate([_initial_parameters(G, self.dims, self.w_off, self.sc_off, P, s)
                               for G, s in zip(self.gates, init_seeds)])
        self.params = torch.from_numpy(flat).to(self.device)
        self.grads = torch.zeros(R * P, dtype=torch.float32, device=self.device)
        self.opt_state = FlatOptimizer(lib, self.eng._stream, R * P, self.device)
        self._G_c = (ctypes.c_int * R)(*self.gates)
        self._seeds_c = (ctypes.c_uint64 * R)(*[s & (2 ** 64 - 1) for s in noise_seeds])
        self.step = 0                 # the noise key's step of the next training batch (every replica's)
        self._bufs: Dict[int, dict] = {}
        self._mi_ws: Dict[tuple, torch.Tensor] = {}

    # ---- one step ----------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        bf = self._bufs.get(B)
        if bf is not None:
            return bf
        R, P, nh, c = self.R, self.n_params, len(self.dims) - 1, Carver(64)
        c.take("u", R * B * U_LD)
        c.take("g_u", R * B * U_LD)
        for l in range(nh):
            c.take(f"h{l}", R * B * self.dims[l][1])
            c.take(f"g{l}", R * B * self.dims[l][1])
        for name in ("y", "pred", "g_pred"):
            c.take(name, R * B)
        c.take("kl", R * (MAX_GATES + 1))
        c.take("sums3", R * 3)
        off, ws = c.off, torch.zeros(c.size, dtype=torch.float32, device=self.device)
        # hidden layers' weight gradients: dW_l = a_l^T g_l (a_0 = u), the slab rule over the batch.  Split: every slab is a whole
        # R * n_params gradient buffer; slab 0 also takes the output layers' gradients (head kernel) and the scalars' (circuit
        # backward), the other slabs' regions of those stay zero - the optimizer's launch sums the slabs in order
        nsplit, rps = slab_rule(B)
        slabs = torch.zeros(nsplit * R * P, dtype=torch.float32, device=self.device) if nsplit > 1 else None
        gt = slabs if nsplit > 1 else self.grads
        descs = [_d(off["u" if l == 0 else f"h{l - 1}"] + r * B * self.dims[l][0], self.dims[l][0],
                    off[f"g{l}"] + r * B * self.dims[l][1], self.dims[l][1], r * P + self.w_off[l], self.dims[l][1],
                    self.dims[l][0], self.dims[l][1], B, bias_off=r * P + self.b_off[l]) for r in range(R) for l in range(nh)]
        wgrad = _Gemm(2, descs, ws, ws, gt, bias_out=gt, nsplit=nsplit, rows_per_split=rps, split_stride=R * P)
        wgrad.upload(self.device)
        ptrs = lambda pre: _ptr_array3(ws, [off[f"{pre}{l}"] for l in range(nh)])
        d, lib = ctypes.byref(self._desc), self.lib
        head_bytes = lib.dib_mlp_small_head_batched_workspace_bytes(d, B, R) if self.batched \
            else lib.dib_mlp_small_head_workspace_bytes(d, B)
        rows = torch.zeros((R, B), dtype=torch.int32, device=self.device)
        head_ws = torch.zeros(int(head_bytes) // 4 + 4, dtype=torch.float32, device=self.device)
        # the arguments of a step that do not change from one step to the next, grouped as the entry points take them
        p = {name: _ptr(ws, o) for name, o in off.items()}
        args = dict(u=p["u"], y=p["y"], gt=_ptr(gt), gt_scalars=_ptr(gt, self.sc_off), fwd=(_ptr(rows), p["u"], p["y"], p["kl"]),
                    head=(1, _lib.LOSS_KINDS["bce_logits"], 1.0 / B, ptrs("h"), ptrs("g"), p["pred"], p["g_pred"], p["g_u"], _ptr(gt)),
                    head_out=(p["sums3"], _ptr(head_ws)), bwd=(_ptr(rows), p["g_u"]))
        bf = dict(ws=ws, off=off, rows=rows, wgrad=wgrad, nsplit=nsplit, slabs=slabs, nslabs=nsplit if nsplit > 1 else 0, gt=gt,
                  head_ws=head_ws, args=args)
        self._bufs[B] = bf
        return bf

    def _check_batch(self, B: int) -> None:
        lib, d, B = self.lib, ctypes.byref(self._desc), int(B)
        if self.batched:
            ok = lib.dib_circuit_batched_supported(self._G_c, self.R, B) and lib.dib_mlp_small_head_batched_supported(d, B, self.R)
        else:
            ok = lib.dib_circuit_supported(self.gates[0], B) and lib.dib_mlp_small_head_supported(d, B)
        if not ok:
            raise ValueError(f"batch size {B} outside the kernels' envelope 1 <= B <= {MAX_BATCH}")

    def _launch_step(self, table_dev: Optional[torch.Tensor], B: int, betas, row_idx: Optional[torch.Tensor] = None) -> dict:
        """one step of every replica.  The batched path takes the R floats `betas` and has its own tables (table_dev None); the
        single path takes its truth table and ONE float, which makes this CircuitIB._step itself, with no call in between"""
        lib, st, R, P = self.lib, self.eng._stream(), self.R, self.n_params
        bf = self._buffers(B)
        a, desc, params = bf["args"], ctypes.byref(self._desc), _ptr(self.params)
        step, ri = self.step & 0xFFFFFFFF, _ptr(row_idx) if row_idx is not None else None
        if self.batched:
            tab = (_ptr(self._tables_dev), self._table_words, self._table_off_c, self._G_c, R, B, params, P, self.sc_off,
                   self._seeds_c, step, (ctypes.c_float * R)(*betas))
            check(lib.dib_circuit_fwd_batched(*tab, ri, *a["fwd"], st), "dib_circuit_fwd_batched")
            check(lib.dib_mlp_small_head_step_batched(desc, params, P, a["u"], B, R, a["y"], *a["head"], P, *a["head_out"], st),
                  "dib_mlp_small_head_step_batched")
            bf["wgrad"].run(lib, st)
            check(lib.dib_circuit_bwd_batched(*tab, *a["bwd"], a["gt"], P, st), "dib_circuit_bwd_batched")
        else:
            tab = (_ptr(table_dev), self.gates[0], B, _ptr(self.params, self.sc_off), self.noise_seeds[0], step, float(betas))
            check(lib.dib_circuit_fwd(*tab, ri, *a["fwd"], st), "dib_circuit_fwd")
            check(lib.dib_mlp_small_head_step(desc, params, a["u"], B, a["y"], *a["head"], *a["head_out"], st),
                  "dib_mlp_small_head_step")
            bf["wgrad"].run(lib, st)
            check(lib.dib_circuit_bwd(*tab, *a["bwd"], a["gt_scalars"], st), "dib_circuit_bwd")
        # grads = the fixed-order sum of the slabs (as given when unsplit), Keras Adam and the step count: one launch
        self.opt_state.reduce_adam(bf["slabs"], bf["nslabs"], self.params, self.grads, R * P, stream=st)
        self.step += 1
        return bf

    def _bce(self, bf) -> torch.Tensor:
        o = bf["off"]["sums3"]
        return bf["ws"][o: o + 3 * self.R].view(self.R, 3)[:, 2]

    def _row_idx(self, row_idx) -> torch.Tensor:
        ri = torch.as_tensor(np.asarray(row_idx) if not torch.is_tensor(row_idx) else row_idx)
        return ri.to(self.device, torch.int32).contiguous()

    def _last_step(self, r: int, B: int) -> dict:
        bf, G = self._bufs[B], self.gates[r]

        def v(name, n):
            o = bf["off"][name] + r * n
            return bf["ws"][o: o + n]

        return {"rows": bf["rows"][r], "u": v("u", B * U_LD).view(B, U_LD), "y": v("y", B), "pred": v("pred", B),
                "g_u": v("g_u", B * U_LD).view(B, U_LD), "kl": v("kl", MAX_GATES + 1)[:G + 1], "bce": v("sums3", 3)[2]}

    # ---- information of the channels ---------------------------------------------------------------
    def _mi_bounds(self, seeds: Sequence[int], n: int, nb: int, per_batch: bool) -> List[np.ndarray]:
        """every replica's [G_r, 2] (lower, upper) in nats ([G_r, nb, 2] with per_batch), replica r on the inputs and the noise
        key of seeds[r]: one launch, one read-back"""
        lib, R, G0 = self.lib, self.R, self.gates[0]
        need = int(lib.dib_circuit_mi_batched_workspace_bytes(R, n, nb) if self.batched else lib.dib_circuit_mi_workspace_bytes(G0, n, nb))
        if need < 0:
            raise ValueError(f"evaluation of {nb} batches of {n} points outside the kernel's envelope (n >= 2, 1 <= nb <= 65535)")
        x = [_evaluation_inputs(s, n, nb) for s in seeds]
        x = x[0] if R == 1 else np.stack(x, 0)              # [R][nb][n] (one replica: no copy)
        ws = self._mi_ws.get((n, nb))
        if ws is None:
            ws = self._mi_ws[(n, nb)] = torch.zeros(need // 8 + 1, dtype=torch.float64, device=self.device)
        xd = torch.from_numpy(x).to(self.device)
        out = torch.empty((R, MAX_GATES if self.batched else G0, nb, 2), dtype=torch.float64, device=self.device)
        if self.batched:
            seeds_c = (ctypes.c_uint64 * R)(*[s & (2 ** 64 - 1) for s in seeds])
            check(lib.dib_circuit_mi_bounds_batched(_ptr(self.params), self.n_params, self.sc_off, self._G_c, R, _ptr(xd), n, nb,
                                                    seeds_c, _ptr(out), _ptr(ws), self.eng._stream()), "dib_circuit_mi_bounds_batched")
        else:
            check(lib.dib_circuit_mi_bounds(_ptr(self.params, self.sc_off), G0, _ptr(xd), n, nb, seeds[0] & (2 ** 64 - 1), _ptr(out),
                                            _ptr(ws), self.eng._stream()), "dib_circuit_mi_bounds")
        res = out.cpu().numpy()
        return [res[r, :G].copy() if per_batch else np.mean(res[r, :G], axis=1) for r, G in enumerate(self.gates)]

    # ---- training loop -----------------------------------------------------------------------
    def _fit(self, table_dev, n: int, B: int, learning_rate: float, b0: Sequence[float], b1: Sequence[float],
             evaluate_mutual_info_freq: Optional[int], seeds: Sequence[int]) -> List[dict]:
        """the notebook's loop for every replica: one history per replica; the host synchronises only at evaluations"""
        R = self.R
        freq = int(evaluate_mutual_info_freq) if evaluate_mutual_info_freq is not None else max(1, n // 200)
        self.set_lr(learning_rate)
        hist = torch.zeros((n, R), dtype=torch.float32, device=self.device)
        betas, bounds, steps = [], [[] for _ in range(R)], []
        for step in range(n):
            beta = [beta_schedule(step, n, b0[r], b1[r]) for r in range(R)]
            betas.append(beta)
            hist[step].copy_(self._bce(self._launch_step(table_dev, B, beta if self.batched else beta[0])))
            if step % freq == 0:
                ev = self._mi_bounds([evaluation_seed(s, step) for s in seeds], 1024, 8, False)
                for r in range(R):
                    bounds[r].append(ev[r] / np.log(2))
                steps.append(step)
        losses, betas = hist.cpu().numpy(), np.asarray(betas, dtype=np.float64).reshape(n, R)
        return [{"bce_loss_series": losses[:, r].copy(), "beta": betas[:, r].copy(),
                 "mutual_information_bounds": np.asarray(bounds[r]).reshape(-1, self.gates[r], 2),
                 "evaluation_steps": np.asarray(steps), "evaluate_mutual_info_freq": freq} for r in range(R)]

    # ---- a replica's weights -----------------------------------------------------------------
    def _replica(self, r: int) -> int:
        if not 0 <= int(r) < self.R:
            raise IndexError(f"replica {r} of {self.R}")
        return int(r)

    def _region(self, r: int, off: int, n: int) -> torch.Tensor:
        """n live parameters of replica r from `off` of its flat slice"""
        o = self._replica(r) * self.n_params + off
        return self.params[o: o + n]

    def _read(self, r: int, off: int, *shape) -> np.ndarray:
        return self._region(r, off, math.prod(shape)).detach().cpu().numpy().reshape(shape).copy()

    def _write(self, r: int, off: int, a, *shape) -> None:
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(shape)   # (ValueError for weights of another shape)
        self._region(r, off, a.size).copy_(torch.as_tensor(a.reshape(-1)))

    def _predictor_weights(self, r: int) -> List[np.ndarray]:
        """Keras-ordered [kernel, bias] per layer; the first kernel is [G_r, width] - its 16 - G_r zero pad rows of the device
        layout are not part of it"""
        out = []
        for l, ((i, o), wo, bo) in enumerate(zip(self.dims, self.w_off, self.b_off)):
            k = self._read(r, wo, i, o)
            out += [k[:self.gates[r]].copy() if l == 0 else k, self._read(r, bo, o)]
        return out

    def _set_predictor_weights(self, r: int, weights: Sequence[np.ndarray]) -> None:
        assert len(weights) == 2 * len(self.dims)
        for l, ((i, o), wo, bo) in enumerate(zip(self.dims, self.w_off, self.b_off)):
            k = np.asarray(weights[2 * l], dtype=np.float32)
            if l == 0:
                k = np.concatenate([k.reshape(self.gates[r], o), np.zeros((U_LD - self.gates[r], o), np.float32)], 0)
            self._write(r, wo, k, i, o)
            self._write(r, bo, weights[2 * l + 1], o)


class _FeatureEncoder:
    """cell 4 SimpleEncoder of gate `index`: get_weights / set_weights = [mu_scaling (1, 1), logvar (1, 1)]; called on x [n, 1]
    it returns [n, 2] = concat(x * mu_scaling, logvar) (a device tensor)"""

    def __init__(self, model: "CircuitIB", index: int):
        self._circuit, self.index = model, int(index)

    def _offsets(self):
        m = self._circuit
        return m.sc_off + self.index, m.sc_off + m.G + self.index

    def get_weights(self) -> List[np.ndarray]:
        return [self._circuit._read(0, o, 1, 1) for o in self._offsets()]

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        for o, w in zip(self._offsets(), weights):
            self._circuit._write(0, o, w, 1)

    def __call__(self, x) -> torch.Tensor:
        s, lv = (self._circuit._region(0, o, 1) for o in self._offsets())
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
        return self._m._predictor_weights(0)

    def set_weights(self, weights: Sequence[np.ndarray]) -> None:
        self._m._set_predictor_weights(0, weights)


class CircuitIB(_CircuitCore):
    """The Boolean-circuit notebook's model on the gfx950 kernels (cell 6 names)."""

    def __init__(self, number_input_gates: int, predictive_arch_spec=(256, 256, 256), activation_function: str = "leaky_relu",
                 noise_seed: int = 0, init_seed: int = 0, device="cuda:0"):
        G = int(number_input_gates)
        if not 1 <= G <= MAX_GATES:
            raise ValueError(f"number_input_gates {G} outside the kernels' envelope 1 <= G <= {MAX_GATES}")
        self.G = G
        self._setup([G], predictive_arch_spec, activation_function, [int(init_seed)], [int(noise_seed)], device, batched=False)
        self.scalars = self.params[self.sc_off: self.sc_off + 2 * G]
        self.feature_encoders = [_FeatureEncoder(self, g) for g in range(G)]
        self.predictive_model = _Predictor(self)
        self._table_key, self._table_dev = None, None

    noise_seed = property(lambda self: self.noise_seeds[0], lambda self, s: self.noise_seeds.__setitem__(0, int(s)))

    # views
    def kernel(self, l):
        i, o = self.dims[l]
        return self._region(0, self.w_off[l], i * o).view(i, o)

    def bias(self, l):
        return self._region(0, self.b_off[l], self.dims[l][1])

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

    _step = _CircuitCore._launch_step   # (table_dev, B, beta, row_idx=None)

    def train_step(self, truth_table, beta: float, batch_size: int = 512, row_idx=None) -> torch.Tensor:
        """cell 6 train_step: one batch drawn from the truth table ([2^G, G + 1] 0/1 rows), BCE + beta sum_g KL_g, Keras Adam.
        Returns the batch's mean BCE (nats) as a fresh device scalar, without synchronising.  row_idx ([B] ints): use these
        rows instead of the device draw."""
        B = int(batch_size) if row_idx is None else int(len(row_idx))
        self._check_batch(B)
        table = self._table(truth_table)
        ri = self._row_idx(row_idx) if row_idx is not None else None
        bf = self._launch_step(table, B, beta, ri)
        o = bf["off"]["sums3"] + 2                     # (_bce(bf)[0] with fewer torch calls: this call is host-bound)
        return bf["ws"][o: o + 1].clone()[0]

    def last_step(self, batch_size: int) -> dict:
        """device views of the last step at this batch size: rows [B], u [B, 16], y [B], pred [B] (logits), g_u [B, 16], kl [G + 1]"""
        return self._last_step(0, int(batch_size))

    # ---- information of the channels ---------------------------------------------------------------
    def estimate_channel_mi_bounds(self, seed: int = 0, evaluation_batch_size: int = 1024, number_evaluation_batches: int = 8,
                                   per_batch: bool = False) -> np.ndarray:
        """cell 6's estimate_mi_sandwich_bounds(feature_encoder, [[-1.], [1]]) for every gate at once: [G, 2] (lower, upper) in
        nats, the mean over the batches ([G, nb, 2] with per_batch).  The inputs of each batch are drawn by the seeded NumPy rule
        of utils.estimate_mi_sandwich_bounds for a 2-row dataset; one dib_circuit_mi_bounds launch."""
        return self._mi_bounds([int(seed)], int(evaluation_batch_size), int(number_evaluation_batches), per_batch)[0]

    # ---- training loop -----------------------------------------------------------------------
    def fit(self, truth_table, number_training_steps: int = 50_000, batch_size: int = 512, learning_rate: float = 1e-3,
            beta_start: float = 1e-3, beta_end: float = 5.0, evaluate_mutual_info_freq: Optional[int] = None,
            seed: int = 0) -> dict:
        """cell 6's loop: for every step assign beta (log-linear ramp), train one batch, and where step % freq == 0 (step 0
        included) estimate every channel's sandwich bounds (seed evaluation_seed(seed, step)).  Returns bce_loss_series [n]
        (nats), beta [n], mutual_information_bounds [n_eval, G, 2] (bits) and evaluation_steps.  The host synchronises only at
        evaluations."""
        self._check_batch(int(batch_size))
        return self._fit(self._table(truth_table), int(number_training_steps), int(batch_size), learning_rate, [beta_start],
                         [beta_end], evaluate_mutual_info_freq, [seed])[0]


class CircuitEnsemble(_CircuitCore):
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
    step number; one learning rate and one Adam step count are shared.  params, grads, m and v are replica-major, each replica
    laid out like CircuitIB's flat buffer."""

    def __init__(self, truth_tables, predictive_arch_spec=(256, 256, 256), activation_function: str = "leaky_relu",
                 init_seeds: Optional[Sequence[int]] = None, noise_seeds: Optional[Sequence[int]] = None, device="cuda:0"):
        tables = [np.asarray(t) for t in truth_tables]
        R = len(tables)
        if R < 1:
            raise ValueError("a CircuitEnsemble takes at least one truth table (R >= 1)")
        init_seeds = [int(s) for s in init_seeds] if init_seeds is not None else list(range(R))
        noise_seeds = [int(s) for s in noise_seeds] if noise_seeds is not None else list(range(R))
        if len(init_seeds) != R or len(noise_seeds) != R:
            raise ValueError(f"init_seeds and noise_seeds take one seed per replica ({R})")
        words = [pack_truth_table(t) for t in tables]          # ValueError unless [2^G, G + 1] 0/1 rows, 1 <= G <= 16
        self.tables = tables
        self._setup([t.shape[1] - 1 for t in tables], predictive_arch_spec, activation_function, init_seeds, noise_seeds, device,
                    batched=True)
        self.G = self.gates
        offs = np.concatenate([[0], np.cumsum([w.shape[0] for w in words])])
        self._tables_dev = torch.from_numpy(np.concatenate(words).view(np.int32)).to(self.device)
        self._table_words = int(offs[-1])
        self._table_off_c = (ctypes.c_int64 * R)(*[int(o) for o in offs[:-1]])

    def _step(self, B: int, betas: Sequence[float], row_idx: Optional[torch.Tensor] = None) -> dict:
        return self._launch_step(None, B, betas, row_idx)

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
            ri = self._row_idx(ri)
        return self._bce(self._launch_step(None, B, betas, ri)).clone()

    def last_step(self, r: int, batch_size: int) -> dict:
        """device views of replica r's last step at this batch size, with the keys of CircuitIB.last_step"""
        return self._last_step(self._replica(r), int(batch_size))

    # ---- information of the channels ---------------------------------------------------------------
    def estimate_channel_mi_bounds(self, seeds: Optional[Sequence[int]] = None, evaluation_batch_size: int = 1024,
                                   number_evaluation_batches: int = 8, per_batch: bool = False) -> List[np.ndarray]:
        """CircuitIB.estimate_channel_mi_bounds(seeds[r], ...) of every replica (default seeds 0..R-1) in ONE
        dib_circuit_mi_bounds_batched launch and one read-back: a list of [G_r, 2] arrays (nats; [G_r, nb, 2] with per_batch)"""
        return self._mi_bounds(_replica_seeds(seeds, self.R), int(evaluation_batch_size), int(number_evaluation_batches), per_batch)

    # ---- training loop -----------------------------------------------------------------------
    def fit(self, number_training_steps: int = 50_000, batch_size: int = 512, learning_rate: float = 1e-3, beta_start=1e-3,
            beta_end=5.0, evaluate_mutual_info_freq: Optional[int] = None, seeds: Optional[Sequence[int]] = None) -> List[dict]:
        """CircuitIB.fit for every replica at once: each replica ramps beta on beta_schedule between its own beta_start and
        beta_end (scalars, or one per replica), and where step % freq == 0 all replicas' bounds come from one launch, replica r
        with the inputs and noise key of CircuitIB.fit(seed=seeds[r]) (default seeds 0..R-1).  Returns one history per replica
        with the keys of CircuitIB.fit.  The host synchronises only at evaluations."""
        b0, b1 = _per_replica(beta_start, self.R, "beta_start"), _per_replica(beta_end, self.R, "beta_end")
        seeds = _replica_seeds(seeds, self.R)
        self._check_batch(int(batch_size))
        return self._fit(None, int(number_training_steps), int(batch_size), learning_rate, b0, b1, evaluate_mutual_info_freq, seeds)

    # ---- access to replicas ------------------------------------------------------------------
    def replica_params(self, r: int) -> torch.Tensor:
        """replica r's slice [n_params] of the live parameter buffer (CircuitIB's layout)"""
        return self._region(r, 0, self.n_params)

    def get_weights(self, r: int) -> dict:
        """replica r: {"predictive_model": Keras-ordered [kernel, bias] per layer (the first kernel [G_r, width]),
        "mu_scaling": [G_r], "logvar": [G_r]}"""
        G = self.G[self._replica(r)]
        return {"predictive_model": self._predictor_weights(r), "mu_scaling": self._read(r, self.sc_off, G),
                "logvar": self._read(r, self.sc_off + G, G)}

    def set_weights(self, r: int, weights: dict) -> None:
        """the counterpart of get_weights: any subset of its keys"""
        G = self.G[self._replica(r)]
        if "predictive_model" in weights:
            self._set_predictor_weights(r, weights["predictive_model"])
        if "mu_scaling" in weights:
            self._write(r, self.sc_off, weights["mu_scaling"], G)
        if "logvar" in weights:
            self._write(r, self.sc_off + G, weights["logvar"], G)

    def to_model(self, r: int) -> CircuitIB:
        """a CircuitIB holding replica r's parameters and Adam state (moments, step count, learning rate) at the current step:
        trained on with the same beta and rows it takes the ensemble's replica r's next step, bit for bit"""
        r = self._replica(r)
        m = CircuitIB(self.G[r], self.units, self.activation_function, noise_seed=self.noise_seeds[r], init_seed=self.init_seeds[r],
                      device=self.device)
        sl = slice(r * self.n_params, (r + 1) * self.n_params)
        m.params.copy_(self.params[sl])
        m.grads.copy_(self.grads[sl])
        m.opt_state.take_state(self.opt_state, sl)
        m.step = self.step
        return m
