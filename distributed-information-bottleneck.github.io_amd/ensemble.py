"""DistributedIBEnsemble: R DistributedIBNet models of ONE architecture trained in lockstep - seeds for error bars on an
information plane, or several beta ramps - sharing every launch of a step.

Replica r is DistributedIBNet(..., init_seed=init_seeds[r], noise_seed=noise_seeds[r], shuffle_seed=shuffle_seeds[r]): its
initial weights, its epoch permutations (_fit.epoch_order's rule), its noise (seed_r, step, dataset row, feature, dim) and its
beta ramp (InfoBottleneckAnnealingCallback's float32 values).  The step counter, the learning rate and Adam's step count are
shared.

One flat buffer holds params | grads | m | v.  All R F encoder chains come first, one stride apart (chain g = r F + f), then
the R integration chains, one stride apart: the encoder bank is ONE dense.chain_plan of R F groups and the integration
networks ONE of R groups, so every Dense layer - forward and dgrad - is one dib_gemm_grouped launch whatever R and F are.
A step (include/dib_ensemble.h for the new entries):
    dib_ens_posenc_rows        batch gather + positional encoding of every (replica, feature)
    dib_gemm_grouped           encoder layers forward                                    one launch per layer, R F groups
    dib_ens_reparam_kl_fwd     u straight into the integration plan's input, KL sums [R][F]
    dib_gemm_grouped           integration layers forward                                one launch per layer, R groups
    dib_ens_loss               task loss, dL/dpred, the History sums of every replica
    dib_gemm_grouped           integration dgrad chain, then g_u = g1 W0^T (mode 1, no activation mask, R groups)
    dib_ens_reparam_kl_bwd     dL/d(mu | logvar) into the encoder plan's last gradient region
    dib_gemm_grouped           encoder dgrad chain; every weight gradient of each network in one launch, into batch slabs
    dib_reduce_splits, dib_adam_step   over all R P parameters
That one replica's weights are not contiguous is hidden by get_flat_weights / set_flat_weights / to_model, which speak the
SINGLE model's flat layout (param_blocks() order).  There is no CPU path: the class needs a GPU and libdib_hip.so.

Out of scope (ValueError before any launch): ragged feature_dimensionalities (one chain plan serves all R F encoders), replicas
of different architectures, data parallelism under an initialised torch.distributed, Keras callbacks inside the lockstep fit,
hipGraph capture."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _fit
from . import losses as _losses
from . import optimizers as _optimizers
from ._flat_optimizer import FlatOptimizer, HoldsFlatOptimizer
from ._gemm_plan import _Gemm, _d, _ptr, slab_rule
from ._host import Carver
from ._lib import ACTIVATIONS, LOSS_KINDS, check
from .dense import chain_plan
from .models import DistributedIBNet, History, InfoBottleneckAnnealingCallback

LOSSES = ("bce_logits", "sparse_cce_logits", "mse")   # kinds 0, 2 and 3 of dib_loss_kernel: the reference's own three
_SPEC = ("feature_dimensionalities", "feature_encoder_architecture", "integration_network_architecture", "output_dimensionality",
         "use_positional_encoding", "number_positional_encoding_frequencies", "activation_fn", "feature_embedding_dimension",
         "output_activation_fn")


def _per_replica(value, R: int, what: str, cast=float) -> list:
    """a scalar for every replica, or one entry per replica"""
    if np.ndim(value) == 0:
        return [cast(value)] * R
    vals = [cast(v) for v in value]
    if len(vals) != R:
        raise ValueError(f"{what} takes a scalar or one value per replica ({R}); got {len(vals)}")
    return vals


def _seeds(seeds, base: int, R: int, what: str) -> List[int]:
    out = [int(s) for s in seeds] if seeds is not None else [int(base) + r for r in range(R)]
    if len(out) != R:
        raise ValueError(f"{what} takes one seed per replica ({R}); got {len(out)}")
    return out


def beta_ramps(beta_start, beta_end, number_pretraining_epochs: int, number_annealing_epochs: int, epochs: int, R: int) -> np.ndarray:
    """float32 [R, epochs]: the beta InfoBottleneckAnnealingCallback(beta_start[r], beta_end[r], n_pre, n_anneal) assigns at the
    start of every epoch, bit for bit (its own beta_at).  number_annealing_epochs == 0 is no ramp: beta_start up to the end of
    the pretraining epochs, beta_end after them."""
    b0, b1 = _per_replica(beta_start, R, "beta_start"), _per_replica(beta_end, R, "beta_end")
    if any(not (b > 0.0 and math.isfinite(b)) for b in b0 + b1):
        raise ValueError("beta_start and beta_end must be positive and finite (the ramp is logarithmic)")
    n_pre, n_anneal = int(number_pretraining_epochs), int(number_annealing_epochs)
    if n_pre < 0 or n_anneal < 0:
        raise ValueError("number_pretraining_epochs and number_annealing_epochs must not be negative")
    out = np.zeros((R, int(epochs)), dtype=np.float32)
    for r in range(R):
        cb = InfoBottleneckAnnealingCallback(b0[r], b1[r], n_pre, n_anneal)
        for e in range(int(epochs)):
            out[r, e] = cb.beta_at(e) if n_anneal > 0 else np.float32(b0[r] if e <= n_pre else b1[r])
    return out


def _chain_offsets(dims):
    """(w_off, b_off, size) of one layer chain in the flat buffer: DenseStack's rule, every block on a multiple of 4 floats"""
    off, w_off, b_off = 0, [], []
    for i, o in dims:
        w_off.append(off); off += (i * o + 3) // 4 * 4
        b_off.append(off); off += (o + 3) // 4 * 4
    return w_off, b_off, off


class EnsembleLayout:
    """Where every parameter of every replica sits: the ensemble's flat layout and the map from the single model's.  Host
    arithmetic only - `blocks` is DistributedIBNet.param_blocks() (or the library's dib_layout_param_block answers)."""

    def __init__(self, blocks: Sequence[dict], n_single: int, R: int, F: int, d: int, n_blocks: int, enc_units: Sequence[int], E: int,
                 int_units: Sequence[int], out_dim: int):
        self.R, self.F, self.n_single = int(R), int(F), int(n_single)
        ew = [d * n_blocks] + [int(u) for u in enc_units] + [2 * E]
        iw = [F * E] + [int(u) for u in int_units] + [int(out_dim)]
        self.enc_dims, self.int_dims = list(zip(ew[:-1], ew[1:])), list(zip(iw[:-1], iw[1:]))
        self.enc_w, self.enc_b, self.enc_stride = _chain_offsets(self.enc_dims)
        self.int_w, self.int_b, self.int_stride = _chain_offsets(self.int_dims)
        self.int_base = R * F * self.enc_stride
        self.n_params = self.int_base + R * self.int_stride      # what the optimizer runs over
        self.pad = self.n_params                                 # one always-zero element: where the single layout's gaps map to
        self.n_alloc = self.n_params + 4
        # single-layout position -> ensemble position of replica 0; replica r adds its strides
        idx = np.full(self.n_single, -1, dtype=np.int64)
        enc_part = np.zeros(self.n_single, dtype=bool)
        for b in blocks:
            n, l = b["rows"] * b["cols"], b["layer"]
            want = (self.enc_dims if b["net"] == 0 else self.int_dims)[l]
            if n != (want[0] * want[1] if b["what"] == 0 else want[1]):
                raise ValueError(f"block {b} of the single layout does not fit the ensemble's layer {want}")
            if b["net"] == 0:
                base = b["feature"] * self.enc_stride + (self.enc_w[l] if b["what"] == 0 else self.enc_b[l])
                enc_part[b["offset"]: b["offset"] + n] = True
            else:
                base = self.int_base + (self.int_w[l] if b["what"] == 0 else self.int_b[l])
            idx[b["offset"]: b["offset"] + n] = base + np.arange(n)
        self._idx0, self._enc_part = idx, enc_part

    def index(self, r: int) -> np.ndarray:
        """int64 [n_single]: the ensemble position of every element of the single model's flat buffer for replica r (the gaps
        of the single layout map to `pad`, which always holds 0)"""
        if not 0 <= int(r) < self.R:
            raise IndexError(f"replica {r} of {self.R}")
        shift = np.where(self._enc_part, r * self.F * self.enc_stride, r * self.int_stride)
        return np.where(self._idx0 >= 0, self._idx0 + shift, self.pad)


def single_blocks(**spec):
    """(param_blocks(), allocated floats) of the single model's flat layout, asked of the library on the host: no device"""
    from ctypes import byref, c_int, c_int64, c_void_p
    from . import _lib
    lib = _lib.load_library()
    dims, enc, units = ([int(v) for v in spec[k]] for k in _SPEC[:3])
    ci = lambda xs: (c_int * max(1, len(xs)))(*xs)
    h = c_void_p()
    check(lib.dib_layout_create(len(dims), ci(dims), len(enc), ci(enc), int(spec["feature_embedding_dimension"]), len(units), ci(units),
                                int(spec["output_dimensionality"]), 1 if spec.get("use_positional_encoding", True) else 0,
                                int(spec.get("number_positional_encoding_frequencies", 5)), ACTIVATIONS[spec.get("activation_fn", "relu")],
                                ACTIVATIONS[spec.get("output_activation_fn")], byref(h)), "dib_layout_create")
    try:
        out, off, rows, cols = [], c_int64(), c_int(), c_int()
        for net, nl in ((0, len(enc) + 1), (1, len(units) + 1)):
            for layer in range(nl):
                for f in (range(len(dims)) if net == 0 else [0]):
                    for what in (0, 1):
                        check(lib.dib_layout_param_block(h, net, layer, f, what, byref(off), byref(rows), byref(cols)), "param_block")
                        out.append(dict(net=net, layer=layer, feature=f, what=what, offset=off.value, rows=rows.value, cols=cols.value))
        return out, (int(lib.dib_layout_param_count(h)) + 3) // 4 * 4
    finally:
        lib.dib_layout_destroy(h)


class DistributedIBEnsemble(HoldsFlatOptimizer):
    def __init__(self, replicas, feature_dimensionalities, feature_encoder_architecture, integration_network_architecture,
                 output_dimensionality, use_positional_encoding=True, number_positional_encoding_frequencies=5, activation_fn='relu',
                 feature_embedding_dimension=32, output_activation_fn=None, *, init_seeds: Optional[Sequence[int]] = None,
                 noise_seeds: Optional[Sequence[int]] = None, shuffle_seeds: Optional[Sequence[int]] = None, init_seed: int = 0,
                 noise_seed: int = 0, shuffle_seed: int = 0, device: Optional[str] = None):
        R = int(replicas)
        if R < 1:
            raise ValueError("a DistributedIBEnsemble takes replicas >= 1")
        self.init_seeds = _seeds(init_seeds, init_seed, R, "init_seeds")
        self.noise_seeds = _seeds(noise_seeds, noise_seed, R, "noise_seeds")
        self.shuffle_seeds = _seeds(shuffle_seeds, shuffle_seed, R, "shuffle_seeds")
        dims = [int(v) for v in feature_dimensionalities]
        if not dims or len(set(dims)) != 1:
            raise ValueError(f"feature_dimensionalities {dims}: a DistributedIBEnsemble needs every feature of the same width (one "
                             "chain plan serves all R F encoders); ragged features train as single DistributedIBNet models")
        activation_fn = activation_fn if activation_fn not in ("None", "") else None
        self._spec = dict(zip(_SPEC, (dims, [int(u) for u in feature_encoder_architecture],
                                      [int(u) for u in integration_network_architecture], int(output_dimensionality),
                                      bool(use_positional_encoding), int(number_positional_encoding_frequencies), activation_fn,
                                      int(feature_embedding_dimension), output_activation_fn)))
        self.R, self.F, self.d, self.E = R, len(dims), dims[0], int(feature_embedding_dimension)
        self.number_features, self.out_dim = self.F, int(output_dimensionality)
        self.n_blocks = int(number_positional_encoding_frequencies) if use_positional_encoding else 1
        if self.n_blocks < 1:
            raise ValueError("number_positional_encoding_frequencies >= 1")
        self._device_arg = device
        self.optimizer = self.loss = None
        self.metrics_names: List[str] = []
        self._step = 0
        self._built = False

    # ---- device state ------------------------------------------------------------------------
    def _build(self) -> None:
        """the envelope question (host only), the template engine (it validates the arguments), then the allocations"""
        if self._built:
            return
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            raise ValueError("DistributedIBEnsemble does not train data-parallel: under an initialised torch.distributed every rank "
                             "would train the same replicas; give each rank its own ensemble of other seeds")
        from . import _lib
        from .engine import HipEngine
        R, F, E = self.R, self.F, self.E
        if not _lib.load_library().dib_ens_supported(R, F, E, 1, self.out_dim, 0):
            raise ValueError(f"DistributedIBEnsemble(replicas={R}, features={F}, embedding={E}, outputs={self.out_dim}) is outside "
                             "the envelope of include/dib_ensemble.h")
        eng = self._template = HipEngine(**self._spec, device=self._device_arg, init_seed=self.init_seeds[0])
        self.lib, self.device, self._stream = eng.lib, eng.device, eng._stream
        self.act, self.out_act = ACTIVATIONS[self._spec["activation_fn"]], ACTIVATIONS[self._spec["output_activation_fn"]]
        lay = self.layout = EnsembleLayout(eng.blocks, eng.params.numel(), R, F, self.d, self.n_blocks,
                                           self._spec["feature_encoder_architecture"], E,
                                           self._spec["integration_network_architecture"], self.out_dim)
        S = lay.n_alloc
        flat = self._flat = torch.zeros(4 * S, dtype=torch.float32, device=self.device)
        self.params, self.grads, m, v = (flat[i * S: (i + 1) * S] for i in range(4))
        self.opt_state = FlatOptimizer(self.lib, self._stream, S, self.device, m=m, v=v)
        self._index = [torch.from_numpy(lay.index(r)).to(self.device) for r in range(R)]
        for r in range(R):
            self._scatter(self.params, r, eng.glorot_uniform(self.init_seeds[r]))
        # uint64 keys as the single model passes them (seed mod 2^64), held in an int64 tensor of the same bits
        u64 = [s & (2 ** 64 - 1) for s in self.noise_seeds]
        self.seeds_dev = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in u64], dtype=torch.int64, device=self.device)
        self.beta_dev = torch.ones(R, dtype=torch.float32, device=self.device)
        self._beta_host = np.ones(R, dtype=np.float32)
        self._metrics2 = torch.zeros(2, R, F + 3, dtype=torch.float32, device=self.device)   # training | validation History sums
        self.metrics_acc, self.metrics_acc_val = self._metrics2[0], self._metrics2[1]
        self._plans: Dict[int, dict] = {}
        self._x = self._y = None
        self._built = True

    def _scatter(self, buf: torch.Tensor, r: int, flat_single) -> None:
        """buf[ensemble positions of replica r] <- a vector in the single model's layout (its gaps are dropped)"""
        src = np.zeros(self.layout.n_single, dtype=np.float32)
        flat_single = np.asarray(flat_single, dtype=np.float32).reshape(-1)
        k = min(len(src), len(flat_single))
        src[:k] = flat_single[:k]
        idx = self.layout.index(r)
        keep = idx != self.layout.pad
        buf[torch.from_numpy(idx[keep]).to(self.device)] = torch.from_numpy(src[keep]).to(self.device)

    def _replica(self, r: int) -> int:
        if not 0 <= int(r) < self.R:
            raise IndexError(f"replica {r} of {self.R}")
        return int(r)

    def get_flat_weights(self, r: int) -> np.ndarray:
        """replica r's parameters in the SINGLE model's flat layout (DistributedIBNet.get_flat_weights)"""
        self._build()
        return self.params[self._index[self._replica(r)]].cpu().numpy()

    def get_flat_grads(self, r: int) -> np.ndarray:
        """replica r's gradients of the last step, in the single model's flat layout"""
        self._build()
        return self.grads[self._index[self._replica(r)]].cpu().numpy()

    def set_flat_weights(self, r: int, flat) -> None:
        self._build()
        self._scatter(self.params, self._replica(r), flat)

    def param_blocks(self):
        """DistributedIBNet.param_blocks(): the single model's flat layout, which the weight access of every replica speaks"""
        self._build()
        return self._template.blocks

    def count_params(self) -> int:
        self._build()
        return int(self._template.n_params)

    def set_beta(self, beta) -> None:
        """beta of every replica (a scalar, or one value per replica), on the device"""
        self._build()
        b = np.asarray(_per_replica(beta, self.R, "beta"), dtype=np.float32)
        if not np.array_equal(b, self._beta_host):
            self.beta_dev.copy_(torch.from_numpy(b))
            self._beta_host = b

    def set_data(self, x, y) -> None:
        """the dataset the steps gather from: x [N, F d], y [N, labels] (uploaded once)"""
        self._build()
        eng = self._template
        xd, y_np = _fit.device_rows(eng, x), _fit.host_rows(y)
        if xd.shape[1] != self.F * self.d:
            raise ValueError(f"x has {xd.shape[1]} columns, the model {self.F} features of {self.d}")
        if y_np.shape[0] != xd.shape[0]:
            raise ValueError("x and y differ in rows")
        self._check_labels(y_np)
        self._x, self._y, self._n_rows = xd, eng.to_device(y_np), int(xd.shape[0])

    def _check_labels(self, y_np: np.ndarray) -> None:
        """once per dataset, on the host: the label layout dib_ens_loss reads - one class index per row inside [0, out_dim) for
        the sparse loss (the kernel indexes the prediction with it), out_dim columns for the others"""
        kind = self._kind()
        if kind == "sparse_cce_logits":
            if y_np.shape[1] < 1 or (y_np.size and (y_np[:, 0].min() < 0 or y_np[:, 0].max() >= self.out_dim
                                                     or np.any(y_np[:, 0] != np.floor(y_np[:, 0])))):
                raise ValueError(f"SparseCategoricalCrossentropy needs one class index in [0, {self.out_dim}) per row")
        elif y_np.shape[1] < self.out_dim:
            raise ValueError(f"loss {kind!r} reads {self.out_dim} label column(s) per row, y is {tuple(y_np.shape)}")

    # ---- compile -----------------------------------------------------------------------------
    def compile(self, optimizer='adam', loss=None, metrics=None, **unknown):
        if unknown:
            raise ValueError(f"compile: unknown argument {sorted(unknown)[0]!r}")
        opt = _optimizers.get(optimizer)
        if opt.name != "adam" or not opt.native:
            raise ValueError(f"optimizer {getattr(opt, 'name', opt)!r}: the lockstep step applies Keras Adam (one dib_adam_step over all "
                             "replicas); other rules and AMSGrad train as single DistributedIBNet models")
        if opt.clip() is not None:
            raise ValueError("gradient clipping is not part of the lockstep step: clipnorm / clipvalue / global_clipnorm need a "
                             "variable table per replica")
        if opt.lr_schedule() is not None:
            raise ValueError("the lockstep step runs at a constant learning rate: decay and schedules are not supported")
        ls = _losses.get(loss)
        if getattr(ls, "kind", None) not in LOSSES or not ls.legacy:
            raise ValueError(f"loss {ls!r}: the lockstep step takes BinaryCrossentropy(from_logits=True), "
                             "SparseCategoricalCrossentropy(from_logits=True) and 'mse' (kinds 0, 2, 3 of dib_loss_kernel)")
        if isinstance(metrics, str):
            metrics = [metrics]
        names = list(metrics or [])
        if names not in ([], ["accuracy"]):
            raise ValueError(f"metrics={names!r}: the lockstep step counts 'accuracy' (or nothing)")
        self.optimizer, self.loss, self.metrics_names = opt, ls, names
        return self

    def _kind(self) -> str:
        if self.loss is None:
            raise RuntimeError("call compile(optimizer=..., loss=...) first")
        return self.loss.kind

    # ---- one batch size's plan ---------------------------------------------------------------
    def _plan(self, n: int) -> dict:
        pl = self._plans.pop(n, None)
        if pl is None:
            R, F, E, lay, lib = self.R, self.F, self.E, self.layout, self.lib
            if not lib.dib_ens_supported(R, F, E, n, self.out_dim, LOSS_KINDS[self._kind()]):
                raise ValueError(f"a batch of {n} rows is outside the envelope of include/dib_ensemble.h (1 <= rows <= 2048)")
            ce, ci = Carver(4), Carver(4)
            enc_ws, enc_g, enc_wgrad = chain_plan(lay.enc_dims, lay.enc_w, lay.enc_b, self.act, n, self.params, self.device, ce,
                                                  R * F, lay.enc_stride, 0)
            ci.take("gu", R * n * F * E)
            int_ws, int_g, int_wgrad = chain_plan(lay.int_dims, lay.int_w, lay.int_b, self.act, n, self.params, self.device, ci,
                                                  R, lay.int_stride, lay.int_base)
            Li = len(lay.int_dims)
            int_g[f"fwd{Li - 1}"].act = self.out_act      # the output activation (chain_plan leaves the last layer linear)
            w1, FE, io = lay.int_dims[0][1], F * E, ci.off
            # the one product chain_plan does not make: g_u = g1 W0^T, no activation mask (u is not an activation's output)
            gu = _Gemm(1, [_d(io["g1"] + r * n * w1, w1, lay.int_base + r * lay.int_stride + lay.int_w[0], w1,
                              io["gu"] + r * n * FE, FE, n, FE, w1) for r in range(R)], int_ws, self.params, int_ws, act=0)
            gu.upload(self.device)
            nsplit, rps = slab_rule(n)
            S = lay.n_alloc
            slabs = torch.zeros(nsplit * S, dtype=torch.float32, device=self.device) if nsplit > 1 else None
            target = slabs if slabs is not None else self.grads
            wg = []
            for ws, descs in ((enc_ws, enc_wgrad), (int_ws, int_wgrad)):
                g = _Gemm(2, descs, ws, ws, target, bias_out=target, nsplit=nsplit, rows_per_split=rps, split_stride=S)
                g.upload(self.device)
                wg.append(g)
            need = int(lib.dib_ens_workspace_bytes(R, F, E, n))
            pl = dict(n=n, enc_ws=enc_ws, enc_off=ce.off, enc_g=enc_g, int_ws=int_ws, int_off=ci.off, int_g=int_g, gu=gu, wgrad=wg,
                      nsplit=nsplit, slabs=slabs, kl=torch.zeros(R, F, dtype=torch.float32, device=self.device),
                      ws=torch.zeros(need // 4, dtype=torch.float32, device=self.device))
            while len(self._plans) >= 4:   # train batch, its tail, validation batch, its tail
                self._plans.pop(next(iter(self._plans)))
        self._plans[n] = pl
        return pl

    def workspace_bytes(self, n: int) -> int:
        """device bytes of the plan of an n-row batch (activations, gradients, slabs, partials) and the flat buffer"""
        self._build()
        pl = self._plan(n)
        return 4 * sum(t.numel() for t in (pl["enc_ws"], pl["int_ws"], pl["kl"], pl["ws"], self._flat)
                       ) + (4 * pl["slabs"].numel() if pl["slabs"] is not None else 0)

    def _view(self, pl, net: str, name: str, groups: int, width: int) -> torch.Tensor:
        o = pl[net + "_off"][name]
        return pl[net + "_ws"][o: o + groups * pl["n"] * width].view(groups, pl["n"], width)

    # ---- the step ----------------------------------------------------------------------------
    def _forward(self, pl, rows: torch.Tensor, step: int, inv_b: float, acc: torch.Tensor, deterministic: bool = False) -> None:
        lib, st, R, F, E, n, lay = self.lib, self._stream(), self.R, self.F, self.E, pl["n"], self.layout
        x, y = self._x, self._y
        ep, ip = (lambda name: _ptr(pl["enc_ws"], pl["enc_off"][name])), (lambda name: _ptr(pl["int_ws"], pl["int_off"][name]))
        Le, Li = len(lay.enc_dims), len(lay.int_dims)
        check(lib.dib_ens_posenc_rows(_ptr(x), x.stride(0), _ptr(rows), R, F, self.d, self.n_blocks, n, ep("a0"), st),
              "dib_ens_posenc_rows")
        for l in range(Le):
            pl["enc_g"][f"fwd{l}"].run(lib, st)
        check(lib.dib_ens_reparam_kl_fwd(ep(f"a{Le}"), _ptr(rows), _ptr(self.seeds_dev), int(step) & 0xFFFFFFFF, 1 if deterministic else 0,
                                         R, F, E, n, ip("a0"), _ptr(pl["kl"]), _ptr(pl["ws"]), st), "dib_ens_reparam_kl_fwd")
        for l in range(Li):
            pl["int_g"][f"fwd{l}"].run(lib, st)
        check(lib.dib_ens_loss(LOSS_KINDS[self._kind()], ip(f"a{Li}"), self.out_dim, _ptr(y), y.stride(0), _ptr(rows), R, F, n,
                               float(inv_b), self.out_act, _ptr(self.beta_dev), _ptr(pl["kl"]), ip(f"g{Li}"), _ptr(acc),
                               _ptr(pl["ws"]), st), "dib_ens_loss")

    def _backward(self, pl, inv_b: float) -> None:
        lib, st, R, F, E, n, lay = self.lib, self._stream(), self.R, self.F, self.E, pl["n"], self.layout
        ep, ip = (lambda name: _ptr(pl["enc_ws"], pl["enc_off"][name])), (lambda name: _ptr(pl["int_ws"], pl["int_off"][name]))
        Le, Li = len(lay.enc_dims), len(lay.int_dims)
        if pl["slabs"] is None:
            self.grads.zero_()
        for l in reversed(range(1, Li)):
            pl["int_g"][f"dgrad{l}"].run(lib, st)
        pl["gu"].run(lib, st)
        check(lib.dib_ens_reparam_kl_bwd(ep(f"a{Le}"), ip("gu"), ip("a0"), _ptr(self.beta_dev), float(inv_b), R, F, E, n,
                                         ep(f"g{Le}"), st), "dib_ens_reparam_kl_bwd")
        for l in reversed(range(1, Le)):
            pl["enc_g"][f"dgrad{l}"].run(lib, st)
        for g in pl["wgrad"]:
            g.run(lib, st)
        if pl["slabs"] is not None:
            S = lay.n_alloc
            check(lib.dib_reduce_splits(_ptr(pl["slabs"]), S, pl["nsplit"], S, _ptr(self.grads), st), "dib_reduce_splits")

    def _rows(self, order_rows) -> torch.Tensor:
        rows = order_rows if isinstance(order_rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(order_rows, dtype=np.int32))
        rows = rows.to(device=self.device, dtype=torch.int32).contiguous()
        if rows.dim() != 2 or rows.shape[0] != self.R or rows.shape[1] < 1:
            raise ValueError(f"order_rows must be int32 [replicas = {self.R}, batch]")
        return rows

    def train_step(self, order_rows, beta=None, apply_optimizer: bool = True) -> None:
        """One lockstep step: replica r trains on the dataset rows order_rows[r] (set_data's x, y) with its noise at the shared
        step counter, which then advances as DistributedIBNet._step does.  order_rows: int32 [R, b], every entry a row of the
        dataset (checked on the host only when it arrives as a host array).  apply_optimizer=False leaves the gradients in
        `grads` (get_flat_grads) and the parameters as they were."""
        self._build()
        if self._x is None:
            raise RuntimeError("set_data(x, y) (or fit) before train_step")
        if not isinstance(order_rows, torch.Tensor):
            a = np.asarray(order_rows)
            if a.size and (a.min() < 0 or a.max() >= self._n_rows):
                raise ValueError("order_rows holds a row outside the dataset")
        rows = self._rows(order_rows)
        if beta is not None:
            self.set_beta(beta)
        self._train(rows, apply_optimizer)

    def _train(self, rows: torch.Tensor, apply_optimizer: bool = True) -> None:
        b = int(rows.shape[1])
        pl = self._plan(b)
        self._forward(pl, rows, self._step, 1.0 / b, self.metrics_acc)
        self._backward(pl, 1.0 / b)
        if apply_optimizer:
            opt = self.optimizer
            self.opt_state.set_lr(opt.learning_rate)
            self.opt_state.adam(self.params, self.grads, self.layout.n_params, opt.beta_1, opt.beta_2, opt.epsilon, stream=self._stream())
        self._step += 1

    def _evaluation_pass(self, xd, yd, bs: int, noise_step: int, acc: torch.Tensor, merge_rows: int = 1024) -> int:
        """_fit.evaluation_pass for every replica: the batches it forms (full batches merged up to merge_rows rows and counted
        one step each, a partial last batch a step of its own), one noise key per pass, the sums into `acc`"""
        keep = (self._x, self._y)
        self._x, self._y = xd, yd
        try:
            kmerge = max(1, min(merge_rows, 2048) // bs)
            n, s0, steps = int(xd.shape[0]), 0, 0
            while s0 < n:
                gb = min(bs, n - s0)
                nb = min(kmerge, (n - s0) // bs) if gb == bs else 1
                rows = torch.arange(s0, s0 + gb * nb, dtype=torch.int32, device=self.device).repeat(self.R, 1)
                self._forward(self._plan(gb * nb), rows, noise_step, 1.0 / gb, acc)
                steps += nb
                s0 += gb * nb
            return steps
        finally:
            self._x, self._y = keep

    def _epoch_logs(self, acc: np.ndarray, nsteps: int, prefix: str, beta: float) -> Dict[str, float]:
        """DistributedIBNet._epoch_logs: loss = row-weighted mean of task + beta sum KL, KL{f} and beta = unweighted means over steps"""
        F = self.F
        rows = max(float(acc[F + 2]), 1.0)
        logs = {prefix + "loss": float(acc[F]) / rows}
        if self.metrics_names:
            logs[prefix + "accuracy"] = float(acc[F + 1]) / rows
        for f in range(F):
            logs[f"{prefix}KL{f}"] = float(acc[f]) / max(nsteps, 1)
        logs[prefix + "beta"] = float(beta)
        return logs

    def _read_metrics(self) -> np.ndarray:
        """[2, R, F + 3]: the training and validation History sums in ONE read-back; both are cleared"""
        out = self._metrics2.cpu().numpy()
        self._metrics2.zero_()
        return out

    def fit(self, x, y, batch_size, epochs, validation_data=None, shuffle=True, beta_start=1., beta_end=1.,
            number_pretraining_epochs=0, number_annealing_epochs=0, verbose=0, callbacks=None) -> List[History]:
        """DistributedIBNet.fit for every replica at once: R History objects with its keys, units and accounting.  One upload of
        every replica's epoch permutation and ONE read-back per epoch."""
        if callbacks:
            raise ValueError("Keras callbacks do not run inside the lockstep fit: beta ramps are fit's own arguments; for the others "
                             "take a replica out with to_model(r)")
        if os.environ.get("DIB_ENABLE_GRAPHS", "0") == "1":
            raise ValueError("DIB_ENABLE_GRAPHS=1: the lockstep step is not captured as a hipGraph (DistributedIBNet.fit's switch); "
                             "unset it for the ensemble")
        if self.optimizer is None or self.loss is None:
            raise RuntimeError("call compile(optimizer=..., loss=...) before fit()")
        R, bs, epochs = self.R, int(batch_size), int(epochs)
        ramps = beta_ramps(beta_start, beta_end, number_pretraining_epochs, number_annealing_epochs, epochs, R)
        if bs < 1:
            raise ValueError("batch_size >= 1")
        self.set_data(x, y)
        n = self._n_rows
        xv = yv = None
        if validation_data is not None:
            xv, yv_np = _fit.device_rows(self._template, validation_data[0]), _fit.host_rows(validation_data[1])
            self._check_labels(yv_np)
            yv = self._template.to_device(yv_np)
        hists = [History() for _ in range(R)]
        for h in hists:
            h.model = self
        bounds = list(range(0, n, bs))
        nsteps = len(bounds)
        self._read_metrics()
        for epoch in range(epochs):
            self.set_beta(ramps[:, epoch])
            # every replica's permutation (_fit.epoch_order's rule), step-major: step s reads one contiguous [R, rows] block
            orders = [(np.random.default_rng([self.shuffle_seeds[r], epoch]).permutation(n) if shuffle else np.arange(n))
                      .astype(np.int32) for r in range(R)]
            blocks = np.concatenate([np.stack([o[s0: s0 + bs] for o in orders]).reshape(-1) for s0 in bounds])
            order_dev = torch.from_numpy(blocks).to(self.device)
            off = 0
            for s0 in bounds:
                gb = min(bs, n - s0)
                self._train(order_dev[off: off + R * gb].view(R, gb))
                off += R * gb
            vsteps = 0
            if xv is not None:
                vsteps = self._evaluation_pass(xv, yv, bs, (1 << 31) + epoch, self.metrics_acc_val)
            sums = self._read_metrics()
            for r in range(R):
                logs = self._epoch_logs(sums[0, r], nsteps, "", ramps[r, epoch])
                if xv is not None:
                    logs.update(self._epoch_logs(sums[1, r], vsteps, "val_", ramps[r, epoch]))
                for k, v in logs.items():
                    hists[r].history.setdefault(k, []).append(float(v))
                hists[r].epoch.append(epoch)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs} - loss: " + " ".join(f"{h.history['loss'][-1]:.4f}" for h in hists))
        return hists

    def evaluate(self, x, y, batch_size) -> List[Dict[str, float]]:
        """DistributedIBNet.evaluate for every replica (noise step 2^31 - 1): R dicts"""
        self._build()
        eng = self._template
        xd, y_np = _fit.device_rows(eng, x), _fit.host_rows(y)
        self._check_labels(y_np)
        self._read_metrics()
        steps = self._evaluation_pass(xd, eng.to_device(y_np), int(batch_size), (1 << 31) - 1, self.metrics_acc)
        sums = self._read_metrics()
        return [self._epoch_logs(sums[0, r], steps, "", self._beta_host[r]) for r in range(self.R)]

    # ---- a replica as a model ----------------------------------------------------------------
    def to_model(self, r: int) -> DistributedIBNet:
        """a DistributedIBNet with replica r's weights, seeds, step counter, beta, compile settings and Adam state (moments,
        step count, learning rate: FlatOptimizer.take_state): fit continues it, and information_per_feature,
        compression_matrices, predict and the callbacks apply to it unchanged"""
        self._build()
        r = self._replica(r)
        m = DistributedIBNet(**self._spec, noise_seed=self.noise_seeds[r], init_seed=self.init_seeds[r],
                             shuffle_seed=self.shuffle_seeds[r], device=str(self.device))
        eng = m._ensure_engine()
        eng.params.copy_(self.params[self._index[r]])
        eng.opt_state.take_state(self.opt_state, self._index[r])
        m._step = self._step
        m.beta.assign(self._beta_host[r])
        if self.optimizer is not None:
            opt = _optimizers.Adam(self.optimizer.learning_rate, self.optimizer.beta_1, self.optimizer.beta_2, self.optimizer.epsilon)
            m.compile(optimizer=opt, loss=self.loss, metrics=list(self.metrics_names))
        return m
