"""HipEngine: device state + launch sequencing of the Distributed-IB step on one MI355X.

PyTorch is used only as plumbing (device memory, streams, torch.distributed); every FLOP of the
path runs in libdib_hip.so (hand-written HIP for gfx950) through the C ABI in include/dib_hip.h.
There is no CPU / eager fallback: constructing a HipEngine without a GPU or without the library
raises.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import byref, c_int, c_int64, c_void_p
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._flat_optimizer import FlatOptimizer, HoldsFlatOptimizer
from ._lib import ACTIVATIONS, LOSS_KINDS, check
from .optimizers import Adam, as_optimizer
from .utils import mi_sandwich_rows


def _ptr(t: Optional[torch.Tensor]):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


class HipEngine(HoldsFlatOptimizer):
    """Owns the flat parameter / gradient / Adam buffers and the activation workspace.

    The architecture arguments mirror DistributedIBNet.__init__ (reference models.py:56-66).
    """

    def __init__(self, feature_dimensionalities: Sequence[int], feature_encoder_architecture: Sequence[int],
                 integration_network_architecture: Sequence[int], output_dimensionality: int,
                 use_positional_encoding: bool = True, number_positional_encoding_frequencies: int = 5,
                 activation_fn: Optional[str] = "relu", feature_embedding_dimension: int = 32,
                 output_activation_fn: Optional[str] = None, device: Optional[str] = None, init_seed: int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs an AMD GPU (torch.cuda.is_available() is False); "
                               "the Distributed-IB path has no CPU fallback")
        self.lib = _lib.load_library()
        if activation_fn not in ACTIVATIONS or output_activation_fn not in ACTIVATIONS:
            raise ValueError(f"unsupported activation {activation_fn!r}/{output_activation_fn!r}; "
                             f"supported: {sorted(k for k in ACTIVATIONS if isinstance(k, str))}")
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self.F = len(feature_dimensionalities)
        self.E = int(feature_embedding_dimension)
        self.dims = [int(d) for d in feature_dimensionalities]
        self.sum_d = sum(self.dims)
        self.out_dim = int(output_dimensionality)
        self.enc_units = [int(u) for u in feature_encoder_architecture]
        self.int_units = [int(u) for u in integration_network_architecture]
        ci = lambda xs: (c_int * max(1, len(xs)))(*xs)
        handle = c_void_p()
        check(self.lib.dib_layout_create(self.F, ci(self.dims), len(self.enc_units), ci(self.enc_units), self.E,
                                         len(self.int_units), ci(self.int_units), self.out_dim,
                                         1 if use_positional_encoding else 0,
                                         int(number_positional_encoding_frequencies), ACTIVATIONS[activation_fn],
                                         ACTIVATIONS[output_activation_fn], byref(handle)), "dib_layout_create")
        self.layout = handle
        self.n_params = int(self.lib.dib_layout_param_count(self.layout))
        n_alloc = (self.n_params + 3) // 4 * 4
        with torch.cuda.device(self.device):
            z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=self.device)
            self.params, self.grads = z(n_alloc), z(n_alloc)
            self.opt_state = FlatOptimizer(self.lib, self._stream, n_alloc, self.device)
            self.beta_dev = torch.ones(1, dtype=torch.float32, device=self.device)  # reference models.py:86
            # History accumulators: training | validation, one tensor (one device-to-host copy reads both: fit synchronises
            # once per epoch - the validation pass is enqueued behind the training steps without reading anything back)
            self._metrics_stride = (self.F + 3 + 3) // 4 * 4
            self._metrics2 = z(2 * self._metrics_stride)
            self.metrics_acc = self._metrics2[: self.F + 3]
            self.metrics_acc_val = self._metrics2[self._metrics_stride: self._metrics_stride + self.F + 3]
            tb = int(self.lib.dib_layout_table_bytes(self.layout))
            self._tables = torch.zeros(tb, dtype=torch.uint8, device=self.device)
            check(self.lib.dib_layout_upload_tables(self.layout, _ptr(self._tables), self._stream()),
                  "dib_layout_upload_tables")
            torch.cuda.synchronize(self.device)
        self._ws: Dict[int, torch.Tensor] = {}      # batch -> step workspace, insertion order = recency
        self._ws_pinned = set()                     # batch sizes whose workspace a captured graph points into
        self._ws_gen: Dict[int, int] = {}           # batch -> number of forwards that (re)wrote its activations
        self._scratch: Optional[torch.Tensor] = None
        self._eval_ws: Dict[int, torch.Tensor] = {}   # batch -> initialised workspace of the evaluation helpers (feature_information)
        self._fused_head: Dict[int, bool] = {}      # loss kind -> dib_output_head_fused_supported
        self._loss_descs: Dict[tuple, "_lib.LossDesc"] = {}   # losses.LossDescriptor -> its checked dib_loss_desc
        self._infonce_ws: Dict[int, torch.Tensor] = {}   # batch -> workspace of dib_infonce_fwd_bwd
        self._grad_transform = None                 # grad_transform(): made by the first clipped step
        self._part_segments: Dict[int, tuple] = {}  # gradient bucket -> its (first, number) of variable-table segments
        self._held_parts: List[int] = []            # global_clipnorm: buckets that have landed, held until the step's last
        self.step_dev: Optional[torch.Tensor] = None   # enable_step_counter(): the device-resident noise step
        self.blocks = self._query_blocks()
        self.set_flat_params(self.glorot_uniform(init_seed))

    # ---- plumbing -----------------------------------------------------------------------------
    def _stream(self):
        return c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    layout = None   # (until __init__ has made it: __del__ also runs on an engine whose __init__ raised)

    def __del__(self):
        try:
            if self.layout:
                self.lib.dib_layout_destroy(self.layout)
                self.layout = None
        except Exception:
            pass

    _WS_KEEP = 4  # unpinned step workspaces kept (train, tail, validation, validation tail)

    def workspace(self, batch: int) -> torch.Tensor:
        """Step workspace for `batch` rows: true LRU over the most recent batch sizes.  A workspace whose raw pointer
        is baked into a captured hipGraph is PINNED (capture_step_graph) and never evicted - freeing it would let the
        caching allocator hand the memory to another tensor while graph replays still write to it."""
        ws = self._ws.pop(batch, None)
        if ws is None:
            nbytes = int(self.lib.dib_workspace_bytes(self.layout, batch))
            if nbytes <= 0:
                raise _lib.DibError(f"dib_workspace_bytes({batch}) -> {nbytes}")
            # include/dib_hip.h contract: the split-batch gradient slabs that no launch writes must read as zero
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            check(self.lib.dib_workspace_init(self.layout, batch, _ptr(ws), self._stream()), "dib_workspace_init")
            unpinned = [b for b in self._ws if b not in self._ws_pinned]
            while len(unpinned) >= self._WS_KEEP:
                self._ws.pop(unpinned.pop(0))  # least recently used first
            self._ws_gen[batch] = self._ws_gen.get(batch, 0) + 1  # a fresh buffer holds nobody's activations
        self._ws[batch] = ws  # (re)insert at the most-recent end
        return ws

    def scratch(self, nbytes: int) -> torch.Tensor:
        """Grow-only scratch for the evaluation helpers (encode_feature, MI bounds): they never touch the step
        workspaces, so callbacks cannot evict or clobber a training workspace (or one a graph / autograd node owns)."""
        n = (int(nbytes) + 3) // 4
        if self._scratch is None or self._scratch.numel() < n:
            self._scratch = torch.empty(n, dtype=torch.float32, device=self.device)
        return self._scratch

    def ws_view(self, batch: int, which: int, numel: int) -> torch.Tensor:
        off = int(self.lib.dib_workspace_offset(self.layout, batch, which))
        if off < 0:
            raise _lib.DibError(f"dib_workspace_offset -> {off}")
        return self.workspace(batch)[off // 4: off // 4 + numel]

    def _query_blocks(self) -> List[dict]:
        out = []
        off, rows, cols = c_int64(), c_int(), c_int()
        for net, nl in ((0, len(self.enc_units) + 1), (1, len(self.int_units) + 1)):
            for layer in range(nl):
                for f in (range(self.F) if net == 0 else [0]):
                    for what in (0, 1):
                        check(self.lib.dib_layout_param_block(self.layout, net, layer, f, what, byref(off), byref(rows),
                                                              byref(cols)), "dib_layout_param_block")
                        out.append(dict(net=net, layer=layer, feature=f, what=what, offset=off.value, rows=rows.value,
                                        cols=cols.value))
        return out

    def glorot_uniform(self, seed: int) -> np.ndarray:
        """Keras Dense defaults: kernel U(+-sqrt(6/(in+out))), bias zeros."""
        rng = np.random.default_rng(seed)
        flat = np.zeros(self.params.numel(), dtype=np.float32)
        for b in self.blocks:
            if b["what"] == 0:
                lim = math.sqrt(6.0 / (b["rows"] + b["cols"]))
                n = b["rows"] * b["cols"]
                flat[b["offset"]: b["offset"] + n] = rng.uniform(-lim, lim, size=n).astype(np.float32)
        return flat

    def set_flat_params(self, flat: np.ndarray) -> None:
        flat = np.asarray(flat, dtype=np.float32).reshape(-1)
        buf = np.zeros(self.params.numel(), dtype=np.float32)
        buf[: min(len(flat), len(buf))] = flat[: len(buf)]
        self.params.copy_(torch.from_numpy(buf))

    def get_flat_params(self) -> np.ndarray:
        return self.params.detach().cpu().numpy().copy()

    def get_flat_grads(self) -> np.ndarray:
        return self.grads.detach().cpu().numpy().copy()

    def optimizer_step(self, opt, grad_scale: float = 1.0, transform: bool = True) -> None:
        """One update of the whole flat buffer from self.grads by any optimizers.Optimizer: Adam and momentum-free SGD through
        adam_step / sgd_step (their launches and bits), every other rule through dib_optimizer_step + dib_optimizer_advance.
        The optimizer's clip arguments transform self.grads first (transform=False: the caller already did, e.g. with a norm
        over several buffers)."""
        st = self.opt_state
        st.bind(opt)
        if transform and opt.clip() is not None:   # the rule then reads the transformed gradient, grad_scale folded in
            self.transform_gradients(opt, grad_scale)
            grad_scale = 1.0
        if not opt.native:
            st.step_range(opt, self.params, self.grads, 0, self.n_params, grad_scale)
            st.advance(opt)
        elif opt.name == "adam":
            self.adam_step(opt.beta_1, opt.beta_2, opt.epsilon, grad_scale)
        else:
            self.sgd_step(grad_scale)

    # ---- gradient clipping and learning-rate schedules (include/dib_grad_transform.h) ------------------------------------------
    def grad_transform(self) -> "GradTransform":
        """the variable table of the layout on the device, the tile partials and the ss array: made once per engine"""
        if self._grad_transform is None:
            from .grad_transform import GradTransform
            host = _lib.HostGradTable.from_layout(self.layout, self.grads.numel())
            self._grad_transform = GradTransform(self.lib, host, self.grads, self._stream)
        return self._grad_transform

    def transform_gradients(self, opt, grad_scale: float = 1.0) -> None:
        """self.grads <- what the rule of `opt` sees (clipvalue, then clipnorm or global_clipnorm, grad_scale folded in), over the
        whole buffer: 1 launch for clipvalue alone, 3 with a norm.  Nothing for an optimizer without clip arguments."""
        clip = opt.clip()
        if clip is not None:
            self.grad_transform().transform(clip, None, grad_scale)

    def part_segments(self, part: int):
        """(first, number) of the variable-table segments of gradient bucket `part`: a bucket is a run of whole variables"""
        if part not in self._part_segments:
            self._part_segments[part] = self.grad_transform().host.segment_range(*self.part_range(part))
        return self._part_segments[part]

    def apply_lr(self, opt) -> None:
        """the learning rate of the next step: a constant through set_lr (nothing when unchanged); `decay` or a schedule through
        the one-thread kernel that reads the device step count, which then owns lr_dev"""
        d = opt.lr_schedule()
        if d is None:
            self.set_lr(opt.learning_rate)
        else:
            self.opt_state.eval_lr(d)

    def set_beta(self, v: float) -> None:
        self.beta_dev.fill_(float(v))

    def get_beta(self) -> float:
        return float(self.beta_dev.item())

    def to_device(self, a, dtype=torch.float32) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device=self.device, dtype=dtype).contiguous()

    # ---- the step -------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, row_idx: Optional[torch.Tensor], row0: int, batch: int, seed: int, step: int,
                deterministic: bool = False, inference: bool = False, hidden_only: bool = False,
                defer_sums: bool = False, companion=None) -> None:
        """reference models.py:96-123 -> ws[U], ws[PRED], KL local sums in ws[STEP_OUT].  inference=True: no backward
        follows (validation / predict), the fused forward skips the stashes it would write for it.  defer_sums=True: the KL
        column sums are left to the step's tail launch (step_tail with TAIL_KL).  companion: DenseStack.companion_forward(...)
        - the custom loop's output encoder runs in the integration network's grid (dib_integration_fwd_and_mlp_fwd)."""
        self.encoder_forward(x, row_idx, row0, batch, seed, step, deterministic, inference, defer_sums)
        ws, st = self.workspace(batch), self._stream()
        if companion is not None:
            assert not hidden_only
            check(self.lib.dib_integration_fwd_and_mlp_fwd(self.layout, batch, _ptr(self.params), _ptr(ws), *companion, st),
                  "dib_integration_fwd_and_mlp_fwd")
        elif hidden_only:  # the output layer is evaluated by the fused head together with the loss
            check(self.lib.dib_integration_fwd_hidden(self.layout, batch, _ptr(self.params), _ptr(ws), st),
                  "dib_integration_fwd_hidden")
        else:
            check(self.lib.dib_integration_fwd(self.layout, batch, _ptr(self.params), _ptr(ws), st), "dib_integration_fwd")

    def encoder_forward(self, x: torch.Tensor, row_idx: Optional[torch.Tensor], row0: int, batch: int, seed: int, step: int,
                        deterministic: bool = False, inference: bool = False, defer_sums: bool = False) -> None:
        """reference models.py:101-115 -> ws[ENC_OUT], ws[U], the KL partials (dib_encoder_bank_fwd)"""
        ws = self.workspace(batch)
        self._ws_gen[batch] += 1
        check(self.lib.dib_encoder_bank_fwd(self.layout, _ptr(x), x.stride(0), _ptr(row_idx), int(row0), batch,
                                            _ptr(self.params), int(seed), int(step) & 0xFFFFFFFF,
                                            (_lib.FWD_DETERMINISTIC if deterministic else 0) | (_lib.FWD_INFERENCE if inference else 0)
                                            | (_lib.FWD_DEFER_SUMS if defer_sums else 0), _ptr(ws), self._stream()),
              "dib_encoder_bank_fwd")

    def loss(self, loss_kind, y: torch.Tensor, row_idx, row0: int, batch: int, inv_global_batch: float,
             defer_sums: bool = False) -> None:
        """loss_kind: a name of LOSS_KINDS (dib_loss_fwd_bwd) or a losses.LossDescriptor (dib_loss_fwd_bwd_ex, the same workspace
        slots: the backward and the tail follow either unchanged)"""
        ws = self.workspace(batch)
        if not isinstance(loss_kind, str):
            desc = self._loss_desc(loss_kind)
            need = 1 if loss_kind.kind == "sparse_cce" else self.out_dim
            if y.dim() != 2 or y.shape[1] < need:
                raise ValueError(f"loss {loss_kind.kind!r} reads {need} label column(s) per row, y is {tuple(y.shape)}")
            check(self.lib.dib_loss_fwd_bwd_ex(self.layout, ctypes.byref(desc), _ptr(y), y.stride(0), _ptr(row_idx), int(row0), batch,
                                               float(inv_global_batch), _lib.HEAD_DEFER_SUMS if defer_sums else 0, _ptr(ws),
                                               self._stream()), "dib_loss_fwd_bwd_ex")
            return
        check(self.lib.dib_loss_fwd_bwd(self.layout, LOSS_KINDS[loss_kind], _ptr(y), y.stride(0), _ptr(row_idx),
                                        int(row0), batch, float(inv_global_batch), _lib.HEAD_DEFER_SUMS if defer_sums else 0,
                                        _ptr(ws), self._stream()),
              "dib_loss_fwd_bwd")

    def step_tail(self, batch: int, part: int, flags: int, inv_global_batch: float = 0.0, optimizer=None,
                  grad_scale: float = 1.0, metrics_acc: Optional[torch.Tensor] = None) -> None:
        """ONE launch for the end of a step (include/dib_hip.h dib_step_tail): any of bucket finalize, the fused head's
        weight-gradient reduce, KL / loss sums, metric accumulation, the optimizer on the bucket and the step-count bump.
        optimizer: an Adam or a momentum-free SGD (as_optimizer) - adds TAIL_ADAM / TAIL_SGD; clipping first is the caller's."""
        opt = None if optimizer is None else as_optimizer(optimizer)
        if opt is not None and not opt.native:
            raise ValueError(f"optimizer {opt.name!r}: the tail applies Adam and momentum-free SGD")
        adam = opt is not None and opt.name == "adam"
        b1, b2, eps = (opt.beta_1, opt.beta_2, opt.epsilon) if adam else (0.9, 0.999, 1e-7)
        flags |= 0 if opt is None else _lib.TAIL_ADAM if adam else _lib.TAIL_SGD
        st = self.opt_state
        check(self.lib.dib_step_tail(self.layout, batch, int(part), int(flags), _ptr(self.params), _ptr(self.grads),
                                     _ptr(st.m), _ptr(st.v), _ptr(st.lr_dev), _ptr(st.t_dev), b1, b2, eps,
                                     float(grad_scale), _ptr(self.beta_dev), float(inv_global_batch),
                                     _ptr(self.metrics_acc if metrics_acc is None else metrics_acc),
                                     _ptr(self.workspace(batch)), self._stream()), "dib_step_tail")

    def optimizer_step_part(self, batch: int, part: int, optimizer, bump: bool) -> None:
        """the optimizer on ONE gradient bucket (after its all-reduce): the data-parallel fit steps buckets 1 and 2 while
        bucket 3 is still on the wire; the launch with bump=True (the last) advances Adam's step count."""
        opt = as_optimizer(optimizer)
        clip = opt.clip()
        if clip is not None and clip[1] == _lib.CLIP_GLOBAL_NORM:
            # the norm is over every bucket: this one's sums of squares now, while later buckets are on the wire; all buckets
            # are transformed (one launch: together they are the whole table) and stepped after the last has landed
            gt, held = self.grad_transform(), self._held_parts
            gt.sumsq(clip, self.part_segments(part))
            held.append(part)
            if not bump:
                return
            assert sum(self.part_segments(p)[1] for p in held) == gt.n_segments, "the buckets of a step cover every variable"
            gt.apply(clip)
            parts = list(held)
            held.clear()
            for k, p in enumerate(parts):
                self._rule_on_part(batch, p, opt, bump=k == len(parts) - 1)
            return
        if clip is not None:   # clipvalue / clipnorm are per variable: the bucket is transformed as soon as it has landed
            self.grad_transform().transform(clip, self.part_segments(part))
        self._rule_on_part(batch, part, opt, bump)

    def _rule_on_part(self, batch: int, part: int, opt, bump: bool) -> None:
        """the rule of `opt` on one bucket whose gradient is final in self.grads; bump: the step's last launch of the rule"""
        if opt.native:   # Adam / momentum-free SGD: the tail's update on the bucket (dib_adam_step's expressions), no finalize
            self.step_tail(batch, part, _lib.TAIL_BUMP if (bump and opt.name == "adam") else 0, optimizer=opt)
            return
        off, cnt = self.part_range(part)
        self.opt_state.step_range(opt, self.params, self.grads, off, cnt)
        if bump:
            self.opt_state.advance(opt)

    def part_range(self, part: int):
        """(offset, count) of gradient bucket `part` in the flat buffers (include/dib_hip.h): 0 = encoder bank,
        1 = integration network, 2 = encoder layers before the last, 3 = last encoder layer (0 = 2 + 3)."""
        off, cnt = c_int64(), c_int64()
        check(self.lib.dib_layout_part_range(self.layout, part, byref(off), byref(cnt)), "dib_layout_part_range")
        return off.value, cnt.value

    def backward(self, row_idx, row0: int, batch: int, seed: int, step: int, inv_global_batch: float,
                 on_integration_grads_ready=None, hidden_only: bool = False, on_encoder_front_grads_ready=None,
                 finish_flags: int = 0, optimizer=None, integration_done: bool = False, companion=None,
                 metrics_acc: Optional[torch.Tensor] = None) -> None:
        """Backward pass, with the hooks of the data-parallel bucket protocol:
        `on_integration_grads_ready(grads_slice)` is called as soon as the integration network's gradients (bucket 1) are
        final - right after dib_integration_bwd - so their all-reduce runs under the whole encoder-bank backward;
        `on_encoder_front_grads_ready(grads_slice)` (three-bucket protocol, needs the first hook too) is called when the
        gradients of the encoder layers before the last (bucket 2) are final; the last layer's weight gradient (bucket 3)
        is computed after it, under that all-reduce, and is the only part left for the caller to reduce afterwards.
        Every bucket is finalised by ONE dib_step_tail launch; the LAST of them also carries `finish_flags` (the step's
        deferred KL / loss sums, the metric accumulation - into `metrics_acc`, default the model's History accumulator) and,
        without hooks, the optimizer (`optimizer`, see step_tail)."""
        opt = None if optimizer is None else as_optimizer(optimizer)
        bump = _lib.TAIL_BUMP if opt is not None and opt.name == "adam" else 0
        ws = self.workspace(batch)
        st = self._stream()
        FIN = _lib.TAIL_FINALIZE
        head = _lib.TAIL_HEAD_WGRAD if hidden_only else 0   # the fused head left its weight-gradient partials to the tail
        if on_integration_grads_ready is None and (integration_done or not hidden_only):
            # no bucket protocol: the rest of the backward pass in one entry - for small batches the dgrad chains are one
            # launch each and ALL weight gradients one grouped launch - then ONE tail launch
            assert on_encoder_front_grads_ready is None
            bflags = _lib.BWD_INTEGRATION_DONE if integration_done else 0
            if companion is not None:   # DenseStack.companion_backward(...): the output encoder's dgrad chain in the same grid
                check(self.lib.dib_backward_and_mlp_bwd(self.layout, batch, _ptr(self.params), _ptr(self.grads), _ptr(self.beta_dev),
                                                        float(inv_global_batch), bflags, _ptr(ws), *companion, st),
                      "dib_backward_and_mlp_bwd")
            else:
                check(self.lib.dib_backward(self.layout, batch, _ptr(self.params), _ptr(self.grads), _ptr(self.beta_dev),
                                            float(inv_global_batch), bflags, _ptr(ws), st), "dib_backward")
            self.step_tail(batch, -1, FIN | head | finish_flags | bump, inv_global_batch, optimizer=opt, metrics_acc=metrics_acc)
            return
        assert companion is None, "a companion pass rides on dib_backward (no bucket hooks)"
        if not integration_done:   # (dib_integration_head_step already ran the integration network's backward)
            fn = self.lib.dib_integration_bwd_hidden if hidden_only else self.lib.dib_integration_bwd
            check(fn(self.layout, batch, _ptr(self.params), _ptr(self.grads), _ptr(ws), st), "dib_integration_bwd")
        if on_integration_grads_ready is not None:
            assert opt is None, "the data-parallel caller steps the optimizer after its all-reduces"
            self.step_tail(batch, 1, FIN | head)
            off, cnt = self.part_range(1)
            on_integration_grads_ready(self.grads[off: off + cnt])
        # (row_idx / row0 / seed / step are not needed by the device backward: eps * sigma = ws[U] - mu)
        if on_encoder_front_grads_ready is not None:
            assert on_integration_grads_ready is not None, "the three-bucket protocol needs both hooks"
            for stage, part in ((1, 2), (2, 3)):
                check(self.lib.dib_encoder_bank_bwd_stage(self.layout, batch, _ptr(self.params), _ptr(self.grads),
                                                          _ptr(self.beta_dev), float(inv_global_batch), stage, _ptr(ws), st),
                      "dib_encoder_bank_bwd_stage")
                self.step_tail(batch, part, FIN | (finish_flags if stage == 2 else 0), inv_global_batch, metrics_acc=metrics_acc)
                if stage == 1:
                    off, cnt = self.part_range(2)
                    on_encoder_front_grads_ready(self.grads[off: off + cnt])
            return
        check(self.lib.dib_encoder_bank_bwd(self.layout, batch, _ptr(self.params), _ptr(self.grads),
                                            _ptr(self.beta_dev), float(inv_global_batch), _ptr(ws), st), "dib_encoder_bank_bwd")
        if on_integration_grads_ready is not None:
            self.step_tail(batch, 0, FIN | finish_flags, inv_global_batch, metrics_acc=metrics_acc)
        else:
            self.step_tail(batch, -1, FIN | head | finish_flags | bump, inv_global_batch, optimizer=opt, metrics_acc=metrics_acc)

    def input_grad(self, x: torch.Tensor, row_idx: Optional[torch.Tensor], row0: int, batch: int) -> torch.Tensor:
        """dL/dx [batch, sum_d] of the loss whose parameter gradients the last backward of this batch size wrote (include/dib_hip.h
        dib_encoder_bank_input_grad): call it after that backward, with the x / row_idx / row0 its training forward read.  Row b is
        batch position b (x row row_idx[b] or row0 + b)."""
        dx = torch.empty((batch, self.sum_d), dtype=torch.float32, device=self.device)
        check(self.lib.dib_encoder_bank_input_grad(self.layout, _ptr(x), x.stride(0), _ptr(row_idx), int(row0), batch,
                                                   _ptr(self.params), _ptr(self.workspace(batch)), _ptr(dx), dx.stride(0),
                                                   self._stream()), "dib_encoder_bank_input_grad")
        return dx

    def accumulate_metrics(self, batch: int, inv_global_batch: float) -> None:
        check(self.lib.dib_metrics_accumulate(self.layout, batch, _ptr(self.beta_dev), float(inv_global_batch),
                                              _ptr(self.metrics_acc), _ptr(self.workspace(batch)), self._stream()),
              "dib_metrics_accumulate")

    def _loss_desc(self, d) -> "_lib.LossDesc":
        """the dib_loss_desc of a losses.LossDescriptor (kept: a captured step holds its address until the launch is recorded);
        a descriptor the library does not take raises here, before anything is launched"""
        desc = self._loss_descs.get(d)
        if desc is None:
            desc = _lib.LossDesc(int(d.kind_id), int(d.metric_id), float(d.param))
            if not self.lib.dib_loss_ex_supported(ctypes.byref(desc), self.out_dim):
                raise ValueError(f"loss descriptor {d!r} is not supported for out_dim {self.out_dim} (include/dib_losses.h)")
            self._loss_descs[d] = desc
        return desc

    def _head_fused(self, kind) -> bool:
        if not isinstance(kind, int):
            # a descriptor never takes the fused one-unit head: its BCE-from-logits and MSE lines know neither a label smoothing
            # nor a metric beyond the 0.5-threshold count
            return False
        fused_head = self._fused_head.get(kind)
        if fused_head is None:
            fused_head = self._fused_head[kind] = bool(self.lib.dib_output_head_fused_supported(self.layout, kind))
        return fused_head

    def train_step(self, x, y, row_idx, row0: int, batch: int, seed: int, step: int, loss_kind: str,
                   inv_global_batch: Optional[float] = None, accumulate: bool = True,
                   on_integration_grads_ready=None, on_encoder_front_grads_ready=None, optimizer=None) -> None:
        """fwd + loss + bwd for the local rows; grads (partial sums over local rows / B_global) land in
        self.grads, ready for the data-parallel all-reduce(sum) and the optimizer step.  optimizer (single process only, anything
        as_optimizer takes): one that rides_in_tail is applied by the step's LAST launch, which also reduces the gradient
        partials, sums the KL / loss partials and accumulates the History metrics (csrc/dib_tail.h)."""
        optimizer = None if optimizer is None else as_optimizer(optimizer)
        if optimizer is not None and not optimizer.rides_in_tail:
            # the step ends with the tail WITHOUT an optimizer flag, then optimizer_step: the clip's launches, the rule's, its advance
            self.train_step(x, y, row_idx, row0, batch, seed, step, loss_kind, inv_global_batch, accumulate,
                            on_integration_grads_ready, on_encoder_front_grads_ready, None)
            self.optimizer_step(optimizer)
            return
        inv = 1.0 / batch if inv_global_batch is None else inv_global_batch
        kind = LOSS_KINDS[loss_kind] if isinstance(loss_kind, str) else loss_kind   # (a losses.LossDescriptor: dib_loss_fwd_bwd_ex)
        fused_head = self._head_fused(kind)
        finish = _lib.TAIL_KL | (_lib.TAIL_LOSS_HEAD if fused_head else _lib.TAIL_LOSS) | (_lib.TAIL_METRICS if accumulate else 0)
        if fused_head:
            # encoder bank, then the integration network's whole share in one entry: hidden layers, output Dense(1) + loss and
            # their backward down to dL/du (one launch of 16-row tiles in the row-tile regime), hidden weight gradients
            self.encoder_forward(x, row_idx, row0, batch, seed, step, defer_sums=True)
            single = on_integration_grads_ready is None   # no bucket protocol: every weight gradient of the step in dib_backward
            check(self.lib.dib_integration_head_step(self.layout, kind, _ptr(y), y.stride(0), _ptr(row_idx), int(row0), batch,
                                                     float(inv), _lib.HEAD_DEFER_SUMS | (_lib.HEAD_DEFER_WGRAD if single else 0),
                                                     _ptr(self.params), _ptr(self.grads),
                                                     _ptr(self.workspace(batch)), self._stream()), "dib_integration_head_step")
            self.backward(row_idx, row0, batch, seed, step, inv, on_integration_grads_ready, hidden_only=True,
                          on_encoder_front_grads_ready=on_encoder_front_grads_ready, finish_flags=finish, optimizer=optimizer,
                          integration_done=True)
            return
        self.forward(x, row_idx, row0, batch, seed, step, defer_sums=True)
        self.loss(loss_kind, y, row_idx, row0, batch, inv, defer_sums=True)
        self.backward(row_idx, row0, batch, seed, step, inv, on_integration_grads_ready, hidden_only=False,
                      on_encoder_front_grads_ready=on_encoder_front_grads_ready, finish_flags=finish, optimizer=optimizer)

    def eval_step(self, x, y, row_idx, row0: int, batch: int, seed: int, step: int, loss_kind: str,
                  inv_global_batch: Optional[float] = None, metrics_acc: Optional[torch.Tensor] = None) -> None:
        """validation: noise stays ON and the KL term is included (reference train.py:263-265).  metrics_acc: where the step's
        History sums go (default: the training accumulator; fit passes `metrics_acc_val`)."""
        inv = 1.0 / batch if inv_global_batch is None else inv_global_batch
        kind = LOSS_KINDS[loss_kind] if isinstance(loss_kind, str) else loss_kind   # (a losses.LossDescriptor: dib_loss_fwd_bwd_ex)
        fused_head = self._head_fused(kind)
        if fused_head:
            self.encoder_forward(x, row_idx, row0, batch, seed, step, inference=True, defer_sums=True)
            check(self.lib.dib_integration_head_step(self.layout, kind, _ptr(y), y.stride(0), _ptr(row_idx), int(row0), batch,
                                                     float(inv), _lib.HEAD_DEFER_SUMS | _lib.HEAD_NO_GRAD, _ptr(self.params), None,
                                                     _ptr(self.workspace(batch)), self._stream()), "dib_integration_head_step")
        else:
            self.forward(x, row_idx, row0, batch, seed, step, inference=True, defer_sums=True)
            self.loss(loss_kind, y, row_idx, row0, batch, inv, defer_sums=True)
        self.step_tail(batch, -1, _lib.TAIL_KL | (_lib.TAIL_LOSS_HEAD if fused_head else _lib.TAIL_LOSS) | _lib.TAIL_METRICS, inv,
                       metrics_acc=metrics_acc)

    # ---- hipGraph capture of a whole step (launch-bound small-batch regime) -----------------------
    def enable_step_counter(self, value: int = 0) -> None:
        """Key the noise with a DEVICE-resident step counter (dib_layout_set_step_counter) so that a captured step
        can be replayed; from now on the by-value `step` arguments are ignored by the kernels."""
        if self.step_dev is None:
            self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
            check(self.lib.dib_layout_set_step_counter(self.layout, _ptr(self.step_dev)), "dib_layout_set_step_counter")
        self.set_step_counter(value)

    def set_step_counter(self, value: int) -> None:
        v = int(value) & 0xFFFFFFFF
        self.step_dev.fill_(v - (1 << 32) if v >= (1 << 31) else v)  # uint32 bit pattern in an int32 tensor

    def capture_step_graph(self, x, y, batch: int, loss_kind: str, inv_global_batch: float, seed: int, train: bool,
                           optimizer=None):
        """Capture fwd + loss [+ bwd + optimizer] + metric accumulation + step-counter bump for `batch` rows whose
        dataset indices are read from a fixed staging buffer.  Returns (graph, idx_stage): copy the batch's int32 row
        indices into idx_stage, then graph.replay().  Everything the step reads that changes between replays (beta,
        lr, Adam t, noise step, row indices) lives in device memory.  optimizer: None (Adam()) or one that rides_in_tail."""
        opt = Adam() if optimizer is None else as_optimizer(optimizer)
        if not opt.rides_in_tail:
            raise ValueError(f"optimizer {opt.name!r} does not ride in the step's tail launch: its step is not captured")
        assert self.step_dev is not None, "call enable_step_counter() first"
        idx_stage = torch.zeros(batch, dtype=torch.int32, device=self.device)
        self.workspace(batch)
        self._ws_pinned.add(batch)  # the graph bakes this workspace's pointer in: never evict it
        # Eager warm-up with EXACTLY the launch sequence that is captured below (the fused output head, the hidden-only
        # integration passes, the optimizer and the counter bump included): every kernel's module load and every
        # hipFuncSetAttribute happens outside the capture.  All state the warm-up touches is restored afterwards.
        saved = [t.clone() for t in (self.metrics_acc, self.grads, self.params, self.adam_m, self.adam_v, self.t_dev,
                                     self.step_dev)]

        def body():
            if train:
                self.train_step(x, y, idx_stage, 0, batch, seed, 0, loss_kind, inv_global_batch, optimizer=opt)
            else:
                self.eval_step(x, y, idx_stage, 0, batch, seed, 0, loss_kind, inv_global_batch)
            self.step_dev.add_(1)

        def restore():
            for t, v in zip((self.metrics_acc, self.grads, self.params, self.adam_m, self.adam_v, self.t_dev, self.step_dev),
                            saved):
                t.copy_(v)

        body()
        restore()
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            body()
        restore()   # (capture does not execute, but keep the contract obvious: the caller's state is untouched)
        return graph, idx_stage

    def release_step_graph(self, batch: int) -> None:
        """The caller has dropped every graph captured for `batch` rows: its workspace may be evicted again (it re-enters
        the LRU as the most recent entry).  Without this, pinned workspaces accumulate for the lifetime of the engine."""
        self._ws_pinned.discard(batch)
        unpinned = [b for b in self._ws if b not in self._ws_pinned]
        while len(unpinned) > self._WS_KEEP:
            self._ws.pop(unpinned.pop(0))

    def adam_step(self, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0) -> None:
        self.opt_state.adam(self.params, self.grads, self.n_params, beta1, beta2, eps, grad_scale)

    def sgd_step(self, grad_scale=1.0) -> None:
        self.opt_state.sgd(self.params, self.grads, self.n_params, grad_scale)

    def read_metrics(self, reset: bool = True) -> np.ndarray:
        m = self.metrics_acc.detach().cpu().numpy().astype(np.float64)
        if reset:
            self.metrics_acc.zero_()
        return m

    def read_metrics_pair(self, reset: bool = True):
        """(training sums, validation sums) with ONE device-to-host copy (= one synchronisation) and one reset."""
        both = self._metrics2.detach().cpu().numpy().astype(np.float64)
        if reset:
            self._metrics2.zero_()
        n, st = self.F + 3, self._metrics_stride
        return both[:n].copy(), both[st: st + n].copy()

    def profile_enable(self, on: bool) -> None:
        check(self.lib.dib_profile_enable(1 if on else 0), "dib_profile_enable")

    def profile_summary(self) -> dict:
        """{kernel symbol: (total ms, launches)} since profile_enable(True); synchronises."""
        return profile_summary(self.lib)


    # ---- views / helpers ---------------------------------------------------------------------
    def pred(self, batch: int) -> torch.Tensor:
        return self.ws_view(batch, _lib.WS_PRED, batch * self.out_dim).view(batch, self.out_dim)

    def u(self, batch: int) -> torch.Tensor:
        return self.ws_view(batch, _lib.WS_U, batch * self.F * self.E).view(batch, self.F * self.E)

    def enc_out(self, batch: int) -> torch.Tensor:
        # stored feature-major [F][B][2E] on the device; presented as [B, F, 2E]
        return self.ws_view(batch, _lib.WS_ENC_OUT, batch * self.F * 2 * self.E).view(self.F, batch, 2 * self.E) \
            .permute(1, 0, 2)

    def enc_h(self, batch: int, layer: int) -> torch.Tensor:
        """post-activation output of encoder hidden layer `layer` as stashed by the training forward: [F, B, units]."""
        w = self.enc_units[layer]
        if layer == 0 and int(self.lib.dib_workspace_h1_stashed(self.layout, _ptr(self.workspace(batch)))) == 0:
            # the last training forward left this layer to the weight gradient's recompute (dib_set_tuning "wgrad_recompute_h1"):
            # the region holds no activations.  Fill it from the inputs that forward left in the workspace and the CURRENT
            # parameters (the unfused path's GEMM: last-bit differences from the step's own values are possible) - or fail.
            rc = int(self.lib.dib_workspace_h1_materialize(self.layout, batch, _ptr(self.params), _ptr(self.workspace(batch)),
                                                           self._stream()))
            if rc != 0:
                raise _lib.DibError(f"enc_h(layer=0): the last forward of batch size {batch} did not stash the first hidden layer (its "
                                    f"layer-2 weight gradient recomputes it) and it could not be recomputed here "
                                    f"(dib_workspace_h1_materialize -> {rc}); dib_set_tuning('wgrad_recompute_h1', 0) before the "
                                    f"forward keeps the stash")
        return self.ws_view(batch, _lib.WS_ENC_H0 + layer, batch * self.F * w).view(self.F, batch, w)

    def int_h(self, batch: int, layer: int) -> torch.Tensor:
        """post-activation output of integration hidden layer `layer`: [B, units]."""
        w = self.int_units[layer]
        return self.ws_view(batch, _lib.WS_INT_H0 + layer, batch * w).view(batch, w)

    def g_u(self, batch: int) -> torch.Tensor:
        return self.ws_view(batch, _lib.WS_G_U, batch * self.F * self.E).view(batch, self.F * self.E)

    def g_pred(self, batch: int) -> torch.Tensor:
        """dL/d(model output) [batch, out_dim]: what backward_from_pred_grad consumes (a view of the step workspace)."""
        return self.ws_view(batch, _lib.WS_G_PRED, batch * self.out_dim).view(batch, self.out_dim)

    def step_out(self, batch: int) -> torch.Tensor:
        return self.ws_view(batch, _lib.WS_STEP_OUT, self.F + 3)

    def encode_feature(self, f: int, x_f) -> torch.Tensor:
        """model.feature_encoders[f](x_f): deterministic [N, 2E] (reference models.py:183, visualization.py:31)."""
        xf = self.to_device(x_f).reshape(-1, self.dims[f])
        n = xf.shape[0]
        out = torch.empty((n, 2 * self.E), dtype=torch.float32, device=self.device)
        ws = self.scratch(int(self.lib.dib_workspace_bytes(self.layout, n)))
        check(self.lib.dib_encode_deterministic(self.layout, int(f), _ptr(xf), n, _ptr(self.params), _ptr(out),
                                                _ptr(ws), self._stream()), "dib_encode_deterministic")
        return out

    def bhattacharyya(self, mu1, lv1, mu2, lv2) -> torch.Tensor:
        mu1, lv1, mu2, lv2 = [self.to_device(t) for t in (mu1, lv1, mu2, lv2)]
        n, d = mu1.shape
        m = mu2.shape[0]
        out = torch.empty((n, m), dtype=torch.float32, device=self.device)
        check(self.lib.dib_bhattacharyya(_ptr(mu1), _ptr(lv1), n, _ptr(mu2), _ptr(lv2), m, d, _ptr(out),
                                         self._stream()), "dib_bhattacharyya")
        return out

    def infonce(self, emb_x: torch.Tensor, emb_y: torch.Tensor, similarity: str = "l2", temperature: float = 1.0,
                want_grads: bool = True, out_gx: Optional[torch.Tensor] = None, out_gy: Optional[torch.Tensor] = None,
                loss_out: Optional[torch.Tensor] = None):
        """Symmetric InfoNCE (reference train.py:201-214, utils.py:131-175) -> (loss [1] device tensor, g_x, g_y).
        out_gx / out_gy: contiguous [B, D] tensors to receive the gradients (e.g. the model's dL/d(output) workspace view and
        the Y encoder's gradient buffer: the training loop then needs no copies).  loss_out: a 1-element float32 device tensor
        to receive the loss (a slot of the caller's per-epoch buffer) instead of a fresh allocation."""
        emb_x, emb_y = emb_x.contiguous(), emb_y.contiguous()
        b, d = emb_x.shape
        ws = self._infonce_ws.get(b)
        if ws is None:
            if len(self._infonce_ws) >= 4:
                self._infonce_ws.pop(next(iter(self._infonce_ws)))
            ws = self._infonce_ws[b] = torch.empty(int(self.lib.dib_infonce_workspace_bytes(b)) // 4, dtype=torch.float32,
                                                   device=self.device)
        loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=self.device)
        assert loss.numel() == 1 and loss.dtype == torch.float32 and loss.device == self.device
        gx = gy = None
        if want_grads:
            for o in (out_gx, out_gy):
                assert o is None or (o.is_contiguous() and tuple(o.shape) == (b, d) and o.dtype == torch.float32)
            gx = out_gx if out_gx is not None else torch.empty_like(emb_x)
            gy = out_gy if out_gy is not None else torch.empty_like(emb_y)
        check(self.lib.dib_infonce_fwd_bwd(_ptr(emb_x), _ptr(emb_y), b, d, _lib.SIMILARITIES[similarity], float(temperature),
                                           _ptr(gx), _ptr(gy), _ptr(loss), _ptr(ws), self._stream()), "dib_infonce_fwd_bwd")
        return loss, gx, gy

    def backward_from_pred_grad(self, g_pred: torch.Tensor, row_idx, row0: int, batch: int, seed: int, step: int,
                                inv_global_batch: Optional[float] = None, finish_flags: int = 0, optimizer=None,
                                companion=None, metrics_acc: Optional[torch.Tensor] = None) -> None:
        """Backward of the model given dL/d(model output) from a custom loss (reference train.py:216-219): the
        beta*KL term (models.py:118) is added inside the encoder-bank backward.  Gradients land in self.grads.
        finish_flags / optimizer: what the backward's last launch also does (step_tail: e.g. TAIL_KL | TAIL_METRICS after a
        forward(defer_sums=True), and the optimizer update of a single-process loop); TAIL_METRICS accumulates into `metrics_acc`
        (a custom loop passes its OWN accumulator: the default is the one model.fit's History is read from)."""
        inv = 1.0 / batch if inv_global_batch is None else inv_global_batch
        dst = self.g_pred(batch)
        if not (g_pred.data_ptr() == dst.data_ptr() and g_pred.shape == dst.shape and g_pred.stride() == dst.stride()):
            dst.copy_(g_pred)   # (a custom loss may have written its gradient straight into the view)
        self.backward(row_idx, row0, batch, seed, step, inv, finish_flags=finish_flags, optimizer=optimizer, companion=companion,
                      metrics_acc=metrics_acc)

    def mi_sandwich_bounds(self, enc_out: torch.Tensor, seed: int, step: int, feature: int):
        """(InfoNCE lower, leave-one-out upper) in nats for one batch enc_out [N, 2E] (reference utils.py:36-62)."""
        rows = mi_sandwich_rows(self.lib, self.device, self.to_device(enc_out), seed, step, feature)
        m = rows.mean(dim=1).cpu().numpy()
        return float(m[0]), float(m[1])

    # Most rows of one deterministic encode of feature_information (whole evaluation batches; one batch when a batch is larger).
    # The encode's scratch is a full step workspace of that many rows - 0.2 MB per row at F = 64 with [128, 128] encoders: 417 MB
    # here, 1.6 GB at 8192 - and larger launches gain little: 8 x 1024 rows at F = 64 take 5.83 / 5.20 / 5.04 / 5.03 ms with 1024 /
    # 2048 / 4096 / 8192 rows per encode (tools/feature_information_bench.py, profiles/feature_information_bench.json).
    FEATURE_INFORMATION_ROWS = 2048

    def _evaluation_workspace(self, batch: int) -> torch.Tensor:
        """An initialised workspace of `batch` rows that belongs to the evaluation helpers alone (never a step workspace: see
        scratch); the two most recent sizes are kept - the full chunk and the tail chunk of feature_information."""
        ws = self._eval_ws.pop(batch, None)
        if ws is None:
            nbytes = int(self.lib.dib_workspace_bytes(self.layout, batch))
            if nbytes <= 0:
                raise _lib.DibError(f"dib_workspace_bytes({batch}) -> {nbytes}")
            while len(self._eval_ws) >= 2:
                self._eval_ws.pop(next(iter(self._eval_ws)))
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
            check(self.lib.dib_workspace_init(self.layout, batch, _ptr(ws), self._stream()), "dib_workspace_init")
        self._eval_ws[batch] = ws
        return ws

    def feature_information(self, x_dev: torch.Tensor, rows, n: int, nb: int, seed: int, step0: int = 0, want_rows: bool = False,
                            *, want_encodings: bool = False):
        """The sandwich bounds of EVERY feature on nb evaluation batches of n rows: batch b is rows[b n : (b + 1) n] of the
        dataset matrix x_dev [N, sum d_f] (device, float32), its noise keyed (seed, step0 + b, position i, feature f) - what
        encode_feature + mi_sandwich_bounds(enc, seed, step0 + b, f) give per (feature, batch).  Per chunk of whole batches:
        one deterministic dib_encoder_bank_fwd into an evaluation workspace and one dib_mi_features_bounds on its ENC_OUT
        (include/dib_mi_features.h); nothing is read back before the end.  A shape outside that kernel's envelope takes the
        per-feature loop.  Returns float64 numpy [F, nb, 2] (lower, upper) in nats; with want_rows also the per-row lower and
        upper bounds [F, nb, n] each; with want_encodings also the encodings used, float32 [F, nb n, 2E]."""
        F, E, n, nb = self.F, self.E, int(n), int(nb)
        rows = self.to_device(rows, dtype=torch.int32).reshape(-1)
        if rows.numel() != nb * n or x_dev.dim() != 2 or x_dev.shape[1] != self.sum_d:
            raise ValueError(f"feature_information: {rows.numel()} rows for {nb} batches of {n}, inputs {tuple(x_dev.shape)}")
        seed, step0 = int(seed) & (2 ** 64 - 1), int(step0)
        dev, f64 = self.device, torch.float64
        out = torch.empty((F, nb, 2), dtype=f64, device=dev)
        lo = torch.empty((F, nb, n), dtype=f64, device=dev) if want_rows else None
        up = torch.empty((F, nb, n), dtype=f64, device=dev) if want_rows else None
        encs = torch.empty((F, nb * n, 2 * E), dtype=torch.float32, device=dev) if want_encodings else None
        if not int(self.lib.dib_mi_features_supported(F, E, n, 1)):
            col = np.concatenate([[0], np.cumsum(self.dims)])
            for b in range(nb):
                xb = x_dev[rows[b * n: (b + 1) * n].long()]
                for f in range(F):
                    enc = self.encode_feature(f, xb[:, col[f]: col[f + 1]])
                    r = mi_sandwich_rows(self.lib, dev, enc, seed, step0 + b, f)
                    out[f, b] = r.mean(dim=1)
                    if want_rows:
                        lo[f, b], up[f, b] = r[0], r[1]
                    if want_encodings:
                        encs[f, b * n: (b + 1) * n] = enc
        else:
            kb = max(1, min(nb, self.FEATURE_INFORMATION_ROWS // n, 65535 // F))
            mi_ws = torch.empty(int(self.lib.dib_mi_features_workspace_bytes(F, E, n, kb)) // 8 + 2, dtype=f64, device=dev)
            for b0 in range(0, nb, kb):
                k = min(kb, nb - b0)
                ws = self._evaluation_workspace(k * n)
                check(self.lib.dib_encoder_bank_fwd(self.layout, _ptr(x_dev), x_dev.stride(0), _ptr(rows[b0 * n:]), 0, k * n,
                                                    _ptr(self.params), 0, 0, _lib.FWD_DETERMINISTIC | _lib.FWD_INFERENCE,
                                                    _ptr(ws), self._stream()), "dib_encoder_bank_fwd")
                off = int(self.lib.dib_workspace_offset(self.layout, k * n, _lib.WS_ENC_OUT)) // 4
                enc = ws[off: off + F * k * n * 2 * E]
                part = out if k == nb else torch.empty((F, k, 2), dtype=f64, device=dev)
                plo = lo if (k == nb or not want_rows) else torch.empty((F, k, n), dtype=f64, device=dev)
                pup = up if (k == nb or not want_rows) else torch.empty((F, k, n), dtype=f64, device=dev)
                check(self.lib.dib_mi_features_bounds(_ptr(enc), k * n, 0, F, E, n, k, seed, (step0 + b0) & 0xFFFFFFFF, 0,
                                                      _ptr(part), _ptr(plo), _ptr(pup), None, _ptr(mi_ws), self._stream()),
                      "dib_mi_features_bounds")
                if k != nb:
                    out[:, b0: b0 + k] = part
                    if want_rows:
                        lo[:, b0: b0 + k], up[:, b0: b0 + k] = plo, pup
                if want_encodings:
                    encs[:, b0 * n: (b0 + k) * n] = enc.view(F, k * n, 2 * E)
        res = [out.cpu().numpy()]
        if want_rows:
            res += [lo.cpu().numpy(), up.cpu().numpy()]
        if want_encodings:
            res.append(encs.cpu().numpy())
        return res[0] if len(res) == 1 else tuple(res)

    def compression_matrices(self, x_dev: torch.Tensor, rows, counts, want_distances: bool = False, *, want_encodings: bool = False):
        """The compression-scheme matrix exp(-Bhattacharyya distance) of EVERY feature on its own display rows: feature f is
        shown on rows[f, :counts[f]] of the dataset matrix x_dev [N, sum d_f] (device, float32); rows is an int32 host table
        [F, n_max] (entries beyond counts[f] are padding, any valid row).  One dib_compression_gather, one deterministic
        dib_encoder_bank_fwd of n_max rows into an evaluation workspace, one dib_compression_matrices on its ENC_OUT
        (include/dib_compression.h) and ONE read-back.  A shape outside that kernel's envelope takes the per-feature launches
        (encode_feature + bhattacharyya).  Returns float32 numpy [F, n_max, n_max], zero outside [:counts[f], :counts[f]]; with
        want_distances also the distances in the same layout; with want_encodings also the encodings used, float32
        [F, n_max, 2E] (rows beyond counts[f] are the padding's).  A row index outside [0, N) raises ValueError before any launch.
        Nothing of the training state is touched."""
        F, E = self.F, self.E
        rows = np.ascontiguousarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows))
        counts = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts).reshape(-1)
        if x_dev.dim() != 2 or x_dev.shape[1] != self.sum_d or rows.ndim != 2 or rows.shape[0] != F or rows.shape[1] < 1 \
                or counts.shape[0] != F:
            raise ValueError(f"compression_matrices: rows {rows.shape}, counts {counts.shape} for {F} features, inputs "
                             f"{tuple(x_dev.shape)}")
        n_max, N = int(rows.shape[1]), int(x_dev.shape[0])
        if not (np.issubdtype(rows.dtype, np.integer) and np.issubdtype(counts.dtype, np.integer)):
            raise ValueError("compression_matrices: rows and counts must be integer tables")
        if rows.min() < 0 or rows.max() >= N or counts.min() < 0 or counts.max() > n_max:
            raise ValueError(f"compression_matrices: row indices must lie in [0, {N}) and counts in [0, {n_max}]")
        dev = self.device
        if not int(self.lib.dib_compression_supported(F, E, n_max)):
            col = np.concatenate([[0], np.cumsum(self.dims)])
            comp = np.zeros((F, n_max, n_max), dtype=np.float32)
            dist = np.zeros((F, n_max, n_max), dtype=np.float32) if want_distances else None
            encs = np.zeros((F, n_max, 2 * E), dtype=np.float32) if want_encodings else None
            for f in range(F):
                c = int(counts[f])
                if c == 0:
                    continue
                idx = torch.from_numpy(rows[f, :c].astype(np.int64)).to(dev)
                enc = self.encode_feature(f, x_dev[idx][:, col[f]: col[f + 1]])
                if want_encodings:
                    encs[f, :c] = enc.cpu().numpy()
                mu, lv = enc[:, :E], enc[:, E:]
                d = self.bhattacharyya(mu, lv, mu, lv).cpu().numpy()
                comp[f, :c, :c] = np.exp(-d)
                if want_distances:
                    dist[f, :c, :c] = d
            res = [comp] + ([dist] if want_distances else []) + ([encs] if want_encodings else [])
            return res[0] if len(res) == 1 else tuple(res)
        table = self.to_device(np.concatenate([rows.reshape(-1), counts]).astype(np.int32), dtype=torch.int32)   # one upload
        xg = torch.empty((n_max, self.sum_d), dtype=torch.float32, device=dev)
        check(self.lib.dib_compression_gather(self.layout, _ptr(x_dev), x_dev.stride(0), N, _ptr(table), n_max, _ptr(xg),
                                              self._stream()), "dib_compression_gather")
        ws = self._evaluation_workspace(n_max)
        check(self.lib.dib_encoder_bank_fwd(self.layout, _ptr(xg), self.sum_d, None, 0, n_max, _ptr(self.params), 0, 0,
                                            _lib.FWD_DETERMINISTIC | _lib.FWD_INFERENCE, _ptr(ws), self._stream()),
              "dib_encoder_bank_fwd")
        off = int(self.lib.dib_workspace_offset(self.layout, n_max, _lib.WS_ENC_OUT)) // 4
        enc = ws[off: off + F * n_max * 2 * E]
        out = torch.empty((2 if want_distances else 1, F, n_max, n_max), dtype=torch.float32, device=dev)
        check(self.lib.dib_compression_matrices(_ptr(enc), n_max, 0, F, E, _ptr(table[F * n_max:]), n_max,
                                                _ptr(out[1]) if want_distances else None, _ptr(out[0]), self._stream()),
              "dib_compression_matrices")
        host = out.cpu().numpy()
        res = [host[0]] + ([host[1]] if want_distances else []) + ([enc.view(F, n_max, 2 * E).cpu().numpy()] if want_encodings else [])
        return res[0] if len(res) == 1 else tuple(res)

    def eps(self, row_idx, row0: int, batch: int, seed: int, step: int) -> torch.Tensor:
        out = torch.empty((batch, self.F, self.E), dtype=torch.float32, device=self.device)
        check(self.lib.dib_philox_normal_fill(_ptr(out), _ptr(row_idx), int(row0), batch, self.F, self.E, int(seed),
                                              int(step) & 0xFFFFFFFF, self._stream()), "dib_philox_normal_fill")
        return out


PROFILE_CATEGORIES = 19  # include/dib_hip.h dib_profile_summary_n: the kernel categories (entry 19 there re-counts a part of 17)


def profile_summary(lib) -> dict:
    """{kernel symbol: (total ms, launches)} of the library's live HIP-event timing since dib_profile_enable(1)."""
    ms = (ctypes.c_double * PROFILE_CATEGORIES)()
    cnt = (c_int * PROFILE_CATEGORIES)()
    check(lib.dib_profile_summary_n(ms, cnt, PROFILE_CATEGORIES), "dib_profile_summary_n")
    bk = lambda mode, ni, nj: 64 if (ni, nj) == (2, 2) or (mode, ni, nj) == (2, 1, 2) else 32  # csrc/host/gemm.h launch_gemm_t
    names = [f"dib_gemm_kernel<{mode}, {ni}, {nj}, {bk(mode, ni, nj)}>"
             for mode in (0, 1, 2) for ni in (1, 2) for nj in (1, 2)]
    names += ["dib_fused_encoder_fwd_kernel", "dib_fused_encoder_bwd_kernel", "other", "dib_attn_fwd_kernel", "dib_attn_bwd_kernel"]
    names += ["dib_wgrad_stream_kernel<4>", "dib_wgrad_stream_kernel<2>"]   # 128- / 64-column tiles (csrc/dib_wgrad_stream.h)
    return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(names) if cnt[i]}
