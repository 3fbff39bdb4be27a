"""Drop-in mirror of the reference's `models.py` surface on the MI355X-native path.

    DistributedIBNet / compile / fit / InfoBottleneckAnnealingCallback /
    SaveCompressionMatricesCallback / PositionalEncoding

Same names, argument meaning and History contract as the TensorFlow/Keras reference
(reference models.py:12-186, train.py:138-178); the device math is hand-written HIP for gfx950
reached through the C ABI (include/dib_hip.h) - see engine.py.  Nothing here falls back to CPU.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _fit
from . import losses as _losses
from . import optimizers as _optimizers


class PositionalEncoding:
    """reference models.py:12-23: concat([x] + [sin(f*x) for f in frequencies], -1).
    Parameter-free; on the hot path it is fused into the encoder-bank kernels - this host class
    only carries the frequency list (and evaluates on numpy for small host-side uses)."""

    def __init__(self, frequencies):
        self.frequencies = np.asarray(frequencies)

    def __call__(self, inputs):
        x = np.asarray(inputs)
        return np.concatenate([x] + [np.sin(f * x) for f in self.frequencies], -1)

    call = __call__


class _BetaVariable:
    """Stands in for `tf.Variable(1., trainable=False)` (reference models.py:86): device-resident
    scalar read by the kernels, so annealing never re-launches or re-captures anything."""

    def __init__(self, model, value=1.0):
        self._model = model
        self._host = np.float32(value)

    def assign(self, value):
        self._host = np.float32(value)
        if self._model._engine is not None:
            self._model._engine.set_beta(float(self._host))
        return self

    def value(self):
        return self._host

    def numpy(self):
        return self._host

    def __float__(self):
        return float(self._host)

    def __mul__(self, other):
        return self._host * other

    __rmul__ = __mul__

    def __repr__(self):
        return f"<beta={float(self._host):.6g}>"


class _FeatureEncoder:
    """`model.feature_encoders[f]`: callable [N, d_f] -> [N, 2E] (mu | logvar), deterministic
    (reference models.py:73-78,183; visualization.py:31)."""

    def __init__(self, model, index):
        self._model, self.index = model, index

    def __call__(self, x_f):
        eng = self._model._ensure_engine()
        return eng.encode_feature(self.index, x_f).detach().cpu().numpy()


class History:
    """Keras History: `.history[k]` = list of per-epoch floats (reference train.py:169-172)."""

    def __init__(self):
        self.history: Dict[str, List[float]] = {}
        self.epoch: List[int] = []
        self.model = None
        # fit(track_information=...): {"epochs": [...], "beta": [...], "bounds": float64 [n_evals, F, 2] (lower, upper) nats}
        self.information: Optional[dict] = None


class Callback:
    """Keras callback protocol subset used by the reference (on_epoch_begin/on_epoch_end, .model)."""

    def __init__(self):
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass


class DistributedIBNet:
    """Distributed IB model: one Gaussian bottleneck per input feature (reference models.py:26-123).

    Constructor arguments are exactly those of the reference (models.py:56-66).  Extra keyword-only
    knobs (`noise_seed`, `init_seed`, `shuffle_seed`, `device`) make runs reproducible: the
    reference samples eps from an unseeded stateful generator, here eps is a counter-based function
    of (noise_seed, step, dataset row, feature, dim).
    """

    def __init__(self,
                 feature_dimensionalities,
                 feature_encoder_architecture,
                 integration_network_architecture,
                 output_dimensionality,
                 use_positional_encoding=True,
                 number_positional_encoding_frequencies=5,
                 activation_fn='relu',
                 feature_embedding_dimension=32,
                 output_activation_fn=None,
                 *, noise_seed: int = 0, init_seed: int = 0, shuffle_seed: int = 0, device: Optional[str] = None):
        self.feature_dimensionalities = [int(d) for d in feature_dimensionalities]
        self.number_features = len(self.feature_dimensionalities)
        self.feature_encoder_architecture = [int(u) for u in feature_encoder_architecture]
        self.integration_network_architecture = [int(u) for u in integration_network_architecture]
        self.output_dimensionality = int(output_dimensionality)
        self.use_positional_encoding = bool(use_positional_encoding)
        self.number_positional_encoding_frequencies = int(number_positional_encoding_frequencies)
        self.activation_fn = activation_fn if activation_fn not in ("None", "") else None
        self.feature_embedding_dimension = int(feature_embedding_dimension)
        self.output_activation_fn = output_activation_fn
        # reference models.py:70
        self.positional_encoding_frequencies = 2 ** np.arange(1, self.number_positional_encoding_frequencies)
        self.noise_seed, self.init_seed, self.shuffle_seed = int(noise_seed), int(init_seed), int(shuffle_seed)
        self._device = device
        self._engine = None
        # data-parallel gradient all-reduce buckets (fit under torch.distributed): 3 = integration / encoder front layers /
        # last encoder layer, each issued as soon as it is final (default); 2 = integration / encoder bank; 1 = one all-reduce
        self.dp_small_batch_rows = 1024   # per-rank batches up to this many rows use ONE gradient bucket (see fit)
        self.validation_merge_rows = 1024  # fit: full validation batches are evaluated together up to this many rows (0: one by one)
        self.syncs_per_epoch = 1   # fit: 2 = A/B switch, round 5's order (the training sums read before the validation pass)
        self._metric = None   # compile: (History key, DIB_METRIC_* name, square root at the end of the epoch)
        self.dp_buckets = int(os.environ.get("DIB_DP_BUCKETS", "3"))
        if self.dp_buckets not in (1, 2, 3):
            raise ValueError(f"DIB_DP_BUCKETS={self.dp_buckets}: 1, 2 or 3")
        self.beta = _BetaVariable(self, 1.0)
        self.feature_encoders = [_FeatureEncoder(self, f) for f in range(self.number_features)]
        self.optimizer = None
        self.loss = None
        self.metrics_names: List[str] = []
        self.losses: list = []
        self.history = None
        self.stop_training = False
        self._step = 0
        self._pending_weights = None

    # ---- engine -----------------------------------------------------------------------------
    def _spec_kwargs(self):
        return dict(feature_dimensionalities=self.feature_dimensionalities,
                    feature_encoder_architecture=self.feature_encoder_architecture,
                    integration_network_architecture=self.integration_network_architecture,
                    output_dimensionality=self.output_dimensionality,
                    use_positional_encoding=self.use_positional_encoding,
                    number_positional_encoding_frequencies=self.number_positional_encoding_frequencies,
                    activation_fn=self.activation_fn,
                    feature_embedding_dimension=self.feature_embedding_dimension,
                    output_activation_fn=self.output_activation_fn)

    def _make_engine(self):
        """The device engine of this model: HipEngine, which raises without a GPU or libdib_hip.so - there is no CPU path."""
        from .engine import HipEngine
        return HipEngine(**self._spec_kwargs(), device=self._device, init_seed=self.init_seed)

    def _ensure_engine(self):
        if self._engine is None:
            self._engine = self._make_engine()
            self._engine.set_beta(float(self.beta.value()))
            if self._pending_weights is not None:
                self._engine.set_flat_params(self._pending_weights)
                self._pending_weights = None
        return self._engine

    def build(self, input_shape):
        """reference models.py:88-94."""
        assert input_shape[-1] == np.sum(self.feature_dimensionalities)
        self._ensure_engine()

    # ---- weights ----------------------------------------------------------------------------
    def get_flat_weights(self) -> np.ndarray:
        return self._ensure_engine().get_flat_params()

    def set_flat_weights(self, flat) -> None:
        self._ensure_engine().set_flat_params(np.asarray(flat, dtype=np.float32))

    def param_blocks(self):
        """[{net, layer, feature, what, offset, rows, cols}] describing the flat buffer."""
        return self._ensure_engine().blocks

    @property
    def trainable_variables(self):
        """Views into the flat parameter buffer, Keras order: per feature encoder (kernel, bias)*, then
        the integration network (reference train.py:196)."""
        eng = self._ensure_engine()
        by = {(b["net"], b["layer"], b["feature"], b["what"]): b for b in eng.blocks}
        out = []
        for f in range(self.number_features):
            for l in range(len(self.feature_encoder_architecture) + 1):
                for what in (0, 1):
                    b = by[(0, l, f, what)]
                    v = eng.params[b["offset"]: b["offset"] + b["rows"] * b["cols"]]
                    out.append(v.view(b["rows"], b["cols"]) if what == 0 else v)
        for l in range(len(self.integration_network_architecture) + 1):
            for what in (0, 1):
                b = by[(1, l, 0, what)]
                v = eng.params[b["offset"]: b["offset"] + b["rows"] * b["cols"]]
                out.append(v.view(b["rows"], b["cols"]) if what == 0 else v)
        return out

    def count_params(self) -> int:
        return int(self._ensure_engine().n_params)

    # ---- call ---------------------------------------------------------------------------------
    def __call__(self, inputs, training=None):
        """reference models.py:96-123: returns the prediction [B, out]; noise is always on (the
        reference's call has no `training` switch).  Sets `self.losses = [beta * sum_f KL_f]`
        (models.py:118) and `self.last_kl` [F] (nats)."""
        eng = self._ensure_engine()
        x = eng.to_device(np.asarray(inputs, dtype=np.float32) if not isinstance(inputs, torch.Tensor) else inputs)
        if x.dim() == 1:
            x = x.view(1, -1)
        B = x.shape[0]
        eng.forward(x, None, 0, B, self.noise_seed, self._step, inference=True)  # not differentiable: forward_autograd is
        self._step += 1
        kl = eng.step_out(B)[: self.number_features].clone() / B
        self.last_kl = kl
        self.losses = [kl.sum() * float(self.beta.value())]
        return eng.pred(B).clone()

    call = __call__

    # ---- autograd bridge for custom PyTorch training loops ------------------------------------------
    def forward_autograd(self, inputs, row_ids=None):
        """Differentiable forward for hand-written loops (the reference's custom-loop contract, train.py:196-220:
        `model(x)`, `model.losses`, `model.trainable_variables` under a gradient tape).

        Returns `(prediction [B, out], kl_loss)` where `kl_loss = beta * sum_f KL_f` (models.py:118) - both are
        autograd-connected to `model.flat_parameters` (a leaf tensor aliasing the engine's flat parameter buffer):

            pred, kl_loss = model.forward_autograd(x)
            loss = my_loss(pred, y) + kl_loss
            loss.backward()                       # runs the HIP backward kernels; fills model.flat_parameters.grad
            torch_optimizer.step()                # any torch.optim optimizer over [model.flat_parameters]

        When `inputs` is a tensor that requires a gradient (the output of another torch module), backward() also fills its
        gradient (dib_encoder_bank_input_grad); otherwise nothing extra is launched.  First derivatives only.  That gradient is
        bit-reproducible except under `row_ids` that repeat a row: the batch positions of a row are summed by torch's index_add_
        (atomic adds, an order that varies from run to run).

        `row_ids` (int tensor [B]) keys the noise per sample; default arange(B).  The batch-mean convention of the
        KL term matches the reference: the caller's loss should be a mean over the batch."""
        eng = self._ensure_engine()
        x = eng.to_device(np.asarray(inputs, dtype=np.float32) if not isinstance(inputs, torch.Tensor) else inputs)
        if x.dim() == 1:
            x = x.view(1, -1)
        idx = None if row_ids is None else eng.to_device(row_ids, dtype=torch.int32)
        step = self._step
        self._step += 1
        pred, kl_loss = _DIBFunction.apply(self.flat_parameters, self, x, idx, step)
        self.losses = [kl_loss]
        return pred, kl_loss

    @property
    def flat_parameters(self) -> torch.Tensor:
        """The engine's flat fp32 parameter buffer as an autograd leaf (shares memory: optimizer updates are seen by
        the kernels directly)."""
        eng = self._ensure_engine()
        if getattr(self, "_flat_leaf", None) is None or self._flat_leaf.data_ptr() != eng.params.data_ptr():
            self._flat_leaf = eng.params.detach().requires_grad_(True)
        return self._flat_leaf

    def predict(self, x, batch_size=None, verbose=0):
        eng = self._ensure_engine()
        xd = _fit.device_matrix(eng, x)
        if xd is None:
            xd = eng.to_device(x)
        n = xd.shape[0]
        bs = int(batch_size or 32768)
        outs = []
        for s0 in range(0, n, bs):
            b = min(bs, n - s0)
            eng.forward(xd, None, s0, b, self.noise_seed, (1 << 30) + s0 // bs, inference=True)
            outs.append(eng.pred(b).clone())
        return torch.cat(outs, 0).cpu().numpy()

    def information_per_feature(self, x, evaluation_batch_size=1024, number_evaluation_batches=8, seed=0, per_batch=False):
        """Lower (InfoNCE) and upper (leave-one-out) bounds, in nats, on the information every feature's channel transmits
        (reference utils.py:10-73 for each encoder, models.py:188-223): float64 [F, 2], the mean over the evaluation batches, or
        [F, number_evaluation_batches, 2] with per_batch=True.

        `x` is an input matrix [N, sum d_f] (array-like, or a float32 tensor already on the model's device).  The batches are the
        rows utils.evaluation_batch_rows(N, evaluation_batch_size, number_evaluation_batches, seed) - the same rows for every
        feature - and the noise of sample i of batch b of feature f is keyed (seed, b, i, f): the quantities
        utils.estimate_mi_sandwich_bounds(self.feature_encoders[f], x_f, ..., seed=seed) gives feature by feature, here from
        one encoder-bank forward and one dib_mi_features_bounds launch sequence per chunk of batches and ONE read-back
        (engine.feature_information).  Nothing of the training state is touched.  Under torch.distributed every rank computes
        the same numbers locally; there is no collective."""
        from . import utils
        eng = self._ensure_engine()
        xd = x if isinstance(x, torch.Tensor) and x.device == eng.device and x.dtype == torch.float32 else eng.to_device(
            x if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float32))
        if xd.dim() == 1:
            xd = xd.view(-1, 1)
        bs, nb = int(evaluation_batch_size), int(number_evaluation_batches)
        rows = utils.evaluation_batch_rows(xd.shape[0], bs, nb, seed)
        bounds = eng.feature_information(xd, rows.astype(np.int32), bs, nb, seed, 0)
        return bounds if per_batch else bounds.mean(axis=1)

    def compression_matrices(self, x_processed, x_raw=None, max_number_to_display=128, rng=None, return_distances=False,
                             cache=None):
        """The compression scheme of every feature (reference visualization.py:14-81, models.py:152-186): for feature f the
        matrix exp(-Bhattacharyya distance) between the Gaussians its encoder assigns to a display sample of its values.
        Returns a list of F dicts: "matrix" float32 [n_f, n_f], "indices" (the sample's rows of x_processed), "values" (their
        raw values, sorted), "counts" (the value frequencies of a feature with < 10 unique values, else None) and, with
        return_distances, "distances" [n_f, n_f].

        `x_processed` is the input matrix [N, sum d_f] (array-like, or a float32 tensor already on the model's device), `x_raw`
        the matrix of the same shape the sample is drawn and labelled from (default: x_processed).  The samples are
        visualization.display_rows(x_raw, ..., rng, cache): the rows visualization.save_compression_matrices draws feature by
        feature under the same `rng`.  All matrices come from ONE deterministic encoder-bank forward, one
        dib_compression_matrices launch and ONE read-back (engine.compression_matrices); an engine without that method takes
        the per-feature loop.  Nothing of the training state is touched.  Under torch.distributed every rank may call it:
        there is no collective."""
        from . import visualization
        eng = self._ensure_engine()
        on_device = isinstance(x_processed, torch.Tensor)
        if x_raw is None:
            x_raw = x_processed.detach().cpu().numpy() if on_device else np.asarray(x_processed)
        sel = visualization.display_rows(x_raw, self.feature_dimensionalities, max_number_to_display, rng, cache)
        F = self.number_features
        if hasattr(eng, "compression_matrices"):
            xd = x_processed if on_device and x_processed.device == eng.device and x_processed.dtype == torch.float32 \
                else eng.to_device(x_processed if on_device else np.asarray(x_processed, dtype=np.float32))
            if xd.dim() == 1:
                xd = xd.view(-1, 1)
            res = eng.compression_matrices(xd, sel["rows"], sel["n_rows"], want_distances=return_distances)
            comp, dist = res if return_distances else (res, None)
            mats = [comp[f, :n, :n] for f, n in enumerate(sel["n_rows"])]
            dists = [dist[f, :n, :n] for f, n in enumerate(sel["n_rows"])] if return_distances else None
        else:
            xp = x_processed.detach().cpu().numpy() if on_device else np.asarray(x_processed)
            split = np.split(xp.reshape(xp.shape[0], -1), np.cumsum(self.feature_dimensionalities)[:-1], axis=-1)
            pairs = [visualization.encoded_compression_matrix(self.feature_encoders[f], split[f][sel["indices"][f]], self)
                     for f in range(F)]
            mats, dists = [p[0] for p in pairs], [p[1] for p in pairs]
        out = []
        for f in range(F):
            d = dict(matrix=mats[f], indices=sel["indices"][f], values=sel["values"][f], counts=sel["counts"][f])
            if return_distances:
                d["distances"] = dists[f]
            out.append(d)
        return out

    # ---- compile / fit ---------------------------------------------------------------------
    def compile(self, optimizer='adam', loss=None, metrics=None, **_):
        """reference train.py:138-142."""
        self.optimizer = _optimizers.get(optimizer)
        self.loss = _losses.get(loss)
        if isinstance(metrics, str):
            metrics = [metrics]
        self.metrics_names = list(metrics or [])
        if len(self.metrics_names) > 1:
            raise ValueError(f"compile(metrics={self.metrics_names!r}): one metric per compile - the step's metric vector has one "
                             "slot (include/dib_hip.h ws[STEP_OUT][F + 1]); widening it would change the C ABI")
        self._metric = None   # (History key, DIB_METRIC_* name, square root at the end of the epoch)
        if self.metrics_names:
            key, metric, root = _losses.get_metric(self.metrics_names[0])
            if hasattr(self.loss, "check_metric"):
                metric = self.loss.check_metric(metric)
            self._metric = (key, metric, root)
        return self

    def _loss_arg(self):
        """what the engine's train_step / eval_step take: the kind's name for the reference's own kinds with today's 'accuracy'
        (dib_loss_fwd_bwd, the fused one-unit head), else the loss's descriptor with the metric (include/dib_losses.h)"""
        loss, metric = self.loss, (self._metric[1] if self._metric else None)
        if not hasattr(loss, "descriptor"):
            return loss.kind   # a foreign object with a `kind`
        if loss.legacy and metric in (None, loss.resolve_metric("accuracy")):
            return loss.kind
        return loss.descriptor(metric)

    def _check_labels(self, loss_arg, y_np: np.ndarray) -> None:
        """once per fit / evaluate, on the host: the label layout a descriptor's kernel reads (include/dib_losses.h), and for
        CategoricalCrossentropy(from_logits=True) that every label row sums to 1 (its gradient softmax(z) - y assumes it)"""
        if isinstance(loss_arg, str):
            return
        C = self.output_dimensionality
        need = 1 if loss_arg.kind == "sparse_cce" else C
        if y_np.ndim != 2 or y_np.shape[1] != need:
            raise ValueError(f"loss {loss_arg.kind!r} needs labels of shape [N, {need}], got {tuple(y_np.shape)}")
        if loss_arg.kind == "cce_logits" and y_np.size:
            worst = float(np.abs(y_np.astype(np.float64).sum(1) - 1.0).max())
            if not worst <= 1e-5:
                raise ValueError(f"CategoricalCrossentropy(from_logits=True): label rows must sum to 1 (worst row is off by {worst:.3g})")

    def _dist(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_rank(), dist.get_world_size()
        return None, 0, 1

    def _epoch_logs(self, acc: np.ndarray, nsteps: int, prefix: str) -> Dict[str, float]:
        """History accounting (reference models.py:115,121; train.py:169-172):
        loss = sample-weighted mean of (task + beta*sum KL); add_metric scalars (KL{f}, beta) =
        unweighted mean over steps."""
        F = self.number_features
        rows = max(acc[F + 2], 1.0)
        logs = {prefix + "loss": acc[F] / rows}
        if self.metrics_names:
            key, _, root = self._metric or ("accuracy", "accuracy", False)
            # every metric is a sample-weighted mean of per-row values; root_mean_squared_error accumulates the squared errors
            # and takes the root here, at the end of the epoch (Keras' RootMeanSquaredError.result)
            logs[prefix + key] = math.sqrt(acc[F + 1] / rows) if root else acc[F + 1] / rows
        for f in range(F):
            logs[f"{prefix}KL{f}"] = acc[f] / max(nsteps, 1)
        logs[prefix + "beta"] = float(self.beta.value())
        return logs

    def fit(self, x=None, y=None, batch_size=None, epochs=1, verbose=1, callbacks=None, validation_data=None,
            shuffle=True, initial_epoch=0, track_information=None, sample_weight=None, class_weight=None, **_):
        """reference train.py:157-166 `model.fit(x, y, epochs=, shuffle=True, batch_size=, callbacks=,
        verbose=, validation_data=)` -> History.

        Data parallel: when torch.distributed is initialised every rank calls fit() with the same
        arguments; each global batch is split row-wise across ranks, flat gradients are
        all-reduced (RCCL over xGMI with the nccl backend) and every rank applies the same update.

        track_information: a dict - `x` (inputs to evaluate on; default: the validation inputs), `every` (epochs, default 1),
        `evaluation_batch_size` (1024), `number_evaluation_batches` (8).  At the end of every epoch with epoch % every == 0
        information_per_feature(x, ..., seed=epoch) is recorded in History.information = {"epochs", "beta", "bounds"
        [n_evals, F, 2] nats} (not in History.history, whose lists stay one entry per epoch).  The inputs are uploaded once;
        the evaluation reads the parameters and writes nothing the steps use: a tracked fit trains exactly like an untracked one.
        """
        if self.optimizer is None or self.loss is None:
            raise RuntimeError("call compile(optimizer=..., loss=...) before fit()")
        if sample_weight is not None or class_weight is not None:
            raise ValueError("fit(sample_weight=, class_weight=) are not supported: every row of a batch weighs 1 / batch in the "
                             "loss kernels and in the History accounting")
        eng = self._ensure_engine()
        dist, rank, world = self._dist()
        F = self.number_features
        xd, y_np = _fit.device_rows(eng, x), _fit.host_rows(y)
        assert xd.shape[-1] == int(np.sum(self.feature_dimensionalities)), "input width != sum(feature dims)"
        yd = eng.to_device(y_np)
        n, bs = xd.shape[0], int(batch_size or 32)
        xvd = yvd = yv_np = None
        if validation_data is not None:
            xvd, yv_np = _fit.device_rows(eng, validation_data[0]), _fit.host_rows(validation_data[1])
            yvd = eng.to_device(yv_np)
        track = _fit.parse_track_information(eng, track_information, xvd)
        cbs = list(callbacks or [])
        for cb in cbs:
            cb.set_model(self) if hasattr(cb, "set_model") else setattr(cb, "model", self)
        hist = History()
        hist.model = self
        self.history = hist
        if track is not None:
            hist.information = {"epochs": [], "beta": [], "bounds": np.zeros((0, F, 2))}
        self.stop_training = False
        kind = self._loss_arg()
        self._check_labels(kind, y_np)
        if validation_data is not None:
            self._check_labels(kind, yv_np)
        for cb in cbs:
            if hasattr(cb, "on_train_begin"):
                cb.on_train_begin()
        can_capture = _fit.bind_optimizer(eng, self.optimizer)
        graphs = {}
        step = _fit.choose_step(self, eng, xd, yd, bs, epochs, kind, dist, rank, world, can_capture, graphs)
        nsteps = len(range(0, n, bs))   # every epoch: one step per batch, the partial last one included
        next_order = None
        try:
            for epoch in range(initial_epoch, epochs):
                for cb in cbs:
                    cb.on_epoch_begin(epoch)
                eng.set_beta(float(self.beta.value()))
                order_dev = next_order if next_order is not None else _fit.epoch_order(eng, n, shuffle, self.shuffle_seed, epoch)
                next_order = None
                for s0 in range(0, n, bs):
                    step(order_dev, s0, min(bs, n - s0))  # last partial batch is kept (Keras)
                # host work under the device's queue: the next epoch's permutation (12 ms of numpy for 2^20 rows - with it at
                # the top of the epoch the device idled 7 % of a config-3 epoch, bench.py extra.fit_surface) and its upload are
                # done while this epoch's steps are still executing; the read-back below is the epoch's only synchronisation
                if epoch + 1 < epochs and not self.stop_training:
                    next_order = _fit.epoch_order(eng, n, shuffle, self.shuffle_seed, epoch + 1)
                # ONE synchronisation per epoch: the validation pass is enqueued right behind the training steps - its History
                # sums go to an accumulator of their own - and both are read back together (round 5 read the training sums
                # first: the device idled through that round trip and the host work behind it, every epoch)
                early = eng.read_metrics_pair()[0] if self.syncs_per_epoch == 2 else None
                vsteps = 0
                if validation_data is not None:
                    _fit.sync_noise_step(eng, (1 << 31) + epoch)  # validation noise stream, same key as the eager path
                    vsteps = _fit.evaluation_pass(eng, xvd, yvd, bs, kind, self.noise_seed, (1 << 31) + epoch,
                                                  self.validation_merge_rows, rank, world, eng.metrics_acc_val)
                    _fit.sync_noise_step(eng, self._step)
                train_sums, val_sums = eng.read_metrics_pair()
                logs = self._epoch_logs(_fit.reduce_metrics(eng, dist, train_sums if early is None else early), nsteps, "")
                if validation_data is not None:
                    logs.update(self._epoch_logs(_fit.reduce_metrics(eng, dist, val_sums), vsteps, "val_"))
                for k, v in logs.items():
                    hist.history.setdefault(k, []).append(float(v))
                hist.epoch.append(epoch)
                if track is not None and epoch % track["every"] == 0:
                    bounds = self.information_per_feature(track["x"], track.get("evaluation_batch_size", 1024),
                                                          track.get("number_evaluation_batches", 8), seed=epoch)
                    info = hist.information
                    info["epochs"].append(epoch)
                    info["beta"].append(float(self.beta.value()))
                    info["bounds"] = np.concatenate([info["bounds"], bounds[None]], 0)
                if verbose and rank == 0:
                    kls = sum(logs[f"KL{f}"] for f in range(F))
                    print(f"Epoch {epoch + 1}/{epochs} - loss: {logs['loss']:.4f} - sumKL: {kls:.4f} nats - "
                          f"beta: {logs['beta']:.3e}" + (f" - val_loss: {logs['val_loss']:.4f}" if 'val_loss' in logs else ""))
                for cb in cbs:
                    cb.on_epoch_end(epoch, logs)
                if self.stop_training:
                    break
            for cb in cbs:
                if hasattr(cb, "on_train_end"):
                    cb.on_train_end()
        finally:
            if graphs:   # the captured step is dropped with `graphs`: its pinned workspace may be evicted again
                torch.cuda.synchronize(eng.device)   # no replay may be in flight when the graph object dies
                graphs.clear()
                eng.release_step_graph(bs)
        return hist

    def evaluate(self, x, y, batch_size=None, verbose=0, return_dict=True):
        eng = self._ensure_engine()
        if self.loss is None:
            raise RuntimeError("call compile() before evaluate()")
        xd, y_np = _fit.device_rows(eng, x), _fit.host_rows(y)
        yd = eng.to_device(y_np)
        kind = self._loss_arg()
        self._check_labels(kind, y_np)
        eng.read_metrics()
        # full batches are evaluated together like fit's validation pass (same per-row numbers; see validation_merge_rows)
        steps = _fit.evaluation_pass(eng, xd, yd, int(batch_size or 32), kind, self.noise_seed, (1 << 31) - 1,
                                     self.validation_merge_rows, 0, 1, None)
        return self._epoch_logs(eng.read_metrics(), steps, "")


class _DIBFunction(torch.autograd.Function):
    """torch.autograd bridge: forward = dib_encoder_bank_fwd + dib_integration_fwd, backward = the HIP backward
    kernels with the caller's dL/dpred injected (engine.backward_from_pred_grad) and, when the inputs require a gradient (they are
    another network's outputs), dL/dx from engine.input_grad.  First derivatives only: a double backward raises."""

    @staticmethod
    def forward(ctx, flat_params, model, x, idx, step):
        eng = model._ensure_engine()
        B = x.shape[0]
        eng.forward(x, idx, 0, B, model.noise_seed, step)
        ctx.model, ctx.idx, ctx.step, ctx.B = model, idx, step, B
        ctx.want_dx = bool(ctx.needs_input_grad[2])
        if ctx.want_dx:
            ctx.save_for_backward(x)   # read again by the input gradient (x itself: the forward gathers from it)
        ctx.beta = float(model.beta.value())
        # the activations the backward kernels re-read live in the engine's workspace for B rows: remember which forward
        # wrote them so that backward() can refuse to run on a workspace another forward has overwritten since
        ctx.ws_gen = eng._ws_gen.get(B) if hasattr(eng, "_ws_gen") else None
        kl = eng.step_out(B)[: model.number_features].sum() / B
        return eng.pred(B).clone(), (kl * ctx.beta).reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pred, g_kl):
        model = ctx.model
        eng = model._ensure_engine()
        if ctx.ws_gen is not None and eng._ws_gen.get(ctx.B) != ctx.ws_gen:
            raise RuntimeError(
                f"forward_autograd: another forward pass with batch size {ctx.B} ran between forward_autograd() and "
                "backward(); it overwrote the stashed activations of this graph node.  Call backward() before the next "
                "model(x) / predict / evaluate / forward_autograd of the same batch size.")
        # d/dparams of (beta * sum KL) scaled by the incoming gradient of the KL-loss output - as a device scalar, no host sync
        if g_kl is not None:
            eng.beta_dev.copy_((g_kl.detach().to(torch.float32) * ctx.beta).reshape(1))
        else:
            eng.set_beta(0.0)
        eng.backward_from_pred_grad(g_pred.contiguous(), ctx.idx, 0, ctx.B, model.noise_seed, ctx.step,
                                    inv_global_batch=1.0 / ctx.B)
        eng.set_beta(float(model.beta.value()))
        gx = None
        if ctx.want_dx:   # (dout already carries the KL path: beta was scaled by g_kl above)
            x, = ctx.saved_tensors
            gx = eng.input_grad(x, ctx.idx, 0, ctx.B)
            if ctx.idx is not None:   # per batch position -> the rows of x they were gathered from
                gx = torch.zeros_like(x).index_add_(0, ctx.idx.long(), gx)
        return eng.grads.clone(), None, gx, None, None


class DistributedIBModule(torch.nn.Module):
    """A DistributedIBNet as a torch.nn.Module, for a model whose inputs come out of another torch module (the reference README's
    "Data that isn't tabular": a subnetwork processes some features and its output is fed into DistributedIBNet):

        dib = DistributedIBModule(DistributedIBNet([4], [128, 128], [256], 1))
        pred, kl_loss = dib(subnetwork(raw))          # differentiable in dib's parameters AND in subnetwork's
        (my_loss(pred, y) + kl_loss).backward(); torch_optimizer.step()

    Its one nn.Parameter, `flat_parameters`, shares memory with the engine's flat parameter buffer, so an optimizer step is seen by
    the kernels directly.  forward(x, row_ids=None) is DistributedIBNet.forward_autograd.  Needs a GPU: there is no CPU path."""

    def __init__(self, net: "DistributedIBNet"):
        super().__init__()
        self.net = net
        eng = net._ensure_engine()   # raises without a GPU
        self.flat_parameters = torch.nn.Parameter(eng.params, requires_grad=True)
        net._flat_leaf = self.flat_parameters   # what forward_autograd differentiates with respect to

    def forward(self, x, row_ids=None):
        eng = self.net._ensure_engine()
        if self.flat_parameters.data_ptr() != eng.params.data_ptr():
            # forward_autograd would differentiate with respect to a fresh leaf and this Parameter would silently get no gradient
            raise RuntimeError("DistributedIBModule.flat_parameters no longer shares memory with the engine's parameter buffer "
                               "(the module was moved or copied, or the engine's buffer was replaced): build a new "
                               "DistributedIBModule(net)")
        self.net._flat_leaf = self.flat_parameters   # (another wrapper, or net.flat_parameters before this one, may have set its own)
        return self.net.forward_autograd(x, row_ids=row_ids)


class InfoBottleneckAnnealingCallback(Callback):
    """Logarithmically ramp beta during training (reference models.py:125-149).

    on_epoch_begin: beta <- exp(log b0 + max(epoch - n_pre, 0)/n_anneal * (log b1 - log b0)),
    evaluated in float32 like the TF ops of the reference (models.py:147-149).
    """

    def __init__(self, beta_start, beta_end, number_pretraining_epochs, number_annealing_epochs):
        super().__init__()
        self.beta_start = beta_start
        self.beta_end = beta_end
        self.number_pretraining_epochs = number_pretraining_epochs
        self.number_annealing_epochs = number_annealing_epochs

    def beta_at(self, epoch) -> np.float32:
        f32 = np.float32
        frac = f32(max(epoch - self.number_pretraining_epochs, 0)) / f32(self.number_annealing_epochs)
        return f32(np.exp(np.log(f32(self.beta_start)) + frac * (np.log(f32(self.beta_end)) - np.log(f32(self.beta_start)))))

    def on_epoch_begin(self, epoch, logs=None):
        self.model.beta.assign(self.beta_at(epoch))


class SaveCompressionMatricesCallback(Callback):
    """Save per-feature compression-scheme matrices during training (reference models.py:152-186;
    defects A1/A2 of SURVEY App. A fixed by intent: the working copy is train.py:253-261).

    Every `save_frequency` epochs: for each feature, encode a sample of the validation values
    deterministically, Bhattacharyya matrix -> exp(-D) -> PNG named
    feature_{f}_log10beta_{log10(beta):.3f}.png (models.py:181).  The matrices are also kept in
    `self.matrices[(epoch, f)]`.

    one_launch=True evaluates all features together - one `model.compression_matrices` call per save: the same display rows
    (the same draws of numpy's global generator), one encoder-bank forward, one matrices launch and one read-back instead of
    an encode, a distance launch and two read-backs per feature.  The validation matrix is uploaded once, and what the display
    rule decides once per feature - the selection of a feature with < 10 unique values, which is deterministic, or that the
    feature is drawn at random - is kept between saves (visualization.display_rows `cache`).
    """

    def __init__(self, save_frequency, x_processed, x_raw, outdir, save_png=True, one_launch=False):
        super().__init__()
        self.save_frequency = save_frequency
        self.x_processed = np.asarray(x_processed)
        self.x_raw = np.asarray(x_raw)
        self.outdir = outdir
        self.save_png = save_png
        self.one_launch = bool(one_launch)
        self._x_dev = None
        self._selection_cache = {}
        self.matrices = {}
        self.betas = {}   # epoch of a save -> beta

    def _save_one_launch(self, epoch, beta_value):
        from . import visualization
        eng = self.model._ensure_engine()
        if self._x_dev is None and hasattr(eng, "compression_matrices"):   # uploaded once (the per-feature loop reads the host copy)
            self._x_dev = eng.to_device(np.asarray(self.x_processed, dtype=np.float32))
        res = self.model.compression_matrices(self._x_dev if self._x_dev is not None else self.x_processed, self.x_raw,
                                              cache=self._selection_cache)
        for feature_ind, r in enumerate(res):
            if self.save_png:
                out_fname = os.path.join(self.outdir, f'feature_{feature_ind}_log10beta_{np.log10(beta_value):.3f}.png')
                visualization.draw_compression_matrix(r["matrix"], r["values"], r["counts"], out_fname)
            self.matrices[(epoch, feature_ind)] = r["matrix"]

    def on_epoch_end(self, epoch, logs=None):
        if (epoch % self.save_frequency) != 0:
            return
        from . import visualization
        dist, rank, _ = self.model._dist()
        if rank != 0:
            return
        beta_value = float(self.model.beta.value())
        self.betas[epoch] = beta_value
        if self.one_launch:
            os.makedirs(self.outdir, exist_ok=True)
            return self._save_one_launch(epoch, beta_value)
        dims = self.model.feature_dimensionalities
        idx = np.cumsum(dims)[:-1]
        features_split = np.split(self.x_processed, idx, axis=-1)
        features_split_raw = np.split(self.x_raw, idx, axis=-1)
        os.makedirs(self.outdir, exist_ok=True)
        for feature_ind in range(self.model.number_features):
            out_fname = os.path.join(self.outdir, f'feature_{feature_ind}_log10beta_{np.log10(beta_value):.3f}.png')
            mat = visualization.save_compression_matrices(
                self.model.feature_encoders[feature_ind], features_split[feature_ind],
                out_fname if self.save_png else None, inp_features_raw=features_split_raw[feature_ind],
                model=self.model)
            self.matrices[(epoch, feature_ind)] = mat


class InfoPerFeatureCallback(Callback):
    """Information (nats) in each compression channel during training (reference models.py:188-223; the kwarg-name
    defect A3 of SURVEY App. A fixed by intent).

    Every `save_frequency` epochs, for each feature: `utils.estimate_mi_sandwich_bounds` on that feature's columns of
    the validation inputs; appends `[infonce_lower, loo_upper]` to `self.bounds` (same flat order as the reference:
    feature-major within an evaluation).  `validation_x` is the validation input matrix [N, sum d_f] (the reference
    passes a tf.data.Dataset of (x, y) and strips y, models.py:210).

    one_launch=True evaluates all features together - `model.information_per_feature(validation_x, ..., seed=epoch)`, the same
    rows and noise keys, one encoder-bank forward and one bound evaluation per chunk of batches instead of one encode, one
    bound call and one read-back per (feature, batch) - and fills `bounds` / `epochs` in the same layout."""

    def __init__(self, save_frequency, validation_x, info_bound_batch_size=1024, info_bound_number_batches=8, one_launch=False):
        super().__init__()
        self.one_launch = bool(one_launch)
        self._x_dev = None
        self.save_frequency = save_frequency
        self.validation_x = np.asarray(validation_x, dtype=np.float32)
        self.bounds = []
        self.epochs = []
        self.info_bound_batch_size = info_bound_batch_size
        self.info_bound_number_batches = info_bound_number_batches

    def on_epoch_end(self, epoch, logs=None):
        if (epoch % self.save_frequency) != 0:
            return
        if self.one_launch:
            if self._x_dev is None:   # uploaded once
                self._x_dev = self.model._ensure_engine().to_device(self.validation_x)
            b = self.model.information_per_feature(self._x_dev, self.info_bound_batch_size, self.info_bound_number_batches,
                                                   seed=epoch)
            self.bounds.extend([float(lo), float(up)] for lo, up in b)
            self.epochs.append(epoch)
            return
        from . import utils
        idx = np.cumsum(self.model.feature_dimensionalities)[:-1]
        split = np.split(self.validation_x, idx, axis=-1)
        for feature_ind in range(self.model.number_features):
            lower, upper = utils.estimate_mi_sandwich_bounds(
                self.model.feature_encoders[feature_ind], split[feature_ind],
                evaluation_batch_size=self.info_bound_batch_size,
                number_evaluation_batches=self.info_bound_number_batches, seed=epoch)
            self.bounds.append([lower, upper])
        self.epochs.append(epoch)
