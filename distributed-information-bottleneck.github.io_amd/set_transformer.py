"""Per-particle Distributed-IB set transformer on the MI355X-native path (BASELINE config 5).

Host-side mirror of the reference notebook
    complex_systems/InfoDecomp_Amorphous_plasticity_per_particle_measurements_and_set_transformer.ipynb, code cell 8:
`particle_encoder` (PositionalEncoding -> Dense(128, LeakyReLU(0.1)) x2 -> Dense(2*32), shared by all particles), the
`train_step` bottleneck (logvar - 3, reparameterised sample, KL summed over (particle, dim) and averaged over the batch),
`set_transformer` (6 x [MultiHeadAttention(12, 128)(x, x, x) -> Add -> LayerNormalization -> Dense(128, relu),
Dense(32, relu) -> Add -> LayerNormalization], tf.reduce_mean over the particle axis, Dense(256, LeakyReLU(0.1)), Dense(1)),
BCE-from-logits + beta * KL, Keras Adam, the linear learning-rate warm-up and the per-STEP log ramp of beta of the
notebook's training loop.  Same names and argument meaning as the notebook's variables.

Every FLOP runs in libdib_hip.so through the C ABI of include/dib_st.h; PyTorch only owns the device memory and there is no
CPU fallback.  What a (batch, particles) shape runs on is decided once per shape, in one place (_st_plan.decide).  At the
notebook's size (32 x 50) a training step is 38 launches: encoder and head on the row-tile MLP kernels (`dib_mlp_small_fwd` /
`_bwd`, `dib_mlp_small_head_step`), per block and direction one flash-attention launch with the q / k / v projections inside
(`dib_attention_fwd_proj` / `_bwd_proj`, up to 64 particles; beyond, `dib_attention_fwd` / `_bwd` next to projection GEMMs)
and one launch for the token-wise half (`dib_st_chain_fwd` / `_bwd`: output projection, Add + LayerNorm, feed-forward,
Add + LayerNorm; up to 4096 tokens), all blocks' weight gradients as one grouped fp32-MFMA GEMM per shape class
(`dib_gemm_grouped`), slab reduce + Keras Adam in one launch (`dib_reduce_adam_step`).  Outside a kernel's envelope a stage
takes its general path: grouped GEMMs for every product (attention="gemm" or key_dim != 128: the per-(neighbourhood, head)
Q K^T, P V and their four backward products as groups, probabilities in HBM), softmax / Add+LayerNorm / mean-pool /
reparameterisation+KL / loss as row kernels.

Parameters live in one flat fp32 buffer in Keras variable-creation order (`param_shapes`, the order of
`particle_encoder.trainable_variables + set_transformer.trainable_variables`), every block 16-byte aligned.
"""
from __future__ import annotations

import ctypes
import math
import os
from ctypes import c_void_p
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import _st_plan
from ._gemm_plan import _ptr, _ptr8
from ._lib import check
from ._st_plan import ACT_RELU, _align4, _BlockDesc  # noqa: F401  (_BlockDesc: the kernel tests build their own)

LOSS_BCE_LOGITS = 0
# Test switch: take train_step's collective branch even on a ONE-rank process group, so that the RCCL calls themselves run
# on the single GPU the test box has (tests/_dp_gpu_st_worker.py).  A 1-rank sum all-reduce is the identity.
_FORCE_DP_BRANCH = False


def convert_to_per_particle_feature_set(particle_positions, types, number_particles_to_use=60):
    """Notebook cell 6: per-particle features (x, x^2, r, log r, log x^2, unit vector, one-hot type), nearest particles
    first.  Host-side data preparation (NumPy), done once per dataset."""
    pos = np.asarray(particle_positions, dtype=np.float32)
    types = np.asarray(types).astype(np.int32)
    one_hot = np.eye(2, dtype=np.float32)[types - 1]
    radii = np.sqrt(np.sum(np.square(pos), -1, keepdims=True) + np.float32(1e-10)).astype(np.float32)
    unit = pos / radii
    feats = np.concatenate([pos, pos ** 2, radii, np.log(radii + np.float32(1e-3)), np.log(pos ** 2 + np.float32(1e-3)),
                            unit, one_hot], -1).astype(np.float32)
    if number_particles_to_use > 0:
        order = np.argsort(np.squeeze(radii, -1), kind="stable")
        feats = feats[order][:number_particles_to_use]
    return feats


def notebook_probe_grid(grid_bound: float = 3.0, grid_side_length: int = 100) -> np.ndarray:
    """Cell 8's probe positions: a grid_side_length x grid_side_length grid on [-grid_bound, grid_bound]^2, [side^2, 2] float32."""
    xx, yy = np.meshgrid(np.linspace(-grid_bound, grid_bound, grid_side_length), np.linspace(-grid_bound, grid_bound, grid_side_length))
    return np.stack([xx, yy], -1).reshape([-1, 2]).astype(np.float32)


def _gaussian_filter1d(x, sigma: float, truncate: float = 4.0) -> np.ndarray:
    """scipy.ndimage.gaussian_filter1d(x, sigma) (mode "reflect", truncate 4) for 1-D x; the result keeps x's dtype."""
    x = np.asarray(x)
    if x.size == 0 or sigma <= 0:
        return x.copy()
    r = int(truncate * float(sigma) + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / float(sigma)) ** 2)
    k /= k.sum()
    xp = np.pad(x.astype(np.float64), r, mode="symmetric")   # scipy's "reflect" = numpy's "symmetric"
    return np.convolve(xp, k, mode="valid").astype(x.dtype)


def information_plane(hist, entropy_y: float = 1.0, smoothing_sigma: float = 1) -> Dict[str, np.ndarray]:
    """The tail of notebook cell 8 on a fit(track_information=True) history: BCE and bounds to bits, BCE and accuracy
    smoothed with gaussian_filter1d(sigma), info_in = mean of the two bounds (already x particles), info_out = entropy_y - BCE
    over the evaluations that have bounds.  Returns the arrays the notebook plots and saves."""
    bce_series_val = np.float32(hist["bce_series_val"]) / np.log(2)
    acc_series_val = np.float32(hist["acc_series_val"])
    info_bounds = np.float32(hist["info_bounds"]).reshape(-1, 2) / np.log(2)
    info_in = np.mean(info_bounds, axis=-1)
    bce_smoothed = _gaussian_filter1d(bce_series_val, smoothing_sigma)
    acc_smoothed = _gaussian_filter1d(acc_series_val, smoothing_sigma)
    start = -len(info_in)
    return dict(info_in=info_in, info_out=entropy_y - bce_smoothed[start:], acc=acc_smoothed[start:],
                validation_bce=bce_series_val, acc_validation=acc_series_val, info_bounds=info_bounds)


def save_information_plane(hist, path: str, entropy_y: float = 1.0, smoothing_sigma: float = 1, info_in_plot_lims=(0, 40),
                           title: Optional[str] = None) -> None:
    """The notebook's information-plane figure (info out and validation accuracy against total information in, bits)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    ip = information_plane(hist, entropy_y, smoothing_sigma)
    fig = plt.figure(figsize=(10, 6))
    ax = plt.gca()
    ax.plot(ip["info_in"], ip["info_out"], lw=4, color="k")
    ax.set_ylim(0, None)
    ax.set_xlim(list(info_in_plot_lims))
    ax.set_xlabel("Total information into model (bits)", fontsize=15)
    ax.set_ylabel("Info out (bits)", fontsize=15)
    ax2 = ax.twinx()
    ax2.plot(ip["info_in"], ip["acc"], lw=2, color="b")
    ax2.set_ylabel("ACC (validation)", color="b", fontsize=15)
    if title:
        plt.title(title, fontsize=15)
    fig.savefig(path)
    plt.close(fig)


def save_information_map(grids, path: str, masks=None, info_cmap: str = "gist_heat_r") -> None:
    """The notebook's per-type information maps (mean of the two bounds, bits) side by side; grids [types, side^2 or side x
    side, 2] nats; masks (optional) [types][side, side] of 1 / NaN (the notebook blanks the centre from the g(r) files)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    grids = np.asarray(grids, dtype=np.float64)
    side = int(round(math.sqrt(grids.shape[1] if grids.ndim == 3 else grids.shape[1] * grids.shape[2])))
    fig = plt.figure(figsize=(9 * len(grids), 8))
    for t, g in enumerate(grids):
        img = np.mean(g.reshape(side, side, 2), axis=-1) / np.log(2)
        if masks is not None:
            img = masks[t] * img
        plt.subplot(1, len(grids), t + 1)
        plt.imshow(img, info_cmap)
        plt.axis("off")
        plt.colorbar()
    fig.savefig(path)
    plt.close(fig)


class SetTransformerDIB:
    """`particle_encoder` + `set_transformer` + `train_step` of the notebook as one device-resident object."""

    def __init__(self, particle_feature_dimensions: int = 12, number_positional_encoding_frequencies: int = 5,
                 particle_encoder_arch_spec: Sequence[int] = (128, 128), bottleneck_dimension: int = 32, key_dim: int = 128,
                 number_heads_per_mha: int = 12, number_attention_blocks: int = 6,
                 ff_arch_per_block: Sequence[int] = (128, 32), final_processing_arch: Sequence[int] = (256,),
                 output_dimensionality: int = 1, logvar_initialization: float = -3.0, layer_norm_epsilon: float = 1e-3,
                 *, init_seed: int = 0, noise_seed: int = 0, device: Optional[str] = None, attention: str = "auto",
                 attention_score_stash_bytes: int = 64 << 30, use_graphs: Optional[bool] = None,
                 skinny_k_min_tokens: int = 1024):
        """use_graphs: replay the whole training step (copy-in, its 38 launches at the notebook's size, Adam, noise-step bump)
        as one captured hipGraph per (batch, particles) shape - the notebook's own configuration, 32 neighbourhoods x 50 particles, is bound by launch
        and dependency latency, not by arithmetic.  Default: the DIB_ENABLE_GRAPHS=1 opt-in shared with DistributedIBNet.fit.
        Single-process only (the data-parallel step has collectives between its launches).
        attention_score_stash_bytes: flash attention keeps the raw [P, P] score tiles of every block for the backward
        (4 tile products per tile pair instead of 5, include/dib_st.h) when all blocks' tiles of a batch shape fit this budget
        (4 x 4096 particles: 19.3 GB of the 288); above it - or with 0 - the backward recomputes them.
        attention: "flash" = dib_attention_fwd/bwd (probabilities never in HBM; key_dim must be 128), "gemm" = the products as
        grouped GEMMs with the [P, P] probabilities stashed in HBM (any key_dim), "auto" (per batch shape, key_dim == 128):
        flash - since the round-2 rewrite of the attention kernels it is the faster path at every measured shape (ms/step flash
        vs gemm: 32 x 50: 3.08 / 4.14, 4 x 512: 4.29 / 4.88, 2 x 2048: 15.0 / 15.7, 4 x 4096: 77.2 / 100.5;
        profiles/r02am_set_transformer_bench.txt, r02final2_set_transformer_bench.txt) and it needs no [P, P] stash in HBM; key_dim != 128: gemm.
        skinny_k_min_tokens: token count from which the q / k / v projections and the context gradient run as streaming
        skinny-K launches (same-box A/B, profiles/r03ad_*: 400 tokens +1.5 %, 1024 -1 %, 1600 -1.7 %, 2048 -5.7 %,
        16 384 -1 % of the step)."""
        self._acquire_device(device)
        self.particle_feature_dimensions = int(particle_feature_dimensions)
        self.number_positional_encoding_frequencies = int(number_positional_encoding_frequencies)
        self.particle_encoder_arch_spec = [int(u) for u in particle_encoder_arch_spec]
        self.bottleneck_dimension = int(bottleneck_dimension)
        self.key_dim, self.number_heads_per_mha = int(key_dim), int(number_heads_per_mha)
        self.number_attention_blocks = int(number_attention_blocks)
        self.ff_arch_per_block = [int(u) for u in ff_arch_per_block]
        assert self.ff_arch_per_block[-1] == self.bottleneck_dimension, "the feed-forward block must return to the model width"
        self.final_processing_arch = [int(u) for u in final_processing_arch]
        self.output_dimensionality = int(output_dimensionality)
        self.logvar_initialization = float(logvar_initialization)
        self.layer_norm_epsilon = float(layer_norm_epsilon)
        self.noise_seed = int(noise_seed)
        if attention not in ("auto", "flash", "gemm"):
            raise ValueError(f"attention={attention!r}")
        if attention == "flash" and self.key_dim != 128:
            raise ValueError("attention='flash' needs key_dim == 128 (the notebook's value)")
        self.attention = attention
        self.attention_score_stash_bytes = int(attention_score_stash_bytes)
        self.skinny_k_min_tokens = int(skinny_k_min_tokens)
        # A/B switches of the dispatch (_st_plan.decide reads them when it plans a shape: set them before the first step of
        # that shape).  Each names a path that is taken where its kernels support the shape; off = the general path.
        self.use_chain = True                   # the token-wise half of a block as one launch per direction (dib_st_chain_*)
        self.defer_wgrads = True                # all blocks' weight gradients at the end of the backward, grouped by shape class
        self.deferred_max_slabs = 8             # ... their row slabs over the tokens at most (each costs the optimizer a pass)
        self.deferred_wgrad_target_wgs = 1536   # ... and the workgroups one of those launches aims at
        self.encoder_row_tiles = True           # the particle encoder on the row-tile MLP kernels (dib_mlp_small_fwd / _bwd)
        self.head_row_tiles = True              # the head's share of a training step as one launch (dib_mlp_small_head_step)
        self.attention_proj = True              # q / k / v projections inside the attention forward (<= 64 particles)
        self.attention_bwd_proj = True          # ... and their input gradient inside the attention backward
        self.attention_impl = "flash" if (attention == "flash" or (attention == "auto" and self.key_dim == 128)) else "gemm"
        assert self.bottleneck_dimension <= 256 and self.bottleneck_dimension % 4 == 0
        # ---- flat parameter layout (Keras creation order) ----
        self.shapes = self.param_shapes()
        self.offsets: Dict[str, int] = {}
        o = 0
        for name, shp in self.shapes.items():
            self.offsets[name] = o
            o = _align4(o + int(np.prod(shp)))
        self.n_alloc = o
        self.n_params = int(sum(int(np.prod(s)) for s in self.shapes.values()))
        fdt = self.state_dtype
        z = lambda n, dt=fdt: torch.zeros(n, dtype=dt, device=self.device)
        self.params, self.grads, self.adam_m, self.adam_v = z(o), z(o), z(o), z(o)
        self.beta_dev = torch.ones(1, dtype=fdt, device=self.device)
        self.lr_dev = torch.full((1,), 1e-4, dtype=fdt, device=self.device)
        self.t_dev = z(1, torch.int64)
        self.set_params(self.init_params(init_seed))
        self._plans: Dict[Tuple[int, int], dict] = {}
        self.max_step_plans = 4
        self.max_graphs = 4                # captured step graphs kept (each pins its plan, workspace and score stash)
        self.use_graphs = (os.environ.get("DIB_ENABLE_GRAPHS", "0") == "1") if use_graphs is None else bool(use_graphs)
        self._graphs: Dict[Tuple[int, int], dict] = {}
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)   # noise step of graph replays (uint32 bits)
        self._step = 0
        self.last = {}
        self._unreduced: Optional[dict] = None   # the plan whose slabs loss_and_backward(reduce=False) left for the optimizer
        self._sync: Optional[torch.Tensor] = None      # dib_reduce_adam_step's grid-sync words, allocated by its first call
        self._info_ws: Optional[torch.Tensor] = None   # float64 workspace of the information estimators, grown on demand

    state_dtype = torch.float32   # parameters, gradients and Adam moments live on the device in the reference's own precision

    def _acquire_device(self, device: Optional[str]) -> None:
        """The GPU and the HIP library: there is no CPU path.  (The device steps - forward, loss_and_backward, _loss_only,
        adam_step - and this method are what tests/_oracle_set_transformer.py overrides in a subclass to run the HOST logic of
        train_step / fit on the float64 checker.)"""
        if not torch.cuda.is_available():
            raise RuntimeError("SetTransformerDIB needs an AMD GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.lib = _lib.load_library()
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")

    # ---- parameters ---------------------------------------------------------------------------------------------
    def param_shapes(self) -> Dict[str, tuple]:
        """Keras creation order.  Kernels [in, out]; MultiHeadAttention kernels [dim, heads, key_dim] / [heads, key_dim, dim]."""
        s: Dict[str, tuple] = {}
        d_in = self.particle_feature_dimensions * self.number_positional_encoding_frequencies
        for l, u in enumerate(self.particle_encoder_arch_spec + [2 * self.bottleneck_dimension]):
            s[f"enc{l}_w"], s[f"enc{l}_b"] = (d_in, u), (u,)
            d_in = u
        D, H, K = self.bottleneck_dimension, self.number_heads_per_mha, self.key_dim
        for b in range(self.number_attention_blocks):
            for nm in ("q", "k", "v"):
                s[f"blk{b}_{nm}_w"], s[f"blk{b}_{nm}_b"] = (D, H, K), (H, K)
            s[f"blk{b}_o_w"], s[f"blk{b}_o_b"] = (H, K, D), (D,)
            s[f"blk{b}_ln1_g"], s[f"blk{b}_ln1_b"] = (D,), (D,)
            d = D
            for l, u in enumerate(self.ff_arch_per_block):
                s[f"blk{b}_ff{l}_w"], s[f"blk{b}_ff{l}_b"] = (d, u), (u,)
                d = u
            s[f"blk{b}_ln2_g"], s[f"blk{b}_ln2_b"] = (D,), (D,)
        d = D
        for l, u in enumerate(self.final_processing_arch):
            s[f"fin{l}_w"], s[f"fin{l}_b"] = (d, u), (u,)
            d = u
        s["out_w"], s["out_b"] = (d, self.output_dimensionality), (self.output_dimensionality,)
        return s

    def init_params(self, seed: int = 0) -> Dict[str, np.ndarray]:
        """Keras defaults: glorot-uniform kernels (receptive-field fan convention for the attention einsum kernels), zero
        biases, LayerNormalization gamma = 1, beta = 0."""
        rng = np.random.default_rng(seed)
        p = {}
        for name, shp in self.shapes.items():
            if name.endswith("_g"):
                a = np.ones(shp)
            elif name.endswith("_b"):
                a = np.zeros(shp)
            else:
                if len(shp) == 2:
                    fan_in, fan_out = shp
                elif "_o_w" in name:
                    fan_in, fan_out = shp[0] * shp[1], shp[2]
                else:
                    fan_in, fan_out = shp[0], shp[1] * shp[2]
                lim = math.sqrt(6.0 / (fan_in + fan_out))
                a = rng.uniform(-lim, lim, size=shp)
            p[name] = a.astype(np.float32)
        return p

    def set_params(self, p: Dict[str, np.ndarray]) -> None:
        flat = np.zeros(self.n_alloc, dtype=np.float32)
        for name, shp in self.shapes.items():
            a = np.asarray(p[name], dtype=np.float32).reshape(-1)
            assert a.size == int(np.prod(shp)), name
            flat[self.offsets[name]: self.offsets[name] + a.size] = a
        self.params.copy_(torch.from_numpy(flat).to(self.params.dtype))

    def _unflatten(self, t: torch.Tensor) -> Dict[str, np.ndarray]:
        flat = t.detach().cpu().numpy()
        return {name: flat[self.offsets[name]: self.offsets[name] + int(np.prod(shp))].reshape(shp).copy()
                for name, shp in self.shapes.items()}

    def get_params(self) -> Dict[str, np.ndarray]:
        return self._unflatten(self.params)

    def get_grads(self) -> Dict[str, np.ndarray]:
        return self._unflatten(self.grads)

    @property
    def trainable_variables(self) -> List[torch.Tensor]:
        """particle_encoder.trainable_variables + set_transformer.trainable_variables: views into the flat buffer."""
        return [self.params[self.offsets[n]: self.offsets[n] + int(np.prod(s))].view(*s) for n, s in self.shapes.items()]

    def reset_optimizer(self):
        self.adam_m.zero_()
        self.adam_v.zero_()
        self.t_dev.zero_()

    # ---- plan: workspace map + descriptor tables for a (batch, particles) shape ------------------------------------------
    def _stream(self):
        return c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _plan(self, B: int, P: int) -> dict:
        """The step plan of a (batch, particles) shape - workspace map, descriptor tables, dispatch decisions
        (_st_plan.build_step_plan) - from the LRU cache.  A plan holds the whole step workspace + the gradient slabs (166 MB at
        4 x 4096): the few most recent shapes are kept (training batch, validation batch, a ragged tail)."""
        key = (B, P)
        if key in self._plans:
            self._plans[key] = self._plans.pop(key)   # most recently used last
            return self._plans[key]
        plan = _st_plan.build_step_plan(self, B, P)
        step_keys = [k for k in self._plans if k[0] != "enc" and k not in self._graphs]   # a captured graph pins its plan
        if len(step_keys) >= self.max_step_plans:
            self._plans.pop(step_keys[0])
        self._plans[key] = plan
        return plan

    def _ensure_stash(self, pl) -> bool:
        """Flash-attention score stash of plan `pl` (one buffer per attention block; 19.3 GB for 4 x 4096 particles x 6 blocks),
        allocated on first use.  It is granted only if (a) all blocks' tiles of this shape plus the stashes of every other live
        plan fit `attention_score_stash_bytes`, (b) the device has that much memory free (free HBM + what the caching
        allocator holds unused, less a 1 GiB reserve) and (c) the allocation itself succeeds; otherwise the plan stays in
        recompute mode (pl["stash_denied"] says why) - a fallback in MEMORY POLICY only, the same kernels run."""
        if pl["stash"] is not None:
            return True
        if pl["stash_block_bytes"] <= 0 or pl["stash_denied"] is not None:
            return False
        need = pl["stash_block_bytes"] * self.number_attention_blocks
        live = sum(q["stash_block_bytes"] * self.number_attention_blocks for q in self._plans.values()
                   if isinstance(q, dict) and q.get("stash") is not None)
        if live + need > self.attention_score_stash_bytes:
            pl["stash_denied"] = f"budget: {live} live + {need} needed > attention_score_stash_bytes = {self.attention_score_stash_bytes}"
            return False
        free, _total = torch.cuda.mem_get_info(self.device)
        cached = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if need > free + cached - (1 << 30):
            pl["stash_denied"] = f"memory: {need} needed, {free} free + {cached} cached on the device"
            return False
        bufs = []
        try:
            for _ in range(self.number_attention_blocks):
                bufs.append(torch.empty(pl["stash_block_bytes"] // 4, dtype=torch.float32, device=self.device))
        except torch.cuda.OutOfMemoryError:
            del bufs
            torch.cuda.empty_cache()
            pl["stash_denied"] = "memory: allocation failed"
            return False
        pl["stash"] = bufs
        return True

    def _f32(self, a, to_device: bool = True) -> torch.Tensor:
        """array or tensor -> float32 tensor on the model's device (to_device=False: a tensor stays what and where it is)"""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return t.to(device=self.device, dtype=torch.float32) if to_device else t

    def _view(self, plan, name, *shape):
        o = plan["off"][name]
        return plan["ws"][o: o + int(np.prod(shape))].view(*shape)

    # ---- forward (notebook train_step, forward part) -------------------------------------------------------------------
    def forward(self, batch_inp, step: Optional[int] = None, deterministic: bool = False, row0: int = 0,
                embs_reparam=None, _step_from_device: bool = False, for_backward: bool = True,
                _skip_head: bool = False) -> torch.Tensor:
        """embs = particle_encoder(batch_inp); logvar - 3; reparameterised sample; kl; loci_prediction = set_transformer(u).
        batch_inp [B, P, particle_feature_dimensions].  Returns the logits [B, out]; self.last holds kl (device scalar).
        embs_reparam [B, P, bottleneck] (optional): use these sampled embeddings instead of the library's counter-based
        noise (the notebook evaluates `set_transformer(tf.random.normal(...))` on its own samples; also how the golden
        fixture, which carries its own noise, is replayed).
        for_backward=False (evaluation passes): the flash attention does not write its score stash (3.2 GB per block at
        4 x 4096 particles); a loss_and_backward after such a forward recomputes the scores instead.
        Backward after any of the three forwards is consistent with it: the bottleneck's noise term is recovered as
        eps * sigma = x0 - mu from the sample that was actually used (dib_token_reparam_kl_bwd) - library noise, an injected
        sample (treated as mu + sigma * eps with its implied eps held fixed: the reparameterised gradient of that sample), or
        the deterministic forward (x0 = mu: the term vanishes).  (Round 2 regenerated the library's eps in the backward, which
        was silently wrong for the last two - advisor finding.)"""
        x = self._f32(batch_inp).contiguous()
        B, P, F0 = x.shape
        assert F0 == self.particle_feature_dimensions
        pl = self._plan(B, P)
        use_stash = bool(for_backward) and pl["impl"] == "flash" and self._ensure_stash(pl)
        lib, st, ws, off, g = self.lib, self._stream(), pl["ws"], pl["off"], pl["g"]
        T, D = pl["T"], self.bottleneck_dimension
        step = self._step if step is None else int(step)
        self._view(pl, "feats", T, F0).copy_(x.view(T, F0))
        ne = len(pl["enc_units"])
        em = pl["enc_mlp"]
        if em is not None:
            check(lib.dib_mlp_small_fwd(ctypes.byref(em["desc"]), _ptr(self.params), _ptr(ws, off["feats"]), F0, None, T,
                                        _ptr(ws, off["pe"]), em["h"], _ptr(ws, off[f"enc_h{ne - 1}"]), st), "dib_mlp_small_fwd")
        else:
            check(lib.dib_positional_encoding(_ptr(ws, off["feats"]), F0, T, F0, self.number_positional_encoding_frequencies,
                                              _ptr(ws, off["pe"]), st), "dib_positional_encoding")
            for l in range(ne):
                g[f"enc{l}_fwd"].run(lib, st)
        check(lib.dib_token_reparam_kl_fwd(_ptr(ws, off[f"enc_h{ne - 1}"]), T, D, self.logvar_initialization, self.noise_seed,
                                           step & 0xFFFFFFFF, _ptr(self.step_dev) if _step_from_device else c_void_p(0),
                                           int(row0), 1 if deterministic else 0, _ptr(ws, off["x0"]),
                                           _ptr(ws, off["kl_sum"]), _ptr(ws, off["kl_ws"]), st), "dib_token_reparam_kl_fwd")
        if embs_reparam is not None:
            self._view(pl, "x0", T, D).copy_(self._f32(embs_reparam).reshape(T, D))
        scale = 1.0 / math.sqrt(self.key_dim)
        H = self.number_heads_per_mha
        for b in range(self.number_attention_blocks):
            xin = "x0" if b == 0 else f"b{b - 1}_x"
            pre = f"blk{b}_"
            if not pl["attn_proj"]:
                g[f"b{b}_qkv_fwd"].run(lib, st)
            if pl["impl"] == "gemm":
                g[f"b{b}_qk"].run(lib, st)
                check(lib.dib_softmax_rows_fwd(_ptr(ws, off[f"b{b}_S"]), B * H * P, P, pl["ldS"], scale, st), "dib_softmax_rows_fwd")
                g[f"b{b}_pv"].run(lib, st)
            else:
                HK = H * self.key_dim
                if pl["attn_proj"]:   # q, k, v = the block input's projections, computed (and written) by the attention launch
                    wo, bo = pl["qkv_off"][b]
                    check(lib.dib_attention_fwd_proj(_ptr(ws, off[xin]), D, _ptr(self.params), wo, bo, B, P, H, self.key_dim, D, HK, scale,
                                                     _ptr(ws, off[f"b{b}_q"]), _ptr(ws, off[f"b{b}_k"]), _ptr(ws, off[f"b{b}_v"]),
                                                     _ptr(ws, off[f"b{b}_ctx"]), _ptr(ws, off[f"b{b}_lse"]), st), "dib_attention_fwd_proj")
                else:
                    check(lib.dib_attention_fwd(_ptr(ws, off[f"b{b}_q"]), _ptr(ws, off[f"b{b}_k"]), _ptr(ws, off[f"b{b}_v"]), B, P, H,
                                                self.key_dim, HK, scale, _ptr(ws, off[f"b{b}_ctx"]), _ptr(ws, off[f"b{b}_lse"]),
                                                _ptr(pl["stash"][b]) if use_stash else c_void_p(0), st), "dib_attention_fwd")
            if pl["chain"]:   # output projection -> Add + LN -> feed-forward -> Add + LN: one launch (16-token tiles)
                ffp = (c_void_p * 3)(*[_ptr(ws, off[f"b{b}_ff{l}"]) for l in range(len(self.ff_arch_per_block))])
                check(lib.dib_st_chain_fwd(ctypes.byref(pl["chain"][b]), T, _ptr(self.params), _ptr(ws, off[f"b{b}_ctx"]),
                                           _ptr(ws, off[xin]), _ptr(ws, off[f"b{b}_h"]), _ptr(ws, off[f"b{b}_xhat1"]),
                                           _ptr(ws, off[f"b{b}_rstd1"]), ffp, _ptr(ws, off[f"b{b}_x"]), _ptr(ws, off[f"b{b}_xhat2"]),
                                           _ptr(ws, off[f"b{b}_rstd2"]), st), "dib_st_chain_fwd")
                continue
            g[f"b{b}_o_fwd"].run(lib, st)
            ks = pl["ksplit"]   # split-K output projection: its slabs are the second addend
            check(lib.dib_add_layernorm_fwd(_ptr(ws, off[xin]), _ptr(ws, off["ksplit_ws"] if ks > 1 else off[f"b{b}_mha"]),
                                            max(ks, 1), T * D, T, D,
                                            _ptr(self.params, self.offsets[pre + "ln1_g"]), _ptr(self.params, self.offsets[pre + "ln1_b"]),
                                            self.layer_norm_epsilon, _ptr(ws, off[f"b{b}_h"]), _ptr(ws, off[f"b{b}_xhat1"]),
                                            _ptr(ws, off[f"b{b}_rstd1"]), st), "dib_add_layernorm_fwd")
            for l in range(len(self.ff_arch_per_block)):
                g[f"b{b}_ff{l}_fwd"].run(lib, st)
            last_ff = f"b{b}_ff{len(self.ff_arch_per_block) - 1}"
            check(lib.dib_add_layernorm_fwd(_ptr(ws, off[f"b{b}_h"]), _ptr(ws, off[last_ff]), 1, 0, T, D,
                                            _ptr(self.params, self.offsets[pre + "ln2_g"]), _ptr(self.params, self.offsets[pre + "ln2_b"]),
                                            self.layer_norm_epsilon, _ptr(ws, off[f"b{b}_x"]), _ptr(ws, off[f"b{b}_xhat2"]),
                                            _ptr(ws, off[f"b{b}_rstd2"]), st), "dib_add_layernorm_fwd")
        xl = "x0" if self.number_attention_blocks == 0 else f"b{self.number_attention_blocks - 1}_x"
        check(lib.dib_mean_pool_fwd(_ptr(ws, off[xl]), B, P, D, _ptr(ws, off["pool"]), st), "dib_mean_pool_fwd")
        # (_skip_head: a training step whose loss_and_backward runs the head's forward itself, in its one-launch head step -
        # the returned logits are then those of the PREVIOUS call until loss_and_backward has run)
        if not (_skip_head and pl["head_mlp"] is not None):
            for l in range(len(self.final_processing_arch)):
                g[f"fin{l}_fwd"].run(lib, st)
            g["out_fwd"].run(lib, st)
        self.attention_impl = pl["impl"]   # what this batch shape ran on (reporting)
        self.last = dict(plan=pl, step=step, row0=int(row0), B=B, P=P, stash=use_stash,
                         kl=self._view(pl, "kl_sum", 1) / B)   # "sum over dimension and particles, avg over batch"
        return self._view(pl, "pred", B, self.output_dimensionality)

    # ---- loss + backward ----------------------------------------------------------------------------------------------
    def loss_and_backward(self, is_loci, inv_global_batch: Optional[float] = None, reduce: bool = True) -> None:
        """bce_losses = mean BCE(is_loci, logits); loss = bce_losses + beta_var * kl; tape.gradient(loss, variables).
        Gradients land in self.grads; self.last gets bce (device scalar).  reduce=False: the batch-slab partials are left for
        adam_step(fused_reduce=True), which sums them in the optimizer's own launch (dib_reduce_adam_step)."""
        pl = self.last["plan"]
        B, P, T = self.last["B"], self.last["P"], pl["T"]
        lib, st, ws, off, g = self.lib, self._stream(), pl["ws"], pl["off"], pl["g"]
        D, H = self.bottleneck_dimension, self.number_heads_per_mha
        y = self._f32(is_loci).reshape(B, -1).contiguous()
        inv = 1.0 / B if inv_global_batch is None else float(inv_global_batch)
        gt = pl["gt"]
        if pl["nsplit"] == 1:
            self.grads.zero_()  # blocks are overwritten; alignment gaps stay zero
        dw = bool(pl["deferred_wgrads"])
        hm = pl["head_mlp"]
        if hm is not None:
            # the head's whole share of the step in one launch: hidden layers, logit, BCE, dL/dlogit, dgrad chain down to the
            # pooled embedding, the output layer's gradient and {loss sum, #correct, loss sum * inv} (csrc/dib_small.h)
            check(lib.dib_mlp_small_head_step(ctypes.byref(hm["desc"]), _ptr(self.params), _ptr(ws, off["pool"]), B, _ptr(y), y.stride(0),
                                              LOSS_BCE_LOGITS, inv, hm["h"], hm["g"], _ptr(ws, off["pred"]), _ptr(ws, off["g_pred"]),
                                              _ptr(ws, off["g_pool"]), _ptr(gt), _ptr(ws, off["out3"]), _ptr(hm["ws"]), st),
                  "dib_mlp_small_head_step")
            if dw:
                g["head_wgrads"].run(lib, st)
            else:
                for l in range(len(self.final_processing_arch) - 1, -1, -1):
                    g[f"fin{l}_wgrad"].run(lib, st)
        else:
            check(lib.dib_loss_rows(LOSS_BCE_LOGITS, _ptr(ws, off["pred"]), self.output_dimensionality, _ptr(y), y.stride(0), B, inv,
                                    _ptr(ws, off["g_pred"]), _ptr(ws, off["out3"]), _ptr(ws, off["loss_ws"]), st), "dib_loss_rows")
            # head (deferred weight gradients: the dgrad chain first, then ONE grouped launch for the head's weight gradients)
            if not dw:
                g["out_wgrad"].run(lib, st)
            g["out_dgrad"].run(lib, st)
            for l in range(len(self.final_processing_arch) - 1, -1, -1):
                if not dw:
                    g[f"fin{l}_wgrad"].run(lib, st)
                g[f"fin{l}_dgrad"].run(lib, st)
            if dw:
                g["head_wgrads"].run(lib, st)
        check(lib.dib_mean_pool_bwd(_ptr(ws, off["g_pool"]), B, P, D, _ptr(ws, off["g_x"]), st), "dib_mean_pool_bwd")
        scale = 1.0 / math.sqrt(self.key_dim)
        nff = len(self.ff_arch_per_block)
        for b in range(self.number_attention_blocks - 1, -1, -1):
            pre = f"blk{b}_"
            gin, gout = _st_plan.block_grad_names(self.number_attention_blocks, b)
            if pl["chain"]:
                # LN2 backward -> feed-forward dgrads -> LN1 backward -> output-projection dgrad in one launch; then the attention
                # backward, ONE grouped launch for the block's weight gradients, and the projections' dgrads (added to gout)
                # (deferred weight gradients, dw: the block's weight-gradient operands stay in buffers of its own)
                gq, gk, gv = pl["grad_names"][b]["qkv"]
                ffp = (c_void_p * 3)(*[_ptr(ws, off[f"b{b}_ff{l}"]) for l in range(nff)])
                gfp = (c_void_p * 3)(*[_ptr(ws, off[nm]) for nm in pl["grad_names"][b]["ff"]])
                # deferred: the gradient of this block's output is [LN1-addend gradient | q/k/v input-gradient slabs] of the
                # NEXT block, summed by the kernel as it loads its tile; the last block's comes from the pooling backward
                from_slabs = dw and b + 1 < self.number_attention_blocks
                check(lib.dib_st_chain_bwd(ctypes.byref(pl["chain"][b]), T, _ptr(self.params),
                                           _ptr(ws, off[f"b{b + 1}_dx"] if from_slabs else off[gin]),
                                           (1 + (H if pl["attn_bwd_proj"] else 3 * pl["ksplit"])) if from_slabs else 1,
                                           T * D if from_slabs else 0,
                                           _ptr(ws, off[f"b{b}_xhat2"]), _ptr(ws, off[f"b{b}_rstd2"]), ffp,
                                           _ptr(ws, off[f"b{b}_xhat1"]), _ptr(ws, off[f"b{b}_rstd1"]), gfp,
                                           _ptr(ws, off[f"b{b}_gln1" if dw else gout]),
                                           _ptr(ws, off["g_ctx"]), _ptr(gt), _ptr(ws, off["chain_ws"]), st), "dib_st_chain_bwd")
                if not dw:
                    g[f"b{b}_ff_wgrad"].run(lib, st)
                    g[f"b{b}_o_wgrad"].run(lib, st)
                if pl["attn_bwd_proj"]:
                    # dq, dk, dv AND the head's share of the projections' input gradient (slab 1 + head of the block's dx region)
                    HK = H * self.key_dim
                    check(lib.dib_attention_bwd_proj(_ptr(ws, off[f"b{b}_q"]), _ptr(ws, off[f"b{b}_k"]), _ptr(ws, off[f"b{b}_v"]),
                                                     _ptr(ws, off["g_ctx"]), _ptr(ws, off[f"b{b}_lse"]), B, P, H, self.key_dim, D, HK, scale,
                                                     _ptr(ws, off[gq]), _ptr(ws, off[gk]), _ptr(ws, off[gv]),
                                                     _ptr(self.params), pl["qkv_off"][b][0], _ptr(ws, off[f"b{b}_dx"]), T * D, st),
                          "dib_attention_bwd_proj")
                    if b == 0:   # block 0's total goes to the buffer the bottleneck's backward reads
                        check(lib.dib_reduce_splits(_ptr(ws, off["b0_dx"]), T * D, 1 + H, T * D, _ptr(ws, off[gout]), st),
                              "dib_reduce_splits")
                    continue
                self._attention_backward(pl, b, B, P, H, scale, gq, gk, gv)
                if not dw:
                    g[f"b{b}_qkv_wgrad"].run(lib, st)
                g[f"b{b}_qkv_dgrad"].run(lib, st)
                if pl["ksplit"] == 1:
                    for nm in "qkv":
                        check(lib.dib_add_inplace(_ptr(ws, off[gout]), _ptr(ws, off[f"g_x{nm}"]), T * D, st), "dib_add_inplace")
                continue
            # x_out = LN2(h + ff): gin -> g_a (gradient of both addends) and, in the same pass, g_z = g_a * relu'(ff output)
            # (the feed-forward branch's pre-activation gradient), d(gamma2, beta2)
            check(lib.dib_add_layernorm_bwd_fused(_ptr(ws, off[gin]), c_void_p(0), _ptr(ws, off[f"b{b}_xhat2"]),
                                                  _ptr(ws, off[f"b{b}_rstd2"]), _ptr(self.params, self.offsets[pre + "ln2_g"]), T, D,
                                                  _ptr(ws, off["g_a"]), _ptr(ws, off[f"b{b}_ff{nff - 1}"]), ACT_RELU,
                                                  _ptr(ws, off["g_z"]), _ptr(gt, self.offsets[pre + "ln2_g"]), _ptr(ws, off["ln_ws"]),
                                                  st), "dib_add_layernorm_bwd_fused")
            for l in range(nff - 1, -1, -1):
                g[f"b{b}_ff{l}_wgrad"].run(lib, st)
                g[f"b{b}_ff{l}_dgrad"].run(lib, st)
            # h = LN1(x + mha): (g_h + g_a, the residual) -> gout, d(gamma1, beta1)
            check(lib.dib_add_layernorm_bwd_fused(_ptr(ws, off["g_h"]), _ptr(ws, off["g_a"]), _ptr(ws, off[f"b{b}_xhat1"]),
                                                  _ptr(ws, off[f"b{b}_rstd1"]), _ptr(self.params, self.offsets[pre + "ln1_g"]), T, D,
                                                  _ptr(ws, off[gout]), c_void_p(0), 0, c_void_p(0),
                                                  _ptr(gt, self.offsets[pre + "ln1_g"]), _ptr(ws, off["ln_ws"]), st),
                  "dib_add_layernorm_bwd_fused")
            # multi-head attention
            g[f"b{b}_o_wgrad"].run(lib, st)
            g[f"b{b}_o_dgrad"].run(lib, st)
            self._attention_backward(pl, b, B, P, H, scale)
            g[f"b{b}_qkv_wgrad"].run(lib, st)
            g[f"b{b}_qkv_dgrad"].run(lib, st)
            # gradient w.r.t. the block's input = residual (already in gout) + the three projection inputs
            if pl["ksplit"] == 1:   # (split-K: the slab reduce ADDS the three projections' gradients to gout itself)
                check(lib.dib_add_inplace(_ptr(ws, off[gout]), _ptr(ws, off["g_xq"]), T * D, st), "dib_add_inplace")
                check(lib.dib_add_inplace(_ptr(ws, off[gout]), _ptr(ws, off["g_xk"]), T * D, st), "dib_add_inplace")
                check(lib.dib_add_inplace(_ptr(ws, off[gout]), _ptr(ws, off["g_xv"]), T * D, st), "dib_add_inplace")
        # bottleneck: d(mu | raw logvar), beta * KL included
        ne = len(pl["enc_units"])
        # eps * sigma = x0 - mu: the gradient of the forward that ran (library noise, embs_reparam or deterministic)
        g_u = "g_x" if self.number_attention_blocks % 2 == 0 else "g_s"   # where the last processed block left dL/d(x0)
        check(lib.dib_token_reparam_kl_bwd(_ptr(ws, off[f"enc_h{ne - 1}"]), _ptr(ws, off[g_u]), _ptr(ws, off["x0"]), T, D,
                                           self.logvar_initialization, _ptr(self.beta_dev), inv,
                                           _ptr(ws, off[f"g_enc_h{ne - 1}"]), st), "dib_token_reparam_kl_bwd")
        em = pl["enc_mlp"]
        if em is not None:   # the encoder's dgrad chain in one launch (its weight gradients: grouped, on the stashes)
            check(lib.dib_mlp_small_bwd(ctypes.byref(em["desc"]), _ptr(self.params), _ptr(ws, off[f"g_enc_h{ne - 1}"]), em["h"], em["g"],
                                        T, st), "dib_mlp_small_bwd")
        for l in range(ne - 1, -1, -1):
            if not dw:   # (deferred: three more groups of the feed-forward class's launch below)
                g[f"enc{l}_wgrad"].run(lib, st)
            if l > 0 and em is None:
                g[f"enc{l}_dgrad"].run(lib, st)
        for name in pl["deferred_wgrads"]:   # every block's weight gradients, one grouped launch per shape class
            g[name].run(lib, st)
        self._unreduced = pl if (pl["nsplit"] > 1 and not reduce) else None
        if pl["nsplit"] > 1 and reduce:
            check(lib.dib_reduce_splits(_ptr(pl["slabs"]), self.n_alloc, pl["nsplit"], self.n_alloc, _ptr(self.grads), st),
                  "dib_reduce_splits")
        out3 = self._view(pl, "out3", 3)
        self.last["bce"] = out3[2:3] if hm is not None else out3[0:1] * inv   # (the head step writes loss sum * inv itself)
        self.last["correct"] = out3[1:2]

    def _attention_backward(self, pl, b: int, B: int, P: int, H: int, scale: float, gq: str = "g_q", gk: str = "g_k",
                            gv: str = "g_v") -> None:
        """g_ctx -> g_q, g_k, g_v of block b (flash kernels, or the grouped-GEMM products with the stashed probabilities);
        gq / gk / gv name the workspace buffers that receive them (flash path)."""
        lib, st, ws, off, g = self.lib, self._stream(), pl["ws"], pl["off"], pl["g"]
        if pl["impl"] == "gemm":
            g[f"b{b}_dv"].run(lib, st)
            g[f"b{b}_dp"].run(lib, st)
            check(lib.dib_softmax_rows_bwd(_ptr(ws, off[f"b{b}_S"]), _ptr(ws, off["g_S"]), B * H * P, P, pl["ldS"], scale, st),
                  "dib_softmax_rows_bwd")
            g[f"b{b}_dq"].run(lib, st)
            g[f"b{b}_dk"].run(lib, st)
        else:
            HK = H * self.key_dim
            check(lib.dib_attention_bwd(_ptr(ws, off[f"b{b}_q"]), _ptr(ws, off[f"b{b}_k"]), _ptr(ws, off[f"b{b}_v"]),
                                        _ptr(ws, off[f"b{b}_ctx"]), _ptr(ws, off["g_ctx"]), _ptr(ws, off[f"b{b}_lse"]),
                                        _ptr(pl["stash"][b]) if self.last.get("stash") else c_void_p(0),   # as the forward ran
                                        B, P, H, self.key_dim, HK, scale, _ptr(ws, off[gq]), _ptr(ws, off[gk]), _ptr(ws, off[gv]),
                                        _ptr(ws, off["attn_delta"]), st), "dib_attention_bwd")

    def adam_step(self, beta_1=0.9, beta_2=0.999, epsilon=1e-7, fused_reduce: bool = False) -> None:
        if fused_reduce and self.n_alloc % 4 == 0:   # slab reduce + Keras-Adam + step-count bump in one launch
            pl = self._unreduced
            if self._sync is None:
                self._sync = torch.zeros(_lib.SYNC_WORDS, dtype=torch.int32, device=self.device)
            check(self.lib.dib_reduce_adam_step(_ptr(pl["slabs"]) if pl is not None else None, pl["nsplit"] if pl is not None else 0,
                                                self.n_alloc, _ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v),
                                                self.n_alloc, _ptr(self.lr_dev), _ptr(self.t_dev), beta_1, beta_2, epsilon, 1.0,
                                                _ptr(self._sync), self._stream()), "dib_reduce_adam_step")
            self._unreduced = None
            return
        pl = self._unreduced
        if pl is not None:   # (a deferred reduce that the fused path could not take)
            check(self.lib.dib_reduce_splits(_ptr(pl["slabs"]), self.n_alloc, pl["nsplit"], self.n_alloc, _ptr(self.grads),
                                             self._stream()), "dib_reduce_splits")
            self._unreduced = None
        check(self.lib.dib_adam_step(_ptr(self.params), _ptr(self.grads), _ptr(self.adam_m), _ptr(self.adam_v), self.n_alloc,
                                     _ptr(self.lr_dev), _ptr(self.t_dev), beta_1, beta_2, epsilon, 1.0, self._stream()),
              "dib_adam_step")

    def train_step(self, batch_inp, is_loci, training: bool = True):
        """The notebook's `train_step(batch_inp, is_loci, training=True)`: returns bce_losses (device scalar tensor [1]).

        Data parallel (BASELINE config 5 shards the neighbourhoods over the GPUs of a node): when torch.distributed is
        initialised every rank calls train_step with the SAME global batch; rank r takes neighbourhoods
        [r*B/N, (r+1)*B/N), the noise is keyed by the global token index (results independent of N), the flat gradient
        buffer is all-reduced (RCCL over xGMI with the nccl backend), every rank applies the same Adam update."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not _FORCE_DP_BRANCH):
            if training and self.use_graphs:
                return self._train_step_graph(batch_inp, is_loci)
            self.forward(batch_inp, for_backward=training, _skip_head=training)
            self.loss_and_backward(is_loci, reduce=False) if training else self._loss_only(is_loci)
            if training:
                self.adam_step(fused_reduce=True)
            self._step += 1
            return self.last["bce"]
        rank, world = dist.get_rank(), dist.get_world_size()
        B, P = int(batch_inp.shape[0]), int(batch_inp.shape[1])
        lo, hi = (B * rank) // world, (B * (rank + 1)) // world
        stats = torch.zeros(2, dtype=self.params.dtype, device=self.device)   # [bce sum / B, kl sum / B] of the local rows
        if hi > lo:
            self.forward(batch_inp[lo:hi], row0=lo * P, for_backward=training, _skip_head=training)
            if training:
                self.loss_and_backward(is_loci[lo:hi], inv_global_batch=1.0 / B)
            else:
                self._loss_only(is_loci[lo:hi], inv_global_batch=1.0 / B)
            stats[0:1] = self.last["bce"]
            stats[1:2] = self.last["kl"] * ((hi - lo) / B)
        elif training:
            self.grads.zero_()
        if training:
            dist.all_reduce(self.grads)        # every rank issues the same collectives, rows or no rows
        dist.all_reduce(stats)
        if training:
            self.adam_step()
        self._step += 1
        self.last["bce"], self.last["kl"] = stats[0:1], stats[1:2]
        return self.last["bce"]

    def _set_step_dev(self, value: int) -> None:
        v = int(value) & 0xFFFFFFFF
        self.step_dev.fill_(v - (1 << 32) if v >= (1 << 31) else v)   # uint32 bit pattern in an int32 tensor

    def _train_step_graph(self, batch_inp, is_loci):
        """train_step as one hipGraph replay: inputs are copied into fixed staging buffers, everything else the step reads
        that changes between replays (beta, learning rate, Adam t, the noise step) already lives in device memory.  The
        eager warm-up runs exactly the captured sequence (module loads / hipFuncSetAttribute outside the capture) and every
        piece of state it touches is restored.  Same launches in the same order as the eager step: bit-identical results."""
        x, y = self._f32(batch_inp), self._f32(is_loci)
        B, P = int(x.shape[0]), int(x.shape[1])
        g = self._graphs.get((B, P))
        if g is None:
            xs = torch.zeros((B, P, self.particle_feature_dimensions), dtype=torch.float32, device=self.device)
            ys = torch.zeros((B, self.output_dimensionality), dtype=torch.float32, device=self.device)
            xs.copy_(x.reshape(xs.shape))
            ys.copy_(y.reshape(ys.shape))
            while len(self._graphs) >= self.max_graphs:   # oldest captured shape first: its plan (and stash) becomes evictable
                torch.cuda.synchronize(self.device)      # no replay may be in flight when a graph object dies
                self._graphs.pop(next(iter(self._graphs)))
            self._graphs[(B, P)] = {}          # pins the plan against LRU eviction from here on
            try:
                self._plan(B, P)
                state = (self.params, self.adam_m, self.adam_v, self.t_dev, self.step_dev, self.grads)
                saved = [t.clone() for t in state]

                def body():
                    self.forward(xs, step=0, _step_from_device=True, _skip_head=True)
                    self.loss_and_backward(ys, reduce=False)
                    self.adam_step(fused_reduce=True)

                self._set_step_dev(self._step)
                body()
                for t, v in zip(state, saved):
                    t.copy_(v)
                torch.cuda.synchronize(self.device)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    body()
            except Exception:
                self._graphs.pop((B, P), None)   # no half-built entry: the next call starts over (or the caller goes eager)
                raise
            g = self._graphs[(B, P)] = dict(graph=graph, xs=xs, ys=ys, last=dict(self.last))
        else:
            g["xs"].copy_(x.reshape(g["xs"].shape))
            g["ys"].copy_(y.reshape(g["ys"].shape))
        self._set_step_dev(self._step)
        g["graph"].replay()
        self._step += 1
        self.last = dict(g["last"], step=self._step - 1)   # kl / bce / correct: tensors of the graph's pool, rewritten by every replay
        return self.last["bce"]

    def _loss_only(self, is_loci, inv_global_batch: Optional[float] = None):
        pl = self.last["plan"]
        B = self.last["B"]
        inv = 1.0 / B if inv_global_batch is None else float(inv_global_batch)
        y = self._f32(is_loci).reshape(B, -1).contiguous()
        ws, off = pl["ws"], pl["off"]
        check(self.lib.dib_loss_rows(LOSS_BCE_LOGITS, _ptr(ws, off["pred"]), self.output_dimensionality, _ptr(y), y.stride(0), B,
                                     inv, _ptr(ws, off["g_pred"]), _ptr(ws, off["out3"]), _ptr(ws, off["loss_ws"]),
                                     self._stream()), "dib_loss_rows")
        out3 = self._view(pl, "out3", 3)
        self.last["bce"] = out3[0:1] * inv
        self.last["correct"] = out3[1:2]

    # ---- the notebook's evaluation helpers ---------------------------------------------------------------------------------
    def particle_encoder(self, feats) -> torch.Tensor:
        """particle_encoder(features): [..., particle_feature_dimensions] -> [..., 2 * bottleneck] (mu | raw logvar)."""
        x = self._f32(feats)
        lead = x.shape[:-1]
        x = x.reshape(-1, self.particle_feature_dimensions).contiguous()
        T, F0 = x.shape[0], self.particle_feature_dimensions
        pl = self._encoder_plan(T)
        lib, st, ws, off = self.lib, self._stream(), pl["ws"], pl["off"]
        ws[off["feats"]: off["feats"] + T * F0].view(T, F0).copy_(x)
        check(lib.dib_positional_encoding(_ptr(ws, off["feats"]), F0, T, F0, self.number_positional_encoding_frequencies,
                                          _ptr(ws, off["pe"]), st), "dib_positional_encoding")
        for gg in pl["g"]:
            gg.run(lib, st)
        E2 = 2 * self.bottleneck_dimension
        o = off[f"enc_h{len(pl['g']) - 1}"]
        return ws[o: o + T * E2].view(T, E2).clone().view(*lead, E2)

    def _encoder_plan(self, T: int) -> dict:
        """Encoder-only plan behind `particle_encoder` (_st_plan.build_encoder_plan); at most a few are kept (evaluation
        batches come in a handful of sizes)."""
        key = ("enc", T)
        if key not in self._plans:
            enc_keys = [k for k in self._plans if k[0] == "enc"]
            if len(enc_keys) >= 4:
                self._plans.pop(enc_keys[0])
            self._plans[key] = _st_plan.build_encoder_plan(self, T)
        return self._plans[key]

    def probe_info_bounds(self, probe_features, data_features, seed: int = 0, step: int = 0, return_samples: bool = False):
        """One pass of the notebook's probe-grid estimator: per-probe (infonce_per, loo_per) in nats for probe particles
        `probe_features` [M, particle_feature_dimensions] against the data particles `data_features`
        [N, particle_feature_dimensions] (both encoded by `particle_encoder`, logvar - 3), on the device in float64."""
        ep = self.particle_encoder(probe_features).reshape(-1, 2 * self.bottleneck_dimension).contiguous()
        ed = self.particle_encoder(data_features).reshape(-1, 2 * self.bottleneck_dimension).contiguous()
        M, N, E = ep.shape[0], ed.shape[0], self.bottleneck_dimension
        ws = torch.empty(int(self.lib.dib_mi_probe_workspace_bytes(M, N, E)) // 8, dtype=torch.float64, device=self.device)
        rows = torch.empty((2, M), dtype=torch.float64, device=self.device)
        u = torch.empty((M, E), dtype=torch.float64, device=self.device) if return_samples else None
        check(self.lib.dib_mi_probe_bounds(_ptr8(ep), M, _ptr8(ed), N, E, self.logvar_initialization, int(seed),
                                           int(step) & 0xFFFFFFFF, 0, _ptr8(rows[0]), _ptr8(rows[1]), _ptr8(u), _ptr8(ws),
                                           self._stream()), "dib_mi_probe_bounds")
        return (rows[0], rows[1], u, ep, ed) if return_samples else (rows[0], rows[1])

    def information_map(self, particle_positions_probe, type_id: int, particle_features_val, num_eval_batches: int = 16,
                        eval_batch_size_probe_grid: int = 512, number_probes_to_eval_at_a_time: int = 100, seed: int = 0):
        """The notebook's per-particle information map for one particle type: for every probe position on the grid, the
        average over `num_eval_batches` random data batches (eval_batch_size_probe_grid neighbourhoods each, all their
        particles) of the lower / upper MI bounds.  Returns info_bounds_grid [n_probes, 2] (nats)."""
        pos = np.asarray(particle_positions_probe, dtype=np.float32)
        types = (type_id + 1) * np.ones(pos.shape[0], dtype=np.float32)
        features = convert_to_per_particle_feature_set(pos, types, number_particles_to_use=-1)
        xv = np.asarray(particle_features_val, dtype=np.float32)
        rng = np.random.default_rng(seed)
        lo_acc = torch.zeros(pos.shape[0], dtype=torch.float64, device=self.device)
        up_acc = torch.zeros_like(lo_acc)
        for probe_ind_start in range(0, pos.shape[0], number_probes_to_eval_at_a_time):
            sl = slice(probe_ind_start, min(pos.shape[0], probe_ind_start + number_probes_to_eval_at_a_time))
            for b in range(num_eval_batches):
                batch_inds = rng.choice(xv.shape[0], size=eval_batch_size_probe_grid, replace=True)
                batch_particles = xv[batch_inds].reshape(-1, self.particle_feature_dimensions)
                lo, up = self.probe_info_bounds(features[sl], batch_particles, seed=seed, step=probe_ind_start * 131 + b)
                lo_acc[sl] += lo
                up_acc[sl] += up
        return torch.stack([lo_acc, up_acc], -1).cpu().numpy() / num_eval_batches

    # ---- information tracking: one launch per estimate over the encoded validation set (include/dib_st.h dib_mi_probe_map /
    # dib_mi_sandwich_batched, csrc/dib_st_info.h) --------------------------------------------------------------------------------
    def _val_table(self, particle_features_val):
        """(particle_encoder outputs of every validation particle [N_val * P, 2E] on the device, N_val, P)."""
        xv = self._f32(particle_features_val, to_device=False)   # (particle_encoder moves it)
        if xv.dim() != 3 or xv.shape[-1] != self.particle_feature_dimensions:
            raise ValueError(f"particle_features_val must be [neighbourhoods, particles, {self.particle_feature_dimensions}], got "
                             f"{tuple(xv.shape)}")
        n_val, P = int(xv.shape[0]), int(xv.shape[1])
        enc = self.particle_encoder(xv.reshape(n_val * P, self.particle_feature_dimensions)).contiguous()
        return enc, n_val, P

    def _f64_workspace(self, nbytes: int) -> torch.Tensor:
        ws = self._info_ws
        if ws is None or ws.numel() * 8 < nbytes:
            ws = self._info_ws = torch.empty(max(int(nbytes) // 8 + 2, 2), dtype=torch.float64, device=self.device)
        return ws

    def sandwich_bounds_batched(self, table, nbhd_idx, seed: int = 0, step: int = 0, logvar_offset: Optional[float] = None,
                                return_rows: bool = False, return_samples: bool = False):
        """dib_mi_sandwich_batched on an encoded table (enc, N_val, P) and neighbourhood indices [nb, n_nbhd]: per-batch
        (lower, upper) means [nb] (nats, float64 device tensors), optionally per-row bounds [nb, n] and the samples [nb, n, E]."""
        enc, n_val, P = table
        idx = np.ascontiguousarray(nbhd_idx, dtype=np.int64)
        if idx.ndim != 2 or idx.size == 0 or idx.min() < 0 or idx.max() >= n_val:
            raise ValueError("nbhd_idx must be a non-empty [batches, neighbourhoods] array of indices into the table")
        nb, nn = idx.shape
        E = self.bottleneck_dimension
        lv = self.logvar_initialization if logvar_offset is None else float(logvar_offset)
        need = int(self.lib.dib_mi_sandwich_batched_workspace_bytes(n_val, P, E, nb, nn))
        if need < 0:
            raise ValueError(f"dib_mi_sandwich_batched: unsupported shape (batches {nb}, neighbourhoods {nn}, particles {P}, E {E})")
        ws = self._f64_workspace(need)
        idx_d = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        out = torch.empty((2, nb), dtype=torch.float64, device=self.device)
        rows = torch.empty((2, nb, nn * P), dtype=torch.float64, device=self.device) if return_rows else None
        u = torch.empty((nb, nn * P, E), dtype=torch.float64, device=self.device) if return_samples else None
        check(self.lib.dib_mi_sandwich_batched(_ptr8(enc), n_val, P, E, _ptr8(idx_d), nb, nn, lv, int(seed) & (2 ** 64 - 1),
                                               int(step) & 0xFFFFFFFF, _ptr8(out[0]), _ptr8(out[1]),
                                               _ptr8(rows[0]) if rows is not None else c_void_p(0),
                                               _ptr8(rows[1]) if rows is not None else c_void_p(0), _ptr8(u), _ptr8(ws),
                                               self._stream()), "dib_mi_sandwich_batched")
        res = (out[0], out[1])
        if return_rows:
            res += (rows[0], rows[1])
        if return_samples:
            res += (u,)
        return res

    def information_bounds(self, particle_features_val, eval_batch_size: int = 32, num_eval_batches: int = 16, seed: int = 0,
                           step: int = 0, _table=None) -> Tuple[float, float]:
        """Cell 8's "Evaluate I(U;X)": num_eval_batches batches of eval_batch_size validation neighbourhoods (drawn with
        replacement by default_rng(seed).choice), all their particles encoded (logvar - 3), cell 5's compute_infos_mus_logvars
        per batch (InfoNCE lower / leave-one-out upper over the batch's conditionals, float64, log-sum-exp; noise keyed
        (seed, step + batch, row, 0)).  Returns (mean(lower), mean(upper)) per particle in nats - the notebook stores them
        x number_particles_to_use.  The validation set is encoded once and all batches run in one launch."""
        table = _table if _table is not None else self._val_table(particle_features_val)
        rng = np.random.default_rng(seed)
        idx = np.stack([rng.choice(table[1], size=int(eval_batch_size)) for _ in range(int(num_eval_batches))])
        lo, up = self.sandwich_bounds_batched(table, idx, seed=seed, step=step)
        return float(np.mean(lo.cpu().numpy())), float(np.mean(up.cpu().numpy()))

    def information_maps(self, particle_positions_probe, particle_features_val, type_ids: Sequence[int] = (0, 1),
                         num_eval_batches: int = 16, eval_batch_size_probe_grid: int = 512,
                         number_probes_to_eval_at_a_time: int = 100, seed: int = 0, _table=None, _return_samples: bool = False):
        """information_map for several particle types at once: returns [len(type_ids), n_probes, 2] (nats); for each type the
        same index draws (default_rng(seed), chunk by chunk, batch by batch), the same noise keys and the same formulas as
        information_map(positions, type_id, particle_features_val, ..., seed=seed), with the validation set encoded once and
        every (chunk, batch) of a type in ONE launch of dib_mi_probe_map."""
        pos = np.asarray(particle_positions_probe, dtype=np.float32).reshape(-1, 2)
        table = _table if _table is not None else self._val_table(particle_features_val)
        enc, n_val, P = table
        M, C, nb, nbs = pos.shape[0], int(number_probes_to_eval_at_a_time), int(num_eval_batches), int(eval_batch_size_probe_grid)
        E = self.bottleneck_dimension
        if M <= 0 or C <= 0 or nb <= 0 or nbs <= 0:
            raise ValueError("information_maps needs probes, a chunk size, batches and a batch size > 0")
        n_chunks = (M + C - 1) // C
        steps = np.array([[(c * C * 131 + b) & 0xFFFFFFFF for b in range(nb)] for c in range(n_chunks)], dtype=np.uint32)
        steps_d = torch.from_numpy(steps.view(np.int32)).to(self.device)
        need = int(self.lib.dib_mi_probe_map_workspace_bytes(M, C, n_val, P, E, nb, nbs))
        if need < 0:
            raise ValueError(f"dib_mi_probe_map: unsupported shape (probes {M}, chunk {C}, batches {nb}, neighbourhoods {nbs}, E {E})")
        ws = self._f64_workspace(need)
        out = torch.empty((len(type_ids), 2, M), dtype=torch.float64, device=self.device)
        # information_map restarts default_rng(seed) for every type: every type sees the same draws
        rng = np.random.default_rng(seed)
        idx = np.empty((n_chunks, nb, nbs), dtype=np.int32)
        for c in range(n_chunks):
            for b in range(nb):
                idx[c, b] = rng.choice(n_val, size=nbs, replace=True)
        idx_d = torch.from_numpy(idx).to(self.device)
        samples = []
        for ti, type_id in enumerate(type_ids):
            features = convert_to_per_particle_feature_set(pos, (int(type_id) + 1) * np.ones(M, dtype=np.float32), number_particles_to_use=-1)
            ep = self.particle_encoder(features).contiguous()
            u = torch.empty((n_chunks, nb, C, E), dtype=torch.float64, device=self.device) if _return_samples else None
            check(self.lib.dib_mi_probe_map(_ptr8(ep), M, C, _ptr8(enc), n_val, P, E, _ptr8(idx_d), nb, nbs, self.logvar_initialization,
                                            int(seed) & (2 ** 64 - 1), _ptr8(steps_d), _ptr8(out[ti, 0]), _ptr8(out[ti, 1]), _ptr8(u),
                                            _ptr8(ws), self._stream()), "dib_mi_probe_map")
            samples.append((ep, u))
        grids = out.transpose(1, 2).cpu().numpy()
        return (grids, samples) if _return_samples else grids

    # ---- the notebook's training loop ------------------------------------------------------------------------------------
    @staticmethod
    def learning_rate_schedule(step: int, learning_rate: float, number_training_steps: int) -> float:
        """min(step / number_linear_ramp_lr_steps, 1) * learning_rate, number_linear_ramp_lr_steps = number_training_steps // 10."""
        return min(step / max(number_training_steps // 10, 1), 1) * learning_rate

    @staticmethod
    def beta_schedule(step: int, beta_start: float, beta_end: float, number_training_steps: int) -> float:
        """np.exp(np.log(beta_start) + float(step) / number_training_steps * (np.log(beta_end) - np.log(beta_start)))."""
        return float(np.exp(np.log(beta_start) + float(step) / number_training_steps * (np.log(beta_end) - np.log(beta_start))))

    def fit(self, particle_features_train, loci_train, number_training_steps=25_000, learning_rate=1e-4, beta_start=2e-6,
            beta_end=2e-1, batch_size=32, particle_features_val=None, loci_val=None, eval_every=None, batch_seed=0,
            verbose=False, track_information=False, eval_start=None, num_eval_batches=16, eval_batch_size=32,
            particle_positions_probe=None, eval_grid_mi_every=1000, eval_batch_size_probe_grid=512, info_seed=0, outdir=None):
        """The notebook's loop: per step ramp the learning rate, anneal beta, draw `batch_size` neighbourhoods with
        replacement, train_step; every `eval_every` steps evaluate BCE and accuracy (sign of the logit) on the validation
        neighbourhoods.  Returns dict(bce_series_val, acc_series_val, bce_series_train).
        track_information=True adds cell 8's information tracking (needs the validation set): at every evaluation from
        eval_start (default number_training_steps // 4) on, information_bounds over num_eval_batches x eval_batch_size
        neighbourhoods -> info_bounds [[P lower, P upper]] (nats, as the notebook stores them) and info_eval_steps; at those of
        them that are multiples of eval_grid_mi_every, information_maps of both particle types on particle_positions_probe
        (default: the notebook's 100 x 100 grid on [-3, 3]^2) -> information_maps {step: [2, probes, 2]}.  The evaluation draws
        from its own generators (seeded from info_seed and the step) and noise keys: the training batches, noise and optimizer
        state are those of the untracked run.  outdir: also write the notebook's history.npz (bits) and
        info_bounds_grid_{step}_type{t}.npy ([side, side, 2], nats)."""
        xtr = torch.from_numpy(np.ascontiguousarray(particle_features_train, dtype=np.float32)).to(self.device)
        ytr = torch.from_numpy(np.ascontiguousarray(loci_train, dtype=np.float32).reshape(-1, 1)).to(self.device)
        rng = np.random.default_rng(batch_seed)
        eval_every = eval_every or max(number_training_steps // 200, 1)
        hist = dict(bce_series_val=[], acc_series_val=[], bce_series_train=[], eval_steps=[])
        if track_information:
            if particle_features_val is None:
                raise ValueError("track_information needs particle_features_val")
            eval_start = number_training_steps // 4 if eval_start is None else int(eval_start)
            probes = notebook_probe_grid() if particle_positions_probe is None else np.asarray(particle_positions_probe, np.float32)
            xv_dev = torch.from_numpy(np.ascontiguousarray(particle_features_val, dtype=np.float32)).to(self.device)
            hist.update(info_bounds=[], info_eval_steps=[], information_maps={})
            if outdir:
                os.makedirs(outdir, exist_ok=True)
        for step in range(number_training_steps):
            self.lr_dev.fill_(self.learning_rate_schedule(step, learning_rate, number_training_steps))
            self.beta_dev.fill_(self.beta_schedule(step, beta_start, beta_end, number_training_steps))
            batch_inds = torch.from_numpy(rng.choice(xtr.shape[0], size=batch_size, replace=True)).to(self.device)
            bce = self.train_step(xtr[batch_inds], ytr[batch_inds])
            if step % eval_every == 0:
                hist["bce_series_train"].append(float(bce.item()))
                if particle_features_val is not None:
                    bces, right, n = [], 0.0, 0
                    xv = np.asarray(particle_features_val, dtype=np.float32)
                    yv = np.asarray(loci_val, dtype=np.float32).reshape(-1, 1)
                    for s0 in range(0, xv.shape[0], batch_size):
                        xb, yb = xv[s0: s0 + batch_size], yv[s0: s0 + batch_size]
                        bces.append(float(self.train_step(xb, yb, training=False).item()))
                        pred = self.forward(xb, for_backward=False).cpu().numpy()   # a second sampled pass, as in the notebook
                        right += float((np.sign(pred) == (yb * 2 - 1)).sum())
                        n += len(xb)
                    hist["bce_series_val"].append(float(np.mean(bces)))
                    hist["acc_series_val"].append(right / n)
                    hist["eval_steps"].append(step)
                    if verbose:
                        print(f"Step: {step}, acc : {right / n:.4f}")
                    if track_information and step >= eval_start:
                        self._track_information(hist, step, xv_dev, probes, num_eval_batches, eval_batch_size, eval_grid_mi_every,
                                                eval_batch_size_probe_grid, info_seed, outdir)
        if track_information and outdir:
            np.savez(os.path.join(outdir, "history.npz"), validation_bce=np.float32(hist["bce_series_val"]) / np.log(2),
                     acc_validation=np.float32(hist["acc_series_val"]),
                     info_bounds=np.float32(hist["info_bounds"]).reshape(-1, 2) / np.log(2))
        return hist

    def _track_information(self, hist, step, xv_dev, probes, num_eval_batches, eval_batch_size, eval_grid_mi_every,
                           eval_batch_size_probe_grid, info_seed, outdir):
        """One evaluation of fit(track_information=True): I(U;X) bounds, and on map steps both particle types' maps, from one
        encoding of the validation set at the current parameters."""
        table = self._val_table(xv_dev)
        P = table[2]
        base = (int(info_seed) << 32) + 2 * int(step)   # generator / noise seeds of this evaluation: bounds base, maps base + 1
        lo, up = self.information_bounds(None, eval_batch_size, num_eval_batches, seed=base, step=0, _table=table)
        hist["info_bounds"].append([P * lo, P * up])
        hist["info_eval_steps"].append(step)
        if step % eval_grid_mi_every == 0:
            grids = self.information_maps(probes, None, (0, 1), num_eval_batches, eval_batch_size_probe_grid, 100, seed=base + 1,
                                          _table=table)
            hist["information_maps"][step] = grids
            if outdir:
                side = int(round(math.sqrt(grids.shape[1])))
                for t in range(grids.shape[0]):
                    g = grids[t].reshape(side, side, 2) if side * side == grids.shape[1] else grids[t]
                    np.save(os.path.join(outdir, f"info_bounds_grid_{step}_type{t}.npy"), g)
