"""CPU checks of DistributedIBEnsemble and the entry points behind it (include/dib_ensemble.h): the new kernels' resources in the
generated gfx950 code (no scratch, at least the occupancy of the single kernels whose bodies they run), the header declarations
against the ctypes bindings, the host-only envelope answers, the ensemble's argument checks, the per-replica beta ramp and the
map between the single model's flat layout and the ensemble's - none of which needs a device.  The resource check reads the
compiler's metadata and counts only."""
import os
import re

import numpy as np
import pytest

import dib_amd
from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)
from dib_amd import _lib, ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ensemble kernel stem -> the single kernel whose body it runs (the gather is modelled on dib_posenc_kernel's 16-row tiling)
TWINS = {"dib_ens_reparam_kl_fwd_kernel": "dib_reparam_kl_fwd_kernel", "dib_ens_reparam_kl_bwd_kernel": "dib_reparam_kl_bwd_kernel",
         "dib_ens_loss_kernel": "dib_loss_kernel", "dib_ens_posenc_rows_kernel": "dib_posenc_kernelILi16E"}
ENTRIES = {"dib_ens_supported": 6, "dib_ens_workspace_bytes": 4, "dib_ens_posenc_rows": 10, "dib_ens_reparam_kl_fwd": 13,
           "dib_ens_loss": 17, "dib_ens_reparam_kl_bwd": 11}


@pytest.mark.parametrize("stem", list(TWINS))
def test_ensemble_kernels_no_scratch_and_the_single_kernels_occupancy(kernels, stem):
    fam = {**family(kernels, "dib_ens_"), **family(kernels, "dib_reparam_kl"), **family(kernels, "dib_loss_kernel"),
           **family(kernels, "dib_posenc_kernel")}
    new = [v for k, v in fam.items() if re.search(r"\d" + stem + r"(I|P|v|E|i|\d)", k)]
    old = [v for k, v in fam.items() if re.search(r"\d" + TWINS[stem] + r"(I|P|v|E|i|\d)", k)]
    assert len(new) == 1 and len(old) == 1, (stem, len(new), len(old))
    k, twin = new[0], old[0]
    assert k["ScratchSize"] == 0, (stem, k)
    assert k["Occupancy"] >= twin["Occupancy"], (stem, k["Occupancy"], twin["Occupancy"])
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 512 // max(1, twin["Occupancy"]), (stem, k)
    assert k["mfma"] == 0


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|int64_t)\s+(dib_\w+)\(([^;]*)\);", text, re.M | re.S)}


def test_entry_points_are_declared_and_bound_and_the_abi_revision_stays():
    decl = _declared("dib_ensemble.h")
    assert set(decl) == set(ENTRIES) == set(_lib.SIGNATURES_ENSEMBLE)
    for name, arity in ENTRIES.items():
        assert len(_lib.SIGNATURES_ENSEMBLE[name][1]) == len(decl[name].split(",")) == arity, (name, "binding vs declaration")
    lib = _lib.load_library()
    assert all(hasattr(lib, name) for name in ENTRIES)
    # entry points were added, none changed
    assert _lib.ABI_VERSION == 7
    assert re.search(r"#define DIB_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "dib_hip.h")).read())
    assert dib_amd.DistributedIBEnsemble is ensemble.DistributedIBEnsemble and "DistributedIBEnsemble" in dib_amd.__all__


def test_host_envelope_answers_without_a_device():
    lib = _lib.load_library()
    # what the envelope must cover at least: 1 <= R <= 64, R F <= 65535 groups, 1 <= n <= 2048, out_dim <= 16, kinds 0, 2, 3
    for shape in ((1, 1, 1, 1, 1, 0), (64, 1023, 32, 2048, 16, 2), (20, 10, 32, 128, 1, 0), (3, 3, 6, 130, 3, 3), (5, 13107, 8, 1, 1, 0),
                  (2, 2, 1024, 2048, 1, 0)):
        assert lib.dib_ens_supported(*shape) == 1, shape
    for shape in ((0, 3, 8, 16, 1, 0), (3, 0, 8, 16, 1, 0), (64, 1024, 8, 16, 1, 0), (3, 3, 0, 16, 1, 0), (3, 3, 1025, 16, 1, 0),
                  (3, 3, 8, 0, 1, 0), (3, 3, 8, 2049, 1, 0), (3, 3, 8, 16, 0, 0), (3, 3, 8, 16, 17, 0), (3, 3, 8, 16, 1, 1),
                  (3, 3, 8, 16, 1, 4), (-1, 3, 8, 16, 1, 0)):
        assert lib.dib_ens_supported(*shape) == 0, shape
    # partials per (replica, row tile, feature) and per (replica, loss workgroup), one arrival counter per (replica, feature) and
    # per replica, rounded up to 256 bytes
    words = 3 * 1 * 2 + 3 + 3 * 3 + 3 * 5 * 3      # n = 130, E = 32: 5 row tiles of 32 rows, 1 loss workgroup
    assert words == 63 and lib.dib_ens_workspace_bytes(3, 3, 32, 130) == 256
    assert lib.dib_ens_workspace_bytes(20, 10, 32, 128) == (20 * 2 + 20 + 200 + 20 * 4 * 10 + 63) // 64 * 256
    assert lib.dib_ens_workspace_bytes(3, 3, 32, 2049) < 0 and lib.dib_ens_workspace_bytes(0, 3, 32, 16) < 0
    # a refusal comes before any pointer is looked at, and before any launch (there is no device here)
    n0 = lib.dib_launch_count()
    assert lib.dib_ens_reparam_kl_fwd(None, None, None, 0, 0, 3, 3, 8, 4096, None, None, None, None) == -4
    assert lib.dib_ens_reparam_kl_bwd(None, None, None, None, 1.0, 3, 3, 2000, 16, None, None) == -4
    assert lib.dib_ens_loss(1, None, 1, None, 1, None, 3, 3, 16, 1.0, 0, None, None, None, None, None, None) == -4
    assert lib.dib_ens_posenc_rows(None, 4, None, 3, 3, 1, 40, 16, None, None) == -4
    assert lib.dib_ens_reparam_kl_fwd(None, None, None, 0, 0, 3, 3, 8, 16, None, None, None, None) == -1
    assert lib.dib_ens_loss(0, None, 1, None, 1, None, 3, 3, 16, 1.0, 0, None, None, None, None, None, None) == -1
    assert lib.dib_launch_count() == n0


SPEC = ([1, 1, 1], [16, 16], [32], 1)


def test_ensemble_argument_checks_need_no_device(monkeypatch):
    E = dib_amd.DistributedIBEnsemble
    with pytest.raises(ValueError, match="replicas >= 1"):
        E(0, *SPEC)
    with pytest.raises(ValueError, match="one seed per replica"):
        E(3, *SPEC, init_seeds=[1, 2])
    with pytest.raises(ValueError, match="one seed per replica"):
        E(3, *SPEC, noise_seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="one seed per replica"):
        E(2, *SPEC, shuffle_seeds=[1])
    with pytest.raises(ValueError, match="same width"):
        E(2, [1, 2, 1], [16], [16], 1)
    ens = E(3, *SPEC, init_seed=10, noise_seed=20, shuffle_seed=30)
    assert (ens.init_seeds, ens.noise_seeds, ens.shuffle_seeds) == ([10, 11, 12], [20, 21, 22], [30, 31, 32])
    bce = dib_amd.losses.BinaryCrossentropy(from_logits=True)
    for bad in ("sgd", "rmsprop", dib_amd.optimizers.Adam(amsgrad=True), dib_amd.optimizers.get("adam", clipnorm=1.0),
                dib_amd.optimizers.get("adam", clipvalue=0.5), dib_amd.optimizers.get("adam", decay=1e-3),
                dib_amd.optimizers.Adam(dib_amd.schedules.ExponentialDecay(1e-3, 100, 0.9))):
        with pytest.raises(ValueError):
            ens.compile(optimizer=bad, loss=bce)
    for bad in (dib_amd.losses.BinaryCrossentropy(), dib_amd.losses.BinaryCrossentropy(from_logits=True, label_smoothing=0.1),
                dib_amd.losses.CategoricalCrossentropy(from_logits=True), "mae", dib_amd.losses.Huber(),
                dib_amd.losses.SparseCategoricalCrossentropy()):
        with pytest.raises(ValueError, match="lockstep"):
            ens.compile(optimizer="adam", loss=bad)
    for bad in (["mse"], ["accuracy", "mae"], "binary_accuracy"):
        with pytest.raises(ValueError, match="accuracy"):
            ens.compile(optimizer="adam", loss=bce, metrics=bad)
    for loss in (bce, dib_amd.losses.SparseCategoricalCrossentropy(from_logits=True), "mse"):
        assert ens.compile(optimizer="adam", loss=loss, metrics=["accuracy"]) is ens
    # fit's own argument checks come before the device is touched
    x, y = np.zeros((8, 3), np.float32), np.zeros((8, 1), np.float32)
    with pytest.raises(ValueError, match="one value per replica"):
        ens.fit(x, y, batch_size=4, epochs=1, beta_start=[0.1, 0.2])
    with pytest.raises(ValueError, match="one value per replica"):
        ens.fit(x, y, batch_size=4, epochs=1, beta_end=[0.1, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match="positive"):
        ens.fit(x, y, batch_size=4, epochs=1, beta_start=0.0)
    with pytest.raises(ValueError, match="callbacks"):
        ens.fit(x, y, batch_size=4, epochs=1, callbacks=[dib_amd.Callback()])
    monkeypatch.setenv("DIB_ENABLE_GRAPHS", "1")   # DistributedIBNet.fit's capture switch: not honoured silently
    with pytest.raises(ValueError, match="hipGraph"):
        ens.fit(x, y, batch_size=4, epochs=1)


def test_beta_ramp_is_the_annealing_callbacks_float32_values():
    b0, b1, n_pre, n_anneal, epochs = [1e-3, 5e-2, 2.0], [1.0, 0.3, 1e-4], 3, 7, 14
    ramps = ensemble.beta_ramps(b0, b1, n_pre, n_anneal, epochs, 3)
    assert ramps.dtype == np.float32 and ramps.shape == (3, epochs)

    class Model:   # what the callback assigns to
        class beta:
            got = None

            @classmethod
            def assign(cls, v):
                cls.got = v

    for r in range(3):
        cb = dib_amd.InfoBottleneckAnnealingCallback(b0[r], b1[r], n_pre, n_anneal)
        cb.set_model(Model)
        for e in range(epochs):
            cb.on_epoch_begin(e)
            assert isinstance(Model.beta.got, np.float32) and ramps[r, e].tobytes() == Model.beta.got.tobytes(), (r, e)
    # a scalar serves every replica; no annealing epochs: no ramp
    assert np.array_equal(ensemble.beta_ramps(1e-2, 1.0, 2, 6, 8, 2)[0], ensemble.beta_ramps([1e-2] * 2, [1.0] * 2, 2, 6, 8, 2)[1])
    assert np.array_equal(ensemble.beta_ramps(0.5, 0.5, 0, 0, 4, 1), np.full((1, 4), 0.5, np.float32))


@pytest.mark.parametrize("R,dims,enc,units,out,E,freq,posenc", [(3, [2, 2, 2], [17, 9], [13], 3, 6, 3, True), (1, [1] * 4, [32, 32], [64, 64], 1, 8, 5, True),
                                                                (4, [3, 3], [], [], 2, 5, 5, False)])
def test_single_layout_to_ensemble_layout_is_a_bijection(R, dims, enc, units, out, E, freq, posenc):
    spec = dict(feature_dimensionalities=dims, feature_encoder_architecture=enc, integration_network_architecture=units,
                output_dimensionality=out, use_positional_encoding=posenc, number_positional_encoding_frequencies=freq,
                activation_fn="relu", feature_embedding_dimension=E, output_activation_fn=None)
    blocks, n_single = ensemble.single_blocks(**spec)
    F, d = len(dims), dims[0]
    lay = ensemble.EnsembleLayout(blocks, n_single, R, F, d, freq if posenc else 1, enc, E, units, out)
    real = np.zeros(n_single, dtype=bool)
    for b in blocks:
        real[b["offset"]: b["offset"] + b["rows"] * b["cols"]] = True
    idx = np.stack([lay.index(r) for r in range(R)])                     # [R, n_single]
    assert (idx[:, ~real] == lay.pad).all() and (idx[:, real] != lay.pad).all()
    hit = idx[:, real].reshape(-1)
    assert hit.min() >= 0 and hit.max() < lay.n_params and len(np.unique(hit)) == hit.size, "two parameters share a position"
    # scatter then gather on a host array gives the vector back, for every replica, and nothing else moves
    rng = np.random.default_rng(R)
    buf = np.zeros(lay.n_alloc, dtype=np.float32)
    vecs = rng.standard_normal((R, n_single)).astype(np.float32) * real
    for r in range(R):
        buf[idx[r][real]] = vecs[r][real]
    for r in range(R):
        assert np.array_equal(buf[idx[r]], vecs[r])
    assert buf[lay.pad] == 0.0
    # every weight matrix sits row-major and contiguous where its chain's layer is: chain g = r F + f, one stride apart
    for b in blocks:
        if b["net"] == 0 and b["what"] == 0:
            for r in range(R):
                at = idx[r][b["offset"]: b["offset"] + b["rows"] * b["cols"]]
                assert at[0] == (r * F + b["feature"]) * lay.enc_stride + lay.enc_w[b["layer"]] and (np.diff(at) == 1).all()
    with pytest.raises(IndexError):
        lay.index(R)


def test_train_repeats_flag_and_its_argument_checks():
    from dib_amd import train
    assert train.get_args([]).repeats == 1 and train.get_args(["--repeats", "5"]).repeats == 5
    train.check_repeats_args(train.get_args([]))
    train.check_repeats_args(train.get_args(["--repeats", "5"]))
    for bad in (["--repeats", "0"], ["--repeats", "3", "--infonce_loss", "True"], ["--repeats", "3", "--info_bounds_frequency", "10"],
                ["--repeats", "3", "--save_compression_matrices_frequency", "10"], ["--repeats", "2", "--subset_information", "True"]):
        with pytest.raises(ValueError, match="--repeats"):
            train.check_repeats_args(train.get_args(bad))


def test_replica_information_plane_is_drawn(tmp_path):
    from dib_amd import visualization
    rng = np.random.default_rng(0)
    path = visualization.save_distributed_info_plane_replicas(rng.random((3, 40, 4)), rng.random((3, 40)), str(tmp_path))
    assert os.path.basename(path) == "distributed_info_plane_replicas.png" and os.path.getsize(path) > 1000
