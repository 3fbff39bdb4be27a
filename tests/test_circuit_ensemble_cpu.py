"""CPU checks of the batched entry points behind CircuitEnsemble: their kernels' resources in the generated gfx950 code (no
scratch, at least the single-replica kernels' waves per SIMD, the same MFMA count - they run the same body), the header
declarations against the ctypes bindings, the host-only envelope answers of the library and the ensemble's argument checks,
none of which needs a device.  The resource check reads the compiler's metadata and counts only."""
import ctypes
import os
import re

import numpy as np
import pytest

import dib_amd
from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)
from dib_amd import _lib, circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# batched kernel stem -> the single-replica kernel whose body it runs
TWINS = {"dib_circuit_batched_fwd_kernel": "dib_circuit_fwd_kernel", "dib_circuit_batched_bwd_kernel": "dib_circuit_bwd_kernel",
         "dib_circuit_batched_mi_kernel": "dib_circuit_mi_kernel",
         "dib_small_integration_batched_kernel": "dib_small_integration_kernel"}
NEW_CIRCUIT = {"dib_circuit_batched_supported": 3, "dib_circuit_fwd_batched": 18, "dib_circuit_bwd_batched": 17,
               "dib_circuit_mi_batched_workspace_bytes": 3, "dib_circuit_mi_bounds_batched": 12}
NEW_HIP = {"dib_mlp_small_head_batched_supported": 3, "dib_mlp_small_head_batched_workspace_bytes": 3,
           "dib_mlp_small_head_step_batched": 20}


@pytest.mark.parametrize("stem", list(TWINS))
def test_batched_kernels_no_scratch_and_the_single_kernels_occupancy(kernels, stem):
    fam = {**family(kernels, "dib_circuit"), **family(kernels, "dib_small_integration")}
    new = [v for k, v in fam.items() if re.search(r"\d" + stem + r"(I|P|v|E|\d)", k)]
    old = [v for k, v in fam.items() if re.search(r"\d" + TWINS[stem] + r"(I|P|v|E|\d)", k)]
    assert len(new) == 1 and len(old) == 1, (stem, len(new), len(old))
    k, twin = new[0], old[0]
    assert k["ScratchSize"] == 0, (stem, k)
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 512 // max(1, twin["Occupancy"]), (stem, k)
    assert k["Occupancy"] >= twin["Occupancy"], (stem, k["Occupancy"], twin["Occupancy"])
    assert k["mfma"] == twin["mfma"], (stem, "the same body: the same MFMA count")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|int64_t)\s+(dib_\w+)\(([^;]*)\);", text, re.M | re.S)}


def test_batched_entry_points_are_declared_and_bound():
    circ, hip = _declared("dib_circuit.h"), _declared("dib_hip.h")
    assert set(NEW_CIRCUIT) <= set(circ) and set(circ) == set(_lib.SIGNATURES_CIRCUIT)
    assert set(NEW_HIP) <= set(hip) and set(NEW_HIP) <= set(_lib.SIGNATURES)
    for name, arity in {**NEW_CIRCUIT, **NEW_HIP}.items():
        args = {**circ, **hip}[name]
        sig = {**_lib.SIGNATURES, **_lib.SIGNATURES_CIRCUIT}[name]
        assert len(sig[1]) == len(args.split(",")) == arity, (name, "arity of the binding vs the declaration")
    # entry points were added, none changed: the ABI revision stays
    assert _lib.ABI_VERSION == 7
    assert re.search(r"#define DIB_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "dib_hip.h")).read())
    assert dib_amd.CircuitEnsemble is circuit.CircuitEnsemble and "CircuitEnsemble" in dib_amd.__all__


def test_host_envelope_checks_of_the_batched_entries_answer_without_a_device():
    lib = _lib.load_library()
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    assert lib.dib_circuit_batched_supported(ints([1, 3, 16]), 3, 512) == 1
    assert lib.dib_circuit_batched_supported(ints([1, 3, 16]), 3, 2048) == 1
    for G, R, B in (([1, 0, 16], 3, 512), ([17], 1, 1), ([4], 0, 8), ([4, 4], 2, 0), ([4, 4], 2, 2049)):
        assert lib.dib_circuit_batched_supported(ints(G), R, B) == 0, (G, R, B)
    assert lib.dib_circuit_batched_supported(None, 1, 8) == 0
    one = lib.dib_circuit_mi_workspace_bytes(16, 1024, 8)
    assert one > 0 and one % 256 == 0 and lib.dib_circuit_mi_batched_workspace_bytes(5, 1024, 8) == 5 * one
    assert lib.dib_circuit_mi_batched_workspace_bytes(0, 1024, 8) < 0 and lib.dib_circuit_mi_batched_workspace_bytes(2, 1, 8) < 0
    d = circuit._predictor_desc(*circuit._flat_layout([256, 256, 256])[:3], "leaky_relu")
    single = lib.dib_mlp_small_head_workspace_bytes(ctypes.byref(d), 512)
    assert lib.dib_mlp_small_head_batched_workspace_bytes(ctypes.byref(d), 512, 6) == 6 * ((single + 63) // 64 * 64)
    assert lib.dib_mlp_small_head_batched_workspace_bytes(ctypes.byref(d), 512, 0) < 0
    assert lib.dib_mlp_small_head_batched_supported(ctypes.byref(d), 512, 0) == 0
    for R in (1, 20):   # the single entry's rule and R >= 1
        assert lib.dib_mlp_small_head_batched_supported(ctypes.byref(d), 512, R) == lib.dib_mlp_small_head_supported(ctypes.byref(d), 512)


def test_ensemble_argument_checks_need_no_device():
    t = circuit.truth_table(circuit.SI_CIRCUITS[0])
    with pytest.raises(ValueError, match="R >= 1"):
        circuit.CircuitEnsemble([])
    with pytest.raises(ValueError, match="one seed per replica"):
        circuit.CircuitEnsemble([t, t, t], init_seeds=[1, 2])
    with pytest.raises(ValueError, match="one seed per replica"):
        circuit.CircuitEnsemble([t, t, t], noise_seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="rows"):
        circuit.CircuitEnsemble([t, t[:-1]])                            # 7 rows: not a power of two
    with pytest.raises(ValueError):
        circuit.CircuitEnsemble([np.zeros((1 << 17, 18), np.int32)])    # 2^17 rows: beyond 2^16
    with pytest.raises(ValueError, match="activation"):
        circuit.CircuitEnsemble([t], activation_function="gelu6")
    with pytest.raises(ValueError, match="one value per replica"):
        circuit._per_replica([0.1, 0.2], 3, "beta")
    assert circuit._per_replica(0.5, 3, "beta") == [0.5] * 3
    # the layout does not depend on the circuit: every G shares CircuitIB's offsets
    dims, w_off, b_off, sc_off, n_params = circuit._flat_layout([256, 256, 256])
    assert dims[0] == (16, 256) and dims[-1] == (256, 1) and sc_off % 64 == 0 and n_params == sc_off + 64
