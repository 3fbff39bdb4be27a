"""CPU checks of the batched measurement / InfoNCE entry points behind MeasurementEnsemble: their kernels' resources in the
generated gfx950 code (no scratch or spills, at least the single-replica kernels' waves per SIMD - they run the same body),
the header declarations against the ctypes bindings, and the ensemble's argument checks that need no device."""
import os
import re

import pytest

import dib_amd
from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)
from dib_amd import _lib, measurement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# batched kernel stem -> the single-replica kernel whose body it runs
TWINS = {"dib_measure_batched_fwd_kernel": "dib_measure_fwd_kernel", "dib_measure_batched_bwd_kernel": "dib_measure_bwd_kernel",
         "dib_infonce_batched_sim_kernel": "dib_infonce_sim_mfma_kernel",
         "dib_infonce_batched_lse_loss_kernel": "dib_infonce_lse_loss_kernel",
         "dib_infonce_batched_grad_kernel": "dib_infonce_grad_mfma_kernel",
         "dib_infonce_batched_grad_final_kernel": "dib_infonce_grad_final_kernel",
         "dib_infonce_batched_small_kernel": "dib_infonce_small_kernel"}


def _template_args(name):
    """the template arguments of a mangled kernel name, e.g. 'ILi2ELi4EE' ('' for a plain kernel)"""
    m = re.search(r"kernel(I(?:Li\d+E)+E)", name)
    return m.group(1) if m else ""


@pytest.mark.parametrize("stem", list(TWINS))
def test_batched_kernels_no_scratch_and_the_single_kernels_occupancy(kernels, stem):
    fam = {**family(kernels, "dib_measure"), **family(kernels, "dib_infonce")}
    new = {k: v for k, v in fam.items() if re.search(r"\d" + stem + r"(I|P|v|E)", k)}
    old = {_template_args(k): v for k, v in fam.items() if re.search(r"\d" + TWINS[stem] + r"(I|P|v|E)", k)}
    assert new and len(new) == len(old), (sorted(new), sorted(old))
    for name, k in new.items():
        twin = old[_template_args(name)]
        assert k["ScratchSize"] == 0, (name, k)
        assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 256, (name, k)
        assert k["Occupancy"] >= twin["Occupancy"], (name, k["Occupancy"], twin["Occupancy"])
        assert k["mfma"] == twin["mfma"], (name, "the same body: the same MFMA count")


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return {m.group(1): m.group(2) for m in re.finditer(r"^(?:int|int64_t)\s+(dib_\w+)\(([^;]*)\);", text, re.M | re.S)}


def test_batched_entry_points_are_declared_and_bound():
    meas, hip = _declared("dib_measure.h"), _declared("dib_hip.h")
    new_meas = {"dib_measure_batched_workspace_bytes", "dib_measure_fwd_batched", "dib_measure_bwd_batched"}
    new_hip = {"dib_infonce_batched_workspace_bytes", "dib_infonce_fwd_bwd_batched"}
    assert new_meas <= set(meas) and set(meas) == set(_lib.SIGNATURES_MEASURE)
    assert new_hip <= set(hip) and new_hip <= set(_lib.SIGNATURES)
    for name, args in [(n, meas[n]) for n in new_meas] + [(n, hip[n]) for n in new_hip]:
        sig = {**_lib.SIGNATURES, **_lib.SIGNATURES_MEASURE}[name]
        assert len(sig[1]) == len(args.split(",")), (name, "arity of the binding vs the declaration")
    # entry points were added, none changed: the ABI revision stays
    assert _lib.ABI_VERSION == 7
    assert re.search(r"#define DIB_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "dib_hip.h")).read())
    assert dib_amd.MeasurementEnsemble is measurement.MeasurementEnsemble


def test_ensemble_argument_checks_need_no_device():
    with pytest.raises(ValueError, match="replicas"):
        measurement.MeasurementEnsemble(0, input_dimensionality=2)
    with pytest.raises(ValueError, match="one seed per replica"):
        measurement.MeasurementEnsemble(3, init_seeds=[1, 2], input_dimensionality=2)
    with pytest.raises(ValueError, match="one seed per replica"):
        measurement.MeasurementEnsemble(3, noise_seeds=[1, 2, 3, 4], input_dimensionality=2)
    with pytest.raises(ValueError, match="reference_timestep"):   # the template model validates before the device check
        measurement.MeasurementEnsemble(3, input_dimensionality=1, number_states=3, reference_timestep=3)
