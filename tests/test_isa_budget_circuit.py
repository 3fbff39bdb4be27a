"""Resource audit of the Boolean-circuit kernels (csrc/dib_circuit.h) in the generated gfx950 code, no GPU needed: no scratch
and full occupancy headroom (256-thread workgroups, small register footprints)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name", ["dib_circuit_fwd_kernel", "dib_circuit_bwd_kernel", "dib_circuit_mi_kernel"])
def test_circuit_kernels_use_no_scratch(kernels, name):
    kernels = family(kernels, "dib_circuit")
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumVgprs"] <= 64 and k["Occupancy"] >= 4, k
