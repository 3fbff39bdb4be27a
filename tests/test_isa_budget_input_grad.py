"""Resource audit of the input-gradient kernel (csrc/dib_input_grad.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch in any instantiation (the
accurate cosf's range reduction included); the accumulators of the NB positional-encoding blocks live in 4 NB AGPRs;
  dib_input_grad_kernel<1>: 62 VGPRs + 4 AGPRs, occupancy 7   (no positional encoding)
  dib_input_grad_kernel<5>: 74 VGPRs + 20 AGPRs, occupancy 5  (the default five blocks)
  dib_input_grad_kernel<8>: 86 VGPRs + 32 AGPRs, occupancy 4
The guards allow a few registers of compiler drift but not the loss of an occupancy step."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


def test_every_instantiation_is_there_and_uses_no_scratch(kernels):
    kernels = family(kernels, "dib_input_grad_kernel")
    assert len(kernels) == 8, sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0, (name, k)


@pytest.mark.parametrize("nb,max_vgprs,min_occupancy", [(1, 68, 7), (5, 80, 5), (8, 92, 4)])
def test_register_budget(kernels, nb, max_vgprs, min_occupancy):
    hits = [k for k in kernels if f"dib_input_grad_kernelILi{nb}E" in k]
    assert len(hits) == 1, (nb, sorted(kernels))
    k = kernels[hits[0]]
    assert k["NumAgprs"] == 4 * nb and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
