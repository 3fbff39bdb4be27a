"""Resource audit of the set-transformer information kernels (csrc/dib_st_info.h) in the generated gfx950 code, no GPU needed:
every instantiation of the tiled bounds kernel (E <= 32 and E <= 64 with the sample in registers, any E <= 256 with it in LDS)
and the table / combine kernels use no scratch, and the register-resident paths leave room for several waves per SIMD."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


def _bounds(kernels, emax):
    return kernels[f"_Z21dib_sti_bounds_kernelILi{emax}EEv10DibStiArgs"]


def test_the_instantiations(kernels):
    kernels = family(kernels, "dib_sti_")
    assert sorted(k for k in kernels if "bounds" in k) == [f"_Z21dib_sti_bounds_kernelILi{e}EEv10DibStiArgs" for e in (0, 32, 64)]
    assert len(kernels) == 6, sorted(kernels)


def test_no_scratch_anywhere(kernels):
    kernels = family(kernels, "dib_sti_")
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0, (name, k)


@pytest.mark.parametrize("emax,max_regs,min_occ", [(32, 168, 3), (64, 256, 2), (0, 168, 3)])
def test_bounds_kernel_registers(kernels, emax, max_regs, min_occ):
    """E <= 32 (the notebook's 32): the 32 sampled coordinates in registers and still 3 waves per SIMD; E <= 64: 2."""
    k = _bounds(kernels, emax)
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= max_regs and k["Occupancy"] >= min_occ, k
