"""Resource audit of the compression-matrix kernels (csrc/dib_compression.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch anywhere, no AGPRs;
  dib_cmp_matrices_kernel: 112 VGPRs, occupancy 4, 26 112 B of static LDS (32 for the two 4 x 4 accumulators, 24 for the staged
                           (mu, var, logvar) of 4 + 4 rows, two dimensions in flight, the rest the division / logarithm temporaries)
  dib_cmp_gather_kernel:    13 VGPRs, occupancy 8
The guards allow a few registers of compiler drift but not the loss of an occupancy step (64 / 96 / 128 / 168 / 256 VGPRs)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name,max_vgprs,min_occupancy,lds", [("dib_cmp_matrices_kernel", 128, 4, 26112), ("dib_cmp_gather_kernel", 64, 8, 0)])
def test_compression_kernels_use_no_scratch_and_keep_their_occupancy(kernels, name, max_vgprs, min_occupancy, lds):
    kernels = family(kernels, "dib_cmp_")
    assert len(kernels) == 2, sorted(kernels)
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == lds, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
