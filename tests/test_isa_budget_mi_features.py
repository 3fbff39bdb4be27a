"""Resource audit of the all-features MI-bound kernels (csrc/dib_mi_features.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch anywhere, no AGPRs;
  dib_mif_bounds_kernel<32>: 149 VGPRs, occupancy 3 (64 for the sample, 64 for the 16 LDS reads in flight of a block of 8 dimensions
                             of two rows, the rest the own log-density, partials and addresses)
  dib_mif_bounds_kernel<64>: 212 VGPRs, occupancy 2 (128 for the sample)
  dib_mif_bounds_kernel<0>:   89 VGPRs, occupancy 5 (the sample in LDS)
  dib_mif_table_kernel:       44 VGPRs, occupancy 8
  dib_mif_combine_kernel:     56 VGPRs, occupancy 8
The guards allow a few registers of compiler drift but not the loss of an occupancy step (64 / 96 / 168 / 256 VGPRs)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name,max_vgprs,min_occupancy", [("dib_mif_bounds_kernelILi32E", 168, 3), ("dib_mif_bounds_kernelILi64E", 256, 2),
                                                          ("dib_mif_bounds_kernelILi0E", 96, 5), ("dib_mif_table_kernel", 64, 8),
                                                          ("dib_mif_combine_kernel", 64, 8)])
def test_mi_features_kernels_use_no_scratch_and_keep_their_occupancy(kernels, name, max_vgprs, min_occupancy):
    kernels = family(kernels, "dib_mif_")
    assert len(kernels) == 5, sorted(kernels)
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
