"""Resource audit of the Monte-Carlo MI kernels (csrc/dib_mi_channel.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch anywhere;
  dib_mic_terms_kernel<32>: 143 VGPRs, occupancy 3 (64 for the sample, 64 for the 16 LDS reads in flight of a block of 8 dimensions
                            of two rows, the rest partials and addresses)
  dib_mic_terms_kernel<64>: 204 VGPRs, occupancy 2 (128 for the sample)
  dib_mic_combine_kernel:    52 VGPRs, occupancy 8
The guards allow a few registers of compiler drift but not the loss of an occupancy step (128 / 168 / 256 VGPRs)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name,max_vgprs,min_occupancy", [("dib_mic_terms_kernelILi32E", 168, 3), ("dib_mic_terms_kernelILi64E", 256, 2),
                                                          ("dib_mic_combine_kernel", 64, 8)])
def test_mi_channel_kernels_use_no_scratch(kernels, name, max_vgprs, min_occupancy):
    kernels = family(kernels, "dib_mic_")
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
