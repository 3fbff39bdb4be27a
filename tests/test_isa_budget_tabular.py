"""Resource audit of the tabular front end's kernels (csrc/dib_tabular.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch, no AGPRs, no static LDS (the
staged variant's tables are dynamic LDS, at most DIB_TAB_STAGE_BYTES);
  dib_tab_quantile_kernel, dib_tab_quantile_staged_kernel: 64 VGPRs, occupancy 8 - what amdgpu_waves_per_eu(8) asks for (left
      alone the compiler keeps the 48 coefficients of the rational in registers: 130 VGPRs, occupancy 3)
The VGPR bound is the occupancy step itself: there is no drift to allow above 64 without losing it."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name", ["dib_tab_quantile_kernel", "dib_tab_quantile_staged_kernel"])
def test_tabular_kernels_use_no_scratch_and_keep_their_occupancy(kernels, name):
    kernels = family(kernels, "dib_tab_")
    assert len(kernels) == 2, sorted(kernels)
    hits = [k for k in kernels if name + "PK" in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= 64 and k["Occupancy"] >= 8, k
