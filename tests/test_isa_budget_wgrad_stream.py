"""Resource audit of the LDS-free weight-gradient kernel (csrc/dib_wgrad_stream.h) in the generated gfx950 code - no GPU
needed, the same cross-compile as tests/test_isa_budget.py.  What the kernel's speed rests on and a source edit can lose: its
accumulators (256 registers of the 128-column tile) live in AGPRs for the whole loop with no v_accvgpr_* traffic inside it, no
LDS and no scratch, and exactly one copy of the unrolled ring body (a second copy - a peeled last trip, a branch on the
cache policy - doubles the MFMA count).  It must also leave the tiled kernels the weight gradients fall back to as they are."""
import os
import re

import pytest

from _isa import SRC, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

RING = 16   # csrc/dib_wgrad_stream.h kWgsRing: MFMA steps (row pairs) in the prefetch ring = steps of the unrolled loop body


def test_ring_depth_is_the_headers():
    src = open(os.path.join(os.path.dirname(SRC), "dib_wgrad_stream.h")).read()
    assert re.search(r"constexpr int kWgsGroups = (\d+);", src).group(1) == str(RING // 4)


# <NT (columns per lane), CH (bias chains), NTL (non-temporal loads)>: MFMAs per ring step, built accvgpr_write / _read counts
@pytest.mark.parametrize("nt,ch,per_step,built_w,built_r", [(4, 2, 16, 544, 16), (4, 4, 16, 528, 16), (2, 4, 8, 256, 0)])
@pytest.mark.parametrize("ntl", [0, 1])
def test_stream_kernel_budget(kernels, nt, ch, ntl, per_step, built_w, built_r):
    hits = [k for k in kernels if f"dib_wgrad_stream_kernelILi{nt}ELi{ch}ELb{ntl}E" in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0 and k["NumVgprs"] + k["NumAgprs"] <= 512
    assert k["NumAgprs"] >= 64 * nt      # the accumulators' home
    assert k["mfma"] == per_step * RING   # one copy of the unrolled ring body, nothing else multiplies
    # zero-initialisations (+ the zero-trip copy) and the epilogue's first reads; none of them inside the loop
    assert k["accvgpr_write"] <= built_w + 16 and k["accvgpr_read"] <= built_r + 16, k


def test_six_instantiations_and_the_tiled_kernels_are_untouched(kernels):
    assert len([k for k in kernels if "dib_wgrad_stream_kernel" in k]) == 6
    for mode in (0, 1, 2):
        hits = [k for k in kernels if f"dib_gemm_kernelILi{mode}ELi2ELi2ELi64E" in k]
        assert len(hits) == 1, hits
        k = kernels[hits[0]]
        assert k["mfma"] == 128 and k["NumAgprs"] == 0 and k["LDSByteSize"] <= 80 * 1024
