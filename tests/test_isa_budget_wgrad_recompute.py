"""Resource audit of the recomputing layer-2 weight-gradient kernel (csrc/dib_wgrad_recompute.h) in the generated gfx950 code - no
GPU needed, the same cross-compile as tests/test_isa_budget_wgrad_stream.py.  What its speed rests on: the 256 output
accumulators in AGPRs for the whole loop, the recomputed h1 tile and its double buffer in VGPRs (its MFMAs are inline assembly
for that reason: left to the compiler they take the AGPR form and shuttle through v_accvgpr_* and scratch), no LDS, no scratch,
one copy of the ring body.  This test counts resources only."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

RING_MFMA = 256      # 16 steps x 16 MFMAs: one copy of dib_wgrad_stream_kernel<4, ...>'s ring body
RECOMPUTE_MFMA = 16  # one 32-row tile of h1: 4 sub-tiles x 4 steps, inside the ring body ...
PROLOGUE_MFMA = 16   # ... and once before the loop for the slab's first tile (the body recomputes the NEXT trip's tile)
# v_accvgpr_* of the built kernel, all outside the loop - the accumulators' zero-initialisations (+ the zero-trip copy) and the
# epilogue's first reads, the counts of dib_wgrad_stream_kernel<4, 2, ...> in the same build: 544 writes, 16 reads; inside the loop: 0
BUILT_ACC_WRITE, BUILT_ACC_READ, LOOP_ACC = 544, 16, 0


# <CH (bias chains), NTL (non-temporal loads), RELU (the fused forward's specialisation)>
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("ntl", [0, 1])
@pytest.mark.parametrize("ch", [2, 4])
def test_recompute_kernel_budget(kernels, ch, ntl, relu):
    hits = [k for k in kernels if f"dib_wgrad_h1_kernelILi{ch}ELb{ntl}ELb{relu}E" in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0 and k["NumVgprs"] + k["NumAgprs"] <= 512
    assert k["NumAgprs"] >= 256      # the accumulators' home
    assert k["loop_mfma"] == RING_MFMA + RECOMPUTE_MFMA     # one copy of the ring body
    assert k["mfma"] == RING_MFMA + RECOMPUTE_MFMA + PROLOGUE_MFMA
    assert k["loop_accvgpr"] == LOOP_ACC
    assert k["accvgpr_write"] == BUILT_ACC_WRITE and k["accvgpr_read"] == BUILT_ACC_READ, k


def test_eight_instantiations_under_their_own_name(kernels):
    kernels = family(kernels, "dib_wgrad_h1_kernel")
    assert len(kernels) == 8
    assert not [k for k in kernels if "dib_wgrad_stream_kernel" in k]     # (tests/test_isa_budget_wgrad_stream.py counts those)
