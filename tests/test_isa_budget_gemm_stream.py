"""Resource audit of the LDS-free forward / dgrad kernel (csrc/dib_gemm_stream.h) in the generated gfx950 code - no GPU needed,
the same cross-compile as tests/test_isa_budget_wgrad_stream.py.  What the kernel's speed rests on and a source edit can lose: its
256 accumulators live in AGPRs for the whole super-block loop with no v_accvgpr_* traffic inside it, no LDS and no scratch (a
spill's reload is a vmcnt(0) in the loop), and exactly one copy of the unrolled super-block body (a second copy - a peeled last
trip, a zero-trip path - doubles the MFMA count and hands the epilogue two sources of its accumulators).  Outside the loop each
accumulator register is written once (the tile's zero-initialisation) and read once (the epilogue, through a vector register - not
moved between accumulator registers to form store operands).  It must also leave the tiled kernels it falls back to as they are."""
import pytest

from _isa import kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

BODY_MFMA = 256      # one super-block: 8 phases x 16 steps x 2 accumulators; no prologue MFMAs
ACC_REGS = 256       # 16 accumulators x 16 registers: zero-initialised (v_accvgpr_write) and read (v_accvgpr_read) once per tile
# <MODE, KIND>: forward linear / relu / leaky relu, dgrad without / with the activation mask
INSTANCES = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 3)]


@pytest.mark.parametrize("mode,kind", INSTANCES)
def test_stream_kernel_budget(kernels, mode, kind):
    hits = [k for k in kernels if f"dib_gemm_stream_kernelILi{mode}ELi{kind}EE" in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, k
    assert k["NumAgprs"] >= 256 and k["NumVgprs"] + k["NumAgprs"] <= 512, k
    assert k["loop_mfma"] == BODY_MFMA and k["mfma"] == BODY_MFMA, k     # one copy of the super-block body, nothing else multiplies
    assert k["loop_accvgpr"] == 0 and k["loop_scratch"] == 0, k
    assert k["accvgpr_write"] == ACC_REGS and k["accvgpr_read"] == ACC_REGS and k["accvgpr_mov"] == 0, k


def test_five_instantiations_and_the_tiled_kernels_are_untouched(kernels):
    assert len([k for k in kernels if "dib_gemm_stream_kernel" in k]) == len(INSTANCES)
    for mode in (0, 1, 2):
        hits = [k for k in kernels if f"dib_gemm_kernelILi{mode}ELi2ELi2ELi64E" in k]
        assert len(hits) == 1, hits
        k = kernels[hits[0]]
        assert k["mfma"] == 128 and k["NumAgprs"] == 0, k
