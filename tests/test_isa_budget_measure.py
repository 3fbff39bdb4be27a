"""Resource audit of the measurement-partition kernels (csrc/dib_measure.h) in the generated gfx950 code, no GPU needed:
no scratch, a register budget that keeps the design's 2 waves per SIMD (8-wave workgroups, one per CU at 83 KB of LDS), and
the MFMA count of the unrolled tile body (layer 1 over two E tiles, 8 x 8 tiles, 8 tiles to the logits: (16 + 64 + 8) x 4)."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


@pytest.mark.parametrize("name", ["dib_measure_fwd_kernel", "dib_measure_bwd_kernel", "dib_measure_symbolize_kernel"])
def test_measure_kernels_no_scratch_two_waves_per_simd_and_mfma_count(kernels, name):
    # "mfma" here has always counted the fp32 16 x 16 x 4 MFMAs alone
    kernels = {k: dict(v, mfma=v["mfma_16x16x4"]) for k, v in family(kernels, "dib_measure").items()}
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 256 and k["Occupancy"] >= 2, k
    assert k["mfma"] == (2 * 8 + 8 * 8 + 8) * 4, k
