"""Resource audit of the subset-information kernel (csrc/dib_subsets.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): one kernel, no scratch (its only array,
the powers of three, is indexed by unrolled constants), no AGPRs, no static LDS (the fold's table is dynamic LDS, at most
DIB_SUBSET_LDS_BYTES); 47 VGPRs and the occupancy 7 the compiler reports for it.  At K = 2 the 53 KB of dynamic LDS allow three
workgroups (twelve waves) per CU, so registers do not bound the kernel until they pass 64 (one workgroup's serial
walk is what bounds the launch)."""
from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


def test_subset_kernel_uses_no_scratch_and_keeps_its_occupancy(kernels):
    kernels = family(kernels, "dib_subset_")
    assert len(kernels) == 1, sorted(kernels)
    (name, k), = kernels.items()
    assert "dib_subset_fold_kernel" in name
    assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= 64 and k["Occupancy"] >= 7, k
