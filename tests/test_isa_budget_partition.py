"""Resource audit of the random-partition kernel (csrc/dib_partition.h) in the generated gfx950 code, no GPU needed: every
activation's instantiation has no scratch (the 8-tile layer chain of a 16-point tile stays in registers) and at most 168 registers (VGPRs + AGPRs, __launch_bounds__(256, 3)),
so that three 256-thread workgroups (one wave per SIMD each) are co-resident on a CU at the notebook's widths."""
import pytest

from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)


def test_one_instantiation_per_activation(kernels):
    kernels = family(kernels, "dib_partition")
    assert sorted(kernels) == [f"_Z30dib_partition_symbolize_kernelILi{a}EEv16DibPartitionArgs" for a in range(4)], sorted(kernels)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_partition_kernel_uses_no_scratch(kernels, act):
    k = kernels[f"_Z30dib_partition_symbolize_kernelILi{act}EEv16DibPartitionArgs"]
    assert k["ScratchSize"] == 0, k
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 168 and k["Occupancy"] >= 3, k
