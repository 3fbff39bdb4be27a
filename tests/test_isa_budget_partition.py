"""Resource audit of the random-partition kernel (csrc/dib_partition.h) in the generated gfx950 code, no GPU needed: every
activation's instantiation has no scratch (the 8-tile layer chain of a 16-point tile stays in registers) and at most 168 registers (VGPRs + AGPRs, __launch_bounds__(256, 3)),
so that three 256-thread workgroups (one wave per SIMD each) are co-resident on a CU at the notebook's widths."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-information-bottleneck.github.io_amd", "csrc", "dib_api.hip")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = next((c for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa_partition") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_partition\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        tail = text[end:end + 4000]
        info[m.group(1)] = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
    return info


def test_one_instantiation_per_activation(kernels):
    assert sorted(kernels) == [f"_Z30dib_partition_symbolize_kernelILi{a}EEv16DibPartitionArgs" for a in range(4)], sorted(kernels)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_partition_kernel_uses_no_scratch(kernels, act):
    k = kernels[f"_Z30dib_partition_symbolize_kernelILi{act}EEv16DibPartitionArgs"]
    assert k["ScratchSize"] == 0, k
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 168 and k["Occupancy"] >= 3, k
