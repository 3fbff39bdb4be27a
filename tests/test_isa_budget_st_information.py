"""Resource audit of the set-transformer information kernels (csrc/dib_st_info.h) in the generated gfx950 code, no GPU needed:
every instantiation of the tiled bounds kernel (E <= 32 and E <= 64 with the sample in registers, any E <= 256 with it in LDS)
and the table / combine kernels use no scratch, and the register-resident paths leave room for several waves per SIMD."""
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
    out = str(tmp_path_factory.mktemp("isa_st_info") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_sti_\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        tail = text[end:end + 4000]
        info[m.group(1)] = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
    return info


def _bounds(kernels, emax):
    return kernels[f"_Z21dib_sti_bounds_kernelILi{emax}EEv10DibStiArgs"]


def test_the_instantiations(kernels):
    assert sorted(k for k in kernels if "bounds" in k) == [f"_Z21dib_sti_bounds_kernelILi{e}EEv10DibStiArgs" for e in (0, 32, 64)]
    assert len(kernels) == 6, sorted(kernels)


def test_no_scratch_anywhere(kernels):
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0, (name, k)


@pytest.mark.parametrize("emax,max_regs,min_occ", [(32, 168, 3), (64, 256, 2), (0, 168, 3)])
def test_bounds_kernel_registers(kernels, emax, max_regs, min_occ):
    """E <= 32 (the notebook's 32): the 32 sampled coordinates in registers and still 3 waves per SIMD; E <= 64: 2."""
    k = _bounds(kernels, emax)
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= max_regs and k["Occupancy"] >= min_occ, k
