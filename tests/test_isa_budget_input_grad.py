"""Resource audit of the input-gradient kernel (csrc/dib_input_grad.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch in any instantiation (the
accurate cosf's range reduction included); the accumulators of the NB positional-encoding blocks live in 4 NB AGPRs;
  dib_input_grad_kernel<1>: 62 VGPRs + 4 AGPRs, occupancy 7   (no positional encoding)
  dib_input_grad_kernel<5>: 74 VGPRs + 20 AGPRs, occupancy 5  (the default five blocks)
  dib_input_grad_kernel<8>: 86 VGPRs + 32 AGPRs, occupancy 4
The guards allow a few registers of compiler drift but not the loss of an occupancy step."""
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
    out = str(tmp_path_factory.mktemp("isa_input_grad") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_input_grad_kernel\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        tail = text[end:end + 4000]
        info[m.group(1)] = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
    return info


def test_every_instantiation_is_there_and_uses_no_scratch(kernels):
    assert len(kernels) == 8, sorted(kernels)
    for name, k in kernels.items():
        assert k["ScratchSize"] == 0, (name, k)


@pytest.mark.parametrize("nb,max_vgprs,min_occupancy", [(1, 68, 7), (5, 80, 5), (8, 92, 4)])
def test_register_budget(kernels, nb, max_vgprs, min_occupancy):
    hits = [k for k in kernels if f"dib_input_grad_kernelILi{nb}E" in k]
    assert len(hits) == 1, (nb, sorted(kernels))
    k = kernels[hits[0]]
    assert k["NumAgprs"] == 4 * nb and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
