"""Resource audit of the Monte-Carlo MI kernels (csrc/dib_mi_channel.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): no scratch anywhere;
  dib_mic_terms_kernel<32>: 143 VGPRs, occupancy 3 (64 for the sample, 64 for the 16 LDS reads in flight of a block of 8 dimensions
                            of two rows, the rest partials and addresses)
  dib_mic_terms_kernel<64>: 204 VGPRs, occupancy 2 (128 for the sample)
  dib_mic_combine_kernel:    52 VGPRs, occupancy 8
The guards allow a few registers of compiler drift but not the loss of an occupancy step (128 / 168 / 256 VGPRs)."""
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
    out = str(tmp_path_factory.mktemp("isa_mi_channel") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_mic_\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        tail = text[end:end + 4000]
        info[m.group(1)] = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
    return info


@pytest.mark.parametrize("name,max_vgprs,min_occupancy", [("dib_mic_terms_kernelILi32E", 168, 3), ("dib_mic_terms_kernelILi64E", 256, 2),
                                                          ("dib_mic_combine_kernel", 64, 8)])
def test_mi_channel_kernels_use_no_scratch(kernels, name, max_vgprs, min_occupancy):
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, (name, sorted(kernels))
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumAgprs"] == 0 and k["NumVgprs"] <= max_vgprs and k["Occupancy"] >= min_occupancy, k
