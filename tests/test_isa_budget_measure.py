"""Resource audit of the measurement-partition kernels (csrc/dib_measure.h) in the generated gfx950 code, no GPU needed:
no scratch, a register budget that keeps the design's 2 waves per SIMD (8-wave workgroups, one per CU at 83 KB of LDS), and
the MFMA count of the unrolled tile body (layer 1 over two E tiles, 8 x 8 tiles, 8 tiles to the logits: (16 + 64 + 8) x 4)."""
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
    out = str(tmp_path_factory.mktemp("isa_measure") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_measure\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        tail = text[end:end + 4000]
        meta = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
        meta["mfma"] = len(re.findall(r"^\s*v_mfma_f32_16x16x4", text[m.end():end], re.M))
        info[m.group(1)] = meta
    return info


@pytest.mark.parametrize("name", ["dib_measure_fwd_kernel", "dib_measure_bwd_kernel", "dib_measure_symbolize_kernel"])
def test_measure_kernels_no_scratch_two_waves_per_simd_and_mfma_count(kernels, name):
    hits = [k for k in kernels if name in k]
    assert len(hits) == 1, hits
    k = kernels[hits[0]]
    assert k["ScratchSize"] == 0, k
    assert k["NumVgprs"] + k.get("NumAgprs", 0) <= 256 and k["Occupancy"] >= 2, k
    assert k["mfma"] == (2 * 8 + 8 * 8 + 8) * 4, k
