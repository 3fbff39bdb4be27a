"""Resource audit of the recomputing layer-2 weight-gradient kernel (csrc/dib_wgrad_recompute.h) in the generated gfx950 code - no
GPU needed, the same cross-compile as tests/test_isa_budget_wgrad_stream.py.  What its speed rests on: the 256 output
accumulators in AGPRs for the whole loop, the recomputed h1 tile and its double buffer in VGPRs (its MFMAs are inline assembly
for that reason: left to the compiler they take the AGPR form and shuttle through v_accvgpr_* and scratch), no LDS, no scratch,
one copy of the ring body.  This test counts resources only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-information-bottleneck.github.io_amd", "csrc", "dib_api.hip")
RING_MFMA = 256      # 16 steps x 16 MFMAs: one copy of dib_wgrad_stream_kernel<4, ...>'s ring body
RECOMPUTE_MFMA = 16  # one 32-row tile of h1: 4 sub-tiles x 4 steps, inside the ring body ...
PROLOGUE_MFMA = 16   # ... and once before the loop for the slab's first tile (the body recomputes the NEXT trip's tile)
# v_accvgpr_* of the built kernel, all outside the loop - the accumulators' zero-initialisations (+ the zero-trip copy) and the
# epilogue's first reads, the counts of dib_wgrad_stream_kernel<4, 2, ...> in the same build: 544 writes, 16 reads; inside the loop: 0
BUILT_ACC_WRITE, BUILT_ACC_READ, LOOP_ACC = 544, 16, 0


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "dib_api.s")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", SRC, "-o", out],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    info = {}
    for m in re.finditer(r"^(_Z\w*dib_wgrad_h1_kernel\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        body, tail = text[m.end():end], text[end:end + 4000]
        meta = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", tail)}
        if "NumVgprs" not in meta:
            continue
        meta["mfma"] = len(re.findall(r"^\s*v_mfma", body, re.M))
        meta["accvgpr_write"] = len(re.findall(r"v_accvgpr_write", body))
        meta["accvgpr_read"] = len(re.findall(r"v_accvgpr_read", body))
        lines = body.splitlines()
        head = next(i for i, l in enumerate(lines) if "Inner Loop Header" in l)
        back = next(i for i in range(head, len(lines)) if "s_cbranch_scc" in lines[i])
        loop = "\n".join(lines[head:back + 1])
        meta["loop_mfma"] = len(re.findall(r"^\s*v_mfma", loop, re.M))
        meta["loop_accvgpr"] = len(re.findall(r"v_accvgpr_", loop))
        info[m.group(1)] = meta
    return info


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
    assert len(kernels) == 8
    assert not [k for k in kernels if "dib_wgrad_stream_kernel" in k]     # (tests/test_isa_budget_wgrad_stream.py counts those)
