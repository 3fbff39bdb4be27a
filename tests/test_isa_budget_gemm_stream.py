"""Resource audit of the LDS-free forward / dgrad kernel (csrc/dib_gemm_stream.h) in the generated gfx950 code - no GPU needed,
the same cross-compile as tests/test_isa_budget_wgrad_stream.py.  What the kernel's speed rests on and a source edit can lose: its
256 accumulators live in AGPRs for the whole super-block loop with no v_accvgpr_* traffic inside it, no LDS and no scratch (a
spill's reload is a vmcnt(0) in the loop), and exactly one copy of the unrolled super-block body (a second copy - a peeled last
trip, a zero-trip path - doubles the MFMA count and hands the epilogue two sources of its accumulators).  Outside the loop each
accumulator register is written once (the tile's zero-initialisation) and read once (the epilogue, through a vector register - not
moved between accumulator registers to form store operands).  It must also leave the tiled kernels it falls back to as they are."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-information-bottleneck.github.io_amd", "csrc", "dib_api.hip")
BODY_MFMA = 256      # one super-block: 8 phases x 16 steps x 2 accumulators; no prologue MFMAs
ACC_REGS = 256       # 16 accumulators x 16 registers: zero-initialised (v_accvgpr_write) and read (v_accvgpr_read) once per tile
# <MODE, KIND>: forward linear / relu / leaky relu, dgrad without / with the activation mask
INSTANCES = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 3)]


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
    for m in re.finditer(r"^(_Z\w*dib_gemm(?:_stream)?_kernel\w+):[^\n]*\n", text, re.M):
        end = text.find(".Lfunc_end", m.end())
        body, tail = text[m.end():end], text[end:end + 4000]
        meta = {k: int(v) for k, v in re.findall(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", tail)}
        if "NumVgprs" not in meta:
            continue
        meta["mfma"] = len(re.findall(r"^\s*v_mfma", body, re.M))
        meta["accvgpr_write"] = len(re.findall(r"v_accvgpr_write", body))
        meta["accvgpr_read"] = len(re.findall(r"v_accvgpr_read", body))
        meta["accvgpr_mov"] = len(re.findall(r"v_accvgpr_mov", body))
        lines = body.splitlines()
        head = next((i for i, l in enumerate(lines) if "Inner Loop Header" in l), None)
        if head is not None:
            back = next((i for i in range(head, len(lines)) if "s_cbranch" in lines[i]), len(lines) - 1)
            loop = "\n".join(lines[head:back + 1])
            meta["loop_mfma"] = len(re.findall(r"^\s*v_mfma", loop, re.M))
            meta["loop_accvgpr"] = len(re.findall(r"v_accvgpr_", loop))
            meta["loop_scratch"] = len(re.findall(r"scratch_", loop))
        info[m.group(1)] = meta
    return info


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
