"""The ISA audit's shared harness: ONE cross-compile of csrc/dib_api.hip to gfx950 assembly per pytest process, ONE parser of the
per-kernel resource statistics, and a per-kernel fingerprint of the generated code (tools/isa_diff.py compares two builds with it).

A tests/test_isa_budget*.py module does `from _isa import kernels  # noqa: F401` and writes assertions on the fixture's
{mangled name: stats}; a test about one kernel family takes `family(kernels, "dib_<family>")`.  No GPU needed: hipcc cross-compiles."""
import functools
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "distributed-information-bottleneck.github.io_amd", "csrc", "dib_api.hip")
FLAGS = ("--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only")
META = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@functools.lru_cache(maxsize=None)
def assembly():
    """The gfx950 assembly of the whole library (about a minute and a half, 22 MB): compiled once per process, whoever asks."""
    with tempfile.TemporaryDirectory(prefix="isa") as tmp:
        out = os.path.join(tmp, "dib_api.s")
        res = subprocess.run([hipcc(), *FLAGS, SRC, "-o", out], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        with open(out) as f:
            return f.read()


def _functions(text):
    """(mangled name, body up to its .Lfunc_end label, what follows up to the next function's) of every function"""
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n", text, re.M):
        end = text.find("\n.Lfunc_end", m.end() - 1)
        if end < 0:
            continue
        nxt = text.find("\n.Lfunc_end", end + 1)
        yield m.group(1), text[m.end():end + 1], text[end + 1:nxt if nxt >= 0 else len(text)]


def _count(pattern, s):
    return len(re.findall(pattern, s, re.M))


def parse(text):
    """{mangled name: stats} of every function with a NumVgprs line.  stats: the compiler's metadata (META); the MFMA and
    v_accvgpr_* counts of the body (mfma_16x16x4: the fp32 16x16x4 MFMAs alone, what tests/test_isa_budget_measure.py counts);
    loop_*: the same counts and the scratch_ instructions between the "Inner Loop Header" and the first s_cbranch after it (the
    back edge of a single-block loop), None where the function has no such header."""
    info = {}
    for name, body, tail in _functions(text):
        meta = {}
        for k, v in re.findall(r"; (%s): (\d+)" % "|".join(META), tail):
            meta.setdefault(k, int(v))
        if "NumVgprs" not in meta:
            continue
        meta["mfma"] = _count(r"^\s*v_mfma", body)
        meta["mfma_16x16x4"] = _count(r"^\s*v_mfma_f32_16x16x4", body)
        for kind in ("write", "read", "mov"):
            meta["accvgpr_" + kind] = _count(r"v_accvgpr_" + kind, body)
        lines = body.splitlines()
        head = next((i for i, l in enumerate(lines) if "Inner Loop Header" in l), None)
        meta["loop_mfma"] = meta["loop_accvgpr"] = meta["loop_scratch"] = None
        if head is not None:
            back = next((i for i in range(head, len(lines)) if "s_cbranch" in lines[i]), len(lines) - 1)
            loop = "\n".join(lines[head:back + 1])
            meta["loop_mfma"] = _count(r"^\s*v_mfma", loop)
            meta["loop_accvgpr"] = _count(r"v_accvgpr_", loop)
            meta["loop_scratch"] = _count(r"scratch_", loop)
        info[name] = meta
    return info


def fingerprint(text):
    """{mangled name: sha1 of the function's code}: its lines up to .Lfunc_end without `;` comments, blank lines and the
    function's ordinal in local labels (.LBB12_3 -> .LBB_3: a kernel added elsewhere must not rename this one's blocks)."""
    prints = {}
    for name, body, _ in _functions(text):
        code = [re.sub(r"(\.L[A-Za-z]+)\d+_", r"\1_", l.split(";", 1)[0]).strip() for l in body.splitlines()]
        prints[name] = hashlib.sha1("\n".join(l for l in code if l).encode()).hexdigest()
    return prints


def family(kernels, stem):
    """The entries of one kernel family, e.g. family(kernels, "dib_partition"): the mangled names with `stem` in them."""
    return {k: v for k, v in kernels.items() if re.fullmatch(r"_Z\w*%s\w+" % stem, k)}


@functools.lru_cache(maxsize=None)
def _kernels():
    return parse(assembly())


@pytest.fixture(scope="session")
def kernels():
    if hipcc() is None:
        pytest.skip("hipcc not available")
    return _kernels()
