"""Resource audit of the CTW level-build kernels (csrc/dib_ctw_levels.h) in the generated gfx950 code, no GPU needed.

Regression guards, pinned at what the cross-compile produces today (hipcc -O3, gfx950): eight kernels, none with scratch or
AGPRs.  The level step is bound by memory traffic and integer atomics, so what matters is that the waves of a CU are many: the
count kernel's two LDS histograms (2 x 4096 ints = 32 KB static) leave room for five workgroups of four waves per CU, the place
kernel's one (16 KB) for ten, and neither may lose that to registers (<= 64 VGPRs = 8 waves per SIMD); the per-node scan and
bottom-up kernels keep only a few values per lane.  The finalize kernel is the exception: the device's float64 lgamma for
counts beyond the host's table is inlined into it and costs it 180 VGPRs (occupancy 2).  It runs once per node, not once per
element of a level, and the level loop as a whole is measured (profiles/ctw_device_bench.json); the bound below keeps it from
growing further."""
from _isa import family, kernels  # noqa: F401  (the fixture: tests/_isa.py's one cross-compile, parsed)

NAMES = ("init", "count", "scan_reduce", "scan_blocks", "finalize", "place", "mix", "output")


def _by_name(kernels):
    fam = family(kernels, "dib_ctw_")
    assert len(fam) == len(NAMES), sorted(fam)
    out = {}
    for short in NAMES:
        (k,) = [v for n, v in fam.items() if f"dib_ctw_{short}_kernel" in n]
        out[short] = k
    return out


def test_no_kernel_of_the_level_build_uses_scratch(kernels):
    for short, k in _by_name(kernels).items():
        print(short, {m: k[m] for m in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")})
        assert k["ScratchSize"] == 0 and k["NumAgprs"] == 0, (short, k)


def test_lds_and_occupancy_as_designed(kernels):
    k = _by_name(kernels)
    assert k["count"]["LDSByteSize"] == 2 * 4096 * 4 and k["place"]["LDSByteSize"] == 4096 * 4
    assert k["scan_blocks"]["LDSByteSize"] <= 1024 * 8 + 64
    for short in ("count", "place", "mix", "scan_reduce"):
        assert k[short]["NumVgprs"] <= 64, (short, k[short]["NumVgprs"])
    assert k["count"]["Occupancy"] >= 5 and k["place"]["Occupancy"] >= 8, (k["count"]["Occupancy"], k["place"]["Occupancy"])
    for short in ("mix", "scan_reduce"):
        assert k[short]["Occupancy"] >= 8, (short, k[short]["Occupancy"])
    assert k["finalize"]["NumVgprs"] <= 192 and k["finalize"]["Occupancy"] >= 2, k["finalize"]
