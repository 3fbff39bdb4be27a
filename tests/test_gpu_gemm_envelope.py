"""The tiled grouped fp32 GEMM (csrc/dib_gemm.h dib_gemm_kernel<MODE, NI, NJ, BK, FLAT>) across its envelope, through the public
entries dib_gemm_grouped, dib_gemm and dib_wgrad_grouped - and the slab reducers dib_reduce_splits / dib_reduce_splits_add.  The
kernel is the building block of every path without a fused kernel and the root of trust of the streaming kernels' bit-identity
tests; here it is held to an independent reference.

Exact data.  fp32 MFMA is an fmaf chain; with operands k/8, |k| <= 16, every product is a multiple of 1/64 of magnitude <= 4 and
every partial sum is exact while 64 max(|A| |B| + |bias|) < 2^24 (test_case_data_is_exact holds the table to that bound).  The
result then does not depend on the summation order, the tile shape or the split, so modes 0 / 1 / 2 with the activation ids 0, 1, 2
and 7 are compared for EQUALITY (as values: -0.0 == 0.0) with the float32 cast of the float64 reference (leaky ids: one float32
rounding, slope * z); a weight gradient's slabs and bias sums are compared slab by slab and summed in float64.  A dropped, doubled
or misplaced k-term, a wrong bias column or a swapped row is a difference of at least 1/64.  Ids 3..6 (tanh, sigmoid, elu,
softplus) go through the device's libm: float64 formula at the building-block tolerance 2e-5 (1 + max |ref|), with two bias
columns at +-100 for the saturated branches.

Guards.  Every operand and the output lie in arenas with leading dimensions wider than the extents and guard rows before, between
and after the groups' blocks (tests/_gemm_cases.py build_buffers).  The operands' guards are NaN - one stray load poisons an
output; the output arena is pre-filled with a NaN of a fixed payload and every element outside the groups' [M, N] and [N] blocks
must still hold that bit pattern.  Nothing is ever accessed outside an allocation (test_blocks_lie_inside_their_arenas).
(Two things no output can show: a weight-gradient tile with tm > 0 that also wrote its bias sums would store the same values to
the same place, and a ragged last tile that is NOT shifted back to the edge computes the same values on the bounds-checked path.)

Variants.  tests/_gemm_cases.py restates the host's tile rule (csrc/host/gemm.h launch_gemm, wgrad_tile_rule) and gives each case
the tuning keys / group count under which the rule picks the variant the case is there for; on the GPU the library's live profile
must show exactly one launch, in that variant's category."""
import ctypes

import numpy as np
import pytest

import _gemm_cases as gc
from _gemm_cases import CASES, REDUCE_CASES, TARGETS

DIB_E_ARG = -1      # include/dib_hip.h

# Edges of the M / N axes the host can never launch on a variant (csrc/host/gemm.h): N <= 64 always gets 64-column tiles and N > 64
# never gets the 128 x 64 tile; a weight gradient with M <= 64 always gets 64-row tiles, one with M > 64 and N <= 64 the 128 x 64 tile;
# the flat tile's shape class is M <= 32, N >= 256.
UNREACHABLE = {
    "g0-22": {"N=1"}, "g0-12": {"N=1"}, "g0-21": {"N=B+1", "N=B+4", "N=2B+3"},
    "g1-22": {"N=1"}, "g1-12": {"N=1"}, "g1-21": {"N=B+1", "N=B+4", "N=2B+3"},
    "g2-22": {"M=1", "N=1"}, "g2-12": {"N=1"}, "g2-21": {"M=1", "N=B+1", "N=B+4", "N=2B+3"},
    "g2-12-flat": {"M=B+1", "M=B+4", "M=2B+3", "N=1", "N=B-1"}, "g2-12-noflat": {"M=B+1", "M=B+4", "M=2B+3", "N=1", "N=B-1"},
}


# =================================================================================================================================
# CPU: the table itself
# =================================================================================================================================
def _tuned(case, key, default):
    return dict(case.tuning).get(key, default)


def _of(target):
    entry, mode, ni, nj, flat = target
    return [c for c in CASES.values() if (c.entry, c.mode, c.variant, c.flat) == (entry, mode, (ni, nj), flat)]


def test_every_case_takes_the_variant_it_names():
    for c in CASES.values():
        got = gc.tile_rule(c.mode, c.max_m, c.max_n, len(c.groups), c.nsplit, _tuned(c, "fwd_small_wgs", 512),
                           _tuned(c, "fwd_narrow_wgs", 1024))
        if c.entry != "gemm":        # (dib_gemm has one instantiation per mode)
            assert got == c.variant, (c.name, got)
        if c.flat is not None:
            assert c.max_m <= 32 and c.max_n >= 256 and _tuned(c, "wgrad_flat_tile", 1) == int(c.flat), c.name
        elif c.mode == 2 and c.entry != "gemm":
            assert not (c.max_m <= 32 and c.max_n >= 256), c.name
        for g in c.groups:
            assert g.M >= 1 and g.N >= 1 and g.K >= 1
            if c.entry == "gemm":
                # dib_gemm times the LDS-free kernel (csrc/host/gemm.h gemm_stream_plan) in the same profile category: no case may
                # qualify for it, or the launch count could not tell which kernel ran
                assert g.M % 128 or g.N % 128 or g.K % 32 or g.M < 8192, c.name
            if c.mode == 1 and c.use_aux and not c.tags & {"act-sweep"}:
                assert c.act != 0, c.name
        assert set(dict(c.tuning)) <= set(gc.TUNING_KEYS)


def test_solver_finds_a_launch_exactly_where_the_rule_allows_one():
    """`feasible` states what the rule hard-wires (e.g. a forward with N <= 64 never gets 128-column tiles); the search over group
    counts and tuning keys must agree with it, so an edge missing from the table is one the host can never launch."""
    for mode, ni, nj in gc.VARIANTS:
        for M in (1, 63, 64, 65, 127, 128, 129, 132, 259, 643, 1153):
            for N in (1, 63, 64, 65, 68, 127, 128, 132, 259, 515):
                assert (gc.solve(mode, ni, nj, M, N) is not None) == gc.feasible(mode, ni, nj, M, N), (mode, ni, nj, M, N)


def test_case_table_reaches_every_branch():
    tags = lambda cases: set().union(*(c.tags for c in cases))
    for target in TARGETS:
        entry, mode, ni, nj, flat = target
        cases = _of(target)
        t = tags(cases)
        assert cases, target
        bm, bn, bk = gc.shape_dims(target)
        assert all(c.dims == gc.tile_dims(mode, ni, nj, bool(flat), entry) for c in cases)
        # every edge of every axis the rule lets this variant see, one axis at a time around the base
        for lab, shape in gc.edge_shapes(target):
            assert (lab in t) == (shape is not None), (target, lab)
        assert {f"K={lab}" for lab in gc.K_LABELS} <= t, target
        # ... and the edges it does not: stated here, independently of `feasible`
        missing = {f"{ax}={lab}" for ax, b in (("M", bm), ("N", bn)) for lab in gc.M_LABELS} - t
        assert missing == UNREACHABLE.get(gc._tname(*target), set()), (target, sorted(missing))
        if mode != 2:
            assert "M=xcd" in t and ("lds" in t) == (entry == "grouped" and (ni, nj) == (2, 2)) and ("direct" in t) != ("lds" in t)
            assert {f"act{a}" for a in gc.EXACT_SLOPE} <= t, target
            if (ni, nj) in ((2, 2), (1, 1)):
                assert {f"act{a}" for a in gc.INEXACT_ACTS} <= t, target
        else:
            # a ragged last tile shifted back to the edge (extent % 4 == 0) and on the bounds-checked path, for M and for N
            if flat is None:
                assert {"M-shifted", "M-checked"} <= t, target
            if nj == 2:
                assert {"N-shifted", "N-checked"} <= t, target
        if entry == "grouped":
            assert "nt-pair" in t, target
    assert "corner=1" in tags(CASES.values())
    for mode in (0, 1, 2):
        for variant in ((2, 2), (1, 1)):        # (2, 2) at BK = 64: the LDS epilogue of modes 0 / 1; (1, 1): a direct epilogue
            sel = [c for c in CASES.values() if c.mode == mode and c.variant == variant and c.entry == "grouped"]
            assert all(c.lds == (mode != 2 and variant == (2, 2)) and c.dims[2] == (64 if variant == (2, 2) else 32) for c in sel)
            t = tags(sel)
            ops = ("a", "b", "c") + (("aux",) if mode == 1 else ())
            assert {f"{k}-{op}" for k in ("off", "ld") for op in ops} <= t, (mode, variant)
            for op in ops:
                for k in ("off", "ld"):
                    assert {f"{k}{r}" for r in (1, 2, 3)} <= tags(c for c in sel if f"{k}-{op}" in c.tags), (mode, variant, k, op)
            assert {"all-misaligned", "k-odd-aligned"} <= t, (mode, variant)
        rag = [c for c in CASES.values() if c.mode == mode and "ragged" in c.tags]
        assert len({c.variant for c in rag}) >= 2
        for c in rag:
            base = c.groups[:4]
            assert len({(g.M, g.N, g.K) for g in base}) == 4 and any(not g.bias for g in base), c.name
            assert c.max_m == max(g.M for g in base) and c.max_n == max(g.N for g in base)
            if mode == 2:
                assert any(g.K < c.rps for g in base) and c.nsplit > 1, c.name
    # the contraction of a weight gradient
    for target in [tg for tg in TARGETS if tg[1] == 2 and tg[0] == "grouped" and tg[4] is not False]:
        cases = _of(target)
        t = tags(cases)
        assert {"slabs-whole", "rps37", "rps100", "short-last-slab", "empty-slab"} <= t, target
        assert any(c.nsplit == 1 for c in cases)
        for c in cases:
            if c.tags & {"slabs-whole", "rps37", "rps100", "empty-slab"}:
                assert any(g.bias for g in c.groups) and any(not g.bias for g in c.groups), c.name
                last = c.slab_rows(c.groups[0], c.nsplit - 1)
                if "empty-slab" in c.tags:
                    assert last[0] >= c.groups[0].K and last[0] == last[1]
                if "short-last-slab" in c.tags:
                    assert 0 < last[1] - last[0] < c.rps
                if "rps37" in c.tags or "rps100" in c.tags:
                    assert c.rps % c.dims[2] and (c.rps % 4 or "rps100" in c.tags)    # (37: no multiple of 4 either)
    # the cache policy: one output of >= 256 MB per mode on the LDS epilogue, streamed rows above the default threshold
    for mode in (0, 1):
        big = [c for c in CASES.values() if "big" in c.tags and c.mode == mode]
        assert len(big) == 1 and big[0].lds and big[0].max_m >= 8192
        assert big[0].max_m * big[0].max_n * 4 >= 256 << 20
    assert sum("big" in c.tags for c in CASES.values()) == 2
    w = [c for c in CASES.values() if c.entry == "wgrad"]
    assert len(w) == 1 and len({g.K for g in w[0].groups}) == 1
    assert any("nomask" in c.tags and c.lds for c in CASES.values()) and any("nomask" in c.tags and not c.lds for c in CASES.values())


def _small(c):
    return "big" not in c.tags


def test_case_data_is_exact():
    """Section "Exact data" of the module docstring, case by case: operands k/8 with |k| <= 16 (the two saturating bias columns of
    the ids 3..6 aside: +-800/8), the bound with a margin of 16, the mask's +0.0 / -0.0 entries."""
    for c in CASES.values():
        data = gc.make_data(c)
        for g, d in zip(c.groups, data):
            assert gc.is_dyadic(d["A"]) and gc.is_dyadic(d["B"]), c.name
            if d["bias"] is not None:
                assert gc.is_dyadic(d["bias"], 2.0 if c.exact else 100.0), c.name
            if d["aux"] is not None and c.exact:
                x = d["aux"]
                assert gc.is_dyadic(x), c.name
                if x.size > 1:
                    z = x[x == 0]
                    assert np.signbit(z).any() and not np.signbit(z).all(), c.name
            if d["aux"] is not None and not c.exact:
                x, lo, hi = d["aux"], {3: -1, 4: 0, 5: -1, 6: 0}[c.act], {3: 1, 4: 1, 5: np.inf, 6: np.inf}[c.act]
                assert (x > lo).all() and (x < hi).all(), c.name
        assert gc.exactness_margin(c, data) >= 16, c.name


def test_blocks_lie_inside_their_arenas():
    """By construction, re-checked: every element a launch may touch is inside its allocation, the groups' blocks do not overlap,
    and there are guard elements before the first and after the last block."""
    for c in filter(_small, CASES.values()):
        b = gc.build_buffers(c, gc.make_data(c))
        batch = b["batch"]
        for g, d in zip(c.groups, b["descs"]):
            K = g.K
            ra, ca = (g.M, K) if c.mode != 2 else (K, g.M)
            rb, cb = (K, g.N) if c.mode != 1 else (g.N, K)
            for buf, off, ld, r, cc in ((b["A"], d["a_off"] + d["a_boff"] * batch, d["lda"], ra, ca),
                                        (b["B"], d["b_off"] + d["b_boff"] * batch, d["ldb"], rb, cb),
                                        (b["C"], d["c_off"] + d["c_boff"] * batch, d["ldc"], g.M, g.N)):
                assert ld > cc and off >= 8 and off + (r - 1) * ld + cc + 8 <= (buf.size if buf is not b["C"] else b["stride"]), c.name
            if b["aux"] is not None:
                assert d["ldaux"] > g.N and 8 <= d["aux_off"] and d["aux_off"] + (g.M - 1) * d["ldaux"] + g.N + 8 <= b["aux"].size
            if d["bias_off"] >= 0:
                lim = b["bias"].size if c.mode == 0 else b["stride"]
                assert 8 <= d["bias_off"] and d["bias_off"] + g.N + 8 <= lim, c.name
        n_written = sum(g.M * g.N + (g.N if c.mode == 2 and g.bias else 0) for g in c.groups) * (c.nsplit if c.mode == 2 else 1)
        assert int(b["written"].sum()) == n_written, c.name        # no two blocks share an element
        assert np.isnan(b["A"]).sum() == b["A"].size - sum(g.M * g.K for g in c.groups), c.name
        assert np.isnan(b["B"]).sum() == b["B"].size - sum(g.N * g.K for g in c.groups), c.name
        assert (b["C"] == gc.GUARD_BITS).all()


def test_reference_notices_a_wrong_element():
    """check_output on a correct buffer passes; one output off by 1/64, one stray store, one missing store each fail."""
    c = CASES["g2-12-slabs-rps37"]
    data = gc.make_data(c)
    b = gc.build_buffers(c, data)
    good = b["C"].copy().view(np.float32)
    for g, dat, (c_pos, ldc, bias_pos) in zip(c.groups, data, b["place"]):
        for s, (want, want_b) in enumerate(gc.expected(c, g, dat)):
            gc._fill(good, s * b["stride"] + c_pos, ldc, want.astype(np.float32))
            if bias_pos >= 0:
                good[s * b["stride"] + bias_pos: s * b["stride"] + bias_pos + g.N] = want_b
    good = good.view(np.int32)
    gc.check_output(c, b, data, good)
    c_pos = b["place"][0][0]
    for pos, val in ((c_pos + 1, None), (c_pos - 1, 0), (c_pos, gc.GUARD_BITS)):
        bad = good.copy()
        if val is None:
            bad.view(np.float32)[pos] += np.float32(1 / 64)
        else:
            bad[pos] = val
        with pytest.raises(AssertionError):
            gc.check_output(c, b, data, bad)


# =================================================================================================================================
# GPU
# =================================================================================================================================
def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off) if t is not None else None


@pytest.fixture
def gpu():
    """(lib, _lib module, torch); restores the tuning keys the cases touch and leaves the profile off"""
    import torch
    from dib_amd import _lib as L
    lib = L.load_library()
    saved = {k: L.get_tuning(k) for k in gc.TUNING_KEYS}
    yield lib, L, torch
    lib.dib_profile_enable(0)
    for k, v in saved.items():
        L.set_tuning(k, v)


def _launch(case, bufs, gpu, tuning=()):
    """One launch of the case -> (the whole output arena as int32, {profile name: launches})"""
    from dib_amd._gemm_plan import DESC, _Gemm
    from dib_amd.engine import profile_summary
    lib, L, torch = gpu
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    up = lambda a: torch.from_numpy(a).cuda() if a is not None else None
    A, B, bias, aux, C = up(bufs["A"]), up(bufs["B"]), up(bufs["bias"]), up(bufs["aux"]), up(bufs["C"])
    descs, mode = bufs["descs"], case.mode
    for k, v in tuple(case.tuning) + tuple(tuning):
        L.set_tuning(k, v)
    if case.entry == "grouped":
        gm = _Gemm(mode, descs, A, B, C, bias=bias, aux=aux, bias_out=C if mode == 2 else None, act=case.act, nsplit=case.nsplit,
                   rows_per_split=case.rps, split_stride=bufs["stride"] if mode == 2 else 0)
        gm.upload(torch.device("cuda"))
        assert (gm.max_m, gm.max_n) == (case.max_m, case.max_n)
        run = lambda: gm.run(lib, stream)
    elif case.entry == "gemm":
        d, = descs
        desc = torch.zeros(256, dtype=torch.uint8, device="cuda")
        if mode == 2:
            bp = _ptr(C, d["bias_off"]) if d["bias_off"] >= 0 else None
        else:
            bp = _ptr(bias, d["bias_off"]) if mode == 0 and d["bias_off"] >= 0 else None
        run = lambda: L.check(lib.dib_gemm(mode, d["M"], d["N"], d["K"], _ptr(A, d["a_off"]), d["lda"], _ptr(B, d["b_off"]), d["ldb"],
                                           _ptr(C, d["c_off"]), d["ldc"], bp, _ptr(aux, d["aux_off"]) if aux is not None else None,
                                           d["ldaux"], case.act, _ptr(desc), stream), "dib_gemm")
    else:
        host = np.zeros(len(descs), dtype=DESC)
        for k in descs[0]:
            host[k] = [d[k] for d in descs]
        dev = torch.from_numpy(host.view(np.uint8).copy()).cuda()
        run = lambda: L.check(lib.dib_wgrad_grouped(len(descs), _ptr(dev), host.ctypes.data_as(ctypes.c_void_p), case.max_m, case.max_n,
                                                    bufs["batch"], _ptr(A), _ptr(B), _ptr(C), _ptr(C), case.nsplit, case.rps,
                                                    bufs["stride"], stream), "dib_wgrad_grouped")
    lib.dib_profile_enable(1)
    try:
        run()
        torch.cuda.synchronize()
        launches = {k: n for k, (_, n) in profile_summary(lib).items()}
    finally:
        lib.dib_profile_enable(0)
    return C.cpu().numpy(), launches


def _expected_launches(case):
    ni, nj = case.variant if case.entry != "gemm" else (2, 2)       # dib_gemm is timed in its mode's 128 x 128 category
    return {gc.profile_name(case.mode, ni, nj): 1}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c.tags & {"nt-pair", "big"}])
def test_gemm_case(name, gpu):
    case = CASES[name]
    data = gc.make_data(case)
    bufs = gc.build_buffers(case, data)
    out, launches = _launch(case, bufs, gpu)
    assert launches == _expected_launches(case), launches
    gc.check_output(case, bufs, data, out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if "nt-pair" in c.tags])
def test_non_temporal_loads_change_no_bit(name, gpu):
    """dib_set_tuning("stream_rows", 1): the streamed operands of every K-tile after the first are loaded non-temporally."""
    case = CASES[name]
    data = gc.make_data(case)
    bufs = gc.build_buffers(case, data)
    out, launches = _launch(case, bufs, gpu)
    out_nt, launches_nt = _launch(case, bufs, gpu, tuning=(("stream_rows", 1),))
    assert launches == launches_nt == _expected_launches(case), (launches, launches_nt)
    gc.check_output(case, bufs, data, out)
    assert np.array_equal(out, out_nt)       # int32 views: the guards' NaNs compare by their bits


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if "big" in c.tags])
def test_non_temporal_store_of_a_large_output(name, gpu):
    """An output of 256 MB from 524288 rows: launch_gemm_t sets both stream flags, the LDS epilogue stores non-temporally."""
    case = CASES[name]
    lib, L, torch = gpu
    assert L.get_tuning("stream_rows") <= case.max_m
    data = gc.make_data(case)
    bufs = gc.build_buffers(case, data)
    out, launches = _launch(case, bufs, gpu)
    assert launches == _expected_launches(case), launches
    gc.check_output(case, bufs, data, out)


@pytest.mark.gpu
@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("n,nsplit,stride", REDUCE_CASES)
def test_reduce_splits_vs_float64(n, nsplit, stride, add, gpu):
    """out = (add ? out : 0) + sum of the slabs, on exact data: equality with the float64 sum; the slabs' padding is NaN (never read),
    the elements around `out` keep their bit pattern."""
    lib, L, torch = gpu
    rng = np.random.default_rng(n + nsplit + add)
    pad = 8
    partial = np.full(2 * pad + nsplit * stride, np.nan, dtype=np.float32)
    slabs = gc.dyadic(rng, (nsplit, n))
    for s in range(nsplit):
        partial[pad + s * stride: pad + s * stride + n] = slabs[s]
    start = gc.dyadic(rng, (n,))
    out = np.full(n + 2 * pad, gc.GUARD_BITS, dtype=np.int32)
    if add:
        out.view(np.float32)[pad: pad + n] = start
    want = slabs.astype(np.float64).sum(0) + (start if add else 0.0)
    pd, od = torch.from_numpy(partial).cuda(), torch.from_numpy(out).cuda()
    fn = lib.dib_reduce_splits_add if add else lib.dib_reduce_splits
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(fn(_ptr(pd, pad), n, nsplit, stride, _ptr(od, pad), stream), "dib_reduce_splits")
    torch.cuda.synchronize()
    got = od.cpu().numpy()
    assert (got[:pad] == gc.GUARD_BITS).all() and (got[pad + n:] == gc.GUARD_BITS).all()
    assert np.array_equal(got.view(np.float32)[pad: pad + n].astype(np.float64), want)
    # refusals: n and stride must be multiples of 4 (the kernel moves float4); nothing is launched
    before = od.clone()
    n0 = lib.dib_launch_count()
    assert fn(_ptr(pd, pad), n + 2, nsplit, stride, _ptr(od, pad), stream) == DIB_E_ARG
    assert fn(_ptr(pd, pad), n, nsplit, stride + 2, _ptr(od, pad), stream) == DIB_E_ARG
    torch.cuda.synchronize()
    assert lib.dib_launch_count() == n0 and torch.equal(od, before)
