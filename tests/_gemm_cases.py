"""Case table, operand builder and exact reference of tests/test_gpu_gemm_envelope.py (no torch here: the table is checked on the CPU).

A case is one launch of the tiled grouped GEMM (csrc/dib_gemm.h dib_gemm_kernel<MODE, NI, NJ, BK, FLAT>) through a public entry:
the groups' shapes, per-operand misalignments, the split of a weight gradient, the tuning keys that make the host's tile rule
(csrc/host/gemm.h launch_gemm / wgrad_tile_rule, restated in `tile_rule`) pick the variant the case is there for, and that variant.

Data (section "exact" of the module docstring of the test file): A, B and bias are k/8 with |k| <= 16, so every product and every
partial sum of the fmaf chain is a multiple of 1/64 far below 2^24 / 64 and the float32 result is the float64 result whatever the
summation order.  Every operand lives in a NaN-filled arena with two guard rows before, between and after the groups' blocks and
leading dimensions wider than the extents; the output arena is pre-filled with a NaN of a fixed payload."""
import itertools
import zlib
from dataclasses import dataclass, field

import numpy as np

BIG = 1 << 30
GUARD_BITS = 0x7FC0BEEF                       # a quiet NaN no arithmetic produces
EXACT_SLOPE = {0: 1.0, 1: 0.0, 2: 0.2, 7: 0.1}    # include/dib_hip.h: linear, relu, leaky_relu (Keras 0.2), LeakyReLU(0.1)
INEXACT_ACTS = (3, 4, 5, 6)                   # tanh, sigmoid, elu, softplus
TUNING_KEYS = ("fwd_small_wgs", "fwd_narrow_wgs", "wgrad_flat_tile", "stream_rows")


def cdiv(a, b):
    return -(-a // b)


# ---- the host's tile rule ------------------------------------------------------------------------------------------------------
def tile_rule(mode, max_m, max_n, count, nsplit=1, small=512, narrow=1024):
    """(NI, NJ) of launch_gemm<MODE> for a launch of `count` groups whose largest are max_m x max_n."""
    if mode == 2:
        ni1, nj1 = max_m <= 64, max_n <= 64
        if not ni1 and not nj1:
            if cdiv(max_m, 128) * cdiv(max_n, 128) * nsplit * count < 256:
                ni1 = True
            if ni1 and cdiv(max_m, 64) * cdiv(max_n, 128) * nsplit * count < 128:
                nj1 = True
    else:
        ni1, nj1 = False, max_n <= 64
        if cdiv(max_m, 128) * cdiv(max_n, 64 if nj1 else 128) * count < small:
            ni1 = True
        if ni1 and not nj1 and cdiv(max_m, 64) * cdiv(max_n, 128) * count < (narrow if mode == 0 else 128):
            nj1 = True
    return (1 if ni1 else 2, 1 if nj1 else 2)


def feasible(mode, ni, nj, M, N):
    """Whether ANY group count / split / tuning makes the rule pick (ni, nj) for an M x N launch: what the rule hard-wires."""
    if mode == 2:
        if M <= 64 or N <= 64:
            return (ni, nj) == (1 if M <= 64 else 2, 1 if N <= 64 else 2)
        return (ni, nj) != (2, 1)
    return (nj == 1) if N <= 64 else (ni, nj) != (2, 1)


def solve(mode, ni, nj, M, N, nsplit=1, base_count=1):
    """The fewest copies of the groups (1, 2, 4 .. 256) and the tuning keys with which the rule picks (ni, nj); None if none."""
    for rep in (1 << i for i in range(9)):
        for small, narrow in itertools.product((0, BIG), repeat=2):
            if tile_rule(mode, M, N, base_count * rep, nsplit, small, narrow) == (ni, nj):
                return rep, ({} if mode == 2 else {"fwd_small_wgs": small, "fwd_narrow_wgs": narrow})
    return None


def tile_dims(mode, ni, nj, flat=False, entry="grouped"):
    """(BM, BN, BK) of the kernel instantiation a launch runs (launch_gemm_t; dib_gemm's own <MODE, 2, 2, 32>)."""
    if flat:
        return 32, 256, 32
    if entry == "gemm":
        return 128, 128, 32
    return 64 * ni, 64 * nj, 64 if (ni, nj) == (2, 2) or (mode, ni, nj) == (2, 1, 2) else 32


def lds_epilogue(mode, ni, nj, entry="grouped"):
    return entry != "gemm" and mode != 2 and (ni, nj) == (2, 2)


def profile_name(mode, ni, nj):
    """The key of engine.profile_summary for category MODE * 4 + (NI == 2 ? 2 : 0) + (NJ == 2 ? 1 : 0)."""
    return f"dib_gemm_kernel<{mode}, {ni}, {nj}, {tile_dims(mode, ni, nj)[2]}>"


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class G:
    """One group.  sh: element shifts of (a_off, b_off, c_off, aux_off; the bias block takes the last one too);
    ld: residues mod 4 of (lda, ldb, ldc, ldaux)."""
    M: int
    N: int
    K: int
    bias: bool = True
    sh: tuple = (0, 0, 0, 0)
    ld: tuple = (0, 0, 0, 0)


@dataclass(frozen=True)
class Case:
    name: str
    entry: str            # "grouped" dib_gemm_grouped | "gemm" dib_gemm | "wgrad" dib_wgrad_grouped
    mode: int
    act: int
    groups: tuple
    variant: tuple        # (NI, NJ) the tile rule must pick
    nsplit: int = 1
    rps: int = 0
    tuning: tuple = ()    # ((key, value), ...)
    flat: object = None   # True / False: the 32 x 256 weight-gradient tile on / off (M <= 32, N >= 256); None: not that shape
    use_aux: bool = True  # mode 1: pass the mask
    tags: frozenset = field(default_factory=frozenset)

    @property
    def max_m(self):
        return max(g.M for g in self.groups)

    @property
    def max_n(self):
        return max(g.N for g in self.groups)

    @property
    def dims(self):
        return tile_dims(self.mode, *self.variant, flat=bool(self.flat), entry=self.entry)

    @property
    def lds(self):
        return lds_epilogue(self.mode, *self.variant, entry=self.entry)

    @property
    def exact(self):
        return self.act in EXACT_SLOPE

    def slab_rows(self, g, s):
        """[kbeg, kend) of slab s of group g (mode 2)"""
        kb = min(g.K, s * self.rps)
        return kb, min(g.K, kb + self.rps)


VARIANTS = [(m, ni, nj) for m in (0, 1, 2) for (ni, nj) in ((2, 2), (1, 2), (1, 1), (2, 1))]
# (entry, mode, ni, nj, flat): the 12 grouped variants, the flat tile on and off, dib_gemm's own 128 x 128 x 32
TARGETS = ([("grouped", m, ni, nj, None) for m, ni, nj in VARIANTS] + [("grouped", 2, 1, 2, True), ("grouped", 2, 1, 2, False)] +
           [("gemm", m, 2, 2, None) for m in (0, 1, 2)])
M_LABELS = ("1", "B-1", "B", "B+1", "B+4", "2B+3")
K_LABELS = ("1", "3", "BK-1", "BK", "BK+1", "2BK", "2BK+4")


def _axis(B):
    return dict(zip(M_LABELS, (1, B - 1, B, B + 1, B + 4, 2 * B + 3)))


def _kaxis(BK):
    return dict(zip(K_LABELS, (1, 3, BK - 1, BK, BK + 1, 2 * BK, 2 * BK + 4)))


def _ok(entry, mode, ni, nj, flat, M, N):
    if flat is not None:
        return M <= 32 and N >= 256
    if entry == "gemm":
        return True
    if mode == 2 and (ni, nj) == (1, 2) and M <= 32 and N >= 256:
        return False          # that shape is the flat tile's (its two targets cover it)
    return feasible(mode, ni, nj, M, N)


def _tname(entry, mode, ni, nj, flat):
    return f"{'gemm' if entry == 'gemm' else 'g'}{mode}-{ni}{nj}" + ("" if flat is None else ("-flat" if flat else "-noflat"))


def _make(name, target, group_list, act, nsplit=1, rps=None, tags=(), use_aux=True):
    """A case on `target` from the groups of ONE copy: replicated / tuned until the tile rule picks the target's variant."""
    entry, mode, ni, nj, flat = target
    mm, mn = max(g.M for g in group_list), max(g.N for g in group_list)
    if rps is None:
        rps = max(g.K for g in group_list) if mode == 2 else 0
    if entry == "gemm":
        rep, tun = 1, {}
    else:
        sol = solve(mode, ni, nj, mm, mn, nsplit, len(group_list))
        assert sol is not None, (name, target)
        rep, tun = sol
    if flat is not None:
        tun = dict(tun, wgrad_flat_tile=int(flat))
    t = {f"mode{mode}", f"act{act}", "lds" if lds_epilogue(mode, ni, nj, entry) else "direct", *tags}
    return Case(f"{_tname(*target)}-{name}", entry, mode, act, tuple(group_list) * rep, (ni, nj), nsplit, rps,
                tuple(sorted(tun.items())), flat, use_aux, frozenset(t))


def shape_dims(target):
    """The tile the shapes of a target are laid around: its own, except that the flat tile's shape class (M <= 32, N >= 256) is walked
    around 32 x 256 with the flat tile on AND off (off: the 64 x 128 x 64 tile, whose BK the K edges follow)"""
    entry, mode, ni, nj, flat = target
    bk = tile_dims(mode, ni, nj, bool(flat), entry)[2]
    return (32, 256, bk) if flat is not None else tile_dims(mode, ni, nj, False, entry)


def _base(target):
    """(BM + 4, BN + 4, 2 BK + 4), or BM - 4 / BN - 4 where the rule cannot give the variant a matrix that tall / wide"""
    entry, mode, ni, nj, flat = target
    bm, bn, bk = shape_dims(target)
    for M, N in itertools.product((bm + 4, bm - 4), (bn + 4, bn - 4)):
        if _ok(entry, mode, ni, nj, flat, M, N):
            return M, N, 2 * bk + 4
    raise AssertionError(target)


def edge_shapes(target):
    """[(label, (M, N, K) or None)]: one axis at a time around the base; where the rule cannot give the variant that extent next to the
    base's other extent, next to B - 4 of the other axis; None where it can give it neither."""
    entry, mode, ni, nj, flat = target
    bm, bn, bk = shape_dims(target)
    M0, N0, K0 = _base(target)
    first = lambda cands: next((c for c in cands if _ok(entry, mode, ni, nj, flat, c[0], c[1])), None)
    out = [(f"M={lab}", first([(v, N0, K0), (v, bn - 4, K0)])) for lab, v in _axis(bm).items()]
    out += [(f"N={lab}", first([(M0, v, K0), (bm - 4, v, K0)])) for lab, v in _axis(bn).items()]
    out += [(f"K={lab}", (M0, N0, v)) for lab, v in _kaxis(bk).items()]
    out += [("corner=1", first([(1, 1, 1)])), ("corner=B+1", first([(bm + 1, bn + 1, bk + 1)]))]
    if mode != 2:
        out.append(("M=xcd", (9 * bm + 1, N0, K0)))     # cdiv(M, BM) = 10: the XCD tile order pads the grid to 16 m-tiles
    return out


def _edge_cases():
    out = []
    acts = (1, 2, 7, 0)
    for target in TARGETS:
        entry, mode, ni, nj, flat = target
        bm, bn, bk = shape_dims(target)
        for i, (lab, shape) in enumerate(edge_shapes(target)):
            if shape is None:
                continue
            M, N, K = shape
            tags = {lab}
            if mode == 2:
                for ax, v, b in (("M", M, bm), ("N", N, bn)):
                    if v > b and v % b:
                        tags.add(f"{ax}-shifted" if v % 4 == 0 else f"{ax}-checked")
            # (a dgrad edge always runs with a mask: id 0 would leave the aux loads of that edge unread)
            act = 0 if mode == 2 else acts[i % (4 if mode == 0 else 3)]
            out.append(_make(lab, target, [G(M, N, K)], act, tags=tags))
    return out


def _act_cases():
    """Every activation id in both epilogues (and dib_gemm's) at the base shape; ids 3..6 with small K so that z spans about +-10."""
    out = []
    for target in TARGETS:
        entry, mode, ni, nj, flat = target
        if mode == 2:
            continue
        M0, N0, K0 = _base(target)
        for act in EXACT_SLOPE:
            out.append(_make(f"act{act}", target, [G(M0, N0, K0)], act, tags={"act-sweep"}))
        if (ni, nj) in ((2, 2), (1, 1)):
            for act in INEXACT_ACTS:
                out.append(_make(f"act{act}", target, [G(M0, N0, 12)], act, tags={"act-sweep"}))
    # a dgrad launch without a mask writes the plain product whatever the activation id
    out.append(_make("nomask", ("grouped", 1, 2, 2, None), [G(132, 132, 132)], 1, use_aux=False, tags={"nomask"}))
    out.append(_make("nomask", ("grouped", 1, 1, 1, None), [G(68, 68, 68)], 2, use_aux=False, tags={"nomask"}))
    return out


def _contraction_cases():
    out = []
    for target in (("grouped", 2, 2, 2, None), ("grouped", 2, 1, 2, None), ("grouped", 2, 1, 1, None), ("grouped", 2, 2, 1, None),
                   ("grouped", 2, 1, 2, True)):
        M0, N0, _ = _base(target)
        two = lambda K: [G(M0, N0, K, bias=True), G(M0, N0, K, bias=False)]     # bias sums on and off per group
        out.append(_make("slabs-whole", target, two(256), 0, nsplit=4, rps=64, tags={"slabs-whole"}))
        out.append(_make("slabs-rps37", target, two(150), 0, nsplit=5, rps=37, tags={"rps37", "short-last-slab"}))   # last: 2 rows
        out.append(_make("slabs-rps100", target, two(250), 0, nsplit=3, rps=100, tags={"rps100", "short-last-slab"}))  # last: 50
        out.append(_make("slabs-empty", target, two(100), 0, nsplit=4, rps=37, tags={"empty-slab"}))   # slab 3: kbeg = 111 >= K
    return out


def _ragged_cases():
    out = []
    shapes = [(132, 200, 68), (70, 132, 5), (1, 1, 1), (259, 60, 130)]
    for target in (("grouped", 0, 2, 2, None), ("grouped", 0, 1, 1, None), ("grouped", 1, 2, 2, None), ("grouped", 1, 1, 2, None),
                   ("grouped", 2, 2, 2, None), ("grouped", 2, 1, 2, None), ("grouped", 2, 1, 1, None)):
        mode = target[1]
        groups = [G(M, N, K, bias=(i != 1)) for i, (M, N, K) in enumerate(shapes)]     # one group with bias_off = -1
        # mode 2: K = 5 and 1 are shorter than a slab, K = 68 leaves the third slab empty
        out.append(_make("ragged", target, groups, 2 if mode != 2 else 0, nsplit=3 if mode == 2 else 1, rps=50 if mode == 2 else None,
                         tags={"ragged"} | ({"k-shorter-than-slab", "empty-slab"} if mode == 2 else set())))
    return out


def _alignment_cases():
    out = []
    for mode in (0, 1, 2):
        for ni, nj in ((2, 2), (1, 1)):      # (2, 2) at BK = 64: the LDS epilogue of modes 0 / 1; (1, 1): a direct one
            target = ("grouped", mode, ni, nj, None)
            M0, N0, K0 = _base(target)
            ops = ("a", "b", "c") + (("aux",) if mode == 1 else ())
            act = 7 if mode == 1 else (2 if mode == 0 else 0)
            for i, op in enumerate(ops):
                for s in (1, 2, 3):
                    sh = tuple(s if j == i else 0 for j in range(4))
                    out.append(_make(f"off-{op}{s}", target, [G(M0, N0, K0, sh=sh)], act, tags={f"off-{op}", f"off{s}"}))
                    out.append(_make(f"ld-{op}{s}", target, [G(M0, N0, K0, ld=sh)], act, tags={f"ld-{op}", f"ld{s}"}))
            out.append(_make("misaligned-all", target, [G(M0, N0, K0, sh=(1, 2, 3, 1), ld=(3, 1, 2, 3))], act, tags={"all-misaligned"}))
            out.append(_make("k-odd-aligned", target, [G(M0, N0, K0 + 3)], act, tags={"k-odd-aligned"}))
    return out


def _stream_cases():
    """The base case of every target again with stream_rows = 1: the non-temporal loads (outputs must not change by a bit)"""
    out = []
    for target in TARGETS:
        if target[0] == "gemm":
            continue            # dib_gemm passes no stream flags
        M0, N0, K0 = _base(target)
        out.append(_make("base", target, [G(M0, N0, K0)], 1 if target[1] != 2 else 0, tags={"nt-pair"}))
    return out


def _big_cases():
    """>= 256 MB of output from >= 8192 rows: the non-temporal store of the LDS epilogue (launch_gemm_t: big_out)"""
    return [_make("big", ("grouped", mode, 2, 2, None), [G(524288, 128, 4)], 2, tags={"big"}) for mode in (0, 1)]


def _wgrad_case():
    """dib_wgrad_grouped: K = -1 (the batch argument) and per-batch offsets; below every streaming threshold -> the tiled kernel"""
    return [_make("batch", ("wgrad", 2, 1, 1, None), [G(132, 68, 150, bias=True), G(70, 132, 150, bias=False)], 0, nsplit=3, rps=64,
                  tags={"wgrad-entry"})]


def build_cases():
    cases = (_edge_cases() + _act_cases() + _contraction_cases() + _ragged_cases() + _alignment_cases() + _stream_cases() +
             _big_cases() + _wgrad_case())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return {c.name: c for c in cases}


CASES = build_cases()
REDUCE_CASES = [(4, 1, 4), (4100, 7, 4104)]     # (n, nsplit, stride) of dib_reduce_splits / dib_reduce_splits_add


# ---- data ----------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def dyadic(rng, shape):
    return (rng.integers(-16, 17, size=shape).astype(np.float32) / np.float32(8))


def _mask_exact(rng, M, N, period=None):
    """aux for the exact activation ids: k/8 with exact +0.0 and -0.0 entries (act' is y > 0: both take the negative-side slope)"""
    rows = M if period is None else period
    x = dyadic(rng, (rows, N))
    r = rng.random((rows, N))
    x[r < 0.08] = 0.0
    x[r < 0.04] = -0.0
    if period is not None:
        x = np.tile(x, (M // period, 1))
    flat = x.reshape(-1)
    flat[0] = 0.0
    if flat.size > 1:
        flat[-1] = -0.0
    return x


def _mask_inexact(rng, act, M, N):
    """aux in the activation's range (it is the activation's OUTPUT)"""
    u = rng.random((M, N))
    if act == 3:
        x = 1.998 * u - 0.999
    elif act == 4:
        x = 0.001 + 0.998 * u
    elif act == 5:
        x = np.where(u < 0.5, -0.999 * 2 * u, 20 * (u - 0.5))
    else:
        x = 0.001 + 10 * u
    return x.astype(np.float32)


def make_data(case):
    """per group: dict(A, B, bias or None, aux or None) of the logical matrices (float32)"""
    rng = _rng(case.name)
    out = []
    for g in case.groups:
        if case.mode == 0:
            A, B = dyadic(rng, (g.M, g.K)), dyadic(rng, (g.K, g.N))
        elif case.mode == 1:
            A, B = dyadic(rng, (g.M, g.K)), dyadic(rng, (g.N, g.K))
        else:
            A, B = dyadic(rng, (g.K, g.M)), dyadic(rng, (g.K, g.N))
        bias = aux = None
        if case.mode == 0 and g.bias:
            bias = dyadic(rng, (g.N,))
            if not case.exact and g.N >= 2:      # the saturated branches of expf / expm1f / log1pf
                bias[0], bias[-1] = 100.0, -100.0
        if case.mode == 1 and case.use_aux:
            if case.exact:
                aux = _mask_exact(rng, g.M, g.N, period=4096 if g.M > 65536 else None)
            else:
                aux = _mask_inexact(rng, case.act, g.M, g.N)
        out.append(dict(A=A, B=B, bias=bias, aux=aux))
    return out


def exactness_margin(case, data):
    """2^24 / (64 max(|A| |B| + |bias|)): above 1 every partial sum of every summation order is exact in float32"""
    worst = 0.0
    for g, d in zip(case.groups, data):
        a, b = np.abs(d["A"]).astype(np.float64), np.abs(d["B"]).astype(np.float64)
        if case.mode == 2:
            worst = max(worst, float((a.T @ b).max()), float(b.sum(0).max()))
            continue
        for lo in range(0, g.M, 65536):
            mag = a[lo: lo + 65536] @ (b if case.mode == 0 else b.T)
            if d["bias"] is not None:
                mag = mag + np.abs(d["bias"])
            worst = max(worst, float(mag.max()))
    return 2.0 ** 24 / (64.0 * max(worst, 1e-30))


def is_dyadic(x, bound=2.0):
    return bool(np.all(x * 8 == np.round(x * 8)) and np.all(np.abs(x) <= bound))


# ---- arenas ---------------------------------------------------------------------------------------------------------------------
class _Arena:
    def __init__(self, lead=0):
        self.cur, self.maxld = lead, 4

    def place(self, rows, cols, res=0, shift=0):
        ld = cols + (-cols) % 4 + 4 + res          # wider than the extent, = res (mod 4)
        pos = self.cur + 2 * ld                    # two guard rows before the block
        pos += (-pos) % 4 + shift
        self.cur = pos + rows * ld
        self.maxld = max(self.maxld, ld)
        return pos, ld

    def close(self):
        self.cur += 2 * self.maxld + 8
        self.cur += (-self.cur) % 4
        return self.cur


def _fill(buf, pos, ld, mat):
    r, c = mat.shape
    view = np.lib.stride_tricks.as_strided(buf[pos:], shape=(r, c), strides=(4 * ld, 4))
    view[...] = mat


def _view(buf, pos, ld, r, c):
    return np.lib.stride_tricks.as_strided(buf[pos:], shape=(r, c), strides=(buf.itemsize * ld, buf.itemsize), writeable=False)


BOFF = dict(a=4, b=8, c=4)      # the per-batch offsets of the dib_wgrad_grouped case (multiples of 4: alignment unchanged)


def build_buffers(case, data):
    """-> dict(A, B, bias, aux: float32 arenas (NaN outside the blocks; bias / aux None where the mode has none), C: int32 arena of
    GUARD_BITS, descs: the groups' descriptors, place: per group (c_pos, ldc, bias_pos), stride: the slab stride (mode 2), written:
    bool mask of C's elements the launch must write, batch)"""
    mode = case.mode
    batch = case.groups[0].K if case.entry == "wgrad" else 0
    lead = 8 * batch
    aa, ab, ac, ax, abias = _Arena(lead), _Arena(lead), _Arena(lead), _Arena(), _Arena()
    descs, place = [], []
    for g in case.groups:
        ra, ca = (g.M, g.K) if mode != 2 else (g.K, g.M)
        rb, cb = (g.K, g.N) if mode != 1 else (g.N, g.K)
        a_pos, lda = aa.place(ra, ca, g.ld[0], g.sh[0])
        b_pos, ldb = ab.place(rb, cb, g.ld[1], g.sh[1])
        c_pos, ldc = ac.place(g.M, g.N, g.ld[2], g.sh[2])
        x_pos, ldx = ax.place(g.M, g.N, g.ld[3], g.sh[3]) if mode == 1 else (0, 0)
        bias_pos = -1
        if g.bias and mode == 0:
            bias_pos, _ = abias.place(1, g.N, 0, g.sh[3])
        elif g.bias and mode == 2:
            bias_pos, _ = ac.place(1, g.N, 0, g.sh[3])
        d = dict(a_off=a_pos, b_off=b_pos, c_off=c_pos, bias_off=bias_pos, aux_off=x_pos, a_boff=0, b_boff=0, c_boff=0, aux_boff=0,
                 M=g.M, N=g.N, K=g.K, lda=lda, ldb=ldb, ldc=ldc, ldaux=ldx)
        if case.entry == "wgrad":
            d.update(K=-1, a_off=a_pos - BOFF["a"] * batch, b_off=b_pos - BOFF["b"] * batch, c_off=c_pos - BOFF["c"] * batch,
                     a_boff=BOFF["a"], b_boff=BOFF["b"], c_boff=BOFF["c"])
        descs.append(d)
        place.append((c_pos, ldc, bias_pos))
    stride = ac.close()
    A = np.full(aa.close(), np.nan, dtype=np.float32)
    B = np.full(ab.close(), np.nan, dtype=np.float32)
    X = np.full(ax.close(), np.nan, dtype=np.float32) if mode == 1 and case.use_aux else None
    bias = np.full(abias.close(), np.nan, dtype=np.float32) if mode == 0 else None
    nslab = case.nsplit if mode == 2 else 1
    C = np.full(nslab * stride, GUARD_BITS, dtype=np.int32)
    written = np.zeros(nslab * stride, dtype=bool)
    for g, d, dat, (c_pos, ldc, bias_pos) in zip(case.groups, descs, data, place):
        _fill(A, d["a_off"] + d["a_boff"] * batch, d["lda"], dat["A"])
        _fill(B, d["b_off"] + d["b_boff"] * batch, d["ldb"], dat["B"])
        if X is not None:
            _fill(X, d["aux_off"], d["ldaux"], dat["aux"])
        if dat["bias"] is not None:
            bias[bias_pos: bias_pos + g.N] = dat["bias"]
        for s in range(nslab):
            w = np.lib.stride_tricks.as_strided(written[s * stride + c_pos:], shape=(g.M, g.N), strides=(ldc, 1))
            w[...] = True
            if mode == 2 and bias_pos >= 0:
                written[s * stride + bias_pos: s * stride + bias_pos + g.N] = True
    return dict(A=A, B=B, bias=bias, aux=X, C=C, descs=descs, place=place, stride=stride, written=written, batch=batch)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _act64(act, z):
    if act == 3:
        return np.tanh(z)
    if act == 4:
        return 1.0 / (1.0 + np.exp(-z))
    if act == 5:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def _act_grad64(act, y):
    if act == 3:
        return 1.0 - y * y
    if act == 4:
        return y * (1.0 - y)
    if act == 5:
        return np.where(y > 0, 1.0, y + 1.0)
    return 1.0 - np.exp(-y)


def _leaky32(z32, gate, slope):
    """float32 statement of the leaky family: one rounding (slope * z) on the negative side"""
    if slope == 1.0:
        return z32
    return np.where(gate > 0, z32, np.float32(slope) * z32)


def expected(case, g, dat, lo=0, hi=None):
    """Rows [lo, hi) of the group's output.  Exact ids: the float32 array the kernel must produce bit for bit (as values).  Ids 3..6:
    the float64 formula.  Mode 2: a list over the slabs of (float64 [M, N] partial product, float64 [N] column sums of B)."""
    A, B = dat["A"].astype(np.float64), dat["B"].astype(np.float64)
    if case.mode == 2:
        out = []
        for s in range(case.nsplit):
            kb, ke = case.slab_rows(g, s)
            out.append((A[kb:ke].T @ B[kb:ke], B[kb:ke].sum(0)))
        return out
    hi = g.M if hi is None else hi
    if case.mode == 0:
        z = A[lo:hi] @ B + (dat["bias"].astype(np.float64) if dat["bias"] is not None else 0.0)
        if not case.exact:
            return _act64(case.act, z)
        z32 = z.astype(np.float32)
        assert np.array_equal(z32.astype(np.float64), z)       # the exactness bound at work
        return _leaky32(z32, z32, EXACT_SLOPE[case.act])
    p = A[lo:hi] @ B.T
    if dat["aux"] is None or case.act == 0:
        want = p.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), p)
        return want
    y = dat["aux"][lo:hi]
    if not case.exact:
        return p * _act_grad64(case.act, y.astype(np.float64))
    p32 = p.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), p)
    return _leaky32(p32, y, EXACT_SLOPE[case.act])


def check_output(case, bufs, data, C_i32, chunk=65536):
    """Everything the launch owes: guards untouched (bit pattern), every group's block equal to the reference."""
    assert C_i32.dtype == np.int32 and C_i32.shape == bufs["C"].shape
    stray = np.flatnonzero(C_i32[~bufs["written"]] != GUARD_BITS)
    assert stray.size == 0, f"{case.name}: {stray.size} elements outside the groups' blocks were written"
    Cf = C_i32.view(np.float32)
    stride = bufs["stride"]
    for gi, (g, dat, (c_pos, ldc, bias_pos)) in enumerate(zip(case.groups, data, bufs["place"])):
        if case.mode == 2:
            tot, tot_b = np.zeros((g.M, g.N)), np.zeros(g.N)
            for s, (want, want_b) in enumerate(expected(case, g, dat)):
                got = _view(Cf, s * stride + c_pos, ldc, g.M, g.N).astype(np.float64)
                assert np.array_equal(got, want), (case.name, gi, s, _first_diff(got, want))
                tot += got
                if bias_pos >= 0:
                    got_b = Cf[s * stride + bias_pos: s * stride + bias_pos + g.N].astype(np.float64)
                    assert np.array_equal(got_b, want_b), (case.name, gi, s, "bias", _first_diff(got_b[None], want_b[None]))
                    tot_b += got_b
            assert np.array_equal(tot, dat["A"].astype(np.float64).T @ dat["B"].astype(np.float64)), (case.name, gi, "slab sum")
            if bias_pos >= 0:
                assert np.array_equal(tot_b, dat["B"].astype(np.float64).sum(0)), (case.name, gi, "bias slab sum")
            continue
        for lo in range(0, g.M, chunk):
            hi = min(g.M, lo + chunk)
            got = _view(Cf, c_pos + lo * ldc, ldc, hi - lo, g.N)
            want = expected(case, g, dat, lo, hi)
            if case.exact:
                assert np.array_equal(got, want), (case.name, gi, _first_diff(got, want, lo))
            else:
                tol = 2e-5 * (1 + np.abs(want).max())           # tests/test_gpu_building_blocks.py
                err = np.abs(got.astype(np.float64) - want)
                assert not np.isnan(got).any() and err.max() <= tol, (case.name, gi, float(err.max()), tol)


def _first_diff(got, want, lo=0):
    bad = np.argwhere(~(got == want))
    r, c = bad[0]
    return f"{len(bad)} differ; first at ({lo + r}, {c}): got {got[r, c]!r}, want {want[r, c]!r}"
