"""NumPy float64 restatement of the order-free CTW tree (DESIGN.md "CTW on the device"): the checker of the level build in
csrc/dib_ctw_levels.h, itself checked against the host estimator csrc/dib_ctw.cpp (tests/test_ctw_levels_host.py).

Window x[0..N): position t has symbol x[t] and context x[t-1], ..., x[0].  Level 0 is the root with every position.  A member t
of a group at level d moves to level d + 1 iff t > d and (d = 0 or the group has >= 2 members); the movers of a group split by
x[t-d-1], each non-empty part is a child node.  counts[s] of a node = its members with x[t] = s (those that stop there
included).  Levels are refined with a stable sort of group * A + symbol, so siblings are contiguous and in symbol order; code
lengths go bottom-up, a parent summing its children serially in symbol order.  The build stops at level 512 and reports `deep`
iff some group of >= 2 members there still has a member with more context (beyond that the host's tree depends on the order of
insertion).  lgamma, log, log2 and pow are the C library's, the ones the host estimator calls."""
import ctypes
import ctypes.util
import math

import numpy as np

MAX_LEVEL = 512

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = ctypes.c_double
_libm.lgamma.argtypes = [ctypes.c_double]
_tables = {}


def _lgamma_table(offset: float, upto: int) -> np.ndarray:
    """lgamma(k + offset) for k = 0 .. upto"""
    have = _tables.get(offset)
    if have is None or len(have) <= upto:
        start = 0 if have is None else len(have)
        more = np.array([_libm.lgamma(float(k) + offset) for k in range(start, upto + 1)], dtype=np.float64)
        have = more if have is None else np.concatenate([have, more])
        _tables[offset] = have
    return have


def ctw_levels(seq, alphabet_size: int, max_level: int = MAX_LEVEL) -> dict:
    """{"rate": float32-rounded bits per symbol (NaN for an empty window), "code_length_bits": L_w(root) unrounded, "nodes": node
    count with the root, "deep": the guard above, "level_nodes": nodes per level, "level_moving": positions that move from each
    level to the next}"""
    A = int(alphabet_size)
    x = np.asarray(seq, dtype=np.int64).reshape(-1)
    N = int(x.size)
    if N and (x.min() < 0 or x.max() >= A):
        raise ValueError(f"symbols must lie in [0, {A})")
    beta = 1.0 / A
    ab = A * beta
    lg_b, lg_ab, ln2 = _libm.lgamma(beta), _libm.lgamma(ab), math.log(2)
    tab_b, tab_ab = _lgamma_table(beta, N), _lgamma_table(ab, N)

    # ---- top-down: levels of (counts [n, A], parent index in the level above, symbol under the parent)
    levels = []
    t = np.arange(N, dtype=np.int64)
    group = np.zeros(N, dtype=np.int64)
    n_groups, parent, child_sym = 1, np.zeros(1, np.int64), np.zeros(1, np.int64)
    level_nodes, level_moving, deep = [], [], False
    d = 0
    while True:
        counts = np.bincount(group * A + x[t], minlength=n_groups * A).reshape(n_groups, A)
        levels.append((counts, parent, child_sym))
        level_nodes.append(n_groups)
        moving = t > d
        if d >= 1:
            moving &= counts.sum(1)[group] >= 2
        n_moving = int(moving.sum())
        if d == max_level:
            deep = n_moving > 0
            level_moving.append(0)
            break
        level_moving.append(n_moving)
        if n_moving == 0:
            break
        tm = t[moving]
        key = group[moving] * A + x[tm - d - 1]
        order = np.argsort(key, kind="stable")
        key, t = key[order], tm[order]
        uniq, group = np.unique(key, return_inverse=True)
        n_groups, parent, child_sym = int(uniq.size), uniq // A, uniq % A
        d += 1

    # ---- bottom-up
    weighted_below, parent_below, sym_below = None, None, None
    for counts, parent, child_sym in reversed(levels):
        total = counts.sum(1)
        local = tab_ab[total] - lg_ab
        for s in range(A):
            local = local - (tab_b[counts[:, s]] - lg_b)
        local = local / ln2
        weighted = local.copy()
        if weighted_below is not None:
            n = counts.shape[0]
            kid_values = np.zeros((n, A))
            has = np.zeros(n, dtype=bool)
            kid_values[parent_below, sym_below] = weighted_below
            has[parent_below] = True
            kids = np.zeros(n)
            for s in range(A):   # serial, in symbol order; an absent child adds 0.0 exactly
                kids = kids + kid_values[:, s]
            for v in np.where(has & (total > 1))[0]:
                lc, le = float(kids[v]), float(local[v])
                weighted[v] = 1 + min(lc, le) - math.log2(1 + math.pow(2, -abs(le - lc)))
        weighted_below, parent_below, sym_below = weighted, parent, child_sym
    bits = float(weighted_below[0])
    rate = float(np.float32(bits / N)) if N else float("nan")
    return {"rate": rate, "code_length_bits": bits, "nodes": int(sum(level_nodes)), "deep": bool(deep),
            "level_nodes": level_nodes, "level_moving": level_moving}


# ---- the cases tests/test_ctw_levels_host.py and tests/test_gpu_ctw_levels.py share -----------------------------------------------
GRID_ALPHABETS = (2, 3, 4, 16)
GRID_LENGTHS = (1, 2, 3, 5, 17, 64, 300, 2000)
GRID_ZERO_PROBABILITIES = (None, 0.9, 0.99)   # None: uniform symbols
GRID_DRAWS = 3


def grid_cases():
    """the 288 random sequences: [(alphabet, sequence uint8)], in a fixed order from a fixed seed"""
    rng = np.random.default_rng(20240)
    out = []
    for A in GRID_ALPHABETS:
        for n in GRID_LENGTHS:
            for p0 in GRID_ZERO_PROBABILITIES:
                for _ in range(GRID_DRAWS):
                    s = rng.integers(0, A, size=n)
                    if p0 is not None:
                        s[rng.random(n) < p0] = 0
                    out.append((A, s.astype(np.uint8)))
    return out


def logistic_symbols(n: int, x0: float = 0.3, alphabet_size: int = 2) -> np.ndarray:
    """symbols of the logistic map x -> 4 x (1 - x) through the partition of [0, 1] into alphabet_size equal cells (2: the
    generating partition)"""
    out = np.empty(n, dtype=np.uint8)
    v = x0
    for i in range(n):
        v = 4.0 * v * (1.0 - v)
        out[i] = min(int(v * alphabet_size), alphabet_size - 1)
    return out


def repeated_block(block_length: int, alphabet_size: int = 2, seed: int = 5) -> np.ndarray:
    """7 random symbols, a random block of block_length symbols twice, 3 random symbols: the positions after the two occurrences
    share a context of at least block_length symbols and both have more"""
    rng = np.random.default_rng(seed)
    block = rng.integers(0, alphabet_size, size=block_length)
    return np.concatenate([rng.integers(0, alphabet_size, size=7), block, block,
                           rng.integers(0, alphabet_size, size=3)]).astype(np.uint8)
