"""Shared by test_cpu_topk.py, test_gpu_topk.py and test_gpu_trainer_extremes.py: the NumPy statement of the score extremes (two stable
argsorts per label group), the score kinds and label layouts the selection can go wrong at, and the comparison.  Nothing here touches
the package under test."""
import zlib

import numpy as np

NS = (1, 2, 255, 256, 257, 4097, 65539, 1 << 20)
KS = (1, 20, 1024)
KINDS = ("equal", "quant8", "tie_run", "mixed", "ulp")
LAYOUTS = ("mixed", "small", "empty", "other", None)
HALF = 1 << 19
FLT_MAX = np.float32(3.4028234663852886e38)


def _rng(*tag):
    return np.random.default_rng(zlib.crc32(repr(tag).encode()))


def scores(n: int, kind: str) -> np.ndarray:
    """float32 [n].
    equal     one value everywhere: the order is the position alone, and every digit pass over the score sees one full bin
    quant8    eight values, both zeros among them: for every k the boundary falls inside a run of ties
    tie_run   random values; the largest and the smallest value each shared by every third position of the 4 000 around n / 2 and by
              the first and the last position: at n = 2^20 a run of ~1 300 ties with members on both sides of position 2^19
    mixed     both signs: +-FLT_MAX, subnormals, the smallest normals, +-0.0, ordinary values, with repeats
    ulp       1 + j ulp and -(1 + j ulp) for distinct j < n: neighbours in rank are one ulp apart wherever k falls (np.nextafter steps)"""
    rng = _rng("scores", n, kind)
    if kind == "equal":
        return np.full(n, 0.75, dtype=np.float32)
    if kind == "quant8":
        s = (rng.integers(0, 8, n).astype(np.float32) - np.float32(3.0)) / np.float32(8.0)
        s[(s == 0) & (np.arange(n) % 2 == 1)] = np.float32(-0.0)
        return s
    if kind == "tie_run":
        s = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        pos = np.arange(n)
        near = np.abs(pos - n // 2) <= 2000
        s[(near & (pos % 3 == 0)) | (pos == 0)] = np.float32(1.5)
        s[(near & (pos % 3 == 1)) | (pos == n - 1)] = np.float32(-1.5)
        return s
    if kind == "mixed":
        table = np.array([FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, 0.0, -0.0, 1.0, -1.0,
                          np.nextafter(np.float32(1.0), np.float32(2.0)), 3e38, -3e38, 6e-39, -6e-39], dtype=np.float32)
        s = rng.standard_normal(n).astype(np.float32)
        pick = rng.random(n) < 0.5
        s[pick] = table[rng.integers(0, table.size, int(pick.sum()))]
        return s
    if kind == "ulp":
        j = rng.permutation(n).astype(np.uint32)
        bits = np.uint32(0x3F800000) + (j >> np.uint32(1))
        bits |= (j & np.uint32(1)) << np.uint32(31)                 # odd j: the negative twin of the same magnitude
        return bits.view(np.float32)
    raise KeyError(kind)


def labels(n: int, how):
    """int64 [n] or None.
    mixed   0 and 1 at random (a third 1)
    small   label 1 at no more than five positions (fewer than k = 20 and k = 1 024), 0 elsewhere
    empty   all 0: group 1 has no member
    other   0, 1 and the labels -1, 2, 7, which are in neither group
    None    no labels: every score in group 0"""
    if how is None:
        return None
    rng = _rng("labels", n, how)
    if how == "mixed":
        return (rng.random(n) < 1.0 / 3.0).astype(np.int64)
    if how == "small":
        y = np.zeros(n, dtype=np.int64)
        y[rng.choice(n, min(5, max(n // 2, 1)), replace=False)] = 1
        return y
    if how == "empty":
        return np.zeros(n, dtype=np.int64)
    if how == "other":
        return np.array([0, 1, -1, 2, 7, 0, 1], dtype=np.int64)[rng.integers(0, 7, n)]
    raise KeyError(how)


def members(n: int, y, g: int) -> np.ndarray:
    if y is None:
        return np.arange(n, dtype=np.int64) if g == 0 else np.zeros(0, dtype=np.int64)
    return np.flatnonzero(np.asarray(y) == g).astype(np.int64)


def reference(s: np.ndarray, y, k: int):
    """(idx[g][end], num[g]): end 0 = np.argsort(-s, kind="stable")[:k], end 1 = np.argsort(s, kind="stable")[:k] over group g's members,
    as positions in `s`"""
    s = np.asarray(s, dtype=np.float32)
    idx, num = [], []
    for g in (0, 1):
        m = members(s.size, y, g)
        sg = s[m]
        idx.append((m[np.argsort(-sg, kind="stable")[:k]], m[np.argsort(sg, kind="stable")[:k]]))
        num.append(int(m.size))
    return idx, num


def check_raw(idx: np.ndarray, val: np.ndarray, counts, s: np.ndarray, want, k: int, sentinel: int, what: str):
    """the kernel's raw buffers (idx int32 [2, 2, k], val float32 [2, 2, k] pre-filled with `sentinel` / its float) against `reference`:
    positions and score BITS equal, the slots past min(k, m_g) untouched, the counts right"""
    want_idx, num = want
    assert list(counts) == [num[0], num[1], 0], (what, counts, num)
    for g in (0, 1):
        for end in (0, 1):
            w = want_idx[g][end][:k]
            c = len(w)
            assert c == min(k, num[g])
            assert np.array_equal(idx[g, end, :c], w), f"{what}: group {g} end {end} positions"
            assert np.array_equal(val[g, end, :c].view(np.int32), s[w].view(np.int32)), f"{what}: group {g} end {end} score bits"
            assert (idx[g, end, c:] == sentinel).all() and (val[g, end, c:] == np.float32(sentinel)).all(), \
                f"{what}: group {g} end {end} wrote past its {c} slots"


def check_extremes(ex, s: np.ndarray, want, k: int, what: str, remap=None):
    """a `metrics.Extremes` against `reference` (positions mapped through `remap` when given)"""
    want_idx, num = want
    assert tuple(ex.num) == tuple(num), what
    for g in (0, 1):
        for end, got in ((0, ex.most[g]), (1, ex.least[g])):
            w = want_idx[g][end][:k]
            assert got[0].dtype == np.int64 and got[1].dtype == np.float32
            assert np.array_equal(got[0], w if remap is None else np.asarray(remap)[w]), f"{what}: group {g} end {end} indices"
            assert np.array_equal(got[1].view(np.int32), s[w].view(np.int32)), f"{what}: group {g} end {end} score bits"
