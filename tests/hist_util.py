"""Shared by test_cpu_hist.py and test_gpu_hist.py: TensorBoard's default histogram edges, a restatement of what
`SummaryWriter.add_histogram` stores (`np.histogram` over those edges, trimmed to the occupied range, five scalars in float64), the
case list, and the comparison.  Nothing here touches the package under test."""
import functools
import math

import numpy as np

FIELDS = ("min", "max", "num", "sum", "sum_squares", "bucket_limit", "bucket")
NS = (1, 2, 255, 256, 257, 90001)
LABELLINGS = ("zeros", "ones", "mixed", "mixed_unlabelled")
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def default_edges() -> np.ndarray:
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    e = np.array([-p for p in reversed(pos)] + [0] + pos, dtype=np.float64)
    e.setflags(write=False)
    return e


def restate(values, edges=None) -> dict:
    """the seven fields for `values` (any float dtype; counted and summed as float64).  ValueError where TensorBoard raises: no value,
    or no value inside the edges."""
    edges = default_edges() if edges is None else np.asarray(edges, np.float64)
    v = np.asarray(values).reshape(-1).astype(np.float64)
    if v.size == 0:
        raise ValueError("no values")
    counts, limits = np.histogram(v, bins=edges)
    filled = np.flatnonzero(counts > 0)
    if filled.size == 0:
        raise ValueError("no value inside the edges")
    first, last = int(filled[0]), int(filled[-1])
    if first > 0:
        kept = counts[first - 1:last + 1]                    # the real bin to the left: empty by construction
    else:
        kept = np.concatenate([[0], counts[:last + 1]])
    return {"min": float(v.min()), "max": float(v.max()), "num": int(v.size), "sum": float(v.sum()), "sum_squares": float(v.dot(v)),
            "bucket_limit": [float(x) for x in limits[first:last + 2]], "bucket": [int(c) for c in kept]}


def specials() -> np.ndarray:
    """float32 values at which the bucketing can go wrong: both zeros, the floats nearest below and above several edges of both signs
    (the first and the last included), subnormals, values beyond the table, and the edges of the explicit 3-edge table"""
    e = default_edges()
    pos = e[e > 0]
    picks = [pos[0], pos[1], pos[len(pos) // 3], pos[len(pos) // 2], pos[290], pos[-2], pos[-1]]
    out = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5]
    for p in picks:
        for sign in (1.0, -1.0):
            f = np.float32(sign * p)
            out += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    out += [1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38]            # subnormals and the smallest normals
    out += [1.0000001e20, -1.0000001e20, 1e21, -1e21, 3e38, -3e38]                 # in num / min / max / sum, in no bucket
    return np.array(out, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def scores(n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    if n == 1:
        return np.array([0.37], np.float32)
    if n == 2:
        return np.array([0.5, 0.5], np.float32)
    sp = specials()
    run = np.full(2000 if n > 4000 else 0, 0.25, np.float32)                      # more equal values than one workgroup's share
    rest = n - sp.size - run.size
    hsc = rng.random(rest // 2).astype(np.float32)                                 # HSC-like scores in [0, 1)
    bce = rng.uniform(-40.0, 40.0, rest - rest // 2).astype(np.float32)            # BCE-like logits of both signs
    mixed = np.concatenate([sp, hsc, bce])
    rng.shuffle(mixed)
    cut = mixed.size // 3
    v = np.concatenate([mixed[:cut], run, mixed[cut:]])                            # the run stays contiguous
    assert v.size == n and v.dtype == np.float32 and np.isfinite(v).all()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def labels(n: int, how: str) -> np.ndarray:
    rng = np.random.default_rng(2000 + n)
    if how == "zeros":
        y = np.zeros(n, np.int64)
    elif how == "ones":
        y = np.ones(n, np.int64)
    elif how == "mixed":
        y = (rng.random(n) < 0.5).astype(np.int64)
    else:
        y = rng.integers(-1, 2, n).astype(np.int64)
    y.setflags(write=False)
    return y


CASES = [(n, how) for n in NS for how in LABELLINGS]


@functools.lru_cache(maxsize=None)
def expected(n: int, how: str, edges_key=None):
    """(restatement of the label-0 scores, of the label-1 scores); None for a group without members; how=None: all scores, once"""
    edges = None if edges_key is None else explicit_edges(edges_key)
    s = scores(n)
    if how is None:
        return restate(s, edges)
    y = labels(n, how)
    return tuple(restate(s[y == k], edges) if (y == k).any() else None for k in (0, 1))


def explicit_edges(key: str) -> np.ndarray:
    if key == "three":
        return np.array([-1.0, 0.0, 1.0])
    assert key == "cap"
    return np.linspace(-40.0, 40.0, 4001)


def check(got, values, want: dict, what=""):
    """`got` (a Histogram, or None for an empty group) against the restatement `want` of `values`: buckets, limits, num, min and max
    exactly; sum and sum_squares against math.fsum within n * 2^-53 * sum|v| resp. n * 2^-53 * sum v^2, the worst case of any
    summation order"""
    if want is None:
        assert got is None, what
        return
    assert got is not None, what
    assert got.bucket == want["bucket"], what
    assert got.bucket_limit == want["bucket_limit"], what
    assert all(isinstance(c, int) for c in got.bucket) and all(isinstance(x, float) for x in got.bucket_limit), what
    assert (got.num, got.min, got.max) == (want["num"], want["min"], want["max"]), what
    v = [float(x) for x in np.asarray(values, np.float64).reshape(-1)]
    n = len(v)
    s, a = math.fsum(v), math.fsum(abs(x) for x in v)
    q = math.fsum(x * x for x in v)
    print(f"{what}: n={n} sum {got.sum!r} (fsum {s!r}, bound {n * U * a:.3e}) sum_squares {got.sum_squares!r} (fsum {q!r}, bound {n * U * q:.3e})")
    assert abs(got.sum - s) <= n * U * a, (what, got.sum, s)
    assert abs(got.sum_squares - q) <= n * U * q, (what, got.sum_squares, q)
