"""Shared by tests/test_cpu_knn.py and tests/test_gpu_knn.py: the feature sets, the shapes and the float64 checks of the nearest-neighbour
search (eoe_amd.neighbors, csrc/knn.hip).  Nothing here touches a GPU."""
import numpy as np

from eoe_amd.neighbors import knn_np

# The smallest sizes at which tile edges (128 queries x 128 references, k-step 32), chunk edges (1 024 references) and the merge of
# several chunks can go wrong; every value of every axis appears in COVER at least twice, against different partners.
NQS = (1, 31, 33, 130)
NRS = (1, 3, 127, 129, 1023, 1025, 2051)
DS = (1, 2, 3, 63, 64, 65, 256, 515)
KS = (1, 5, 16, 64)
COVER = (  # (nq, nr, D, k)
    (1, 1, 1, 1), (1, 3, 2, 5), (31, 127, 3, 16), (33, 129, 63, 64), (130, 1023, 64, 5), (31, 1025, 65, 16), (33, 2051, 256, 1),
    (130, 2051, 515, 64), (1, 1025, 515, 5), (130, 129, 3, 64), (33, 3, 65, 16), (31, 1023, 2, 64), (130, 127, 1, 5),
    (1, 2051, 64, 16), (33, 1, 256, 64), (31, 3, 63, 1), (130, 1025, 2, 1), (33, 127, 1, 16), (1, 129, 256, 5), (31, 2051, 3, 5),
    (33, 1023, 63, 5),
)
# real-valued features: a chunk edge, several chunks, a ragged k tail and a list as long as the kernel takes
REAL_SHAPES = ((33, 1025, 65, 5), (130, 2051, 256, 16), (31, 129, 515, 64), (1, 1023, 3, 1))
MAGNITUDES = (1e-3, 1.0, 1e3)


def cover_is_complete():
    return all({c[a] for c in COVER} == set(vals) for a, vals in enumerate((NQS, NRS, DS, KS)))


def exact_features(n, D, seed, lo=-8, hi=8):
    """integers in [lo, hi] as fp32: every norm, dot product and squared distance is an integer below 2^18 (D <= 515), exact in fp32
    in any summation order"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, D)).astype(np.float32)


def real_features(n, D, seed, magnitude=1.0, offset=0.0):
    return (np.random.default_rng(seed).standard_normal((n, D)) * magnitude + offset).astype(np.float32)


def check_exact(idx, d2, q, r, k, what=""):
    """idx and d2 of a search over integer-valued features equal knn_np's, ties and tails included"""
    want_idx, want_d2, _ = knn_np(q, r, k)
    np.testing.assert_array_equal(np.asarray(idx, dtype=np.int64), want_idx, err_msg=f"{what}: indices")
    np.testing.assert_array_equal(np.asarray(d2, dtype=np.float64), want_d2, err_msg=f"{what}: distances")


def check_real(idx, d2, q, r, k, what=""):
    """The three properties of a search over real-valued features, for every query row, against float64 distances.
    B(q, r) = (2 D + 8) 2^-24 (|q|^2 + |r|^2) is the first-order rounding bound of an fp32 fmaf-chain norm and dot product plus two
    additions; it is not a measured tolerance.
      * a returned d2 lies within B of the float64 distance to the returned index
      * d2 is non-decreasing, equal values in ascending index
      * a reference that was not returned is no nearer in float64 than the k-th returned one, up to the bound of each of the two
        computed distances that were compared (2 B, each B taken at its own pair)
    Returns the largest |error| / B seen (for printing)."""
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    nq, D = q64.shape
    nr = r64.shape[0]
    idx, d2 = np.asarray(idx, dtype=np.int64), np.asarray(d2, dtype=np.float64)
    kk = min(k, nr)
    assert (idx[:, kk:] == -1).all() and np.isposinf(d2[:, kk:]).all(), f"{what}: the tail past the {nr} references"
    qn, rn = (q64 ** 2).sum(1), (r64 ** 2).sum(1)
    worst = 0.0
    for i in range(nq):
        true = ((q64[i][None, :] - r64) ** 2).sum(1)
        B = (2 * D + 8) * 2.0 ** -24 * (qn[i] + rn)
        got = idx[i, :kk]
        assert ((got >= 0) & (got < nr)).all() and np.unique(got).size == kk, f"{what}: row {i} returns {got}"
        err = np.abs(d2[i, :kk] - true[got])
        assert (err <= B[got]).all(), f"{what}: row {i}: d2 off by {err.max()} where the bound is {B[got].min()}"
        worst = max(worst, float((err / B[got]).max()))
        step = np.diff(d2[i, :kk])
        assert (step >= 0).all(), f"{what}: row {i}: distances descend"
        assert (np.diff(got)[step == 0] > 0).all(), f"{what}: row {i}: equal distances out of index order"
        rest = np.ones(nr, bool)
        rest[got] = False
        last = got[-1]
        assert (true[rest] >= true[last] - (B[rest] + B[last])).all(), f"{what}: row {i}: a nearer reference was left out"
    return worst
