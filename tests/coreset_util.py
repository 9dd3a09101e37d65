"""Shared by tests/test_cpu_coreset.py and tests/test_gpu_coreset.py: the feature sets, the shapes and the float64 checks of the greedy
k-center selection (eoe_amd.coreset, csrc/coreset.hip).  Nothing here touches a GPU."""
import numpy as np

from eoe_amd.coreset import CORESET_ROWS_PER_WAVE as W, CORESET_ROWS_PER_WORKGROUP as R, kcenter_np

# The smallest sizes at which the kernel's row map can go wrong: a wave takes W rows, a workgroup R; one value above 2 000 rows for
# many workgroups.  Columns: a lane takes four at a time, a wave 256.
NS = (1, 2, W - 1, W, W + 1, R - 1, R, R + 1, 2 * R + 1, 2051)
DS = (1, 3, 4, 63, 64, 65, 515, 2048)
COVER = (  # (n, D, m, start)
    (1, 1, 1, 0), (2, 3, 2, 1), (2, 64, 1, 0), (W - 1, 4, W - 2, 3), (W, 63, W, W - 1), (W + 1, 65, 2, 4),
    (R - 1, 515, R - 2, R - 2), (R, 2048, R, 0), (R + 1, 64, (R + 1) // 8, R // 2), (2 * R + 1, 3, 2 * R + 1, 2 * R),
    (2 * R + 1, 2048, (2 * R + 1) // 8, 1), (2051, 4, 2051, 1000), (2051, 65, 2051 // 8, 2050), (2051, 515, 2, 0),
    (R + 1, 1, R, 0), (W + 1, 2048, W + 1, W), (W - 1, 515, 1, W - 2), (R - 1, 1, 2, R // 2), (W, 65, W - 1, 0),
    (R, 3, R - 1, R - 1), (2, 4, 2, 0), (1, 63, 1, 0),
)


def cover_is_complete():
    """every n and D above, m in {1, 2, n - 1, n} and one m = n // 8 of a set of 16 rows or more, start at 0, at n - 1 and inside"""
    ns, ds = {c[0] for c in COVER}, {c[1] for c in COVER}
    ms = {"1": any(m == 1 for _, _, m, _ in COVER), "2": any(m == 2 for _, _, m, _ in COVER),
          "n-1": any(m == n - 1 and n > 3 for n, _, m, _ in COVER), "n": any(m == n and n > 2 for n, _, m, _ in COVER),
          "n/8": any(m == n // 8 and n >= 16 for n, _, m, _ in COVER)}
    starts = {"0": any(s == 0 and n > 1 for n, _, _, s in COVER), "n-1": any(s == n - 1 and n > 1 for n, _, _, s in COVER),
              "inside": any(0 < s < n - 1 for n, _, _, s in COVER)}
    in_range = all(1 <= m <= n and 0 <= s < n for n, _, m, s in COVER)
    return ns == set(NS) and ds == set(DS) and all(ms.values()) and all(starts.values()) and in_range


def exact_features(n, D, seed, lo=-8, hi=8):
    """integers in [lo, hi] as fp32: every difference is an integer of at most 16 in size and every squared distance an integer below
    2^20 (D <= 2048), exact in fp32 in any summation order"""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, D)).astype(np.float32)


def real_features(n, D, seed, magnitude=1.0, offset=0.0):
    return (np.random.default_rng(seed).standard_normal((n, D)) * magnitude + offset).astype(np.float32)


def check_exact(idx, radius, assign, d2min, x, m, start, what=""):
    """the four outputs of a selection over integer-valued features are `kcenter_np`'s, byte for byte once its float64 distances are
    rounded to fp32 (they are integers: the rounding changes nothing); NaN entries compare by their position"""
    want_idx, want_radius, want_assign, want_d2min, _ = kcenter_np(x, m, start)
    np.testing.assert_array_equal(np.asarray(idx, dtype=np.int64), want_idx, err_msg=f"{what}: idx")
    np.testing.assert_array_equal(np.asarray(assign, dtype=np.int64), want_assign, err_msg=f"{what}: assign")
    for name, got, want in (("radius", radius, want_radius), ("d2min", d2min, want_d2min)):
        got, want = np.asarray(got, dtype=np.float32), want.astype(np.float32)
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: {name}: NaN positions"
        assert np.where(np.isnan(got), np.float32(0), got).tobytes() == np.where(np.isnan(want), np.float32(0), want).tobytes(), \
            f"{what}: {name}: {got} against {want}"


def gamma(D):
    """the relative error bound of an fp32 squared distance in the difference form: every term (x - c)^2 takes the rounding of the
    difference twice (it is squared) and at most D roundings of the sums it passes through, D + 2 factors (1 + e), |e| <= 2^-24"""
    u = (D + 2) * 2.0 ** -24
    return u / (1.0 - u)


def check_real(idx, radius, d2min, x, what=""):
    """The device's own sequence replayed in float64 on real-valued features (no non-finite rows), at EVERY step t >= 1:
      * the chosen row's true distance to its nearest earlier centre is at least (1 - g) / (1 + g) of the true maximum over the
        rows not yet chosen (it was the largest COMPUTED one, and both were computed within g)
      * radius[t] lies within g, relatively, of that true distance
    and at the end d2min lies within g of the true distance to the nearest centre.  g = gamma(D).
    Returns (the smallest chosen / maximum ratio, the largest relative error / g) for printing."""
    x64 = x.astype(np.float64)
    n, D = x64.shape
    g = gamma(D)
    idx, radius, d2min = np.asarray(idx, dtype=np.int64), np.asarray(radius, dtype=np.float64), np.asarray(d2min, dtype=np.float64)
    assert ((idx >= 0) & (idx < n)).all() and np.unique(idx).size == idx.size, f"{what}: centres {idx}"
    assert np.isposinf(radius[0])
    true = ((x64 - x64[idx[0]]) ** 2).sum(1)
    free = np.ones(n, bool)
    free[idx[0]] = False
    ratio, err = 1.0, 0.0
    for t in range(1, idx.size):
        c = idx[t]
        assert free[c], f"{what}: step {t} chooses row {c} again"
        top = true[free].max()
        assert true[c] >= (1 - g) / (1 + g) * top, f"{what}: step {t}: row {c} lies at {true[c]}, the farthest row at {top}"
        assert abs(radius[t] - true[c]) <= g * true[c], f"{what}: step {t}: radius {radius[t]} against {true[c]}"
        if top > 0:
            ratio, err = min(ratio, true[c] / top), max(err, abs(radius[t] - true[c]) / (g * true[c]))
        free[c] = False
        true = np.minimum(true, ((x64 - x64[c]) ** 2).sum(1))
    assert (np.abs(d2min - true) <= g * true).all(), f"{what}: d2min off by {np.abs(d2min - true).max()}"
    assert (d2min[idx] == 0).all()
    pos = true > 0
    if pos.any():
        err = max(err, float((np.abs(d2min - true)[pos] / (g * true[pos])).max()))
    return ratio, err
