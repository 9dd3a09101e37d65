"""Shared by tests/test_cpu_breakdown.py and tests/test_gpu_breakdown.py: seeded cases for `eoe_amd.metrics.class_breakdown` (scores,
class ids, normal classes), the sub-problems written out for sklearn, and the comparison of two `Breakdown`s."""
import numpy as np

KINDS = ("continuous", "quant8", "equal", "zeros")
LEVELS = (1e-9, 0.5, 0.95, 1.0)                 # 1e-9: place m = 1; 1.0: the last positive


def scores(n: int, kind: str, seed: int = 0) -> np.ndarray:
    """float32 [n]: continuous; quantised to 8 levels (ties everywhere); all equal; -0.0 / 0.0 / a few other values"""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    if kind == "continuous":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "quant8":
        return (np.floor(rng.random(n) * 8.0) / 8.0).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=n)


def class_ids(n: int, K: int, seed: int = 0, spread: bool = False) -> np.ndarray:
    """int64 [n] over min(K, n) classes, every one of them present, in no order; `spread`: ids that are neither dense nor sorted"""
    K = min(K, n)
    rng = np.random.default_rng([seed, n, K])
    ids = np.concatenate([np.arange(K), rng.integers(0, K, n - K)])
    ids = ids[rng.permutation(n)].astype(np.int64)
    return (ids * 7 + 3) % 1031 if spread else ids          # 7 is a unit mod the prime 1031: distinct ids stay distinct


def normal_sets(ids: np.ndarray):
    """the normal-class sets to try on these ids: one class (one_vs_rest), all but one (leave_one_out), every second, all, none"""
    present = np.unique(ids)
    sets = [present[:1], present[1:], present[::2], present, present[:0]]
    seen, out = set(), []
    for s in sets:
        if tuple(s) not in seen:
            seen.add(tuple(s))
            out.append([int(c) for c in s])
    return out


def named_cases():
    """(name, scores, ids, normal classes): the cases the issue lists, small enough for sklearn per class"""
    cases = []
    for kind in KINDS:                                                              # both sides with several classes
        cases.append((f"{kind}/5 classes", scores(300, kind), class_ids(300, 5), [0, 3]))
    cases.append(("non-contiguous ids", scores(200, "quant8", 1), class_ids(200, 6, 1, spread=True),
                  [int(c) for c in np.unique(class_ids(200, 6, 1, spread=True))[[1, 4]]]))
    ids = class_ids(120, 4, 2)
    ids[ids == 2] = 1
    ids[7] = 2                                                                      # class 2: one sample, anomalous
    cases.append(("a class of one sample (anomalous)", scores(120, "continuous", 2), ids.copy(), [0]))
    cases.append(("a class of one sample (nominal)", scores(120, "quant8", 2), ids.copy(), [2, 1]))
    cases.append(("one class per side", scores(90, "zeros", 3), class_ids(90, 2, 3), [1]))
    cases.append(("one_vs_rest", scores(257, "continuous", 4), class_ids(257, 10, 4), [6]))
    cases.append(("leave_one_out", scores(257, "quant8", 4), class_ids(257, 10, 4), [c for c in range(10) if c != 6]))
    # 20 positives in the anomalous class 1 and 20 in the pooled problem: 19 / 20 is the place boundary
    ids = np.array([0] * 30 + [1] * 20 + [2] * 15, dtype=np.int64)
    cases.append(("twenty positives", scores(65, "continuous", 5), ids, [0, 2]))
    cases.append(("twenty positives, ties", scores(65, "quant8", 5), ids, [0, 2]))
    cases.append(("empty pool: no anomalous class", scores(50, "continuous", 6), class_ids(50, 3, 6), [0, 1, 2]))
    cases.append(("empty pool: no nominal class", scores(50, "quant8", 6), class_ids(50, 3, 6), []))
    return cases


def sub_problem(s, ids, normal, k):
    """(labels, scores) of class k against the pool of the other side; label 1 = anomalous"""
    anomalous = ~np.isin(ids, normal)
    side_k = int(k not in normal)
    keep = (ids == k) | (anomalous != bool(side_k))
    return anomalous[keep].astype(np.int64), s[keep]


def assert_same(a, b, what=""):
    """two `Breakdown`s of the same problem from the two paths: the integer tables equal, the thresholds bit-equal, the rates equal
    (one float64 division of equal integers), the APs within n_k * 2^-52 (each is a float64 sum of n_k terms in [0, 1] over n_k)"""
    assert np.array_equal(a.classes, b.classes) and a.names == b.names and np.array_equal(a.side, b.side), what
    assert np.array_equal(a.n, b.n) and a.tpr_level == b.tpr_level, what
    assert a.counts.dtype == b.counts.dtype == np.int64 and np.array_equal(a.counts, b.counts), (what, a.counts, b.counts)
    assert a.thresholds.dtype == b.thresholds.dtype and a.thresholds.tobytes() == b.thresholds.tobytes(), (what, a.thresholds, b.thresholds)
    assert np.array_equal(a.auc, b.auc, equal_nan=True) and np.array_equal(a.fpr, b.fpr, equal_nan=True), what
    assert np.array_equal([a.fpr_at_tpr, a.threshold], [b.fpr_at_tpr, b.threshold], equal_nan=True), what
    for k, (x, y) in enumerate(zip(a.ap, b.ap)):
        if x is None or y is None or x != x or y != y:
            assert (x is None and y is None) or (x != x and y != y), (what, k, x, y)
        else:
            assert abs(x - y) <= int(a.n[k]) * 2.0 ** -52, (what, k, x, y)
