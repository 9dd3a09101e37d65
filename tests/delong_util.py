"""Shared by tests/test_cpu_delong.py and tests/test_gpu_delong.py: seeded cases for `eoe_amd.metrics.delong` and the independent
statement of DeLong's estimator they are checked against -- float64 NumPy written from the definition: the m x n0 matrix psi (1, 1/2, 0),
its row and column means V10 and V01, `np.cov(..., ddof=1)` of them, and the doubled integer counts taken from the same matrix.  It
shares no code with the product's host path (no sort, no `searchsorted`)."""
import functools
import math
import warnings
from statistics import NormalDist

import numpy as np

SIZES = (2, 3, 64, 257, 1000)
SHARES = ("one", "tenth", "half", "all_but_one")
KINDS = ("continuous", "quant4", "equal", "zeros", "inf", "ignored")
COLUMNS = (1, 2, 3, 8)


def labels_for(n: int, share: str) -> np.ndarray:
    """label 1 on m of n samples, spread evenly: one sample, 10 %, 50 %, all but one"""
    m = {"one": 1, "tenth": max(1, n // 10), "half": n // 2, "all_but_one": n - 1}[share]
    y = np.zeros(n, np.int64)
    y[(np.arange(m) * n) // m] = 1
    return y


def make_case(n: int, share: str, kind: str, K: int, seed: int = 0):
    """(labels int64 [n], scores float32 [K, n]).  Column 0 is the base; columns 1 .. K-2 are the base plus small noise (correlated
    models); with K >= 2 the last column repeats the base bit for bit."""
    rng = np.random.default_rng([seed, n, SHARES.index(share), KINDS.index(kind), K])
    y = labels_for(n, share)
    base = rng.normal(size=n) + 0.8 * y
    cols = [base] + [base + 0.05 * (j + 1) * rng.normal(size=n) for j in range(max(K - 2, 0))]
    s = np.stack(cols).astype(np.float32)
    if kind == "quant4":                                              # heavy ties: four values
        s = (np.clip(np.floor(s + 2.0), 0.0, 3.0) / 4.0).astype(np.float32)
    elif kind == "equal":
        s[:] = np.float32(0.5)
    elif kind == "zeros":                                             # -0.0 against 0.0, and a few other values around them
        z = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s = np.where(rng.random(s.shape) < 0.7, z[None, :], np.sign(s) * np.float32(1.0)).astype(np.float32)
    elif kind == "inf":
        hit = rng.random(s.shape)
        s[hit < 0.15] = np.float32(np.inf)
        s[hit > 0.85] = np.float32(-np.inf)
    elif kind == "ignored":                                           # a fifth of the samples carries label -1 and a NaN score
        drop = rng.random(n) < 0.2
        y = np.where(drop, -1, y)
        s[:, drop] = np.float32(np.nan)
    if K >= 2:
        s = np.concatenate([s, s[:1]])
    return y, np.ascontiguousarray(s[:K] if K == 1 else s)


@functools.lru_cache(maxsize=None)
def case(n: int, share: str, kind: str, K: int):
    y, s = make_case(n, share, kind, K)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s, brute_force(y, s)


def grid():
    """the (n, share, kind, K) of the CPU grid: every size, share and kind at K = 1 and 3, every K at the continuous and the tied kind"""
    out = [(n, sh, kd, K) for n in SIZES for sh in SHARES for kd in KINDS for K in (1, 3)]
    out += [(n, sh, kd, K) for n in SIZES for sh in SHARES for kd in ("continuous", "quant4") for K in (2, 8)]
    return out


def pairs(K: int):
    return [(k, l) for k in range(K) for l in range(k, K)]


def brute_force(y: np.ndarray, s: np.ndarray) -> dict:
    """DeLong from the definition.  Integers: T_pos, T_neg [K], A, B [K (K + 1) / 2], m, n0; floats: auc [K], cov [K, K]"""
    K = s.shape[0]
    pos, neg = y == 1, y == 0
    m, n0 = int(pos.sum()), int(neg.sum())
    a, b = np.zeros((K, m), np.int64), np.zeros((K, n0), np.int64)
    v10, v01, auc = np.zeros((K, m)), np.zeros((K, n0)), np.full(K, np.nan)
    for k in range(K):
        sp, sn = s[k][pos], s[k][neg]
        gt, eq = sp[:, None] > sn[None, :], sp[:, None] == sn[None, :]
        doubled = 2 * gt.astype(np.int64) + eq.astype(np.int64)
        a[k], b[k] = doubled.sum(axis=1), doubled.sum(axis=0)
        if m and n0:
            psi = gt.astype(np.float64) + 0.5 * eq.astype(np.float64)
            v10[k], v01[k], auc[k] = psi.mean(axis=1), psi.mean(axis=0), psi.mean()
    ref = {"m": m, "n0": n0, "T_pos": a.sum(axis=1), "T_neg": b.sum(axis=1),
           "A": np.array([int(np.sum(a[k] * a[l])) for k, l in pairs(K)], np.int64),
           "B": np.array([int(np.sum(b[k] * b[l])) for k, l in pairs(K)], np.int64), "auc": auc}
    cov = np.full((K, K), np.nan)
    if m > 1 and n0 > 1:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cov = np.atleast_2d(np.cov(v10, ddof=1)) / m + np.atleast_2d(np.cov(v01, ddof=1)) / n0
    ref["cov"] = cov
    return ref


def table_of(test) -> dict:
    """an `AucTest`'s integer table in the layout of `brute_force`"""
    c = test.counts
    return {"m": c["n_pos"], "n0": c["n_neg"], "T_pos": c["T_pos"], "T_neg": c["T_neg"], "A": c["A"], "B": c["B"]}


def assert_tables_equal(got: dict, want: dict, what):
    assert got["m"] == want["m"] and got["n0"] == want["n0"], what
    for key in ("T_pos", "T_neg", "A", "B"):
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, key, g.tolist(), w.tolist())
    assert np.array_equal(got["T_pos"], got["T_neg"]), what


# ---- float checks: 1e-9 relative against the brute force, nothing absolute.  The product divides exact integers once; the brute force
# sums at most 1e5 float64 terms, about 2e-11: the bound allows 50 x that.  Where the brute force's INTEGERS say that a covariance is
# zero (m A == T T and n0 B == T T) the product's must be the float 0.0 exactly.
REL = 1e-9


def close(got, want) -> bool:
    return abs(got - want) <= REL * abs(want)


def assert_floats_agree(test, ref, what, level: float = 0.95):
    K = ref["auc"].size
    m, n0 = ref["m"], ref["n0"]
    assert test.n_pos == m and test.n_neg == n0 and test.auc.shape == (K,) and test.cov.shape == (K, K), what
    assert np.all(np.abs(test.auc - ref["auc"]) <= REL * np.abs(ref["auc"])), (what, test.auc, ref["auc"])
    lo, hi = test.ci(level)
    if not (m > 1 and n0 > 1):
        assert np.isnan(test.cov).all() and np.isnan(test.var).all() and np.isnan(test.se).all(), what
        assert np.isnan(lo).all() and np.isnan(hi).all(), what
        return
    assert np.all(np.abs(test.cov - ref["cov"]) <= REL * np.abs(ref["cov"])), (what, test.cov, ref["cov"])
    for p, (k, l) in enumerate(pairs(K)):
        tt = int(ref["T_pos"][k]) * int(ref["T_pos"][l])
        if m * int(ref["A"][p]) == tt and n0 * int(ref["B"][p]) == tt:
            assert test.cov[k, l] == 0.0 and test.cov[l, k] == 0.0 and (k != l or (test.var[k] == 0.0 and test.se[k] == 0.0)), (what, k, l)
    assert np.array_equal(test.var, np.diagonal(test.cov)) and np.array_equal(test.se, np.sqrt(test.var)), what
    assert np.all(test.var >= 0.0), what
    z = NormalDist().inv_cdf((1.0 + level) / 2.0)
    for k in range(K):
        se = math.sqrt(float(ref["cov"][k, k]))
        for got, want in ((lo[k], min(max(ref["auc"][k] - z * se, 0.0), 1.0)), (hi[k], min(max(ref["auc"][k] + z * se, 0.0), 1.0))):
            assert close(got, want), (what, k, got, want)
        assert 0.0 <= lo[k] <= test.auc[k] <= hi[k] <= 1.0, (what, k)
    for k in range(K):
        for l in range(K):
            diff, zz, p = test.compare(k, l)
            want_diff = float(ref["auc"][k] - ref["auc"][l])
            assert close(diff, want_diff), (what, k, l, diff, want_diff)
            vd = float(ref["cov"][k, k] + ref["cov"][l, l] - 2.0 * ref["cov"][k, l])
            if vd == 0.0:                                              # the definition for a difference without variance
                want_z, want_p = (0.0, 1.0) if want_diff == 0.0 else (math.copysign(math.inf, want_diff), 0.0)
                assert (zz, p) == (want_z, want_p), (what, k, l, zz, p)
                continue
            want_z = want_diff / math.sqrt(vd)
            assert close(zz, want_z) and close(p, math.erfc(abs(want_z) / math.sqrt(2.0))), (what, k, l, zz, want_z, p)
