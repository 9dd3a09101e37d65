"""Shared by tests/test_cpu_mahalanobis.py and tests/test_gpu_mahalanobis.py: the feature sets, the shapes and the float64 checks of the
Gaussian baseline (eoe_amd.mahalanobis, csrc/mahalanobis.hip).  Nothing here touches a GPU."""
import numpy as np

from eoe_amd.mahalanobis import mahalanobis_np, moments_np

U = 2.0 ** -24                                 # the unit roundoff of fp32

# The smallest sizes at which the kernels' edges can go wrong.  Tiles are 128 wide (columns of the scatter matrix; queries and rows of
# W of the score), the k-step is 32 (rows of x for the scatter, columns for the score), loads are quads of 4 columns, the scatter's
# rows are cut into slices that are multiples of 32 rows, the column sums into slices of 256 rows, 512 slices at most.
#   rows      1, 2: a single row / pair; 31, 33: one k-step less and more one row; 129, 130: a query tile and one or two rows;
#             1025: four column-sum slices and one row, 33 scatter slices at D <= 128; 2051: 65 scatter slices at D <= 128, 17 query
#             tiles; 131329: more than 512 column-sum slices of 256 rows, so the slices grow to 257 rows (fits only, narrow)
#   D         1, 2, 3: less than a quad; 63, 64, 65: two k-steps less one, exactly, plus one; 127, 129: a tile less and more one;
#             256: two whole tiles (3 upper tiles); 515: five tiles, the last ragged, rows that are no multiple of 16 bytes
#   P         1, 3: less than a quad of rows; 64, 65: a wave's rows and one more; D: the square case that `lower` takes
FIT_NS = (2, 31, 33, 129, 130, 1025, 2051, 131329)
NQS = (1, 2, 31, 33, 129, 130, 1025, 2051)
DS = (1, 2, 3, 63, 64, 65, 127, 129, 256, 515)
PS = (1, 3, 64, 65, "D")
FIT_COVER = (  # (n, D)
    (2, 1), (2, 129), (31, 2), (31, 256), (33, 3), (33, 515), (129, 63), (129, 1), (130, 64), (130, 127), (1025, 65), (1025, 256),
    (2051, 127), (2051, 515), (131329, 1), (131329, 3), (1025, 2), (2051, 64), (130, 63), (33, 65), (31, 129), (2, 3),
)
SCORE_COVER = (  # (nq, D, P); P == "D": the square case
    (1, 1, 1), (2, 2, "D"), (31, 3, 3), (33, 63, 64), (129, 64, 65), (130, 65, "D"), (1025, 127, 1), (2051, 129, 3), (1, 256, 64),
    (2, 515, 65), (31, 515, "D"), (33, 256, "D"), (129, 129, 1), (130, 127, 64), (1025, 1, 65), (2051, 2, 3), (1, 3, "D"), (2, 63, 1),
    (2051, 64, "D"), (1025, 65, 3),
)
REAL_FITS = ((33, 65), (1025, 256), (2051, 515), (130, 3))
REAL_SCORES = ((33, 65, 65), (130, 256, 256), (1025, 515, 515), (31, 129, 64))
MAGNITUDES = (1e-3, 1.0, 1e3)


def cover_is_complete():
    """every value of every axis appears in its table at least twice, against different partners"""
    def twice(table, axis, values):
        for v in values:
            partners = {tuple(x for a, x in enumerate(c) if a != axis) for c in table if c[axis] == v}
            if len(partners) < 2:
                return False
        return {c[axis] for c in table} == set(values)
    return (twice(FIT_COVER, 0, FIT_NS) and twice(FIT_COVER, 1, DS) and twice(SCORE_COVER, 0, NQS) and twice(SCORE_COVER, 1, DS)
            and twice(SCORE_COVER, 2, PS))


def paired_features(n, D, seed, c=3):
    """fp32 [n, D]: n // 2 rows v of integers in [-8, 8], their negations and, for an odd n, a zero row, permuted and shifted by c.
    The mean is exactly c, every centred value, product and partial sum is an integer below 2^24 and m4 is below 2^53: the mean, the
    scatter matrix and m4 are exact in any summation order."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, size=(n // 2, D))
    rows = np.concatenate([v, -v] + ([np.zeros((1, D), np.int64)] if n % 2 else []))
    x = (rows[rng.permutation(n)] + c).astype(np.float32)
    assert n * 64 < 2 ** 24 and n * (64.0 * D) ** 2 < 2 ** 53 and (x.astype(np.float64).mean(0) == c).all()
    return x


def exact_score_inputs(nq, D, P, seed):
    """(x fp32 [nq, D], mean fp32 [D], W fp32 [P, D]): x - mean holds integers in [-2, 2], the mean integers in [-4, 4], W = tril of
    integers in {-1, 0, 1}.  Asserted here for the data returned: every partial sum of a y_ij and of a d2_i stays below 2^24, so the
    result is exact in fp32 in any summation order."""
    rng = np.random.default_rng(seed)
    z = rng.integers(-2, 3, size=(nq, D))
    mean = rng.integers(-4, 5, size=D)
    W = np.tril(rng.integers(-1, 2, size=(P, D)))
    assert int((np.abs(z) @ np.abs(W).T).max()) < 2 ** 24 and int(((z @ W.T) ** 2).sum(1).max()) < 2 ** 24
    return (z + mean).astype(np.float32), mean.astype(np.float32), W.astype(np.float32)


def real_features(n, D, seed, magnitude=1.0, offset=0.0):
    return (np.random.default_rng(seed).standard_normal((n, D)) * magnitude + offset).astype(np.float32)


def real_score_inputs(nq, D, P, seed, magnitude=1.0, offset=0.0):
    """real-valued queries around a real-valued mean and a lower-triangular W with entries of the size of an inverse Cholesky factor"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((nq, D)) * magnitude + offset).astype(np.float32)
    mean = (rng.standard_normal(D) * 0.1 * magnitude + offset).astype(np.float32)
    W = np.tril(rng.standard_normal((P, D)) / (magnitude * np.sqrt(D))).astype(np.float32)
    return x, mean, W


def check_exact_fit(mean, scatter, m4, counts, x, what=""):
    """the four results of a fit over `paired_features` equal moments_np's bit for bit, both triangles of the scatter matrix included"""
    want_mean, want_S, want_m4, want_counts = moments_np(x)
    D = x.shape[1]
    assert tuple(int(c) for c in counts) == want_counts, f"{what}: counts {counts}, not {want_counts}"
    assert np.asarray(mean, np.float32).tobytes() == want_mean.tobytes(), f"{what}: mean"
    S = np.asarray(scatter, np.float64).reshape(D, D)
    assert S.tobytes() == S.T.copy().tobytes(), f"{what}: the scatter matrix is not symmetric"
    np.testing.assert_array_equal(S, want_S, err_msg=f"{what}: scatter")
    assert float(m4) == want_m4, f"{what}: m4 {float(m4)}, not {want_m4}"


def check_real_fit(mean, scatter, m4, counts, x, what=""):
    """A fit over real-valued features against float64 of the same fp32 x, with first-order rounding bounds, not measured tolerances:
      * mean: the float64 column sum is rounded once, |mean - mean64| <= 2^-24 |mean64| + 2 n 2^-53 mean_i |x_i| (the second term: the
        two float64 sums, the kernel's and this check's)
      * scatter, against the float64 Z^T Z of the fp32 z = x - mean (the kernel's own mean): |S_ab - S64_ab| <= (n + 4) 2^-24
        sum_i |z_ia z_ib| -- a chain of at most n fmafs per slice, the slices added in float64
      * m4, against the float64 sum over the same z: |z_i|^2 is ceil(D / 64) fmafs and 6 additions per lane, all terms positive, so its
        relative error is (ceil(D / 64) + 6) 2^-24 to first order, taken as (ceil(D / 64) + 8) 2^-24, and twice that once squared
    Returns the largest |error| / bound of the scatter matrix (for printing)."""
    n, D = x.shape
    ok = np.isfinite(x).all(1)
    xs = x[ok]
    used = int(ok.sum())
    assert tuple(int(c) for c in counts) == (used, n - used), f"{what}: counts {counts}"
    mean = np.asarray(mean, np.float32)
    x64 = xs.astype(np.float64)
    mean64 = x64.mean(0)
    assert (np.abs(mean - mean64) <= U * np.abs(mean64) + 2 * used * 2.0 ** -53 * np.abs(x64).mean(0)).all(), f"{what}: mean"
    z = (xs - mean).astype(np.float64)
    S = np.asarray(scatter, np.float64).reshape(D, D)
    assert S.tobytes() == S.T.copy().tobytes(), f"{what}: the scatter matrix is not symmetric"
    bound = (used + 4) * U * (np.abs(z).T @ np.abs(z))
    err = np.abs(S - z.T @ z)
    assert (err <= bound).all(), f"{what}: scatter off by {err.max()} where the bound is {bound[err > bound].min()}"
    q = (z * z).sum(1)
    want_m4 = float((q * q).sum())
    assert abs(float(m4) - want_m4) <= 2 * (-(-D // 64) + 8) * U * want_m4, f"{what}: m4 {float(m4)} against {want_m4}"
    return float((err / np.where(bound > 0, bound, 1.0)).max())


def route_bounds(x):
    """How far a fit from the kernel's moments may lie from `moments_np`'s fit of the same fp32 features, from the bounds above:
    (E, e_mu, ds, S, mu, s) with
      * E [D, D] = (n + 4) 2^-24 sum_i |z_ia z_ib|, the scatter matrix's bound; e_mu = trace(E) / (n D), that of mu = trace(S) / (n D)
      * ds, the bound of the Ledoit-Wolf shrinkage s = min(beta, delta) / delta, carried through its formula term by term:
          delta_ = |S|_F^2 / n^2 moves by at most e_d = (2 sum |S_ab| E_ab + sum E_ab^2) / n^2,
          beta = (m4 / n - delta_) / (D n) by e_beta = (e4 / n + e_d) / (D n), e4 = 2 (ceil(D / 64) + 8) 2^-24 m4 (m4's bound),
          delta = (delta_ - tr^2 / D) / D by e_delta = (e_d + (2 tr e_tr + e_tr^2) / D) / D with tr = trace(S) / n, e_tr = trace(E) / n,
          min(beta, delta) by max(e_beta, e_delta), so s by ds = (max(e_beta, e_delta) + s e_delta) / (delta - e_delta)
    Not a measured tolerance.  The two routes' means may differ in a last bit; that moves S in second order only, which the caller
    covers with 1 %."""
    mean, S, m4, (n, _) = moments_np(x)
    D = x.shape[1]
    z = np.abs((x[np.isfinite(x).all(1)] - mean).astype(np.float64))
    E = (n + 4) * U * (z.T @ z)
    tr, e_tr = np.trace(S) / n, np.trace(E) / n
    e_d = (2 * (np.abs(S) * E).sum() + (E * E).sum()) / (n * n)
    delta_ = (S * S).sum() / (n * n)
    beta, e_beta = (m4 / n - delta_) / (D * n), (2 * (-(-D // 64) + 8) * U * m4 / n + e_d) / (D * n)
    delta, e_delta = (delta_ - tr * tr / D) / D, (e_d + (2 * tr * e_tr + e_tr * e_tr) / D) / D
    assert delta > e_delta > 0
    s = min(beta, delta) / delta
    return E, e_tr / D, (max(e_beta, e_delta) + s * e_delta) / (delta - e_delta), S, tr / D, s


def score_bound(x, mean, W):
    """(float64 d2 of the finite rows, its bound, the mask of the finite rows): the bound of `check_real_score`"""
    x64, m64, W64 = x.astype(np.float64), mean.astype(np.float64), W.astype(np.float64)
    P, D = W.shape
    ok = np.isfinite(x).all(1)
    z = x64[ok] - m64
    y = z @ W64.T
    a = np.abs(z) @ np.abs(W64).T
    want = (y * y).sum(1)
    return want, U * (2 * (D + 2) * (np.abs(y) * a).sum(1) + (P + 2) * want), ok


def check_exact_score(d2, x, mean, W, what=""):
    want = mahalanobis_np(x, mean, W)
    np.testing.assert_array_equal(np.asarray(d2, np.float64), want, err_msg=f"{what}: d2")


def check_real_score(d2, x, mean, W, what=""):
    """Every finite query row against float64 of the same fp32 x, mean and W:
      |d2 - d2_64| <= 2^-24 (2 (D + 2) sum_j |y_j| a_j + (P + 2) sum_j y_j^2),  a_j = sum_k |W_jk| |x_k - mean_k|
    -- the subtraction and a chain of D fmafs per y_j (an error of (D + 2) 2^-24 a_j, doubled by the square), then P squares and
    additions.  A first-order rounding bound, not a measured tolerance.  Returns the largest |error| / bound (for printing)."""
    want, bound, ok = score_bound(x, mean, W)
    d2 = np.asarray(d2, np.float64)
    assert np.isnan(d2[~ok]).all(), f"{what}: a non-finite query row must give NaN"
    err = np.abs(d2[ok] - want)
    assert (err <= bound).all(), f"{what}: d2 off by {err.max()} where the bound is {bound[err > bound].min()}"
    return float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
