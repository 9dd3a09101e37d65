"""The Gaussian baseline in feature space: a mean and a shrunk covariance fitted to the normal training features, and the Mahalanobis
distance of a test feature from them -- the parametric comparison that outlier-exposure results are reported against, next to the
k-NN one of `eoe_amd.neighbors`.

  fit_gaussian(feats, shrinkage)   mean, Ledoit-Wolf (or fixed) shrunk covariance and its inverse Cholesky factor -> `FeatureGaussian`.
                                   GPU tensors take their moments from `eoe_feature_moments` (csrc/mahalanobis.hip: the scatter matrix on
                                   the fp32 matrix cores, no centred copy of the features), CPU tensors and arrays from `moments_np`.
  mahalanobis(queries, gauss)      squared distances, fp32 [nq]: GPU tensors through `eoe_mahalanobis_score`, the rest through
                                   `mahalanobis_np`.
  mahalanobis_score(d2)            the distance: the square root.
  moments_np, ledoit_wolf_np, mahalanobis_np   the statements of the results in float64 NumPy.

One contract for both routes: a feature row with a NaN or an infinity is left out of the fit and counted (`nonfinite`); a query row
with one gets d2 = NaN.  The mean is the float64 column mean rounded once to fp32, the centred values are formed in fp32, the
covariance is (1 - s) S / n + s mu I with mu = trace(S) / (n D), and W = L^-1 (cov = L L^T, float64 on the host) is rounded once to fp32:
d2 = |W (x - mean)|^2.
"""
import numpy as np

from .neighbors import _host, _rows

MAHALANOBIS_MAX_D = 2048


class FeatureGaussian:
    """`mean` fp32 [D] and `W` fp32 [D, D] (lower triangular, the inverse Cholesky factor of `cov`): tensors on the device of the
    features; `cov` float64 [D, D] NumPy, after shrinkage; `shrinkage` in [0, 1]; `n` rows fitted, `nonfinite` rows left out.
    `lower`: W is lower triangular, as `fit_gaussian` makes it (a hand-made W of other directions sets it False)."""

    def __init__(self, mean, cov, shrinkage, W, n, nonfinite, lower: bool = True):
        self.mean, self.cov, self.shrinkage, self.W = mean, cov, float(shrinkage), W
        self.n, self.nonfinite, self.lower = int(n), int(nonfinite), bool(lower)

    def __repr__(self):
        return f"FeatureGaussian(D={self.cov.shape[0]}, n={self.n}, shrinkage={self.shrinkage:.6g}, nonfinite={self.nonfinite})"


def check_shrinkage(shrinkage):
    """"ledoit_wolf" or a number in [0, 1], returned as it is"""
    if isinstance(shrinkage, str):
        if shrinkage != "ledoit_wolf":
            raise ValueError(f"shrinkage must be 'ledoit_wolf' or a number in [0, 1], not {shrinkage!r}")
    elif isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float, np.integer, np.floating)) or not 0.0 <= shrinkage <= 1.0:
        raise ValueError(f"shrinkage must be 'ledoit_wolf' or a number in [0, 1], not {shrinkage!r}")
    return shrinkage


def _features(x, what="feats"):
    x = np.asarray(_host(x))
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"{what} must be [n, D] with D >= 1, not {x.shape}")
    return x.astype(np.float32, copy=False)


def moments_np(x):
    """(mean fp32 [D], scatter float64 [D, D], m4 float, (rows used, rows excluded)) of fp32 features [n, D], as the kernel defines
    them: over the rows without a NaN or an infinity, mean = float64 column mean rounded to fp32, z = x - mean formed in fp32,
    scatter = Z^T Z and m4 = sum_i (|z_i|^2)^2 in float64.  No row used: zeros."""
    x = _features(x)
    n, D = x.shape
    ok = np.isfinite(x).all(axis=1)
    used = int(ok.sum())
    if used == 0:
        return np.zeros(D, np.float32), np.zeros((D, D), np.float64), 0.0, (0, n)
    xs = x[ok]
    mean = (xs.astype(np.float64).sum(axis=0) / used).astype(np.float32)
    z = (xs - mean).astype(np.float64)                     # fp32 - fp32, rounded to fp32, then widened
    q = (z * z).sum(axis=1)
    return mean, z.T @ z, float((q * q).sum()), (used, n - used)


def ledoit_wolf_np(scatter, m4: float, n: int) -> float:
    """The Ledoit-Wolf shrinkage of the biased covariance S / n, from the scatter matrix S of n centred rows and their fourth moment
    m4 = sum_i (|z_i|^2)^2: sklearn's `ledoit_wolf_shrinkage`, whose sum over the products of squared columns is m4."""
    S = np.asarray(scatter, dtype=np.float64)
    D = S.shape[0]
    if S.shape != (D, D) or n < 1:
        raise ValueError(f"scatter must be [D, D] of n >= 1 rows, not {S.shape} of {n}")
    tr = np.trace(S) / n
    mu = tr / D
    delta_ = float((S * S).sum()) / (n * n)
    beta = (m4 / n - delta_) / (D * n)
    delta = (delta_ - 2.0 * mu * tr + D * mu * mu) / D
    beta = min(beta, delta)
    return 0.0 if beta == 0 else float(beta / delta)


def mahalanobis_np(q, mean, W):
    """float64 [nq]: sum_j (sum_k W[j,k] (q[i,k] - mean[k]))^2 of the values given, NaN for a query row with a NaN or an infinity"""
    q = np.asarray(_host(q), dtype=np.float64)
    mean, W = np.asarray(_host(mean), dtype=np.float64).ravel(), np.asarray(_host(W), dtype=np.float64)
    if q.ndim != 2 or W.ndim != 2 or W.shape[1] != q.shape[1] or mean.size != q.shape[1]:
        raise ValueError(f"queries [nq, D], mean [D] and W [P, D] do not fit: {q.shape}, {mean.shape}, {W.shape}")
    ok = np.isfinite(q).all(axis=1)
    d2 = np.full(q.shape[0], np.nan, np.float64)
    y = (q[ok] - mean) @ W.T
    d2[ok] = (y * y).sum(axis=1)
    return d2


def _device_rows(name, t, fn):
    import torch
    if not (hasattr(t, "is_cuda") and t.is_cuda):
        raise RuntimeError(f"{fn} needs GPU tensors ({name} is not one; the public functions take host arrays as they are)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D float32 tensor, not {tuple(t.shape)} {t.dtype}")
    if not 1 <= t.shape[1] <= MAHALANOBIS_MAX_D:
        raise ValueError(f"the feature width must be in [1, {MAHALANOBIS_MAX_D}], not {t.shape[1]}")


def _scratch(scratch, need, dev):
    import torch
    if scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if scratch.dtype != torch.uint8 or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous() or scratch.data_ptr() % 16:
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {dev}")
    return scratch


def moments_device(x, scratch=None):
    """`eoe_feature_moments` on a GPU-resident fp32 [n, D] tensor (rows may be strided, the last axis is contiguous): (mean fp32 [D],
    scatter float64 [D, D], m4 float64 [1], counts int32 [2] = rows used, rows excluded) on the device.  `scratch`: a uint8 GPU tensor
    of at least `eoe_feature_moments_scratch_bytes(n, D)` bytes to reuse (its content does not matter)."""
    import torch
    from ._lib import check, lib
    _device_rows("feats", x, "moments_device")
    n, D = x.shape
    x, ld = _rows(x.detach(), D)
    dev = x.device
    mean = torch.empty(D, dtype=torch.float32, device=dev)
    scatter = torch.empty((D, D), dtype=torch.float64, device=dev)
    m4 = torch.empty(1, dtype=torch.float64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    scratch = _scratch(scratch, lib.eoe_feature_moments_scratch_bytes(n, D), dev)
    xp = x.data_ptr() if n else mean.data_ptr()          # an empty tensor has no storage to point at; nothing of it is read
    with torch.cuda.device(dev):
        check(lib.eoe_feature_moments(xp, ld, n, D, mean.data_ptr(), scatter.data_ptr(), m4.data_ptr(), counts.data_ptr(),
                                      scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "eoe_feature_moments")
    return mean, scatter, m4, counts


def mahalanobis_device(queries, mean, W, lower: bool = False, scratch=None):
    """`eoe_mahalanobis_score` on GPU-resident fp32 tensors: queries [nq, D] and W [P, D] (rows may be strided), mean [D] ->
    (d2 fp32 [nq], count int32 [1] of the non-finite query rows) on the device.  `lower=True` (P == D) promises a lower-triangular
    W and skips the k-steps above the diagonal."""
    import torch
    from ._lib import check, lib
    _device_rows("queries", queries, "mahalanobis_device")
    _device_rows("W", W, "mahalanobis_device")
    nq, D = queries.shape
    P = W.shape[0]
    if W.shape[1] != D or not 1 <= P <= MAHALANOBIS_MAX_D or W.device != queries.device:
        raise ValueError(f"W must be [P, {D}] with 1 <= P <= {MAHALANOBIS_MAX_D} on the queries' device, not {tuple(W.shape)} on {W.device}")
    if not (hasattr(mean, "is_cuda") and mean.is_cuda) or mean.dtype != torch.float32 or mean.numel() != D or mean.device != queries.device:
        raise ValueError(f"mean must be a float32 GPU tensor of {D} entries on the queries' device")
    if lower and P != D:
        raise ValueError(f"lower=True needs a square W, not {tuple(W.shape)}")
    (q, ldq), (w, ldw) = _rows(queries.detach(), D), _rows(W.detach(), D)
    mean = mean.detach().reshape(-1).contiguous()
    dev = q.device
    d2 = torch.empty(nq, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = _scratch(scratch, lib.eoe_mahalanobis_score_scratch_bytes(nq, D, P), dev)
    if nq == 0:
        return d2, count
    with torch.cuda.device(dev):
        check(lib.eoe_mahalanobis_score(q.data_ptr(), ldq, nq, D, mean.data_ptr(), w.data_ptr(), ldw, P, 1 if lower else 0, d2.data_ptr(),
                                        count.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
              "eoe_mahalanobis_score")
    return d2, count


def fit_gaussian(feats, shrinkage="ledoit_wolf") -> FeatureGaussian:
    """Mean and shrunk covariance of the rows of `feats` [n, D] (fp32): GPU tensors through `eoe_feature_moments`, CPU tensors and arrays
    through `moments_np`.  `shrinkage`: "ledoit_wolf" (`ledoit_wolf_np`) or a number s in [0, 1]; cov = (1 - s) S / n + s mu I.  The
    Cholesky factor and its inverse are taken in float64 on the host (D <= 2048) and rounded once to fp32.  Refuses fewer than 2
    usable rows and a covariance that is not positive definite."""
    import torch
    check_shrinkage(shrinkage)
    on_gpu = hasattr(feats, "is_cuda") and feats.is_cuda
    if on_gpu:
        mean_t, scatter, m4, counts = moments_device(feats)
        S, m4 = scatter.cpu().numpy(), float(m4.item())
        used, excluded = (int(c) for c in counts.tolist())
        dev = feats.device
    else:
        if hasattr(feats, "dtype") and hasattr(feats, "is_cuda") and feats.dtype != torch.float32:
            raise ValueError(f"feats must be float32, not {feats.dtype}")
        mean, S, m4, (used, excluded) = moments_np(feats)
        mean_t, dev = torch.from_numpy(mean), torch.device("cpu")
    D = S.shape[0]
    if used < 2:
        raise ValueError(f"a Gaussian needs at least 2 usable feature rows, not {used} ({excluded} hold a NaN or an infinity)")
    s = ledoit_wolf_np(S, m4, used) if isinstance(shrinkage, str) else float(shrinkage)
    cov = (1.0 - s) * (S / used)
    cov[np.diag_indices(D)] += s * (np.trace(S) / used / D)
    refusal = (f"the covariance of {used} rows in {D} dimensions is not positive definite at shrinkage {s:.6g}: "
               "use shrinkage='ledoit_wolf' or a larger number")
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(refusal) from None
    # a pivot at the rounding level of the largest variance is a zero that rounding made positive
    pivots = np.diag(L) ** 2
    if not np.isfinite(L).all() or pivots.min() <= D * 2.0 ** -52 * float(np.diag(cov).max()):
        raise ValueError(refusal)
    W = torch.linalg.solve_triangular(torch.from_numpy(L), torch.eye(D, dtype=torch.float64), upper=False)
    return FeatureGaussian(mean_t, cov, s, W.to(torch.float32).to(dev), used, excluded)


def mahalanobis(queries, gauss: FeatureGaussian):
    """The squared Mahalanobis distance of every row of `queries` [nq, D] (fp32) from `gauss`, fp32 [nq] on the device of the queries:
    GPU tensors through `eoe_mahalanobis_score`, CPU tensors and arrays through `mahalanobis_np`; NaN for a non-finite row."""
    import torch
    if hasattr(queries, "is_cuda") and queries.is_cuda:
        return mahalanobis_device(queries, gauss.mean.to(queries.device), gauss.W.to(queries.device),
                                  lower=gauss.lower and gauss.W.shape[0] == gauss.W.shape[1])[0]
    if hasattr(queries, "dtype") and hasattr(queries, "is_cuda") and queries.dtype != torch.float32:
        raise ValueError(f"queries must be float32, not {queries.dtype}")
    return torch.from_numpy(mahalanobis_np(_features(queries, "queries"), gauss.mean, gauss.W).astype(np.float32))


def mahalanobis_score(d2):
    """the Mahalanobis distance, the anomaly score of the Gaussian baseline: the square root of `mahalanobis`'s result"""
    return d2.sqrt()
