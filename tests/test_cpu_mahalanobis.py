"""CPU: the Gaussian baseline's entry points exist and refuse bad arguments before any launch, the scratch sizes grow with their
arguments, `moments_np`, `ledoit_wolf_np`, `fit_gaussian` and `mahalanobis` on CPU arrays against scikit-learn and on hand-worked
cases, and the refusals of the trainer's `mahalanobis_baseline` argument."""
import numpy as np
import pytest
import torch

import mahalanobis_util as mu

NEW_SYMBOLS = ("eoe_feature_moments", "eoe_feature_moments_scratch_bytes", "eoe_mahalanobis_score", "eoe_mahalanobis_score_scratch_bytes")
X, M, SC, M4, C, S, W, D2 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000      # non-null, 16-byte aligned, never read


def test_the_four_entry_points_are_exported_and_the_abi_version_stays():
    from eoe_amd import _lib
    assert _lib.lib.eoe_abi_version() == 5 and _lib.ABI_VERSION == 5
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(_lib.lib, name)
    assert mu.cover_is_complete()


def test_feature_moments_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_feature_moments, lib.eoe_last_error
    # eoe_feature_moments(x, ld, n, D, mean, scatter, m4, counts, scratch, stream)
    good = [X, 8, 10, 8, M, SC, M4, C, S, None]
    for i in (0, 4, 5, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert f(*args) == 1 and b"feature_moments" in err() and b"null" in err(), i
    for D in (0, 2049, -1):
        args = list(good)
        args[1] = args[3] = D
        assert f(*args) == 1 and b"D must be" in err(), D
    args = list(good)
    args[1] = 7
    assert f(*args) == 1 and b"ld must be" in err()
    for n in (-1, (1 << 30) + 1):
        args = list(good)
        args[2] = n
        assert f(*args) == 1 and b"n must be" in err(), n
    for i, off in ((0, 2), (4, 2), (5, 4), (6, 4), (7, 2), (8, 4), (8, 8)):
        args = list(good)
        args[i] += off
        assert f(*args) == 1 and b"aligned" in err(), (i, off)


def test_mahalanobis_score_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_mahalanobis_score, lib.eoe_last_error
    # eoe_mahalanobis_score(x, ldx, nq, D, mean, W, ldw, P, lower, d2, count, scratch, stream)
    good = [X, 8, 10, 8, M, W, 8, 8, 1, D2, C, S, None]
    for i in (0, 4, 5, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert f(*args) == 1 and b"mahalanobis_score" in err() and b"null" in err(), i
    for D in (0, 2049):
        args = list(good)
        args[1] = args[3] = args[6] = args[7] = D
        assert f(*args) == 1 and b"D must be" in err(), D
    for P in (0, 2049, -1):
        args = list(good)
        args[7], args[8] = P, 0
        assert f(*args) == 1 and b"P must be" in err(), P
    args = list(good)
    args[1] = 7
    assert f(*args) == 1 and b"ldx" in err()
    args = list(good)
    args[6] = 7
    assert f(*args) == 1 and b"ldw" in err()
    for P in (7, 9):
        args = list(good)
        args[7] = P
        assert f(*args) == 1 and b"lower" in err(), P
    args = list(good)
    args[2] = -1
    assert f(*args) == 1 and b"nq must be" in err()
    for i, off in ((0, 2), (4, 2), (5, 2), (9, 2), (10, 2), (11, 4), (11, 8)):
        args = list(good)
        args[i] += off
        assert f(*args) == 1 and b"aligned" in err(), (i, off)
    args = list(good)
    args[2] = 0                                                         # no query: nothing to launch
    assert f(*args) == 0


def test_the_scratch_sizes_are_positive_monotone_and_zero_outside_the_ranges():
    from eoe_amd._lib import lib
    mom, sco = lib.eoe_feature_moments_scratch_bytes, lib.eoe_mahalanobis_score_scratch_bytes
    assert mom(0, 1) > 0 and mom(2, 1) > 0 and sco(0, 1, 1) > 0 and sco(1, 1, 1) > 0
    for D in (1, 64, 512, 2048):
        sizes = [mom(n, D) for n in (0, 1, 2, 31, 33, 129, 1025, 2051, 5000, 45000, 131329, 1 << 20, 1 << 30)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0, (D, sizes)
    for n in (2, 1025, 45000):
        sizes = [mom(n, D) for D in (1, 64, 128, 129, 256, 512, 515, 1024, 2048)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (n, sizes)
    # the partial tiles do not grow with n: the flags, norms and column sums of the rows and at most 255 + 136 tiles of 64 KB
    for n in (45000, 1 << 20):
        assert mom(n, 2048) <= 391 * 65536 + n * 8 + 512 * 2048 * 8 + 4096
        assert mom(n, 512) <= 265 * 65536 + n * 8 + 512 * 512 * 8 + 4096
    base = (100, 512, 512)
    steps = {0: (1, 31, 130, 10000, 1 << 30), 1: (1, 64, 515, 2048), 2: (1, 3, 128, 129, 515, 2048)}
    for axis, values in steps.items():
        sizes = [sco(*[v if a == axis else base[a] for a in range(3)]) for v in values]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (axis, sizes)
        if axis != 1:                                                   # the width does not enter: y is never stored
            assert sizes[-1] > sizes[0], (axis, sizes)
    assert sco(10000, 512, 512) < 10000 * 512 * 4 // 50
    for bad in ((-1, 8), ((1 << 30) + 1, 8), (4, 0), (4, 2049)):
        assert mom(*bad) == 0, bad
    for bad in ((-1, 8, 8), ((1 << 30) + 1, 8, 8), (4, 0, 8), (4, 2049, 8), (4, 8, 0), (4, 8, 2049)):
        assert sco(*bad) == 0, bad


def _real_data(n=256, D=17, seed=0, grid=256.0):
    """Well-conditioned, correlated, off-centre real values.  With `grid` they lie on multiples of 1 / 256 and n is a power of two, so a
    column mean is a multiple of 2^-16 below 32 and x - mean has at most 21 significant bits: the fp32 mean and the fp32 centred values
    that the contract prescribes are then exact, and the comparison with scikit-learn, which centres in float64, shows no fp32 rounding
    (2^-24 per centred value otherwise: 1e-8 of the covariance, above the 1e-9 asked for here)."""
    rng = np.random.default_rng(seed)
    mix = np.eye(D) + 0.3 * rng.standard_normal((D, D))
    x = rng.standard_normal((n, D)) @ mix + rng.standard_normal(D) * 2
    if grid:
        assert n & (n - 1) == 0 and np.abs(x).max() < 31
        x = np.round(x * grid) / grid
    return x.astype(np.float32)


def test_the_numpy_statements_and_fit_gaussian_agree_with_scikit_learn():
    cov_mod = pytest.importorskip("sklearn.covariance")
    from eoe_amd import mahalanobis as mh
    x = _real_data()
    n, D = x.shape
    mean, S, m4, counts = mh.moments_np(x)
    assert mean.dtype == np.float32 and S.dtype == np.float64 and counts == (n, 0)
    x64 = x.astype(np.float64)
    assert np.array_equal(mean.astype(np.float64), x64.mean(0))        # the grid: the fp32 mean is the float64 mean
    want_cov, want_s = cov_mod.ledoit_wolf(x64)
    s = mh.ledoit_wolf_np(S, m4, n)
    assert s == pytest.approx(want_s, rel=1e-9) and 0 < s < 1
    for data in (x, torch.from_numpy(x)):
        g = mh.fit_gaussian(data)
        assert g.shrinkage == pytest.approx(want_s, rel=1e-9) and (g.n, g.nonfinite) == (n, 0)
        assert g.cov.dtype == np.float64 and g.W.dtype == torch.float32 and g.mean.dtype == torch.float32 and not g.W.is_cuda
        np.testing.assert_allclose(g.cov, want_cov, rtol=1e-9, atol=0)
        assert torch.equal(g.W, torch.tril(g.W))
    # the formula alone on values off any grid, fed with moments centred in float64 as scikit-learn centres them
    y = _real_data(200, 17, seed=2, grid=0).astype(np.float64)
    z = y - y.mean(0)
    assert mh.ledoit_wolf_np(z.T @ z, float(((z * z).sum(1) ** 2).sum()), 200) == pytest.approx(cov_mod.ledoit_wolf_shrinkage(y), rel=1e-9)
    fixed = mh.fit_gaussian(x, shrinkage=0.25)
    np.testing.assert_allclose(fixed.cov, cov_mod.shrunk_covariance(cov_mod.empirical_covariance(x64), 0.25), rtol=1e-9, atol=0)
    # distances: W is rounded to fp32 by design, so 1e-4 is that rounding (D 2^-24 cond), not a measured tolerance
    q = _real_data(50, D, seed=1, grid=0)
    emp = cov_mod.EmpiricalCovariance().fit(x64)
    plain = mh.fit_gaussian(x, shrinkage=0.0)
    np.testing.assert_allclose(plain.cov, emp.covariance_, rtol=1e-9, atol=0)
    d2 = mh.mahalanobis(q, plain)
    assert d2.dtype == torch.float32 and d2.shape == (50,)
    np.testing.assert_allclose(d2.numpy(), emp.mahalanobis(q.astype(np.float64)), rtol=1e-4)
    np.testing.assert_allclose(mh.mahalanobis_np(q, plain.mean, plain.W), emp.mahalanobis(q.astype(np.float64)), rtol=1e-4)
    assert torch.equal(mh.mahalanobis_score(d2), d2.sqrt())


def test_the_shrinkage_formula_on_a_case_worked_by_hand():
    from eoe_amd import mahalanobis as mh
    # rows (+-1, 0), (0, +-2): S = diag(2, 8), n = 4, |z|^2 = 1, 1, 4, 4, m4 = 34
    x = np.array([[1, 0], [-1, 0], [0, 2], [0, -2]], np.float32)
    mean, S, m4, counts = mh.moments_np(x + 5)
    assert mean.tolist() == [5, 5] and S.tolist() == [[2, 0], [0, 8]] and m4 == 34 and counts == (4, 0)
    # tr = 2.5, mu = 1.25, delta_ = 68 / 16 = 4.25, beta = (8.5 - 4.25) / 8 = 0.53125, delta = (4.25 - 6.25 + 3.125) / 2 = 0.5625
    assert mh.ledoit_wolf_np(S, m4, 4) == 0.53125 / 0.5625
    g = mh.fit_gaussian(x + 5)
    s = 0.53125 / 0.5625
    np.testing.assert_allclose(g.cov, [[(1 - s) * 0.5 + s * 1.25, 0], [0, (1 - s) * 2 + s * 1.25]], rtol=1e-15)


def test_hand_worked_cases():
    from eoe_amd import mahalanobis as mh
    # D = 1: the distance is (x - mean)^2 / variance; Ledoit-Wolf has nothing to shrink towards (delta = 0)
    x = np.array([[1], [3], [5], [7]], np.float32)
    g = mh.fit_gaussian(x)
    assert g.shrinkage == 0.0 and g.cov.tolist() == [[5.0]] and g.mean.tolist() == [4.0] and g.n == 4
    d2 = mh.mahalanobis(np.array([[4], [9], [-1]], np.float32), g)
    np.testing.assert_allclose(d2.numpy(), [0, 5, 5], rtol=1e-6)
    # identity covariance: the distance is the squared Euclidean distance from the mean
    x = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.float32) + np.array([10, 20], np.float32)
    g = mh.fit_gaussian(x, shrinkage=0.0)
    assert g.cov.tolist() == [[1, 0], [0, 1]] and g.W.tolist() == [[1, 0], [0, 1]] and g.mean.tolist() == [10, 20]
    assert mh.mahalanobis(np.array([[13, 24], [10, 20]], np.float32), g).tolist() == [25, 0]
    assert mh.mahalanobis_score(mh.mahalanobis(np.array([[13, 24]], np.float32), g)).tolist() == [5]
    # a non-finite row is excluded from the fit and counted, a non-finite query is NaN
    dirty = np.concatenate([x, [[np.nan, 0], [0, np.inf], [-np.inf, np.nan]]]).astype(np.float32)[[4, 0, 1, 5, 2, 3, 6]]
    g2 = mh.fit_gaussian(dirty, shrinkage=0.0)
    assert (g2.n, g2.nonfinite) == (4, 3) and g2.cov.tolist() == g.cov.tolist() and torch.equal(g2.mean, g.mean) and torch.equal(g2.W, g.W)
    m = mh.moments_np(dirty)
    assert m[3] == (4, 3) and m[1].tolist() == [[4, 0], [0, 4]] and m[2] == 16
    d2 = mh.mahalanobis(np.array([[11, 20], [np.nan, 20], [10, np.inf]], np.float32), g)
    assert d2[0] == 1 and torch.isnan(d2[1:]).all()
    assert np.isnan(mh.mahalanobis_np(np.array([[np.inf, 0]]), g.mean, g.W)).all()
    empty = mh.moments_np(np.full((3, 2), np.nan, np.float32))
    assert empty[0].tolist() == [0, 0] and empty[1].tolist() == [[0, 0], [0, 0]] and empty[2] == 0 and empty[3] == (0, 3)
    # fewer than 2 usable rows
    for few in (x[:1], dirty[[0, 1, 3]], x[:0]):
        with pytest.raises(ValueError, match="at least 2 usable feature rows"):
            mh.fit_gaussian(few)
    # a singular covariance (the second column repeats the first) is refused at shrinkage 0, naming it, and accepted at 0.1
    a = np.random.default_rng(3).standard_normal((20, 1)).astype(np.float32)
    sing = np.concatenate([a, a, np.random.default_rng(4).standard_normal((20, 1)).astype(np.float32)], 1)
    with pytest.raises(ValueError, match="not positive definite at shrinkage 0"):
        mh.fit_gaussian(sing, shrinkage=0.0)
    ok = mh.fit_gaussian(sing, shrinkage=0.1)
    assert ok.shrinkage == 0.1 and np.isfinite(mh.mahalanobis(sing, ok).numpy()).all()
    for bad in ("oas", -0.1, 1.5, True, None):
        with pytest.raises(ValueError, match="shrinkage must be"):
            mh.fit_gaussian(x, shrinkage=bad)
    with pytest.raises(ValueError, match="float32"):
        mh.fit_gaussian(torch.from_numpy(x).double())
    with pytest.raises(ValueError, match="do not fit"):
        mh.mahalanobis_np(x, g.mean, np.eye(3))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        mh.moments_device(torch.from_numpy(x))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        mh.mahalanobis_device(torch.from_numpy(x), g.mean, g.W)


def test_the_exact_inputs_are_exact_in_float64_too():
    """what the GPU tests compare against: integer-valued moments and distances"""
    from eoe_amd import mahalanobis as mh
    for n, D in ((2, 1), (129, 65), (1025, 256)):
        x = mu.paired_features(n, D, 7)
        mean, S, m4, counts = mh.moments_np(x)
        assert (mean == 3).all() and counts == (n, 0) and (S == np.round(S)).all() and np.abs(S).max() < 2 ** 24 and m4 == round(m4) < 2 ** 53
        z = x.astype(np.int64) - 3
        assert np.array_equal(S, (z.T @ z).astype(np.float64)) and m4 == float(((z * z).sum(1) ** 2).sum())
    x, mean, W = mu.exact_score_inputs(130, 515, 515, 5)
    d2 = mh.mahalanobis_np(x, mean, W)
    y = (x.astype(np.int64) - mean.astype(np.int64)) @ W.astype(np.int64).T
    assert np.array_equal(d2, ((y * y).sum(1)).astype(np.float64)) and d2.max() < 2 ** 24


def test_the_trainer_checks_the_shrinkage_and_refuses_a_source_without_normal_inputs():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    kw = dict(dataset=None, epochs=1, batch_size=4, classes=["a"], device="cpu")
    for bad in ("oas", 2.0, -1, True):
        with pytest.raises(ValueError, match="shrinkage must be"):
            TRAINER["hsc"](CNN32(), mahalanobis_baseline=True, mahalanobis_shrinkage=bad, **kw)
    on = TRAINER["hsc"](CNN32(), mahalanobis_baseline=True, mahalanobis_shrinkage=0.5, **kw)    # needs neither extremes nor neighbors
    off = TRAINER["hsc"](CNN32(), **kw)
    assert (on.with_mahalanobis, on.mahalanobis_shrinkage, off.with_mahalanobis, off.mahalanobis_shrinkage) == (True, 0.5, False, "ledoit_wolf")
    assert on.mahalanobis_results == {} and off.mahalanobis_results == {} and on.n_neighbors == 0 and on.n_extremes == 0

    class NoNormals:
        nominal_label = 0

        def test_inputs(self, rows):
            raise AssertionError

        def loaders(self, *a, **k):
            raise AssertionError("no loader may be asked for")
    with pytest.raises(NotImplementedError, match=r"mahalanobis_baseline=True needs a source with normal_inputs\(rows\); NoNormals has none"):
        on.eval_cls(CNN32(), NoNormals(), 0, "a", 0)
