"""GPU tier: `eoe_feature_moments` and `eoe_mahalanobis_score` (csrc/mahalanobis.hip) -- mean, scatter matrix, fourth moment and distances
against the float64 NumPy statements (`mahalanobis.moments_np`, `mahalanobis_np`) bit for bit on integer-valued inputs at every tile,
k-step and slice edge (tests/mahalanobis_util.py), first-order rounding bounds on real-valued ones, strided and unaligned inputs,
non-finite rows, repeatability under a dirty scratch, `fit_gaussian` / `mahalanobis` on both routes, and the trainer's
`mahalanobis_baseline=True` on the small CNN32 task of test_gpu_knn."""
import json
import os

import numpy as np
import pytest
import torch

import mahalanobis_util as mu
from eoe_amd import mahalanobis as mh
from eoe_amd import metrics, neighbors

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 64


def place(x, D, pad=0, shift=0):
    """x on the device with rows `D + pad` apart, the padding NaN, starting `shift` floats past a 16-byte boundary"""
    n, ld = x.shape[0], D + pad
    buf = torch.full((n * ld + 4 + shift,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + n * ld].view(n, ld)
    view[:, :D] = torch.from_numpy(x).cuda()
    return buf, view, ld


def guarded(n, dtype):
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")


def unguard(name, t, n):
    a = t.cpu().numpy()
    assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + n:] == SENTINEL).all(), f"{name}: written outside its {n} entries"
    return a[GUARD:GUARD + n]


def raw_moments(x, fill=0xA5, pad=0, shift=0):
    """one `eoe_feature_moments` call.  The outputs sit between guard words pre-filled with SENTINEL, the scratch is pre-filled with the
    byte `fill`.  Returns (mean fp32 [D], scatter f64 [D, D], m4, counts) on the host."""
    from eoe_amd._lib import check, lib
    n, D = x.shape
    keep, xv, ld = place(x, D, pad, shift)
    mean, scatter, m4, counts = guarded(D, torch.float32), guarded(D * D, torch.float64), guarded(1, torch.float64), guarded(2, torch.int32)
    scratch = torch.full((lib.eoe_feature_moments_scratch_bytes(n, D),), fill, dtype=torch.uint8, device="cuda")
    check(lib.eoe_feature_moments(xv.data_ptr(), ld, n, D, mean[GUARD:].data_ptr(), scatter[GUARD:].data_ptr(), m4[GUARD:].data_ptr(),
                                  counts[GUARD:].data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "eoe_feature_moments")
    return (unguard("mean", mean, D), unguard("scatter", scatter, D * D).reshape(D, D), float(unguard("m4", m4, 1)[0]),
            unguard("counts", counts, 2).tolist())


def raw_score(x, mean, W, lower=0, fill=0xA5, pad=0, shift=0):
    """one `eoe_mahalanobis_score` call, guarded like `raw_moments`; pad and shift apply to x, W and (shift) the mean.
    Returns (d2 fp32 [nq], count) on the host."""
    from eoe_amd._lib import check, lib
    (nq, D), P = x.shape, W.shape[0]
    kx, xv, ldx = place(x, D, pad, shift)
    kw, wv, ldw = place(W, D, pad, shift)
    km, mv, _ = place(mean.reshape(1, D), D, 0, shift)
    d2, count = guarded(nq, torch.float32), guarded(1, torch.int32)
    scratch = torch.full((lib.eoe_mahalanobis_score_scratch_bytes(nq, D, P),), fill, dtype=torch.uint8, device="cuda")
    check(lib.eoe_mahalanobis_score(xv.data_ptr(), ldx, nq, D, mv.data_ptr(), wv.data_ptr(), ldw, P, lower, d2[GUARD:].data_ptr(),
                                    count[GUARD:].data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "eoe_mahalanobis_score")
    return unguard("d2", d2, nq), int(unguard("count", count, 1)[0])


def same_fit(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes() \
        and a[3] == b[3]


def test_the_covering_tables_hold_every_edge_value():
    assert mu.cover_is_complete()


@pytest.mark.parametrize("n,D", mu.FIT_COVER)
def test_paired_integer_features_give_numpys_moments_bit_for_bit(n, D):
    x = mu.paired_features(n, D, 100 + n % 1000 + D)
    mean, scatter, m4, counts = raw_moments(x)
    mu.check_exact_fit(mean, scatter, m4, counts, x, f"{n}x{D}")


@pytest.mark.parametrize("nq,D,P", mu.SCORE_COVER)
def test_integer_inputs_give_numpys_distances_bit_for_bit_and_lower_changes_no_byte(nq, D, P):
    P = D if P == "D" else P
    x, mean, W = mu.exact_score_inputs(nq, D, P, 200 + nq + D + P)
    d2, count = raw_score(x, mean, W)
    assert count == 0
    mu.check_exact_score(d2, x, mean, W, f"{nq}x{D}x{P}")
    if P == D:
        low = raw_score(x, mean, W, lower=1)
        assert low[0].tobytes() == d2.tobytes() and low[1] == 0


@pytest.mark.parametrize("n,D", [(33, 65), (1025, 256), (130, 515), (2, 3)])
def test_strided_and_unaligned_features_give_the_fit_of_contiguous_ones(n, D):
    x = mu.paired_features(n, D, 11)
    base = raw_moments(x)
    mu.check_exact_fit(*base, x, "contiguous")
    real = mu.real_features(n, D, 12, offset=1.0)
    real_base = raw_moments(real)
    for pad, shift in ((4 - D % 4 if D % 4 else 4, 0), (1, 0), (0, 1), (3, 1)):
        assert same_fit(raw_moments(x, pad=pad, shift=shift), base), (pad, shift)
        assert same_fit(raw_moments(real, pad=pad, shift=shift), real_base), (pad, shift)


@pytest.mark.parametrize("nq,D,P", [(33, 65, 65), (130, 256, 3), (31, 515, 515), (1, 3, 1)])
def test_strided_and_unaligned_queries_and_factors_give_the_distances_of_contiguous_ones(nq, D, P):
    x, mean, W = mu.exact_score_inputs(nq, D, P, 13)
    base = raw_score(x, mean, W)
    mu.check_exact_score(base[0], x, mean, W, "contiguous")
    xr, mr, Wr = mu.real_score_inputs(nq, D, P, 14)
    real_base = raw_score(xr, mr, Wr)
    for pad, shift in ((4 - D % 4 if D % 4 else 4, 0), (1, 0), (0, 1), (3, 1)):
        got = raw_score(x, mean, W, pad=pad, shift=shift)
        assert got[0].tobytes() == base[0].tobytes() and got[1] == base[1], (pad, shift)
        assert raw_score(xr, mr, Wr, pad=pad, shift=shift)[0].tobytes() == real_base[0].tobytes(), (pad, shift)


@pytest.mark.parametrize("n,D", mu.REAL_FITS)
def test_real_features_keep_every_moment_within_its_rounding_bound(n, D):
    cases = [(m, 0.0) for m in mu.MAGNITUDES] + [(1.0, 100.0)]                        # the last: a common offset, the cancellation case
    for mag, off in cases:
        x = mu.real_features(n, D, 21, mag, off)
        worst = mu.check_real_fit(*raw_moments(x), x, f"{n}x{D} magnitude {mag} offset {off}")
        print(f"moments real {n}x{D} mag={mag} off={off}: worst scatter |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("nq,D,P", mu.REAL_SCORES)
def test_real_queries_stay_within_the_rounding_bound_for_every_row(nq, D, P):
    cases = [(m, 0.0) for m in mu.MAGNITUDES] + [(1.0, 100.0)]
    for mag, off in cases:
        x, mean, W = mu.real_score_inputs(nq, D, P, 22, mag, off)
        d2, count = raw_score(x, mean, W)
        assert count == 0
        worst = mu.check_real_score(d2, x, mean, W, f"{nq}x{D}x{P} magnitude {mag} offset {off}")
        print(f"score real {nq}x{D}x{P} mag={mag} off={off}: worst |err| / bound = {worst:.4f}")
        if P == D:
            assert raw_score(x, mean, W, lower=1)[0].tobytes() == d2.tobytes()


def test_non_finite_rows_are_left_out_of_the_fit_and_counted():
    n, D = 1025, 129
    for make in (lambda: mu.paired_features(n, D, 31), lambda: mu.real_features(n, D, 32, offset=2.0)):
        x = make()
        bad = {0: (0, np.nan), 31: (128, np.inf), 32: (64, -np.inf), 255: (127, np.nan), 256: (1, np.inf), n + 5: (3, np.nan)}
        dirty = np.insert(x, [0, 30, 30, 252, 252, n], 0.0, axis=0)                   # six more rows, at the positions of `bad`
        assert dirty.shape[0] == n + 6
        for row, (col, v) in bad.items():
            assert (dirty[row] == 0).all()
            dirty[row] = x[row % n]                                                   # finite values around the bad one
            dirty[row, col] = v
        assert np.array_equal(dirty[np.isfinite(dirty).all(1)], x)
        got, alone = raw_moments(dirty), raw_moments(x)
        assert got[3] == [n, 6] and alone[3] == [n, 0]
        # An excluded row adds +0 to every sum, so the fit is that of the remaining rows in their order; the slices are cut by
        # position, though, and here they cut the remaining rows differently from the fit of those rows alone: integer features,
        # exact under any cut, compare bit for bit, real ones within the bounds (and bit for bit below, where the cuts agree).
        if (x == np.round(x)).all():
            assert got[0].tobytes() == alone[0].tobytes() and got[1].tobytes() == alone[1].tobytes() and got[2] == alone[2]
            mu.check_exact_fit(got[0], got[1], got[2], (n, 6), dirty, "dirty")
        else:
            mu.check_real_fit(*got, dirty, "dirty")
    # real features whose slices agree (two of 32 rows either way; the bad rows make a third slice that adds nothing): the same bytes
    # as the fit of those rows alone
    x = mu.real_features(64, 65, 33)
    tail = np.concatenate([x, np.full((3, 65), np.nan, np.float32)])
    got, alone = raw_moments(tail), raw_moments(x)
    assert got[3] == [64, 3] and alone[3] == [64, 0] and same_fit(got[:3] + ([0, 0],), alone[:3] + ([0, 0],))
    mu.check_real_fit(*got, tail, "tail")
    # real features, bad rows in the middle, one slice of everything in both runs (31 and 26 rows: one k-step, one column-sum slice):
    # every chain sees the same rows in the same order with +0 terms between them, over all three tiles of D = 256.  A bad row holds
    # large finite values next to its NaN or infinity, in both operands' columns: a row zeroed in one operand only would show.
    # m4 is held to its bound: its float64 tree pairs the rows' norms by position.
    x = mu.real_features(26, 256, 35, offset=1.0)
    mid = np.insert(x, [0, 5, 5, 13, 26], 1e3, axis=0)
    for row, col, v in ((0, 255, np.nan), (6, 0, np.inf), (7, 128, -np.inf), (16, 127, np.nan), (30, 200, np.inf)):
        assert (mid[row] == 1e3).all()
        mid[row, col] = v
    assert np.array_equal(mid[np.isfinite(mid).all(1)], x)
    got, alone = raw_moments(mid), raw_moments(x)
    assert got[3] == [26, 5] and alone[3] == [26, 0]
    assert got[0].tobytes() == alone[0].tobytes() and got[1].tobytes() == alone[1].tobytes()
    mu.check_real_fit(*got, mid, "middle")
    # no row usable: zeros
    mean, scatter, m4, counts = raw_moments(np.full((5, 3), np.inf, np.float32))
    assert counts == [0, 5] and not mean.any() and not scatter.any() and m4 == 0.0


def test_non_finite_queries_give_nan_and_are_counted():
    nq, D = 130, 129
    x, mean, W = mu.exact_score_inputs(nq, D, D, 34)
    clean = raw_score(x, mean, W)[0]
    for row, col, v in ((0, 0, np.nan), (31, 128, np.inf), (127, 64, -np.inf), (128, 3, np.nan)):
        x[row, col] = v
    for lower in (0, 1):
        d2, count = raw_score(x, mean, W, lower=lower)
        assert count == 4 and np.isnan(d2[[0, 31, 127, 128]]).all()
        rest = np.setdiff1d(np.arange(nq), [0, 31, 127, 128])
        assert d2[rest].tobytes() == clean[rest].tobytes()
        np.testing.assert_array_equal(d2.astype(np.float64), mh.mahalanobis_np(x, mean, W))          # NaN rows compare equal here


def test_runs_over_different_scratch_fills_give_the_same_bytes():
    x = mu.real_features(2051, 130, 41, offset=1.0)
    runs = [raw_moments(x, fill) for fill in (0x00, 0x00, 0xFF, 0x5A)]
    assert all(same_fit(r, runs[0]) for r in runs[1:])
    q, mean, W = mu.real_score_inputs(1025, 130, 130, 42)
    scores = [raw_score(q, mean, W, fill=fill) for fill in (0x00, 0x00, 0xFF, 0x5A)]
    assert all(s[0].tobytes() == scores[0][0].tobytes() and s[1] == 0 for s in scores[1:])


def test_fit_gaussian_and_mahalanobis_on_device_tensors_agree_with_the_cpu_route():
    from eoe_amd._lib import lib
    n, D = 1025, 65
    rng = np.random.default_rng(51)
    mix = np.eye(D) + 0.2 * rng.standard_normal((D, D))
    x = (rng.standard_normal((n, D)) @ mix + 1.0).astype(np.float32)
    x[7, 3] = np.nan
    q = (rng.standard_normal((130, D)) @ mix + 1.0).astype(np.float32)
    q[5, 0] = np.inf
    xt, qt = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    keep = np.arange(130) != 5
    # the device wrapper is the raw route
    raw = raw_moments(x)
    mean, scatter, m4, counts = mh.moments_device(xt)
    assert mean.is_cuda and scatter.dtype == torch.float64 and counts.tolist() == [n - 1, 1]
    assert same_fit((mean.cpu().numpy(), scatter.cpu().numpy(), float(m4.item()), counts.tolist()), raw)
    need = lib.eoe_feature_moments_scratch_bytes(n, D)
    own = torch.full((need + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    again = mh.moments_device(xt, scratch=own)
    assert torch.equal(again[1], scatter) and torch.equal(again[0], mean)
    with pytest.raises(ValueError, match="scratch"):
        mh.moments_device(xt, scratch=own[:need - 16])
    with pytest.raises(RuntimeError, match="GPU tensors"):
        mh.moments_device(xt.cpu())
    mu.check_real_fit(*raw, x, "route")
    # Both fits, within the bounds that `route_bounds` carries from the moments to the shrinkage.  With s' = s + (at most) ds and
    # S' = S + (at most) E:  cov' - cov = (1 - s) (S' - S) / n + (s - s') S' / n + (s (mu' - mu) + (s' - s) mu') I, so
    # |cov' - cov| <= (1 - s) E / n + ds (|S| + E) / n + (s e_mu + ds (mu + e_mu)) I; ds = 0 under a fixed shrinkage.  1 % on top for the
    # terms of second order (the two routes' means may differ in a last bit).
    E, e_mu, ds_lw, S_cpu, mu_cpu, s_lw = mu.route_bounds(x)
    used = n - 1
    for shrinkage in ("ledoit_wolf", 0.0, 0.3):
        dev, cpu = mh.fit_gaussian(xt, shrinkage=shrinkage), mh.fit_gaussian(x, shrinkage=shrinkage)
        assert dev.W.is_cuda and dev.mean.is_cuda and not cpu.W.is_cuda and (dev.n, dev.nonfinite) == (cpu.n, cpu.nonfinite) == (used, 1)
        assert dev.cov.dtype == np.float64 and dev.W.dtype == torch.float32 and torch.equal(dev.W, torch.tril(dev.W))
        if isinstance(shrinkage, str):
            assert cpu.shrinkage == pytest.approx(s_lw, rel=1e-12) and 0 < cpu.shrinkage < 1
            print(f"ledoit-wolf shrinkage: device {dev.shrinkage!r}, host {cpu.shrinkage!r}, bound of the difference {ds_lw:.3e}")
            assert abs(dev.shrinkage - cpu.shrinkage) <= 1.01 * ds_lw < 0.1 * cpu.shrinkage
            ds = ds_lw
        else:
            assert dev.shrinkage == cpu.shrinkage == shrinkage
            ds = 0.0
        s = cpu.shrinkage
        lim = 1.01 * ((1 - s) * E / used + ds * (np.abs(S_cpu) + E) / used + np.eye(D) * (s * e_mu + ds * (mu_cpu + e_mu)))
        diff = np.abs(dev.cov - cpu.cov)
        print(f"shrinkage {shrinkage}: worst |cov difference| / bound = {(diff / lim).max():.4f}")
        assert (diff <= lim).all()
        d_dev, d_cpu = mh.mahalanobis(qt, dev), mh.mahalanobis(q, cpu)
        assert d_dev.is_cuda and d_dev.dtype == torch.float32 and not d_cpu.is_cuda and d_dev.shape == (130,)
        assert torch.isnan(d_dev[5]) and torch.isnan(d_cpu[5])
        # the kernel on the device fit's own mean and W: within the distance bound of float64 on the same values
        mu.check_real_score(d_dev.cpu().numpy(), q, dev.mean.cpu().numpy(), dev.W.cpu().numpy(), f"route shrinkage {shrinkage}")
        # the two routes on ONE Gaussian, the CPU fit's: the kernel within the distance bound of the float64 statement, which the CPU
        # route rounds once to fp32 (2^-24 of the distance more between the two)
        d_x = mh.mahalanobis(qt, cpu)
        assert d_x.is_cuda
        d_x = d_x.cpu().numpy()
        worst = mu.check_real_score(d_x, q, cpu.mean.numpy(), cpu.W.numpy(), f"one Gaussian, shrinkage {shrinkage}")
        want, bound, ok = mu.score_bound(q, cpu.mean.numpy(), cpu.W.numpy())
        assert np.array_equal(d_cpu.numpy()[ok], want.astype(np.float32)) and np.array_equal(ok, keep)
        assert (np.abs(d_x[ok].astype(np.float64) - d_cpu.numpy()[ok].astype(np.float64)) <= bound + mu.U * want).all()
        print(f"shrinkage {shrinkage}: kernel against the CPU route on the CPU fit, worst |err| / bound = {worst:.4f}")
        assert torch.equal(mh.mahalanobis_score(d_dev)[keep], d_dev.sqrt()[keep])
    # strided rows, no queries, hand-made directions
    strided = torch.full((130, 72), float("nan"), device="cuda")
    strided[:, :D] = qt
    dev = mh.fit_gaussian(xt)
    assert torch.equal(mh.mahalanobis(strided[:, :D], dev)[keep], mh.mahalanobis(qt, dev)[keep])
    assert tuple(mh.mahalanobis(qt[:0], dev).shape) == (0,)
    top = mh.FeatureGaussian(dev.mean, dev.cov, dev.shrinkage, dev.W[-3:].contiguous(), dev.n, dev.nonfinite, lower=False)
    d3 = mh.mahalanobis(qt, top).cpu().numpy()
    mu.check_real_score(d3, q, dev.mean.cpu().numpy(), dev.W[-3:].cpu().numpy(), "three directions")
    with pytest.raises(ValueError, match="at least 2 usable"):
        mh.fit_gaussian(xt[7:8])
    with pytest.raises(ValueError, match="lower"):
        mh.mahalanobis_device(qt, dev.mean, dev.W[:3], lower=True)


# ------------------------------------------------------------------------------------------------ trainer
def test_trainer_scores_the_mahalanobis_baseline_and_leaves_everything_else_alone(tmp_path):
    import copy
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    from test_gpu_knn import KW, _model, _task
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    ds = _task()
    torch.manual_seed(1)
    model, _ = TRAINER["hsc"](_model(), dataset=ds, **KW).train_cls(_model(), ds, 0, "a", 0)

    def trainer(name, **extra):
        return TRAINER["hsc"](_model(), dataset=ds, logger=JsonLogger(str(tmp_path / name)), **extra, **KW)
    # 12 normal images in 256 dimensions: the covariance needs its shrinkage
    on, off = trainer("on", mahalanobis_baseline=True), trainer("off")
    res_on, res_off = on.eval_cls(copy.deepcopy(model), ds, 0, "a", 0), off.eval_cls(copy.deepcopy(model), ds, 0, "a", 0)
    assert list(on.mahalanobis_results) == [0] and off.mahalanobis_results == {} and on.neighbors == {} and on.knn_results == {}
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off")}
    assert sorted(set(files["on"]) - set(files["off"])) == ["eval_cls0_it0_mahalanobis.json"] and set(files["off"]) <= set(files["on"])
    res = on.mahalanobis_results[0]
    assert res == json.load(open(tmp_path / "on" / "eval_cls0_it0_mahalanobis.json"))
    assert sorted(res) == ["D", "auc", "avg_prec", "n_normal", "nonfinite", "shrinkage"]
    assert (res["n_normal"], res["D"], res["nonfinite"]) == (12, 256, 0) and 0 < res["shrinkage"] <= 1
    # the same baseline from features embedded here, scored by the float64 statement
    m = copy.deepcopy(model).cuda().eval()
    on._normalize_hook(m, ds)
    refs = neighbors.embed(m, [(ds.normal_inputs(torch.arange(12))[0],)], trainer=on)
    test_feats = neighbors.embed(m, [ds.test_inputs(torch.arange(lo, min(lo + 16, 24)))[:2] for lo in (0, 16)], trainer=on)
    gauss = mh.fit_gaussian(refs)
    assert gauss.shrinkage == res["shrinkage"]
    score = np.sqrt(mh.mahalanobis_np(test_feats, gauss.mean, gauss.W))
    assert abs(res["auc"] - metrics.roc_auc(ds.test_y.cpu().numpy(), score)) <= 1e-6
    assert abs(res["avg_prec"] - metrics.average_precision(ds.test_y.cpu().numpy(), score)) <= 1e-6
    # nothing else moved
    for f in files["off"]:
        if os.path.isfile(tmp_path / "off" / f):
            text_on, text_off = (tmp_path / "on" / f).read_bytes(), (tmp_path / "off" / f).read_bytes()
            if text_on != text_off:                                                   # the text log: one more line, the baseline's
                extra = [ln for ln in text_on.splitlines() if ln not in text_off.splitlines()]
                assert len(extra) == 1 and b"Mahalanobis baseline" in extra[0], f
    assert (res_on[0].auc, res_on[1].avg_prec) == (res_off[0].auc, res_off[1].avg_prec)
    # with neighbors=k on as well: the same neighbours and k-NN results as without the new option
    both = trainer("both", extremes=3, neighbors=4, knn_baseline=True, mahalanobis_baseline=True, mahalanobis_shrinkage=0.5)
    knn = trainer("knn", extremes=3, neighbors=4, knn_baseline=True)
    both.eval_cls(copy.deepcopy(model), ds, 0, "a", 0)
    knn.eval_cls(copy.deepcopy(model), ds, 0, "a", 0)
    key = "eval_cls0_it0"
    assert torch.equal(both.neighbors[key].idx, knn.neighbors[key].idx) and torch.equal(both.neighbors[key].d2, knn.neighbors[key].d2)
    assert both.knn_results == knn.knn_results and knn.mahalanobis_results == {} and both.mahalanobis_results[0]["shrinkage"] == 0.5
    assert sorted(set(os.listdir(tmp_path / "both")) - set(os.listdir(tmp_path / "knn"))) == ["eval_cls0_it0_mahalanobis.json"]
    # a classifier head is refused before scoring
    from eoe_amd.models import CNN32
    asked = []
    with pytest.raises(NotImplementedError, match="mahalanobis_baseline=True .* a classifier head has no embedding"):
        clf = TRAINER["hsc"](CNN32(clf=True), dataset=ds, mahalanobis_baseline=True, **KW)
        clf.compute_anomaly_score = lambda *a, **k: asked.append(1)
        clf.eval_cls(CNN32(clf=True), ds, 0, "a", 0)
    assert not asked

    # so are features wider than the kernels take (3 x 32 x 32 = 3072 > 2048), before scoring as well
    class Wide(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward(self, x):
            return (x.float() * self.w).reshape(x.shape[0], -1)
    with pytest.raises(NotImplementedError, match="at most 2048 dimensions; the model's features have 3072"):
        wide = TRAINER["hsc"](Wide(), dataset=ds, mahalanobis_baseline=True, **KW)
        wide.compute_anomaly_score = lambda *a, **k: asked.append(1)
        wide.eval_cls(Wide(), ds, 0, "a", 0)
    assert not asked
    eoe_amd.set_compute_dtype(old)


def test_a_run_with_the_option_off_leaves_the_files_it_leaves_today(tmp_path):
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    from test_gpu_knn import KW, _model, _task
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")

    def run(name, **extra):
        torch.manual_seed(2)
        np.random.seed(2)
        tr = TRAINER["hsc"](_model(), dataset=_task(), logger=JsonLogger(str(tmp_path / name)), **extra, **KW)
        out = tr.run(run_seeds=1)[1]
        return tr, out, sorted(os.path.relpath(os.path.join(d, f), tmp_path / name) for d, _, fs in os.walk(tmp_path / name) for f in fs)
    (tr_a, res_a, files_a), (tr_b, res_b, files_b) = run("without"), run("defaults", mahalanobis_baseline=False, mahalanobis_shrinkage="ledoit_wolf")
    assert tr_a.mahalanobis_results == {} and tr_b.mahalanobis_results == {}
    assert files_a == files_b and "results.json" in files_a and not any("mahalanobis" in f for f in files_a)
    assert (tmp_path / "without" / "results.json").read_bytes() == (tmp_path / "defaults" / "results.json").read_bytes()
    assert res_a == res_b
    # with the option on, `run` fills one entry per class and starts the next run empty
    tr_c, res_c, files_c = run("with", mahalanobis_baseline=True)
    assert list(tr_c.mahalanobis_results) == [0] and res_c["cls_aucs"] == res_a["cls_aucs"]
    assert [f for f in files_c if f not in files_a] == ["eval_cls0_it0_mahalanobis.json"]
    tr_c.mahalanobis_results["stale"] = None
    torch.manual_seed(2)
    tr_c.run(run_seeds=1)
    assert list(tr_c.mahalanobis_results) == [0]
    eoe_amd.set_compute_dtype(old)
