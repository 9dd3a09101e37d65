"""CPU tier: the ROC and precision-recall curves of `eoe_amd.metrics` on host arrays against the fixture g23 (sklearn's own
`roc_curve` / `precision_recall_curve` on stored inputs, tests/golden/make_golden_curves.py), `mean_plot` against the reference's
own, the containers, and the argument checks.  The counts are integers and each rate is one IEEE division of the same two
integers, so the comparisons are exact."""
import numpy as np
import pytest

from eoe_amd import metrics

CASES = ("n2", "n3_tie", "n255", "n256", "n257", "n513_equal", "n1000_quarters", "n1023", "n1024", "n1025", "n600_separated", "n300_zeros")
MEAN_CASES = ("n255", "n1000_quarters", "n1025")
trapz = getattr(np, "trapezoid", None) or np.trapz


def same(got, want, what):
    """equal shapes, equal values in float64 and, for thresholds, equal bits (`-0.0 == 0.0` would pass a value comparison)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), what
    if want.dtype == np.float32:
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


@pytest.mark.parametrize("case", CASES)
def test_host_curves_equal_sklearn(golden, case):
    g = golden("g23_curves")
    y, s = g[f"{case}/y"], g[f"{case}/s"]
    for prefix, got in (("roc", metrics.roc_curve(y, s)), ("rocfull", metrics.roc_curve(y, s, drop_intermediate=False))):
        for name, arr in zip(("fpr", "tpr", "thr"), got):
            same(arr, g[f"{case}/{prefix}_{name}"], f"{case} {prefix} {name}")
    for name, arr in zip(("prec", "rec", "thr"), metrics.precision_recall_curve(y, s)):
        same(arr, g[f"{case}/prc_{name}"], f"{case} prc {name}")
    fpr, tpr, thr = metrics.roc_curve(y, s)
    assert thr.size - 1 == int(g[f"{case}/K_roc"]) and np.isinf(thr[0])
    # the area under the curve is the rank statistic the trainer reports, the step sum its average precision
    assert abs(trapz(tpr, fpr) - metrics.roc_auc(y, s)) < 1e-12
    assert abs(trapz(tpr, fpr) - float(g[f"{case}/auc"])) < 1e-12
    prec, rec, _ = metrics.precision_recall_curve(y, s)
    assert abs(-np.sum(np.diff(rec) * prec[:-1]) - metrics.average_precision(y, s)) < 1e-12


def test_host_curves_take_tensors_lists_and_float64(golden):
    import torch
    g = golden("g23_curves")
    y, s = g["n257/y"], g["n257/s"]
    want = metrics.roc_curve(y, s)
    for yy, ss in ((torch.from_numpy(y), torch.from_numpy(s)), (y.tolist(), s)):
        for a, b in zip(metrics.roc_curve(yy, ss), want):
            same(a, b, "roc from a tensor / list")
    fpr, tpr, thr = metrics.roc_curve(y, s.astype(np.float64))
    assert thr.dtype == np.float64 and np.array_equal(thr, want[2].astype(np.float64)) and np.array_equal(fpr, want[0])


def _containers(g, cases):
    rocs = [metrics.ROC(float(g[f"{c}/auc"]), tpr=g[f"{c}/roc_tpr"], fpr=g[f"{c}/roc_fpr"], ths=g[f"{c}/roc_thr"]) for c in cases]
    prcs = [metrics.PRC(float(g[f"{c}/ap"]), prec=g[f"{c}/prc_prec"], rec=g[f"{c}/prc_rec"], ths=g[f"{c}/prc_thr"]) for c in cases]
    return rocs, prcs


def test_mean_plot_equals_reference_and_leaves_its_random_state(golden):
    g = golden("g23_curves")
    rocs, prcs = _containers(g, MEAN_CASES)
    before = np.random.get_state()
    try:
        np.random.seed(7)
        m_roc = metrics.mean_plot(rocs)
        m_prc = metrics.mean_plot(prcs)
        state = np.random.get_state()
    finally:
        np.random.set_state(before)
    assert isinstance(m_roc, metrics.ROC) and isinstance(m_prc, metrics.PRC)
    for got, key in ((m_roc.tpr, "roc_tpr"), (m_roc.fpr, "roc_fpr"), (m_roc.ths, "roc_ths"), (m_prc.prec, "prc_prec"),
                     (m_prc.rec, "prc_rec"), (m_prc.ths, "prc_ths")):
        want = g[f"mean/{key}"]
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), key
    assert m_roc.auc == float(g["mean/roc_auc"]) and m_roc.std == float(g["mean/roc_std"]) and m_roc.n == int(g["mean/roc_n"]) == 3
    assert m_prc.avg_prec == float(g["mean/prc_avg_prec"]) and m_prc.std == float(g["mean/prc_std"]) and m_prc.n == 3
    assert m_roc.get_score() == m_roc.auc and m_roc.get_x() is m_roc.fpr and m_roc.get_y() is m_roc.tpr
    assert state[0] == "MT19937" and np.array_equal(state[1], g["mean/state_keys"]) and state[2] == int(g["mean/state_pos"])
    # the inputs are left alone, and nothing to average is None
    assert len(rocs[2].ths) == g["n1025/roc_thr"].size
    assert metrics.mean_plot([]) is None and metrics.mean_plot(None) is None and metrics.mean_plot([rocs[0], None]) is None


def test_containers_keep_their_positional_form_and_gain_the_curve():
    r = metrics.ROC(0.75, 0.1, 3)
    assert (r.auc, r.std, r.n, r.get_score()) == (0.75, 0.1, 3, 0.75) and r.tpr is None and r.fpr is None and r.ths is None
    r = metrics.ROC(0.5)
    assert r.std is None and r.n == -1 and r.get_x() is None and r.get_y() is None
    p = metrics.PRC(0.25, 0.2, 4)
    assert (p.avg_prec, p.std, p.n, p.get_score()) == (0.25, 0.2, 4, 0.25) and p.prec is None and p.rec is None and p.ths is None
    tpr, fpr, ths = [0.0, 1.0], [0.0, 0.5], [np.inf, 0.3]
    r = metrics.ROC(0.9, tpr=tpr, fpr=fpr, ths=ths)
    assert r.get_x() is fpr and r.get_y() is tpr and r.ths is ths and r.get_score() == 0.9
    p = metrics.PRC(0.8, prec=tpr, rec=fpr, ths=ths)
    assert p.get_x() is fpr and p.get_y() is tpr and p.ths is ths and p.get_score() == 0.8
    with pytest.raises(TypeError):
        metrics.ROC(0.9, None, -1, tpr)                 # the curve fields are keyword-only: a fourth positional argument is an error


def test_curves_reject_nonfinite_scores_and_single_class_inputs():
    y = np.array([0, 1, 1, 0])
    for bad in (np.nan, np.inf, -np.inf):
        s = np.array([0.1, bad, 0.3, 0.2], np.float32)
        with pytest.raises(ValueError):
            metrics.roc_curve(y, s)
        with pytest.raises(ValueError):
            metrics.precision_recall_curve(y, s)
    s = np.array([0.1, 0.4, 0.3, 0.2], np.float32)
    for one_class in (np.zeros(4, np.int64), np.ones(4, np.int64)):
        with pytest.raises(ValueError):
            metrics.roc_curve(one_class, s)
        with pytest.raises(ValueError):
            metrics.precision_recall_curve(one_class, s)
    with pytest.raises(ValueError):
        metrics.roc_curve(y[:3], s)


def test_c_abi_declares_the_curve_entry_points_and_rejects_bad_arguments():
    """additive: two new symbols, the ABI version stays; bad arguments are an error code before any launch (no GPU here)"""
    import ctypes as C
    from eoe_amd import _lib
    lib = _lib.lib
    assert {"eoe_rank_curves", "eoe_rank_curves_scratch_bytes"} <= set(_lib.header_symbols())
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5
    assert lib.eoe_rank_curves_scratch_bytes(0) == 0 and lib.eoe_rank_curves_scratch_bytes((1 << 20) + 1) == 0
    assert lib.eoe_rank_curves_scratch_bytes(-5) == 0
    for n in (1, 257, 10000, 1 << 20):
        assert lib.eoe_rank_curves_scratch_bytes(n) >= 16 * n
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    good = [p, p, 1, 8, 1] + [p] * 9
    for i in (0, 1, 5, 6, 7, 8, 9, 10, 11, 12):                       # every pointer but the stream
        args = list(good)
        args[i] = None
        assert lib.eoe_rank_curves(*args) == 1, i
        assert b"rank_curves" in lib.eoe_last_error()
    for n in (0, -1, (1 << 20) + 1):
        args = list(good)
        args[3] = n
        assert lib.eoe_rank_curves(*args) == 1 and b"n must be" in lib.eoe_last_error()
