"""GPU tier: `eoe_rank_curves` (csrc/curves.hip) through `eoe_amd.metrics` -- every case of the fixture g23 (sklearn's curves on
stored inputs) with exact equality, the device against the host path, the areas against `eoe_auc_ap`, the C ABI's error paths, and
the trainer's `curves=True` run against its default."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from eoe_amd import metrics

pytestmark = pytest.mark.gpu

CASES = ("n2", "n3_tie", "n255", "n256", "n257", "n513_equal", "n1000_quarters", "n1023", "n1024", "n1025", "n600_separated", "n300_zeros")
trapz = getattr(np, "trapezoid", None) or np.trapz


def same(got, want, what):
    """equal shapes, equal values in float64 and, for thresholds, equal bits (`-0.0 == 0.0` would pass a value comparison)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), what
    if want.dtype == np.float32:
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what


def step_sum(prec, rec):
    return float(-np.sum(np.diff(rec) * prec[:-1]))


@pytest.mark.parametrize("case", CASES)
def test_device_curves_equal_sklearn(golden, case):
    g = golden("g23_curves")
    y, s = torch.from_numpy(g[f"{case}/y"]).cuda(), torch.from_numpy(g[f"{case}/s"]).cuda()
    full, roc = metrics.rank_curves_device(y, s)
    assert full[0].size == int(g[f"{case}/K"]) and roc[0].size == int(g[f"{case}/K_roc"])          # K, K_roc
    for prefix, got in (("roc", metrics.roc_curve(y, s)), ("rocfull", metrics.roc_curve(y, s, drop_intermediate=False))):
        for name, arr in zip(("fpr", "tpr", "thr"), got):
            same(arr, g[f"{case}/{prefix}_{name}"], f"{case} {prefix} {name}")
    for name, arr in zip(("prec", "rec", "thr"), metrics.precision_recall_curve(y, s)):
        same(arr, g[f"{case}/prc_{name}"], f"{case} prc {name}")
    (fpr, tpr, _), (prec, rec, _) = metrics.curves_device(y, s)
    same(fpr, g[f"{case}/roc_fpr"], "curves_device fpr")
    same(prec, g[f"{case}/prc_prec"], "curves_device precision")
    auc, ap = metrics.auc_ap_device(y, s)
    assert abs(trapz(tpr, fpr) - auc) < 1e-12 and abs(step_sum(prec, rec) - ap) < 1e-12


def test_device_equals_host_on_larger_and_ragged_inputs():
    """several count workgroups and several compaction chunks, with and without ties; labels may live on the host"""
    rng = np.random.default_rng(5)
    for n, levels in ((4097, None), (5000, 40), (3001, 2)):
        s = rng.standard_normal(n).astype(np.float32)
        if levels:
            s = (np.round(s * levels) / levels).astype(np.float32)
        y = (rng.random(n) < 0.3).astype(np.int64)
        st = torch.from_numpy(s).cuda()
        for drop in (True, False):
            for a, b in zip(metrics.roc_curve(torch.from_numpy(y), st, drop), metrics.roc_curve(y, s, drop)):
                same(a, b, f"roc n={n} levels={levels} drop={drop}")
        dev, host = metrics.precision_recall_curve(torch.from_numpy(y).cuda(), st), metrics.precision_recall_curve(y, s)
        for a, b in zip(dev, host):
            same(a, b, f"prc n={n} levels={levels}")
        auc, ap = metrics.auc_ap_device(torch.from_numpy(y), st)
        fpr, tpr, _ = metrics.roc_curve(torch.from_numpy(y), st)
        assert abs(trapz(tpr, fpr) - auc) < 1e-12 and abs(step_sum(dev[0], dev[1]) - ap) < 1e-12
    # n = 1: one slot
    full, roc = metrics.rank_curves_device(torch.ones(1, dtype=torch.int64), torch.tensor([0.5]).cuda())
    assert [a.tolist() for a in full] == [[0], [1], [0.5]] and [a.tolist() for a in roc] == [[0], [1], [0.5]]


def test_device_curves_reject_nonfinite_and_single_class():
    y = torch.tensor([0, 1, 1, 0]).cuda()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            metrics.roc_curve(y, torch.tensor([0.1, bad, 0.3, 0.2]).cuda())
    s = torch.tensor([0.1, 0.4, 0.3, 0.2]).cuda()
    for one_class in (torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            metrics.roc_curve(one_class, s)
        with pytest.raises(ValueError):
            metrics.precision_recall_curve(one_class, s)


def test_rank_curves_bad_arguments_return_the_error_code():
    from eoe_amd._lib import lib
    n = 8
    s, y = torch.rand(n).cuda(), torch.zeros(n, dtype=torch.int64).cuda()
    i64 = torch.empty((4, n), dtype=torch.int64, device="cuda")
    f32 = torch.empty((2, n), dtype=torch.float32, device="cuda")
    counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.eoe_rank_curves_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = [s.data_ptr(), y.data_ptr(), 1, n, 1, i64[0].data_ptr(), i64[1].data_ptr(), f32[0].data_ptr(), i64[2].data_ptr(),
            i64[3].data_ptr(), f32[1].data_ptr(), counts.data_ptr(), scratch.data_ptr(), st]
    for i in (0, 1, 5, 6, 7, 8, 9, 10, 11, 12):
        args = list(good)
        args[i] = None
        assert lib.eoe_rank_curves(*args) == 1, i
    for bad_n in (0, -3, (1 << 20) + 1):
        args = list(good)
        args[3] = bad_n
        assert lib.eoe_rank_curves(*args) == 1 and b"n must be" in lib.eoe_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [-7, -7]                                 # nothing was launched
    assert lib.eoe_rank_curves(*good) == 0
    assert counts.tolist()[0] == n                                     # random scores: all distinct


def _run(tmp_path, curves):
    from eoe_amd.data import SyntheticAD
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(11)
    ds = SyntheticAD(n_train_normal=64, n_oe=64, n_test=64, res=32, shift=0.3, seed=4)
    logdir = str(tmp_path / ("curves" if curves else "plain"))
    kw = {"curves": True} if curves else {}
    tr = TRAINER["hsc"](CNN32(bias=True), dataset=ds, epochs=2, lr=1e-3, wdk=0.0, milestones=[], batch_size=32, classes=["only"],
                        logger=JsonLogger(logdir), **kw)
    np.random.seed(123)
    _, res = tr.run(run_seeds=2)
    return tr, res, logdir, np.random.get_state()


def test_trainer_curves_agree_with_its_scores_and_the_default_is_untouched(tmp_path):
    tr, res, logdir, state = _run(tmp_path, True)
    plain, res_plain, logdir_plain, state_plain = _run(tmp_path, False)
    # ---- the default: the same scores, no curve, no draw, no curve file
    assert res_plain == res
    assert plain.curves is None
    np.random.seed(123)
    untouched = np.random.get_state()
    assert np.array_equal(state_plain[1], untouched[1]) and state_plain[2] == untouched[2]
    assert not any(f.endswith(("_roc.json", "_prc.json")) for f in os.listdir(logdir_plain))
    # ---- curves=True
    c = tr.curves
    assert set(c) == {"train_rocs", "eval_rocs", "eval_prcs", "mean_train_rocs", "mean_eval_rocs", "mean_eval_prcs"}
    assert all(len(c[k]) == 1 for k in c) and all(len(c[k][0]) == 2 for k in ("train_rocs", "eval_rocs", "eval_prcs"))
    for seed in range(2):
        roc, prc, troc = c["eval_rocs"][0][seed], c["eval_prcs"][0][seed], c["train_rocs"][0][seed]
        assert roc.auc == res["cls_aucs"][0][seed]
        with open(os.path.join(logdir, f"eval_cls0_it{seed}_anomaly_scores.json")) as f:
            scores = np.array(list(json.load(f).values()))
        assert abs(trapz(roc.tpr, roc.fpr) - roc.auc) < 1e-12 and abs(step_sum(prc.prec, prc.rec) - prc.avg_prec) < 1e-12
        assert abs(trapz(troc.tpr, troc.fpr) - troc.auc) < 1e-12
        assert roc.ths.dtype == np.float32 and np.isinf(roc.ths[0]) and float(roc.ths[-1]) == scores.min()
        assert float(prc.ths[0]) == scores.min() and float(prc.ths[-1]) == scores.max() and float(roc.ths[1]) == scores.max()
        assert roc.fpr[0] == 0 and roc.tpr[0] == 0 and roc.fpr[-1] == 1 and roc.tpr[-1] == 1
        assert prc.prec[-1] == 1 and prc.rec[-1] == 0 and prc.rec[0] == 1 and prc.ths.size == prc.prec.size - 1
        assert troc.fpr[-1] == 1 and troc.tpr[-1] == 1 and troc.ths.size == troc.fpr.size
        with open(os.path.join(logdir, f"eval_cls0_it{seed}_roc.json")) as f:
            j = json.load(f)
        assert j["fpr"] == roc.fpr.tolist() and j["tpr"] == roc.tpr.tolist() and j["ths"] == roc.ths.tolist() and j["auc"] == roc.auc
        with open(os.path.join(logdir, f"eval_cls0_it{seed}_prc.json")) as f:
            j = json.load(f)
        assert j["prec"] == prc.prec.tolist() and j["rec"] == prc.rec.tolist() and j["avg_prec"] == prc.avg_prec
    # the seeds' means: mean_plot's draws in the reference's order, and no other draw
    np.random.seed(123)
    want = [metrics.mean_plot(copy.deepcopy(c[k][0])) for k in ("train_rocs", "eval_rocs", "eval_prcs")]
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2] == after[2]
    for got, w in zip((c["mean_train_rocs"][0], c["mean_eval_rocs"][0], c["mean_eval_prcs"][0]), want):
        assert type(got) is type(w) and got.n == 2 and got.get_score() == w.get_score() and got.std == w.std
        assert np.array_equal(got.get_x(), w.get_x()) and np.array_equal(got.get_y(), w.get_y()) and np.array_equal(got.ths, w.ths)
    assert c["mean_eval_rocs"][0].auc == res["mean_auc"]
