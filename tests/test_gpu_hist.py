"""GPU tier: `eoe_score_hist` (csrc/hist.hip) through `eoe_amd.metrics` -- every case of tests/hist_util.py against the restatement of
TensorBoard's histogram applied to host copies, the unlabelled form, explicit edges at 3 and at the cap, repeatability bit for bit, a
dirty scratch buffer, the refusals, and the trainer's `histograms=True` run against its default."""
import json
import os

import numpy as np
import pytest
import torch

import hist_util
from eoe_amd import metrics

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,how", hist_util.CASES)
def test_device_histograms_equal_the_restatement(n, how):
    s, y = hist_util.scores(n), hist_util.labels(n, how)
    st, yt = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    want = hist_util.expected(n, how)
    got = metrics.score_histograms(yt, st)
    for k in (0, 1):
        hist_util.check(got[k], s[y == k], want[k], f"n={n} {how} label {k}")
        one = metrics.score_histogram(st, yt, k)
        assert (one is None and got[k] is None) or one == got[k]
    host = metrics.score_histograms(y, s)                                          # the host path: the same integers and ends
    for d, h in zip(got, host):
        assert (d is None) == (h is None)
        if d is not None:
            assert (d.bucket, d.bucket_limit, d.num, d.min, d.max) == (h.bucket, h.bucket_limit, h.num, h.min, h.max)
    if how == "zeros":                                                              # the unlabelled form; labels may live on the host
        hist_util.check(metrics.score_histogram(st), s, hist_util.expected(n, None), f"n={n} unlabelled")
        assert metrics.score_histograms(torch.from_numpy(y.copy()), st)[0] == got[0]


@pytest.mark.parametrize("key", ("three", "cap"))
def test_device_histograms_with_explicit_edges(key):
    edges = hist_util.explicit_edges(key)
    for n in (257, 90001):
        s, y = hist_util.scores(n), hist_util.labels(n, "mixed_unlabelled")
        st, yt = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
        got = metrics.score_histograms(yt, st, bins=edges)
        for k in (0, 1):
            hist_util.check(got[k], s[y == k], hist_util.expected(n, "mixed_unlabelled", key)[k], f"{key} n={n} label {k}")
        hist_util.check(metrics.score_histogram(st, bins=edges), s, hist_util.expected(n, None, key), f"{key} n={n}")


def test_two_runs_give_the_same_bytes_and_a_dirty_scratch_changes_nothing():
    from eoe_amd._lib import lib
    for n in (257, 90001):
        s, y = hist_util.scores(n), hist_util.labels(n, "mixed_unlabelled")
        st, yt = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
        need = lib.eoe_score_hist_scratch_bytes(n)
        runs = [metrics.score_hist_device(st, yt) for _ in range(2)]
        runs.append(metrics.score_hist_device(st, yt, scratch=torch.zeros(need, dtype=torch.uint8, device="cuda")))
        runs.append(metrics.score_hist_device(st, yt, scratch=torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")))
        counts, stats, edges = runs[0]
        assert counts.shape == (2, edges.size - 1) and stats.shape == (2, 5) and stats.dtype == np.float64
        assert counts[0].sum() + counts[1].sum() <= n and int(stats[0, 0] + stats[1, 0]) == int((y >= 0).sum())
        for c, t, _ in runs[1:]:
            assert c.tobytes() == counts.tobytes() and t.tobytes() == stats.tobytes()
        with pytest.raises(ValueError):
            metrics.score_hist_device(st, yt, scratch=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))


def test_device_refusals_and_an_empty_group():
    y = torch.tensor([0, 1, 1, 0]).cuda()
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            metrics.score_histograms(y, torch.tensor([0.1, bad, 0.3, 0.2]).cuda())
    s = torch.tensor([0.1, 0.4, 0.3, 0.2]).cuda()
    with pytest.raises(ValueError):
        metrics.score_histograms(y[:3], s)
    with pytest.raises(ValueError):
        metrics.score_histogram(s, bins=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        metrics.score_histogram(s, bins=np.arange(metrics.HIST_MAX_EDGES + 1, dtype=np.float64))
    with pytest.raises(ValueError):
        metrics.score_histogram(torch.zeros(0).cuda())
    assert metrics.score_histograms(torch.zeros(4, dtype=torch.int64), s)[1] is None
    assert metrics.score_histograms(torch.full((4,), -1), s) == (None, None)
    counts, stats, _ = metrics.score_hist_device(s, torch.ones(4, dtype=torch.int64))
    assert stats[0].tolist() == [0.0] * 5 and stats[1, 0] == 4.0 and counts[0].sum() == 0 and counts[1].sum() == 4


def test_score_hist_bad_arguments_launch_nothing():
    from eoe_amd._lib import lib
    n = 8
    s = torch.rand(n).cuda()
    edges = np.array([-1.0, 0.0, 1.0])
    dev_edges = torch.from_numpy(edges).cuda()
    counts = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((2, 5), -7.0, dtype=torch.float64, device="cuda")
    scratch = torch.empty(lib.eoe_score_hist_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    good = [s.data_ptr(), None, n, edges.ctypes.data, dev_edges.data_ptr(), 3, counts.data_ptr(), stats.data_ptr(), scratch.data_ptr(),
            torch.cuda.current_stream().cuda_stream]
    for i in (0, 3, 4, 6, 7, 8):
        args = list(good)
        args[i] = None
        assert lib.eoe_score_hist(*args) == 1, i
    for i, v in ((2, 0), (5, 1), (5, 4002)):
        args = list(good)
        args[i] = v
        assert lib.eoe_score_hist(*args) == 1
    unsorted = np.array([-1.0, 1.0, 0.0])
    args = list(good)
    args[3] = unsorted.ctypes.data
    assert lib.eoe_score_hist(*args) == 1 and b"ascending" in lib.eoe_last_error()
    torch.cuda.synchronize()
    assert counts.flatten().tolist() == [-7] * 4 and stats.flatten().tolist() == [-7.0] * 10     # nothing was launched
    assert lib.eoe_score_hist(*good) == 0
    assert counts.tolist() == [[0, n], [0, 0]] and stats[0, 0].item() == n and stats[1].tolist() == [0.0] * 5


def _run(tmp_path, histograms):
    from eoe_amd.data import SyntheticAD
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(11)
    ds = SyntheticAD(n_train_normal=48, n_oe=48, n_test=40, res=32, shift=0.3, seed=4)
    logdir = str(tmp_path / ("hist" if histograms else "plain"))
    kw = {"histograms": True} if histograms else {}
    tr = TRAINER["hsc"](CNN32(bias=True), dataset=ds, epochs=2, lr=1e-3, wdk=0.0, milestones=[], batch_size=32, classes=["only"],
                        logger=JsonLogger(logdir), **kw)
    _, res = tr.run(run_seeds=1)
    return tr, res, logdir, ds


def test_trainer_histograms_agree_with_its_scores_and_the_default_is_untouched(tmp_path):
    tr, res, logdir, ds = _run(tmp_path, True)
    plain, res_plain, logdir_plain, _ = _run(tmp_path, False)
    # ---- the switch changes nothing else
    assert res_plain == res and plain.last_losses == tr.last_losses and len(tr.last_scores) == 2
    for (la, sc), (la_p, sc_p) in zip(tr.last_scores, plain.last_scores):
        assert torch.equal(la, la_p) and torch.equal(sc, sc_p)
    with open(os.path.join(logdir, "eval_cls0_it0_anomaly_scores.json"), "rb") as f, \
            open(os.path.join(logdir_plain, "eval_cls0_it0_anomaly_scores.json"), "rb") as g:
        logged = f.read()
        assert logged == g.read()
    # ---- the default: nothing kept, nothing written
    assert plain.histograms == {} and plain.logger.histograms == {}
    assert not os.path.exists(os.path.join(logdir_plain, "histograms.json"))
    assert sorted(os.listdir(logdir_plain)) == sorted(f for f in os.listdir(logdir) if f != "histograms.json")
    # ---- histograms=True: one pair per epoch and the evaluation's pair, under the reference's tags
    t_norm, t_anom = "Training: CLS0 SEED0 anomaly_scores normal", "Training: CLS0 SEED0 anomaly_scores anomalous"
    e_nom, e_anom = "Eval: (SD0) anomaly_scores cls0 nominal", "Eval: (SD0) anomaly_scores cls0 anomalous"
    h = tr.histograms
    assert set(h) == {t_norm, t_anom, e_nom, e_anom}
    assert set(h[t_norm]) == set(h[t_anom]) == {0, 1} and set(h[e_nom]) == set(h[e_anom]) == {0}
    for ep, (la, sc) in enumerate(tr.last_scores):
        la, sc = la.cpu().numpy(), sc.cpu().numpy()
        assert sc.dtype == np.float32 and (la == 0).sum() == 48 and (la == 1).any()
        for tag, k in ((t_norm, 0), (t_anom, 1)):
            hist_util.check(h[tag][ep], sc[la == k], hist_util.restate(sc[la == k]), f"{tag} step {ep}")
    test_scores = np.array(list(json.loads(logged).values()), np.float64).astype(np.float32)
    test_y = ds.test_y.numpy()
    for tag, k in ((e_nom, 0), (e_anom, 1)):
        hist_util.check(h[tag][0], test_scores[test_y == k], hist_util.restate(test_scores[test_y == k]), tag)
    # ---- the logger holds the same objects and its file the same numbers
    assert tr.logger.histograms == h
    with open(os.path.join(logdir, "histograms.json")) as f:
        j = json.load(f)
    assert {t: {int(s): metrics.Histogram(**d) for s, d in steps.items()} for t, steps in j.items()} == h
