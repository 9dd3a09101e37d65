"""GPU tier: `eoe_class_breakdown` (csrc/breakdown.hip) through `metrics.class_breakdown` on device scores against the host path on the
same arrays -- the integer tables equal, the thresholds bit-equal, the APs within n_k * 2^-52, two runs the same bytes -- over the
sizes that hit tile and chunk edges, every score family, class layout, normal-class set and TPR level (tests/breakdown_util.py); a tie
group across a tile boundary; the refusals; and the trainer's option end to end in both AD modes."""
import json
import os

import numpy as np
import pytest
import torch

import breakdown_util as bu
from eoe_amd import metrics

pytestmark = pytest.mark.gpu


def _raw_bytes(bd):
    return bd.counts.tobytes() + bd.thresholds.tobytes() + np.array([np.nan if a is None else a for a in bd.ap]).tobytes()


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 513, 1031))
def test_device_equals_the_host_path_and_itself(n):
    for K in (1, 2, 3, 37) + ((1024,) if n == 1031 else ()):
        if K > n and K != 1:
            continue
        ids = bu.class_ids(n, K, seed=K, spread=(K == 3))
        idt = torch.from_numpy(ids).cuda() if K == 2 else ids                        # class ids may live on either side
        for kind in (bu.KINDS if K != 1024 else ("continuous", "zeros")):            # 1 024 classes: mostly one-sample classes
            s = bu.scores(n, kind, seed=K)
            st = torch.from_numpy(s.copy()).cuda()
            for normal in bu.normal_sets(ids):
                for q in bu.LEVELS:
                    what = f"n={n} K={K} {kind} normal={normal[:4]} q={q}"
                    dev, host = metrics.class_breakdown(st, idt, normal, tpr=q), metrics.class_breakdown(s, ids, normal, tpr=q)
                    bu.assert_same(dev, host, what)
                    if q == 0.95:
                        assert _raw_bytes(metrics.class_breakdown(st, idt, normal, tpr=q)) == _raw_bytes(dev), what


def test_a_tie_group_across_a_tile_boundary_is_written_by_its_smallest_index():
    n = 513
    ids = np.where(np.arange(n) % 2 == 0, 3, 5).astype(np.int64)                     # nominal classes 3 and 5 ...
    ids[250:263] = 7                                                                # ... an anomalous class around the tile edge at 256
    ids[400:420] = 9                                                                # and a second anomalous class with low scores
    s = bu.scores(n, "continuous", 9) * np.float32(0.25)
    s[250:254], s[254:259], s[259:263] = 5.0, 0.0, -5.0
    s[254] = -0.0                                                                   # the group's smallest index: its bits are the threshold's
    s[400:420] = -7.0
    st = torch.from_numpy(s.copy()).cuda()
    for q in (0.5, 9 / 13):                                                         # places 7 and 9 of 13: inside the group of 254..258
        dev, host = metrics.class_breakdown(st, ids, [3, 5], tpr=q), metrics.class_breakdown(s, ids, [3, 5], tpr=q)
        bu.assert_same(dev, host, f"q={q}")
        row = dev.classes.tolist().index(7)
        assert dev.thresholds[row].tobytes() == np.float32(-0.0).tobytes() and dev.counts[row, 2] == 9        # tps: 4 above + the 5 tied
        assert dev.counts[row, 1] == int((s[np.isin(ids, [3, 5])] >= 0.0).sum())
    s[254], s[258] = 0.0, -0.0                                                      # now the smallest index carries +0.0
    dev = metrics.class_breakdown(torch.from_numpy(s.copy()).cuda(), ids, [3, 5], tpr=0.5)
    bu.assert_same(dev, metrics.class_breakdown(s, ids, [3, 5], tpr=0.5))
    assert dev.thresholds[dev.classes.tolist().index(7)].tobytes() == np.float32(0.0).tobytes()
    # the pooled threshold across the same edge: all 33 anomalous samples, place 7 again
    dev = metrics.class_breakdown(torch.from_numpy(s.copy()).cuda(), ids, [3, 5], tpr=7 / 33)
    bu.assert_same(dev, metrics.class_breakdown(s, ids, [3, 5], tpr=7 / 33))
    assert dev.thresholds[-1].tobytes() == np.float32(0.0).tobytes() and dev.counts[-1, 2] == 9


def test_named_cases_and_refusals_on_the_device():
    for name, s, ids, normal in bu.named_cases():
        for q in (0.95, 19 / 20, 1.0):
            bu.assert_same(metrics.class_breakdown(torch.from_numpy(s.copy()).cuda(), ids, normal, tpr=q),
                           metrics.class_breakdown(s, ids, normal, tpr=q), f"{name} q={q}")
    s, ids = torch.rand(40).cuda(), bu.class_ids(40, 3)
    for bad in (float("nan"), float("inf"), float("-inf")):
        b = s.clone()
        b[11] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            metrics.class_breakdown(b, ids, [0])
    with pytest.raises(ValueError, match="as many class ids as scores"):
        metrics.class_breakdown(s, ids[:39], [0])
    with pytest.raises(ValueError, match="tpr must be in"):
        metrics.class_breakdown(s, ids, [0], tpr=0.0)
    with pytest.raises(ValueError, match="at most 1024 classes"):
        metrics.class_breakdown(torch.zeros(1025).cuda(), np.arange(1025), [0])
    with pytest.raises(ValueError, match="1048576 scores"):
        metrics.class_breakdown(torch.zeros((1 << 20) + 1).cuda(), np.zeros((1 << 20) + 1, np.int64), [0])


def test_a_class_id_outside_the_table_is_in_no_class_and_no_pool():
    """the C entry point alone: ids outside [0, K) (the Python layer never makes one) change nothing for the others"""
    n, K = 300, 4
    s, ids = bu.scores(n, "quant8", 11), bu.class_ids(n, K, 11).astype(np.int32)
    side, keep = np.array([0, 1, 1, 0], np.uint8), np.arange(n) % 5 != 0
    m_cls = np.array([metrics.place_for_tpr(0.95, int(((ids == k) & keep).sum())) for k in range(K)], np.int32)
    m_pooled = metrics.place_for_tpr(0.95, int((np.isin(ids, [1, 2]) & keep).sum()))
    m_cls[[0, 3]] = m_pooled
    want = metrics.class_breakdown_device(torch.from_numpy(s[keep].copy()).cuda(), ids[keep], side, m_cls, m_pooled)
    bad = ids.copy()
    bad[~keep] = np.where(np.arange((~keep).sum()) % 2 == 0, -1, K)
    got = metrics.class_breakdown_device(torch.from_numpy(s.copy()).cuda(), bad, side, m_cls, m_pooled)
    assert got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert np.all(np.abs(got[1] - want[1]) <= want[0][:K, 3] * 2.0 ** -52)          # the members sit at other indices: another summation order


# ------------------------------------------------------------------------------------------------------------ the trainer's option
def _set():
    from eoe_amd.data import LabelledImageSet
    g = torch.Generator().manual_seed(5)
    img = lambda n, lo, hi: torch.randint(lo, hi, (n, 32, 32, 3), generator=g, dtype=torch.uint8)   # noqa: E731
    train = torch.cat([img(16, 0, 100), img(16, 80, 180), img(16, 160, 256)])
    train_y = torch.arange(3).repeat_interleave(16)
    test = torch.cat([img(8, 0, 100), img(8, 80, 180), img(8, 160, 256)])
    test_y = torch.arange(3).repeat_interleave(8)
    perm = torch.randperm(24, generator=g)
    return LabelledImageSet(train, train_y, test[perm], test_y[perm], img(24, 0, 256), ["dark", "grey", "bright"], crop=32,
                            mean=[0.5] * 3, std=[0.25] * 3), test_y[perm].numpy()


@pytest.mark.parametrize("mode", ("one_vs_rest", "leave_one_out"))
def test_trainer_breaks_the_test_scores_down_by_class(tmp_path, mode):
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(0)
    lset, test_y = _set()
    d = str(tmp_path / "on")
    tr = HSCTrainer(CNN32(bias=True), dataset=lset, epochs=1, lr=1e-3, batch_size=8, ad_mode=mode, logger=JsonLogger(d), breakdown=True)
    tr.run(run_classes=[0, 2])
    assert sorted(tr.breakdowns) == [0, 2] and all(len(v) == 1 for v in tr.breakdowns.values())
    for c in (0, 2):
        with open(f"{d}/eval_cls{c}_it0_anomaly_scores.json") as f:
            logged = json.load(f)
        rows = np.array([int(k) for k in logged], dtype=np.int64)
        s = np.array(list(logged.values()), dtype=np.float32)
        assert sorted(rows.tolist()) == list(range(24))
        normal = tr.get_nominal_classes(c)
        want = metrics.class_breakdown(s, test_y[rows], normal, tpr=0.95, names=["dark", "grey", "bright"])
        got = tr.breakdowns[c][0]
        bu.assert_same(got, want, f"{mode} task {c}")
        assert got.side.tolist() == [int(k not in normal) for k in range(3)] and got.n.tolist() == [8, 8, 8]
        assert np.isfinite(got.auc).all() and np.isfinite(got.fpr_at_tpr)
        with open(f"{d}/eval_cls{c}_it0_breakdown.json") as f:
            assert json.load(f) == json.loads(json.dumps(got.to_json()))
    m = tr.breakdown_matrix()
    assert m.shape == (3, 3) and m.dtype == np.float64
    assert np.isnan(m[1]).all() and np.isfinite(m[[0, 2]]).all()                     # task 1 did not run: its row is the only NaNs
    assert np.array_equal(m[0], tr.breakdowns[0][0].auc) and np.array_equal(m[2], tr.breakdowns[2][0].auc)
    with open(f"{d}/breakdown_auc.json") as f:
        logged = json.load(f)
    assert logged["auc"][1] == [None] * 3 and logged["auc"][0] == m[0].tolist() and logged["classes"] == ["dark", "grey", "bright"]
    assert logged["fpr_at_tpr"] == [tr.breakdowns[0][0].fpr_at_tpr, None, tr.breakdowns[2][0].fpr_at_tpr] and logged["tpr_level"] == 0.95


def test_trainer_without_the_option_writes_no_breakdown(tmp_path):
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(0)
    lset, _ = _set()
    d = str(tmp_path / "off")
    tr = HSCTrainer(CNN32(bias=True), dataset=lset, epochs=1, lr=1e-3, batch_size=8, logger=JsonLogger(d))
    tr.run(run_classes=[1])
    assert tr.breakdowns == {} and os.path.exists(f"{d}/eval_cls1_it0_anomaly_scores.json")
    assert not [f for f in os.listdir(d) if "breakdown" in f]
