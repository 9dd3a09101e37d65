"""CPU tier: the host path of `eoe_amd.metrics.class_breakdown` against sklearn on every class's sub-problem and on the pooled problem,
the place of a TPR level, the refusals, the C ABI's argument checks (no GPU here: nothing is launched), and the trainer's and the data
layer's wiring."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest
import torch

import breakdown_util as bu
from eoe_amd import metrics


def _fpr_at(y, s, q):
    from sklearn.metrics import roc_curve
    fpr, tpr, thr = roc_curve(y, s, drop_intermediate=False)
    at = int(np.argmax(tpr >= q))
    return fpr[at], thr[at]


def _check_against_sklearn(bd, s, ids, normal, q, what):
    from sklearn.metrics import average_precision_score, roc_auc_score
    anomalous = ~np.isin(ids, normal)
    assert bd.classes.tolist() == np.unique(ids).tolist() and bd.tpr_level == q
    for j, k in enumerate(bd.classes):
        where = (what, int(k))
        assert bd.n[j] == (ids == k).sum() and bd.side[j] == int(k not in normal), where
        y, sub = bu.sub_problem(s, ids, normal, int(k))
        if y.min() == y.max():                                                      # an empty pool: NaN rows
            assert np.isnan(bd.auc[j]) and np.isnan(bd.fpr[j]) and (bd.ap[j] is None or np.isnan(bd.ap[j])), where
            assert (bd.ap[j] is None) == (bd.side[j] == 0), where
            continue
        assert abs(bd.auc[j] - roc_auc_score(y, sub)) <= 1e-12, where
        assert bd.fpr[j] == _fpr_at(y, sub, q)[0], where
        if bd.side[j]:
            assert abs(bd.ap[j] - average_precision_score(y, sub)) <= int(bd.n[j]) * 2.0 ** -52, where
        else:
            assert bd.ap[j] is None, where
    if anomalous.all() or not anomalous.any():
        assert np.isnan(bd.fpr_at_tpr) and np.isnan(bd.threshold), what
    else:
        fpr, thr = _fpr_at(anomalous.astype(np.int64), s, q)
        assert bd.fpr_at_tpr == fpr and bd.threshold == thr, what


@pytest.mark.parametrize("case", bu.named_cases(), ids=lambda c: c[0])
def test_host_path_equals_sklearn_on_every_sub_problem_and_pooled(case):
    name, s, ids, normal = case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for q in (0.5, 0.95, 1.0, 19 / 20):
            _check_against_sklearn(metrics.class_breakdown(s, ids, normal, tpr=q), s, ids, normal, q, f"{name} q={q}")


def test_place_for_tpr_is_the_smallest_m_whose_rate_reaches_the_level():
    for n_pos in (1, 2, 3, 7, 19, 20, 21, 100, 997, 1 << 20):
        for q in (1e-9, 0.05, 0.5, 0.95, 19 / 20, 1.0, 1 / 3, 0.7, 0.999999):
            m = metrics.place_for_tpr(q, n_pos)
            assert 1 <= m <= n_pos and m / n_pos >= q and (m == 1 or (m - 1) / n_pos < q), (n_pos, q, m)
    assert metrics.place_for_tpr(19 / 20, 20) == 19 and metrics.place_for_tpr(0.95, 20) == 19 and metrics.place_for_tpr(0.95, 0) == 0
    # a level the ceiling alone would miss by one: every k / n of the divisions sklearn makes
    for n_pos in (10, 20, 49, 100):
        for k in range(1, n_pos + 1):
            assert metrics.place_for_tpr(k / n_pos, n_pos) == k, (k, n_pos)


def test_inputs_of_any_kind_names_and_json():
    s, ids = bu.scores(60, "quant8"), bu.class_ids(60, 3)
    want = metrics.class_breakdown(s, ids, [1], names=["cat", "dog", "truck"])
    assert want.names == ["cat", "dog", "truck"] and want.side.tolist() == [1, 0, 1] and want.ap[1] is None
    bu.assert_same(metrics.class_breakdown(torch.from_numpy(s), torch.from_numpy(ids), torch.tensor([1]), names={0: "cat", 1: "dog", 2: "truck"}),
                   want)
    assert metrics.class_breakdown(s, ids.tolist(), (1,)).names == ["0", "1", "2"]
    assert metrics.class_breakdown(s, ids, [1], names=["cat"]).names == ["cat", "1", "2"]
    d = json.loads(json.dumps(want.to_json(), allow_nan=False))
    assert d["classes"] == [0, 1, 2] and d["ap"][1] is None and d["auc"] == want.auc.tolist() and d["tpr_level"] == 0.95
    assert d["fpr_at_tpr"] == want.fpr_at_tpr and d["threshold"] == want.threshold and d["n"] == want.n.tolist()
    hard = want.hardest()
    assert hard == (int(want.classes[np.argmin(want.auc)]), want.names[int(np.argmin(want.auc))], float(want.auc.min()))
    empty = metrics.class_breakdown(s, ids, [0, 1, 2])
    assert empty.hardest() is None and json.loads(json.dumps(empty.to_json(), allow_nan=False))["auc"] == [None] * 3
    assert empty.counts[:, :3].tolist() == [[0, 0, 0]] * 4 and empty.counts[:3, 3].tolist() == empty.n.tolist()
    # float64 scores are compared as float64: two scores one float32 rounding apart are not a tie
    s64 = np.array([0.1, 0.1 + 1e-12, 0.3, 0.05], dtype=np.float64)
    assert metrics.class_breakdown(s64, [0, 1, 1, 0], [0]).auc.tolist() == [1.0, 1.0]
    assert metrics.class_breakdown(s64.astype(np.float32), [0, 1, 1, 0], [0]).auc.tolist() == [0.875, 0.875]


def test_refusals():
    s, ids = bu.scores(40, "continuous"), bu.class_ids(40, 3)
    for bad in (np.nan, np.inf, -np.inf):
        b = s.copy()
        b[11] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            metrics.class_breakdown(b, ids, [0])
    with pytest.raises(ValueError, match="as many class ids as scores"):
        metrics.class_breakdown(s, ids[:39], [0])
    with pytest.raises(ValueError, match="as many class ids as scores"):
        metrics.class_breakdown(s[:0], ids[:0], [0])
    for q in (0.0, -0.1, 1.0000001, float("nan"), True, "0.95"):
        with pytest.raises(ValueError, match="tpr must be in"):
            metrics.class_breakdown(s, ids, [0], tpr=q)
    with pytest.raises(ValueError, match="integers"):
        metrics.class_breakdown(s, ids.astype(np.float32), [0])
    many = np.arange(1025)
    with pytest.raises(ValueError, match="at most 1024 classes"):
        metrics.class_breakdown(np.zeros(1025, np.float32), many, [0])
    assert len(metrics.class_breakdown(np.zeros(1024, np.float32), many[:1024], [0]).classes) == 1024
    with pytest.raises(RuntimeError):
        metrics.class_breakdown_device(s, ids.astype(np.int32), np.zeros(3, np.uint8), np.ones(3, np.int32), 1)


def test_c_abi_declares_the_breakdown_entry_points_and_rejects_bad_arguments_before_any_launch():
    """additive: two new symbols, the ABI version stays; bad arguments are error code 1 and a message that names the argument"""
    from eoe_amd import _lib
    lib = _lib.lib
    new = {"eoe_class_breakdown", "eoe_class_breakdown_scratch_bytes"}
    assert new <= set(_lib.header_symbols()) and new <= set(_lib.SIGNATURES)
    assert all(getattr(lib, name) is not None for name in new)
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5
    sb = lib.eoe_class_breakdown_scratch_bytes
    for n, K in ((0, 3), (-1, 3), ((1 << 20) + 1, 3), (100, 0), (100, -1), (100, 1025), (0, 0)):
        assert sb(n, K) == 0, (n, K)
    for n, K in ((1, 1), (100, 10), (1 << 20, 1024), (1, 1024), (1 << 20, 1)):
        assert sb(n, K) >= 4 * 4 * n and sb(n, K) % 4 == 0, (n, K)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p += -p % 16
    f, err = lib.eoe_class_breakdown, lib.eoe_last_error
    # eoe_class_breakdown(scores, class_ids, side_per_class, m_per_class, m_pooled, n, K, out_counts, out_ap, out_thr, scratch, stream)
    good = [p, p, p, p, 1, 8, 2, p, p, p, p, None]
    names = {0: b"scores", 1: b"class_ids", 2: b"side_per_class", 3: b"m_per_class", 7: b"out_counts", 8: b"out_ap", 9: b"out_thr",
             10: b"scratch"}
    for i, name in names.items():
        args = list(good)
        args[i] = None
        assert f(*args) == 1 and b"class_breakdown: null " + name in err(), (i, err())
    for n in (0, -1, (1 << 20) + 1):
        args = list(good)
        args[5] = n
        assert f(*args) == 1 and b"n must be in [1, 1048576]" in err(), (n, err())
    for K in (0, -1, 1025):
        args = list(good)
        args[6] = K
        assert f(*args) == 1 and b"K must be in [1, 1024]" in err(), (K, err())
    for mp in (-1, 9):
        args = list(good)
        args[4] = mp
        assert f(*args) == 1 and b"m_pooled must be in" in err(), (mp, err())
    for i, off in ((0, 2), (1, 2), (3, 2), (7, 4), (8, 4), (9, 2), (10, 1)):         # the side table is bytes: any address
        args = list(good)
        args[i] = p + off
        assert f(*args) == 1 and names[i] + b" must be " in err() and b"-byte aligned" in err(), (i, err())


def test_trainer_takes_the_option_and_refuses_a_source_without_classes_before_scoring():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    on = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", breakdown=True, breakdown_tpr=0.9)
    off = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu")
    assert on.with_breakdown and on.breakdown_tpr == 0.9 and on.breakdowns == {}
    assert not off.with_breakdown and off.breakdown_tpr == 0.95 and off.breakdowns == {}
    for bad in (0.0, 1.5, -1, True, "0.9"):
        with pytest.raises(ValueError, match="breakdown_tpr"):
            TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", breakdown=True, breakdown_tpr=bad)

    class Forgetful:
        nominal_label, normalize = 0, None

        def loaders(self, *a, **k):
            raise AssertionError("the refusal must come before any scoring")

    with pytest.raises(NotImplementedError, match="breakdown=True needs a source with test_classes"):
        on.eval_cls(CNN32(bias=True), Forgetful(), 0, "0", 0)
    with pytest.raises(AssertionError, match="before any scoring"):                 # without the option the source is asked for its loaders
        off.eval_cls(CNN32(bias=True), Forgetful(), 0, "0", 0)


def test_labelled_set_hands_its_test_classes_to_the_source():
    from eoe_amd.data import LabelledImageSet, ResidentImageSource
    assert ResidentImageSource.test_classes is None
    u8 = torch.zeros((6, 8, 8, 3), dtype=torch.uint8)
    test_classes = torch.tensor([2, 0, 1, 1, 2, 0])
    lset = LabelledImageSet(u8, torch.tensor([0, 0, 1, 1, 2, 2]), u8, test_classes, u8, ["a", "b", "c"], 8, device="cpu")
    src = lset.source([1], seed=0)
    assert torch.equal(src.test_classes, test_classes) and src.test_y.tolist() == [1, 1, 0, 0, 1, 1]
    plain = ResidentImageSource(u8, u8, u8, torch.tensor([0, 1, 0, 1, 0, 1]), 8, device="cpu")
    assert plain.test_classes is None


def _hand_made(classes, auc, fpr_at_tpr):
    k = len(classes)
    return metrics.Breakdown(classes, [str(c) for c in classes], [0] * k, [1] * k, auc, [None] * k, [0.0] * k, 0.95, fpr_at_tpr, 0.0)


def test_breakdown_matrix_puts_the_nan_cells_where_they_belong():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    tr = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", breakdown=True, classes=["a", "b", "c", "d"])
    assert tr.breakdown_matrix().shape == (4, 4) and np.isnan(tr.breakdown_matrix()).all()
    nan = float("nan")
    tr.breakdowns = {0: [_hand_made([0, 1, 3], [0.5, 0.75, nan], 0.1), _hand_made([0, 1, 3], [0.7, 0.25, nan], 0.3)],      # two seeds
                     2: [_hand_made([1, 2, 7], [1.0, 0.0, 0.4], nan)],               # class 7 is not one of the trainer's
                     3: [_hand_made([0], [nan], nan), _hand_made([0, 2], [0.25, nan], 0.5)]}
    m = tr.breakdown_matrix()
    assert m.dtype == np.float64 and m.shape == (4, 4)
    want = np.array([[0.6, 0.5, nan, nan], [nan, nan, nan, nan], [nan, 1.0, 0.0, nan], [0.25, nan, nan, nan]])
    assert np.array_equal(np.isnan(m), np.isnan(want)) and np.allclose(m[~np.isnan(want)], want[~np.isnan(want)], rtol=0, atol=1e-15)
