"""CPU tier: the float64 statement of the greedy k-center selection (`coreset.kcenter_np`) on hand-worked sets, the 2-approximation
against a brute-force optimum, non-finite rows, the share form of m, argument checks of the Python layer, of the C ABI and of the
trainer, and `kcenter` on CPU tensors."""
import itertools
import math

import numpy as np
import pytest
import torch

import coreset_util

NEW_SYMBOLS = ("eoe_feature_coreset", "eoe_feature_coreset_scratch_bytes")
X, I, R, A, D2, C, S = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000      # non-null, 16-byte aligned addresses nothing reads


def test_the_two_entry_points_are_exported_and_the_abi_version_stays():
    from eoe_amd import _lib
    import eoe_amd
    assert _lib.lib.eoe_abi_version() == 5 and _lib.ABI_VERSION == 5
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(_lib.lib, name)
    assert coreset_util.cover_is_complete()
    assert eoe_amd.coreset.kcenter is not None and "coreset" in eoe_amd.__all__
    assert coreset_util.R == 4 * coreset_util.W                                       # four waves of W rows


def test_feature_coreset_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_feature_coreset, lib.eoe_last_error
    # eoe_feature_coreset(x, ldx, n, D, m, start, idx, radius, assign, d2min, counts, scratch, stream)
    good = [X, 8, 10, 8, 5, 0, I, R, A, D2, C, S, None]

    def refused(i, v, msg):
        args = list(good)
        args[i] = v
        assert f(*args) == 1 and b"feature_coreset" in err() and msg in err(), (i, v, err())
    for i in (0, 6, 7, 8, 9, 10, 11):
        refused(i, None, b"null")
    for D in (0, 2049, -1):
        refused(3, D, b"D must be")
    refused(1, 7, b"ldx")
    for n in (0, -1, 1 << 24):
        refused(2, n, b"n must be")
    for m in (0, 11, -1):
        refused(4, m, b"m must be")
    for start in (-1, 10):
        refused(5, start, b"start must be")
    refused(0, X + 2, b"aligned")
    refused(11, S + 4, b"aligned")
    sb = lib.eoe_feature_coreset_scratch_bytes
    assert sb(10, 8, 5) >= 8 * 5 + 4 * 10 and sb(10, 8, 5) % 16 == 0 and sb(1000, 8, 5) > sb(10, 8, 5) and sb(1000, 8, 500) > sb(1000, 8, 5)
    for n, D, m in ((0, 4, 1), (4, 0, 1), (4, 2049, 1), (4, 4, 0), (4, 4, 5), (1 << 24, 4, 1)):
        assert sb(n, D, m) == 0


def test_kcenter_np_on_hand_worked_sets():
    from eoe_amd.coreset import kcenter_np
    # collinear points 0 1 3 7 12 from the left end: the far end, then the widest gaps' far sides
    x = np.array([[0.], [1.], [3.], [7.], [12.]])
    idx, radius, assign, d2min, bad = kcenter_np(x, 5, 0)
    assert idx.tolist() == [0, 4, 3, 2, 1] and radius.tolist() == [np.inf, 144., 25., 9., 1.] and bad == 0
    assert assign.tolist() == [0, 4, 3, 2, 1] and d2min.tolist() == [0.] * 5
    idx, radius, assign, d2min, _ = kcenter_np(x, 2, 0)
    assert idx.tolist() == [0, 4] and assign.tolist() == [0, 0, 0, 1, 1] and d2min.tolist() == [0., 1., 9., 25., 0.]
    idx, radius, assign, d2min, _ = kcenter_np(x, 3, 2)                                  # an interior start: 12, then 7 (4 from 3) before 0 (3 from 3)
    assert idx.tolist() == [2, 4, 3] and radius.tolist() == [np.inf, 81., 16.]
    assert assign.tolist() == [0, 0, 0, 2, 1] and d2min.tolist() == [9., 4., 0., 0., 0.]
    # equal distances: the lowest row is chosen, and the earliest centre keeps a row at equal distance from two
    x = np.array([[0., 0.], [2., 0.], [0., 2.], [-2., 0.], [1., 1.]])
    idx, radius, assign, d2min, _ = kcenter_np(x, 3, 0)
    assert idx.tolist() == [0, 1, 2] and radius.tolist() == [np.inf, 4., 4.]
    assert assign.tolist() == [0, 1, 2, 0, 0] and d2min.tolist() == [0., 0., 0., 4., 2.]  # row 4: sqrt(2) from all three centres
    # duplicates: the lowest index first, radius 0 once only duplicates remain, m = n a permutation
    x = np.array([[5., 5.], [0., 0.], [5., 5.], [0., 0.], [5., 5.], [9., 9.]])
    idx, radius, assign, d2min, _ = kcenter_np(x, 6, 1)
    assert idx.tolist() == [1, 5, 0, 2, 3, 4] and radius.tolist() == [np.inf, 162., 32., 0., 0., 0.]
    assert sorted(idx.tolist()) == list(range(6)) and assign.tolist() == [2, 0, 3, 4, 5, 1] and not d2min.any()
    idx, radius, assign, _, _ = kcenter_np(x, 3, 1)
    assert idx.tolist() == [1, 5, 0] and assign.tolist() == [2, 0, 2, 0, 2, 1]          # a duplicate stays with the first of its kind
    one = kcenter_np(np.array([[3., 4.]]), 1, 0)
    assert one[0].tolist() == [0] and np.isposinf(one[1][0]) and one[2].tolist() == [0] and one[3].tolist() == [0.]


def test_greedy_cover_is_within_twice_the_optimum_on_every_seed():
    from eoe_amd.coreset import kcenter_np
    for seed in range(20):
        x = np.random.default_rng(seed).standard_normal((10, 2))
        dist = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
        opt = min(dist[:, list(cs)].min(axis=1).max() for cs in itertools.combinations(range(10), 3))
        idx, radius, assign, d2min, _ = kcenter_np(x, 3, seed % 10)
        cover = math.sqrt(d2min.max())
        assert cover <= 2 * opt, (seed, cover, opt)
        assert cover >= opt - 1e-12                                                  # no three rows cover better than the best three
        assert np.allclose(d2min, dist[:, idx].min(axis=1) ** 2) and (np.diff(radius[1:]) <= 0).all()


def test_non_finite_rows_are_skipped_and_counted_and_a_non_finite_start_raises():
    from eoe_amd.coreset import kcenter_np
    x = np.array([[0.], [np.nan], [3.], [np.inf], [7.], [-np.inf]])
    idx, radius, assign, d2min, bad = kcenter_np(x, 3, 0)
    assert bad == 3 and idx.tolist() == [0, 4, 2] and radius.tolist() == [np.inf, 49., 9.]
    assert assign.tolist() == [0, -1, 2, -1, 1, -1] and np.isnan(d2min[[1, 3, 5]]).all() and d2min[[0, 2, 4]].tolist() == [0., 0., 0.]
    idx, radius, _, _, _ = kcenter_np(x, 6, 2)                                           # three eligible rows for six centres
    assert idx.tolist() == [2, 4, 0, -1, -1, -1] and radius[:3].tolist() == [np.inf, 16., 9.] and np.isnan(radius[3:]).all()
    for start in (1, 3, 5):
        with pytest.raises(ValueError, match="start row"):
            kcenter_np(x, 2, start)


def test_m_as_a_share_of_the_rows_and_argument_errors():
    from eoe_amd import coreset
    x = coreset_util.exact_features(40, 5, 1)
    for share, m in ((0.25, 10), (0.26, 11), (0.001, 1), (0.999, 40), (np.float32(0.5), 20)):
        assert coreset.kcenter_np(x, share)[0].size == m and coreset.kcenter(x, share).m == m
    for bad in (0, 41, -1, True, 1.0, 0.0, 1.5, -0.5, "3", None):
        with pytest.raises(ValueError, match="m "):
            coreset.kcenter_np(x, bad)
    for bad in (-1, 40, True, 1.0, None):
        with pytest.raises(ValueError, match="start must be"):
            coreset.kcenter_np(x, 3, bad)
    for shape in ((0, 5), (5,), (2, 3, 4), (4, 0), (4, 2049)):
        with pytest.raises(ValueError):
            coreset.kcenter_np(np.zeros(shape, np.float32), 1)
    with pytest.raises(ValueError, match="float32"):
        coreset.kcenter(torch.zeros(4, 4, dtype=torch.float64), 2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        coreset.kcenter_device(torch.zeros(4, 4), 2)


def test_kcenter_on_cpu_tensors_is_kcenter_np_and_the_container_follows():
    from eoe_amd import coreset
    x = coreset_util.exact_features(50, 7, 3)
    x[17, 2] = np.nan
    want = coreset.kcenter_np(x, 6, 4)
    for arg in (x, torch.from_numpy(x)):
        cs = coreset.kcenter(arg, 6, 4)
        assert cs.idx.dtype == torch.int64 and cs.assign.dtype == torch.int64 and cs.radius.dtype == cs.d2min.dtype == torch.float32
        assert np.array_equal(cs.idx.numpy(), want[0]) and np.array_equal(cs.assign.numpy(), want[2]) and cs.nonfinite == 1
        assert np.array_equal(cs.radius.numpy(), want[1].astype(np.float32))
        assert np.array_equal(cs.d2min.numpy(), want[3].astype(np.float32), equal_nan=True)
        assert (cs.m, cs.n) == (6, 50) and cs.cover() == math.sqrt(np.nanmax(want[3]))
        assert cs.sizes().tolist() == np.bincount(want[2][want[2] >= 0], minlength=6).tolist() and int(cs.sizes().sum()) == 49
    ids = np.arange(50) * 3 + 100
    d = cs.as_dict(ref_ids=ids)
    assert d["centres"] == ids[want[0]].tolist() and d["radius"] == [float(math.sqrt(r)) for r in want[1][1:]]
    assert (d["m"], d["n"], d["nonfinite"], d["cover"], d["sizes"]) == (6, 50, 1, cs.cover(), cs.sizes().tolist())
    assert cs.as_dict()["centres"] == want[0].tolist()
    with pytest.raises(ValueError, match="ref_ids"):
        cs.as_dict(ref_ids=ids[:10])
    import json
    json.dumps(d)
    short = coreset.kcenter(np.array([[0.], [np.nan], [2.]], np.float32), 3)             # a tail without centres is left out
    assert short.idx.tolist() == [0, 2, -1] and short.as_dict()["centres"] == [0, 2] and short.as_dict()["sizes"] == [1, 1]


def test_the_trainer_refuses_a_coreset_without_neighbors_and_values_outside_the_ranges():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    kw = dict(dataset=None, epochs=1, batch_size=4, classes=["a"], device="cpu")
    with pytest.raises(ValueError, match="neighbors must be at least 1"):
        TRAINER["hsc"](CNN32(), extremes=3, knn_coreset=8, **kw)
    with pytest.raises(ValueError, match="neighbors must be at least 1"):
        TRAINER["hsc"](CNN32(), knn_coreset=0.5, **kw)
    for bad in (True, False, -1, 1.0, 1.5, -0.25, "4", None):
        with pytest.raises(ValueError, match="knn_coreset must be"):
            TRAINER["hsc"](CNN32(), extremes=3, neighbors=4, knn_coreset=bad, **kw)
    a = TRAINER["hsc"](CNN32(), extremes=3, neighbors=4, knn_coreset=100, **kw)
    b = TRAINER["hsc"](CNN32(), extremes=3, neighbors=4, knn_coreset=0.1, **kw)
    off = TRAINER["hsc"](CNN32(), extremes=3, neighbors=4, **kw)
    assert (a.knn_coreset, b.knn_coreset, off.knn_coreset) == (100, 0.1, 0) and a.coresets == {} and off.coresets == {}
