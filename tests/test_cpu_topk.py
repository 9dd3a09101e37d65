"""CPU tier: the host path of `eoe_amd.metrics.score_extremes` against a ranking written out by hand and against tests/topk_util.py,
the `indices=` mapping, `Extremes.as_dict`, the refusals, the C ABI's argument checks (no GPU here: nothing is launched) and the
trainer's switch."""
import ctypes as C
import json

import numpy as np
import pytest

import topk_util
from eoe_amd import metrics

# twelve scores: ties (0.5 three times, 2.0 twice), a -0.0 / 0.0 pair in each group's reach, a label -1 holding the largest value
S12 = np.array([0.5, 2.0, -0.0, 0.5, 9.0, 0.0, -1.0, 2.0, 0.5, -0.0, 0.0, -3.0], dtype=np.float32)
Y12 = np.array([0,   1,   0,    0,   -1,  0,   1,    1,   0,   1,    1,   0], dtype=np.int64)
# group 0: positions 0, 2, 3, 5, 8, 11 = 0.5, -0.0, 0.5, 0.0, 0.5, -3.0;  group 1: positions 1, 6, 7, 9, 10 = 2.0, -1.0, 2.0, -0.0, 0.0
MOST_0, LEAST_0 = [0, 3, 8, 2, 5, 11], [11, 2, 5, 0, 3, 8]
MOST_1, LEAST_1 = [1, 7, 9, 10, 6], [6, 9, 10, 1, 7]


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32).tolist()


def test_host_path_equals_the_ranking_written_out_by_hand():
    ex = metrics.score_extremes(Y12, S12, k=4)
    assert isinstance(ex, metrics.Extremes) and ex.num == (6, 5)
    assert ex.most[0][0].tolist() == MOST_0[:4] and ex.least[0][0].tolist() == LEAST_0[:4]
    assert ex.most[1][0].tolist() == MOST_1[:4] and ex.least[1][0].tolist() == LEAST_1[:4]
    for pair in ex.most + ex.least:                                                # the selected elements' own bits: -0.0 stays -0.0
        assert pair[0].dtype == np.int64 and pair[1].dtype == np.float32
        assert _bits(pair[1]) == _bits(S12[pair[0]])
    assert _bits(ex.most[0][1])[3] == _bits([-0.0])[0] and _bits(ex.least[1][1])[1:3] == _bits([-0.0, 0.0])
    topk_util.check_extremes(ex, S12, topk_util.reference(S12, Y12, 4), 4, "hand case")
    # tensors and float64 input take the same path
    import torch
    assert metrics.score_extremes(torch.from_numpy(Y12), torch.from_numpy(S12), k=4) == ex
    assert metrics.score_extremes(Y12.tolist(), S12.astype(np.float64), k=4) == ex
    # no labels: everything in group 0, the label -1 element included
    whole = metrics.score_extremes(None, S12, k=3)
    assert whole.num == (12, 0) and whole.most[0][0].tolist() == [4, 1, 7] and whole.least[0][0].tolist() == [11, 6, 2]
    assert whole.most[1][0].size == 0 and whole.least[1][1].size == 0


def test_k_larger_than_a_group_returns_the_whole_group_ranked():
    ex = metrics.score_extremes(Y12, S12, k=6)                                     # group 0 exactly, group 1 one short
    assert ex.most[0][0].tolist() == MOST_0 and ex.least[0][0].tolist() == LEAST_0
    assert ex.most[1][0].tolist() == MOST_1 and ex.least[1][0].tolist() == LEAST_1
    big = metrics.score_extremes(Y12, S12, k=1024)
    assert big == ex
    assert metrics.score_extremes(Y12, S12) == ex                                  # the default k = 20
    one = metrics.score_extremes(np.zeros(12, np.int64), S12, k=2)                  # a label nobody carries
    assert one.num == (12, 0) and one.most[1][0].size == 0 and one.least[1][0].size == 0
    none = metrics.score_extremes(np.full(12, -1), S12, k=2)
    assert none.num == (0, 0) and all(p[0].size == 0 for p in none.most + none.least)


@pytest.mark.parametrize("kind", topk_util.KINDS)
def test_host_path_equals_the_reference_on_the_device_cases(kind):
    for n in (1, 2, 257, 4097):
        s = topk_util.scores(n, kind)
        for how in topk_util.LAYOUTS:
            y = topk_util.labels(n, how)
            for k in (1, 20):
                topk_util.check_extremes(metrics.score_extremes(y, s, k), s, topk_util.reference(s, y, k), k, f"{kind} n={n} {how} k={k}")


def test_indices_map_the_returned_positions_only():
    remap = np.arange(12, dtype=np.int64)[::-1] * 10 + 3
    ex = metrics.score_extremes(Y12, S12, k=4, indices=remap)
    plain = metrics.score_extremes(Y12, S12, k=4)
    for a, b in zip(ex.most + ex.least, plain.most + plain.least):
        assert a[0].tolist() == remap[b[0]].tolist() and _bits(a[1]) == _bits(b[1])   # ties still in ascending POSITION
    assert ex.most[0][0].tolist() == [113, 83, 33, 93]
    import torch
    assert metrics.score_extremes(Y12, S12, k=4, indices=torch.from_numpy(remap.copy())) == ex
    with pytest.raises(ValueError):
        metrics.score_extremes(Y12, S12, k=4, indices=remap[:5])


def test_as_dict_layout_survives_json():
    d = metrics.score_extremes(Y12, S12, k=2).as_dict()
    assert list(d) == ["nominal", "anomalous"] and all(list(v) == ["most", "least", "num"] for v in d.values())
    assert d["nominal"] == {"most": [[0, 0.5], [3, 0.5]], "least": [[11, -3.0], [2, -0.0]], "num": 6}
    assert d["anomalous"] == {"most": [[1, 2.0], [7, 2.0]], "least": [[6, -1.0], [9, -0.0]], "num": 5}
    assert all(type(i) is int and type(v) is float for grp in d.values() for lst in (grp["most"], grp["least"]) for i, v in lst)
    assert json.loads(json.dumps(d)) == d
    empty = metrics.score_extremes(np.zeros(12, np.int64), S12, k=2).as_dict()["anomalous"]
    assert empty == {"most": [], "least": [], "num": 0}


def test_refusals():
    for bad in (np.nan, np.inf, -np.inf):
        b = S12.copy()
        b[3] = bad                                                                  # a member of group 0
        with pytest.raises(ValueError):
            metrics.score_extremes(Y12, b)
        with pytest.raises(ValueError):
            metrics.score_extremes(None, b)
        b = S12.copy()
        b[4] = bad                                                                  # label -1: in neither group, ignored
        assert metrics.score_extremes(Y12, b, k=6) == metrics.score_extremes(Y12, S12, k=6)
        with pytest.raises(ValueError):
            metrics.score_extremes(None, b)                                        # ... but a member when there are no labels
    assert metrics.EXTREMES_MAX_K == 1024 and metrics.EXTREMES_MAX_N == 1 << 20
    for k in (0, -1, 1025, 2.5, None, True):
        with pytest.raises(ValueError):
            metrics.score_extremes(Y12, S12, k=k)
    metrics.score_extremes(Y12, S12, k=1)
    metrics.score_extremes(Y12, S12, k=np.int64(1024))
    with pytest.raises(ValueError):
        metrics.score_extremes(Y12[:5], S12)
    with pytest.raises(ValueError):
        metrics.score_extremes(np.zeros(0, np.int64), np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        metrics.score_extremes(None, np.zeros(0, np.float32))


def test_c_abi_declares_the_extremes_entry_points_and_rejects_bad_arguments():
    """additive: two new symbols; bad arguments are error code 1 and a message before any launch (no GPU here)"""
    from eoe_amd import _lib
    lib = _lib.lib
    new = {"eoe_score_extremes", "eoe_score_extremes_scratch_bytes"}
    assert new <= set(_lib.header_symbols()) and new <= set(_lib.SIGNATURES)
    assert all(getattr(lib, name) is not None for name in new)
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5
    sb = lib.eoe_score_extremes_scratch_bytes
    for n, k in ((0, 20), (-3, 20), ((1 << 20) + 1, 20), (100, 0), (100, -1), (100, 1025), (0, 0)):
        assert sb(n, k) == 0, (n, k)
    for n, k in ((1, 1), (100, 20), (1 << 20, 1024), (1, 1024), (1 << 20, 1)):
        assert sb(n, k) >= 4 * 1024 * 8 and sb(n, k) % 16 == 0, (n, k)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p += -p % 16                                                                   # the scratch must be 16-byte aligned
    # eoe_score_extremes(scores, labels, n, k, out_idx, out_val, out_counts, scratch, stream)
    good = [p, None, 8, 2, p, p, p, p, None]
    for i in (0, 4, 5, 6, 7):                                                       # every pointer but the labels and the stream
        args = list(good)
        args[i] = None
        assert lib.eoe_score_extremes(*args) == 1, i
        assert b"score_extremes" in lib.eoe_last_error() and b"null" in lib.eoe_last_error()
    for n in (0, -1, (1 << 20) + 1):
        args = list(good)
        args[2] = n
        assert lib.eoe_score_extremes(*args) == 1 and b"n must be" in lib.eoe_last_error()
    for k in (0, -1, 1025):
        args = list(good)
        args[3] = k
        assert lib.eoe_score_extremes(*args) == 1 and b"k must be" in lib.eoe_last_error()
    args = list(good)
    args[7] = p + 4
    assert lib.eoe_score_extremes(*args) == 1 and b"aligned" in lib.eoe_last_error()


def test_trainer_takes_the_option():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    on = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", extremes=5)
    off = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu")
    assert on.n_extremes == 5 and off.n_extremes == 0 and on.extremes == {} and off.extremes == {}
    for bad in (-1, 1025, 2.5, True):
        with pytest.raises(ValueError):
            TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", extremes=bad)

