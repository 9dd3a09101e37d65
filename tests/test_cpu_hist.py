"""CPU tier: the score histograms of `eoe_amd.metrics` on host arrays against the restatement of TensorBoard's `make_histogram` in
tests/hist_util.py (and that restatement against `make_histogram` itself where TensorBoard is installed), the refusals, the C ABI's
argument checks, the logger's JSON file and the trainer's switch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hist_util
from eoe_amd import metrics


def test_default_edges_are_tensorboards_table():
    e = hist_util.default_edges()
    assert e.size == 1549 and e[774] == 0.0 and e[775] == 1e-12 and e[773] == -1e-12 and e[-1] < 1e20 <= e[-1] * 1.1
    assert np.array_equal(e, -e[::-1]) and (np.diff(e) > 0).all()
    assert np.array_equal(metrics.default_edges(), e)
    assert metrics.default_edges() is metrics.default_edges()


@pytest.mark.parametrize("n", hist_util.NS)
def test_restatement_equals_make_histogram(n):
    summary = pytest.importorskip("torch.utils.tensorboard.summary")
    edges = hist_util.default_edges()
    for how in hist_util.LABELLINGS + (None,):
        s = hist_util.scores(n)
        groups = [s] if how is None else [s[hist_util.labels(n, how) == k] for k in (0, 1)]
        for v in groups:
            if v.size == 0:
                continue
            want = hist_util.restate(v)
            proto = summary.make_histogram(v.astype(np.float64), edges)              # float64 in: the same sums, field by field
            assert (proto.min, proto.max, int(proto.num), proto.sum, proto.sum_squares) == \
                   (want["min"], want["max"], want["num"], want["sum"], want["sum_squares"])
            assert list(proto.bucket_limit) == want["bucket_limit"] and [int(c) for c in proto.bucket] == want["bucket"]
            proto32 = summary.make_histogram(v, edges)                             # float32 in: compared as float64 all the same
            assert list(proto32.bucket_limit) == want["bucket_limit"] and [int(c) for c in proto32.bucket] == want["bucket"]
            assert (proto32.min, proto32.max, int(proto32.num)) == (want["min"], want["max"], want["num"])


@pytest.mark.parametrize("n,how", hist_util.CASES)
def test_host_histograms_equal_the_restatement(n, how):
    s, y = hist_util.scores(n), hist_util.labels(n, how)
    want = hist_util.expected(n, how)
    got = metrics.score_histograms(y, s)
    for k in (0, 1):
        hist_util.check(got[k], s[y == k], want[k], f"n={n} {how} label {k}")
        one = metrics.score_histogram(s, y, k)
        assert (one is None and got[k] is None) or one == got[k]
    if how == "zeros":                                                              # the unlabelled form, tensors and float64 input
        import torch
        whole = hist_util.expected(n, None)
        hist_util.check(metrics.score_histogram(s), s, whole, f"n={n} unlabelled")
        assert metrics.score_histogram(torch.from_numpy(s.copy())) == metrics.score_histogram(s)
        assert metrics.score_histogram(s.astype(np.float64)) == metrics.score_histogram(s)
        assert metrics.score_histograms(torch.from_numpy(y.copy()), torch.from_numpy(s.copy()))[0] == got[0]


@pytest.mark.parametrize("key", ("three", "cap"))
def test_host_histograms_with_explicit_edges(key):
    edges = hist_util.explicit_edges(key)
    n = 257
    s, y = hist_util.scores(n), hist_util.labels(n, "mixed_unlabelled")
    got = metrics.score_histograms(y, s, bins=edges)
    for k in (0, 1):
        hist_util.check(got[k], s[y == k], hist_util.expected(n, "mixed_unlabelled", key)[k], f"{key} label {k}")
    hist_util.check(metrics.score_histogram(s, bins=edges.tolist()), s, hist_util.expected(n, None, key), key)


def test_trimming_by_hand():
    h = metrics.score_histogram(np.array([0.0, -0.0, 1e-12, 5e-13]))               # an edge belongs to the bin on its right
    e = hist_util.default_edges()
    assert h.bucket == [0, 3, 1] and h.bucket_limit == [0.0, 1e-12, e[776]]        # the real (empty) bin [-1e-12, 0) in front
    assert (h.num, h.min, h.max) == (4, 0.0, 1e-12)
    h = metrics.score_histogram(np.array([-1.0, 1.0, 2.0]), bins=[-1.0, 0.0, 1.0])  # bin 0 occupied: a made-up empty bin in front
    assert h.bucket == [0, 1, 1] and h.bucket_limit == [-1.0, 0.0, 1.0] and (h.num, h.max, h.sum, h.sum_squares) == (3, 2.0, 2.0, 6.0)
    h = metrics.score_histogram(np.array([1e21, -1e21], np.float32))                # TensorBoard raises here; no bucket, the scalars stay
    assert h.bucket == [] and h.bucket_limit == [] and h.num == 2 and h.min == -h.max == float(np.float32(-1e21))
    assert set(h.as_dict()) == set(hist_util.FIELDS) == set(metrics.Histogram.FIELDS)


def test_refusals():
    s = np.array([0.1, 0.4, 0.3, 0.2], np.float32)
    y = np.array([0, 1, 1, 0])
    for bad in (np.nan, np.inf, -np.inf):
        b = s.copy()
        b[1] = bad
        with pytest.raises(ValueError):
            metrics.score_histogram(b)
        with pytest.raises(ValueError):
            metrics.score_histograms(y, b)
    with pytest.raises(ValueError):
        metrics.score_histograms(y[:3], s)
    with pytest.raises(ValueError):
        metrics.score_histogram(s, y[:3], 0)
    with pytest.raises(ValueError):
        metrics.score_histogram(np.zeros(0, np.float32))
    for bins in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0], [0.0, np.nan, 1.0], [0.0, np.inf], "doane"):
        with pytest.raises(ValueError):
            metrics.score_histogram(s, bins=bins)
    assert metrics.HIST_MAX_EDGES == 4001
    metrics.score_histogram(s, bins=np.arange(metrics.HIST_MAX_EDGES, dtype=np.float64) - 5.0)
    with pytest.raises(ValueError):
        metrics.score_histogram(s, bins=np.arange(metrics.HIST_MAX_EDGES + 1, dtype=np.float64))
    with pytest.raises(ValueError):
        metrics.score_histogram(s, y)                                              # labels without a label
    with pytest.raises(ValueError):
        metrics.score_histogram(s, y, 2)
    # a label nobody carries
    assert metrics.score_histograms(np.zeros(4, np.int64), s)[1] is None and metrics.score_histograms(np.ones(4, np.int64), s)[0] is None
    assert metrics.score_histograms(np.full(4, -1), s) == (None, None)
    assert metrics.score_histogram(s, np.zeros(4, np.int64), 1) is None


def test_c_abi_declares_the_histogram_entry_points_and_rejects_bad_arguments():
    """additive: two new symbols; bad arguments are error code 1 and a message before any launch (no GPU here)"""
    from eoe_amd import _lib
    lib = _lib.lib
    assert {"eoe_score_hist", "eoe_score_hist_scratch_bytes"} <= set(_lib.header_symbols())
    assert lib.eoe_score_hist_scratch_bytes(0) == 0 and lib.eoe_score_hist_scratch_bytes(-5) == 0
    for n in (1, 256, 257, 90001, (1 << 31) - 1):
        b = lib.eoe_score_hist_scratch_bytes(n)
        assert 80 <= b <= 256 * 80 and b % 80 == 0
    assert lib.eoe_score_hist_scratch_bytes(256) == 80 and lib.eoe_score_hist_scratch_bytes(257) == 160
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    edges = (C.c_double * 3)(-1.0, 0.0, 1.0)
    e = C.addressof(edges)
    good = [p, p, 8, e, p, 3, p, p, p, None]
    for i in (0, 3, 4, 6, 7, 8):                                                   # every pointer but the labels and the stream
        args = list(good)
        args[i] = None
        assert lib.eoe_score_hist(*args) == 1, i
        assert b"score_hist" in lib.eoe_last_error()
    for n in (0, -1):
        args = list(good)
        args[2] = n
        assert lib.eoe_score_hist(*args) == 1 and b"n must be" in lib.eoe_last_error()
    many = (C.c_double * 4002)(*range(4002))
    for E, tab in ((1, e), (0, e), (4002, C.addressof(many))):
        args = list(good)
        args[3], args[5] = tab, E
        assert lib.eoe_score_hist(*args) == 1 and b"E must be" in lib.eoe_last_error()
    for bad in ((0.0, 0.0, 1.0), (0.0, 2.0, 1.0), (0.0, float("nan"), 1.0), (0.0, 1.0, float("inf"))):
        tab = (C.c_double * 3)(*bad)
        args = list(good)
        args[3] = C.addressof(tab)
        assert lib.eoe_score_hist(*args) == 1 and b"ascending" in lib.eoe_last_error()


def test_logger_keeps_histograms_and_round_trips_them_through_json(tmp_path):
    from eoe_amd.training.ad_trainer import JsonLogger
    a = metrics.score_histogram(hist_util.scores(257))
    b = metrics.score_histogram(hist_util.scores(255))
    log = JsonLogger(str(tmp_path / "log"))
    log.add_histogram("Training: CLS0 SEED0 anomaly_scores normal", a, 0)
    log.add_histogram("Training: CLS0 SEED0 anomaly_scores normal", b, 1)
    log.add_histogram("Eval: (SD0) anomaly_scores cls0 nominal", a, 0)
    assert log.histograms["Training: CLS0 SEED0 anomaly_scores normal"] == {0: a, 1: b}
    with open(os.path.join(str(tmp_path / "log"), "histograms.json")) as f:
        j = json.load(f)
    assert set(j) == {"Training: CLS0 SEED0 anomaly_scores normal", "Eval: (SD0) anomaly_scores cls0 nominal"}
    assert set(j["Training: CLS0 SEED0 anomaly_scores normal"]) == {"0", "1"}
    for tag, step, h in (("Training: CLS0 SEED0 anomaly_scores normal", "0", a), ("Training: CLS0 SEED0 anomaly_scores normal", "1", b),
                         ("Eval: (SD0) anomaly_scores cls0 nominal", "0", a)):
        assert set(j[tag][step]) == set(hist_util.FIELDS)
        assert metrics.Histogram(**j[tag][step]) == h                             # floats survive JSON bit for bit
    quiet = JsonLogger(None)                                                       # no directory: kept in memory, nothing written
    quiet.add_histogram("t", a, 3)
    assert quiet.histograms == {"t": {3: a}}


def test_trainer_takes_the_switch():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    on = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu", histograms=True)
    off = TRAINER["hsc"](CNN32(bias=True), dataset=None, device="cpu")
    assert on.with_histograms is True and off.with_histograms is False and on.histograms == {} and off.histograms == {}
