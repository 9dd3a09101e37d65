"""CPU tier: the host path of `eoe_amd.metrics.delong` against DeLong's estimator written from its definition (tests/delong_util.py) --
the integer table exactly, the floats to the brute force's own rounding --, the worked example as rational numbers, the edge
definitions, the refusals, the C ABI's argument checks (no GPU here: nothing is launched) and the trainer's option parsing."""
import ctypes as C
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import delong_util as du
from eoe_amd import metrics


def test_the_worked_example_as_rational_numbers():
    y = np.array([1, 0, 1, 0, 0])
    s = np.array([0.8, 0.7, 0.6, 0.5, 0.6], np.float32)
    t = metrics.delong(y, s)
    c = t.counts
    assert (t.n_pos, t.n_neg) == (2, 3) and c["T_pos"].tolist() == [9] and c["T_neg"].tolist() == [9]
    assert c["A"].tolist() == [6 * 6 + 3 * 3] and c["B"].tolist() == [2 * 2 + 4 * 4 + 3 * 3]
    m, n0, T, A, B = 2, 3, 9, 45, 29
    s10, s01 = Fraction(m * A - T * T, m * (m - 1) * 4 * n0 * n0), Fraction(n0 * B - T * T, n0 * (n0 - 1) * 4 * m * m)
    assert s10 == Fraction(1, 8) and s01 == Fraction(1, 16)
    assert t.cov_fraction(0, 0) == s10 / m + s01 / n0 == Fraction(1, 12)
    assert t.auc.tolist() == [0.75] and t.var.tolist() == [1 / 12] and t.cov.tolist() == [[1 / 12]] and t.se.tolist() == [math.sqrt(1 / 12)]
    du.assert_tables_equal(du.table_of(t), du.brute_force(y, s.reshape(1, -1)), "worked example")


@pytest.mark.parametrize("n", du.SIZES)
def test_host_table_equals_the_brute_force_table_and_the_floats_agree(n):
    seen_none = checked = 0
    for (nn, share, kind, K) in du.grid():
        if nn != n:
            continue
        what = (n, share, kind, K)
        y, s, ref = du.case(n, share, kind, K)
        t = metrics.delong(y, s)
        if ref["m"] == 0 or ref["n0"] == 0:
            assert t is None, what
            seen_none += 1
            continue
        checked += 1
        du.assert_tables_equal(du.table_of(t), ref, what)
        du.assert_floats_agree(t, ref, what)
        keep = y >= 0
        for k in range(K if kind != "inf" else 0):                     # bit for bit (`roc_auc` ranks finite scores only)
            assert t.auc[k] == metrics.roc_auc(y[keep], s[k][keep]), what
        if K >= 2:                                                     # the last column repeats the first
            assert t.compare(0, K - 1) == (0.0, 0.0, 1.0) and t.compare(K - 1, 0) == (0.0, 0.0, 1.0), what
            assert t.pvalues()[0, K - 1] == 1.0 and np.array_equal(t.cov[0], t.cov[K - 1], equal_nan=True), what
        assert np.array_equal(np.diagonal(t.pvalues()), np.ones(K)) or not (ref["m"] > 1 and ref["n0"] > 1), what
        json.dumps(t.to_json())
    assert checked + seen_none == 64 and seen_none <= 4                          # a class is lost only where the ignored labels take its one sample


def test_auc_equals_roc_auc_with_ignored_labels_removed():
    y, s, _ = du.case(1000, "tenth", "ignored", 3)
    keep = y >= 0
    t = metrics.delong(y, s)
    assert [metrics.roc_auc(y[keep], s[k][keep]) for k in range(3)] == t.auc.tolist()
    # lists of columns, CPU tensors, float64 and a single row are the same call
    assert metrics.delong(torch.from_numpy(y.copy()), torch.from_numpy(s.copy())).cov.tolist() == t.cov.tolist()
    assert metrics.delong(y, s.astype(np.float64)).counts["A"].tolist() == t.counts["A"].tolist()
    assert metrics.delong(y[keep], [s[0][keep], s[1][keep]]).cov.tolist() == t.cov[:2, :2].tolist()
    assert metrics.delong(y, s[0]).auc.tolist() == t.auc[:1].tolist()


def test_edge_definitions():
    s = np.array([0.1, 0.35, 0.4, 0.8], np.float32)
    assert metrics.delong([0, 0, 0, 0], s) is None and metrics.delong([1, 1, 1, 1], s) is None and metrics.delong([-1, 1, 1, 2], s) is None
    for y in ([1, 0, 0, 0], [0, 1, 1, 1], [1, 0, -1, -1]):             # one positive or one negative: the variance is undefined
        t = metrics.delong(y, s)
        lo, hi = t.ci()
        assert np.isfinite(t.auc).all() and np.isnan(t.cov).all() and np.isnan(t.var).all() and np.isnan(t.se).all()
        assert np.isnan(lo).all() and np.isnan(hi).all() and t.cov_fraction(0, 0) is None
        j = t.to_json()
        assert j["var"] == [None] and j["se"] == [None] and j["cov"] == [[None]] and j["ci_lo"] == [None] and j["ci_hi"] == [None]
        assert json.loads(json.dumps(j, allow_nan=False)) == j
        assert t.compare(0, 0) == (0.0, 0.0, 1.0)                      # a column against itself: identically zero, whatever the variance
        t2 = metrics.delong(y, np.stack([s, s[::-1].copy()]))
        d, z, p = t2.compare(0, 1)
        assert d == t2.auc[0] - t2.auc[1] and math.isnan(z) and math.isnan(p) and math.isnan(t2.pvalues()[0, 1]) and t2.pvalues()[1, 1] == 1.0
    t = metrics.delong([0, 0, 1, 1], s)                                 # perfect separation
    assert t.auc.tolist() == [1.0] and t.var.tolist() == [0.0] and t.se.tolist() == [0.0] and [x.tolist() for x in t.ci()] == [[1.0], [1.0]]
    t = metrics.delong([1, 1, 0, 0], s)                                 # and the other way round
    assert t.auc.tolist() == [0.0] and t.var.tolist() == [0.0] and [x.tolist() for x in t.ci(0.5)] == [[0.0], [0.0]]
    # two models, both perfect in opposite directions: a difference without variance
    t = metrics.delong([0, 0, 1, 1], np.stack([s, -s]))
    assert t.compare(0, 1) == (1.0, math.inf, 0.0) and t.compare(1, 0) == (-1.0, -math.inf, 0.0)
    assert t.pvalues().tolist() == [[1.0, 0.0], [0.0, 1.0]]


def test_ci_compare_and_json():
    y, s, ref = du.case(257, "half", "continuous", 3)
    t = metrics.delong(y, s)
    for level in (0.5, 0.9, 0.95, 0.999):
        du.assert_floats_agree(t, ref, ("levels", level), level)
    lo90, hi90 = t.ci(0.9)
    lo99, hi99 = t.ci(0.99)
    assert np.all(lo99 < lo90) and np.all(hi90 < hi99)
    for bad in (0.0, 1.0, -0.1, 1.5, True, "0.95", None):
        with pytest.raises(ValueError):
            t.ci(bad)
    d, z, p = t.compare(0, 1)
    d2, z2, p2 = t.compare(1, 0)
    assert (d, z, p) == (-d2, -z2, p2) and 0.0 < p <= 1.0 and np.array_equal(t.pvalues(), t.pvalues().T)
    j = t.to_json(0.9)
    assert json.loads(json.dumps(j, allow_nan=False)) == j
    assert j["auc"] == t.auc.tolist() and j["cov"] == t.cov.tolist() and j["n_pos"] == t.n_pos and j["n_neg"] == t.n_neg
    assert j["level"] == 0.9 and j["ci_lo"] == lo90.tolist() and j["ci_hi"] == hi90.tolist() and j["pvalues"] == t.pvalues().tolist()
    assert j["var"] == t.var.tolist() and j["se"] == t.se.tolist()


def test_refusals():
    y = np.array([0, 1, 0, 1, 1, 0])
    s = np.linspace(0.0, 1.0, 6).astype(np.float32)
    bad = s.copy()
    bad[2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        metrics.delong(y, bad)
    with pytest.raises(ValueError, match="NaN"):
        metrics.delong(y, np.stack([s, bad]))
    assert metrics.delong(np.array([0, 1, -1, 1, 1, 0]), bad) is not None          # the NaN belongs to an ignored sample
    with pytest.raises(ValueError, match="columns"):
        metrics.delong(y, np.tile(s, (9, 1)))
    assert metrics.delong(y, np.tile(s, (8, 1))).auc.shape == (8,)
    with pytest.raises(ValueError, match="columns"):
        metrics.delong(y, np.zeros((0, 6), np.float32))
    with pytest.raises(ValueError, match="samples"):
        metrics.delong(np.zeros(metrics.DELONG_MAX_N + 1, np.int8), np.zeros(metrics.DELONG_MAX_N + 1, np.float32))
    with pytest.raises(ValueError, match="samples"):
        metrics.delong([1], [0.5])
    with pytest.raises(ValueError, match="labels"):
        metrics.delong(y[:5], s)
    assert metrics.DELONG_MAX_N == metrics.BREAKDOWN_MAX_N and metrics.DELONG_MAX_COLUMNS == 8
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.delong_device(y, torch.from_numpy(s))
    with pytest.raises(RuntimeError, match="differ"):                  # the invariant T_pos == T_neg is checked
        metrics.AucTest([9], [8], [45], [29], 2, 3)


def test_c_abi_checks_its_arguments_and_launches_nothing():
    from eoe_amd import _lib
    from eoe_amd._lib import lib
    assert lib.eoe_abi_version() == _lib.ABI_VERSION                    # additive: the ABI version does not move
    ok = C.c_void_p(4096)                                              # never dereferenced: every call below is refused first
    call = lambda **kw: lib.eoe_delong_counts(*[kw.get(k, d) for k, d in (("scores", ok), ("labels", ok), ("n", 100), ("K", 2), ("out", ok),   # noqa: E731
                                                                           ("scratch", ok), ("stream", None))])
    for kw, msg in (({"scores": None}, "null scores"), ({"labels": None}, "null labels"), ({"out": None}, "null out"),
                    ({"scratch": None}, "null scratch"), ({"n": 1}, "n must be in [2, 1048576], not 1"),
                    ({"n": (1 << 20) + 1}, "n must be in [2, 1048576]"), ({"K": 0}, "K must be in [1, 8], not 0"),
                    ({"K": 9}, "K must be in [1, 8], not 9"), ({"scores": C.c_void_p(4098)}, "scores must be 4-byte aligned"),
                    ({"labels": C.c_void_p(4100)}, "labels must be 8-byte aligned"), ({"out": C.c_void_p(4100)}, "out must be 8-byte aligned"),
                    ({"scratch": C.c_void_p(4097)}, "scratch must be 4-byte aligned")):
        assert call(**kw) != 0 and msg in lib.eoe_last_error().decode(), kw
    for n, K in ((1, 1), (2, 0), (2, 9), ((1 << 20) + 1, 1)):
        assert lib.eoe_delong_scratch_bytes(n, K) == 0 and lib.eoe_delong_slices(n, K) == 0
    tile = metrics.DELONG_TILE
    for n, K in ((2, 1), (256, 1), (257, 3), (4097, 8), (10_000, 1), (90_000, 5), (1 << 20, 8)):
        blocks = -(-n // tile) + 1
        assert lib.eoe_delong_scratch_bytes(n, K) == -(-4 * n // 256) * 256 + K * blocks * tile * 4
        # about 2 048 workgroups: cdiv(2048, row blocks x K) slices, at least one and at most 64
        assert lib.eoe_delong_slices(n, K) == metrics.delong_slices(n, K) == min(max(-(-2048 // (blocks * K)), 1), 64)
    assert metrics.delong_slices(2, 1) == 64 and metrics.delong_slices(1 << 20, 8) == 1 and metrics.delong_slices(1, 1) == 0
    assert metrics.delong_slices(10_000, 1) * 41 >= 256                # 10 000 scores: 41 row blocks still fill 256 CUs


def test_trainer_option_parsing():
    from eoe_amd.metrics import ROC
    from eoe_amd.training import HSCTrainer
    tr = HSCTrainer(None, dataset=lambda c, s: None)
    assert tr.auc_ci is None and tr.auc_tests == {}
    assert HSCTrainer(None, dataset=lambda c, s: None, auc_ci=0.95).auc_ci == 0.95
    assert HSCTrainer(None, dataset=lambda c, s: None, auc_ci=None).auc_ci is None
    for bad in (0.0, 1.0, 1, -0.5, 95, True, False, "0.95"):
        with pytest.raises(ValueError, match="auc_ci"):
            HSCTrainer(None, dataset=lambda c, s: None, auc_ci=bad)
    roc = ROC(0.5)
    assert not any(hasattr(roc, a) for a in ("ci", "se", "var"))


def test_auc_ci_none_creates_neither_file_nor_attribute_and_a_level_creates_both(tmp_path):
    """`run(train=False)` on host scores (a CPU device and a model that is its own score): the host path of the option end to end"""
    import os
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    y, s, _ = du.case(64, "half", "continuous", 3)

    class Source:
        nominal_label = 0

        def __init__(self, col):
            self.col = col

        def loaders(self, batch_size, num_workers=0, shuffle_test=False):
            x = torch.from_numpy(s[self.col].copy()).reshape(-1, 1)
            return None, [(x[i:i + batch_size], torch.from_numpy(y[i:i + batch_size].copy())) for i in range(0, len(y), batch_size)]

    class Trainer(HSCTrainer):
        def compute_anomaly_score(self, feats, center, **kw):
            return feats.reshape(-1)

    def run(name, **kw):
        logdir = str(tmp_path / name)
        tr = Trainer(torch.nn.Identity(), dataset=lambda c, seed: Source(seed), device="cpu", batch_size=16, logger=JsonLogger(logdir), **kw)
        rocs = []
        eval_cls = tr.eval_cls
        tr.eval_cls = lambda *a, **k: (lambda out: (rocs.append(out[0]), out)[1])(eval_cls(*a, **k))   # keep the ROCs `run` gets
        tr.run(run_seeds=3, train=False)
        assert tr._seed_scores is None                                 # scores are kept only while `run` compares seeds
        eval_cls(torch.nn.Identity(), Source(0), 0, "0", 0)            # a direct call keeps nothing
        assert tr._seed_scores is None
        return tr, rocs, logdir

    tr, rocs, logdir = run("on", auc_ci=0.9)
    off, rocs_off, logdir_off = run("off")
    added = {f"eval_cls0_it{i}_auc_ci.json" for i in range(3)} | {"eval_cls0_auc_compare.json"}
    assert set(os.listdir(logdir)) - set(os.listdir(logdir_off)) == added and not set(os.listdir(logdir_off)) & added
    assert off.auc_tests == {} and not any(hasattr(r, a) for r in rocs_off for a in ("ci", "se", "var"))
    want = metrics.delong(y, s)
    assert tr.auc_tests[0].cov.tolist() == want.cov.tolist() and tr.auc_tests[0].auc.tolist() == want.auc.tolist()
    for i, r in enumerate(rocs):
        assert r.auc == rocs_off[i].auc == want.auc[i] and r.var == want.var[i] and r.se == want.se[i]
        assert r.ci == (want.ci(0.9)[0][i], want.ci(0.9)[1][i]) and r.ci[0] < r.auc < r.ci[1]
        with open(os.path.join(logdir, f"eval_cls0_it{i}_auc_ci.json")) as f:
            assert json.load(f) == metrics.delong(y, s[i]).to_json(0.9)
    with open(os.path.join(logdir, "eval_cls0_auc_compare.json")) as f:
        assert json.load(f) == {"seeds": [0, 1, 2], **want.to_json(0.9)}


def test_a_nan_test_score_costs_the_interval_not_the_run(tmp_path):
    import os
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    y = np.array([0, 1, 0, 1, 1, 0])
    s = np.array([0.1, 0.9, 0.2, np.nan, 0.7, 0.3], np.float32)

    class Source:
        nominal_label = 0

        def loaders(self, batch_size, num_workers=0, shuffle_test=False):
            return None, [(torch.from_numpy(s.copy()).reshape(-1, 1), torch.from_numpy(y.copy()))]

    class Trainer(HSCTrainer):
        def compute_anomaly_score(self, feats, center, **kw):
            return feats.reshape(-1)

    lines = []
    logger = JsonLogger(str(tmp_path / "nan"))
    logger.logtxt = lines.append
    tr = Trainer(torch.nn.Identity(), dataset=lambda c, seed: Source(), device="cpu", logger=logger, auc_ci=0.95)
    tr.run(run_seeds=2, train=False)
    assert tr.auc_tests == {} and not any("auc_ci" in f or "auc_compare" in f for f in os.listdir(str(tmp_path / "nan")))
    assert sum("no confidence interval" in x for x in lines) == 2
