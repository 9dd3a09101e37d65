"""CPU tier of the bootstrap (`metrics.bootstrap`): the generator's known answers, the draws, the NumPy statement against a plain
Python double loop, the container, the host route's standard error against DeLong's, the C ABI's argument checks and the trainer's
option on host scores."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import bootstrap_util as bu
from eoe_amd import metrics


def test_the_feature_is_there():
    import eoe_amd
    assert callable(metrics.bootstrap) and callable(metrics.bootstrap_np) and callable(metrics.bootstrap_device)
    assert eoe_amd.bootstrap is metrics.bootstrap and eoe_amd.Bootstrap is metrics.Bootstrap
    assert metrics.BOOTSTRAP_CHUNK == 16384 and metrics.BOOTSTRAP_MAX_REPLICATES == 65536


def test_philox_known_answers():
    hexes = lambda a: " ".join(f"{int(x):08x}" for x in a)                                          # noqa: E731
    assert hexes(metrics.philox4x32([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(metrics.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(metrics.philox4x32([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over leading axes: the rows are the single calls
    ctr = np.array([[0, 0, 0, 0], [5, 7, 1, 0], [0xFFFFFFFF] * 4], np.uint64)
    out = metrics.philox4x32(ctr, [3, 9])
    assert out.shape == (3, 4) and out.dtype == np.uint32
    for row, c in zip(out, ctr):
        assert np.array_equal(row, metrics.philox4x32(c, [3, 9]))


def test_multiplicities():
    y = np.array([1, 0, -1, 0, 1, 2, 0, 1, 0, 0, 0, 1, 1], np.int64)
    m, n0 = int((y == 1).sum()), int((y == 0).sum())
    seen = []
    for b, seed in ((0, 0), (1, 0), (2, 0), (0, 1), (0, 1 << 32), (3, (1 << 32) + 12345), (65535, (1 << 64) - 1)):
        c = metrics.bootstrap_multiplicities_np(y, b, seed)
        assert c.dtype == np.int32 and c.shape == y.shape and (c >= 0).all()
        assert c[y == 1].sum() == m and c[y == 0].sum() == n0 and (c[(y != 0) & (y != 1)] == 0).all()
        assert np.array_equal(c, metrics.bootstrap_multiplicities_np(y, b, seed))
        seen.append(c.tolist())
    # replicates differ from each other, and seed differs from seed + 2^32: the high word is the second key word
    big = np.tile(y, 40)
    draws = {(b, seed): metrics.bootstrap_multiplicities_np(big, b, seed).tolist() for b in (0, 1, 2) for seed in (0, 1 << 32)}
    assert len({tuple(v) for v in draws.values()}) == 6
    # the draws of the statement, written out: word q of call j selects position (w * size) >> 32
    pos = np.flatnonzero(y == 1)
    want = np.zeros(y.size, np.int64)
    for j in range((m + 3) // 4):
        w = metrics.philox4x32([j, 2, 1, 0], [7, 0])
        for q in range(4):
            if 4 * j + q < m:
                want[pos[(int(w[q]) * m) >> 32]] += 1
    assert np.array_equal(metrics.bootstrap_multiplicities_np(y, 2, 7)[y == 1], want[y == 1])
    assert metrics.bootstrap_multiplicities_np(np.array([2, -1, 3]), 0, 0).tolist() == [0, 0, 0]
    for bad in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            metrics.bootstrap_multiplicities_np(y, 0, bad)


CASES = [(12, "half", "continuous"), (12, "half", "four"), (11, "half", "tied"), (12, "one_pos", "continuous"), (12, "one_neg", "four"),
         (12, "half", "special"), (12, "mixed", "four"), (12, "mixed", "special"), (2, "half", "continuous"), (3, "half", "four"),
         (9, "mixed", "continuous")]


@pytest.mark.parametrize("n,split,kind", CASES)
@pytest.mark.parametrize("tpr", [0.95, 1.0, 0.5])
def test_numpy_statement_against_a_double_loop(n, split, kind, tpr):
    K, B, seed = 2, 6, (1 << 32) + 5
    y, s = bu.case(n, split, kind, n, K)
    u2, fps, ap, m, n0 = metrics.bootstrap_np(y, s, B, seed, tpr)
    wu2, wfps, wap, wm, wn0 = bu.brute(y, s, B, seed, tpr)
    assert (m, n0) == (wm, wn0) and u2.shape == fps.shape == ap.shape == (K, B + 1) and u2.dtype == fps.dtype == np.int64
    assert u2.tolist() == wu2 and fps.tolist() == wfps
    assert np.abs(ap - np.array(wap)).max() <= bu.ap_bound(n)
    # the same scores as float64 are the same problem
    u2d, fpsd, apd, _, _ = metrics.bootstrap_np(y, s.astype(np.float64), B, seed, tpr)
    assert np.array_equal(u2d, u2) and np.array_equal(fpsd, fps) and np.array_equal(apd, ap)
    if m == 1 and n0 == 1:                                             # every replicate is the sample itself
        assert (u2 == u2[:, -1:]).all() and (fps == fps[:, -1:]).all() and (ap == ap[:, -1:]).all()


def test_one_positive_and_one_negative_repeat_the_point_estimate():
    y = np.array([2, 1, -1, 0], np.int64)
    for s in ([0.0, 0.3, 9.0, 0.7], [0.0, 0.7, 9.0, 0.3], [0.0, -0.0, 9.0, 0.0], [0.0, math.inf, 1.0, -math.inf]):
        b = metrics.bootstrap(y, np.array(s, np.float32), replicates=9, seed=3)
        for stat in metrics.BOOTSTRAP_STATS:
            reps = getattr(b, stat + "_reps")
            assert reps.shape == (1, 9) and (reps == getattr(b, stat)[0]).all() and b.se(stat)[0] == 0.0
    assert metrics.bootstrap(y, np.array([0.0, -0.0, 9.0, 0.0], np.float32), 3).auc[0] == 0.5


def test_full_sample_column_is_the_point_estimate():
    y, s = bu.case(300, "mixed", "four", 4, K=3)
    b = metrics.bootstrap(y, s, replicates=20, seed=1)
    used = (y == 0) | (y == 1)
    for k in range(3):
        assert b.auc[k] == pytest.approx(metrics.roc_auc(y[used], s[k][used]), abs=1e-15)
        assert b.ap[k] == pytest.approx(metrics.average_precision(y[used], s[k][used]), abs=bu.ap_bound(300))
    assert b.n_pos == int((y == 1).sum()) and b.n_neg == int((y == 0).sum()) and b.replicates == 20 and b.seed == 1


def test_container():
    y, s = bu.case(200, "half", "continuous", 9, K=3)
    b = metrics.bootstrap(y, s, replicates=101, seed=2, tpr=0.9)
    assert b.tpr == 0.9 and b.auc_reps.shape == b.ap_reps.shape == b.fpr_reps.shape == (3, 101)
    assert np.array_equal(b.auc_reps, b.counts["u2"][:, :-1] / (2 * b.n_pos * b.n_neg))
    assert np.array_equal(b.fpr_reps, b.counts["fps"][:, :-1] / b.n_neg)
    pairs = metrics._pairs(3)
    for stat in metrics.BOOTSTRAP_STATS:
        reps = getattr(b, stat + "_reps")
        lo, hi = b.ci(0.9, stat)
        assert lo.shape == hi.shape == (3,) and (lo <= hi).all()
        assert np.array_equal(lo, np.quantile(reps, (1 - 0.9) / 2, axis=1)) and np.array_equal(hi, np.quantile(reps, (1 + 0.9) / 2, axis=1))
        wide_lo, wide_hi = b.ci(0.99, stat)
        assert (wide_lo <= lo).all() and (hi <= wide_hi).all()
        assert np.allclose(b.se(stat), reps.std(axis=1, ddof=1), rtol=0, atol=0)
        dlo, dhi = b.diff_ci(0.9, stat)
        p = b.diff_p(stat)
        assert dlo.shape == dhi.shape == p.shape == (len(pairs),) and (dlo <= dhi).all() and ((0 < p) & (p <= 1)).all()
        for i, (k, l) in enumerate(pairs):
            if k == l:
                assert dlo[i] == 0.0 and dhi[i] == 0.0 and p[i] == 1.0
            else:
                d = reps[k] - reps[l]
                assert dlo[i] == np.quantile(d, (1 - 0.9) / 2) and dhi[i] == np.quantile(d, (1 + 0.9) / 2)
                assert p[i] == min(1.0, 2 * min((d <= 0).sum() + 1, (d >= 0).sum() + 1) / 102)
    js = b.to_json(0.9)
    assert json.loads(json.dumps(js, allow_nan=False)) == js
    assert set(js) == {"n_pos", "n_neg", "replicates", "seed", "tpr", "level", "pairs", "auc", "ap", "fpr"}
    assert set(js["ap"]) == {"value", "se", "ci_lo", "ci_hi", "diff_ci_lo", "diff_ci_hi", "diff_p"} and js["pairs"] == [list(x) for x in pairs]
    # a column against a copy of itself: the paired difference is identically zero
    twin = metrics.bootstrap(y, np.stack([s[0], s[0]]), replicates=50)
    for stat in metrics.BOOTSTRAP_STATS:
        dlo, dhi = twin.diff_ci(0.95, stat)
        assert dlo.tolist() == [0.0, 0.0, 0.0] and dhi.tolist() == [0.0, 0.0, 0.0] and twin.diff_p(stat).tolist() == [1.0, 1.0, 1.0]
    for bad in (0.0, 1.0, True, "0.9"):
        with pytest.raises(ValueError, match="level"):
            b.ci(bad)
    with pytest.raises(ValueError, match="stat"):
        b.ci(0.9, "f1")
    # a clearly better column: its difference to noise is significant and the interval excludes 0
    good = metrics.bootstrap(y, np.stack([s[0] + 3.0 * (y == 1), np.random.default_rng(0).standard_normal(200).astype(np.float32)]), 200)
    assert good.diff_p("auc")[1] == pytest.approx(2 / 201) and good.diff_ci(0.95, "auc")[0][1] > 0 and good.diff_ci(0.95, "ap")[0][1] > 0


def test_what_the_public_call_refuses_and_skips():
    y, s = bu.case(50, "half", "continuous", 1, K=2)
    assert metrics.bootstrap(np.zeros(50, np.int64), s, 5) is None and metrics.bootstrap(np.ones(50, np.int64), s, 5) is None
    assert metrics.bootstrap(np.full(50, 2), s, 5) is None
    nan = s.copy()
    nan[1, np.flatnonzero(y == 1)[0]] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        metrics.bootstrap(y, nan, 5)
    ignored = s.copy()
    y2 = y.copy()
    y2[3] = -1
    ignored[0, 3] = np.nan                                             # a NaN under an ignored label is not a used score
    assert metrics.bootstrap(y2, ignored, 5) is not None
    for kw, msg in (({"replicates": 0}, "replicates"), ({"replicates": 65537}, "replicates"), ({"replicates": 2.5}, "replicates"),
                    ({"tpr": 0.0}, "tpr"), ({"tpr": 1.5}, "tpr"), ({"seed": -1}, "seed")):
        with pytest.raises(ValueError, match=msg):
            metrics.bootstrap(y, s, **{"replicates": 5, **kw})
    with pytest.raises(ValueError, match="score columns"):
        metrics.bootstrap(y, np.zeros((9, 50), np.float32), 5)
    with pytest.raises(ValueError, match="as many labels"):
        metrics.bootstrap(y[:-1], s, 5)
    with pytest.raises(ValueError, match="between 2 and"):
        metrics.bootstrap(y[:1], s[:, :1], 5)
    with pytest.raises(ValueError, match="one length"):
        metrics.bootstrap(y, [s[0], s[1][:-1]], 5)
    with pytest.raises(RuntimeError, match="GPU scores"):
        metrics.bootstrap_device(y, s, 5)
    # a list of host columns and CPU tensors are the host route
    a, b = metrics.bootstrap(y, [s[0], s[1]], 7, seed=4), metrics.bootstrap(torch.from_numpy(y), torch.from_numpy(s), 7, seed=4)
    assert np.array_equal(a.counts["u2"], b.counts["u2"]) and np.array_equal(a.counts["ap"], b.counts["ap"])


def test_standard_error_of_the_auc_against_delong():
    """continuous scores, n = 2000 with m = 400, B = 2000, the host route.  The margin is not a measurement: five standard deviations
    of a standard deviation estimated from B replicates, 5 / sqrt(2 (B - 1)) = 0.079, plus 2 / min(m, n0) = 0.005 for the stratified
    estimator's finite-sample factor, both relative to DeLong's standard error."""
    n, m, B = 2000, 400, 2000
    rng = np.random.default_rng(2024)
    y = np.zeros(n, np.int64)
    y[rng.permutation(n)[:m]] = 1
    s = (rng.standard_normal(n) + 1.0 * (y == 1)).astype(np.float32)
    boot, dl = metrics.bootstrap(y, s, replicates=B, seed=0), metrics.delong(y, s)
    assert boot.auc[0] == dl.auc[0]
    margin = 5 / math.sqrt(2 * (B - 1)) + 2 / min(m, n - m)
    ratio = boot.se("auc")[0] / dl.se[0]
    print(f"bootstrap se {boot.se('auc')[0]:.6f}, DeLong se {dl.se[0]:.6f}, ratio {ratio:.4f}, margin {margin:.4f}")
    assert abs(ratio - 1.0) <= margin
    lo, hi = boot.ci(0.95)
    dlo, dhi = dl.ci(0.95)
    assert lo[0] < boot.auc[0] < hi[0] and abs(lo[0] - dlo[0]) < dl.se[0] and abs(hi[0] - dhi[0]) < dl.se[0]


def test_c_abi_checks_its_arguments_and_launches_nothing():
    from eoe_amd import _lib
    from eoe_amd._lib import lib
    assert lib.eoe_abi_version() == _lib.ABI_VERSION                    # additive: the ABI version does not move
    ok = C.c_void_p(4096)                                              # never dereferenced: every call below is refused first
    names = (("scores", ok), ("labels", ok), ("n", 100), ("K", 2), ("B", 10), ("seed", 0), ("tpr", 0.95), ("u2", ok), ("fps", ok), ("ap", ok),
             ("counts", ok), ("scratch", ok), ("stream", None))
    call = lambda **kw: lib.eoe_bootstrap_counts(*[kw.get(k, d) for k, d in names])                 # noqa: E731
    for kw, msg in (({"scores": None}, "null scores"), ({"labels": None}, "null labels"), ({"u2": None}, "null output table"),
                    ({"fps": None}, "null output table"), ({"ap": None}, "null output table"), ({"counts": None}, "null counts"),
                    ({"scratch": None}, "null scratch"), ({"n": 1}, "n must be in [2, 1048576], not 1"),
                    ({"n": (1 << 20) + 1}, "n must be in [2, 1048576]"), ({"K": 0}, "K must be in [1, 8], not 0"),
                    ({"K": 9}, "K must be in [1, 8], not 9"), ({"B": 0}, "B must be in [1, 65536], not 0"),
                    ({"B": 65537}, "B must be in [1, 65536], not 65537"), ({"tpr": 0.0}, "tpr must be in (0, 1]"),
                    ({"tpr": 1.25}, "tpr must be in (0, 1]"), ({"tpr": math.nan}, "tpr must be in (0, 1]"),
                    ({"scores": C.c_void_p(4098)}, "4-byte aligned"), ({"labels": C.c_void_p(4100)}, "8-byte aligned"),
                    ({"ap": C.c_void_p(4100)}, "8-byte aligned"), ({"scratch": C.c_void_p(4100)}, "scratch must be 8-byte aligned")):
        assert call(**kw) == 1 and msg in lib.eoe_last_error().decode(), kw
    dnames = (("labels", ok), ("n", 100), ("b", 0), ("seed", 0), ("out", ok), ("scratch", ok), ("stream", None))
    draws = lambda **kw: lib.eoe_bootstrap_draws(*[kw.get(k, d) for k, d in dnames])                # noqa: E731
    for kw, msg in (({"labels": None}, "null labels"), ({"out": None}, "null out"), ({"scratch": None}, "null scratch"),
                    ({"n": 1}, "n must be in [2, 1048576], not 1"), ({"b": -1}, "b must be in [0, 65536), not -1"),
                    ({"b": 65536}, "b must be in [0, 65536)"), ({"out": C.c_void_p(4098)}, "8-byte aligned, out 4-byte")):
        assert draws(**kw) == 1 and msg in lib.eoe_last_error().decode(), kw
    for n, K, B in ((1, 1, 1), (2, 0, 1), (2, 9, 1), ((1 << 20) + 1, 1, 1), (2, 1, 0), (2, 1, 65537)):
        assert lib.eoe_bootstrap_scratch_bytes(n, K, B) == 0
    # nothing in the scratch grows with B; per column a 64-bit counter, a position and a flag byte per sample
    up = lambda x, a: -(-x // a) * a                                                                # noqa: E731
    for n, K in ((2, 1), (256, 1), (257, 3), (16385, 8), (90_000, 5), (1 << 20, 8)):
        want = up(4 * n, 256) + K * up(n, 256) * 12 + K * up(n, 256) + 256
        assert lib.eoe_bootstrap_scratch_bytes(n, K, 1) == lib.eoe_bootstrap_scratch_bytes(n, K, 65536) == want


def test_trainer_option_parsing():
    from eoe_amd.metrics import PRC, ROC
    from eoe_amd.training import HSCTrainer
    tr = HSCTrainer(None, dataset=lambda c, s: None)
    assert tr.bootstrap is None and tr.bootstraps == {}
    on = HSCTrainer(None, dataset=lambda c, s: None, bootstrap=50, bootstrap_level=0.9, bootstrap_seed=1 << 40)
    assert (on.bootstrap, on.bootstrap_level, on.bootstrap_seed) == (50, 0.9, 1 << 40)
    for bad in (0, -1, 65537, 2.0, True, "50"):
        with pytest.raises(ValueError, match="bootstrap"):
            HSCTrainer(None, dataset=lambda c, s: None, bootstrap=bad)
    for bad in (0.0, 1.0, True, "0.9"):
        with pytest.raises(ValueError, match="bootstrap_level"):
            HSCTrainer(None, dataset=lambda c, s: None, bootstrap=5, bootstrap_level=bad)
    for bad in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="bootstrap_seed"):
            HSCTrainer(None, dataset=lambda c, s: None, bootstrap=5, bootstrap_seed=bad)
    assert not hasattr(ROC(0.5), "boot_ci") and not any(hasattr(PRC(0.5), a) for a in ("ci", "se"))


def _host_trainer(tmp_path, name, y, s, lines=None, **kw):
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger

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

    logdir = str(tmp_path / name)
    logger = JsonLogger(logdir)
    if lines is not None:
        logger.logtxt = lines.append
    tr = Trainer(torch.nn.Identity(), dataset=lambda c, seed: Source(seed), device="cpu", batch_size=16, logger=logger, **kw)
    kept = []
    eval_cls = tr.eval_cls
    tr.eval_cls = lambda *a, **k: (lambda out: (kept.append(out), out)[1])(eval_cls(*a, **k))       # keep what `run` gets
    tr.run(run_seeds=s.shape[0], train=False)
    assert tr._boot_scores is None                                     # scores are kept only while `run` compares seeds
    return tr, kept, logdir


def test_trainer_off_changes_nothing_and_on_logs_intervals_and_the_comparison(tmp_path):
    """`run(train=False)` on host scores (a CPU device and a model that is its own score): the host route of the option end to end"""
    y, s = bu.case(64, "half", "continuous", 3, K=3)
    lines = []
    tr, kept, logdir = _host_trainer(tmp_path, "on", y, s, lines, bootstrap=40, bootstrap_level=0.9, bootstrap_seed=5)
    off, kept_off, logdir_off = _host_trainer(tmp_path, "off", y, s)
    added = {f"eval_cls0_it{i}_bootstrap.json" for i in range(3)} | {"eval_cls0_bootstrap_compare.json"}
    assert set(os.listdir(logdir)) - set(os.listdir(logdir_off)) == added and not set(os.listdir(logdir_off)) & added
    assert off.bootstraps == {} and not any(hasattr(r, "boot_ci") or hasattr(p, "ci") or hasattr(p, "se") for r, p in kept_off)
    assert off.auc_tests == {} and tr.auc_tests == {}                  # independent of auc_ci
    assert sorted(tr.bootstraps[0]) == [0, 1, 2]
    for i, (roc, prc) in enumerate(kept):
        want = metrics.bootstrap(y, s[i], 40, seed=5)
        got = tr.bootstraps[0][i]
        assert np.array_equal(got.counts["u2"], want.counts["u2"]) and np.array_equal(got.counts["ap"], want.counts["ap"])
        assert roc.auc == kept_off[i][0].auc and prc.avg_prec == kept_off[i][1].avg_prec
        assert roc.boot_ci == tuple(float(x[0]) for x in want.ci(0.9, "auc")) and prc.ci == tuple(float(x[0]) for x in want.ci(0.9, "ap"))
        assert prc.se == want.se("ap")[0] and prc.ci[0] <= prc.ci[1]
        with open(os.path.join(logdir, f"eval_cls0_it{i}_bootstrap.json")) as f:
            assert json.load(f) == want.to_json(0.9)
    with open(os.path.join(logdir, "eval_cls0_bootstrap_compare.json")) as f:
        assert json.load(f) == {"seeds": [0, 1, 2], **metrics.bootstrap(y, s, 40, seed=5).to_json(0.9)}
    tails = [x for x in lines if "bootstrap CI of the AP" in x]
    assert len(tails) == 3 and all(x.startswith("Eval: class") and "90% bootstrap CI of the AP [" in x for x in tails)
    # together with auc_ci both tails are there, DeLong's first
    both = []
    _host_trainer(tmp_path, "both", y, s[:1], both, bootstrap=10, auc_ci=0.95)
    line = [x for x in both if "bootstrap CI" in x]
    assert len(line) == 1 and line[0].index("CI of the AUC") < line[0].index("bootstrap CI of the AP")


def test_a_nan_test_score_costs_the_intervals_not_the_run(tmp_path):
    y = np.array([0, 1, 0, 1, 1, 0])
    s = np.array([[0.1, 0.9, 0.2, np.nan, 0.7, 0.3]] * 2, np.float32)
    lines = []
    tr, kept, logdir = _host_trainer(tmp_path, "nan", y, s, lines, bootstrap=10)
    assert tr.bootstraps == {} and not any("bootstrap" in f for f in os.listdir(logdir))
    assert sum("no bootstrap intervals" in x for x in lines) == 2
