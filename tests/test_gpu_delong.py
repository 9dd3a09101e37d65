"""GPU tier: `eoe_delong_counts` (csrc/delong.hip) through `eoe_amd.metrics.delong_device` / `delong` -- the int64 table against the host
path's, integer for integer, on the CPU grid and at the kernel's tile and slice edges; the 16-bit casts, two runs, the NaN refusal,
lists of columns; and `ADTrainer(auc_ci=0.95)` on a tiny CNN32 task with two seeds."""
import json
import os

import numpy as np
import pytest
import torch

import delong_util as du
from eoe_amd import metrics

pytestmark = pytest.mark.gpu

TILE = metrics.DELONG_TILE


def _device_table(y, s):
    t_pos, t_neg, A, B, m, n0, bad = metrics.delong_device(y, torch.from_numpy(np.array(s)).cuda())           # a writable copy
    return {"T_pos": t_pos, "T_neg": t_neg, "A": A, "B": B, "m": m, "n0": n0}, bad


def _host_table(y, s):
    t_pos, t_neg, A, B, m, n0 = metrics._delong_host(np.asarray(y), np.asarray(s).reshape(-1, len(y)))
    return {"T_pos": t_pos, "T_neg": t_neg, "A": A, "B": B, "m": m, "n0": n0}


@pytest.mark.parametrize("n", du.SIZES)
def test_device_table_equals_the_host_table_on_the_cpu_grid(n):
    for (nn, share, kind, K) in du.grid():
        if nn != n:
            continue
        what = (n, share, kind, K)
        y, s, ref = du.case(n, share, kind, K)
        got, bad = _device_table(y, s)
        assert bad == 0, what                                          # the NaN scores of the "ignored" kind carry label -1
        du.assert_tables_equal(got, _host_table(y, s), what)           # T_pos == T_neg in the raw output is part of it
        du.assert_tables_equal(got, ref, what)
        t = metrics.delong(y, torch.from_numpy(s.copy()).cuda())
        if ref["m"] == 0 or ref["n0"] == 0:
            assert t is None, what
        else:
            host = metrics.delong(y, s)
            assert t.auc.tolist() == host.auc.tolist() and np.array_equal(t.cov, host.cov, equal_nan=True), what


def _edge_case(m, n0, K, kind, seed):
    rng = np.random.default_rng([seed, m, n0, K])
    y = np.zeros(m + n0, np.int64)
    y[rng.permutation(m + n0)[:m]] = 1
    base = rng.normal(size=m + n0) + 0.5 * y
    s = np.stack([base + 0.1 * j * rng.normal(size=m + n0) for j in range(K)]).astype(np.float32)
    if kind == "quant4":
        s = (np.clip(np.floor(s + 2.0), 0.0, 3.0) / 4.0).astype(np.float32)
    return y, s


def _edge_sizes():
    """(m, n0, K): a side of one tile, one more and one less, one sample past two tiles, a side of one sample, n = 4097; and opposite
    sides of exactly as many tiles as there are slices, one tile more (a slice walks two tiles, the last slices are empty) and one
    sample more than that"""
    out = []
    for side in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        out += [(side, 300, 1), (300, side, 2), (side, 1, 1), (1, side, 3), (side, side, 1)]
    out += [(4096, 1, 1), (1, 4096, 1), (2048, 2049, 1), (409, 3688, 3), (TILE, 4097 - TILE, 8), (4097 - TILE - 1, TILE + 1, 8)]
    for K in (8, 1):
        small = 40
        # the smallest opposite side with more tiles than its n has slices (a slice walks two tiles), and the one a tile below it
        first = next(b for b in range(TILE, metrics.DELONG_MAX_N, TILE) if b // TILE > metrics.delong_slices(small + b, K))
        for big in (first - TILE, first):
            out += [(small, big, K), (big + 1, small, K)]
    return out


@pytest.mark.parametrize("kind", ["continuous", "quant4"])
def test_device_table_equals_the_host_table_at_tile_and_slice_edges(kind):
    sizes = _edge_sizes()
    assert any(n0 // TILE > metrics.delong_slices(m + n0, K) for m, n0, K in sizes)          # some workgroup walks two tiles
    assert any(m + n0 == 4097 for m, n0, K in sizes)
    for i, (m, n0, K) in enumerate(sizes):
        y, s = _edge_case(m, n0, K, kind, i)
        got, bad = _device_table(y, s)
        assert bad == 0
        du.assert_tables_equal(got, _host_table(y, s), (kind, m, n0, K))


def test_half_precision_scores_are_cast_to_float32():
    y, s, _ = du.case(1000, "tenth", "continuous", 3)
    for dt in (torch.float16, torch.bfloat16):
        dev = torch.from_numpy(s.copy()).cuda().to(dt)
        t_pos, t_neg, A, B, m, n0, bad = metrics.delong_device(y, dev)
        want = _host_table(y, dev.float().cpu().numpy())
        du.assert_tables_equal({"T_pos": t_pos, "T_neg": t_neg, "A": A, "B": B, "m": m, "n0": n0}, want, str(dt))
        assert metrics.delong(y, dev).cov.tolist() == metrics.delong(y, dev.float().cpu().numpy()).cov.tolist()


def test_two_calls_give_the_same_bytes_and_lists_equal_the_stacked_call():
    y, s = _edge_case(700, 3397, 5, "quant4", 99)
    dev = torch.from_numpy(s).cuda()
    first, second = metrics.delong_device(y, dev), metrics.delong_device(torch.from_numpy(y).cuda(), dev)
    for a, b in zip(first[:4], second[:4]):
        assert a.dtype == np.int64 and a.tobytes() == b.tobytes()
    assert first[4:] == second[4:] == (700, 3397, 0) and first[0].tolist() == first[1].tolist()
    stacked, listed = metrics.delong(y, dev), metrics.delong(y, [dev[k].clone() for k in range(5)])
    for key in ("T_pos", "T_neg", "A", "B"):
        assert np.array_equal(stacked.counts[key], listed.counts[key])
    assert stacked.cov.tolist() == listed.cov.tolist() == metrics.delong(y, s).cov.tolist()
    single = metrics.delong(y, dev[2])                                 # a 1-d tensor is one column
    assert single.auc.tolist() == [stacked.auc[2]] and single.var.tolist() == [stacked.var[2]]
    with pytest.raises(ValueError, match="one length"):
        metrics.delong(y, [dev[0], dev[1][:-1]])
    with pytest.raises(ValueError, match="columns"):
        metrics.delong(y, [dev[0]] * 9)
    with pytest.raises(ValueError, match="labels"):
        metrics.delong(y[:-1], dev)


def test_a_nan_on_the_device_raises_from_the_wrapper():
    y, s = _edge_case(300, 600, 2, "continuous", 7)
    s[1, int(np.flatnonzero(y == 0)[-1])] = np.nan
    s[0, int(np.flatnonzero(y == 1)[0])] = np.nan
    assert metrics.delong_device(y, torch.from_numpy(s).cuda())[6] == 2
    with pytest.raises(ValueError, match="NaN"):
        metrics.delong(y, torch.from_numpy(s).cuda())
    y[np.isnan(s).any(axis=0)] = -1                                     # ignored samples may hold anything
    assert metrics.delong(y, torch.from_numpy(s).cuda()).cov.tolist() == metrics.delong(y, s).cov.tolist()


# ---- the trainer: the size of tests/test_gpu_trainer_extremes.py (40 test images of 32 x 32, CNN32, one epoch)
N_TEST = 40


def _source():
    from eoe_amd.data import ResidentImageSource
    rng = np.random.default_rng(17)
    img = lambda n, lo, hi: torch.from_numpy(rng.integers(lo, hi, (n, 32, 32, 3)).astype(np.uint8))    # noqa: E731
    labels = torch.zeros(N_TEST, dtype=torch.int64)
    labels[list(range(3, N_TEST, 4))] = 1
    return ResidentImageSource(img(48, 60, 160), img(32, 0, 256), img(N_TEST, 0, 256), labels, crop=32, padding=2, seed=3)


def _run(tmp_path, name, **kw):
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(11)
    logdir = str(tmp_path / name)
    tr = HSCTrainer(CNN32(bias=True), dataset=_source(), epochs=1, lr=1e-3, batch_size=16, logger=JsonLogger(logdir), **kw)
    rocs = []
    eval_cls = tr.eval_cls
    tr.eval_cls = lambda *a, **k: (lambda out: (rocs.append(out[0]), out)[1])(eval_cls(*a, **k))       # keep the ROCs `run` gets
    _, res = tr.run(run_seeds=2)
    return tr, res, rocs, logdir


def test_trainer_auc_ci_logs_intervals_and_compares_the_seeds(tmp_path):
    tr, res, rocs, logdir = _run(tmp_path, "on", auc_ci=0.95)
    off, res_off, rocs_off, logdir_off = _run(tmp_path, "off")
    added = {"eval_cls0_it0_auc_ci.json", "eval_cls0_it1_auc_ci.json", "eval_cls0_auc_compare.json"}
    assert set(os.listdir(logdir)) - set(os.listdir(logdir_off)) == added and not set(os.listdir(logdir_off)) & added
    assert res == res_off and tr.last_losses == off.last_losses
    assert tr._seed_scores is None and off._seed_scores is None        # the seeds' scores are released after the comparison
    assert off.auc_tests == {} and len(rocs_off) == 2 and not any(hasattr(r, a) for r in rocs_off for a in ("ci", "se", "var"))
    test = tr.auc_tests[0]
    assert set(tr.auc_tests) == {0} and (test.n_pos, test.n_neg) == (10, 30) and test.auc.shape == (2,)
    logged = []
    for seed, roc in enumerate(rocs):
        with open(os.path.join(logdir, f"eval_cls0_it{seed}_auc_ci.json")) as f:
            j = json.load(f)
        logged.append(j["auc"][0])
        assert j["level"] == 0.95 and (j["n_pos"], j["n_neg"]) == (10, 30)
        assert roc.ci == (j["ci_lo"][0], j["ci_hi"][0]) and roc.se == j["se"][0] and roc.var == j["var"][0]
        assert 0.0 <= roc.ci[0] <= roc.auc <= roc.ci[1] <= 1.0 and roc.ci[0] < roc.ci[1] and roc.se == np.sqrt(roc.var) > 0.0
        assert roc.auc == j["auc"][0]                                  # `eoe_auc_ap`: the same doubled count over 2 m n0, one fp64 division
        assert roc.auc == res["cls_aucs"][0][seed]
        # the interval is the host path's on the scores the evaluation logged
        with open(os.path.join(logdir, f"eval_cls0_it{seed}_anomaly_scores.json")) as f:
            s = np.array(list(json.load(f).values()), dtype=np.float64).astype(np.float32)
        assert metrics.delong(_source().test_y.cpu().numpy(), s).to_json(0.95) == j
    assert test.auc.tolist() == logged                                 # bit for bit
    with open(os.path.join(logdir, "eval_cls0_auc_compare.json")) as f:
        j = json.load(f)
    assert j == {"seeds": [0, 1], **test.to_json(0.95)} and j["auc"] == logged
    assert np.array_equal(test.pvalues(), test.pvalues().T) and test.pvalues()[0, 0] == 1.0 and 0.0 <= test.pvalues()[0, 1] <= 1.0
