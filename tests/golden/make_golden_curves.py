"""Generates tests/golden/g23_curves.npz: the ROC and precision-recall curves the reference's trainer makes
(`training/ad_trainer.py:452-455, 516-522`: sklearn's `roc_curve`, `auc`, `precision_recall_curve`, `average_precision_score`, called
here as it calls them) on stored inputs, and `mean_plot` of the reference's `utils/logger.py:94-122` on three ROCs and three PRCs.
Run by hand where the reference and sklearn are available; the tests only read the .npz.

    python tests/golden/make_golden_curves.py <the reference's src/eoe directory>

`logger.py` is executed by file path, nothing re-typed; what it imports and this fixture does not need (`cv2`, `torchvision`,
tensorboard, ...) is stubbed in `sys.modules` when it is not installed.  Inputs and outputs only are stored.

Cases (float32 scores, labels 0 / 1), the smallest at which each stage of the device path can go wrong:
  n2             one sample of each class
  n3_tie         one tie across the classes
  n255 n256 n257 no ties: the edge of the count pass's 256-wide tile
  n513_equal     every score equal: one threshold, nothing to drop
  n1000_quarters scores rounded to quarters: heavy ties, about 25 thresholds
  n1023 n1025    no ties: the edge of the compaction's 1 024-wide chunk (n1024 itself too)
  n600_separated every positive above every negative: drop_intermediate leaves three of the 600 points
  n300_zeros     -0.0 and 0.0 mixed into the scores, -0.0 first: one group whose threshold keeps the sign bit
Per case: `y`, `s`; `roc_fpr`, `roc_tpr`, `roc_thr` (drop_intermediate=True, the default the trainer uses), `rocfull_*`
(drop_intermediate=False), `prc_prec`, `prc_rec`, `prc_thr`, `auc`, `ap`, `K` (distinct scores), `K_roc` (ROC points before the
prepended one).
`mean/`: under np.random.seed(7), `mean_plot` of the ROCs of n255, n1000_quarters, n1025 and then of their PRCs: the returned arrays
and scalars, and the Mersenne Twister state afterwards (`state_keys`, `state_pos`).
"""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
from sklearn.metrics import auc as compute_auc, average_precision_score, precision_recall_curve, roc_curve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

MEAN_CASES = ("n255", "n1000_quarters", "n1025")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def load_logger(ref: str):
    blank = lambda n: type(n, (), {})      # noqa: E731
    wanted = {"cv2": {}, "torchvision": {}, "torchvision.utils": {}, "torchvision.transforms": {"Compose": blank("Compose")},
              "torch.utils.tensorboard": {"SummaryWriter": blank("SummaryWriter")}, "tqdm": {"tqdm": blank("tqdm")},
              "matplotlib": {}, "matplotlib.pyplot": {}}
    for name, attrs in wanted.items():
        try:
            importlib.import_module(name)
        except Exception:
            m = _stub(name, **attrs)
            if "." in name:
                parent, child = name.rsplit(".", 1)
                if parent in sys.modules:
                    setattr(sys.modules[parent], child, m)
    spec = importlib.util.spec_from_file_location("eoe_ref_logger", os.path.join(ref, "utils", "logger.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def inputs():
    rng = np.random.default_rng(23)
    cases = {}

    def labels(n, p=0.3):
        y = (rng.random(n) < p).astype(np.int64)
        y[0], y[1] = 0, 1
        return y

    def distinct(n):
        while True:
            s = rng.standard_normal(n).astype(np.float32)
            if np.unique(s).size == n:
                return s

    cases["n2"] = (np.array([1, 0], np.int64), np.array([0.25, 0.75], np.float32))
    cases["n3_tie"] = (np.array([1, 0, 1], np.int64), np.array([0.5, 0.5, 0.125], np.float32))
    for n in (255, 256, 257, 1023, 1024, 1025):
        cases[f"n{n}"] = (labels(n), distinct(n))
    cases["n513_equal"] = (labels(513), np.full(513, 0.25, np.float32))
    cases["n1000_quarters"] = (labels(1000), (np.round(rng.standard_normal(1000) * 4) / 4).astype(np.float32))
    y = labels(600, 0.4)
    s = distinct(600)
    s = np.where(y == 1, np.abs(s) + 1.0, -np.abs(s) - 1.0).astype(np.float32)
    assert np.unique(s).size == 600
    cases["n600_separated"] = (y, s)
    y, s = labels(300, 0.5), distinct(300)
    zeros = rng.permutation(300)[:40]
    s[zeros] = np.where(rng.random(40) < 0.5, np.float32(-0.0), np.float32(0.0))
    s[zeros.min()] = np.float32(-0.0)                      # the group's smallest index is a negative zero ...
    s[zeros.max()] = np.float32(0.0)                       # ... and a positive one is in it
    cases["n300_zeros"] = (y, s)
    return cases


def main():
    logger = load_logger(sys.argv[1])
    out, rocs, prcs = {}, {}, {}
    for name, (y, s) in inputs().items():
        assert s.dtype == np.float32 and y.dtype == np.int64 and (y == 0).any() and (y == 1).any()
        fpr, tpr, thr = roc_curve(y, s)                                              # ad_trainer.py:453, 517
        auc = compute_auc(fpr, tpr)                                                  # :454, 518
        ffpr, ftpr, fthr = roc_curve(y, s, drop_intermediate=False)
        prec, rec, pthr = precision_recall_curve(y, s)                               # :520
        ap = average_precision_score(y, s)                                           # :521
        assert thr.dtype == np.float32 and pthr.dtype == np.float32
        rocs[name] = logger.ROC(tpr, fpr, thr, auc)                                  # :455, 519
        prcs[name] = logger.PRC(prec, rec, pthr, ap)                                 # :522
        rec_ = {"y": y, "s": s, "roc_fpr": fpr, "roc_tpr": tpr, "roc_thr": thr, "rocfull_fpr": ffpr, "rocfull_tpr": ftpr,
                "rocfull_thr": fthr, "prc_prec": prec, "prc_rec": rec, "prc_thr": pthr, "auc": np.float64(auc), "ap": np.float64(ap),
                "K": np.int64(pthr.size), "K_roc": np.int64(thr.size - 1)}
        out.update({f"{name}/{k}": v for k, v in rec_.items()})
        print(name, "n", y.size, "K", pthr.size, "K_roc", thr.size - 1, "auc", auc, "ap", ap)
    assert int(out["n513_equal/K"]) == 1 and int(out["n600_separated/K_roc"]) == 3 and 20 <= int(out["n1000_quarters/K"]) <= 40
    assert int(out["n1023/K"]) == 1023 and int(out["n1025/K_roc"]) < 1025
    z = out["n300_zeros/prc_thr"]
    assert np.signbit(z[z == 0]).all() and z[z == 0].size == 1

    lengths = {len(rocs[c].ths) for c in MEAN_CASES} | {len(prcs[c].ths) for c in MEAN_CASES}
    assert len(lengths) == 6
    np.random.seed(7)
    m_roc = logger.mean_plot([rocs[c] for c in MEAN_CASES])
    m_prc = logger.mean_plot([prcs[c] for c in MEAN_CASES])
    state = np.random.get_state()
    assert state[0] == "MT19937" and state[3] == 0
    out.update({"mean/roc_tpr": m_roc.tpr, "mean/roc_fpr": m_roc.fpr, "mean/roc_ths": m_roc.ths, "mean/roc_auc": np.float64(m_roc.auc),
                "mean/roc_std": np.float64(m_roc.std), "mean/roc_n": np.int64(m_roc.n),
                "mean/prc_prec": m_prc.prec, "mean/prc_rec": m_prc.rec, "mean/prc_ths": m_prc.ths,
                "mean/prc_avg_prec": np.float64(m_prc.avg_prec), "mean/prc_std": np.float64(m_prc.std), "mean/prc_n": np.int64(m_prc.n),
                "mean/state_keys": np.asarray(state[1], np.uint32), "mean/state_pos": np.int64(state[2])})
    print("mean roc", m_roc.tpr.shape, m_roc.auc, "mean prc", m_prc.prec.shape, m_prc.avg_prec, "state pos", state[2])

    path = os.path.join(HERE, "g23_curves.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
