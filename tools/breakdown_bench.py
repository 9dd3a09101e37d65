"""Times the per-class breakdown of an evaluation's scores (eoe_amd.metrics.class_breakdown, csrc/breakdown.hip) on GPU-resident scores
at 10 000 scores / 10 classes (a CIFAR-10 test set), 10 000 / 100 and 90 000 / 30 -- on the same box in the same run:

  hip_kernels   `eoe_class_breakdown` alone (two memsets and two launches) into preallocated buffers; device events around a window of
                back-to-back calls.
  device_call   `metrics.class_breakdown(scores, classes, normal)` as the trainer calls it: class ids on the host mapped to 0..K-1, the
                one upload, the buffers, the kernels, the one copy back, the `Breakdown`; wall clock.
  host_call     what a user would do otherwise with this package: copy the scores to the host, then the same table from sorts (through
                `metrics.class_breakdown` on the arrays); wall clock, the device-to-host copy included.
  sklearn_calls the scores copied to the host, then per class `roc_auc_score`, `roc_curve(drop_intermediate=False)` for the FPR at the
                level and -- for an anomalous class -- `average_precision_score` on the class's sub-problem: K sorts of overlapping
                subsets; wall clock.  Skipped (null) without sklearn.
A warm-up, then repeats alternating the variants; medians over the repeats, and every repeat's value under `all_ms`.  One class is
normal (`one_vs_rest`), the scores are HSC-like (uniform in [0, 1)) and, second, quantised to 256 values (ties everywhere).  The device
and the host path are compared (equal integers, bit-equal thresholds) before anything is timed.  One JSON line per case.

  python tools/breakdown_bench.py [--repeats 5] [--window 0.2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd import metrics                    # noqa: E402
from eoe_amd._lib import check, lib            # noqa: E402

TPR = 0.95


def window_ms(fn, window_s):
    """ms per call over a window of at least window_s seconds, by device events"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        total = start.elapsed_time(end)
        if total >= window_s * 1e3:
            return total / n
        n = max(n * 2, int(n * 1.2 * window_s * 1e3 / max(total, 1e-3)))


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def sklearn_table(s, ids, normal):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    anomalous = ~np.isin(ids, normal)
    rows = []
    for k in np.unique(ids):
        side = int(k not in normal)
        keep = (ids == k) | (anomalous != bool(side))
        y, sub = anomalous[keep], s[keep]
        fpr, tpr, _ = roc_curve(y, sub, drop_intermediate=False)
        rows.append((roc_auc_score(y, sub), fpr[np.argmax(tpr >= TPR)], average_precision_score(y, sub) if side else None))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    rng = np.random.default_rng(0)
    for n, K in ((10_000, 10), (10_000, 100), (90_000, 30)):
        for kind in ("hsc", "ties256"):
            s = rng.random(n).astype(np.float32)
            if kind == "ties256":
                s = np.floor(s * np.float32(256.0)) / np.float32(256.0)
            ids = rng.integers(0, K, n).astype(np.int64)
            normal = [0]
            sc = torch.from_numpy(s).cuda()
            # the raw call's inputs, as class_breakdown prepares them
            side = np.array([0] + [1] * (K - 1), dtype=np.uint8)
            sizes = np.bincount(ids, minlength=K)
            m_pooled = metrics.place_for_tpr(TPR, int(sizes[1:].sum()))
            m_cls = np.array([m_pooled] + [metrics.place_for_tpr(TPR, int(c)) for c in sizes[1:]], dtype=np.int32)
            d_ids, d_m = torch.from_numpy(ids.astype(np.int32)).cuda(), torch.from_numpy(m_cls).cuda()
            d_side = torch.from_numpy(side).cuda()
            o_cnt = torch.empty((K + 1, 4), dtype=torch.int64, device="cuda")
            o_ap, o_thr = torch.empty(K, dtype=torch.float64, device="cuda"), torch.empty(K + 1, dtype=torch.float32, device="cuda")
            scratch = torch.empty(lib.eoe_class_breakdown_scratch_bytes(n, K), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def hip_kernels():
                check(lib.eoe_class_breakdown(sc.data_ptr(), d_ids.data_ptr(), d_side.data_ptr(), d_m.data_ptr(), m_pooled, n, K,
                                              o_cnt.data_ptr(), o_ap.data_ptr(), o_thr.data_ptr(), scratch.data_ptr(), st),
                      "eoe_class_breakdown")

            device_call = lambda: metrics.class_breakdown(sc, ids, normal, TPR)                     # noqa: E731
            host_call = lambda: metrics.class_breakdown(sc.cpu().numpy(), ids, normal, TPR)          # noqa: E731
            sklearn_calls = lambda: sklearn_table(sc.cpu().numpy(), ids, normal)                     # noqa: E731

            dev, host = device_call(), host_call()
            assert np.array_equal(dev.counts, host.counts) and dev.thresholds.tobytes() == host.thresholds.tobytes()
            assert all((x is None and y is None) or abs(x - y) <= n * 2.0 ** -52 for x, y in zip(dev.ap, host.ap))
            hip_kernels()
            torch.cuda.synchronize()
            assert np.array_equal(o_cnt.cpu().numpy(), dev.counts)
            variants = {"hip_kernels": lambda: window_ms(hip_kernels, a.window), "device_call": lambda: wall_ms(device_call, 10),
                        "host_call": lambda: wall_ms(host_call, 5)}
            if have_sklearn:
                variants["sklearn_calls"] = lambda: wall_ms(sklearn_calls, 1)
            for _ in range(2):
                hip_kernels(), device_call(), host_call()
            if have_sklearn:
                sklearn_calls()
            t = {k: [] for k in variants}
            for _ in range(a.repeats):
                for k, fn in variants.items():
                    t[k].append(fn())
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"case": "eval_class_breakdown", "n": n, "classes": K, "tpr": TPR, "scores": kind,
                              "box": torch.cuda.get_device_name(0),
                              **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                              "sklearn_calls_ms": round(med["sklearn_calls"], 5) if have_sklearn else None,
                              "hip_kernels_gcompares_per_s": n * n / (med["hip_kernels"] * 1e-3) / 1e9,
                              "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                              "speedup_device_call_vs_sklearn_calls": med["sklearn_calls"] / med["device_call"] if have_sklearn else None,
                              "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
