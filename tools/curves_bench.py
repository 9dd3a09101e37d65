"""Times the ROC + precision-recall curves of one epoch tail (eoe_amd.metrics, csrc/curves.hip) on GPU-resident scores, at the two
sizes the trainer meets -- n = 10 000 (a CIFAR test set) and n = 90 000 (a leave-one-out training epoch) -- on the same box in the
same run:

  hip_kernels   `eoe_rank_curves` alone (the memset and its three launches) into preallocated buffers; device events around a window
                of back-to-back calls.  The achieved rate counts the n^2 score pairs the count pass visits.
  device_call   `metrics.curves_device(labels, scores)` as the trainer calls it: the finite check, the buffers, the kernels, the copy
                of K, K_roc and the used table entries to the host and the divisions there; wall clock.
  host_call     the path the device one replaces: copy scores and labels to the host, then `metrics.roc_curve` +
                `metrics.precision_recall_curve` on the arrays (a stable sort each); wall clock, the device-to-host copy included.
A warm-up, then repeats alternating the variants; medians over the repeats.  Scores are random floats (K within a few of n, the most the
compaction and the copy can be asked for) and, second, scores rounded to 1/50 (heavy ties, K of a few hundred).  The two paths are
compared for equality before anything is timed.  One JSON line per case.

  python tools/curves_bench.py [--repeats 5] [--window 0.2]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for n in (10_000, 90_000):
        for ties in (False, True):
            s = rng.standard_normal(n).astype(np.float32)
            if ties:
                s = (np.round(s * 50) / 50).astype(np.float32)
            y = (rng.random(n) < 0.1).astype(np.int64)
            sc, la = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
            i64 = torch.empty((4, n), dtype=torch.int64, device="cuda")
            f32 = torch.empty((2, n), dtype=torch.float32, device="cuda")
            counts = torch.empty(2, dtype=torch.int32, device="cuda")
            scratch = torch.empty(lib.eoe_rank_curves_scratch_bytes(n), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def hip_kernels():
                check(lib.eoe_rank_curves(sc.data_ptr(), la.data_ptr(), 1, n, 1, i64[0].data_ptr(), i64[1].data_ptr(), f32[0].data_ptr(),
                                          i64[2].data_ptr(), i64[3].data_ptr(), f32[1].data_ptr(), counts.data_ptr(), scratch.data_ptr(), st),
                      "eoe_rank_curves")

            device_call = lambda: metrics.curves_device(la, sc)                                   # noqa: E731

            def host_call():
                hs, hy = sc.cpu().numpy(), la.cpu().numpy()
                return metrics.roc_curve(hy, hs), metrics.precision_recall_curve(hy, hs)

            for dev, host in zip(device_call(), host_call()):
                for d, h in zip(dev, host):
                    assert d.shape == h.shape and np.array_equal(d, h)
            hip_kernels()
            K, K_roc = counts.cpu().tolist()
            for _ in range(3):
                hip_kernels(), device_call(), host_call()
            t = {"hip_kernels": [], "device_call": [], "host_call": []}
            for _ in range(a.repeats):
                t["hip_kernels"].append(window_ms(hip_kernels, a.window))
                t["device_call"].append(wall_ms(device_call, 20))
                t["host_call"].append(wall_ms(host_call, 10))
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"case": "epoch_tail_curves", "n": n, "ties": ties, "K": K, "K_roc": K_roc, "box": torch.cuda.get_device_name(0),
                              **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                              "hip_kernels_gpairs_per_s": float(n) * n / (med["hip_kernels"] * 1e-3) / 1e9,
                              "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                              "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
