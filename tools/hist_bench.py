"""Times the two score histograms of one epoch tail (eoe_amd.metrics, csrc/hist.hip) on GPU-resident scores, at the two sizes the
trainer meets -- n = 10 000 (a CIFAR test set) and n = 90 000 (a leave-one-out training epoch) -- on the same box in the same run:

  hip_kernels   `eoe_score_hist` alone (the memset and its two launches) into preallocated buffers; device events around a window of
                back-to-back calls.
  device_call   `metrics.score_histograms(labels, scores)` as the trainer calls it: the finite check, the buffers, the kernels, the one
                copy of the counts and scalars to the host and the trimming there; wall clock.
  host_call     what a user would do otherwise: copy scores and labels to the host, then `np.histogram` over TensorBoard's edges once
                per label (through `metrics.score_histograms` on the arrays, trimming and scalars included); wall clock, the
                device-to-host copies included.
A warm-up, then repeats alternating the variants; medians over the repeats.  Scores are HSC-like (uniform in [0, 1)) and, second,
BCE-like logits (uniform in [-40, 40)); a tenth of the labels is 1.  The two paths are compared for equal buckets before anything is
timed.  One JSON line per case.

  python tools/hist_bench.py [--repeats 5] [--window 0.2]"""
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
    edges = metrics.default_edges()
    host_edges, dev_edges = metrics._device_edges(edges, torch.device("cuda", 0))
    for n in (10_000, 90_000):
        for kind in ("hsc", "bce"):
            s = (rng.random(n) if kind == "hsc" else rng.uniform(-40.0, 40.0, n)).astype(np.float32)
            y = (rng.random(n) < 0.1).astype(np.int64)
            sc, la = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
            counts = torch.empty((2, edges.size - 1), dtype=torch.int32, device="cuda")
            stats = torch.empty((2, 5), dtype=torch.float64, device="cuda")
            scratch = torch.empty(lib.eoe_score_hist_scratch_bytes(n), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def hip_kernels():
                check(lib.eoe_score_hist(sc.data_ptr(), la.data_ptr(), n, host_edges.ctypes.data, dev_edges.data_ptr(), edges.size,
                                         counts.data_ptr(), stats.data_ptr(), scratch.data_ptr(), st), "eoe_score_hist")

            device_call = lambda: metrics.score_histograms(la, sc)                               # noqa: E731

            def host_call():
                return metrics.score_histograms(la.cpu().numpy(), sc.cpu().numpy())

            for d, h in zip(device_call(), host_call()):
                assert (d.bucket, d.bucket_limit, d.num, d.min, d.max) == (h.bucket, h.bucket_limit, h.num, h.min, h.max)
            for _ in range(3):
                hip_kernels(), device_call(), host_call()
            t = {"hip_kernels": [], "device_call": [], "host_call": []}
            for _ in range(a.repeats):
                t["hip_kernels"].append(window_ms(hip_kernels, a.window))
                t["device_call"].append(wall_ms(device_call, 20))
                t["host_call"].append(wall_ms(host_call, 10))
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"case": "epoch_tail_histograms", "n": n, "scores": kind, "buckets": [len(d.bucket) for d in device_call()],
                              "box": torch.cuda.get_device_name(0), **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                              "hip_kernels_mscores_per_s": n / (med["hip_kernels"] * 1e-3) / 1e6,
                              "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                              "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
