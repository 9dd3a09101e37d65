"""Times DeLong's AUC test (eoe_amd.metrics.delong, csrc/delong.hip) on GPU-resident scores at 10 000 and at 90 000 scores, with K = 1
and K = 5 score columns, at roughly 10 % and at 50 % positives -- on the same box in the same run:

  hip_kernels   `eoe_delong_counts` alone (a memset and three launches) into preallocated buffers; device events around a window of
                back-to-back calls.
  device_call   `metrics.delong(labels, scores)` as the trainer calls it: host labels, the one upload, the buffers, the kernels, the
                one copy back, the `AucTest`; wall clock.
  host_call     what a user would do otherwise with this package: copy the scores to the host, then the same table from sorts (through
                `metrics.delong` on the arrays); wall clock, the device-to-host copy included.
A warm-up, then repeats alternating the variants; medians over the repeats, and every repeat's value under `all_ms`.  The scores are
HSC-like (uniform in [0, 1), the positives shifted up; columns 1.. are column 0 plus noise).  The device and the host path are compared
(equal integers) before anything is timed.  The host route is O(n log n) and the device route O(n_pos n_neg): no ratio is promised.
One JSON line per case.

  python tools/delong_bench.py [--repeats 5] [--window 0.2]"""
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
        for K in (1, 5):
            for share in (0.1, 0.5):
                y = (rng.random(n) < share).astype(np.int64)
                base = rng.random(n) + 0.3 * y
                s = np.stack([base + 0.05 * j * rng.standard_normal(n) for j in range(K)]).astype(np.float32)
                sc, la = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
                P = K * (K + 1) // 2
                out = torch.empty(2 * K + 2 * P + 3, dtype=torch.int64, device="cuda")
                scratch = torch.empty(lib.eoe_delong_scratch_bytes(n, K), dtype=torch.uint8, device="cuda")
                st = torch.cuda.current_stream().cuda_stream

                def hip_kernels():
                    check(lib.eoe_delong_counts(sc.data_ptr(), la.data_ptr(), n, K, out.data_ptr(), scratch.data_ptr(), st),
                          "eoe_delong_counts")

                device_call = lambda: metrics.delong(y, sc)                                   # noqa: E731
                host_call = lambda: metrics.delong(y, sc.cpu().numpy())                      # noqa: E731

                dev, host = device_call(), host_call()
                assert all(np.array_equal(dev.counts[k], host.counts[k]) for k in ("T_pos", "T_neg", "A", "B"))
                assert dev.cov.tolist() == host.cov.tolist()
                hip_kernels()
                torch.cuda.synchronize()
                assert out[:K].cpu().tolist() == dev.counts["T_pos"].tolist()
                variants = {"hip_kernels": lambda: window_ms(hip_kernels, a.window), "device_call": lambda: wall_ms(device_call, 10),
                            "host_call": lambda: wall_ms(host_call, 5)}
                for _ in range(2):
                    hip_kernels(), device_call(), host_call()
                t = {k: [] for k in variants}
                for _ in range(a.repeats):
                    for k, fn in variants.items():
                        t[k].append(fn())
                med = {k: float(np.median(v)) for k, v in t.items()}
                m, n0 = dev.n_pos, dev.n_neg
                print(json.dumps({"case": "eval_delong", "n": n, "columns": K, "n_pos": m, "n_neg": n0,
                                  "box": torch.cuda.get_device_name(0),
                                  **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                                  "hip_kernels_gcompares_per_s": 2.0 * K * m * n0 / (med["hip_kernels"] * 1e-3) / 1e9,
                                  "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                                  "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
