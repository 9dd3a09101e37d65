"""Times the ranking of an evaluation's scores (eoe_amd.metrics.score_extremes, csrc/topk.hip) on GPU-resident scores, k = 20, two
label groups, at n = 10 000 (a CIFAR test set) and n = 90 000 -- on the same box in the same run:

  hip_kernels   `eoe_score_extremes` alone (the memset and its seven launches) into preallocated buffers; device events around a window
                of back-to-back calls.
  device_call   `metrics.score_extremes(labels, scores, 20)` as the trainer calls it: the buffers, the kernels, the one copy of the 4 k
                pairs and three counts to the host, the `Extremes`; wall clock.
  host_call     what a user would do otherwise: copy scores and labels to the host, then the two stable argsorts per group (through
                `metrics.score_extremes` on the arrays); wall clock, the device-to-host copies included.
  torch_topk    `torch.topk` per group and end on the device (boolean-mask the group, largest / smallest 20, `.cpu()` of the four
                results); wall clock.  For reference only: `torch.topk` fixes no order among equal scores, so it is not the same result.
A warm-up, then repeats alternating the variants; medians over the repeats.  Scores are HSC-like (uniform in [0, 1)) and, second,
quantised to 256 values (ties everywhere); a tenth of the labels is 1.  The device and the host path are compared for equal positions
and score bits before anything is timed.  One JSON line per case.

  python tools/topk_bench.py [--repeats 5] [--window 0.2]"""
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

K = 20


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
        for kind in ("hsc", "ties256"):
            s = rng.random(n).astype(np.float32)
            if kind == "ties256":
                s = np.floor(s * np.float32(256.0)) / np.float32(256.0)
            y = (rng.random(n) < 0.1).astype(np.int64)
            sc, la = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
            out = torch.empty(8 * K + 3, dtype=torch.int32, device="cuda")
            scratch = torch.empty(lib.eoe_score_extremes_scratch_bytes(n, K), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def hip_kernels():
                check(lib.eoe_score_extremes(sc.data_ptr(), la.data_ptr(), n, K, out.data_ptr(), out.data_ptr() + 16 * K,
                                             out.data_ptr() + 32 * K, scratch.data_ptr(), st), "eoe_score_extremes")

            device_call = lambda: metrics.score_extremes(la, sc, K)                                 # noqa: E731

            def host_call():
                return metrics.score_extremes(la.cpu().numpy(), sc.cpu().numpy(), K)

            def torch_topk():
                res = []
                for g in (0, 1):
                    member = torch.nonzero(la == g).reshape(-1)
                    sg = sc[member]
                    for largest in (True, False):
                        v, i = torch.topk(sg, min(K, sg.numel()), largest=largest)
                        res.append((member[i].cpu(), v.cpu()))
                return res

            assert device_call() == host_call()
            for _ in range(3):
                hip_kernels(), device_call(), host_call(), torch_topk()
            t = {"hip_kernels": [], "device_call": [], "host_call": [], "torch_topk": []}
            for _ in range(a.repeats):
                t["hip_kernels"].append(window_ms(hip_kernels, a.window))
                t["device_call"].append(wall_ms(device_call, 20))
                t["host_call"].append(wall_ms(host_call, 10))
                t["torch_topk"].append(wall_ms(torch_topk, 10))
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"case": "eval_score_extremes", "n": n, "k": K, "scores": kind, "box": torch.cuda.get_device_name(0),
                              **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                              "hip_kernels_mscores_per_s": n / (med["hip_kernels"] * 1e-3) / 1e6,
                              "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                              "speedup_device_call_vs_torch_topk": med["torch_topk"] / med["device_call"],
                              "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
