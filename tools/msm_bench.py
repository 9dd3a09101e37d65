"""Times the multi-scale-mode filters (eoe_amd.msm.msm_filter, csrc/msm.hip) against the reference-equivalent torch chain
(torch.fft lpf / hpf + MinMaxNorm, conv2d Gaussian blur with reflect borders) on the same device and input.

Per (shape, case): a warm-up, then repeats alternating HIP and torch; each repeat times a window of >= --window seconds of
back-to-back calls with device events and reports ms per call; the median over the repeats is printed, with the max abs
difference between the two outputs (NaN positions must agree).  One JSON line per case.

  python tools/msm_bench.py [--repeats 5] [--window 0.5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd.msm import msm_filter, torch_blur, torch_fft_filter   # noqa: E402


def window_ms(fn, window_s):
    """ms per call over a window of at least window_s seconds"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 1, 0.0
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for shape in ((256, 3, 224, 224), (256, 3, 32, 32)):
        x = torch.rand(shape, generator=g, device="cuda")
        for op, mag in (("lpf", 8), ("hpf", 8), ("blur", 8)):
            hip = lambda: msm_filter(x, op, mag)
            ref = (lambda: torch_blur(x, mag)) if op == "blur" else (lambda: torch_fft_filter(x, op, mag))
            yh, yr = hip(), ref()
            torch.cuda.synchronize()
            nan_h, nan_r = torch.isnan(yh), torch.isnan(yr)
            ok = nan_h & nan_r
            diff = float((yh - yr).abs()[~ok].max()) if bool((~ok).any()) else 0.0
            for _ in range(3):
                hip(), ref()
            th, tr = [], []
            for _ in range(a.repeats):
                th.append(window_ms(hip, a.window))
                tr.append(window_ms(ref, a.window))
            print(json.dumps({"shape": list(shape), "op": op, "magnitude": mag, "hip_ms": float(np.median(th)),
                              "torch_ms": float(np.median(tr)), "speedup": float(np.median(tr) / np.median(th)),
                              "max_abs_diff": diff, "nan_agree": bool(torch.equal(nan_h, nan_r)),
                              "hip_ms_all": [round(t, 4) for t in th], "torch_ms_all": [round(t, 4) for t in tr]}), flush=True)


if __name__ == "__main__":
    main()
