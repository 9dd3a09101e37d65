"""Times the sharpen multi-scale mode (csrc/sharpen.hip: eoe_amd.msm.sharpen_u8 on uint8 NHWC, msm_sharpen on fp32 NCHW) at
256x3x32^2 and 256x3x224^2, with host Pillow's UnsharpMask on the same batch (one thread, image by image: what the reference's
PilUnsharpMask costs in a DataLoader worker) as the yardstick, and checks the kernel's bytes against Pillow's.

Device times: a warm-up, then the median over --repeats windows of >= --window seconds of back-to-back calls timed with device
events (ms per call).  Host: the median of --host-repeats passes over the batch.  One JSON line per (shape, layout).

  python tools/sharpen_bench.py [--repeats 5] [--window 0.5] [--host-repeats 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd.msm import msm_sharpen, sharpen_percent, sharpen_u8   # noqa: E402


def window_ms(fn, window_s):
    """ms per call over a window of at least window_s seconds"""
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


def pillow(u8: np.ndarray, percent: int):
    from PIL import Image, ImageFilter
    f = ImageFilter.UnsharpMask(2, percent, 3)
    return np.stack([np.asarray(Image.fromarray(img).filter(f)) for img in u8])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--magnitude", type=int, default=4)
    a = ap.parse_args()
    torch.set_num_threads(1)
    torch.cuda.set_device(0)
    percent = sharpen_percent(a.magnitude)
    rng = np.random.default_rng(0)
    for n, h in ((256, 32), (256, 224)):
        u8 = rng.integers(0, 256, (n, h, h, 3), dtype=np.uint8)
        host, ref = [], None
        for _ in range(a.host_repeats):
            t0 = time.perf_counter()
            ref = pillow(u8, percent)
            host.append((time.perf_counter() - t0) * 1e3)
        ud = torch.from_numpy(u8).cuda()
        xd = ud.permute(0, 3, 1, 2).float().div(255).contiguous()
        for layout, fn in (("u8_nhwc", lambda: sharpen_u8(ud, percent)), ("f32_nchw", lambda: msm_sharpen(xd, a.magnitude))):
            y = fn()
            torch.cuda.synchronize()
            got = y.cpu() if layout == "u8_nhwc" else y.mul(255).round().to(torch.uint8).permute(0, 2, 3, 1).cpu()
            exact = bool(np.array_equal(got.numpy(), ref))
            for _ in range(3):
                fn()
            t = [window_ms(fn, a.window) for _ in range(a.repeats)]
            print(json.dumps({"shape": [n, 3, h, h], "layout": layout, "magnitude": a.magnitude, "hip_ms": float(np.median(t)),
                              "pillow_host_ms": float(np.median(host)), "speedup": float(np.median(host) / np.median(t)),
                              "bytes_equal_pillow": exact, "hip_ms_all": [round(v, 4) for v in t],
                              "pillow_host_ms_all": [round(v, 2) for v in host]}), flush=True)


if __name__ == "__main__":
    main()
