"""Times the per-task normalisation kernels (eoe_amd.normalize, csrc/normstats.hip) against the reference's formulation on the
same box in the same run.

  operator   `gcn_normalize` (GCN l1 + the per-channel affine, one launch) against the same operator in stock torch ops on the
             device (tests/normstats_util.py::torch_gcn_normalize: row mean, sub_, abs().mean, div_, then sub_ / div_ per
             channel) at 256 x 3 x 224 x 224 and 256 x 3 x 32 x 32, fp32.  Like for like: BOTH sides work in place on a scratch
             batch of their own that is normalised again and again (the values stay finite and the cost does not depend on
             them), so neither side pays for a copy or an allocation of the batch.  A warm-up, then repeats alternating HIP and
             torch; each repeat times a window of >= --window seconds of back-to-back calls with device events; medians over the
             repeats.  The outputs are compared once, out of place, on the fresh batch.  The achieved bytes / s
             count the operator's algorithmic traffic (one read, one write of the batch) and stand next to the box's copy rate
             (eoe_probe_copy over 256 MiB, read + write).
  fit        `fit_statistics` (statistics kernel + host recurrence, device events do not see the host part: wall clock around a
             synchronise) on 1 300 images of 256 x 256 x 3 and 5 000 of 32 x 32 x 3 resident on the device, against the
             reference's host loop restated with torch on the CPU (batches of two through RunningStats; per-image GCN, then
             min / max), both modes; the host loop is timed three times, median.
One JSON line per case.

  python tools/norm_bench.py [--repeats 5] [--window 0.5] [--skip-fit]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the torch yardsticks live with the test helpers
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd import _lib                                                          # noqa: E402
from eoe_amd.normalize import fit_statistics, gcn_normalize                        # noqa: E402
from normstats_util import torch_gcn_normalize                                     # noqa: E402


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


def copy_rate_gbs(window_s):
    """the box's copy-kernel rate, bytes read + written per second"""
    nbytes = 256 << 20
    src = torch.empty(nbytes // 4, device="cuda").normal_()
    dst = torch.empty_like(src)
    s = torch.cuda.current_stream().cuda_stream
    fn = lambda: _lib.check(_lib.lib.eoe_probe_copy(dst.data_ptr(), src.data_ptr(), nbytes, s), "eoe_probe_copy")   # noqa: E731
    fn()
    return 2.0 * nbytes / (window_ms(fn, window_s) * 1e-3) / 1e9


def host_fit(u8: torch.Tensor, mode: str):
    """the host-side fit the device path replaces, with torch on the CPU in fp32: the running statistics over pairs of images, or
    every image contrast-normalised on its own and the extremes of the lot"""
    imgs = u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
    if mode == "normalize":
        channels = imgs.shape[1]
        avg, spread, groups = torch.zeros(channels), torch.zeros(channels), 0
        for start in range(0, imgs.shape[0], 2):
            vals = imgs[start:start + 2].movedim(1, -1).reshape(-1, channels)
            groups += 1
            before = avg
            avg = before + (vals.mean(dim=0) - before) / groups
            spread = spread + ((vals - avg) * (vals - before)).mean(dim=0)
        return avg.tolist(), (spread / groups).sqrt().tolist()
    lo, hi = float("inf"), float("-inf")
    for one in imgs:
        centred = one - one.mean()
        centred = centred / centred.abs().mean()
        lo, hi = min(lo, float(centred.min())), max(hi, float(centred.max()))
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--skip-fit", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    copy_gbs = copy_rate_gbs(a.window)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "copy_kernel_gbs": round(copy_gbs, 1)}), flush=True)
    shift, rng = [-1.7, -1.7, -1.7], [3.9, 3.9, 3.9]
    for shape in ((256, 3, 224, 224), (256, 3, 32, 32)):
        x = torch.rand(shape, generator=g, device="cuda")
        sh = torch.tensor(shift, device="cuda")
        rg = torch.tensor(rng, device="cuda")
        yh, yr = gcn_normalize(x, "l1", sh, rg), torch_gcn_normalize(x, "l1", sh, rg)
        torch.cuda.synchronize()
        diff = float((yh - yr).abs().max())
        del yh, yr
        buf_h, buf_r = x.clone(), x.clone()                                                   # one scratch batch per side
        hip = lambda: gcn_normalize(buf_h, "l1", sh, rg, out=buf_h)                            # noqa: E731
        ref = lambda: torch_gcn_normalize(buf_r, "l1", sh, rg, inplace=True)                   # noqa: E731
        for _ in range(3):
            hip(), ref()
        th, tr = [], []
        for _ in range(a.repeats):
            th.append(window_ms(hip, a.window))
            tr.append(window_ms(ref, a.window))
        nbytes = 2.0 * x.numel() * 4
        print(json.dumps({"case": "gcn_normalize", "shape": list(shape), "hip_ms": float(np.median(th)), "torch_ms": float(np.median(tr)),
                          "speedup": float(np.median(tr) / np.median(th)), "hip_gbs": nbytes / (np.median(th) * 1e-3) / 1e9,
                          "torch_gbs": nbytes / (np.median(tr) * 1e-3) / 1e9, "copy_kernel_gbs": round(copy_gbs, 1),
                          "max_abs_diff": diff, "hip_ms_all": [round(t, 4) for t in th], "torch_ms_all": [round(t, 4) for t in tr]}),
              flush=True)
    if a.skip_fit:
        return
    cpu_g = torch.Generator().manual_seed(0)
    for n, hw in ((1300, 256), (5000, 32)):
        u8 = torch.randint(0, 256, (n, hw, hw, 3), generator=cpu_g, dtype=torch.uint8)
        dev = u8.cuda()
        for mode in ("normalize", "gcn-normalize"):
            fit_statistics(dev, None, mode)
            th = []
            for _ in range(a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = fit_statistics(dev, None, mode)
                th.append((time.perf_counter() - t0) * 1e3)
            t_hosts = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = host_fit(u8, mode)
                t_hosts.append((time.perf_counter() - t0) * 1e3)
            t_host = float(np.median(t_hosts))
            got = (st["mean"], st["std"]) if mode == "normalize" else (st["mean"][0], st["mean"][0] + st["std"][0])
            dev_rel = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.abs(np.asarray(want, np.float64))))
            print(json.dumps({"case": "fit_statistics", "mode": mode, "images": n, "size": hw, "hip_ms": float(np.median(th)),
                              "host_loop_ms": t_host, "speedup": t_host / float(np.median(th)), "max_rel_diff_to_host_fp32": dev_rel,
                              "hip_ms_all": [round(t, 3) for t in th],
                              "host_loop_ms_all": [round(t, 1) for t in t_hosts]}), flush=True)


if __name__ == "__main__":
    main()
