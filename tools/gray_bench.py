"""Times the 1-channel input path (eoe_amd.data.grayscale_u8 and the one-channel augment kernel, csrc/augment.hip) against the
same work in stock torch ops on the device, on the same box in the same run, at the Fashion-MNIST workload's sizes.

  grayscale  `grayscale_u8` on 50 000 x 32 x 32 x 3 (CIFAR-100 as outlier exposure, converted once per resident set) against
             `((x.to(int32) * w).sum(-1) + 0x8000) >> 16` cast back to uint8 (the same integer formula, so the outputs are compared
             for equality).  Achieved bytes / s count one read of the colour set and one write of the gray set and stand next to
             the box's copy rate (eoe_probe_copy over 256 MiB, read + write).
  step       `augment_batch` on a resident 1-channel set for one half of a step batch, 128 x 28 x 28 from 28 x 28 sources with
             padding 3 (and from 32 x 32 sources, the OE half), against the torch-op chain on the device: gather by index, zero
             pad, per-sample crop through an index grid, flip through the same grid, / 255, + 0.001 * randn, Normalize.  The
             torch side draws its noise with torch.randn (another generator, same cost class), so only the noise-free outputs
             are compared.
A warm-up, then repeats alternating HIP and torch; each repeat times a window of >= --window seconds of back-to-back calls with
device events; medians over the repeats.  One JSON line per case.

  python tools/gray_bench.py [--repeats 5] [--window 0.5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd import _lib                                   # noqa: E402
from eoe_amd.data import augment_batch, grayscale_u8       # noqa: E402


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


def torch_grayscale(x, w):
    return (((x.to(torch.int32) * w).sum(-1, keepdim=True) + 0x8000) >> 16).to(torch.uint8)


def torch_augment(src, params, crop, pad, mean, std, noise_std):
    """the chain in torch ops: src uint8 [n_src, H, W, 1], params int64 [n, 4] = (index, top, left, flip), flip first"""
    n = params.shape[0]
    x = torch.nn.functional.pad(src[params[:, 0], :, :, 0], (pad, pad, pad, pad))                       # [n, H + 2p, W + 2p], zeros
    ar = torch.arange(crop, device=src.device)
    ys = (params[:, 1] + pad)[:, None] + ar[None, :]                                                    # [n, crop]
    cols = params[:, 2][:, None] + ar[None, :]                                                          # in the flipped source
    W = src.shape[2]
    xs = torch.where(params[:, 3][:, None] > 0, W - 1 - cols, cols) + pad
    # a flipped source column outside [0, W) is padding on the other side: W - 1 - c + pad stays inside the padded row
    out = x[torch.arange(n, device=src.device)[:, None, None], ys[:, :, None], xs[:, None, :]]
    out = out.to(torch.float32).div(255.0).unsqueeze(1)
    if noise_std > 0:
        out = out + noise_std * torch.randn_like(out)
    return (out - mean) / std


def alternate(hip, ref, repeats, window):
    for _ in range(3):
        hip(), ref()
    th, tr = [], []
    for _ in range(repeats):
        th.append(window_ms(hip, window))
        tr.append(window_ms(ref, window))
    return th, tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    copy_gbs = copy_rate_gbs(a.window)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "copy_kernel_gbs": round(copy_gbs, 1)}), flush=True)

    colour = torch.randint(0, 256, (50000, 32, 32, 3), generator=g, device="cuda", dtype=torch.uint8)
    w = torch.tensor([19595, 38470, 7471], dtype=torch.int32, device="cuda")
    equal = bool(torch.equal(grayscale_u8(colour), torch_grayscale(colour, w)))
    th, tr = alternate(lambda: grayscale_u8(colour), lambda: torch_grayscale(colour, w), a.repeats, a.window)
    nbytes = 4.0 * colour.shape[0] * 32 * 32
    print(json.dumps({"case": "grayscale_u8", "shape": list(colour.shape), "hip_ms": float(np.median(th)), "torch_ms": float(np.median(tr)),
                      "speedup": float(np.median(tr) / np.median(th)), "hip_gbs": nbytes / (np.median(th) * 1e-3) / 1e9,
                      "copy_kernel_gbs": round(copy_gbs, 1), "outputs_equal": equal,
                      "hip_ms_all": [round(t, 4) for t in th], "torch_ms_all": [round(t, 4) for t in tr]}), flush=True)
    del colour

    n, crop, pad = 128, 28, 3
    mean, std = [0.2861], [0.3530]
    mean_t, std_t = torch.tensor(mean, device="cuda").view(1, 1, 1, 1), torch.tensor(std, device="cuda").view(1, 1, 1, 1)
    for hw in (28, 32):
        src = torch.randint(0, 256, (50000, hw, hw, 1), generator=g, device="cuda", dtype=torch.uint8)
        p64 = torch.stack([torch.randint(0, 50000, (n,), generator=g, device="cuda"),
                           torch.randint(-pad, hw + pad - crop + 1, (n,), generator=g, device="cuda"),
                           torch.randint(-pad, hw + pad - crop + 1, (n,), generator=g, device="cuda"),
                           torch.randint(0, 2, (n,), generator=g, device="cuda")], dim=1)
        p32 = p64.to(torch.int32).contiguous()
        diff = float((augment_batch(src, p32, (crop, crop), mean, std, True, 0.0, 0)
                      - torch_augment(src, p64, crop, pad, mean_t, std_t, 0.0)).abs().max())
        hip = lambda: augment_batch(src, p32, (crop, crop), mean_t.view(1), std_t.view(1), True, 0.001, 7)      # noqa: E731
        ref = lambda: torch_augment(src, p64, crop, pad, mean_t, std_t, 0.001)                                  # noqa: E731
        th, tr = alternate(hip, ref, a.repeats, a.window)
        print(json.dumps({"case": "augment_batch_c1", "batch": n, "source": hw, "crop": crop, "padding": pad,
                          "hip_ms": float(np.median(th)), "torch_ms": float(np.median(tr)), "speedup": float(np.median(tr) / np.median(th)),
                          "max_abs_diff_without_noise": diff, "hip_ms_all": [round(t, 4) for t in th],
                          "torch_ms_all": [round(t, 4) for t in tr]}), flush=True)


if __name__ == "__main__":
    main()
