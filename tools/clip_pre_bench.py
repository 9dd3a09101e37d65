"""Times CLIP's preprocessing inside the train chain (eoe_amd.data.augment_resize_batch, csrc/augment.hip: crop / flip, Pillow's bicubic
upsample, L -> RGB, ToTensor, noise, Normalize in one launch) against the same work composed from the kernels that were there
before it, on the same box in the same run, at the sizes of the reference's small-image CLIP runners:

  rgb32   256 slots, 32 x 32 x 3 crops (padding 4) of a 50 000-image set -> 224 x 224   (main/train_clip_cifar.py)
  gray28  256 slots, 28 x 28 x 1 crops (padding 3) of a 60 000-image set -> 224 x 224   (main/train_clip_fmnist.py)

  fused     one `augment_resize_batch`
  composed  `crop_flip_u8 -> resize_u8 -> [channel repeat] -> augment_batch` with identity params: four launches (five for gray), two
            uint8 intermediates, the tap tables rebuilt on the host and uploaded in every call (what `resize_u8` does)

Both produce the same bits (checked here before anything is timed).  A warm-up, then repeats alternating the two; each repeat times a
window of >= --window seconds of back-to-back calls with device events; medians over the repeats.  Bytes: the fused kernel's
algorithmic traffic is the crops read plus the fp32 batch written; the rate stands next to the box's copy rate (eoe_probe_copy over
256 MiB, read + write).  One JSON line per case.

  python tools/clip_pre_bench.py [--repeats 5] [--window 0.5]"""
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
from eoe_amd.data import CLIP_MEAN, CLIP_STD, augment_batch, augment_resize_batch, crop_flip_u8, resize_u8   # noqa: E402


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


def composed(src, p, ident, S, P, mean, std, flip_first, noise_std, seed):
    u8 = resize_u8(crop_flip_u8(src, p, (S, S), flip_first), (P, P), "bicubic")
    if u8.shape[3] == 1:
        u8 = u8.repeat(1, 1, 1, 3).contiguous()
    return augment_batch(u8, ident, (P, P), mean, std, True, noise_std, seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    copy_gbs = copy_rate_gbs(a.window)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "copy_kernel_gbs": round(copy_gbs, 1)}), flush=True)
    mean, std = torch.tensor(CLIP_MEAN, device="cuda"), torch.tensor(CLIP_STD, device="cuda")
    n, P = 256, 224
    for case, n_src, S, C, pad, flip_first in (("rgb32", 50000, 32, 3, 4, False), ("gray28", 60000, 28, 1, 3, True)):
        src = torch.randint(0, 256, (n_src, S, S, C), generator=g, device="cuda", dtype=torch.uint8)
        p = torch.stack([torch.randint(0, n_src, (n,), generator=g, device="cuda"),
                         torch.randint(-pad, pad + 1, (n,), generator=g, device="cuda"),
                         torch.randint(-pad, pad + 1, (n,), generator=g, device="cuda"),
                         torch.randint(0, 2, (n,), generator=g, device="cuda")], dim=1).to(torch.int32).contiguous()
        ident = torch.zeros_like(p)
        ident[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
        fused = lambda: augment_resize_batch(src, p, S, P, mean, std, flip_first, 0.001, 7)              # noqa: E731
        chain = lambda: composed(src, p, ident, S, P, mean, std, flip_first, 0.001, 7)                   # noqa: E731
        equal = bool(torch.equal(fused(), chain()))
        for _ in range(3):
            fused(), chain()
        tf, tc = [], []
        for _ in range(a.repeats):
            tf.append(window_ms(fused, a.window))
            tc.append(window_ms(chain, a.window))
        # without the noise: what the memory system alone allows (the noise is ~100 VALU operations per output element in both forms)
        tf0 = window_ms(lambda: augment_resize_batch(src, p, S, P, mean, std, flip_first, 0.0, 7), a.window)
        tc0 = window_ms(lambda: composed(src, p, ident, S, P, mean, std, flip_first, 0.0, 7), a.window)
        nbytes = float(n * S * S * C + 4 * n * 3 * P * P)
        print(json.dumps({"case": case, "slots": n, "crop": S, "channels": C, "n_px": P, "fused_ms": float(np.median(tf)),
                          "composed_ms": float(np.median(tc)), "speedup": float(np.median(tc) / np.median(tf)),
                          "fused_gbs": nbytes / (np.median(tf) * 1e-3) / 1e9, "copy_kernel_gbs": round(copy_gbs, 1),
                          "fused_ms_without_noise": tf0, "composed_ms_without_noise": tc0, "outputs_equal": equal,
                          "fused_ms_all": [round(t, 4) for t in tf], "composed_ms_all": [round(t, 4) for t in tc]}), flush=True)
        del src


if __name__ == "__main__":
    main()
