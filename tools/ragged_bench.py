"""Times the ragged image sets (eoe_amd.data.RaggedImageSet, csrc/augment.hip) on the device, on one box in one run:

  (a) resize   Resize(256, bilinear) of --images synthetic images with ImageNet-like shapes (most around 500 x 375 and 375 x 500, a
               few extremes) as ONE ragged `resize_u8` -- two launches for the whole set, the tap tables built once per distinct
               (in, out) on the host -- against a host Pillow loop over the same images (`Image.resize`, one image at a time; skipped
               where Pillow is missing).  The results are compared byte for byte on the first --check images.
  (b) augment  the ragged `augment_batch` at 256 slots of 224 x 224 out of that resized set (per-image legal origins) against the
               unchanged uniform `augment_batch` at 256 slots of 224 x 224 out of a [n, 256, 256, 3] tensor.  The two move the
               same bytes; they are interleaved, repeat by repeat.  With and without the noise (the noise is ~100 VALU operations per
               output element in both, the gather shows without it).

A warm-up, then repeats; each repeat times a window of >= --window seconds of back-to-back calls with device events; medians over the
repeats.  One JSON line per part.

  python tools/ragged_bench.py [--images 1000] [--repeats 5] [--window 0.5] [--check 40]"""
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
from eoe_amd.data import RaggedImageSet, augment_batch, ragged_crop_origins, resize_u8, resized_hw   # noqa: E402


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


def shapes(n, rng):
    """(H, W) per image: 45 % about 375 x 500, 35 % about 500 x 375, the rest anything from 120 to 1600 px a side"""
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.45:
            out.append((375 + int(rng.integers(-40, 41)), 500 + int(rng.integers(-20, 21))))
        elif u < 0.80:
            out.append((500 + int(rng.integers(-20, 21)), 375 + int(rng.integers(-40, 41))))
        else:
            out.append((int(rng.integers(120, 1601)), int(rng.integers(120, 1601))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--check", type=int, default=40)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    hw = shapes(a.images, rng)
    # smooth images with some texture: a random 1/8-size image blown up, so that Pillow and the kernel see something image-like
    imgs = []
    for H, W in hw:
        small = rng.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3), dtype=np.uint8)
        imgs.append(np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.uint8))[:H, :W] ^ rng.integers(0, 8, (H, W, 3), dtype=np.uint8)))
    raw = RaggedImageSet(imgs, device="cuda")
    print(json.dumps({"box": torch.cuda.get_device_name(0), "images": len(raw), "raw_mb": round(raw.arena.numel() / 1e6, 1),
                      "distinct_shapes": len(set(hw))}), flush=True)

    # ---- (a) Resize(256)
    out = resize_u8(raw, 256, "bilinear")
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(a.repeats):                                 # the whole call: plan and tap tables on the host, two launches
        t0 = time.perf_counter()
        out = resize_u8(raw, 256, "bilinear")
        torch.cuda.synchronize()
        t_dev.append((time.perf_counter() - t0) * 1e3)
    pil_ms, equal = None, None
    try:
        from PIL import Image
        t0 = time.perf_counter()
        ref = []
        for im in imgs:
            h, w = resized_hw(im.shape[0], im.shape[1], 256)
            ref.append(np.asarray(Image.fromarray(im).resize((w, h), Image.BILINEAR)))
        pil_ms = (time.perf_counter() - t0) * 1e3
        equal = all(np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(min(a.check, len(ref))))
    except ImportError:
        pass
    print(json.dumps({"part": "resize", "images": len(raw), "device_ms": float(np.median(t_dev)), "device_ms_all": [round(t, 2) for t in t_dev],
                      "pillow_loop_ms": pil_ms, "pillow_ms_per_256": None if pil_ms is None else pil_ms * 256 / len(raw),
                      "speedup": None if pil_ms is None else pil_ms / float(np.median(t_dev)), "bytes_equal_to_pillow": equal,
                      "resized_mb": round(out.arena.numel() / 1e6, 1)}), flush=True)

    # ---- (b) augment_batch, 256 slots of 224 x 224
    n, S = 256, 224
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, len(out), (n,), generator=g)
    tl = ragged_crop_origins(out.sizes[idx.numpy()], S, 0, g)
    flip = torch.randint(0, 2, (n,), generator=g)
    p_r = torch.stack([idx, tl[:, 0], tl[:, 1], flip], dim=1).to(torch.int32).cuda()
    uni = torch.randint(0, 256, (len(out), 256, 256, 3), dtype=torch.uint8, device="cuda")
    p_u = torch.stack([idx, torch.randint(0, 256 - S + 1, (n,), generator=g), torch.randint(0, 256 - S + 1, (n,), generator=g), flip],
                      dim=1).to(torch.int32).cuda()
    mean, std = torch.tensor([0.485, 0.456, 0.406], device="cuda"), torch.tensor([0.229, 0.224, 0.225], device="cuda")
    res = {"part": "augment", "slots": n, "crop": S}
    for tag, noise in (("", 0.001), ("_without_noise", 0.0)):
        ragged = lambda: augment_batch(out, p_r, (S, S), mean, std, False, noise, 7)         # noqa: E731
        uniform = lambda: augment_batch(uni, p_u, (S, S), mean, std, False, noise, 7)        # noqa: E731
        for _ in range(3):
            ragged(), uniform()
        tr, tu = [], []
        for _ in range(a.repeats):
            tr.append(window_ms(ragged, a.window))
            tu.append(window_ms(uniform, a.window))
        nbytes = float(n * S * S * 3 + 4 * n * 3 * S * S)
        res.update({f"ragged_ms{tag}": float(np.median(tr)), f"uniform_ms{tag}": float(np.median(tu)),
                    f"ragged_over_uniform{tag}": float(np.median(tr) / np.median(tu)),
                    f"ragged_gbs{tag}": nbytes / (np.median(tr) * 1e-3) / 1e9,
                    f"ragged_ms_all{tag}": [round(t, 4) for t in tr], f"uniform_ms_all{tag}": [round(t, 4) for t in tu]})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
