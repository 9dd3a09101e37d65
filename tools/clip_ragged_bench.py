"""Times CLIP's own transform on RAW images of mixed sizes (Resize(224, BICUBIC) with the aspect ratio kept, CenterCrop(224):
`clip_official/clip/clip.py:58-65`, what the test split of the 224 x 224 CLIP runners gets) on the device, on one box in one run, over
--images synthetic images with the shape distribution of tools/ragged_bench.py:

  windowed   `data.clip_preprocess_ragged`: each pass of the ragged Resize writes only the CenterCrop window, the horizontal pass runs
             only over the source rows the vertical window's taps touch
  composed   what there was: `resize_u8(set, 224, "bicubic")` of every whole image, then the ragged centre crop (`crop_flip_u8`)
  pillow     a host loop, `Image.resize((w', h'), BICUBIC)` and a crop, one image at a time (skipped where Pillow is missing)

The whole calls are timed with a host clock around a device synchronise (plan and tap tables on the host, uploads, launches), the two
device forms alternated repeat by repeat; "launches" times the kernel launches alone from plans and tables made beforehand
(device events over a window of back-to-back repeats).  The three results are compared byte for byte: windowed against composed on
every image, both against Pillow on the first --check images.  One JSON line per part.

  python tools/clip_ragged_bench.py [--images 1000] [--repeats 5] [--window 0.5] [--check 40] [--n-px 224]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd import _lib, data                     # noqa: E402
from ragged_bench import shapes, window_ms         # noqa: E402  (the same shape distribution and timing window)


def composed(raw, n_px):
    full = data.resize_u8(raw, n_px, "bicubic")
    tl = torch.from_numpy(data.center_origins(full.sizes, n_px))
    idx = torch.arange(len(full))
    p = torch.stack([idx, tl[:, 0], tl[:, 1], torch.zeros_like(idx)], dim=1).to(torch.int32).to(raw.device)
    return data.crop_flip_u8(full, p, (n_px, n_px), True)


def launches(raw, n_px, window):
    """(a function that enqueues the pass launches of a plan made once, the plan): tables and descriptors are on the device already"""
    taps = data._TapArena(_lib.EOE_RESIZE_BICUBIC)
    plan = data.ragged_resize_plan(raw.sizes, 3, n_px, taps, raw.offsets_host, window is not None, window)
    dev, st = raw.device, torch.cuda.current_stream().cuda_stream
    taps_dev = taps.tensor().to(dev)
    mid = torch.empty(plan["mid_bytes"], dtype=torch.uint8, device=dev)
    out = torch.empty(plan["out_bytes"], dtype=torch.uint8, device=dev)
    steps = []
    for name, src, dst in (("h", raw.arena, mid), ("v", mid, out)):
        offs, desc, biggest = plan[name]
        steps.append((src, dst, torch.from_numpy(offs).to(dev), torch.from_numpy(desc).to(dev), biggest))

    def run():
        for src, dst, offs, desc, biggest in steps:
            _lib.check(_lib.lib.eoe_ragged_resize_pass_u8(src.data_ptr(), dst.data_ptr(), offs.data_ptr(), desc.data_ptr(),
                                                          taps_dev.data_ptr(), len(raw), biggest, st), "eoe_ragged_resize_pass_u8")
    return run, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--check", type=int, default=40)
    ap.add_argument("--n-px", type=int, default=224)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    hw = shapes(a.images, rng)
    imgs = []
    for H, W in hw:                                          # the images of tools/ragged_bench.py
        small = rng.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3), dtype=np.uint8)
        imgs.append(np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.uint8))[:H, :W] ^ rng.integers(0, 8, (H, W, 3), dtype=np.uint8)))
    raw = data.RaggedImageSet(imgs, device="cuda")
    px = a.n_px
    win = data.clip_window(raw.sizes, px)
    full = np.array([data.resized_hw(h, w, px) for h, w in hw], dtype=np.int64)
    print(json.dumps({"box": torch.cuda.get_device_name(0), "images": len(raw), "raw_mb": round(raw.arena.numel() / 1e6, 1),
                      "distinct_shapes": len(set(hw)), "n_px": px,
                      "resized_mb": round(float((full[:, 0] * full[:, 1] * 3).sum()) / 1e6, 1), "window_mb": round(len(raw) * px * px * 3 / 1e6, 1)}),
          flush=True)

    # ---- the whole calls
    w_out, c_out = data.clip_preprocess_ragged(raw, px), composed(raw, px)
    torch.cuda.synchronize()
    equal_dev = bool(torch.equal(w_out, c_out))
    t_w, t_c = [], []
    for _ in range(a.repeats):
        for fn, ts in ((lambda: data.clip_preprocess_ragged(raw, px), t_w), (lambda: composed(raw, px), t_c)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    pil_ms, equal_pil = None, None
    try:
        from PIL import Image
        t0 = time.perf_counter()
        ref = []
        for im, (h, w), (top, left, _, _) in zip(imgs, full.tolist(), win.tolist()):
            ref.append(np.asarray(Image.fromarray(im).resize((w, h), Image.BICUBIC))[top:top + px, left:left + px])
        pil_ms = (time.perf_counter() - t0) * 1e3
        k = min(a.check, len(ref))
        equal_pil = bool(np.array_equal(w_out[:k].cpu().numpy(), np.stack(ref[:k])))
    except ImportError:
        pass
    mw, mc = float(np.median(t_w)), float(np.median(t_c))
    print(json.dumps({"part": "calls", "windowed_ms": mw, "composed_ms": mc, "composed_over_windowed": mc / mw,
                      "windowed_ms_all": [round(t, 2) for t in t_w], "composed_ms_all": [round(t, 2) for t in t_c],
                      "pillow_loop_ms": pil_ms, "pillow_over_windowed": None if pil_ms is None else pil_ms / mw,
                      "windowed_equals_composed": equal_dev, "windowed_equals_pillow": equal_pil}), flush=True)

    # ---- the launches alone
    run_w, plan_w = launches(raw, px, win)
    run_f, plan_f = launches(raw, px, None)
    for _ in range(3):
        run_w(), run_f()
    l_w, l_f = [], []
    for _ in range(a.repeats):
        l_w.append(window_ms(run_w, a.window))
        l_f.append(window_ms(run_f, a.window))
    rows_kept = float(plan_w["mid_sizes"][:, 0].sum()) / float(raw.sizes[:, 0].sum())
    print(json.dumps({"part": "launches", "windowed_ms": float(np.median(l_w)), "whole_resize_ms": float(np.median(l_f)),
                      "whole_over_windowed": float(np.median(l_f) / np.median(l_w)),
                      "windowed_ms_all": [round(t, 4) for t in l_w], "whole_ms_all": [round(t, 4) for t in l_f],
                      "windowed_mid_mb": round(plan_w["mid_bytes"] / 1e6, 1), "whole_mid_mb": round(plan_f["mid_bytes"] / 1e6, 1),
                      "windowed_out_mb": round(plan_w["out_bytes"] / 1e6, 1), "whole_out_mb": round(plan_f["out_bytes"] / 1e6, 1),
                      "source_rows_kept": round(rows_kept, 4)}), flush=True)


if __name__ == "__main__":
    main()
