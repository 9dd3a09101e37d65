"""Generates tests/golden/g25_ragged.npz with Pillow alone: what the reference's 224 x 224 chains (`main/train_imagenet.py:30-41`,
`train_cub.py`, `train_dtd.py`, `train_mvtec.py`, `train_custom.py`: Resize(256) -> ColorJitter -> RandomCrop(224) ...; test:
Resize(256) -> CenterCrop(224)) do to images of mixed sizes, at a target of 16.  Run by hand where Pillow is available; the tests only
read the .npz.

    python tests/golden/make_golden_ragged.py

torchvision is not installed where this was made, so Pillow is called directly, with the calls torchvision makes on PIL images:
`Resize(n)` -> `img.resize((w, h), filter)` with (h, w) by torchvision's shorter-side rule (restated below, independently of the
product), the image itself when its shorter side is n already; `Resize((h, w))` -> `img.resize((w, h), filter)`; `CenterCrop(n)` ->
the window at int(round((H - n) / 2.0)); ColorJitter -> ImageEnhance.Brightness / Contrast / Color and the HSV round trip, as
tests/golden/make_golden.py g14 does; RandomCrop's zero padding follows the jitter.
Inputs: tests/ragged_util.py (an integer formula).  Recorded per filter (bilinear, bicubic), channel count (1, 3) and image:
r/ the Resize(16) result, cc/ its CenterCrop(16), p/ the Resize((16, 16)) result; jit/k the three ColorJitter + crop cases; the
Pillow version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
import ragged_util as ru   # noqa: E402

FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def to_pil(a: np.ndarray):
    return Image.fromarray(a[..., 0], mode="L") if a.shape[2] == 1 else Image.fromarray(a, mode="RGB")


def to_np(im, C: int) -> np.ndarray:
    a = np.asarray(im, dtype=np.uint8)
    return a.reshape(a.shape[0], a.shape[1], C)


def tv_resize(a: np.ndarray, size, filt: str) -> np.ndarray:
    """torchvision.transforms.functional.resize on a PIL image"""
    H, W, C = a.shape
    if isinstance(size, int):
        short, long = (W, H) if W <= H else (H, W)
        if short == size:
            return a
        new_short, new_long = size, int(size * long / short)
        w, h = (new_short, new_long) if W <= H else (new_long, new_short)
    else:
        h, w = size
    return to_np(to_pil(a).resize((w, h), FILTERS[filt]), C)


def tv_hue(img, hue_factor):                              # torchvision.transforms.functional_pil.adjust_hue
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(int(hue_factor * 255) & 0xFF)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


OPS = [lambda im, f: ImageEnhance.Brightness(im).enhance(f), lambda im, f: ImageEnhance.Contrast(im).enhance(f),
       lambda im, f: ImageEnhance.Color(im).enhance(f), tv_hue]


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for C in (1, 3):
        for filt in ru.FILTERS:
            for i, a in enumerate(ru.images(C)):
                r = tv_resize(a, ru.TARGET, filt)
                assert r.shape[:2] == ru.RESIZED[i], (i, r.shape)
                out[f"r/{filt}/c{C}/{i}"] = r
                out[f"cc/{filt}/c{C}/{i}"] = np.ascontiguousarray(ru.center_crop(r, ru.TARGET))
                out[f"p/{filt}/c{C}/{i}"] = tv_resize(a, (ru.TARGET, ru.TARGET), filt)
    # float32 as the draws are: sample_color_jitter hands fp32 factors to the kernel, Pillow gets the same numbers as Python floats
    for k, (i, order, factors, (top, left), flip) in enumerate(ru.JITTER):
        f32 = np.asarray(factors, dtype=np.float32)
        pim = to_pil(out[f"r/bilinear/c3/{i}"])
        for op in order:
            pim = OPS[op](pim, float(f32[op]))
        out[f"jit/{k}"] = ru.crop_flip(to_np(pim, 3), top, left, flip, ru.TARGET, True)
    path = os.path.join(HERE, "g25_ragged.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
