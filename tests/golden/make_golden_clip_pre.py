"""Generates tests/golden/g24_clip_pre.npz with Pillow: what 'clip_pil_preprocessing' of the reference's small-image CLIP runners
(`main/train_clip_cifar.py:26-35`, `train_clip_fmnist.py:27-36`, `train_clip_mnist.py:25-29`; the transform itself:
`training/clip.py:34-43`, `clip_official/clip/clip.py:58-65`) does to the PIL image that RandomCrop / RandomHorizontalFlip hand it:
Resize(n_px, BICUBIC) -> CenterCrop(n_px) -> convert("RGB").  Run by hand where Pillow is available; the tests only read the .npz.

    python tests/golden/make_golden_clip_pre.py

torchvision is not installed where this was made, so Pillow is called directly, with the calls torchvision makes on PIL images:
`Resize(n)` of a square image -> `img.resize((n, n), BICUBIC)`; `CenterCrop(n)` of an n x n image cuts nothing; `convert("RGB")`.
Inputs (tests/clip_pre_util.py FIXTURE_CASES): two random 32 x 32 RGB crops -> 224 and one 28 x 28 L crop -> 224 -> RGB (the CIFAR-10 and
the Fashion-MNIST / MNIST chains), and small odd cases: 9 -> 23 in RGB and L, 9 -> 23 bilinear, 12 -> 12.  Recorded: the RGB result
per case; the Pillow version."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
import clip_pre_util as cu   # noqa: E402

FILTERS = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def pil_clip_pre(crop: np.ndarray, n_px: int, filt: str) -> np.ndarray:
    im = Image.fromarray(crop[..., 0], mode="L") if crop.shape[2] == 1 else Image.fromarray(crop, mode="RGB")
    im = im.resize((n_px, n_px), FILTERS[filt]).convert("RGB")
    out = np.asarray(im, dtype=np.uint8)
    assert out.shape == (n_px, n_px, 3)
    return out


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for case, (_, _, _, P, filt) in cu.FIXTURE_CASES.items():
        out[case] = np.stack([pil_clip_pre(c, P, filt) for c in cu.fixture_crops(case)])
    path = os.path.join(HERE, "g24_clip_pre.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
