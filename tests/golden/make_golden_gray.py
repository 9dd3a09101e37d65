"""Generates tests/golden/g22_gray.npz with Pillow: what the reference's 1-channel transform chain (`main/train_fmnist.py:31-38`:
Grayscale(1) -> RandomHorizontalFlip -> RandomCrop(28, padding=3) -> ToTensor -> noise -> 'normalize') does to PIL images up to
ToTensor.  Run by hand where the reference and Pillow are available; the tests only read the .npz.

    python tests/golden/make_golden_gray.py <the reference's src/eoe directory>

The reference directory is only read to check that the chain restated here is the one its runner builds (the transforms named in
`main/train_fmnist.py`, and the empty chain of `main/train_mnist.py`).  torchvision is not installed where this was made, so Pillow
is called directly, with the calls torchvision makes on PIL images (torchvision/transforms/_functional_pil.py; named by function,
since the file is not at hand to cite lines):
  * `Grayscale(1)` -> `to_grayscale`: `img.convert("L")`;
  * `RandomCrop(S, padding=p)` -> `pad` (constant mode, fill 0): `ImageOps.expand(img, border=p, fill=0)`, then `crop`:
    `img.crop((left, top, left + width, top + height))` in the padded image;
  * `RandomHorizontalFlip` -> `hflip`: `img.transpose(Image.FLIP_LEFT_RIGHT)`.
Crop origins in the fixture's rows are relative to the UNPADDED image (they may be negative), as the kernels take them.

Inputs (tests/gray_util.py): 24 colour images of 32 x 32 x 3 (image 0 starts with white, black, red, green, blue; image 1 with
colours whose weighted sum sits on a rounding boundary k * 65536 - 0x8000 + {-1, 0, 1}), 24 gray images of 28 x 28, 4 of 6 x 5.
Recorded: the L image of every colour image; per crop case and row both orders, flip-then-crop (`main/train_fmnist.py`,
`main/train_cifar.py`) and crop-then-flip (`main/train_clip_imagenet.py`); the Pillow version.
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
import gray_util as gu   # noqa: E402


def check_reference(ref: str):
    with open(os.path.join(ref, "main", "train_fmnist.py")) as f:
        txt = f.read()
    chain = ["transforms.Grayscale(1)", "transforms.RandomHorizontalFlip(p=0.5)", "transforms.RandomCrop(28, padding=3)",
             "transforms.ToTensor()", "x + 0.001 * torch.randn_like(x)", "'normalize'"]
    at = [txt.index(c) for c in chain]
    assert at == sorted(at), "the FMNIST chain is not in the order restated here"
    with open(os.path.join(ref, "main", "train_mnist.py")) as f:
        txt = "".join(f.read().split())
    assert "train_transform=transforms.Compose([])" in txt, "the MNIST chain is not empty"


def pil_crop_flip(img: np.ndarray, top: int, left: int, flip: int, out_hw, pad: int, flip_first: bool) -> np.ndarray:
    im = Image.fromarray(img, mode="L")
    if flip_first and flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    im = ImageOps.expand(im, border=pad, fill=0)
    Ho, Wo = out_hw
    im = im.crop((left + pad, top + pad, left + pad + Wo, top + pad + Ho))
    if (not flip_first) and flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    out = np.asarray(im, dtype=np.uint8)
    assert out.shape == (Ho, Wo)
    return out


def main():
    check_reference(sys.argv[1])
    out = {"pillow_version": np.array(PIL.__version__)}
    colour = gu.colour_set()
    out["L"] = np.stack([np.asarray(Image.fromarray(c, mode="RGB").convert("L"), dtype=np.uint8) for c in colour])
    assert np.array_equal(out["L"][0].ravel()[:5], [255, 0, 76, 150, 29])          # white, black, red, green, blue
    bp = gu.boundary_pixels()
    sums = (bp.astype(np.int64) * np.asarray(gu.L_WEIGHTS)).sum(1) + 0x8000
    res, cnt = np.unique(sums % 65536, return_counts=True)               # not every target has a solution in bytes; most do
    assert res.tolist() == [0, 1, 65535] and cnt.min() >= 10 and len(np.unique(sums >> 16)) >= 20
    assert np.array_equal(out["L"][1].ravel()[:len(bp)], sums >> 16)
    for name, (_, out_hw, pad) in gu.CROP_CASES.items():
        src, rows = gu.case_source(name, out["L"]), gu.case_rows(name)
        out[f"{name}/rows"] = rows
        for ff in (1, 0):
            out[f"{name}/ff{ff}"] = np.stack([pil_crop_flip(src[i], t, l, f, out_hw, pad, bool(ff)) for i, t, l, f in rows])
    path = os.path.join(HERE, "g22_gray.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "; boundary pixels", len(bp))


if __name__ == "__main__":
    main()
