"""Generates tests/golden/g18_sharpen.npz by running the REFERENCE's own PilUnsharpMask (`utils/transformations.py:114-123`, the
sharpen MSM: Pillow's ImageFilter.UnsharpMask(percent=int(magnitude * 100)) with radius 2, threshold 3) on uint8 PIL images with
the installed Pillow.  Run by hand where the reference is available; the tests only read the .npz.  torchvision and kornia are
absent, so their imports are stubbed: PilUnsharpMask uses neither.

Inputs: `image(name, h, w, c)` below, a pure function of its arguments (a smooth pattern, flat patches that stay under the
threshold, and noise from oracle.fill's counter-based generator), stored as `in/<case>` (NHWC uint8, C = 1 for mode L).  The
224^2 input is not stored: the tests regenerate it and check it against `in_grid/224` (its [::4, ::4] sub-grid); its outputs are
stored on the same sub-grid."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.fill import uniform_pm1   # noqa: E402

REF = "/root/reference/src/eoe"
MAGNITUDES = (0, 1, 2, 4, 8, 16, 32)
# case -> (h, w, c, number of images, magnitudes)
CASES = {"rgb32": (32, 32, 3, 4, MAGNITUDES), "l28": (28, 28, 1, 4, MAGNITUDES), "rgb3x3": (3, 3, 3, 2, MAGNITUDES),
         "l5x7": (5, 7, 1, 2, MAGNITUDES), "rgb5x7": (5, 7, 3, 2, MAGNITUDES),
         "rgb224": (224, 224, 3, 1, (0, 1, 4, 32, 64, 128, 256))}           # 64-256: the ImageNet driver's defaults
GRID = 4


def image(name: str, h: int, w: int, c: int) -> np.ndarray:
    """uint8 [h, w, c]: a smooth pattern, a flat patch in the top-left quarter and noise"""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((h, w, c))
    for ch in range(c):
        out[..., ch] = 128 + 90 * np.sin(2 * np.pi * x / (5.0 + 3 * ch) + ch) * np.cos(2 * np.pi * y / (7.0 + 2 * ch))
    noise = uniform_pm1(f"g18/{name}", h * w * c).reshape(h, w, c)
    out += 40 * noise
    out[: h // 4 + 1, : w // 4 + 1] = 100 + np.round(2 * noise[: h // 4 + 1, : w // 4 + 1])   # |d| <= 3: left alone
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


def images(case: str) -> np.ndarray:
    h, w, c, n, _ = CASES[case]
    return np.stack([image(f"{case}/{i}", h, w, c) for i in range(n)])


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _load_reference():
    class _Compose:
        def __init__(self, transforms):
            self.transforms = transforms

    _stub("torchvision").__path__ = []
    _stub("torchvision.transforms", Compose=_Compose, Normalize=type("Normalize", (), {}),
          Grayscale=type("Grayscale", (), {})).__path__ = []
    _stub("torchvision.transforms.functional", to_tensor=None, to_pil_image=None)
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    _stub("kornia").__path__ = []
    _stub("kornia.filters", gaussian_blur2d=None)
    spec = importlib.util.spec_from_file_location("ref_transformations", f"{REF}/utils/transformations.py")
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


def main():
    from PIL import Image
    T = _load_reference()
    out = {}
    for case, (h, w, c, n, mags) in CASES.items():
        x = images(case)
        if case == "rgb224":
            out["in_grid/224"] = x[:, ::GRID, ::GRID]
        else:
            out[f"in/{case}"] = x
        for mag in mags:
            ys = []
            for img in x:
                pil = Image.fromarray(img if c == 3 else img[..., 0], "RGB" if c == 3 else "L")
                y = np.asarray(T.PilUnsharpMask(mag)(pil))
                ys.append(y if c == 3 else y[..., None])
            y = np.stack(ys)
            out[f"out/{case}/{mag}"] = y[:, ::GRID, ::GRID] if case == "rgb224" else y
    path = os.path.join(HERE, "g18_sharpen.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
