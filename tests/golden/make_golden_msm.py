"""Generates tests/golden/g17_msm.npz by running the REFERENCE's own MSM filters (`utils/transformations.py`:
GpuDFTLowPassFilter, GpuDFTHighPassFilter, ConditionalCompose(gpu=True)) on CPU torch, in fp32 and fp64.  Run by hand where the
reference is available; the tests only read the .npz.  torchvision and kornia are absent, so their imports are stubbed: the
fft filters do not use them, and the reference's Blur (kornia gaussian_blur2d) is therefore not pinned here -- only by the numpy
restatement in eoe_amd.msm (DESIGN.md says so).

Inputs: oracle.fill("g17/<size>", shape, std=0.25, mean=0.5) in fp32 (fp64 = the same values widened); 224^2 outputs are
stored on the pixel grid [::8, ::8] only, to keep the file small."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.fill import fill   # noqa: E402

REF = "/root/reference/src/eoe"
SHAPES = {"32": (1, 3, 32, 32), "28": (2, 1, 28, 28), "224": (1, 1, 224, 224)}
MAGNITUDES = (0, 1, 2, 4, 8, 16, 32)
# 224^2 also takes the rest of the ImageNet driver's defaults (multiscale_imagenet.py); at 28^2 / 32^2 they clip to n/2 = 16
MAGNITUDES_BY_SIZE = {"32": MAGNITUDES, "28": MAGNITUDES, "224": MAGNITUDES + (64, 128, 256)}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


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
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def golden_input(size: str) -> np.ndarray:
    return fill(f"g17/{size}", SHAPES[size], std=0.25, mean=0.5)


def main():
    out = {}
    for size, shape in SHAPES.items():
        x32 = golden_input(size)
        if size != "224":
            out[f"in64/{size}"] = x32.astype(np.float64)
        for op, cls in (("lpf", T.GpuDFTLowPassFilter), ("hpf", T.GpuDFTHighPassFilter)):
            for mag in MAGNITUDES_BY_SIZE[size]:
                f = cls(types.SimpleNamespace(magnitude=mag))
                for dt, tag in ((torch.float64, "out64"), (torch.float32, "out32")):
                    y = f(torch.from_numpy(x32).to(dt)).numpy()
                    if size == "224":
                        y = y[:, :, ::8, ::8]
                    if tag == "out32" and size == "32":
                        continue
                    out[f"{tag}/{op}/{size}/{mag}"] = y
    x = golden_input("32").repeat(2, 0).astype(np.float64)
    x[1] = 1.0 - x[1]
    y = torch.tensor([0, 1])
    lpf = T.GpuDFTLowPassFilter(types.SimpleNamespace(magnitude=4))
    hpf = T.GpuDFTHighPassFilter(types.SimpleNamespace(magnitude=2))
    compose = T.ConditionalCompose([(0, lpf, None), (0, None, hpf)], gpu=True)
    out["compose/x"], out["compose/y"] = x, y.numpy()
    out["compose/out"] = compose(torch.from_numpy(x), y).numpy()
    path = os.path.join(HERE, "g17_msm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
