"""Inputs and the CPU reference of the CLIP-preprocessing tests (fixture g24_clip_pre, made by tests/golden/make_golden_clip_pre.py with
Pillow): the chain RandomCrop / flip -> Resize(P, BICUBIC) -> CenterCrop(P) -> convert("RGB") -> ToTensor -> noise -> Normalize of the
reference's small-image CLIP runners, restated from oracle.augment functions only.

Inputs are pure functions of a name (oracle.fill), so the fixture holds only Pillow's results."""
import numpy as np

from oracle import augment as oaug
from oracle import fill as ofill

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # clip_official/clip/clip.py:64

# fixture cases: name -> (images, side S, channels, n_px P, filter).  The two the reference's runners have, and small odd ones: a
# width that is no multiple of 4 with both channel counts and both filters, and S = P (the taps round to the identity)
FIXTURE_CASES = {"rgb32": (2, 32, 3, 224, "bicubic"), "l28": (1, 28, 1, 224, "bicubic"), "rgb9": (2, 9, 3, 23, "bicubic"),
                 "l9": (2, 9, 1, 23, "bicubic"), "rgb9lin": (2, 9, 3, 23, "bilinear"), "rgb12": (1, 12, 3, 12, "bicubic"),
                 "l12": (1, 12, 1, 12, "bicubic")}


def images(name: str, n: int, H: int, W: int, C: int) -> np.ndarray:
    """uint8 NHWC [n, H, W, C] of a name"""
    return ofill.fill_int(f"g24/{name}", (n, H, W, C), 0, 256).astype(np.uint8)


def fixture_crops(case: str) -> np.ndarray:
    n, S, C, _, _ = FIXTURE_CASES[case]
    return images(case, n, S, S, C)


def params(name: str, n: int, n_src: int, Hs: int, Ws: int, S: int, pad: int) -> np.ndarray:
    """int32 [n, 4] = (index, top, left, flip): scattered indices, origins over the whole padded range; the first rows sit in the
    corners, so that padded zeros enter the filter on every side"""
    lo_t, hi_t, lo_l, hi_l = -pad, Hs + pad - S, -pad, Ws + pad - S
    p = np.stack([ofill.fill_int(f"g24/{name}/i", (n,), 0, n_src), ofill.fill_int(f"g24/{name}/t", (n,), lo_t, hi_t + 1),
                  ofill.fill_int(f"g24/{name}/l", (n,), lo_l, hi_l + 1), ofill.fill_int(f"g24/{name}/f", (n,), 0, 2)], axis=1)
    corners = [(lo_t, lo_l, 1), (lo_t, hi_l, 0), (hi_t, lo_l, 0), (hi_t, hi_l, 1)]
    for r, (t, l, f) in enumerate(corners[:n]):
        p[r, 1:] = (t, l, f)
    return p.astype(np.int32)


def oracle_crops(src: np.ndarray, p: np.ndarray, S: int, flip_first: bool) -> np.ndarray:
    """uint8 [n, S, S, C]: the crop / flip of oracle.augment.augment_batch (a 1-channel set enters as three equal planes)"""
    C = src.shape[3]
    src3 = src if C == 3 else np.repeat(src, 3, axis=3)
    f = oaug.augment_batch(src3, p, S, S, None, None, flip_first, 0.0, 0)                  # [n, 3, S, S] = byte / 255
    u8 = np.rint(f * np.float32(255.0)).astype(np.uint8).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(u8[..., :C])


def oracle_resized(crops: np.ndarray, P: int, filt: str = "bicubic") -> np.ndarray:
    """uint8 [n, P, P, 3]: Resize(P) (CenterCrop(P) of the square result is the identity) and convert("RGB") per image"""
    out = np.stack([oaug.resize(c, (P, P), filt) for c in crops])
    return out if out.shape[3] == 3 else np.repeat(out, 3, axis=3)


def oracle_bytes(src, p, S, P, flip_first=True, filt="bicubic") -> np.ndarray:
    return oracle_resized(oracle_crops(src, p, S, flip_first), P, filt)


def oracle_f32(u8: np.ndarray, mean=None, std=None, noise_std: float = 0.0, seed: int = 0) -> np.ndarray:
    """ToTensor -> noise -> Normalize on uint8 [n, P, P, 3] -> float32 NCHW, in the operations and order of oracle.augment.augment_batch"""
    n, P = u8.shape[0], u8.shape[1]
    out = (u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    if noise_std > 0:
        out = out + np.float32(noise_std) * oaug.noise(seed, n, P, P)
    if mean is not None:
        out = (out - np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)) / np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
    return np.ascontiguousarray(out.astype(np.float32))
