"""Multi-scale modes (MSM), the reference's frequency-analysis filters (`src/eoe/datasets/__init__.py:157-221,287-309`,
`utils/transformations.py`): a label-conditioned lpf / hpf / blur applied to the step batch on the device, after the CPU chain
(crop, flip, ToTensor, noise) and before Normalize (`training/ad_trainer.py:413-425,501-505`), and `sharpen`, Pillow's
UnsharpMask, which the reference runs on the uint8 PIL image between the PIL augmentations and ToTensor (`datasets/cifar.py:99-118`).
The filters are the HIP kernels of csrc/msm.hip (`eoe_msm_filter`) and csrc/sharpen.hip (`eoe_msm_sharpen_u8` / `_f32`, byte-exact
with Pillow); sharpen has no host path, so it needs a GPU device."""
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

TRANSFORMS = ("blur", "sharpen", "hpf", "lpf")                                    # utils/transformations.py:20
DS_PARTS = {"train_nominal": 0, "train_oe": 1, "test_nominal": 2, "test_anomalous": 3}   # datasets/__init__.py:150-154
GPU_OPS = ("lpf", "hpf", "blur")                                                  # fp32 filters (msm_filter)
SHARPEN_RADIUS, SHARPEN_THRESHOLD = 2.0, 3                                        # ImageFilter.UnsharpMask defaults


class MSM:
    """`MSM(transform, ds_part, magnitude=None)` with the reference's string form `lpf+train_nominal--M4`"""

    def __init__(self, transform: str, ds_part: str, magnitude: int = None):
        if transform not in TRANSFORMS:
            raise ValueError(f"unknown MSM transform {transform!r}; known: {TRANSFORMS}")
        if ds_part not in DS_PARTS:
            raise ValueError(f"unknown MSM dataset part {ds_part!r}; known: {tuple(DS_PARTS)}")
        self.transform_str, self.ds_part_str = transform, ds_part
        self.ds_part = DS_PARTS[ds_part]
        self.magnitude = magnitude

    def set_magnitude(self, magnitude: int) -> "MSM":
        self.magnitude = magnitude
        return self

    def __str__(self):
        return "+".join((self.transform_str, self.ds_part_str)) + f"--M{self.magnitude}"

    __repr__ = __str__

    @staticmethod
    def load(msm: str, load_magnitude: bool = True) -> "MSM":
        transform, ds_part = msm.split("+")
        magnitude = None
        if "--M" in ds_part:
            ds_part, magnitude = ds_part.split("--M")
        res = MSM(transform, ds_part)
        if load_magnitude and magnitude is not None:
            res.set_magnitude(int(magnitude))
        return res


def check_supported(msms: Sequence[MSM], device=None):
    """lpf / hpf / blur run anywhere msm_filter runs; sharpen only on a GPU device (there is no host path).  device None: not
    checked here (apply_msms checks the batch's device)"""
    for m in msms:
        if m.transform_str == "sharpen":
            if device is not None and torch.device(device).type != "cuda":
                raise NotImplementedError(f"MSM transform 'sharpen' ({m}) needs a GPU device: Pillow's UnsharpMask is built as a HIP "
                                          f"kernel only, with no host path (device {device})")
        elif m.transform_str not in GPU_OPS:
            raise NotImplementedError(f"MSM transform {m.transform_str!r} ({m}) is not built")


def sharpen_percent(magnitude) -> int:
    """PilUnsharpMask's percent (transformations.py:120)"""
    return int(magnitude * 100)


def blur_taps_k(sigma: float, width: int) -> int:
    """kernel size of the reference's Blur (transformations.py:146,152)"""
    k = 2 * int(int(sigma / 2) + 0.5) + 1
    return max(min(k, 2 * int(int(width / 2) + 0.5) - 1), 3)


# ------------------------------------------------------------------------------------------------------------ operators
_OPS = {"lpf": 1, "hpf": 2, "blur": 3}


def host_operator(op: str, n: int, magnitude: int, rank_limited: bool = False):
    """the library's fp64 operator (eoe_msm_operator): dense -> (G complex n x n, (0, 1)); rank-limited -> (U complex n x r, (c, s))
    with G = c I + s U U^H"""
    from ._lib import check, lib
    cols = C.c_int(0)
    cs = (C.c_double * 2)()
    check(lib.eoe_msm_operator(_OPS[op], n, int(magnitude), int(rank_limited), None, None, C.byref(cols), cs), "eoe_msm_operator")
    r = cols.value
    re = np.zeros((n, max(r, 1)), np.float64)
    im = np.zeros_like(re)
    check(lib.eoe_msm_operator(_OPS[op], n, int(magnitude), int(rank_limited), re.ctypes.data, im.ctypes.data, C.byref(cols), cs),
          "eoe_msm_operator")
    return (re + 1j * im)[:, :r], (cs[0], cs[1])


_DEVICE_OPS: Dict[Tuple, torch.Tensor] = {}


def _device_operator(op: str, n: int, magnitude: int, form: int, device) -> torch.Tensor:
    """fp32 operator in the layout eoe_msm_filter reads, built once per (op, n, magnitude, form, device)"""
    key = (op, n, int(magnitude), form, str(device))
    t = _DEVICE_OPS.get(key)
    if t is None:
        from ._lib import EOE_MSM_FORM_DENSE
        if form == EOE_MSM_FORM_DENSE:
            g, _ = host_operator(op, n, magnitude, False)
            host = np.concatenate([g.real.ravel(), g.imag.ravel()])
        else:
            u, _ = host_operator(op, n, magnitude, True)
            ut = np.concatenate([u.real, u.imag], axis=1)                          # n x 2r
            host = np.concatenate([ut.ravel(), ut.T.ravel(), np.zeros(1)])          # [Ut | Ut^T] (never empty)
        t = torch.from_numpy(host.astype(np.float32)).to(device)
        _DEVICE_OPS[key] = t
    return t


_WORKSPACE: Dict[str, torch.Tensor] = {}


def _workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    if nbytes == 0:
        return None
    key = str(device)
    w = _WORKSPACE.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _WORKSPACE[key] = w
    return w


def msm_filter(x: torch.Tensor, op: str, magnitude: int, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = op(x) on the rows selected by `rows` (bool / uint8 mask of x.shape[0], None = all), bit copies elsewhere; x fp32
    NCHW in the [0, 1] pixel scale, on the GPU.  Out of place: x is not modified."""
    from ._lib import check, lib
    if op == "sharpen":
        raise ValueError("msm_filter: sharpen is not an fp32 filter (Pillow's UnsharpMask on uint8 images); use msm_sharpen or "
                         "sharpen_u8")
    if op not in _OPS:
        raise ValueError(f"msm_filter: unknown op {op!r}; known: {tuple(_OPS)}")
    if not x.is_cuda:
        raise RuntimeError("msm_filter needs a GPU tensor (there is no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n_img, ch, h, w = x.shape
    y = torch.empty_like(x)
    if n_img == 0:
        return y
    form, nbytes = C.c_int(0), C.c_size_t(0)
    check(lib.eoe_msm_workspace(_OPS[op], n_img, ch, h, w, int(magnitude), C.byref(form), C.byref(nbytes)), "eoe_msm_workspace")
    oper = None
    if form.value != 0:
        oper = _device_operator(op, h, magnitude, form.value, x.device)
    ws = _workspace(nbytes.value, x.device)
    r = None
    if rows is not None:
        r = rows.to(device=x.device, dtype=torch.uint8).contiguous()
        assert r.shape == (n_img,)
    check(lib.eoe_msm_filter(_OPS[op], x.data_ptr(), y.data_ptr(), None if r is None else r.data_ptr(), n_img, ch, h, w,
                             int(magnitude), None if oper is None else oper.data_ptr(), None if ws is None else ws.data_ptr(),
                             nbytes.value, torch.cuda.current_stream(x.device).cuda_stream), "eoe_msm_filter")
    return y


def _rows_arg(rows, n_img, device):
    if rows is None:
        return None
    r = rows.to(device=device, dtype=torch.uint8).contiguous()
    assert r.shape == (n_img,)
    return r


def msm_sharpen(x: torch.Tensor, magnitude, rows: Optional[torch.Tensor] = None, radius: float = SHARPEN_RADIUS,
                threshold: int = SHARPEN_THRESHOLD) -> torch.Tensor:
    """the reference's PilUnsharpMask(magnitude) on fp32 NCHW batches in [0, 1] on the GPU (`eoe_msm_sharpen_f32`): sharpens
    q = clamp(rint(x * 255)) and returns q' / 255, bit-exact with ToTensor(Pillow(q)) for batches on the k / 255 grid.  Rows as in
    msm_filter; magnitude 0 is a bit copy; out of place."""
    from ._lib import check, lib
    if not x.is_cuda:
        raise RuntimeError("msm_sharpen needs a GPU tensor (there is no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 4
    x = x.contiguous()
    n_img, ch, h, w = x.shape
    y = torch.empty_like(x)
    if n_img == 0:
        return y
    r = _rows_arg(rows, n_img, x.device)
    check(lib.eoe_msm_sharpen_f32(x.data_ptr(), y.data_ptr(), None if r is None else r.data_ptr(), n_img, ch, h, w, float(radius),
                                  sharpen_percent(magnitude), int(threshold), torch.cuda.current_stream(x.device).cuda_stream),
          "eoe_msm_sharpen_f32")
    return y


def sharpen_u8(imgs: torch.Tensor, percent: int, rows: Optional[torch.Tensor] = None, radius: float = SHARPEN_RADIUS,
               threshold: int = SHARPEN_THRESHOLD) -> torch.Tensor:
    """Pillow's `ImageFilter.UnsharpMask(radius, percent, threshold)` on uint8 NHWC images [n, H, W, C] (C = 1 or 3) on the GPU,
    byte-exact (`eoe_msm_sharpen_u8`); rows as in msm_filter; out of place"""
    from ._lib import check, lib
    if not imgs.is_cuda:
        raise RuntimeError("sharpen_u8 needs a GPU tensor (there is no CPU fallback)")
    assert imgs.dtype == torch.uint8 and imgs.dim() == 4
    imgs = imgs.contiguous()
    n_img, h, w, ch = imgs.shape
    out = torch.empty_like(imgs)
    if n_img == 0:
        return out
    r = _rows_arg(rows, n_img, imgs.device)
    check(lib.eoe_msm_sharpen_u8(imgs.data_ptr(), out.data_ptr(), None if r is None else r.data_ptr(), n_img, h, w, ch, float(radius),
                                 int(percent), int(threshold), torch.cuda.current_stream(imgs.device).cuda_stream), "eoe_msm_sharpen_u8")
    return out


# ------------------------------------------------------------------------------------------------------------ routing
def routing(msms: Sequence[MSM], split: str) -> List[Tuple[str, int, bool, bool]]:
    """(op, magnitude, on nominal rows, on anomalous rows) in list order, as `load_dataset` builds the conditional transforms
    (datasets/__init__.py:287-309): train -- train_nominal filters the nominal rows, train_oe every OE row; test -- test_nominal
    / test_anomalous filter the rows of that label"""
    if split not in ("train", "test"):
        raise ValueError(f"split must be 'train' or 'test', not {split!r}")
    parts = ("train_nominal", "train_oe") if split == "train" else ("test_nominal", "test_anomalous")
    out = []
    for m in msms:
        if m.ds_part_str in parts:
            out.append((m.transform_str, m.magnitude, m.ds_part_str == parts[0], m.ds_part_str == parts[1]))
    return out


def apply_msms(imgs: torch.Tensor, lbls: torch.Tensor, msms: Sequence[MSM], split: str = "train", nominal_label: int = 0) -> torch.Tensor:
    """the MSMs of `split` on a step batch ([normal | OE] rows for train, labelled test rows for test); returns `imgs` itself when
    no MSM applies, a new tensor otherwise.  sharpen runs as msm_sharpen (percent = int(magnitude * 100)) on the fp32 batch"""
    steps = routing(msms, split)
    if not steps:
        return imgs
    check_supported(msms, imgs.device)
    nominal = lbls.to(imgs.device) == nominal_label
    for op, mag, on_nom, on_anom in steps:
        if mag is None:
            raise ValueError(f"MSM {op} has no magnitude set")
        rows = None if (on_nom and on_anom) else (nominal if on_nom else ~nominal)
        imgs = msm_sharpen(imgs, mag, rows) if op == "sharpen" else msm_filter(imgs, op, mag, rows)
    return imgs


# ------------------------------------------------------------------------------------------------------------ restatements
def fft_filter_np(x: np.ndarray, op: str, magnitude: int) -> np.ndarray:
    """numpy restatement of GpuDFTLowPassFilter / GpuDFTHighPassFilter (+ MinMaxNorm) in the dtype of x"""
    if magnitude <= 0:
        return x.copy()
    n, c, h, w = x.shape
    e = min(magnitude, min(w // 2, h // 2))
    f = np.fft.fftshift(np.fft.fft2(x), axes=(-2, -1))
    if op == "lpf":
        f[:, :, :e, :] = 0
        f[:, :, h - e:, :] = 0
        f[:, :, :, :e] = 0
        f[:, :, :, w - e:] = 0
    else:
        f[:, :, h // 2 - e:h // 2 + e, w // 2 - e:w // 2 + e] = 0
    y = np.fft.ifft2(np.fft.ifftshift(f, axes=(-2, -1))).real.astype(x.dtype)
    y = y - y.reshape(n, -1).min(1)[:, None, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / y.reshape(n, -1).max(1)[:, None, None, None]


def blur_np(x: np.ndarray, sigma: float) -> np.ndarray:
    """numpy restatement of kornia's gaussian_blur2d as the reference's Blur calls it (reflect borders, separable taps)"""
    if sigma <= 0:
        return x.copy()
    k = blur_taps_k(sigma, x.shape[-1])
    t = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-t ** 2 / (2.0 * sigma ** 2))
    g /= g.sum()
    p = k // 2
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect")
    h, w = x.shape[-2:]
    tmp = sum(g[q] * xp[:, :, :, q:q + w] for q in range(k))
    return sum(g[q] * tmp[:, :, q:q + h, :] for q in range(k))


def sharpen_box(radius: float = SHARPEN_RADIUS) -> Tuple[int, int, int]:
    """(r, ww, fw) of Pillow's box passes for a Gaussian radius (_gaussian_blur_radius with 3 passes, ImagingHorizontalBoxBlur), in
    Pillow's float / double / uint32 arithmetic"""
    f = np.float32
    s2 = f(f(radius) * f(radius) / f(3))
    big_l = f(math.sqrt(12.0 * float(s2) + 1.0))
    small_l = f(math.floor((float(big_l) - 1.0) / 2.0))
    a = f(f(f(2) * small_l + f(1)) * f(small_l * f(small_l + f(1)) - f(3) * s2))
    a = f(a / f(f(6) * f(s2 - f(small_l + f(1)) * f(small_l + f(1)))))
    big_r = f(small_l + a)
    r = int(big_r)
    ww = int(f(f(1 << 24) / f(big_r * f(2) + f(1))))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def unsharp_np(u8: np.ndarray, percent: int, radius: float = SHARPEN_RADIUS, threshold: int = SHARPEN_THRESHOLD) -> np.ndarray:
    """numpy restatement of Pillow's ImageFilter.UnsharpMask on uint8 images [..., H, W, C] (libImaging/UnsharpMask.c over
    BoxBlur.c: 3 horizontal + 3 vertical box passes with replicated edges, each rounded to uint8; then |d| > threshold ?
    clamp(src + trunc(d * percent / 100)) : src), byte-exact"""
    assert u8.dtype == np.uint8 and u8.ndim >= 3
    r, ww, fw = sharpen_box(radius)

    def box(a, axis):
        n = a.shape[axis]
        t = lambda k: np.take(a, np.clip(np.arange(n) + k, 0, n - 1), axis=axis).astype(np.uint64)
        v = (sum(t(k) for k in range(-r, r + 1)) * ww + (t(-r - 1) + t(r + 1)) * fw) & 0xFFFFFFFF
        return (((v + (1 << 23)) & 0xFFFFFFFF) >> 24).astype(np.uint8)

    b = u8
    for axis in (-2, -2, -2, -3, -3, -3):
        b = box(b, axis)
    src = u8.astype(np.int64)
    dp = (src - b) * int(percent)
    out = np.clip(src + np.sign(dp) * (np.abs(dp) // 100), 0, 255)
    return np.where(np.abs(src - b) > threshold, out, src).astype(np.uint8)


def torch_fft_filter(x: torch.Tensor, op: str, magnitude: int) -> torch.Tensor:
    """the reference's torch.fft chain (GpuDFTLowPassFilter / GpuDFTHighPassFilter + MinMaxNorm) on any device: the yardstick of
    tools/msm_bench.py and the tests"""
    if magnitude <= 0:
        return x
    n, c, h, w = x.shape
    e = min(magnitude, min(w // 2, h // 2))
    f2 = torch.fft.fftshift(torch.fft.fft2(x))
    if op == "lpf":
        f2[:, :, :e, :] = 0
        f2[:, :, -e:, :] = 0
        f2[:, :, :, :e] = 0
        f2[:, :, :, -e:] = 0
    else:
        f2[:, :, h // 2 - e:h // 2 + e, w // 2 - e:w // 2 + e] = 0
    img = torch.fft.ifft2(torch.fft.ifftshift(f2)).real
    img = img.flatten(1).sub(img.flatten(1).min(1)[0].unsqueeze(1)).reshape(img.shape)
    return img.flatten(1).div(img.flatten(1).max(1)[0].unsqueeze(1)).reshape(img.shape)


def torch_blur(x: torch.Tensor, sigma: float) -> torch.Tensor:
    """kornia's gaussian_blur2d restated with torch conv2d (reflect padding, separable normalised taps)"""
    if sigma <= 0:
        return x
    k = blur_taps_k(sigma, x.shape[-1])
    t = torch.arange(k, dtype=torch.float32, device=x.device) - k // 2
    g = torch.exp(-t ** 2 / (2.0 * float(sigma) ** 2))
    g = g / g.sum()
    c = x.shape[1]
    xp = torch.nn.functional.pad(x, (k // 2, k // 2, k // 2, k // 2), mode="reflect")
    y = torch.nn.functional.conv2d(xp, g.view(1, 1, 1, k).repeat(c, 1, 1, 1), groups=c)
    return torch.nn.functional.conv2d(y, g.view(1, 1, k, 1).repeat(c, 1, 1, 1), groups=c)
