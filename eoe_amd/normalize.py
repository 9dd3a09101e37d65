"""Per-task input normalisation: the reference's transform strings 'normalize' and 'gcn-normalize' resolved on the device.

The reference's dataset base class replaces the string that ends every runner's transform chain once per task
(`datasets/bases.py:293-372`): it walks the raw normal training set and either fits a per-channel mean / std with
`RunningStats` (`utils/stats.py`) or, for 'gcn-normalize', takes the extremes of the set after global contrast normalisation
(GCN, per sample: subtract the sample's mean, divide by its mean absolute deviation, `bases.py:30-45`) and installs
`GlobalContrastNormalization('l1')` followed by `Normalize([tmin] * C, [tmax - tmin] * C)`.

Here one kernel (`eoe_set_moments_u8`) reduces the resident uint8 set to exact integer sums per image, and the host restates
the reference's arithmetic on them in float64:
  * `RunningStats` is NOT the textbook mean / std.  It is a recurrence over DataLoader batches of two images in dataset order
    (`bases.py:339-344`): n += 1; d = x - m; m += mean(d) / n; m2 += mean((x - m) * d); std = sqrt(m2 / n).  The running mean is
    a mean of batch means (a last batch of one image weighs as much as a pair) and the variance term of a batch is
    mean((x - m_new)(x - m_old)) = E[x^2] - (m_new + m_old) E[x] + m_new m_old, which needs only the batch's E[x] and E[x^2].
  * GCN is increasing and affine per sample, so the extremes of the normalised set are the extremes over the images of
    (min_i - mean_i) / scale_i and (max_i - mean_i) / scale_i; with S = sum v, D = sum |N v - S| (N = C*H*W) these are the
    exact rationals N (N min - S) / D and N (N max - S) / D.
Under data parallelism every rank fits the same statistics from its own copy of the set: the sums are integers, so all ranks
get identical bits and no collective is needed.

The per-step operator is `gcn_normalize` (`eoe_gcn_normalize`: GCN and the per-channel affine in one launch).
"""
from typing import Optional, Sequence

import numpy as np
import torch

STD_NORM, GCN_NORM = 0, 1
# the transform strings the reference replaces (`bases.py:24-27`)
NORM_MODES = {"norm": STD_NORM, "normalise": STD_NORM, "normalize": STD_NORM,
              "gcn-norm": GCN_NORM, "gcn-normalise": GCN_NORM, "gcn-normalize": GCN_NORM}
_SCALES = {"l1": 1, "l2": 2}


def norm_mode(name: str) -> int:
    """STD_NORM (0) or GCN_NORM (1) for a transform string, case-insensitive as in the reference (`bases.py:308`)"""
    key = name.lower() if isinstance(name, str) else name
    if key not in NORM_MODES:
        raise ValueError(f"unknown normalisation mode {name!r}; the valid strings are {', '.join(sorted(NORM_MODES))}")
    return NORM_MODES[key]


def check_ds_statistics(stats: dict, mode: int) -> dict:
    """a statistics dict handed in from a snapshot must belong to the requested mode (a dict without 'mode' is mean / std, as
    `bases.py:326` reads it); a mismatch is an error, never a silent refit.  Returns it with plain Python values."""
    have = int(stats.get("mode", STD_NORM))
    if have != mode:
        raise ValueError(f"ds_statistics were fitted in mode {have} but mode {mode} is requested "
                         f"({STD_NORM} = mean / std, {GCN_NORM} = global contrast normalisation)")
    as_list = lambda v: [float(a) for a in (v.tolist() if hasattr(v, "tolist") else v)]      # noqa: E731
    return {"mean": as_list(stats["mean"]), "std": as_list(stats["std"]), "mode": have}


# ------------------------------------------------------------------------------------------------------------ statistics
def set_moments_u8(images_u8: torch.Tensor, index=None):
    """`eoe_set_moments_u8` over a uint8 NHWC set [n, H, W, C] on the GPU, C = 1 or 3.  Returns device int64 tensors
    (chan_sums [m, C, 2] = per channel sum v, sum v^2; img_stats [m, 3] = min, max, sum |N v - S|) for the m listed rows"""
    from ._lib import check, lib
    if not images_u8.is_cuda:
        raise RuntimeError("set_moments_u8 needs a GPU tensor (there is no CPU fallback)")
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.is_contiguous()
    n, H, W, C = images_u8.shape
    idx = None
    if index is not None:
        idx = torch.as_tensor(index, dtype=torch.int64)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise IndexError(f"index outside the image set of {n} rows")
        idx = idx.to(images_u8.device).contiguous()
    m = n if idx is None else idx.numel()
    chan = torch.empty((m, C, 2), dtype=torch.int64, device=images_u8.device)
    img = torch.empty((m, 3), dtype=torch.int64, device=images_u8.device)
    if m > 0:
        check(lib.eoe_set_moments_u8(images_u8.data_ptr(), n, H, W, C, None if idx is None else idx.data_ptr(), m, chan.data_ptr(),
                                     img.data_ptr(), torch.cuda.current_stream(images_u8.device).cuda_stream), "eoe_set_moments_u8")
    return chan, img


def running_stats_from_sums(chan_sums: np.ndarray, pixels: int, batch: int = 2):
    """the reference's `RunningStats` over batches of `batch` consecutive images (`bases.py:339-344`, `utils/stats.py`), from the
    images' integer channel sums [m, C, 2] (sum v, sum v^2 of uint8 values; `pixels` = H*W per image and channel), in float64
    and in the [0, 1] scale of ToTensor.  Returns (mean [C], std [C])"""
    s = np.asarray(chan_sums, dtype=np.int64)
    m, C = s.shape[0], s.shape[1]
    mean, m2, n = np.zeros(C), np.zeros(C), 0
    for b in range(0, m, batch):
        tot = s[b:b + batch].sum(axis=0)                         # exact
        cnt = float(pixels * min(batch, m - b))
        ex, ex2 = tot[:, 0] / (255.0 * cnt), tot[:, 1] / (65025.0 * cnt)
        n += 1
        new = mean + (ex - mean) / n
        m2 = m2 + (ex2 - (new + mean) * ex + new * mean)
        mean = new
    if n == 0:
        return np.full(C, np.nan), np.full(C, np.nan)
    return mean, np.sqrt(m2 / n)


def gcn_extremes_from_stats(img_stats: np.ndarray, totals: np.ndarray, features: int):
    """(tmin, tmax) of the set after `global_contrast_normalization(x, 'l1')` per image (`bases.py:356-362`), from the images'
    integer (min, max, D = sum |N v - S|) [m, 3], S = sum v [m] and N = `features`: (min / 255 - mean_i) / scale_i is the exact
    rational N (N min - S) / D, likewise for max"""
    st, S, N = np.asarray(img_stats, dtype=np.int64), np.asarray(totals, dtype=np.int64).reshape(-1), int(features)
    # the numerators are exact integers below 2^63 for every image the kernel takes; Python ints, since they can pass 2^53
    lo = np.array([N * (N * int(a) - int(b)) for a, b in zip(st[:, 0], S)], dtype=np.float64)
    hi = np.array([N * (N * int(a) - int(b)) for a, b in zip(st[:, 1], S)], dtype=np.float64)
    D = st[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((lo / D).min()), float((hi / D).max())        # a constant image is 0 / 0 = nan, as in the reference


def fit_statistics(images_u8: torch.Tensor, index=None, mode: str = "normalize") -> dict:
    """what `TorchvisionDataset._update_transforms` extracts from the raw normal training set (`bases.py:293-372`), for a uint8
    NHWC set resident on the GPU and the rows `index` (ascending rows of the normal classes; None = every row), in dataset order:
      'normalize'      {'mean': [C floats], 'std': [C floats], 'mode': 0}             (the RunningStats recurrence)
      'gcn-normalize'  {'mean': [tmin] * C, 'std': [tmax - tmin] * C, 'mode': 1}      (extremes of the GCN'd set)
    All six spellings of the reference are accepted.  The values are plain Python floats, so a snapshot holding the dict loads
    without this package."""
    which = norm_mode(mode)
    chan, img = set_moments_u8(images_u8, index)
    _, H, W, C = images_u8.shape
    chan, img = chan.cpu().numpy(), img.cpu().numpy()
    if chan.shape[0] == 0:
        raise ValueError("fit_statistics: no image listed")
    if which == STD_NORM:
        mean, std = running_stats_from_sums(chan, H * W)
        return {"mean": [float(v) for v in mean], "std": [float(v) for v in std], "mode": STD_NORM}
    tmin, tmax = gcn_extremes_from_stats(img, chan[:, :, 0].sum(axis=1), C * H * W)
    return {"mean": [tmin] * C, "std": [tmax - tmin] * C, "mode": GCN_NORM}


# ------------------------------------------------------------------------------------------------------------ operator
def _coef(v, C, device, name):
    t = torch.as_tensor(v, dtype=torch.float32, device=device).reshape(-1).contiguous()
    if t.numel() != C:
        raise ValueError(f"gcn_normalize: {name} must hold one value per channel ({C}), not {t.numel()}")
    return t


def gcn_normalize(x: torch.Tensor, scale: str = "l1", shift=None, range=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """global contrast normalisation and the per-channel Normalize that follows it, one HIP launch (`eoe_gcn_normalize`):
    y = ((x - mean_i) / scale_i - shift[c]) / range[c] on fp32 NCHW, mean_i over all features of sample i, scale_i = mean |x -
    mean_i| ('l1') or sqrt(sum (x - mean_i)^2) / n_features ('l2', the reference's definition).  shift / range: C values each,
    both or neither.  out=x works in place (same bits as out of place).  No epsilon: a constant sample gives non-finite values."""
    from ._lib import check, lib
    if not x.is_cuda:
        raise RuntimeError("gcn_normalize needs a GPU tensor (there is no CPU fallback)")
    if scale not in _SCALES:
        raise ValueError(f"gcn_normalize: scale must be 'l1' or 'l2', not {scale!r}")
    if (shift is None) != (range is None):
        raise ValueError("gcn_normalize: shift and range go together (both or neither)")
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
    n, C, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.is_contiguous()
    if n == 0:
        return out
    sh = rg = None
    if shift is not None:
        sh, rg = _coef(shift, C, x.device, "shift"), _coef(range, C, x.device, "range")
    check(lib.eoe_gcn_normalize(x.data_ptr(), out.data_ptr(), n, C, H, W, _SCALES[scale], None if sh is None else sh.data_ptr(),
                                None if rg is None else rg.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream),
          "eoe_gcn_normalize")
    return out


class GlobalContrastNormalization:
    """drop-in for the reference's transform of the same name (`utils/transformations.py:326-349`): same constructor, and the
    call works IN PLACE on an [n, c, h, w] batch and returns its argument"""

    def __init__(self, gcn=None, scale="l1"):
        self.scale = scale
        if gcn is not None:
            assert gcn.scale == scale

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        assert self.scale in ("l1", "l2")
        return gcn_normalize(x, self.scale, out=x)


class GcnNormalize:
    """what a source in 'gcn-normalize' mode reports as `.normalize`: GCN(scale) followed by Normalize(shift, range).  The trainer
    runs it on the step batch after the multi-scale modes and before the encoder; the call is out of place (step batches may be
    tensors the source keeps)."""

    def __init__(self, shift: Sequence[float], range: Sequence[float], scale: str = "l1"):
        if scale not in _SCALES:
            raise ValueError(f"scale must be 'l1' or 'l2', not {scale!r}")
        self.shift, self.range, self.scale = [float(v) for v in shift], [float(v) for v in range], scale
        self._dev = {}

    @classmethod
    def from_statistics(cls, stats: dict, scale: str = "l1") -> "GcnNormalize":
        stats = check_ds_statistics(stats, GCN_NORM)
        return cls(stats["mean"], stats["std"], scale)

    def _coefs(self, device):
        if device not in self._dev:                      # uploaded once per device, not per step
            self._dev[device] = (torch.tensor(self.shift, dtype=torch.float32, device=device),
                                 torch.tensor(self.range, dtype=torch.float32, device=device))
        return self._dev[device]

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        sh, rg = self._coefs(x.device)
        return gcn_normalize(x.contiguous(), self.scale, sh, rg)

    def __repr__(self):
        return f"GcnNormalize(shift={self.shift}, range={self.range}, scale={self.scale!r})"
