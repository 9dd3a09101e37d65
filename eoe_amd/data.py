"""The step-batch contract of the hot path and synthetic sources that honour it.

The reference's datasets / PIL pipelines are out of scope (disk I/O; absent in both containers); what the
training loop depends on is the layout `BalancedConcatLoader` produces (`src/eoe/datasets/bases.py:570-600`):
  imgs   = cat([normal_i, oe_i[:len(normal_i)]])        labels = [nominal]*n + [anomalous]*n
  idcs   = cat([normal idcs, oe idcs + len(normal dataset)])
with OE indices tiled when the OE set is smaller than the normal set (:580-584), OE sampled with replacement iff it
holds >= 10 000 samples (`bases.py:561`), a ragged last batch (no drop_last) and len(loader) = len(normal loader).
"""
import math
from typing import Iterator, List, Optional, Sequence, Tuple

import torch


def balanced_concat(normal: Sequence[torch.Tensor], oe_iter: Iterator, n_normal_dataset: int) -> List[torch.Tensor]:
    """BalancedConcatLoader.__next__ (bases.py:591-597) on (imgs, lbls, idcs) triples"""
    oe = [a for a in next(oe_iter)]
    while oe[1].shape[0] < normal[1].shape[0]:
        oe = [torch.cat([a, b]) for a, b in zip(oe, next(oe_iter))]
    oe[-1] = oe[-1] + n_normal_dataset
    n = normal[0].shape[0]
    return [torch.cat([i, j[:n]]) for i, j in zip(normal, oe)]


def tile_oe_indices(oe_indices: torch.Tensor, n_normal: int) -> torch.Tensor:
    if len(oe_indices) < n_normal:
        r = int(math.ceil(n_normal / len(oe_indices)))
        oe_indices = oe_indices.reshape(1, -1).repeat(r, 1).reshape(-1)
    return oe_indices


class ListSource:
    """a fixed list of step batches [(imgs, lbls[, idcs]), ...] per epoch -- what the parity tests feed"""

    nominal_label, anomalous_label = 0, 1

    def __init__(self, train_batches, test_batches=None, normalize=None):
        self.train_batches, self.test_batches, self.normalize = list(train_batches), list(test_batches or []), normalize
        self.ds_statistics = None

    def loaders(self, batch_size=None, **kw):
        return self.train_batches, self.test_batches


class SyntheticAD:
    """in-memory synthetic one-vs-rest task: normal samples ~ N(0,1), anomalies / OE ~ N(0,1) + shift * pattern.
    Produces step batches with the BalancedConcatLoader layout; test split holds labelled normal + anomalous."""

    nominal_label, anomalous_label = 0, 1

    def __init__(self, n_train_normal=512, n_oe=512, n_test=256, res=224, shift=0.5, seed=0, normalize=None):
        g = torch.Generator().manual_seed(seed)
        self.res = res
        pattern = torch.randn((1, 3, res, res), generator=g)
        self.train_normal = torch.randn((n_train_normal, 3, res, res), generator=g)
        self.oe = torch.randn((n_oe, 3, res, res), generator=g) + shift * pattern
        half = n_test // 2
        self.test_x = torch.cat([torch.randn((half, 3, res, res), generator=g),
                                 torch.randn((n_test - half, 3, res, res), generator=g) + shift * pattern])
        self.test_y = torch.cat([torch.zeros(half, dtype=torch.int64), torch.ones(n_test - half, dtype=torch.int64)])
        self.normalize = normalize
        self.ds_statistics = None
        self._g = g

    def _epoch(self, batch_size):
        n, m = self.train_normal.shape[0], self.oe.shape[0]
        perm = torch.randperm(n, generator=self._g)
        oe_idx = tile_oe_indices(torch.arange(m), n)
        if m >= 10000:                                   # bases.py:561: with replacement for large OE sets
            oe_order = oe_idx[torch.randint(len(oe_idx), (len(oe_idx),), generator=self._g)]
        else:
            oe_order = oe_idx[torch.randperm(len(oe_idx), generator=self._g)]

        def oe_batches():
            for s in range(0, len(oe_order), batch_size):
                idx = oe_order[s:s + batch_size]
                yield self.oe[idx], torch.ones(len(idx), dtype=torch.int64), idx.clone()

        oe_it = oe_batches()
        for s in range(0, n, batch_size):
            idx = perm[s:s + batch_size]
            normal = (self.train_normal[idx], torch.zeros(len(idx), dtype=torch.int64), idx.clone())
            yield tuple(balanced_concat(normal, oe_it, n))

    def loaders(self, batch_size, **kw):
        class _Train:
            def __init__(s, outer):
                s.outer = outer

            def __iter__(s):
                return s.outer._epoch(batch_size)

            def __len__(s):
                return math.ceil(s.outer.train_normal.shape[0] / batch_size)

        test = [(self.test_x[s:s + batch_size], self.test_y[s:s + batch_size],
                 torch.arange(s, min(s + batch_size, len(self.test_y)))) for s in range(0, len(self.test_y), batch_size)]
        return _Train(self), test



# ---------------------------------------------------------------------------------------------------------------------
# on-device input pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _channels(src_u8, who):
    """the channel count of a uint8 NHWC set, 1 or 3"""
    C = int(src_u8.shape[3])
    if C not in (1, 3):
        raise ValueError(f"{who}: images must have 1 or 3 channels, not {C}")
    return C


def resized_hw(H, W, size):
    """the (h, w) that `torchvision.transforms.Resize(size)` gives an H x W image (`transforms/functional.py`
    `_compute_resized_output_size`): an int scales the SHORTER side to `size` and the other one to int(size * long / short) -- the
    image is unchanged when the shorter side equals `size` already --, a pair is (h, w) itself"""
    H, W = int(H), int(W)
    if not isinstance(size, int):
        h, w = size
        return int(h), int(w)
    short, long = (W, H) if W <= H else (H, W)
    if short == size:
        return H, W
    new_long = int(size * long / short)
    return (new_long, size) if W <= H else (size, new_long)


class RaggedImageSet:
    """uint8 HWC images of DIFFERENT sizes and one channel count (1 or 3), as the 224 x 224 tasks have them after `Resize(256)`
    (`main/train_imagenet.py:30-34`: 256 x W' or H' x 256 per image).  Layout:
      `arena`        one flat uint8 tensor, the images back to back, each row-major HWC.  Every image STARTS at a multiple of
                     16 bytes (`ALIGN`; the gap is zeros) and the arena's length is a multiple of 16, so an equal-size set is a
                     strided view.  Rows are not aligned -- W * C is odd for most images -- and no kernel assumes they are.
      `offsets`      int64 [n] on the arena's device: the byte at which image i starts (int64: one ImageNet class after
                     Resize(256) is about 340 MB, an OE pool more)
      `sizes_dev`    int32 [n, 2] = (H_i, W_i) on the arena's device
      `sizes`, `offsets_host`   host copies (numpy): crop origins are drawn and launches sized on the host
    Usable without a GPU (packing, indexing, `.to`); the kernels that read it (`resize_u8`, `augment_batch`, `crop_flip_u8`,
    `color_jitter_crop_u8`) need it on one."""

    ALIGN = 16

    def __init__(self, images, device=None):
        """images: a sequence of uint8 numpy arrays or tensors [H, W], [H, W, 1] or [H, W, 3] (mixed channel counts are refused)"""
        import numpy as np
        ts = []
        for i, im in enumerate(images):
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() not in (2, 3):
                raise ValueError(f"RaggedImageSet: image {i} must be uint8 [H, W] or [H, W, C], not {t.dtype} {list(t.shape)}")
            t = t.unsqueeze(-1) if t.dim() == 2 else t
            if t.shape[2] not in (1, 3) or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"RaggedImageSet: image {i} must be a non-empty image of 1 or 3 channels, not {list(t.shape)}")
            if ts and t.shape[2] != ts[0].shape[2]:
                raise ValueError(f"RaggedImageSet: mixed channel counts (image 0 has {ts[0].shape[2]}, image {i} has {t.shape[2]}); "
                                 "convert the set to one mode first")
            ts.append(t)
        if not ts:
            raise ValueError("RaggedImageSet: at least one image is needed")
        sizes = np.array([[t.shape[0], t.shape[1]] for t in ts], dtype=np.int32)
        offsets, total = self.layout(sizes, ts[0].shape[2])
        arena = torch.zeros(total, dtype=torch.uint8)
        for t, o in zip(ts, offsets):
            arena[int(o):int(o) + t.numel()] = t.reshape(-1).cpu()
        self._set(arena, offsets, sizes, int(ts[0].shape[2]))
        if device is not None and torch.device(device) != self.arena.device:
            self._set(self.arena.to(device), offsets, sizes, self.channels)

    @classmethod
    def layout(cls, sizes, channels):
        """(int64 offsets [n], arena length) of images of `sizes` [n, 2]: each image starts at the next multiple of ALIGN"""
        import numpy as np
        nbytes = sizes[:, 0].astype(np.int64) * sizes[:, 1].astype(np.int64) * int(channels)
        padded = (nbytes + cls.ALIGN - 1) // cls.ALIGN * cls.ALIGN
        ends = np.cumsum(padded)
        return (ends - padded).astype(np.int64), int(ends[-1]) if len(ends) else 0

    def _set(self, arena, offsets_host, sizes_host, channels):
        import numpy as np
        self.arena, self.channels = arena, int(channels)
        self.offsets_host = np.ascontiguousarray(offsets_host, dtype=np.int64)
        self.sizes = np.ascontiguousarray(sizes_host, dtype=np.int32).reshape(-1, 2)
        self.offsets = torch.from_numpy(self.offsets_host.copy()).to(arena.device)
        self.sizes_dev = torch.from_numpy(self.sizes.copy()).to(arena.device)

    @classmethod
    def from_parts(cls, arena, offsets_host, sizes_host, channels):
        """a set over an arena that is laid out already (what the ragged Resize returns)"""
        self = cls.__new__(cls)
        self._set(arena, offsets_host, sizes_host, channels)
        return self

    @classmethod
    def from_tensor(cls, images_u8, device=None):
        """the equal-size set of a uint8 tensor [n, H, W, C] (or [n, H, W])"""
        import numpy as np
        t = images_u8.unsqueeze(-1) if images_u8.dim() == 3 else images_u8
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] not in (1, 3) or 0 in t.shape:
            raise ValueError(f"RaggedImageSet.from_tensor: a non-empty uint8 [n, H, W, C] with C = 1 or 3 is needed, not {t.dtype} "
                             f"{list(images_u8.shape)}")
        n, H, W, C = t.shape
        sizes = np.tile(np.array([[H, W]], dtype=np.int32), (n, 1))
        offsets, total = cls.layout(sizes, C)
        dev = t.device if device is None else torch.device(device)
        arena = torch.zeros((n, total // n), dtype=torch.uint8, device=dev)
        arena[:, :H * W * C] = t.reshape(n, -1).to(dev)
        return cls.from_parts(arena.reshape(-1), offsets, sizes, C)

    def to(self, device):
        if torch.device(device) == self.arena.device:
            return self
        return RaggedImageSet.from_parts(self.arena.to(device), self.offsets_host, self.sizes, self.channels)

    @property
    def device(self):
        return self.arena.device

    @property
    def is_cuda(self):
        return self.arena.is_cuda

    def __len__(self):
        return int(self.sizes.shape[0])

    def __getitem__(self, i):
        i = int(i)
        if not -len(self) <= i < len(self):
            raise IndexError(f"image {i} of a set of {len(self)}")
        (H, W), o = self.sizes[i], int(self.offsets_host[i])
        return self.arena[o:o + int(H) * int(W) * self.channels].view(int(H), int(W), self.channels)

    @property
    def is_uniform(self):
        return bool((self.sizes == self.sizes[0]).all())

    def as_tensor(self):
        """uint8 [n, H, W, C] of an equal-size set (a copy); a set of mixed sizes has no such tensor"""
        if not self.is_uniform:
            raise ValueError("RaggedImageSet.as_tensor: the images differ in size (Resize them to one (h, w), or crop them)")
        n, (H, W) = len(self), (int(v) for v in self.sizes[0])
        return self.arena.view(n, -1)[:, :H * W * self.channels].reshape(n, H, W, self.channels).contiguous()


def _ragged_args(who, src, params):
    if not (src.is_cuda and params.is_cuda):
        raise RuntimeError(f"{who} needs GPU tensors (there is no CPU fallback)")
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 4 and params.is_contiguous()
    return (src.arena.data_ptr(), src.offsets.data_ptr(), src.sizes_dev.data_ptr(), len(src))


def augment_batch(src_u8, params, out_hw, mean=None, std=None, flip_first=True, noise_std=0.001, seed=0):
    """gather + RandomCrop(zero padding) + RandomHorizontalFlip + ToTensor + noise + Normalize in ONE kernel over a uint8
    NHWC image set resident in HBM (`eoe_augment_batch_c`, include/eoe_hip.h): replaces the PIL transform chain of
    `main/train_cifar.py:31-38` / `main/train_clip_imagenet.py:27-36` / `main/train_fmnist.py:31-38` (after its Grayscale) and the
    Normalize of `ad_trainer.py:413-425`.
    src_u8 uint8 [n_src,Hs,Ws,C] (GPU), C = 1 or 3; params int32 [n,4] = (index, top, left, flip) (GPU) -> fp32 NCHW [n,C,Ho,Wo];
    mean / std hold C values.  A `RaggedImageSet` takes `eoe_ragged_augment_batch`: top / left are relative to image `index`'s own
    extents; the result is what this function gives on that image alone, bit for bit (n = 0: an empty batch, no launch)."""
    import ctypes as C                                  # noqa: F401
    from ._lib import check, lib
    if isinstance(src_u8, RaggedImageSet):
        args = _ragged_args("augment_batch", src_u8, params)
        ch, n, (Ho, Wo), dev = src_u8.channels, params.shape[0], out_hw, src_u8.device
        m = torch.as_tensor(mean, dtype=torch.float32, device=dev).contiguous() if mean is not None else None
        s = torch.as_tensor(std, dtype=torch.float32, device=dev).contiguous() if std is not None else None
        for name, t in (("mean", m), ("std", s)):
            if t is not None and t.numel() != ch:
                raise ValueError(f"augment_batch: {name} must hold one value per channel ({ch}), not {t.numel()}")
        out = torch.empty((n, ch, Ho, Wo), dtype=torch.float32, device=dev)
        if n:
            check(lib.eoe_ragged_augment_batch(*args, ch, params.data_ptr(), None if m is None else m.data_ptr(),
                                               None if s is None else s.data_ptr(), out.data_ptr(), n, Ho, Wo, 1 if flip_first else 0,
                                               float(noise_std), int(seed), torch.cuda.current_stream().cuda_stream),
                  "eoe_ragged_augment_batch")
        return out
    if not (src_u8.is_cuda and params.is_cuda):
        raise RuntimeError("augment_batch needs GPU tensors (there is no CPU fallback)")
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 4 and src_u8.is_contiguous()
    ch = _channels(src_u8, "augment_batch")
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 4 and params.is_contiguous()
    n, (Ho, Wo) = params.shape[0], out_hw
    dev = src_u8.device
    m = torch.as_tensor(mean, dtype=torch.float32, device=dev).contiguous() if mean is not None else None
    s = torch.as_tensor(std, dtype=torch.float32, device=dev).contiguous() if std is not None else None
    for name, t in (("mean", m), ("std", s)):
        if t is not None and t.numel() != ch:
            raise ValueError(f"augment_batch: {name} must hold one value per channel ({ch}), not {t.numel()}")
    out = torch.empty((n, ch, Ho, Wo), dtype=torch.float32, device=dev)
    check(lib.eoe_augment_batch_c(src_u8.data_ptr(), src_u8.shape[0], src_u8.shape[1], src_u8.shape[2], ch, params.data_ptr(),
                                  None if m is None else m.data_ptr(), None if s is None else s.data_ptr(), out.data_ptr(), n, Ho, Wo,
                                  1 if flip_first else 0, float(noise_std), int(seed), torch.cuda.current_stream().cuda_stream),
          "eoe_augment_batch_c")
    return out


def crop_flip_u8(src_u8, params, out_hw, flip_first=True):
    """the crop / flip of augment_batch alone (`eoe_crop_flip_u8_c`: same params, zero padding, both flip orders): uint8 NHWC
    [n, Ho, Wo, C] (C = 1 or 3, as the set), the PIL image the reference's uint8 transforms see between RandomCrop /
    RandomHorizontalFlip and ToTensor.  A `RaggedImageSet` takes `eoe_ragged_crop_flip_u8` (origins relative to each image)."""
    from ._lib import check, lib
    if isinstance(src_u8, RaggedImageSet):
        args = _ragged_args("crop_flip_u8", src_u8, params)
        n, (Ho, Wo) = params.shape[0], out_hw
        out = torch.empty((n, Ho, Wo, src_u8.channels), dtype=torch.uint8, device=src_u8.device)
        if n:
            check(lib.eoe_ragged_crop_flip_u8(*args, src_u8.channels, params.data_ptr(), out.data_ptr(), n, Ho, Wo,
                                              1 if flip_first else 0, torch.cuda.current_stream().cuda_stream), "eoe_ragged_crop_flip_u8")
        return out
    if not (src_u8.is_cuda and params.is_cuda):
        raise RuntimeError("crop_flip_u8 needs GPU tensors (there is no CPU fallback)")
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 4 and src_u8.is_contiguous()
    ch = _channels(src_u8, "crop_flip_u8")
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 4 and params.is_contiguous()
    n, (Ho, Wo) = params.shape[0], out_hw
    out = torch.empty((n, Ho, Wo, ch), dtype=torch.uint8, device=src_u8.device)
    check(lib.eoe_crop_flip_u8_c(src_u8.data_ptr(), src_u8.shape[0], src_u8.shape[1], src_u8.shape[2], ch, params.data_ptr(),
                                 out.data_ptr(), n, Ho, Wo, 1 if flip_first else 0, torch.cuda.current_stream().cuda_stream),
          "eoe_crop_flip_u8_c")
    return out


def grayscale_u8(src_u8):
    """`transforms.Grayscale(1)` (`main/train_fmnist.py:32`) on a uint8 NHWC colour set [n, H, W, 3] on the GPU -> uint8 [n, H, W, 1],
    byte-exact with Pillow's `Image.convert("L")` that torchvision calls: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
    (`eoe_grayscale_u8`).  Deterministic and first in the chain, so a resident set is converted ONCE, not per sample.  A
    non-contiguous input is made contiguous first (a copy); the result is always a new tensor."""
    from ._lib import check, lib
    if not src_u8.is_cuda:
        raise RuntimeError("grayscale_u8 needs a GPU tensor (there is no CPU fallback)")
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 4
    if src_u8.shape[3] != 3:
        raise ValueError(f"grayscale_u8: images must have 3 channels, not {src_u8.shape[3]}")
    src_u8 = src_u8.contiguous()
    n, H, W, _ = src_u8.shape
    out = torch.empty((n, H, W, 1), dtype=torch.uint8, device=src_u8.device)
    if out.numel():
        check(lib.eoe_grayscale_u8(src_u8.data_ptr(), out.data_ptr(), n * H * W, torch.cuda.current_stream().cuda_stream),
              "eoe_grayscale_u8")
    return out


def _resize_tables_host(in_size, out_size, filt):
    """Pillow's filter taps for one axis from the library's host helper (double precision, the exact part)"""
    import ctypes as C
    from ._lib import check, lib
    k = C.c_int(0)
    check(lib.eoe_resize_coeffs(in_size, out_size, filt, None, None, 0, C.byref(k)), "eoe_resize_coeffs")
    bounds = torch.empty((out_size, 2), dtype=torch.int32)
    kk = torch.empty((out_size, k.value), dtype=torch.int32)
    check(lib.eoe_resize_coeffs(in_size, out_size, filt, bounds.data_ptr(), kk.data_ptr(), k.value, None), "eoe_resize_coeffs")
    return bounds, kk, k.value


def _resize_tables(in_size, out_size, filt, device):
    """the same, uploaded once"""
    bounds, kk, ks = _resize_tables_host(in_size, out_size, filt)
    return bounds.to(device), kk.to(device), ks


class _TapArena:
    """the tap tables of a ragged Resize in ONE int32 array: `eoe_resize_coeffs` runs once per distinct (in, out) of the set -- a
    few hundred for a real set, not once per image -- and an image's pass names its tables by their positions in the array"""

    def __init__(self, filt, tables=_resize_tables_host):
        self.filt, self.tables, self.at, self.chunks, self.seen, self.bounds = filt, tables, 0, [], {}, {}

    def entry(self, in_size, out_size):
        """(position of bounds, position of kk, ksize); (0, 0, 0) for a pass Pillow skips"""
        key = (int(in_size), int(out_size))
        if key[0] == key[1]:
            return 0, 0, 0
        if key not in self.seen:
            bounds, kk, ks = self.tables(key[0], key[1], self.filt)
            self.seen[key] = (self.at, self.at + bounds.numel(), ks)
            self.bounds[key] = bounds.reshape(-1, 2).numpy()
            self.chunks += [bounds.reshape(-1), kk.reshape(-1)]
            self.at += bounds.numel() + kk.numel()
        return self.seen[key]

    def reach(self, in_size, out_size, first, count):
        """[lo, hi): the source positions that the taps of outputs [first, first + count) touch; an identity pass touches its own"""
        if int(in_size) == int(out_size):
            return int(first), int(first) + int(count)
        self.entry(in_size, out_size)
        b = self.bounds[(int(in_size), int(out_size))]
        # Pillow's xmin and xmin + count never decrease with the output position (Resample.c: both follow the tap centre), so the
        # first and the last row of the window span its union
        last = int(first) + int(count) - 1
        return int(b[int(first), 0]), int(b[last, 0]) + int(b[last, 1])

    def tensor(self):
        if self.at >= 1 << 31:
            raise ValueError("resize_u8: the tap tables of this set exceed 2^31 entries")
        return torch.cat(self.chunks) if self.chunks else torch.zeros(1, dtype=torch.int32)


def ragged_resize_plan(sizes, channels, size, taps, src_offsets, packed_out, window=None):
    """the launch geometry of a ragged Resize, on the host (numpy): per image the shapes after the horizontal and after the
    vertical pass (Pillow's order), where each intermediate and each result starts, and the per-axis descriptor rows
    (outer, axis_in, axis_out, inner, bounds_at, kk_at, ksize, first) of `eoe_ragged_resize_pass_u8`.
    packed_out: the results lie back to back without gaps (the [n, h, w, C] tensor of a pair `size`), else at ALIGN-ed starts.
    window: int [n, 4] = (top, left, height, width) per image, a crop of the RESIZED image (CenterCrop behind Resize): only the
    window is computed and written.  The horizontal pass then writes columns [left, left + width) of the source rows [r0, r1) that
    the vertical window's taps touch (`_TapArena.reach`; an image without a vertical pass: the window's own rows) into an
    [r1 - r0, width, C] intermediate, and the vertical pass, whose tables count source rows from 0, gets the position row 0 of that
    intermediate would have: its start minus r0 rows (possibly in front of the intermediate; no tap of the window goes below r0).
    A window outside its resized image is a ValueError.  Without a window every `first` is 0 and the rows are what they always were.
    Returns dict(out_sizes, mid_sizes, mid_offsets, mid_bytes, out_offsets, out_bytes, h=(offs, desc, max_bytes) | None, v=... | None):
    a pass is None only when it is the identity for EVERY image; otherwise its identity images are copied by the kernel."""
    import numpy as np
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    n, C = len(sizes), int(channels)
    full = np.array([resized_hw(h, w, size) for h, w in sizes], dtype=np.int64).reshape(-1, 2)
    if (full < 1).any():
        i = int(np.argmax((full < 1).any(axis=1)))
        raise ValueError(f"resize_u8: image {i} of {tuple(sizes[i])} would become {tuple(full[i])}")
    H, W, Ho, Wo = sizes[:, 0], sizes[:, 1], full[:, 0], full[:, 1]
    zeros = np.zeros(n, dtype=np.int64)
    if window is None:
        top, left, wh, ww, r0, r1 = zeros, zeros, Ho, Wo, zeros, H
    else:
        win = np.asarray(window, dtype=np.int64).reshape(-1, 4)
        if len(win) != n:
            raise ValueError(f"resize_u8: {len(win)} windows for {n} images")
        top, left, wh, ww = win[:, 0], win[:, 1], win[:, 2], win[:, 3]
        bad = (top < 0) | (left < 0) | (wh < 1) | (ww < 1) | (top + wh > Ho) | (left + ww > Wo)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"resize_u8: the window (top, left, height, width) = {tuple(int(v) for v in win[i])} of image {i} lies "
                             f"outside its resized image of {tuple(int(v) for v in full[i])}")
        reach = np.array([taps.reach(H[i], Ho[i], top[i], wh[i]) for i in range(n)], dtype=np.int64).reshape(-1, 2)
        r0, r1 = reach[:, 0], reach[:, 1]
        assert (r0 >= 0).all() and (r1 <= H).all() and (r0 < r1).all()
    out_sizes = np.stack([wh, ww], axis=1)
    need_h, need_v = bool(((W != Wo) | (ww != Wo)).any()), bool(((H != Ho) | (wh != Ho)).any())
    if not need_h:                                       # the vertical pass reads the source images themselves, all their rows
        r0, r1 = zeros, H
    mid_sizes = np.stack([r1 - r0, ww], axis=1)
    mid_offsets, mid_bytes = RaggedImageSet.layout(mid_sizes, C)
    if packed_out:
        nb = wh * ww * C
        out_offsets, out_bytes = np.cumsum(nb) - nb, int(nb.sum())
    else:
        out_offsets, out_bytes = RaggedImageSet.layout(out_sizes, C)
    src_offsets = np.asarray(src_offsets, dtype=np.int64)

    def axis_pass(src_off, dst_off, outer, a_in, a_full, a_out, inner, first):
        ent = {}
        for pair in set(zip(a_in.tolist(), a_full.tolist())):
            ent[pair] = taps.entry(*pair)
        e = np.array([ent[p] for p in zip(a_in.tolist(), a_full.tolist())], dtype=np.int64).reshape(-1, 3)
        desc = np.stack([outer, a_in, a_out, inner, e[:, 0], e[:, 1], e[:, 2], first], axis=1)
        if desc.max() >= 1 << 31:
            raise ValueError("resize_u8: an image of this set is too large for the pass descriptors (2^31)")
        return (np.ascontiguousarray(np.stack([src_off, dst_off], axis=1).astype(np.int64)), np.ascontiguousarray(desc.astype(np.int32)),
                int((outer * a_out * inner).max()))

    ones, cs = np.ones(n, dtype=np.int64), np.full(n, C, dtype=np.int64)
    plan = dict(out_sizes=out_sizes.astype(np.int32), mid_sizes=mid_sizes.astype(np.int32), mid_offsets=mid_offsets, mid_bytes=mid_bytes,
                out_offsets=out_offsets.astype(np.int64), out_bytes=out_bytes, h=None, v=None)
    if need_h:                                           # rows [r0, r1) of [H, W, C] -> [r1 - r0, ww, C]: into the scratch when a vertical pass follows
        plan["h"] = axis_pass(src_offsets + r0 * W * C, mid_offsets if need_v else plan["out_offsets"], r1 - r0, W, Wo, ww, cs, left)
    if need_v:                                           # [H, ww, C] -> [wh, ww, C], the row is `inner`
        plan["v"] = axis_pass(mid_offsets - r0 * ww * C if need_h else src_offsets, plan["out_offsets"], ones, H, Ho, wh, ww * C, top)
    return plan


def _run_resize_plan(rs, plan, taps, out):
    """the one or two launches of a plan of `ragged_resize_plan` over the set `rs`, into the flat uint8 `out`"""
    from ._lib import check, lib
    n, dev = len(rs), rs.device
    st = torch.cuda.current_stream().cuda_stream
    taps_dev = taps.tensor().to(dev)
    mid = torch.empty(plan["mid_bytes"], dtype=torch.uint8, device=dev) if plan["h"] and plan["v"] else None     # freed on return
    cur = rs.arena
    for name in ("h", "v"):
        if plan[name] is None:
            continue
        offs, desc, biggest = plan[name]
        dst = mid if (name == "h" and plan["v"] is not None) else out
        offs_d, desc_d = torch.from_numpy(offs).to(dev), torch.from_numpy(desc).to(dev)
        check(lib.eoe_ragged_resize_pass_u8(cur.data_ptr(), dst.data_ptr(), offs_d.data_ptr(), desc_d.data_ptr(), taps_dev.data_ptr(), n,
                                            biggest, st), "eoe_ragged_resize_pass_u8")
        cur = dst


def _resize_ragged(rs, size, filt):
    if not rs.is_cuda:
        raise RuntimeError("resize_u8 needs the set on a GPU (there is no CPU fallback)")
    pair = not isinstance(size, int)
    taps = _TapArena(filt)
    plan = ragged_resize_plan(rs.sizes, rs.channels, size, taps, rs.offsets_host, pair)
    n, C, dev = len(rs), rs.channels, rs.device
    if plan["h"] is None and plan["v"] is None:          # Resize leaves every image as it is
        return rs.as_tensor() if pair else rs
    out = torch.zeros(plan["out_bytes"], dtype=torch.uint8, device=dev)        # zeros: the gaps between aligned starts
    _run_resize_plan(rs, plan, taps, out)
    if pair:
        h, w = plan["out_sizes"][0]
        return out.view(n, int(h), int(w), C)
    return RaggedImageSet.from_parts(out, plan["out_offsets"], plan["out_sizes"], C)


def resize_window_u8(rs, size, window, interpolation="bilinear", out=None):
    """Resize(size) of every image of a `RaggedImageSet`, then the crop `window` = (top, left, height, width) of the resized image --
    int [n, 4], one height and one width for the whole set -- computing only the window: uint8 [n, height, width, C], byte for
    byte `resize_u8(rs, size, interpolation)` followed by that crop.  Each pass of `eoe_ragged_resize_pass_u8` writes its window of
    the output axis, and the horizontal pass runs only over the source rows the vertical window's taps touch
    (`ragged_resize_plan`).  A window that leaves its resized image is a ValueError before any launch.
    out: a contiguous uint8 tensor of that shape on the set's device to write into (default: a new one)."""
    import numpy as np
    from ._lib import EOE_RESIZE_BILINEAR, EOE_RESIZE_BICUBIC
    if not isinstance(rs, RaggedImageSet):
        raise TypeError("resize_window_u8 works on a RaggedImageSet (a tensor set takes resize_u8, then crop_flip_u8)")
    if interpolation not in ("bilinear", "bicubic"):
        raise ValueError(f"resize_window_u8: interpolation must be 'bilinear' or 'bicubic', not {interpolation!r}")
    win = np.asarray(window, dtype=np.int64).reshape(-1, 4)
    if len(win) != len(rs) or (win[:, 2:] != win[0, 2:]).any():
        raise ValueError(f"resize_window_u8: one (top, left, height, width) per image with one height and width is needed "
                         f"({len(win)} rows for {len(rs)} images)")
    taps = _TapArena(EOE_RESIZE_BILINEAR if interpolation == "bilinear" else EOE_RESIZE_BICUBIC)
    plan = ragged_resize_plan(rs.sizes, rs.channels, size, taps, rs.offsets_host, True, win)
    shape = (len(rs), int(win[0, 2]), int(win[0, 3]), rs.channels)
    if out is not None and not (out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous() and out.device == rs.device):
        raise ValueError(f"resize_window_u8: out must be a contiguous uint8 {list(shape)} on {rs.device}")
    if not rs.is_cuda:
        raise RuntimeError("resize_window_u8 needs the set on a GPU (there is no CPU fallback)")
    if plan["h"] is None and plan["v"] is None:          # every window is its whole image, which Resize leaves as it is
        return rs.as_tensor() if out is None else out.copy_(rs.as_tensor())
    out = torch.empty(shape, dtype=torch.uint8, device=rs.device) if out is None else out
    _run_resize_plan(rs, plan, taps, out)
    return out


def resize_u8(src_u8, size, interpolation="bilinear"):
    """`torchvision.transforms.Resize(size)` as the reference applies it to PIL images (`main/train_imagenet.py:31`,
    `main/train_clip_imagenet.py:28`; bicubic for CLIP's preprocessing, `clip_official/clip/clip.py:60`), on a uint8 NHWC image
    set in HBM and byte-exact with Pillow: `size` = (h, w), or an int = the shorter side (the other int(size * long / short)).
    Deterministic, so a resident dataset is resized ONCE, not per step.
    A `RaggedImageSet` is resized image by image under the same rule (`resized_hw`), all images in one launch per pass
    (`eoe_ragged_resize_pass_u8`): an int gives a new RaggedImageSet (256 x W' or H' x 256 per image), a pair the plain tensor
    [n, h, w, C] -- how `Resize((256, 256))` of `main/train_clip_imagenet.py:28` turns a raw mixed set into the tensor path."""
    from ._lib import check, lib, EOE_RESIZE_BILINEAR, EOE_RESIZE_BICUBIC
    if isinstance(src_u8, RaggedImageSet):
        return _resize_ragged(src_u8, size, {"bilinear": EOE_RESIZE_BILINEAR, "bicubic": EOE_RESIZE_BICUBIC}[interpolation])
    if not src_u8.is_cuda:
        raise RuntimeError("resize_u8 needs a GPU tensor (there is no CPU fallback)")
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 4 and src_u8.is_contiguous()
    filt = {"bilinear": EOE_RESIZE_BILINEAR, "bicubic": EOE_RESIZE_BICUBIC}[interpolation]
    n, H, W, _ = src_u8.shape
    ch = _channels(src_u8, "resize_u8")                  # the passes work on [outer, axis, inner] bytes: the channels are `inner`
    if isinstance(size, int):
        Ho, Wo = (int(size * H / W), size) if W <= H else (size, int(size * W / H))
    else:
        Ho, Wo = size
    st = torch.cuda.current_stream().cuda_stream
    cur = src_u8
    if Wo != W:
        b, k, ks = _resize_tables(W, Wo, filt, src_u8.device)
        nxt = torch.empty((n, H, Wo, ch), dtype=torch.uint8, device=src_u8.device)
        check(lib.eoe_resize_pass_u8(cur.data_ptr(), nxt.data_ptr(), b.data_ptr(), k.data_ptr(), ks, n * H, W, Wo, ch, st), "eoe_resize_pass_u8")
        cur = nxt
    if Ho != H:
        b, k, ks = _resize_tables(H, Ho, filt, src_u8.device)
        nxt = torch.empty((n, Ho, Wo, ch), dtype=torch.uint8, device=src_u8.device)
        check(lib.eoe_resize_pass_u8(cur.data_ptr(), nxt.data_ptr(), b.data_ptr(), k.data_ptr(), ks, n, H, Ho, Wo * ch, st), "eoe_resize_pass_u8")
        cur = nxt
    return cur


def color_jitter_u8(src_u8, idx, factors, order):
    """`torchvision.transforms.ColorJitter` with its random draws made explicit (`main/train_cifar.py:32`,
    `main/train_clip_imagenet.py:29`: brightness = contrast = saturation = hue = 0.01), byte-exact with Pillow: gathers
    src_u8[idx] (uint8 NHWC) and applies, per image, the four ops in `order` (int32 [n, 4], a permutation of 0 brightness,
    1 contrast, 2 saturation, 3 hue) with `factors` (fp32 [n, 4] = b, c, s around 1 and h around 0) -> uint8 [n, H, W, 3]"""
    from ._lib import check, lib
    if not src_u8.is_cuda:
        raise RuntimeError("color_jitter_u8 needs GPU tensors (there is no CPU fallback)")
    if src_u8.dim() != 4 or src_u8.shape[3] != 3:
        raise ValueError(f"color_jitter_u8: images must have 3 channels, not {src_u8.shape[-1]} (the ops are defined on RGB)")
    dev = src_u8.device
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    factors = factors.to(device=dev, dtype=torch.float32).contiguous()
    order = order.to(device=dev, dtype=torch.int32).contiguous()
    n, (_, H, W, _) = idx.shape[0], src_u8.shape
    assert factors.shape == (n, 4) and order.shape == (n, 4) and src_u8.dtype == torch.uint8 and src_u8.is_contiguous()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    scratch = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.eoe_color_jitter_u8(src_u8.data_ptr(), src_u8.shape[0], idx.data_ptr(), factors.data_ptr(), order.data_ptr(),
                                  scratch.data_ptr(), out.data_ptr(), n, H, W, torch.cuda.current_stream().cuda_stream), "eoe_color_jitter_u8")
    return out


def color_jitter_crop_u8(src, params, out_hw, factors, order, flip_first=True):
    """ColorJitter of the WHOLE image params[slot, 0] of a `RaggedImageSet` (3 channels), then the crop / flip of `crop_flip_u8`
    with the same params -> uint8 [n, Ho, Wo, 3], equal byte for byte to `color_jitter_u8` on that image followed by `crop_flip_u8`
    (`eoe_ragged_color_jitter_crop_u8`).  The jittered whole image is never written: the contrast op needs the rounded gray mean of
    the whole image as it stands in front of that op, every op is pointwise once it is known, so one pass sums over the slot's
    image and the second jitters only the pixels under the crop window.  The zero padding stays 0 (RandomCrop pads after the
    jitter).  factors fp32 [n, 4], order int32 [n, 4] as `color_jitter_u8` takes them."""
    from ._lib import check, lib
    if not isinstance(src, RaggedImageSet):
        raise TypeError("color_jitter_crop_u8 works on a RaggedImageSet (a tensor set takes color_jitter_u8, then crop_flip_u8)")
    if src.channels != 3:
        raise ValueError(f"color_jitter_crop_u8: images must have 3 channels, not {src.channels} (the ops are defined on RGB)")
    args = _ragged_args("color_jitter_crop_u8", src, params)
    dev, n, (Ho, Wo) = src.device, params.shape[0], out_hw
    factors = factors.to(device=dev, dtype=torch.float32).contiguous()
    order = order.to(device=dev, dtype=torch.int32).contiguous()
    assert factors.shape == (n, 4) and order.shape == (n, 4)
    out = torch.empty((n, Ho, Wo, 3), dtype=torch.uint8, device=dev)
    if n:
        scratch = torch.empty(n, dtype=torch.int32, device=dev)
        check(lib.eoe_ragged_color_jitter_crop_u8(*args, params.data_ptr(), factors.data_ptr(), order.data_ptr(), scratch.data_ptr(),
                                                  out.data_ptr(), n, Ho, Wo, 1 if flip_first else 0,
                                                  torch.cuda.current_stream().cuda_stream), "eoe_ragged_color_jitter_crop_u8")
    return out


def sample_color_jitter(n, brightness, contrast, saturation, hue, generator=None):
    """the draws of `ColorJitter.get_params`: a random permutation of the four ops and uniform factors in
    [max(0, 1 - x), 1 + x] (hue: [-x, x]) per image"""
    order = torch.stack([torch.randperm(4, generator=generator) for _ in range(n)]).to(torch.int32)
    u = torch.rand((n, 4), generator=generator)
    lo = torch.tensor([max(0.0, 1 - brightness), max(0.0, 1 - contrast), max(0.0, 1 - saturation), -hue])
    hi = torch.tensor([1 + brightness, 1 + contrast, 1 + saturation, hue])
    return (lo + u * (hi - lo)).to(torch.float32), order


CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)      # clip.py:64


def clip_preprocess(src_u8, n_px=224):
    """CLIP's `_transform` (`clip_official/clip/clip.py:58-65`): Resize(n_px, bicubic) -> CenterCrop(n_px) -> ToTensor ->
    Normalize(CLIP mean / std), on a uint8 NHWC set in HBM -> fp32 NCHW.  A `RaggedImageSet` (RGB) goes through
    `clip_preprocess_ragged`: each image is resized at its own aspect ratio and only its centre window is computed."""
    if isinstance(src_u8, RaggedImageSet):
        u8 = clip_preprocess_ragged(src_u8, n_px)
        p = torch.zeros((u8.shape[0], 4), dtype=torch.int32)
        p[:, 0] = torch.arange(u8.shape[0], dtype=torch.int32)
        return augment_batch(u8, p.to(u8.device), (int(n_px), int(n_px)), CLIP_MEAN, CLIP_STD, True, 0.0, 0)
    r = resize_u8(src_u8, n_px, "bicubic")
    n, H, W, _ = r.shape
    # torchvision's CenterCrop: top = int(round((H - n_px) / 2.0))
    idx = torch.arange(n)
    p = torch.stack([idx, torch.full_like(idx, int(round((H - n_px) / 2.0))), torch.full_like(idx, int(round((W - n_px) / 2.0))),
                     torch.zeros_like(idx)], dim=1).to(torch.int32).to(r.device)
    return augment_batch(r, p, (n_px, n_px), CLIP_MEAN, CLIP_STD, True, 0.0, 0)


def clip_window(sizes, n_px):
    """int64 [n, 4] = (top, left, n_px, n_px): where CLIP's CenterCrop(n_px) lies in each image of `sizes` (int [n, 2]) after its
    Resize(n_px) -- the `resized_hw` target, the origin torchvision's, int(round((s - n_px) / 2.0)) with Python's half-to-even
    (`center_origins`).  The shorter side becomes n_px, so the window lies inside the resized image and cuts only the longer axis."""
    import numpy as np
    full = np.array([resized_hw(h, w, int(n_px)) for h, w in np.asarray(sizes).reshape(-1, 2)], dtype=np.int64).reshape(-1, 2)
    return np.concatenate([center_origins(full, n_px), np.full((len(full), 2), int(n_px), dtype=np.int64)], axis=1)


def clip_preprocess_ragged(rs, n_px=224, out=None):
    """the PIL part of CLIP's `_transform` on RAW images of mixed sizes (`clip_official/clip/clip.py:58-65`, what the test split of
    `main/train_clip_imagenet.py`, `train_clip_cub.py`, `train_clip_dtd.py`, `train_clip_mvtec.py` gets: `val_transform` is empty,
    `training/clip.py:44-46`): Resize(n_px, BICUBIC) with the aspect ratio kept, then CenterCrop(n_px) -> uint8 [n, n_px, n_px, 3],
    packed, byte for byte Pillow's `resize` at `resized_hw` followed by the crop at torchvision's origin.  Only the window is
    computed (`resize_window_u8`): 224 of the 298 columns of a 4 : 3 image.  The filter is CLIP's bicubic.  RGB only."""
    if not isinstance(rs, RaggedImageSet):
        raise TypeError("clip_preprocess_ragged works on a RaggedImageSet (a tensor set takes clip_preprocess)")
    if rs.channels != 3:
        raise ValueError(f"clip_preprocess_ragged: the ragged CLIP path is RGB only, not {rs.channels} channel(s): convert the images "
                         "to RGB before packing them")
    if int(n_px) < 1:
        raise ValueError(f"clip_preprocess_ragged: n_px must be positive, not {n_px}")
    return resize_window_u8(rs, int(n_px), clip_window(rs.sizes, n_px), "bicubic", out)


_TAP_TABLES = {}             # (crop, n_px, filter, device) -> (bounds, kk) on that device: uploaded once, not per step


def _cached_resize_tables(in_size, out_size, filt, device):
    key = (int(in_size), int(out_size), int(filt), str(device))
    if key not in _TAP_TABLES:
        _TAP_TABLES[key] = _resize_tables(in_size, out_size, filt, device)[:2]
    return _TAP_TABLES[key]


def augment_resize_batch(src_u8, params, crop, n_px, mean=None, std=None, flip_first=True, noise_std=0.001, seed=0,
                         interpolation="bicubic"):
    """the tail of the reference's small-image CLIP chains (`main/train_clip_cifar.py:26-35`, `train_clip_fmnist.py:27-36`,
    `train_clip_mnist.py:25-29`) in ONE kernel (`eoe_augment_resize_batch`): gather + RandomCrop(crop, zero padding) +
    RandomHorizontalFlip, then 'clip_pil_preprocessing' (`training/clip.py:34-43`: Resize(n_px, BICUBIC) -> CenterCrop(n_px) ->
    convert("RGB")), ToTensor, noise, Normalize.  The upsample follows the random crop, so it cannot be done once on the resident
    set as `resize=` is; per slot the crop, Pillow's two uint8 passes and the L -> RGB replication run out of LDS, byte-exact with
    `crop_flip_u8 -> resize_u8`, and only the fp32 batch is written.
    src_u8 uint8 [n_src,Hs,Ws,C] (GPU), C = 1 or 3; params int32 [n,4] = (index, top, left, flip) (GPU); crop: the square crop's
    side (<= 64); n_px >= crop (<= 256) -> fp32 NCHW [n,3,n_px,n_px]; mean / std hold three values, also for C = 1"""
    from ._lib import check, lib, EOE_RESIZE_BILINEAR, EOE_RESIZE_BICUBIC
    if not (src_u8.is_cuda and params.is_cuda):
        raise RuntimeError("augment_resize_batch needs GPU tensors (there is no CPU fallback)")
    assert src_u8.dtype == torch.uint8 and src_u8.dim() == 4 and src_u8.is_contiguous()
    ch = _channels(src_u8, "augment_resize_batch")
    assert params.dtype == torch.int32 and params.dim() == 2 and params.shape[1] == 4 and params.is_contiguous()
    if interpolation not in ("bilinear", "bicubic"):
        raise ValueError(f"augment_resize_batch: interpolation must be 'bilinear' or 'bicubic', not {interpolation!r}")
    filt = EOE_RESIZE_BILINEAR if interpolation == "bilinear" else EOE_RESIZE_BICUBIC
    ch_crop, cw_crop = (crop, crop) if isinstance(crop, int) else (int(crop[0]), int(crop[1]))
    n_px = int(n_px)
    if ch_crop != cw_crop:
        raise ValueError(f"augment_resize_batch: the crop must be square, not {ch_crop} x {cw_crop} (CenterCrop after Resize is the "
                         "identity only for square crops)")
    if not 0 < ch_crop <= n_px:
        raise ValueError(f"augment_resize_batch: {ch_crop} -> {n_px} is not an upsample (only n_px >= crop is built)")
    n, dev = params.shape[0], src_u8.device
    m = torch.as_tensor(mean, dtype=torch.float32, device=dev).contiguous() if mean is not None else None
    s = torch.as_tensor(std, dtype=torch.float32, device=dev).contiguous() if std is not None else None
    for name, t in (("mean", m), ("std", s)):
        if t is not None and t.numel() != 3:
            raise ValueError(f"augment_resize_batch: {name} must hold three values (the batch is RGB), not {t.numel()}")
    out = torch.empty((n, 3, n_px, n_px), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    bounds, kk = _cached_resize_tables(ch_crop, n_px, filt, dev)
    check(lib.eoe_augment_resize_batch(src_u8.data_ptr(), src_u8.shape[0], src_u8.shape[1], src_u8.shape[2], ch, params.data_ptr(),
                                       ch_crop, cw_crop, n_px, filt, bounds.data_ptr(), kk.data_ptr(),
                                       None if m is None else m.data_ptr(), None if s is None else s.data_ptr(), out.data_ptr(), n,
                                       1 if flip_first else 0, float(noise_std), int(seed), torch.cuda.current_stream().cuda_stream),
          "eoe_augment_resize_batch")
    return out


def gray_set(images_u8, device):
    """a resident set under `Grayscale(1)`: `[n, H, W]` is taken as `[n, H, W, 1]`, a 3-channel set is converted once on the
    device (`grayscale_u8`), a 1-channel set passes through (Grayscale(1) of an `L` image is the identity)"""
    t = images_u8.unsqueeze(-1) if images_u8.dim() == 3 else images_u8
    if t.dim() != 4 or t.shape[3] not in (1, 3):
        raise ValueError(f"grayscale: an image set is [n, H, W], [n, H, W, 1] or [n, H, W, 3], not {list(images_u8.shape)}")
    t = t.to(device).contiguous()
    return grayscale_u8(t) if t.shape[3] == 3 else t


def _resident(t, device):
    """an image set as the source keeps it: on the device; a tensor contiguous, a RaggedImageSet as packed"""
    return t.to(device) if isinstance(t, RaggedImageSet) else t.to(device).contiguous()


def _set_channels(t):
    """the channel count of a resident image set, a tensor [n, H, W, C] or a RaggedImageSet"""
    return t.channels if isinstance(t, RaggedImageSet) else int(t.shape[3])


def _check_clip_ragged_half(what, rs, crop, n_px):
    """`clip_preprocessing` on a train half that stays ragged (`main/train_clip_cub.py:26`, `train_clip_dtd.py:26`: Resize(256) keeps
    the aspect ratio): after RandomCrop(n_px) CLIP's PIL stage is the identity on RGB, so the ragged chain runs as it is, with CLIP's
    Normalize.  Any other crop would need the per-sample upsample of a ragged crop, which no runner has"""
    if int(crop) != n_px:
        raise NotImplementedError(f"clip_preprocessing on a RaggedImageSet needs crop == n_px (the {what} set is ragged, crop {crop}, "
                                  f"n_px {n_px}): resampling a ragged crop per sample is not built, and no runner of the reference "
                                  "needs it (a pair `resize=` gives the tensor path)")
    if rs.channels != 3:
        raise ValueError(f"clip_preprocessing on a RaggedImageSet is RGB only; the {what} set has {rs.channels} channel(s): convert "
                         "the images to RGB before packing them")


def _check_clip_ragged_test(rs, test_resize, device):
    """`clip_preprocessing` with a ragged test set: CLIP's own transform runs alone on the RAW test images, once, at construction
    (`clip_preprocess_ragged`), which is a HIP kernel"""
    if test_resize is not None:
        raise ValueError("test_resize= cannot be combined with clip_preprocessing on a ragged test set: CLIP's transform is applied to "
                         "the raw test images (val_transform is empty, training/clip.py:44-46)")
    if rs.channels != 3:
        raise ValueError(f"clip_preprocessing on a RaggedImageSet is RGB only; the test set has {rs.channels} channel(s): convert the "
                         "images to RGB before packing them")
    if torch.device(device).type != "cuda":
        raise NotImplementedError("clip_preprocessing on a RaggedImageSet test set is applied at construction by a HIP kernel (the "
                                  f"windowed ragged Resize): not built for device {str(device)!r}")


def _check_crop_fits(what, rs, crop, padding):
    """RandomCrop(crop, padding) on a ragged set fails in torchvision for an image that is smaller than the crop after padding
    ("Required crop size ... is larger than input image size ..."): found here, once, not in some later step"""
    small = ((rs.sizes + 2 * int(padding)) < int(crop)).any(axis=1)
    if small.any():
        i = int(small.argmax())
        h, w = (int(v) for v in rs.sizes[i])
        raise ValueError(f"required crop size ({crop}, {crop}) is larger than {what} image {i} of size ({h}, {w}) after Resize"
                         + (f" and padding {padding}" if padding else "") + f" ({int(small.sum())} such image(s) in the set)")


def center_origins(sizes, crop):
    """torchvision's CenterCrop origin per image and axis, int64 [n, 2]: int(round((H - crop) / 2.0)) (Python's round: halves to
    even), and for an image smaller than the crop the origin its symmetric zero padding implies, -((crop - H) // 2)"""
    import numpy as np
    d = np.asarray(sizes, dtype=np.int64) - int(crop)
    return np.where(d >= 0, np.rint(d / 2.0).astype(np.int64), -((-d) // 2))


def ragged_crop_origins(sizes, crop, padding, generator=None):
    """RandomCrop(crop, padding) origins for images of `sizes` (int [n, 2]), relative to each UNPADDED image, int64 [n, 2] =
    (top, left): per image uniform over its own legal origins [-padding, H_i + padding - crop] (W likewise).  ONE vectorised draw per
    coordinate, all tops first, then all lefts: u = torch.rand(n, float64) from the generator, origin = -padding + floor(u * k_i)
    with k_i = H_i + 2 * padding - crop + 1 the number of legal origins (every origin has probability 1 / k_i up to 2^-53)."""
    hw = torch.as_tensor(sizes, dtype=torch.int64).reshape(-1, 2)
    k = hw + 2 * int(padding) - int(crop) + 1
    if len(k) and int(k.min()) < 1:
        raise ValueError("ragged_crop_origins: an image is smaller than the crop after padding")
    cols = []
    for a in (0, 1):
        u = torch.rand(len(k), generator=generator, dtype=torch.float64)
        cols.append(torch.minimum((u * k[:, a].to(torch.float64)).floor().to(torch.int64), k[:, a] - 1) - int(padding))
    return torch.stack(cols, dim=1)


class ResidentImageSource:
    """step-batch source whose uint8 images live in HBM: every step batch ([normal half | OE half], the BalancedConcatLoader
    contract of `datasets/bases.py:570-600`) is gathered, cropped, flipped, noised and normalised by one kernel; the host only
    draws (index, crop origin, flip) per sample.  Batches come out already normalised, so `.normalize` is None (the trainer
    then installs no second Normalize).

    `normalize` (optional): one of the reference's transform strings ('normalize' / 'gcn-normalize' and their spellings,
    eoe_amd.normalize.NORM_MODES) instead of ready `mean` / `std`: the statistics are fitted as the reference fits them
    (`bases.py:293-372`) over the resident normal set after `resize`, restricted to `normal_index`, unless `ds_statistics` (the
    dict of a snapshot) is given, which wins (`bases.py:326-329`).  `.ds_statistics` then holds the dict.  'normalize' feeds the
    `mean` / `std` path; under 'gcn-normalize' batches leave in the [0, 1] scale and `.normalize` is a
    `GcnNormalize(shift, range, 'l1')` that the trainer runs on the step batch.

    `normal_index` (optional): the rows of `normal_u8` that ARE the normal training set -- the reference's `Subset` over the
    samples of the normal classes (`bases.py:169-203`); batches report those rows' indices in the full set, as the reference's
    datasets do (`cifar.py:106-121`), and OE indices are offset by the length of the FULL normal set (`bases.py:596`).

    `grayscale=True` is the 1-channel chain of the 28 x 28 tasks (`main/train_fmnist.py:31-38`: Grayscale(1) -> flip ->
    RandomCrop(28, padding=3) -> ToTensor -> noise -> 'normalize'): a resident set that arrives with 3 channels is converted once
    with `grayscale_u8` (Grayscale is deterministic and first in the chain), one that is gray already passes through, as
    Grayscale(1) of an `L` image is the identity; `[n, H, W]` sets are taken as `[n, H, W, 1]`.  The normal and the OE set may
    differ in size (28 x 28 and 32 x 32): the crop origin is drawn per half.  Batches are `[., 1, crop, crop]`, statistics have one
    element.  ColorJitter is defined on RGB and is in no 1-channel chain of the reference: together with `grayscale` it is refused.

    `flip=False` leaves RandomHorizontalFlip out (`main/train_mnist.py`: no flip, no crop, no noise): the flip bits are zeros and
    NO flip draw is made, as an empty `Compose` draws nothing -- the generator then yields other crop origins in later steps than
    with `flip=True`, whose draw order is what it always was.

    `clip_preprocessing=n_px` puts CLIP's own transform where the reference's small-image CLIP runners have it
    (`main/train_clip_cifar.py:26-35`, `train_clip_fmnist.py:27-36`, `train_clip_mnist.py:25-29`): after RandomCrop / flip and before
    ToTensor, 'clip_pil_preprocessing' = Resize(n_px, BICUBIC) -> CenterCrop(n_px) -> convert("RGB") (`training/clip.py:34-43`), and
    Normalize with CLIP's mean / std (the defaults then; `mean` / `std` take three values, also under `grayscale=True`).  The
    upsample follows the random crop, so it runs per sample per step: each half is one `augment_resize_batch` launch in place of
    `augment_batch`; draws and draw order are unchanged, ColorJitter still comes first.  Batches are `[., 3, n_px, n_px]`.  Test
    batches get CLIP's transform alone on the raw test images (`val_transform` is empty, `training/clip.py:44-46`), which must be
    square, and are built one at a time while the loader is iterated.  Where the stage is the identity -- a 3-channel set whose
    crop (test images: whose size) is n_px already -- the path without the option runs, bit for bit.  Only square crops of at
    most 64 px and upsampling to at most 256 px are built; `normalize=` / `ds_statistics=` (statistics fitted on the set) and a
    pre-tensor sharpen MSM are refused with it.

    Each of `normal_u8`, `oe_u8`, `test_u8` may be a `RaggedImageSet` -- images of mixed sizes, the chains of
    `main/train_imagenet.py:30-41` (Resize(256) -> ColorJitter -> RandomCrop(224) -> flip; test: Resize(256) -> CenterCrop(224)),
    `train_cub.py`, `train_dtd.py`, `train_mvtec.py`, `train_custom.py` -- independently of the other two:
      * `resize=` / `test_resize=` run the ragged Resize once; an int keeps every image's aspect ratio;
      * a crop origin is drawn per sample over THAT image's legal origins (`ragged_crop_origins`: one vectorised draw for the tops,
        one for the lefts, then the flips, where the tensor path has its three draws; the tensor path's draws are unchanged); an
        image smaller than the crop after Resize and padding is a ValueError here, at construction;
      * with `color_jitter` a ragged half takes `color_jitter_crop_u8` and then `augment_batch` with identity params (the shape of
        the sharpen path); the jitter draws and their place in the draw order are those of the tensor path;
      * test batches are CenterCrop(crop) per image at torchvision's origin (`center_origins`);
      * `normalize=` fits over the uint8 tensor Resize -> CenterCrop(crop) of the normal rows, as the reference does
        (`datasets/imagenet.py:89-93, 273-278`), with the unchanged `fit_statistics`.  (The tensor path fits over the whole resized
        images, which is the same thing only where the crop is the image.)
      * `normal_index`, `set_oe_subset`, MSMs and `defer_normalize` work as on tensors: they select rows or act on the batch.
      * `clip_preprocessing=n_px` with ragged sets is the chain of the 224 x 224 CLIP runners (`main/train_clip_imagenet.py`,
        `train_clip_cub.py`, `train_clip_dtd.py`, `train_clip_mvtec.py`), each set on its own.  A ragged TEST set gets CLIP's
        transform alone on the raw images -- Resize(n_px, BICUBIC) at each image's aspect ratio, CenterCrop(n_px) -- once, at
        construction (`clip_preprocess_ragged`: only the centre window is computed), and becomes a `[n, n_px, n_px, 3]` tensor whose
        batches take the identity path; `test_resize=` is a ValueError with it, since CLIP's transform works on the raw images.  A
        ragged NORMAL / OE set (after `resize=int`; a pair `resize=` gives the tensor and the tensor path) needs `crop == n_px`:
        after RandomCrop(n_px) CLIP's PIL stage is the identity on RGB, so the ragged chain above runs unchanged -- same draws, draw
        order and kernels as without the option -- with CLIP's mean / std (or the given three values).  Another crop is a
        NotImplementedError (no runner resamples a ragged crop), a 1-channel ragged set a ValueError: the ragged CLIP path is RGB.
    `grayscale=True` is refused with a ragged set."""

    nominal_label, anomalous_label = 0, 1
    test_classes = None                # the test rows' original class ids (int64 [n_test]) when the source comes from a LabelledImageSet

    def __init__(self, normal_u8, oe_u8, test_u8, test_labels, crop, padding=0, mean=None, std=None, flip_first=True,
                 noise_std=0.001, seed=0, device="cuda", resize=None, test_resize=None, color_jitter=None, interpolation="bilinear",
                 normal_index=None, normalize=None, ds_statistics=None, grayscale=False, flip=True, clip_preprocessing=None):
        """resize / test_resize: `transforms.Resize` argument applied once to the resident train / test sets (None: as given);
        color_jitter: (brightness, contrast, saturation, hue) of `transforms.ColorJitter`, drawn per sample per step;
        clip_preprocessing: n_px of CLIP's transform inside the chain (the class docstring)"""
        dev = torch.device(device)
        if grayscale and any(isinstance(t, RaggedImageSet) for t in (normal_u8, oe_u8, test_u8)):
            raise NotImplementedError("grayscale=True on a RaggedImageSet is not built: convert the images to one channel before "
                                      "packing them (a 1-channel RaggedImageSet is accepted)")
        if clip_preprocessing is not None:
            if normalize is not None or ds_statistics is not None:
                raise ValueError("clip_preprocessing normalises with CLIP's own (or the given three-valued) mean / std, as "
                                 "'clip_tensor_preprocessing' does; it cannot be combined with normalize= / ds_statistics=")
            if not isinstance(crop, int):
                if len(crop) != 2 or int(crop[0]) != int(crop[1]):
                    raise ValueError(f"clip_preprocessing needs a square crop, not {tuple(crop)}: CenterCrop(n_px) after "
                                     "Resize(n_px) is the identity only then")
                crop = int(crop[0])
            if not 0 < crop <= int(clip_preprocessing):
                raise NotImplementedError(f"clip_preprocessing={clip_preprocessing} on a crop of {crop}: only upsampling "
                                          "(n_px >= crop) is built")
            if mean is None and std is None:
                mean, std = CLIP_MEAN, CLIP_STD
            # a ragged half stays ragged unless `resize` is a pair (which gives the tensor): CLIP's PIL stage is then the identity
            # only on an RGB crop of n_px, and Normalize with CLIP's statistics is all that is new
            for what, t in (("normal", normal_u8), ("OE", oe_u8)):
                if isinstance(t, RaggedImageSet) and (resize is None or isinstance(resize, int)):
                    _check_clip_ragged_half(what, t, crop, int(clip_preprocessing))
            if isinstance(test_u8, RaggedImageSet):
                _check_clip_ragged_test(test_u8, test_resize, dev)
        if grayscale and color_jitter is not None:
            raise ValueError("color_jitter works on RGB images and cannot be combined with grayscale=True (no chain of the "
                             "reference has both)")
        if grayscale:
            self.normal, self.oe, self.test = (gray_set(t, dev) for t in (normal_u8, oe_u8, test_u8))
        else:
            self.normal, self.oe, self.test = (_resident(t, dev) for t in (normal_u8, oe_u8, test_u8))
        self.grayscale, self.flip = bool(grayscale), bool(flip)
        if resize is not None:
            self.normal, self.oe = resize_u8(self.normal, resize, interpolation), resize_u8(self.oe, resize, interpolation)
        if test_resize is not None:
            self.test = resize_u8(self.test, test_resize, interpolation)
        if clip_preprocessing is not None and isinstance(self.test, RaggedImageSet):
            # CLIP's transform alone on the raw test images (val_transform is empty, training/clip.py:44-46): deterministic, so it runs
            # once, here; the test batches then take the identity path (a 3-channel set whose size is n_px already)
            self.test = clip_preprocess_ragged(self.test, int(clip_preprocessing))
        self.color_jitter = color_jitter
        self.test_y = test_labels.clone()
        self.crop, self.padding, self.mean, self.std = int(crop), int(padding), mean, std
        if color_jitter is not None and any(isinstance(t, RaggedImageSet) and t.channels != 3 for t in (self.normal, self.oe)):
            raise ValueError("color_jitter works on RGB images; a 1-channel RaggedImageSet cannot take it")
        for what, t in (("normal", self.normal), ("OE", self.oe)):
            if isinstance(t, RaggedImageSet):
                _check_crop_fits(what, t, self.crop, self.padding)
        self.flip_first, self.noise_std, self.seed = flip_first, noise_std, int(seed)
        self.clip_preprocessing = None if clip_preprocessing is None else int(clip_preprocessing)
        if self.clip_preprocessing is not None:
            th, tw, px = self.test.shape[1], self.test.shape[2], self.clip_preprocessing
            if th != tw:
                raise ValueError(f"clip_preprocessing needs square test images, not {th} x {tw}: Resize(n_px) of another shape is "
                                 "not n_px x n_px and CenterCrop would cut it")
            for what, side, chans in (("crop", self.crop, _set_channels(self.normal)), ("test images", th, self.test.shape[3])):
                if self._clip_px(side, chans) is not None and not (side <= px and side <= 64 and px <= 256):
                    raise NotImplementedError(f"clip_preprocessing={px} on {what} of {side} px: only upsampling from at most 64 px to "
                                              "at most 256 px is built")
        self.normalize = None
        self.ds_statistics = None
        self.normal_index = None if normal_index is None else torch.as_tensor(normal_index, dtype=torch.int64).clone()
        self._gcn = None
        if normalize is not None:
            self._resolve_normalize(normalize, ds_statistics)
        elif ds_statistics is not None:
            raise ValueError("ds_statistics needs the normalisation mode they belong to (normalize=...)")
        self._g = torch.Generator().manual_seed(seed)
        self._step = 0
        self.oe_subset = None

    def set_oe_subset(self, indices=None):
        """restrict outlier exposure to the listed rows of the resident OE set (None: the full set again): the OE half of every
        step batch is drawn only from them.  This is the reference's `oe_limit_samples` / the evolve experiment's
        `oe.train_set.indices = [...]` (`bases.py:196-201`, `evolve/__init__.py:71-77`): a `Subset` over the OE data.  As there,
        the list is tiled when it is shorter than the normal set (`bases.py:580-584`), the with-replacement rule looks at the
        length of the SUBSET (`bases.py:561`), and a batch reports for an OE sample its row in the FULL OE set (the wrapped
        dataset returns its own index, `cifar.py:106-121`: a `Subset` does not renumber) plus the length of the full normal set
        (`bases.py:596`).  Rows may repeat; order is kept."""
        if indices is None:
            self.oe_subset = None
            return
        idx = torch.as_tensor([int(i) for i in indices], dtype=torch.int64)
        if idx.numel() == 0:
            raise ValueError("an OE subset needs at least one row (None restores the full set)")
        if int(idx.min()) < 0 or int(idx.max()) >= len(self.oe):
            raise IndexError(f"OE subset names rows outside the resident OE set of {len(self.oe)} images")
        self.oe_subset = idx

    def _resolve_normalize(self, normalize, ds_statistics):
        """turn the transform string into numbers, once per task (`bases.py:293-372`).  Under data parallelism every rank does
        this on its own copy of the set: the fit works on exact integer sums, so all ranks get the same bits without a collective."""
        from . import normalize as _norm
        if self.mean is not None or self.std is not None:
            raise ValueError("normalize= fits the statistics itself; it cannot be combined with mean= / std=")
        mode = _norm.norm_mode(normalize)
        if ds_statistics is not None:
            stats = _norm.check_ds_statistics(ds_statistics, mode)
        elif isinstance(self.normal, RaggedImageSet):
            # the reference's fit: Resize -> CenterCrop(crop) of the normal training images (datasets/imagenet.py:89-93, 273-278)
            rows = self.normal_index if self.normal_index is not None else torch.arange(len(self.normal))
            stats = _norm.fit_statistics(self._center_crops(self.normal, rows), None, normalize)
        else:
            stats = _norm.fit_statistics(self.normal, self.normal_index, normalize)
        self.ds_statistics = stats
        if mode == _norm.STD_NORM:
            self.mean, self.std = list(stats["mean"]), list(stats["std"])
        else:
            self._gcn = _norm.GcnNormalize.from_statistics(stats, "l1")
            self.normalize = self._gcn

    def defer_normalize(self, on: bool = True):
        """leave Normalize out of the batches and report (mean, std) as `.normalize` for the encoder's fused normalise: the
        multi-scale modes filter in the [0, 1] pixel scale, before Normalize (training/ad_trainer.py:413-425)"""
        self._defer = bool(on)
        if self._gcn is not None:                        # GCN mode: batches are in the [0, 1] scale anyway, the operator stays
            return
        self.normalize = (self.mean, self.std) if on and self.mean is not None else None

    def _norm_args(self):
        return (None, None) if getattr(self, "_defer", False) else (self.mean, self.std)

    def pre_tensor_msms(self, msms):
        """claim the train sharpen MSMs: the source then applies them where the reference does, to the uint8 crop / flip output
        before ToTensor and the noise (`datasets/cifar.py:99-118`): per half, crop_flip_u8 -> sharpen_u8 -> augment_batch with
        identity params and the same seed (the noise depends only on seed, slot and element, so it is unchanged).  Returns the
        claimed MSMs, which the trainer then leaves out of the step batch's apply_msms; test batches (centre crops, no noise)
        stay with apply_msms."""
        self._pre_msms = [m for m in msms if m.transform_str == "sharpen" and m.ds_part_str in ("train_nominal", "train_oe")]
        if self._pre_msms and self.clip_preprocessing is not None and self._clip_px(self.crop, _set_channels(self.normal)) is not None:
            self._pre_msms = []
            raise NotImplementedError("a train sharpen MSM works on the uint8 crop in front of clip_preprocessing's upsample; that "
                                      "combination is not built")
        return list(self._pre_msms)

    def _clip_px(self, side, channels):
        """n_px where clip_preprocessing has work to do on square uint8 images of this side (train: the crop, test: the image) and
        channel count; None where the option is off or the stage is the identity: 3 channels, n_px wide already"""
        px = self.clip_preprocessing
        return None if px is None or (side == px and channels == 3) else px

    def _augment_half(self, src, p, nominal, mean, std, seed, jitter=None):
        """one half of a step batch: augment_batch, or with claimed sharpen MSMs for this half the reference's order.
        jitter: (factors, order) of a ragged half under color_jitter -- ColorJitter and the crop / flip are then one uint8 stage
        (`color_jitter_crop_u8`) in front of the sharpen MSMs and of augment_batch with identity params"""
        ops = [m for m in getattr(self, "_pre_msms", ()) if (m.ds_part_str == "train_nominal") == nominal]
        if self.clip_preprocessing is not None and self._clip_px(self.crop, _set_channels(src)) is not None:   # a sharpen MSM is refused together with it (pre_tensor_msms)
            return augment_resize_batch(src, p, self.crop, self.clip_preprocessing, mean, std, self.flip_first, self.noise_std, seed)
        if (not ops and jitter is None) or p.shape[0] == 0:
            return augment_batch(src, p, (self.crop, self.crop), mean, std, self.flip_first, self.noise_std, seed)
        from .msm import sharpen_percent, sharpen_u8
        if jitter is not None:
            u8 = color_jitter_crop_u8(src, p, (self.crop, self.crop), jitter[0], jitter[1], self.flip_first)
        else:
            u8 = crop_flip_u8(src, p, (self.crop, self.crop), self.flip_first)
        for m in ops:
            if m.magnitude is None:
                raise ValueError(f"MSM {m} has no magnitude set")
            u8 = sharpen_u8(u8, sharpen_percent(m.magnitude))
        ident = torch.zeros_like(p)
        ident[:, 0] = torch.arange(p.shape[0], dtype=torch.int32, device=p.device)
        return augment_batch(u8, ident, (self.crop, self.crop), mean, std, self.flip_first, self.noise_std, seed)

    def _params(self, idx, Hs, Ws):
        n = len(idx)
        top = torch.randint(-self.padding, Hs + self.padding - self.crop + 1, (n,), generator=self._g)
        left = torch.randint(-self.padding, Ws + self.padding - self.crop + 1, (n,), generator=self._g)
        # flip=False: no RandomHorizontalFlip in the chain, so no draw (the class docstring)
        flip = torch.randint(0, 2, (n,), generator=self._g) if self.flip else torch.zeros(n, dtype=torch.int64)
        return torch.stack([idx.to(torch.int64), top, left, flip], dim=1).to(torch.int32)

    def _params_ragged(self, idx, sizes):
        """_params for rows `idx` of a ragged set with the host table `sizes`: the origins of `ragged_crop_origins` (tops, then
        lefts), then the flips as the tensor path draws them"""
        idx = idx.to(torch.int64)
        tl = ragged_crop_origins(torch.from_numpy(sizes)[idx], self.crop, self.padding, self._g)
        flip = torch.randint(0, 2, (len(idx),), generator=self._g) if self.flip else torch.zeros(len(idx), dtype=torch.int64)
        return torch.stack([idx, tl[:, 0], tl[:, 1], flip], dim=1).to(torch.int32)

    def _draw(self, idx, src):
        if isinstance(src, RaggedImageSet):
            return self._params_ragged(idx, src.sizes)
        return self._params(idx, src.shape[1], src.shape[2])

    def _center_crops(self, src, rows):
        """uint8 [len(rows), crop, crop, C]: CenterCrop(crop) of the listed images of a ragged set"""
        rows = torch.as_tensor(rows, dtype=torch.int64)
        tl = torch.from_numpy(center_origins(src.sizes[rows.numpy()], self.crop))
        p = torch.stack([rows, tl[:, 0], tl[:, 1], torch.zeros_like(rows)], dim=1).to(torch.int32).to(src.device)
        return crop_flip_u8(src, p, (self.crop, self.crop), True)

    def _epoch(self, batch_size):
        subset = self.normal_index if self.normal_index is not None else torch.arange(len(self.normal))
        oe_rows = self.oe_subset if self.oe_subset is not None else torch.arange(len(self.oe))
        n, n_full, m = len(subset), len(self.normal), len(oe_rows)
        perm = subset[torch.randperm(n, generator=self._g)]
        oe_idx = tile_oe_indices(oe_rows, n)
        if m >= 10000:                                   # bases.py:561: OE sets of >= 10 000 samples are drawn with replacement
            oe_order = oe_idx[torch.randint(len(oe_idx), (len(oe_idx),), generator=self._g)]
        else:
            oe_order = oe_idx[torch.randperm(len(oe_idx), generator=self._g)]
        dev = self.normal.device
        for s in range(0, n, batch_size):
            ni = perm[s:s + batch_size]
            oi = oe_order[s:s + batch_size][:len(ni)]            # the OE half is cut to the normal half's size (bases.py:597)
            self._step += 1
            # two launches (normal half from its image set, OE half from the other), written into one batch tensor
            pn = self._draw(ni, self.normal).to(dev)
            po = self._draw(oi, self.oe).to(dev)
            seed = (self.seed * 65521 + self._step) % (1 << 23)
            src_n, src_o, jit_n, jit_o = self.normal, self.oe, None, None
            if self.color_jitter is not None:
                # ColorJitter comes first in the reference's chains (train_cifar.py:32, train_clip_imagenet.py:29): the gathered,
                # jittered uint8 images become the "set" the crop / flip kernel reads (slot i = image i)
                fn, on = sample_color_jitter(len(ni), *self.color_jitter, generator=self._g)
                fo, oo = sample_color_jitter(len(oi), *self.color_jitter, generator=self._g)
                # a ragged half keeps its set and its indices: the jitter runs under the crop window (_augment_half)
                if isinstance(self.normal, RaggedImageSet):
                    jit_n = (fn, on)
                else:
                    src_n = color_jitter_u8(self.normal, ni, fn, on)
                    pn[:, 0] = torch.arange(len(ni), dtype=torch.int32, device=dev)
                if isinstance(self.oe, RaggedImageSet):
                    jit_o = (fo, oo)
                else:
                    src_o = color_jitter_u8(self.oe, oi, fo, oo)
                    po[:, 0] = torch.arange(len(oi), dtype=torch.int32, device=dev)
            mean, std = self._norm_args()
            xn = self._augment_half(src_n, pn, True, mean, std, 2 * seed, jit_n)
            xo = self._augment_half(src_o, po, False, mean, std, 2 * seed + 1, jit_o)
            lbls = torch.cat([torch.full((len(ni),), self.nominal_label, dtype=torch.int64),
                              torch.full((len(oi),), self.anomalous_label, dtype=torch.int64)])
            yield torch.cat([xn, xo]), lbls, torch.cat([ni, oi + n_full])      # OE indices offset by the FULL normal set (bases.py:596)

    def loaders(self, batch_size, **kw):
        outer = self

        class _Train:
            def __iter__(s):
                return outer._epoch(batch_size)

            def __len__(s):
                n = len(outer.normal) if outer.normal_index is None else len(outer.normal_index)
                return math.ceil(n / batch_size)

        if self.clip_preprocessing is not None and self._clip_px(self.test.shape[1], self.test.shape[3]) is not None:
            # CLIP's transform on the raw test images (val_transform is empty, training/clip.py:44-46): the same kernel with an
            # identity "crop" of the whole image, no noise; 224 x 224 x 3 floats per image, so a batch exists only while it is used
            class _Test:
                def __iter__(s):
                    for lo in range(0, len(outer.test_y), batch_size):
                        yield outer._clip_test_batch(torch.arange(lo, min(lo + batch_size, len(outer.test_y))))

                def __len__(s):
                    return math.ceil(len(outer.test_y) / batch_size)

            return _Train(), _Test()
        # test split: centre crop, no flip, no noise (val_transform: ToTensor + normalize, train_cifar.py:39-42)
        return _Train(), [self._test_batch(idx) for idx in self._test_index_batches(batch_size)]

    def _test_index_batches(self, batch_size):
        return (torch.arange(s, min(s + batch_size, len(self.test_y))) for s in range(0, len(self.test_y), batch_size))

    def _test_batch(self, idx):
        """(images, labels, indices) of the listed test rows (without clip_preprocessing, or where its stage is the identity): CenterCrop(crop) of each image -- a ragged set:
        at its own origin (train_imagenet.py:38-41, `center_origins`)"""
        # under clip_preprocessing a test set that comes here is n_px x n_px x 3 -- given so, or made so from a ragged set at
        # construction: CLIP's transform alone is the identity on it, whatever the train crop is (val_transform is empty)
        side = self.crop if self.clip_preprocessing is None else self.clip_preprocessing
        if isinstance(self.test, RaggedImageSet):
            tl = torch.from_numpy(center_origins(self.test.sizes, side))
            p = torch.stack([idx, tl[idx, 0], tl[idx, 1], torch.zeros_like(idx)], dim=1).to(torch.int32).to(self.test.device)
        else:
            Hs, Ws = self.test.shape[1], self.test.shape[2]
            p = torch.stack([idx, torch.full_like(idx, (Hs - side) // 2), torch.full_like(idx, (Ws - side) // 2),
                             torch.zeros_like(idx)], dim=1).to(torch.int32).to(self.test.device)
        return augment_batch(self.test, p, (side, side), *self._norm_args(), True, 0.0, 0), self.test_y[idx], idx

    def _clip_test_batch(self, idx):
        """(images, labels, indices) of the listed test rows under an active clip_preprocessing stage: CLIP's transform of the whole
        image (an identity "crop"), no noise"""
        p = torch.zeros((len(idx), 4), dtype=torch.int32)
        p[:, 0] = idx
        x = augment_resize_batch(self.test, p.to(self.test.device), self.test.shape[1], self.clip_preprocessing, *self._norm_args(), True,
                                 0.0, 0)
        return x, self.test_y[idx], idx

    def test_images(self, rows):
        """the test loader's images of the listed test rows, in the listed order (repeats allowed): fp32 NCHW on the set's device, by
        the route `preview(train=False)` takes -- `_test_batch`, or the loader's output under an active clip_preprocessing stage.
        Deterministic: no random draw is consumed."""
        idx = torch.as_tensor(rows).to(torch.int64).cpu().reshape(-1)
        if len(idx) and (int(idx.min()) < 0 or int(idx.max()) >= len(self.test_y)):
            raise IndexError(f"test_images: rows outside the test set of {len(self.test_y)} images")
        if self.clip_preprocessing is not None and self._clip_px(self.test.shape[1], self.test.shape[3]) is not None:
            return self._clip_test_batch(idx)[0]
        return self._test_batch(idx)[0]

    def test_inputs(self, rows):
        """(images, labels, indices) as the test loader yields them for the listed dataset indices, in the listed order (repeats
        allowed), bit for bit: every row of a test batch is made from its own image alone, so a batch of chosen rows equals those rows
        of the loader's batches.  What `eoe_amd.explain` differentiates for the rows a ranking picked."""
        idx = torch.as_tensor(rows).to(torch.int64).cpu().reshape(-1)
        return self.test_images(idx), self.test_y[idx], idx

    def test_pictures(self, rows):
        """`test_images(rows)` without the Normalize, whether the batches carry it or not: fp32 NCHW in ToTensor's [0, 1] scale, the
        pictures `eoe_amd.explain.overlay` lays a map over (it reads fp32 pictures as 255 x).  A source in GCN mode hands out [0, 1]
        images anyway."""
        was = getattr(self, "_defer", False)
        self._defer = True                               # _norm_args() then leaves (mean, std) out; nothing else reads the flag
        try:
            return self.test_images(rows)
        finally:
            self._defer = was

    @property
    def n_normal(self) -> int:
        """the size of the normal training set (`normal_index`, or the whole resident normal set)"""
        return len(self.normal) if self.normal_index is None else len(self.normal_index)

    def normal_inputs(self, rows):
        """(images, indices) of the listed rows of the normal TRAINING set (positions in [0, n_normal), any order, repeats allowed)
        under the TEST transform -- the route `test_images` takes, applied to `self.normal`: the centre crop (a ragged set: at each
        image's own origin) or CLIP's transform of the whole image where the test split gets it, Normalize as the test batches carry
        it; no flip, no noise, no colour jitter, and no draw from any generator, so training after a call is bit for bit what it was.
        `indices` are the rows of the resident normal set (through `normal_index`: the labelled set's training rows).  What the
        nearest-neighbour search embeds as its reference set.  A ragged normal set under a clip_preprocessing stage that is not the
        identity has no counterpart on the test route (the test split is resized once at construction) and raises."""
        pos = torch.as_tensor(rows).to(torch.int64).cpu().reshape(-1)
        n = self.n_normal
        if len(pos) and (int(pos.min()) < 0 or int(pos.max()) >= n):
            raise IndexError(f"normal_inputs: rows outside the normal training set of {n} images")
        idx = pos if self.normal_index is None else self.normal_index[pos]
        src = self.normal
        px = self.clip_preprocessing
        if isinstance(src, RaggedImageSet):
            if px is not None:
                raise NotImplementedError("normal_inputs: the test route resizes a ragged test split to CLIP's n_px once, at "
                                          "construction; the ragged normal training set has no such copy, so its images under the "
                                          "test transform are not built")
            tl = torch.from_numpy(center_origins(src.sizes, self.crop))
            p = torch.stack([idx, tl[idx, 0], tl[idx, 1], torch.zeros_like(idx)], dim=1).to(torch.int32).to(src.device)
            return augment_batch(src, p, (self.crop, self.crop), *self._norm_args(), True, 0.0, 0), idx
        Hs, Ws = src.shape[1], src.shape[2]
        if px is not None and self._clip_px(Hs, src.shape[3]) is not None:
            if Hs != Ws:
                raise NotImplementedError(f"normal_inputs: CLIP's transform of a {Hs} x {Ws} normal set is not built (square images only)")
            p = torch.zeros((len(idx), 4), dtype=torch.int32)
            p[:, 0] = idx
            return augment_resize_batch(src, p.to(src.device), Hs, px, *self._norm_args(), True, 0.0, 0), idx
        side = self.crop if px is None else px
        p = torch.stack([idx, torch.full_like(idx, (Hs - side) // 2), torch.full_like(idx, (Ws - side) // 2), torch.zeros_like(idx)],
                        dim=1).to(torch.int32).to(src.device)
        return augment_batch(src, p, (side, side), *self._norm_args(), True, 0.0, 0), idx

    def normal_pictures(self, rows):
        """`normal_inputs(rows)[0]` without the Normalize: fp32 NCHW in ToTensor's [0, 1] scale (as `test_pictures`)"""
        was = getattr(self, "_defer", False)
        self._defer = True
        try:
            return self.normal_inputs(rows)[0]
        finally:
            self._defer = was

    PREVIEW_SEED = 0x9E3779B1

    def preview(self, percls=40, train=True):
        """`TorchvisionDataset.preview` (`bases.py:246-291`): (fp32 NCHW tensor, {label: count}) = the first `percls` images per label
        of the loader's output taken in batches of 10, label 0 first, cut to the rarest label's number, and how many samples of each
        label the split holds (`n_normal_anomalous`: the row headers of the preview figure).  Train batches are drawn from a PRIVATE
        generator (seeded from the source's seed) with the step counter put back afterwards: asking for a preview leaves the
        source's own random state, and so every later batch, unchanged.  Test batches are built only as far as needed."""
        if train:
            n_normal = len(self.normal) if self.normal_index is None else len(self.normal_index)
            counts = {self.nominal_label: n_normal, self.anomalous_label: len(self.oe) if self.oe_subset is None else len(self.oe_subset)}
        else:
            labels, numbers = torch.unique(self.test_y, return_counts=True)
            counts = {int(k): int(v) for k, v in zip(labels.tolist(), numbers.tolist())}
        kept = self._g, self._step
        self._g = torch.Generator().manual_seed((self.seed + self.PREVIEW_SEED) % (1 << 63))
        try:
            if train:
                batches = self._epoch(10)
            elif self.clip_preprocessing is not None and self._clip_px(self.test.shape[1], self.test.shape[3]) is not None:
                batches = iter(self.loaders(10)[1])
            else:
                batches = (self._test_batch(idx) for idx in self._test_index_batches(10))
            xs, ys = [], []
            for xb, yb, _ in batches:
                xs.append(xb)
                ys.append(yb)
                y = torch.cat(ys)
                if all(int((y == c).sum()) >= percls for c in counts):
                    break
        finally:
            self._g, self._step = kept
        x, y = torch.cat(xs), torch.cat(ys).to(xs[0].device)
        out = [x[y == c][:percls] for c in sorted(set(y.tolist()))]
        percls = min(o.shape[0] for o in out)
        return torch.cat([o[:percls] for o in out]), counts


def normal_subset(class_labels, normal_classes) -> torch.Tensor:
    """rows of a labelled set that belong to the normal classes, ascending: `TorchvisionDataset.create_subset`
    (`datasets/bases.py:192-195`: np.argwhere(np.isin(labels, normal_classes)))"""
    lab = torch.as_tensor(class_labels, dtype=torch.int64)
    keep = torch.zeros(len(lab), dtype=torch.bool)
    for c in normal_classes:
        keep |= lab == int(c)
    return torch.nonzero(keep).flatten()


def ad_targets(class_labels, normal_classes, nominal_label: int = 0) -> torch.Tensor:
    """the reference's `target_transform` (`datasets/bases.py:137-139`): anomalous iff the sample's class is not a normal class"""
    lab = torch.as_tensor(class_labels, dtype=torch.int64)
    normal = torch.zeros(len(lab), dtype=torch.bool)
    for c in normal_classes:
        normal |= lab == int(c)
    return torch.where(normal, torch.tensor(nominal_label), torch.tensor(1 - nominal_label)).to(torch.int64)


class LabelledImageSet:
    """A multi-class image set resident in HBM (uint8 NHWC + integer class labels) from which the class x seed loop of
    `ADTrainer.run` draws one anomaly-detection task per call, as the reference's `load_dataset(dsstr, datapath,
    self.get_nominal_classes(c), 0, ...)` does (`training/ad_trainer.py:248-253`, `datasets/__init__.py:237-340`):
      * normal training samples = the training rows whose class is one of `normal_classes` (`bases.py:169-203`);
      * the test split is the WHOLE test set, labelled nominal (0) for the normal classes and anomalous (1) for the rest
        (`bases.py:130-139`) -- under `leave_one_out` the anomalies are the one held-out class, under `one_vs_rest` all others;
      * outlier exposure comes from a separate image set (`oe_u8`), every sample labelled anomalous (`datasets/__init__.py:300`).
    The images are uploaded once; a task is an index list over them (`ResidentImageSource(normal_index=...)`), so iterating 30
    classes x 2 seeds does not copy the set 60 times."""

    def __init__(self, train_u8, train_classes, test_u8, test_classes, oe_u8, classes, crop, device="cuda", normalize=None,
                 grayscale=False, **source_kw):
        """normalize: one of the reference's transform strings ('normalize', 'gcn-normalize', ...): every task then gets the
        statistics of ITS normal classes (`bases.py:293-372`), fitted once per class set and kept (the reference keeps them in
        `stats_cache.json`, `bases.py:374-410`): thirty classes x two seeds fit thirty times.
        grayscale: the 1-channel chain of `ResidentImageSource(grayscale=True)`; colour sets are converted here, once for all
        tasks.  `flip=False` and the other options of the source go through `source_kw`."""
        dev = torch.device(device)
        if grayscale and any(isinstance(t, RaggedImageSet) for t in (train_u8, test_u8, oe_u8)):
            raise NotImplementedError("grayscale=True on a RaggedImageSet is not built: convert the images to one channel before "
                                      "packing them (a 1-channel RaggedImageSet is accepted)")
        if grayscale:
            if source_kw.get("color_jitter") is not None:
                raise ValueError("color_jitter works on RGB images and cannot be combined with grayscale=True")
            self.train, self.test, self.oe = (gray_set(t, dev) for t in (train_u8, test_u8, oe_u8))
            source_kw = dict(source_kw, grayscale=True)
        else:
            px, rsz = source_kw.get("clip_preprocessing"), source_kw.get("resize")
            for what, t in (("normal", train_u8), ("OE", oe_u8)):             # the source's refusal, in front of the device work below
                if px is not None and isinstance(t, RaggedImageSet) and (rsz is None or isinstance(rsz, int)) and isinstance(crop, int):
                    _check_clip_ragged_half(what, t, crop, int(px))
            if px is not None and isinstance(test_u8, RaggedImageSet):
                # CLIP's transform on the raw test images is the same for every task: once, here, not once per class and seed
                _check_clip_ragged_test(test_u8, source_kw.get("test_resize"), dev)
                test_u8 = clip_preprocess_ragged(_resident(test_u8, dev), int(px))
            self.train, self.test, self.oe = (_resident(t, dev) for t in (train_u8, test_u8, oe_u8))
        self.train_classes =torch.as_tensor(train_classes, dtype=torch.int64).clone()
        self.test_classes = torch.as_tensor(test_classes, dtype=torch.int64).clone()
        self.classes = list(classes)
        self.crop, self.source_kw, self.device = crop, dict(source_kw), dev
        self.normalize, self._stats = normalize, {}

    def no_classes(self) -> int:
        return len(self.classes)

    def source(self, normal_classes, seed: int = 0, ds_statistics=None, oe_subset=None) -> ResidentImageSource:
        """ds_statistics: the dict of a snapshot to score with (wins over fitting, and is not kept for later tasks); it is used
        only by a set built with `normalize=`: one built with ready `mean=` / `std=` keeps those, whatever a snapshot carries.
        oe_subset: rows of the OE set to restrict outlier exposure to (`ResidentImageSource.set_oe_subset`)"""
        key = tuple(sorted(int(c) for c in normal_classes))
        given = ds_statistics if ds_statistics is not None else self._stats.get(key)
        kw = dict(self.source_kw)
        if self.normalize is not None:
            kw.update(normalize=self.normalize, ds_statistics=given)
        # without a mode the set was built with ready mean= / std= (or none): a snapshot's statistics are not looked at, as before
        src = ResidentImageSource(self.train, self.oe, self.test, ad_targets(self.test_classes, normal_classes), self.crop,
                                  seed=seed, device=self.device, normal_index=normal_subset(self.train_classes, normal_classes),
                                  **kw)
        if self.normalize is not None and ds_statistics is None:
            self._stats.setdefault(key, src.ds_statistics)
        src.normal_classes = tuple(int(c) for c in normal_classes)
        src.test_classes = self.test_classes          # what ad_targets collapsed to 0 / 1 (metrics.class_breakdown)
        if oe_subset is not None:
            src.set_oe_subset(oe_subset)
        return src
