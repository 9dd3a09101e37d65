"""Image grids from the device: the pictures of the reference's `Logger.logimg` (`utils/logger.py:202-295`) -- the trainer's
`training_cls…_preview` / `eval_cls…_preview` and every figure of the evolve experiment -- composed where the images lie.

The reference pulls each image through the host dataset, stacks float tensors, `F.interpolate`s them when a side exceeds `maxres`,
normalises every image to its own [min, max] (`make_grid(normalize=True, scale_each=True)`, or its own rule under `mark`), tiles
them with `make_grid` and multiplies by 255 on the host.  Here the images are in HBM already -- an fp32 NCHW batch of the loaders, the
uint8 NHWC OE pool, or a `RaggedImageSet` arena with its `CenterCrop` windows -- and `image_grid` is one launch pair of
`csrc/grid.hip` (per-cell min / max, then gather + resize + normalise + tile + frame + separator) that writes the finished uint8
picture; the host copies it back once and encodes the PNG (`JsonLogger.logimg`).

A CPU source takes the numpy path of this file, which yields the same bytes (the same fp32 operations in the same order).

What differs from the reference, deliberately:
  * Frame colours under `mark`: the reference stores 0...255 colour values into a [0, 1] tensor, multiplies by 255 and lets
    `astype(ubyte)` of up to 65 025.0 decide, which numpy leaves undefined.  Here the frame byte IS the colour value.
  * A constant image (`hi == lo`) under `mark` is 0 / 0 in the reference; here it is all 0.
  * A single image is padded and placed like any other (`Hg = h + 2 pad`); torchvision's `make_grid` returns a lone image bare.
  * Text is not drawn (no OpenCV): `rowheaders` go to a side file and no black header column is added (`JsonLogger.logimg`).
"""
from typing import Optional, Sequence

import numpy as np
import torch

# utils/logger.py:29-33; entry j of `mark` takes COLORS[j % 17]
COLORS = [(224, 28, 28), (28, 224, 224), (28, 28, 224), (164, 96, 96), (96, 164, 96), (96, 96, 164), (128, 64, 32), (128, 32, 128),
          (32, 128, 128), (164, 164, 32), (255, 124, 32), (255, 124, 32), (124, 255, 32), (164, 64, 255), (164, 196, 124),
          (196, 124, 164), (124, 164, 196)]
INDEX_LIMIT = 1 << 31


def grid_geometry(per: int, h: int, w: int, nrow: int = 8, pad: int = 2, maxres: int = 128, row_sep_at=(None, None)) -> dict:
    """the layout of one picture of `per` cells cut from h x w images: cell size (ch, cw), xmaps, ymaps, Hg, Wg and the separator
    (sep_height rows in front of row sep_pos; the picture then has rows = Hg + sep_height rows)"""
    if nrow < 1:
        raise ValueError(f"image_grid: nrow must be at least 1, not {nrow}")
    if pad < 0 or maxres < 1 or h < 1 or w < 1:
        raise ValueError(f"image_grid: pad >= 0, maxres >= 1 and non-empty images are needed, not pad={pad}, maxres={maxres}, {h} x {w}")
    ch, cw = (maxres, maxres) if (h > maxres or w > maxres) else (h, w)
    xmaps = max(min(nrow, per), 1)
    ymaps = -(-per // xmaps)
    Hg, Wg = (ch + pad) * ymaps + pad, (cw + pad) * xmaps + pad
    sep_height = sep_at = 0
    if row_sep_at is not None and len(row_sep_at) == 2 and row_sep_at[0] is not None:
        sep_height, sep_at = int(row_sep_at[0]), int(row_sep_at[1])
        if sep_height < 0 or sep_at < 0:
            raise ValueError(f"image_grid: row_sep_at must be (height >= 0, at >= 0), not {tuple(row_sep_at)}")
    return {"ch": ch, "cw": cw, "xmaps": xmaps, "ymaps": ymaps, "Hg": Hg, "Wg": Wg, "sep_height": sep_height, "sep_at": sep_at,
            "sep_pos": min((ch + pad) * sep_at + pad // 2, Hg), "rows": Hg + sep_height}


def mark_colors(mark, n: int) -> np.ndarray:
    """int32 [n]: the frame colour 0xRRGGBB of every cell, -1 where there is none.  `mark[j]` -- an int or a list of cells -- takes
    COLORS[j % 17], as `zip(mark, cycle(COLORS))` pairs them (`logger.py:240-245`); a later entry paints over an earlier one"""
    out = np.full(n, -1, dtype=np.int32)
    for j, m in enumerate(mark):
        r, g, b = COLORS[j % len(COLORS)]
        for cell in ([m] if isinstance(m, (int, np.integer)) else m):
            cell = int(cell)
            if not -n <= cell < n:
                raise IndexError(f"image_grid: mark names cell {cell} of {n}")
            out[cell % n] = (r << 16) | (g << 8) | b
    return out


class _Cells:
    """where the cells of a call lie: the source form, its tensors and the table (row, top, left) of the listed cells"""

    def __init__(self, src, rows, crop):
        from .data import RaggedImageSet
        from .evolve import OEPool
        self.pool = None
        if isinstance(src, OEPool):
            if crop is not None:
                raise ValueError("image_grid: an OEPool brings its own crop")
            ids = np.arange(len(src)) if rows is None else np.asarray(rows, dtype=np.int64)
            rows, self.pool = src.rows(ids).reshape(ids.shape), src
            src = src.images
        elif isinstance(src, RaggedImageSet):
            if crop is None:
                raise ValueError("image_grid: a RaggedImageSet needs crop= (the CenterCrop(crop) windows are shown)")
            self.pool = OEPool(src, None, crop)
        elif crop is not None:
            raise ValueError("image_grid: crop= selects the windows of a RaggedImageSet; a tensor is shown whole")
        if isinstance(src, RaggedImageSet):
            self.form, self.C, (self.h, self.w), self.n_src = "ragged", src.channels, self.pool.crop, len(src)
            self.device = src.device
        elif isinstance(src, torch.Tensor):
            if src.dtype == torch.float32 and src.dim() == 4:
                self.form, (self.n_src, self.C, self.h, self.w) = "f32", src.shape
            elif src.dtype == torch.uint8 and src.dim() in (3, 4):
                src = src.unsqueeze(-1) if src.dim() == 3 else src
                self.form, (self.n_src, self.h, self.w, self.C) = "u8", src.shape
            else:
                raise ValueError(f"image_grid: an fp32 NCHW or a uint8 NHWC tensor is needed, not {src.dtype} {list(src.shape)}")
            src, self.device = src.contiguous(), src.device
        else:
            raise TypeError(f"image_grid: a tensor, a RaggedImageSet or an OEPool is needed, not {type(src).__name__}")
        if self.C not in (1, 3):
            raise ValueError(f"image_grid: c (channels) must be 1 or 3, not {self.C}")
        self.src = src
        rows = np.arange(self.n_src, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
        self.shape, rows = rows.shape, rows.reshape(-1)
        if len(rows) and (rows.min() < 0 or rows.max() >= self.n_src):
            raise IndexError(f"image_grid: rows outside the set of {self.n_src} images")
        self.table = np.zeros((len(rows), 4), dtype=np.int32)
        self.table[:, 0] = rows
        if self.form == "ragged":
            self.table[:, 1:3] = self.pool._origins[rows]

    def host(self) -> np.ndarray:
        """fp32 [n, C, h, w]: the cells of a CPU source, uint8 forms in ToTensor's scale"""
        rows = self.table[:, 0]
        if self.form == "f32":
            return self.src.numpy()[rows]
        u8 = self.pool._windows_host(rows) if self.form == "ragged" else self.src.numpy()[rows]
        return np.ascontiguousarray(u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


def _taps(n_in: int, n_out: int):
    """torch's bilinear source indices and weights of one axis (align_corners=False): fp32, as `csrc/grid.hip` computes them"""
    one, half = np.float32(1.0), np.float32(0.5)
    f = (np.float32(n_in) / np.float32(n_out)) * (np.arange(n_out, dtype=np.float32) + half) - half
    f = np.maximum(f, np.float32(0.0))
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(f - i0.astype(np.float32), np.float32(0.0), one)
    return i0, i1, one - l1, l1


def _compose_host(x: np.ndarray, groups: int, geo: dict, pad: int, colors: Optional[np.ndarray]) -> np.ndarray:
    """the numpy statement of `csrc/grid.hip`: uint8 [groups, rows, Wg, 3] of the cells x (fp32 [n, C, h, w])"""
    n, C, h, w = x.shape
    ch, cw, per = geo["ch"], geo["cw"], n // groups
    if (ch, cw) != (h, w):
        y0, y1, ly0, ly1 = _taps(h, ch)
        x0, x1, lx0, lx1 = _taps(w, cw)
        top, bot = x[:, :, y0], x[:, :, y1]
        ly0, ly1 = ly0[:, None], ly1[:, None]
        x = ly0 * (lx0 * top[..., x0] + lx1 * top[..., x1]) + ly1 * (lx0 * bot[..., x0] + lx1 * bot[..., x1])
    assert x.dtype == np.float32
    lo, hi = x.min(axis=(1, 2, 3), keepdims=True), x.max(axis=(1, 2, 3), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        if colors is None:
            v = (np.clip(x, lo, hi) - lo) / np.maximum(hi - lo, np.float32(1e-5))
        else:
            v = np.where(hi - lo > 0, (x - lo) / (hi - lo), np.float32(0.0))
    cells = (v * np.float32(255.0)).astype(np.int32).astype(np.uint8).transpose(0, 2, 3, 1)
    cells = np.repeat(cells, 3, axis=3) if C == 1 else np.ascontiguousarray(cells)
    if colors is not None:
        for k in np.nonzero(colors >= 0)[0]:
            rgb = [(int(colors[k]) >> s) & 255 for s in (16, 8, 0)]
            cells[k, 0], cells[k, -1], cells[k, :, 0], cells[k, :, -1] = rgb, rgb, rgb, rgb
    pic = np.zeros((groups, geo["Hg"], geo["Wg"], 3), dtype=np.uint8)
    for k in range(n):
        g, (r, c) = k // per, divmod(k % per, geo["xmaps"])
        y, xx = pad + r * (ch + pad), pad + c * (cw + pad)
        pic[g, y:y + ch, xx:xx + cw] = cells[k]
    if geo["sep_height"] > 0:
        sep = np.zeros((groups, geo["sep_height"], geo["Wg"], 3), dtype=np.uint8)
        pic = np.concatenate([pic[:, :geo["sep_pos"]], sep, pic[:, geo["sep_pos"]:]], axis=1)
    return pic


def image_grids(src, rows=None, *, crop=None, nrow: int = 8, pad: int = 2, maxres: int = 128, mark=None,
                row_sep_at=(None, None)) -> torch.Tensor:
    """`image_grid` for several pictures of equally many cells at once: `rows` is [k, per] (for an OEPool: ids) and the result uint8
    [k, rows, Wg, 3] in one buffer, from ONE launch pair.  `mark` numbers the cells over all pictures (cell j of picture g is
    g * per + j)"""
    cells = _Cells(src, rows, crop)
    if len(cells.shape) != 2:
        raise ValueError(f"image_grids: rows must be [pictures, cells per picture], not {list(cells.shape)}")
    groups, per = cells.shape
    return _grids(cells, groups, per, nrow, pad, maxres, mark, row_sep_at)


def image_grid(src, rows=None, *, crop=None, nrow: int = 8, pad: int = 2, maxres: int = 128, mark=None,
               row_sep_at=(None, None)) -> torch.Tensor:
    """the picture `logger.logimg` hands to `cv2.imwrite` (before any text header): uint8 [Hg, Wg, 3] on `src`'s device.

    src   an fp32 NCHW tensor [n, c, h, w], c in {1, 3} (what the loaders yield), shown as it is;
          a uint8 NHWC tensor [N, H, W, C] (the uniform OE pool): the value is u8 / 255, as ToTensor;
          a `RaggedImageSet` with `crop=` (an int or (h, w)): each image's CenterCrop(crop) window, zero where it leaves the image
          (`data.center_origins`; the windows `OEPool.distances` compares);
          an `OEPool`: its set, `valid_indices` and crop; `rows` are then ids (`pool.rows`).
    rows  the images to show, in order, repeats allowed (None: all).
    Cells of h x w, or `maxres` x `maxres` when h or w exceeds it (torch's `F.interpolate(mode='bilinear')`: align_corners=False, no
    antialias).  xmaps = min(nrow, n), ymaps = ceil(n / xmaps), Hg = (h + pad) * ymaps + pad, Wg = (w + pad) * xmaps + pad; cell k at
    (pad + (k // xmaps) * (h + pad), pad + (k % xmaps) * (w + pad)); padding and unused cells are 0; one channel fills all three.
    `row_sep_at = (height, at)` inserts `height` black rows at y = (h + pad) * at + pad // 2 (`logger.py:276-282`).
    Without `mark`: `make_grid(normalize=True, scale_each=True)`: per image over the cell values after the resize,
    v = (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5), byte = trunc(v * 255).  With `mark` (`logger.py:234-246`):
    v = (x - lo) / (hi - lo) and the outermost 1-pixel frame of every marked cell takes a colour: entry j of `mark`, an int or a
    list of cells, takes COLORS[j % 17].  n = 0 gives an empty picture [0, 0, 3].  The module docstring lists what differs from the
    reference."""
    cells = _Cells(src, rows, crop)
    if len(cells.shape) != 1:
        raise ValueError(f"image_grid: rows must be a flat list, not {list(cells.shape)} (image_grids takes [pictures, cells])")
    n = cells.shape[0]
    if n == 0:
        grid_geometry(0, cells.h, cells.w, nrow, pad, maxres, row_sep_at)      # the refusals hold for the empty case too
        return torch.empty((0, 0, 3), dtype=torch.uint8, device=cells.device)
    return _grids(cells, 1, n, nrow, pad, maxres, mark, row_sep_at)[0]


def _grids(cells: _Cells, groups: int, per: int, nrow, pad, maxres, mark, row_sep_at) -> torch.Tensor:
    nrow, pad, maxres, n = int(nrow), int(pad), int(maxres), groups * per
    geo = grid_geometry(per, cells.h, cells.w, nrow, pad, maxres, row_sep_at)
    if n * cells.C * geo["ch"] * geo["cw"] >= INDEX_LIMIT or groups * geo["rows"] * geo["Wg"] * 3 >= INDEX_LIMIT:
        raise ValueError(f"image_grid: n = {n} cells of {cells.C} x {geo['ch']} x {geo['cw']} exceed 32-bit indexing")
    colors = None if mark is None else mark_colors(mark, n)
    if cells.device.type != "cuda":
        return torch.from_numpy(_compose_host(cells.host(), groups, geo, pad, colors))
    from ._lib import check, lib
    dev, src = cells.device, cells.src
    cells.table[:, 3] = -1 if colors is None else colors
    out = torch.empty((groups, geo["rows"], geo["Wg"], 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        table = torch.from_numpy(cells.table).to(dev)
        minmax = torch.empty(2 * n, dtype=torch.float32, device=dev)
        tail = (table.data_ptr(), n, groups, nrow, pad, maxres, geo["sep_height"], geo["sep_at"], int(colors is not None),
                minmax.data_ptr(), out.data_ptr(), out.numel(), torch.cuda.current_stream(dev).cuda_stream)
        if cells.form == "f32":
            check(lib.eoe_grid_f32(src.data_ptr(), cells.n_src, cells.C, cells.h, cells.w, *tail), "eoe_grid_f32")
        elif cells.form == "u8":
            check(lib.eoe_grid_u8(src.data_ptr(), cells.n_src, cells.h, cells.w, cells.C, *tail), "eoe_grid_u8")
        else:
            check(lib.eoe_grid_ragged_u8(src.arena.data_ptr(), src.arena.numel(), src.offsets.data_ptr(), src.sizes_dev.data_ptr(),
                                         cells.n_src, cells.C, cells.h, cells.w, *tail), "eoe_grid_ragged_u8")
    return out


_PILLOW_WARNED = False


def save_png(path: str, img: np.ndarray) -> bool:
    """writes the uint8 [H, W, 3] picture with Pillow; without Pillow warns once and writes nothing"""
    global _PILLOW_WARNED
    try:
        from PIL import Image
    except ImportError:
        if not _PILLOW_WARNED:
            import warnings
            warnings.warn("Pillow is not installed: logimg returns its pictures but writes no PNG files")
            _PILLOW_WARNED = True
        return False
    Image.fromarray(np.ascontiguousarray(img)).save(path, format="PNG")
    return True


def host_rows(src, rows: Sequence[int]) -> torch.Tensor:
    """what the reference's way copies back: the listed rows of a device uint8 set as ToTensor makes them, fp32 NCHW on the host
    (tools/grid_bench.py times image_grid of this against image_grid on the device)"""
    u8 = src[torch.as_tensor(np.asarray(rows, dtype=np.int64), device=src.device)].cpu()
    return torch.from_numpy(np.ascontiguousarray(u8.numpy().transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
