"""Generates tests/golden/g26_grid.npz: the pictures the reference's `Logger.logimg` (`utils/logger.py:202-295`) hands to `cv2.imwrite`,
on stored inputs.  Run by hand where the reference is available; the tests only read the .npz.

    python tests/golden/make_golden_grid.py <the reference's src/eoe directory>

`logger.py` is executed by file path, nothing re-typed.  What it imports and is not installed is stubbed in `sys.modules`: `cv2`
(`imwrite` captures the array, `cvtColor` and `putText` return their input), tensorboard, tqdm and matplotlib (blank), and
`torchvision.utils.make_grid` by `make_grid` below, a plain torch statement of torchvision's documented rule (single-channel images
repeated to three, per-image `norm_range` with `scale_each`, `xmaps = min(nrow, n)`, cells `padding` apart on `pad_value`) -- without
its shortcut that returns a lone image unpadded.  Inputs and the captured pictures only are stored.

Cases (`names`; per case `<name>/params` (JSON: nrow, pad, maxres, mark, row_sep_at, rows, input), `<name>/ref` and for a marked
case `<name>/frame_mask` (bool [H, W]: the frame pixels of the marked cells) and `<name>/frame_rgb` (uint8 [H, W, 3]: the colour
each must have, COLORS[j % 17] of `mark[j]`); inputs under `in/<input>`: fp32 NCHW, or uint8 NHWC fed to the reference as u8 / 255):
  n{1,5,16,17}_nrow{16,4}   3 x 9 x 7 floats with negative values: the partial last row and the xmaps = n < nrow edge
  pad0, pad3                n = 5, nrow = 4
  sep_pad0 sep_pad3 sep2    row_sep_at (16, 1) at pad 0 and 3 (pad // 2 in the position), (16, 2) at n = 17, nrow = 4
  gray                      3 images 1 x 28 x 28
  const                     n = 5 with one constant image, no mark: the 1e-5 branch
  u8_rows                   6 uint8 images 32 x 32 x 3 through the row list [5, 4, 3, 3, 2, 1, 0]
  mark_flat mark_nested mark18 mark_sep   mark=[0, 1, 4]; [[0, 3]]; 18 marks on 17 cells (the 18th wraps to colour 0 and repaints
                            cell 5); [[0, 3], 7] with row_sep_at (16, 1) on 12 uint8 cells, nrow = 6.  No constant image.
  resize224 resize130       4 uint8 images 224 x 224 x 3 (cell 128 x 128, scale 1.75); 2 of 130 x 100 x 3 (one side exceeds maxres)
  strips, second_pass       3 strips of 4 cells of the uint8 set (nrow = 16); the strips as uint8 cells, maxres = 1024, nrow = 1
"""
import importlib
import importlib.util
import json
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
CAPTURED = []


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0):
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if normalize:
        tensor = tensor.clone()
        assert scale_each and value_range is None
        for img in tensor:
            low, high = float(img.min()), float(img.max())
            img.clamp_(min=low, max=high)
            img.sub_(low).div_(max(high - low, 1e-5))
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    if "." in name:
        parent, child = name.rsplit(".", 1)
        if parent in sys.modules:
            setattr(sys.modules[parent], child, m)
    return m


def load_logger(ref: str):
    blank = lambda n: type(n, (), {})      # noqa: E731
    _stub("cv2", imwrite=lambda file, img: CAPTURED.append(np.array(img)), cvtColor=lambda img, code: img,
          putText=lambda img, *a, **k: img, COLOR_RGB2BGR=4, FONT_HERSHEY_SIMPLEX=0)
    _stub("torchvision")
    _stub("torchvision.utils", make_grid=make_grid)
    _stub("torchvision.transforms", Compose=blank("Compose"))
    for name, attrs in {"torch.utils.tensorboard": {"SummaryWriter": blank("SummaryWriter")}, "tqdm": {"tqdm": blank("tqdm")},
                        "matplotlib": {"use": lambda *a, **k: None}, "matplotlib.pyplot": {}}.items():
        try:
            importlib.import_module(name)
        except Exception:
            _stub(name, **attrs)
    spec = importlib.util.spec_from_file_location("eoe_ref_logger", os.path.join(ref, "utils", "logger.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def inputs():
    rng = np.random.default_rng(26)
    x = {f"f{n}": (rng.standard_normal((n, 3, 9, 7)) * 1.5 - 0.25).astype(np.float32) for n in (1, 5, 16, 17)}
    x["gray"] = rng.standard_normal((3, 1, 28, 28)).astype(np.float32)
    const = x["f5"].copy()
    const[2] = np.float32(0.375)
    x["const"] = const
    x["u8"] = rng.integers(0, 256, (6, 32, 32, 3), dtype=np.uint8)

    def blocky(n, h, w, b):
        """random levels in b x b blocks: every 1.75-wide (1.02-wide) step of the resize crosses block borders, and the stored input
        stays small"""
        return rng.integers(0, 256, (n, -(-h // b), -(-w // b), 3), dtype=np.uint8).repeat(b, axis=1).repeat(b, axis=2)[:, :h, :w].copy()

    x["u8_224"], x["u8_130"] = blocky(4, 224, 224, 4), blocky(2, 130, 100, 2)
    return x


def cases():
    c = {}
    for n in (1, 5, 16, 17):
        for nrow in (16, 4):
            c[f"n{n}_nrow{nrow}"] = dict(input=f"f{n}", nrow=nrow)
    c["pad0"] = dict(input="f5", nrow=4, pad=0)
    c["pad3"] = dict(input="f5", nrow=4, pad=3)
    c["sep_pad0"] = dict(input="f5", nrow=4, pad=0, row_sep_at=[16, 1])
    c["sep_pad3"] = dict(input="f5", nrow=4, pad=3, row_sep_at=[16, 1])
    c["sep2"] = dict(input="f17", nrow=4, row_sep_at=[16, 2])
    c["gray"] = dict(input="gray", nrow=8)
    c["const"] = dict(input="const", nrow=4)
    c["u8_rows"] = dict(input="u8", rows=[5, 4, 3, 3, 2, 1, 0], nrow=4)
    c["mark_flat"] = dict(input="f5", nrow=4, mark=[0, 1, 4])
    c["mark_nested"] = dict(input="f5", nrow=4, mark=[[0, 3]])
    c["mark18"] = dict(input="f17", nrow=16, mark=list(range(17)) + [5])
    c["mark_sep"] = dict(input="u8", rows=[0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0], nrow=6, mark=[[0, 3], 7], row_sep_at=[16, 1])
    c["resize224"] = dict(input="u8_224", nrow=8)
    c["resize130"] = dict(input="u8_130", nrow=8)
    return c


def frames(colors, p, n, h, w):
    """where the marked cells' frames lie and which colour each has, by the layout rule of the issue"""
    nrow, pad, mark = p["nrow"], p["pad"], p["mark"]
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    rgb = np.zeros(((h + pad) * ymaps + pad, (w + pad) * xmaps + pad, 3), np.uint8)
    mask = np.zeros(rgb.shape[:2], bool)
    for j, m in enumerate(mark):
        for k in ([m] if isinstance(m, int) else m):
            y, x = pad + (k // xmaps) * (h + pad), pad + (k % xmaps) * (w + pad)
            cell = np.zeros((h, w), bool)
            cell[0] = cell[-1] = cell[:, 0] = cell[:, -1] = True
            mask[y:y + h, x:x + w] |= cell
            rgb[y:y + h, x:x + w][cell] = colors[j % len(colors)]
    sep = p["row_sep_at"]
    if sep[0] is not None:
        pos = (h + pad) * sep[1] + pad // 2
        mask = np.concatenate([mask[:pos], np.zeros((sep[0], mask.shape[1]), bool), mask[pos:]])
        rgb = np.concatenate([rgb[:pos], np.zeros((sep[0],) + rgb.shape[1:], np.uint8), rgb[pos:]])
    return mask, rgb


def main():
    ref = load_logger(sys.argv[1])
    logger = object.__new__(ref.Logger)
    logger.dir = tempfile.mkdtemp()
    logger._Logger__active = True
    x, out, names = inputs(), {}, []

    def run(name, tensor, p):
        p = dict(dict(nrow=8, pad=2, maxres=128, mark=None, row_sep_at=[None, None], rows=None), **p)
        del CAPTURED[:]
        with np.errstate(invalid="ignore"):
            img = logger.logimg(name, tensor, nrow=p["nrow"], pad=p["pad"], maxres=p["maxres"], mark=p["mark"],
                                row_sep_at=tuple(p["row_sep_at"]))
        assert len(CAPTURED) == 1 and np.array_equal(CAPTURED[0], img) and img.dtype == np.uint8
        out[f"{name}/params"], out[f"{name}/ref"] = np.array(json.dumps(p)), CAPTURED[0]
        if p["mark"] is not None:
            h, w = (min(s, p["maxres"]) for s in tensor.shape[2:])
            out[f"{name}/frame_mask"], out[f"{name}/frame_rgb"] = frames(ref.COLORS, p, tensor.shape[0], h, w)
            assert out[f"{name}/frame_mask"].shape == img.shape[:2]
        names.append(name)
        print(name, img.shape)
        return img

    def tensor_of(p):
        a = x[p["input"]]
        if a.dtype == np.uint8:
            a = a[p["rows"]] if p.get("rows") is not None else a
            a = np.ascontiguousarray(a.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)       # ToTensor
        return torch.from_numpy(a)

    for name, p in cases().items():
        run(name, tensor_of(p), p)
    strip_rows = [[0, 1, 2, 3], [5, 5, 4, 0], [2, 4, 1, 3]]
    strips = np.stack([run(f"strip{i}", tensor_of(dict(input="u8", rows=r)), dict(input="u8", rows=r, nrow=16))
                       for i, r in enumerate(strip_rows)])
    second = torch.from_numpy(strips).permute(0, 3, 1, 2).float().div(255)                              # tree.py:308
    run("second_pass", second, dict(input="strips", nrow=1, maxres=1024))
    for k, v in x.items():
        out[f"in/{k}"] = v
    out["names"] = np.array(names)
    out["strip_rows"] = np.array(strip_rows)
    path = os.path.join(HERE, "g26_grid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
