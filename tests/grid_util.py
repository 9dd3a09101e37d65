"""The grid fixture (tests/golden/g26_grid.npz, made by tests/golden/make_golden_grid.py) for the CPU and the GPU tests: case loading
and the comparison rules.  Nothing of the kernel is restated here; what a comparison needs beyond the reference picture (where the
marked cells' frames lie and which colour they must have) is stored in the fixture."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_grid.npz")
RESIZE_CASES = ("resize224", "resize130")
_CACHE = {}


def fixture() -> dict:
    if "g" not in _CACHE:
        _CACHE["g"] = dict(np.load(GOLDEN))
    return _CACHE["g"]


def case_names() -> list:
    return [str(n) for n in fixture()["names"] if str(n) != "second_pass"]


def case(name: str, device="cpu"):
    """(src, rows, kwargs of image_grid, reference picture, frame mask or None, frame colours or None)"""
    g = fixture()
    p = json.loads(str(g[f"{name}/params"]))
    src = torch.from_numpy(g["in/" + p["input"]]).to(device)
    kw = dict(nrow=p["nrow"], pad=p["pad"], maxres=p["maxres"], mark=p["mark"], row_sep_at=tuple(p["row_sep_at"]))
    return src, p["rows"], kw, g[f"{name}/ref"], g.get(f"{name}/frame_mask"), g.get(f"{name}/frame_rgb")


def as_f32(src: torch.Tensor, rows) -> torch.Tensor:
    """a uint8 NHWC input as the reference is fed it: the listed rows as ToTensor makes them (u8 / 255, fp32 NCHW)"""
    a = src.cpu().numpy()
    a = a[rows] if rows is not None else a
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)).to(src.device)


def compare(name: str, got, ref, mask, rgb) -> float:
    """the comparison rules.  Every byte equals the reference picture; in a resize case every byte lies within 1 of it (the
    reference's CPU bilinear kernel may order its four products differently; a few ulp in front of a truncation move a byte by at
    most one).  The frame pixels of marked cells are compared against COLORS, not against the reference, which leaves them to an
    undefined cast.  Prints and returns the share of differing bytes."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    inner = np.ones(ref.shape[:2], bool) if mask is None else ~mask
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))[inner]
    share = float((diff != 0).mean())
    print(f"{name}: {share * 100:.4f} % of {diff.size} bytes differ from the reference, max difference {int(diff.max())}")
    assert int(diff.max()) <= (1 if name in RESIZE_CASES else 0), (name, int(diff.max()), share)
    if mask is not None:
        assert mask.any() and np.array_equal(got[mask], rgb[mask]), f"{name}: frame pixels differ from COLORS"
    return share


def second_pass_inputs():
    g = fixture()
    return g["strip_rows"].tolist(), [g[f"strip{i}/ref"] for i in range(len(g["strip_rows"]))], g["second_pass/ref"]
