"""Generates tests/golden/g28_vit_narrow.npz by running the REFERENCE's own `VisualTransformer` (`clip_official/clip/model.py:202-236`) in
fp32 on the CPU at a width that is no multiple of 256: (input_resolution, patch, width, layers, heads, output_dim) =
(64, 16, 192, 2, 3, 64) -- ViT-Ti's width and head count, 17 tokens, n = 2.  Run by hand where the reference is available
(`python tools/make_golden_vit_narrow.py <reference checkout>`); the tests only read the .npz.  The reference is imported at run time.

Weights: oracle.models.deterministic_init(tag="g28", width, layers) on the oracle's VisualTransformer, whose state dict the reference's
module loads strictly; inputs oracle.fill "g28/x", loss = sum(out * fill("g28/dy")).  Stored: the output [2, 64] and the l2 norm of every
parameter's gradient, by the reference's parameter name."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fill, models as omodels   # noqa: E402

GEOMETRY = (64, 16, 192, 2, 3, 64)
N = 2


def main(ref_root):
    spec = importlib.util.spec_from_file_location("_ref_clip_model", os.path.join(ref_root, "src", "eoe", "models", "clip_official", "clip", "model.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    res, patch, width, layers, heads, out_dim = GEOMETRY
    oracle = omodels.deterministic_init(omodels.VisualTransformer(*GEOMETRY), tag="g28", width=width, layers=layers)
    m = ref.VisualTransformer(*GEOMETRY).float()
    m.load_state_dict(oracle.state_dict(), strict=True)
    x = torch.from_numpy(fill.fill("g28/x", (N, 3, res, res), std=1.0))
    dy = torch.from_numpy(fill.fill("g28/dy", (N, out_dim), std=1.0))
    out = m(x)
    (out * dy).sum().backward()
    data = {"out": out.detach().numpy().astype(np.float32), "geometry": np.array(GEOMETRY, dtype=np.int64)}
    for name, p in m.named_parameters():
        data[f"gnorm/{name}"] = np.float64(p.grad.double().norm().item())
    path = os.path.join(ROOT, "tests", "golden", "g28_vit_narrow.npz")
    np.savez(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
