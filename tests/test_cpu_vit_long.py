"""The oracle's VisualTransformer at a geometry behind the short attention kernels (144 / 16: 82 tokens) against the reference's own module:
tests/golden/g27_vit_long.npz, written by tools/make_golden_vit_long.py.  tests/test_gpu_vit_long.py holds the HIP tower to the same
fixture."""
import numpy as np
import torch

from oracle import fill, models as omodels


def test_oracle_vit_at_82_tokens_reproduces_the_reference(golden):
    g = golden("g27_vit_long")
    geo = tuple(int(v) for v in g["geometry"])
    assert geo == (144, 16, 256, 2, 4, 64)
    m = omodels.deterministic_init(omodels.VisualTransformer(*geo), tag="g27", width=geo[2], layers=geo[3])
    assert m.positional_embedding.shape[0] == 82
    x = torch.from_numpy(fill.fill("g27/x", (2, 3, geo[0], geo[0]), std=1.0))
    dy = torch.from_numpy(fill.fill("g27/dy", (2, geo[5]), std=1.0))
    out = m(x)
    (out * dy).sum().backward()
    # two fp32 evaluations of the same formulas in another order
    assert np.abs(out.detach().numpy() - g["out"]).max() <= 1e-4 * max(1.0, np.abs(g["out"]).max())
    names = [n for n, _ in m.named_parameters()]
    assert {f"gnorm/{n}" for n in names} == {k for k in g if k.startswith("gnorm/")}
    for n, p in m.named_parameters():
        ref = float(g[f"gnorm/{n}"])
        assert abs(p.grad.double().norm().item() - ref) <= 1e-4 * ref + 1e-9, (n, ref)
