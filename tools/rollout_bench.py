"""Times an attention-rollout batch (eoe_amd.explain.attention_rollout, csrc/rollout.hip) at 256 x 3 x 224^2 on ViT-B/32 (50 tokens) and
ViT-B/16 (197 tokens), next to what the same model costs anyway -- on the same box in the same run, wall clock around a device synchronise:

  score_fwd        forward-only scoring of the batch (no_grad forward + hsc_score), as eval_cls does it
  rollout          explain.attention_rollout(model, images): the forward pass with eoe_attn_probs and eoe_rollout_step per block
  rollout_torch    the same rollout with the probabilities and the products written with torch operations on the device (softmax over
                   the heads' q k^T / 8 in fp32, mean over the heads, row normalisation, bmm); the tower's own kernels for the rest
  input_gradient   explain.input_gradient(model, images, score_fn("hsc")): the other explanation, one backward per batch
A warm-up, then `--repeats` rounds alternating the four; medians.  One JSON line per tower.

  python tools/rollout_bench.py [--repeats 5] [--batch 256] [--dtype fp16] [--towers b32,b16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402
from eoe_amd import explain                    # noqa: E402
from eoe_amd.models import ClipViTB32Custom    # noqa: E402

TOWERS = {"b32": ("ViT-B/32", 32), "b16": ("ViT-B/16", 16)}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rollout_torch(model, images, residual=0.5):
    """attention_rollout's arithmetic with torch operations in place of the two kernels"""
    vit = model.feature_model
    n, grid, patch = images.shape[0], vit.input_resolution // vit.patch_size, vit.patch_size
    L = grid * grid + 1
    blocks = list(vit.transformer.resblocks)
    eye = torch.eye(L, device=images.device)
    r = None
    with torch.no_grad():
        tok = vit.embed(images)
        for i, blk in enumerate(blocks):
            h = blk.n_head
            qkv = explain.block_qkv(blk, tok).view(n, L, 3, h, 64)
            q, k = qkv[:, :, 0].permute(0, 2, 1, 3).float(), qkv[:, :, 1].permute(0, 2, 1, 3).float()
            p = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * 0.125, dim=3).mean(dim=1)
            a = (1.0 - residual) * p + residual * eye
            a = a / a.sum(dim=2, keepdim=True)
            r = a if r is None else torch.bmm(a, r)
            if i + 1 < len(blocks):
                tok = blk.forward_tokens(tok, n)
        m = r[:, 0, 1:].reshape(n, grid, 1, grid, 1).expand(n, grid, patch, grid, patch)
        return m.reshape(n, grid * patch, grid * patch).contiguous()


def bench(tower, a):
    name, patch = TOWERS[tower]
    torch.manual_seed(0)
    model = ClipViTB32Custom(patch_size=patch).cuda().eval()
    g = torch.Generator().manual_seed(1)
    images = torch.rand((a.batch, 3, 224, 224), generator=g).cuda()
    fn = explain.score_fn("hsc")
    keep = {}

    def score_fwd():
        with torch.no_grad():
            keep["scores"] = eoe_amd.hsc_score(model(images))

    def rollout():
        keep["maps"] = explain.attention_rollout(model, images)

    def rollout_torch_():
        keep["maps_torch"] = rollout_torch(model, images)

    def input_gradient():
        keep["grad"] = explain.input_gradient(model, images, fn)

    steps = ((score_fwd, "score_fwd"), (rollout, "rollout"), (rollout_torch_, "rollout_torch"), (input_gradient, "input_gradient"))
    for _ in range(2):
        for f, _n in steps:
            f()
    dev = float((keep["maps"] - keep["maps_torch"]).abs().max())
    assert torch.isfinite(keep["maps"]).all() and dev < 1e-4, dev
    t = {k: [] for _, k in steps}
    for _ in range(a.repeats):
        for f, k in steps:
            t[k].append(wall_ms(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"case": "rollout", "batch": a.batch, "res": 224, "model": name + " + HSC", "tokens": (224 // patch) ** 2 + 1,
                      "dtype": a.dtype, "box": torch.cuda.get_device_name(0), **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                      "rollout_over_score_fwd": med["rollout"] / med["score_fwd"],
                      "rollout_over_input_gradient": med["rollout"] / med["input_gradient"],
                      "rollout_over_rollout_torch": med["rollout"] / med["rollout_torch"], "hip_vs_torch_max_abs": dev,
                      "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}), flush=True)
    del model, images, keep
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--towers", default="b32,b16")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    eoe_amd.set_compute_dtype(a.dtype)
    eoe_amd.set_grad_scale(eoe_amd.default_grad_scale())
    for tower in a.towers.split(","):
        bench(tower, a)


if __name__ == "__main__":
    main()
