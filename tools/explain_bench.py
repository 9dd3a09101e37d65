"""Times an explained batch (eoe_amd.explain, csrc/explain.hip) at 256 x 3 x 224^2, ViT-B/32 + HSC, next to what the same model costs
anyway -- on the same box in the same run, wall clock around a device synchronise:

  score_fwd        forward-only scoring of the batch (no_grad forward + hsc_score), as eval_cls does it
  train_step       one training step (forward, hsc_loss, backward, FusedAdam)
  input_gradient   explain.input_gradient(model, images, score_fn("hsc")): one forward with the tape on and one backward to the pixels
  saliency         explain.saliency(grad, mode="max", pool=32)
  overlay          explain.overlay(maps, images, 0.6)
so that the cost of an explanation reads as "one backward more per explained batch".  A warm-up, then `--repeats` rounds alternating
the five; medians.  One JSON line.

  python tools/explain_bench.py [--repeats 5] [--batch 256] [--dtype fp16]"""
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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="fp16")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    eoe_amd.set_compute_dtype(a.dtype)
    eoe_amd.set_grad_scale(eoe_amd.default_grad_scale())
    torch.manual_seed(0)
    model = ClipViTB32Custom().cuda().train()
    opt = eoe_amd.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-3)
    g = torch.Generator().manual_seed(1)
    images = torch.rand((a.batch, 3, 224, 224), generator=g).cuda()
    labels = (torch.arange(a.batch) >= a.batch // 2).to(torch.int64).cuda()
    fn = explain.score_fn("hsc")
    keep = {}

    def score_fwd():
        model.eval()
        with torch.no_grad():
            keep["scores"] = eoe_amd.hsc_score(model(images))
        model.train()

    def train_step():
        opt.zero_grad()
        eoe_amd.hsc_loss(model(images), labels, 0).backward()
        opt.step()

    def input_gradient():
        keep["grad"] = explain.input_gradient(model, images, fn)

    def saliency():
        keep["maps"] = explain.saliency(keep["grad"], mode="max", pool=32)

    def overlay():
        keep["heat"] = explain.overlay(keep["maps"], images, 0.6)

    steps = (score_fwd, train_step, input_gradient, saliency, overlay)
    for _ in range(2):
        for f in steps:
            f()
    assert torch.isfinite(keep["grad"]).all() and keep["heat"].shape == (a.batch, 224, 224, 3)
    t = {f.__name__: [] for f in steps}
    for _ in range(a.repeats):
        for f in steps:
            t[f.__name__].append(wall_ms(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"case": "explain", "batch": a.batch, "res": 224, "model": "ViT-B/32 + HSC", "dtype": a.dtype,
                      "box": torch.cuda.get_device_name(0), **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                      "input_gradient_over_train_step": med["input_gradient"] / med["train_step"],
                      "input_gradient_minus_score_fwd_ms": med["input_gradient"] - med["score_fwd"],
                      "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
