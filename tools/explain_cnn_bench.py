"""Times an explained batch of the BatchNorm CNNs (eoe_amd.explain, csrc/explain.hip): CNN32 at 256 x 3 x 32^2 and CNN28 at 256 x 1 x
28^2, HSC score -- on the same box in the same run, wall clock around a device synchronise:

  score_fwd             forward-only scoring of the batch (no_grad forward + hsc_score), as eval_cls does it
  input_gradient        explain.input_gradient(model, images, score_fn("hsc")): the last hop by eoe_conv_image_dgrad
  input_gradient_torch  the same call with the last hop done by torch.nn.functional.conv_transpose2d on the kernel's own dy (cast to
                        fp32 NCHW, then times scale_inv / std): the yardstick
and the last hop alone, `--inner` launches between two synchronises, host clock over the launch count -- a time per call that
includes the launches' own cost, not kernel time:
  dgrad_kernel          ops.conv_image_dgrad on a 16-bit dy of the first layer's shape (one launch)
  dgrad_torch           the conv_transpose2d route on the same dy (several launches: permute + cast, conv_transpose2d, multiply)
A warm-up, then `--repeats` rounds alternating them; medians, with the smallest and largest round beside them.  One JSON line per model.

  python tools/explain_cnn_bench.py [--repeats 7] [--batch 256] [--dtype fp16] [--inner 50]

Kernel time proper comes from a profiler run of its own; `--profile-loop N` does nothing but N calls of each of the two last-hop routes
per model, for
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/explain_cnn_bench.py --profile-loop 200
whose kernel statistics list conv_image_dgrad_kernel next to the kernels of the torch route."""
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
import torch.nn.functional as F   # noqa: E402

import eoe_amd       # noqa: E402
from eoe_amd import explain, ops               # noqa: E402
from eoe_amd.models import CNN28, CNN32        # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_image_dgrad(dy, conv_w, n, Hi, Wi, stride, pad, std=None, scale_inv=1.0, out=None):
    """ops.conv_image_dgrad by stock torch: dy [n Ho Wo, cout] -> fp32 NCHW, conv_transpose2d with the fp32 weight, the scaling"""
    cout, cin, kh, kw = conv_w.shape
    Ho, Wo = (Hi + 2 * pad - kh) // stride + 1, (Wi + 2 * pad - kw) // stride + 1
    g = dy.view(n, Ho, Wo, cout).permute(0, 3, 1, 2).float()
    opad = (Hi + 2 * pad - kh) % stride
    dx = F.conv_transpose2d(g, conv_w.detach(), stride=stride, padding=pad, output_padding=opad)
    m = torch.full((cin,), float(scale_inv), device=dy.device) if std is None else float(scale_inv) / std
    return dx * m.view(1, cin, 1, 1)


def bench(name, a):
    ch, res, cout = {"CNN32": (3, 32, 32), "CNN28": (1, 28, 16)}[name]
    torch.manual_seed(0)
    model = (CNN32 if name == "CNN32" else CNN28)(bias=True).cuda().train()
    model.set_normalize((0.5,) * ch, (0.25,) * ch)
    g = torch.Generator().manual_seed(1)
    images = torch.rand((a.batch, ch, res, res), generator=g).cuda()
    fn = explain.score_fn("hsc")
    dy = torch.randn((a.batch * res * res, cout), generator=g).to(eoe_amd.compute_dtype()).cuda()
    std = model.normalize[1]
    keep = {}
    real = ops.conv_image_dgrad

    def score_fwd():
        model.eval()
        with torch.no_grad():
            keep["scores"] = eoe_amd.hsc_score(model(images))
        model.train()

    def input_gradient():
        keep["grad"] = explain.input_gradient(model, images, fn)

    def input_gradient_torch():
        ops.conv_image_dgrad = torch_image_dgrad
        try:
            keep["grad_torch"] = explain.input_gradient(model, images, fn)
        finally:
            ops.conv_image_dgrad = real

    def dgrad_kernel():
        for _ in range(a.inner):
            keep["dx"] = real(dy, model.conv1.weight, a.batch, res, res, 1, 2, std=std, scale_inv=1.0 / 256.0)

    def dgrad_torch():
        for _ in range(a.inner):
            keep["dx_torch"] = torch_image_dgrad(dy, model.conv1.weight, a.batch, res, res, 1, 2, std=std, scale_inv=1.0 / 256.0)

    if a.profile_loop:
        a.inner = a.profile_loop
        dgrad_kernel()
        dgrad_torch()
        torch.cuda.synchronize()
        return
    steps = (score_fwd, input_gradient, input_gradient_torch, dgrad_kernel, dgrad_torch)
    for _ in range(2):
        for f in steps:
            f()
    rel = lambda x, y: float((x - y).norm() / y.norm())      # noqa: E731
    assert torch.isfinite(keep["grad"]).all()
    agree = {"input_gradient_vs_torch": rel(keep["grad"], keep["grad_torch"]), "dgrad_vs_torch": rel(keep["dx"], keep["dx_torch"])}
    t = {f.__name__: [] for f in steps}
    for _ in range(a.repeats):
        for f in steps:
            t[f.__name__].append(wall_ms(f))
    for k in ("dgrad_kernel", "dgrad_torch"):
        t[k] = [x / a.inner for x in t[k]]
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()}
    flops = 2.0 * a.batch * res * res * cout * ch * 25
    byts = a.batch * res * res * (cout * 2.0 + ch * 4.0)
    print(json.dumps({"case": "explain_cnn", "model": f"{name} + HSC", "batch": a.batch, "res": res, "dtype": a.dtype,
                      "box": torch.cuda.get_device_name(0), **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                      "dgrad_kernel_over_torch": med["dgrad_kernel"] / med["dgrad_torch"],
                      "input_gradient_over_torch": med["input_gradient"] / med["input_gradient_torch"],
                      "input_gradient_minus_score_fwd_ms": med["input_gradient"] - med["score_fwd"],
                      "dgrad_call_gflops": flops / med["dgrad_kernel"] * 1e-6, "dgrad_call_gbytes_per_s": byts / med["dgrad_kernel"] * 1e-6,
                      "min_max_ms": spread, "relative_distance": agree, "inner": a.inner,
                      "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--profile-loop", type=int, default=0)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    eoe_amd.set_compute_dtype(a.dtype)
    eoe_amd.set_grad_scale(eoe_amd.default_grad_scale())
    for name in ("CNN32", "CNN28"):
        bench(name, a)


if __name__ == "__main__":
    main()
