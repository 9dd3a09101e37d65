"""Times Grad-CAM on WideResNet + CBAM (eoe_amd.explain.grad_cam, csrc/gradcam.hip) at 256 x 3 x 224^2 and, with res=32, at 256 x 3 x
32^2, HSC score -- on the same box in the same run, wall clock around a device synchronise:

  score_fwd          forward-only scoring of the batch (no_grad forward + hsc_score), as eval_cls does it
  grad_cam_layer4    explain.grad_cam(model, images, score_fn("hsc"), layer="layer4"): the backward is pool and fc only
  grad_cam_layer1    the same at layer1: the backward crosses layers 4 ... 2 without a parameter gradient
and the maps alone from one (A, dA) of each of the two layers, both modes:
  maps_kernels       explain.cam_map + explain.cam_upsample (eoe_cam_weights, eoe_cam_map, eoe_cam_upsample)
  maps_torch         the same maps from torch operations on the same A and dA: mean, a product-sum over C, relu, F.interpolate
A warm-up, then `--repeats` rounds alternating them; medians, with the smallest and largest round beside them.  The kernels' own time
comes from the library's profiler scopes (cam_weights, cam_map, cam_upsample) over a loop of its own.  One JSON line per resolution.

  python tools/gradcam_bench.py [--repeats 5] [--batch 256] [--dtype fp16] [--res 224 32]"""
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
from eoe_amd import _lib, explain, ops         # noqa: E402
from eoe_amd.models import WideResNet          # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_maps(A, dA, mode, H, W):
    if mode == "gradcam":
        m = torch.relu((A * dA.mean(dim=(1, 2))[:, None, None, :]).sum(dim=3))
    else:
        m = torch.relu((A * dA).sum(dim=3))
    return F.interpolate(m[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]


def layer_tensors(model, x, layer, sf):
    """(A, dA) of one layer as grad_cam sees them"""
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        a = model.features(x, layer)
    leaf = model.leaf_of(a)
    out = model.head(leaf, layer)
    (dA,) = torch.autograd.grad(sf(out).sum(), leaf)
    for p in model.parameters():
        p.requires_grad_(True)
    model.train()
    return a.detach(), dA.detach()


def bench(res, a):
    torch.manual_seed(0)
    model = WideResNet(res=res).cuda()
    with torch.no_grad():                                            # a trained encoder's state: live spatial gates, used statistics
        for n, p in model.named_parameters():
            if "SpatialGate" in n and n.endswith("bn.weight"):
                p.fill_(1.0)
    x = torch.rand((a.batch, 3, res, res), device="cuda")
    sf = explain.score_fn("hsc")
    model.train()
    with torch.no_grad():
        model(x)                                                     # one training-mode forward moves the running statistics
    model.eval()

    def score_fwd():
        with torch.no_grad():
            return sf(model(x))

    routes = {"score_fwd": score_fwd,
              "grad_cam_layer4": lambda: explain.grad_cam(model, x, sf, layer="layer4"),
              "grad_cam_layer1": lambda: explain.grad_cam(model, x, sf, layer="layer1")}
    tensors = {layer: layer_tensors(model, x, layer, sf) for layer in ("layer4", "layer1")}
    model.eval()
    agree = {}
    for layer, (A, dA) in tensors.items():
        for mode in ("gradcam", "hirescam"):
            key = f"{layer}_{mode}"
            routes[f"maps_kernels_{key}"] = lambda A=A, dA=dA, mode=mode: explain.cam_upsample(explain.cam_map(A, dA, mode), res, res)
            routes[f"maps_torch_{key}"] = lambda A=A, dA=dA, mode=mode: torch_maps(A, dA, mode, res, res)
            k, t = routes[f"maps_kernels_{key}"](), routes[f"maps_torch_{key}"]()
            agree[key] = float((k - t).abs().max() / t.abs().max().clamp_min(1e-30))
    for fn in routes.values():
        fn()
    times = {k: [] for k in routes}
    for _ in range(a.repeats):
        for k, fn in routes.items():
            times[k].append(wall_ms(fn))
    # the kernels' own time: the profiler scopes over a loop of the map routes alone
    scopes = {}
    for k, fn in routes.items():
        if not k.startswith("maps_kernels"):
            continue
        _lib.prof_enable(True)
        try:
            for _ in range(a.inner):
                fn()
            torch.cuda.synchronize()
            prof = _lib.prof_collect()
        finally:
            _lib.prof_enable(False)
        scopes[k] = {name: round(v["total_ms"] / max(v["launches"], 1) * 1e3, 2) for name, v in prof.items() if name.startswith("cam_")}
        scopes[k]["sum"] = round(sum(scopes[k].values()), 2)
    row = {"bench": "gradcam", "res": res, "batch": a.batch, "dtype": a.dtype, "repeats": a.repeats,
           "layer_shapes": {layer: list(A.shape) for layer, (A, _) in tensors.items()},
           "ms": {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in times.items()},
           "kernel_us_per_launch": scopes, "maps_max_rel_diff_to_torch": agree}
    med = {k: v["median"] for k, v in row["ms"].items()}
    row["grad_cam_layer4_over_score_fwd"] = round(med["grad_cam_layer4"] / med["score_fwd"], 3)
    row["grad_cam_layer1_over_score_fwd"] = round(med["grad_cam_layer1"] / med["score_fwd"], 3)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="fp16", choices=("fp16", "bf16"))
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--res", type=int, nargs="+", default=[224, 32])
    a = ap.parse_args()
    eoe_amd.set_compute_dtype(a.dtype)
    ops.set_grad_scale(ops.default_grad_scale())
    for res in a.res:
        bench(res, a)


if __name__ == "__main__":
    main()
