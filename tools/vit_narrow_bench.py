"""Measures the LayerNorm kernels at widths with and without a partial last 256-column group, and one training step of a narrow tower
beside ViT-B's width:

  * eoe_layernorm_fwd (16-bit out, statistics) and eoe_layernorm_bwd (16-bit dy, dres, dx16, all three column sums) at 12 800 rows for
    D = 192, 256, 384, 512 in ONE process.  GB/s = the bytes the call must move (forward 4 + 2 per element, backward 2 + 4 + 4 in and
    4 + 2 out) over the time.  Every call takes the next of --sets buffer sets, so that the working set (--sets x up to 0.2 GB) does not
    stay in the 256 MB last-level cache between calls.
  * one HSC training step (forward, loss, backward, FusedAdam) of a 12-layer tower at 224 / 16 (197 tokens) for width 384 and 768.

Median of --repeats windows of >= --window seconds of back-to-back calls timed with device events, the sides alternated window by window.
The yardstick of a narrow width is the neighbouring multiple of 256 in the same run.

  python tools/vit_narrow_bench.py [--repeats 5] [--window 0.3] [--rows 12800] [--n 64] [--sets 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd                       # noqa: E402
from eoe_amd import ops              # noqa: E402

WIDTHS = (192, 256, 384, 512)
STEP_WIDTHS = (384, 768)


def window_ms(fn, window_s):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        total = start.elapsed_time(end)
        if total >= window_s * 1e3:
            return total / n
        n = max(n * 2, int(n * 1.2 * window_s * 1e3 / max(total, 1e-3)))


def median_ms(fns, repeats, window_s):
    """{name: median ms per call}, the functions alternated window by window"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ts[k].append(window_ms(fn, window_s))
    return {k: float(np.median(v)) for k, v in ts.items()}


def ln_calls(rows, D, dtype, sets):
    """(forward call, backward call) at width D, each walking `sets` buffer sets"""
    g = torch.Generator(device="cuda").manual_seed(D)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
    gamma, beta = 1 + 0.1 * r(D), 0.1 * r(D)
    bufs = []
    for _ in range(sets):
        x = r(rows, D)
        bufs.append(dict(x=x, y=torch.empty((rows, D), dtype=dtype, device="cuda"), stats=torch.empty((rows, 2), device="cuda"),
                         dy=r(rows, D).to(dtype), res=r(rows, D), dx=torch.empty((rows, D), device="cuda"),
                         dx16=torch.empty((rows, D), dtype=dtype, device="cuda")))
        ops.layernorm_fwd(x, gamma, beta, rows, D, D, bufs[-1]["y"], bufs[-1]["stats"])
    sums = [torch.zeros(D, device="cuda") for _ in range(3)]
    turn = [0, 0]

    def fwd():
        b = bufs[turn[0] % sets]
        turn[0] += 1
        ops.layernorm_fwd(b["x"], gamma, beta, rows, D, D, b["y"], b["stats"])

    def bwd():
        b = bufs[turn[1] % sets]
        turn[1] += 1
        ops.layernorm_bwd(b["dy"], b["x"], b["stats"], gamma, rows, D, D, b["dx"], D, dres=b["res"], dx16=b["dx16"], dgamma=sums[0],
                          dbeta=sums[1], dxsum=sums[2])
    return fwd, bwd


def step_call(width, n, dtype):
    from eoe_amd.models import ClipViTB32Custom
    torch.manual_seed(0)
    m = ClipViTB32Custom(layers=12, input_resolution=224, patch_size=16, width=width, output_dim=512).cuda().train()
    opt = eoe_amd.FusedAdam(m.parameters(), lr=1e-4, weight_decay=1e-3)
    imgs = torch.randn(n, 3, 224, 224, device="cuda")
    lbls = (torch.arange(n, device="cuda") >= n // 2).long()

    def step():
        opt.zero_grad()
        loss = eoe_amd.hsc_loss(m(imgs), lbls, 0)
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rows", type=int, default=12800)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--dtype", default="fp16")
    a = ap.parse_args()
    eoe_amd.set_compute_dtype(a.dtype)
    dtype = eoe_amd.compute_dtype()
    fns = {}
    for D in WIDTHS:
        fns[f"fwd{D}"], fns[f"bwd{D}"] = ln_calls(a.rows, D, dtype, a.sets)
    t = median_ms(fns, a.repeats, a.window)
    res = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "rows": a.rows, "layernorm": {}, "step": {}}
    for D in WIDTHS:
        fb, bb = 6.0 * a.rows * D, 16.0 * a.rows * D
        res["layernorm"][D] = {"fwd_us": 1e3 * t[f"fwd{D}"], "fwd_GBps": fb / t[f"fwd{D}"] / 1e6, "bwd_us": 1e3 * t[f"bwd{D}"],
                               "bwd_GBps": bb / t[f"bwd{D}"] / 1e6}
        print(f"D={D:4d}  fwd {1e3 * t[f'fwd{D}']:7.2f} us {fb / t[f'fwd{D}'] / 1e6:7.0f} GB/s   bwd {1e3 * t[f'bwd{D}']:7.2f} us "
              f"{bb / t[f'bwd{D}'] / 1e6:7.0f} GB/s", flush=True)
    del fns
    torch.cuda.empty_cache()
    steps = {f"w{w}": step_call(w, a.n, dtype) for w in STEP_WIDTHS}
    ts = median_ms(steps, a.repeats, a.window)
    for w in STEP_WIDTHS:
        res["step"][w] = {"n": a.n, "ms": ts[f"w{w}"]}
        print(f"12 layers, 224 / 16, width {w}, n = {a.n}: {ts[f'w{w}']:.3f} ms per step", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
