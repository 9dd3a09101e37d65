"""Times the long-sequence attention kernels (csrc/attention_long.hip: ops.attn_long_fwd / attn_long_bwd) at the training batch, n = 256
images x 12 heads, L in {145, 197, 257, 577} (ViT-B/32 at 384^2, ViT-B/16 at 224^2, one token behind four key blocks, ViT-B/16 at
384^2), fp16 and bf16, against torch.nn.functional.scaled_dot_product_attention on the same tensors (forward, and backward through
autograd on q, k, v), and against the short kernels at L = 64 scaled by (L / 64)^2 as a sanity line.

Median of --repeats windows of >= --window seconds of back-to-back calls timed with device events (ms per call), the sides alternated
(the other tools' window_ms).  `tf` = useful attention flops (4 n h L^2 64 forward, 10 n h L^2 64 backward: the five products a
backward needs, not the nine this one runs) per second; `frac_of_mfma_loop` = that over the bare fp16 MFMA loop of this box
(eoe_probe_mfma_f16, bench.py's box.mfma_f16_loop_tf), measured in the same process.  One JSON line per (dtype, L).

  python tools/attn_long_bench.py [--repeats 5] [--window 0.3] [--n 256] [--heads 12]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402
import torch.nn.functional as F   # noqa: E402

from eoe_amd import _lib, ops   # noqa: E402

LENGTHS = (145, 197, 257, 577)


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


def mfma_loop_tf():
    """bench.py's box.mfma_f16_loop_tf: 8 workgroups of 4 waves per CU in a bare v_mfma_f32_16x16x32_f16 loop, best of three"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    iters, blocks = 20000, cus * 8
    s = ops._stream()
    fn = lambda: _lib.check(_lib.lib.eoe_probe_mfma_f16(None, iters, blocks, s), "eoe_probe_mfma_f16")   # noqa: E731
    fn()
    best = min(window_ms(fn, 0.15) for _ in range(3)) * 1e-3
    return 2.0 * 16 * 16 * 32 * 8 * iters * 4 * blocks / best / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--heads", type=int, default=12)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    n, heads = a.n, a.heads
    D = heads * 64
    peak = mfma_loop_tf()
    for dtype, dname in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        # the sanity line: the short kernels at their longest sequence
        q64 = torch.randn(n * 64, 3 * D, device="cuda").to(dtype)
        d64, o64, g64 = torch.randn(n * 64, D, device="cuda").to(dtype), torch.empty(n * 64, D, device="cuda", dtype=dtype), torch.empty_like(q64)
        short = median_ms({"fwd": lambda: ops.attn_fwd(q64, o64, n, 64, heads), "bwd": lambda: ops.attn_bwd(q64, d64, g64, n, 64, heads)},
                          a.repeats, a.window)
        del q64, d64, o64, g64
        for L in LENGTHS:
            qkv = torch.randn(n * L, 3 * D, device="cuda").to(dtype)
            dout = torch.randn(n * L, D, device="cuda").to(dtype)
            out, dqkv = torch.empty(n * L, D, device="cuda", dtype=dtype), torch.empty_like(qkv)
            # the same tensors as torch sees them: [n, heads, L, 64] views of the packed rows
            q, k, v = (t.detach().requires_grad_(True) for t in qkv.reshape(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4))
            do4 = dout.reshape(n, L, heads, 64).permute(0, 2, 1, 3)
            with torch.no_grad():
                ref = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(n * L, D).double()
            y = ops.attn_long_fwd(qkv, out, n, L, heads).double()
            rel = float(((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item())
            o_t = F.scaled_dot_product_attention(q, k, v)

            def torch_fwd():
                with torch.no_grad():
                    F.scaled_dot_product_attention(q, k, v)

            def torch_bwd():
                torch.autograd.grad(o_t, (q, k, v), do4, retain_graph=True)

            t = median_ms({"hip_fwd": lambda: ops.attn_long_fwd(qkv, out, n, L, heads),
                           "hip_bwd": lambda: ops.attn_long_bwd(qkv, dout, dqkv, n, L, heads),
                           "torch_fwd": torch_fwd, "torch_bwd": torch_bwd}, a.repeats, a.window)
            ff, fb = 4.0 * n * heads * L * L * 64, 10.0 * n * heads * L * L * 64
            print(json.dumps({"dtype": dname, "n": n, "heads": heads, "L": L,
                              "hip_fwd_ms": round(t["hip_fwd"], 4), "hip_bwd_ms": round(t["hip_bwd"], 4),
                              "torch_sdpa_fwd_ms": round(t["torch_fwd"], 4), "torch_sdpa_bwd_ms": round(t["torch_bwd"], 4),
                              "fwd_speedup_vs_torch": round(t["torch_fwd"] / t["hip_fwd"], 3), "bwd_speedup_vs_torch": round(t["torch_bwd"] / t["hip_bwd"], 3),
                              "short64_scaled_fwd_ms": round(short["fwd"] * (L / 64.0) ** 2, 4), "short64_scaled_bwd_ms": round(short["bwd"] * (L / 64.0) ** 2, 4),
                              "fwd_tf": round(ff / t["hip_fwd"] / 1e9, 1), "bwd_tf": round(fb / t["hip_bwd"] / 1e9, 1),
                              "mfma_f16_loop_tf": round(peak, 1), "fwd_frac_of_mfma_loop": round(ff / t["hip_fwd"] / 1e9 / peak, 4),
                              "bwd_frac_of_mfma_loop": round(fb / t["hip_bwd"] / 1e9 / peak, 4), "rel_rms_vs_torch": rel}), flush=True)
            del qkv, dout, out, dqkv, q, k, v, o_t


if __name__ == "__main__":
    main()
