"""Times one mutation's candidate search of the evolve experiment (eoe_amd.evolve.OEPool, csrc/evolve.hip) at the reference's
pool size, P = 100 candidates against K = 1 parent image, for 32 x 32 x 3 and 256 x 256 x 3 images, on the same box in the same run:

  hip_kernels   `eoe_pool_sqdist_u8` + `eoe_pool_rank` on a resident uint8 set (gather by index included: the kernel reads the listed
                rows), device events around a window of back-to-back calls.  The achieved bytes / s count the candidate bytes
                (P * D), the traffic the kernel cannot avoid.
  hip_call      the whole `OEPool.distances` call as the operators use it: both kernels, the index upload and the one copy of
                distances + order back to the host; wall clock.
  torch_device  the reference's expression `(sample.unsqueeze(0) - new_samples).pow(2).flatten(1).sum(1)` plus `.sort()` with
                stock torch ops on the device over ALREADY GATHERED fp32 tensors (the gather and the uint8 -> fp32 conversion
                are not charged to it); device events, same window rule.
  host          the host loop the device path replaces: gather the 100 images one at a time from a CPU uint8 array, ToTensor
                them, the same expression and sort with torch on the CPU; wall clock.
A warm-up, then repeats alternating the variants; medians over the repeats.  One JSON line per image size.

  python tools/evolve_bench.py [--repeats 5] [--window 0.2]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402

import eoe_amd       # noqa: E402,F401
from eoe_amd._lib import check, lib            # noqa: E402
from eoe_amd.evolve import OEPool              # noqa: E402

P, K = 100, 1


def window_ms(fn, window_s):
    """ms per call over a window of at least window_s seconds, by device events"""
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


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    for hw, n_set in ((32, 4000), (256, 400)):
        host_u8 = rng.integers(0, 256, (n_set, hw, hw, 3), dtype=np.uint8)
        pool = OEPool(torch.from_numpy(host_u8).cuda())
        D = pool.features
        parent = [int(rng.integers(0, n_set))]
        cands = [int(i) for i in rng.integers(0, n_set, P)]
        q, c = np.asarray(parent, np.int32), np.asarray(cands, np.int32)
        # ---- the kernels alone
        need = ctypes.c_size_t(0)
        check(lib.eoe_pool_sqdist_workspace(D, K, P, ctypes.byref(need)), "eoe_pool_sqdist_workspace")
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        dist = torch.empty((K, P), dtype=torch.int64, device="cuda")
        order = torch.empty((K, P), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def hip_kernels():
            check(lib.eoe_pool_sqdist_u8(pool.images.data_ptr(), n_set, D, q.ctypes.data, K, c.ctypes.data, P, dist.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st), "eoe_pool_sqdist_u8")
            check(lib.eoe_pool_rank(dist.data_ptr(), K, P, order.data_ptr(), st), "eoe_pool_rank")

        hip_call = lambda: pool.distances(parent, cands)                                       # noqa: E731
        # ---- the reference's expression on the device, operands gathered beforehand
        sample = pool.images[parent[0]].permute(2, 0, 1).float().div(255)
        new_samples = pool.images[torch.as_tensor(cands, device="cuda")].permute(0, 3, 1, 2).float().div(255).contiguous()
        torch_device = lambda: (sample.unsqueeze(0) - new_samples).pow(2).flatten(1).sum(1).sort()      # noqa: E731

        def host():
            s = torch.from_numpy(host_u8[parent[0]]).permute(2, 0, 1).float().div(255)
            new = torch.stack([torch.from_numpy(host_u8[i]).permute(2, 0, 1).float().div(255) for i in cands])
            return (s.unsqueeze(0) - new).pow(2).flatten(1).sum(1).sort()

        # the variants agree (fp32 against exact integers)
        val, arg = torch_device()
        d_int, o_int = hip_call()
        exact = d_int[0] / 255.0 ** 2
        rel = float(np.max(np.abs(exact - val.cpu().numpy()[np.argsort(arg.cpu().numpy())]) / np.maximum(exact, 1e-9)))
        for _ in range(3):
            hip_kernels(), hip_call(), torch_device(), host()
        t = {"hip_kernels": [], "hip_call": [], "torch_device": [], "host": []}
        for _ in range(a.repeats):
            t["hip_kernels"].append(window_ms(hip_kernels, a.window))
            t["torch_device"].append(window_ms(torch_device, a.window))
            t["hip_call"].append(wall_ms(hip_call, 50))
            t["host"].append(wall_ms(host, 3))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"case": "candidate_search", "size": hw, "P": P, "K": K, "D": D, "box": torch.cuda.get_device_name(0),
                          **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                          "hip_kernels_gbs": P * D / (med["hip_kernels"] * 1e-3) / 1e9,
                          "torch_device_gbs_fp32": 4.0 * P * D / (med["torch_device"] * 1e-3) / 1e9,
                          "speedup_kernels_vs_torch_device": med["torch_device"] / med["hip_kernels"],
                          "speedup_call_vs_host": med["host"] / med["hip_call"], "max_rel_diff_to_fp32": rel,
                          "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
