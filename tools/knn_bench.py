"""Times the nearest-neighbour search in feature space (eoe_amd.neighbors.feature_knn, csrc/knn.hip) on GPU-resident fp32 features,
k = 5, at the shapes the trainer meets: the extremes of an evaluation against CIFAR one_vs_rest's normal set (80 x 5 000 x 512), the
whole test split against it (10 000 x 5 000 x 512) and against leave_one_out's (10 000 x 45 000 x 512), and a small 256-wide case.
Three routes, medians of `--repeats` alternated repeats:

  feature_knn    the whole `neighbors.feature_knn(q, r, k)` call: scratch, three launches, int64 indices; wall clock around a
                 synchronised call.  `tf` is 2 nq nr D over that time, against the 122 TF of an untuned LDS-tiled fp32-MFMA GEMM.
  cdist_topk     `torch.cdist(q, r)` + `torch.topk(k, largest=False)` on the device: the nq x nr matrix is materialised.
  host_numpy     the features copied back, d2 = |q|^2 + |r|^2 - 2 q r^T in float32 NumPy, argpartition + sort of the k smallest
                 (once per shape where nq nr > 10^8).
`peak_mb` is the device memory each device route allocates at its peak on top of the features.  Before anything is timed the
routes' index sets are compared (cdist_topk may order ties differently and rounds differently: the agreement is reported, not
asserted).  One JSON line per shape.

  python tools/knn_bench.py [--repeats 5]"""
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

import eoe_amd       # noqa: E402,F401
from eoe_amd import neighbors                  # noqa: E402

K = 5
SHAPES = ((80, 5_000, 512), (10_000, 5_000, 512), (10_000, 45_000, 512), (3_000, 1_300, 256))
GUIDE_TF = 122.0


def wall_ms(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for nq, nr, D in SHAPES:
        q = torch.randn((nq, D), generator=g, device="cuda")
        r = torch.randn((nr, D), generator=g, device="cuda")

        def fused():
            return neighbors.feature_knn(q, r, K).idx

        def cdist_topk():
            return torch.topk(torch.cdist(q, r), K, dim=1, largest=False).indices

        def host_numpy():
            qh, rh = q.cpu().numpy(), r.cpu().numpy()
            d2 = (qh * qh).sum(1)[:, None] + (rh * rh).sum(1)[None, :] - 2.0 * (qh @ rh.T)
            part = np.argpartition(d2, K - 1, axis=1)[:, :K]
            return np.take_along_axis(part, np.argsort(np.take_along_axis(d2, part, axis=1), axis=1, kind="stable"), axis=1)

        host_calls = a.repeats if nq * nr <= 10 ** 8 else 1
        ours, theirs = fused().cpu().numpy(), cdist_topk().cpu().numpy()
        agree = {"cdist_topk_rows_equal": float((ours == theirs).all(1).mean())}
        mem = {"feature_knn": peak_mb(fused), "cdist_topk": peak_mb(cdist_topk)}
        for _ in range(2):
            fused(), cdist_topk()
        t = {"feature_knn": [], "cdist_topk": [], "host_numpy": []}
        for i in range(a.repeats):
            t["feature_knn"].append(wall_ms(fused))
            t["cdist_topk"].append(wall_ms(cdist_topk))
            if i < host_calls:
                t0 = time.perf_counter()
                hidx = host_numpy()
                t["host_numpy"].append((time.perf_counter() - t0) * 1e3)
        agree["host_numpy_rows_equal"] = float((ours == hidx).all(1).mean())
        med = {k: float(np.median(v)) for k, v in t.items()}
        tf = 2.0 * nq * nr * D / (med["feature_knn"] * 1e-3) / 1e12
        print(json.dumps({"case": "feature_knn", "nq": nq, "nr": nr, "D": D, "k": K, "box": torch.cuda.get_device_name(0),
                          **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          **{f"{k}_peak_mb": round(v, 2) for k, v in mem.items()},
                          "feature_knn_tf": round(tf, 2), "fraction_of_guide_gemm": round(tf / GUIDE_TF, 3),
                          "speedup_vs_cdist_topk": round(med["cdist_topk"] / med["feature_knn"], 3),
                          "speedup_vs_host_numpy": round(med["host_numpy"] / med["feature_knn"], 2),
                          "host_numpy_calls": host_calls, **agree}), flush=True)


if __name__ == "__main__":
    main()
