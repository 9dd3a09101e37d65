"""Times the Gaussian baseline in feature space (eoe_amd.mahalanobis, csrc/mahalanobis.hip) on GPU-resident fp32 features at the shapes
the trainer meets: the fit over CIFAR leave_one_out's and one_vs_rest's normal sets (45 000 x 512, 5 000 x 512), the score of the whole
test split and of an evaluation's extremes (10 000 x 512, 80 x 512), and both once at D = 1024.  Medians of `--repeats` alternated
repeats, wall clock around a synchronised call.

  fit     moments      `mahalanobis.moments_device(x)`: mean, scatter matrix, fourth moment and counts, six launches.  `tf` is
                       n D (D + 1) flop (the upper triangle) over that time.
          torch        `xc = x - x.mean(0); xc.T @ xc` on the device: a centred copy of x and the vendor GEMM.
          host         the features copied back and `sklearn.covariance.LedoitWolf().fit` (NumPy's float64 moments where scikit-learn
                       is missing); once per shape where n D^2 > 10^10.
          fit_gaussian the whole public call: moments, the scatter matrix copied back, Cholesky and inverse on the host, W copied over.
  score   mahalanobis  `mahalanobis.mahalanobis_device(q, mean, W, lower=True)`, three launches; `tf` is 2 nq D^2 over that time
                       (the skipped upper triangle counted, as for the torch route).
          torch        `((q - mean) @ W.T).square().sum(1)` on the device: a centred copy and the nq x D product are materialised.
          host         the features copied back and `mahalanobis_np`.
`*_extra_mb` is the device memory a device route allocates at its peak on top of its inputs, outputs included.  Before anything is timed
the routes' results are compared and the largest relative difference is reported, not asserted.  One JSON line per case.

  python tools/mahalanobis_bench.py [--repeats 5]"""
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
from eoe_amd import mahalanobis as mh          # noqa: E402

FITS = ((45_000, 512), (5_000, 512), (45_000, 1024))
SCORES = ((10_000, 512), (80, 512), (10_000, 1024))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def features(n, D, g):
    """correlated, off-centre: a covariance with a spread of eigenvalues and a mean that matters"""
    mix = torch.eye(D, device="cuda") + torch.randn((D, D), generator=g, device="cuda") * (0.5 / D ** 0.5)
    return (torch.randn((n, D), generator=g, device="cuda") @ mix + 1.0).contiguous()


def medians(routes, repeats, host_calls):
    for _ in range(2):
        for name, fn in routes.items():
            if name != "host":
                fn()
    t = {name: [] for name in routes}
    for i in range(repeats):
        for name, fn in routes.items():
            if name == "host":
                if i < host_calls:
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e3)
            else:
                t[name].append(wall_ms(fn))
    return {k: float(np.median(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    box = torch.cuda.get_device_name(0)
    try:
        from sklearn.covariance import LedoitWolf
    except ImportError:
        LedoitWolf = None
    gauss = {}
    for n, D in FITS:
        x = features(n, D, g)

        def moments():
            return mh.moments_device(x)

        def torch_route():
            xc = x - x.mean(0)
            return xc.T @ xc

        def host():
            xh = x.cpu().numpy()
            if LedoitWolf is not None:
                return LedoitWolf().fit(xh).covariance_
            m = mh.moments_np(xh)
            return m[1] / n

        def fit():
            return mh.fit_gaussian(x)

        S, St = moments()[1], torch_route().double()
        diff = float(((S - St).abs().max() / St.abs().max()).item())
        mem = {"moments": extra_mb(moments), "torch": extra_mb(torch_route)}
        med = medians({"moments": moments, "torch": torch_route, "host": host, "fit_gaussian": fit}, a.repeats,
                      a.repeats if n * D * D <= 10 ** 10 else 1)
        gauss[D] = fit()
        print(json.dumps({"case": "fit", "n": n, "D": D, "box": box, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          **{f"{k}_extra_mb": round(v, 2) for k, v in mem.items()},
                          "moments_tf": round(n * D * (D + 1.0) / (med["moments"] * 1e-3) / 1e12, 2),
                          "torch_tf": round(2.0 * n * D * D / (med["torch"] * 1e-3) / 1e12, 2),
                          "speedup_vs_torch": round(med["torch"] / med["moments"], 3),
                          "speedup_vs_host": round(med["host"] / med["moments"], 2), "host_is": "sklearn" if LedoitWolf else "numpy",
                          "shrinkage": gauss[D].shrinkage, "scatter_max_rel_diff_vs_torch": diff}), flush=True)
    for nq, D in SCORES:
        q = features(nq, D, g)
        mean, W = gauss[D].mean, gauss[D].W

        def ours():
            return mh.mahalanobis_device(q, mean, W, lower=True)[0]

        def torch_route():
            return ((q - mean) @ W.T).square().sum(1)

        def host():
            return mh.mahalanobis_np(q.cpu().numpy(), mean.cpu().numpy(), W.cpu().numpy())

        d, dt = ours(), torch_route()
        diff = float(((d - dt).abs() / dt).max().item())
        mem = {"mahalanobis": extra_mb(ours), "torch": extra_mb(torch_route)}
        med = medians({"mahalanobis": ours, "torch": torch_route, "host": host}, a.repeats, a.repeats)
        print(json.dumps({"case": "score", "nq": nq, "D": D, "box": box, **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          **{f"{k}_extra_mb": round(v, 2) for k, v in mem.items()},
                          "mahalanobis_tf": round(2.0 * nq * D * D / (med["mahalanobis"] * 1e-3) / 1e12, 2),
                          "torch_tf": round(2.0 * nq * D * D / (med["torch"] * 1e-3) / 1e12, 2),
                          "speedup_vs_torch": round(med["torch"] / med["mahalanobis"], 3),
                          "speedup_vs_host": round(med["host"] / med["mahalanobis"], 2), "d2_max_rel_diff_vs_torch": diff}), flush=True)


if __name__ == "__main__":
    main()
