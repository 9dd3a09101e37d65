"""Times the greedy k-center selection (eoe_amd.coreset.kcenter, csrc/coreset.hip) on GPU-resident fp32 features at the shapes a
memory bank is cut from: CIFAR leave_one_out's normal set at 1 % and at 10 % (45 000 x 512, m = 450 and 4 500) and one_vs_rest's
at 10 % (5 000 x 512, m = 500).  Three routes, medians of `--repeats` alternated repeats:

  kcenter        the whole `coreset.kcenter(x, m)` call: scratch, m chained launches, int64 indices, the counts read back at the
                 end; wall clock around a synchronised call.
  torch_ops      the same selection composed from torch ops on the device, per centre `((x - x[c]) ** 2).sum(1)`, `torch.minimum`
                 and a masked `argmax`; the index stays on the device there too.
  host_numpy     `coreset.kcenter_np` on the features copied back, float64.  Every centre costs the same pass, so it is timed over
                 the first `--host-centres` centres and scaled to m (`host_numpy_centres` says how many were run).
`pass_tbs` is what a pass of the kernel achieves, n D 4 m bytes over the time of the call, next to `read_tbs`, a plain fp32 read
of the same matrix (`x.sum()`) timed in the same process: the floor a pass is judged against.  Before anything is timed the routes'
centres are compared (torch_ops rounds and sums in another order, so a near tie may fall the other way and every later centre
with it: the agreement is reported, not asserted).  One JSON line per shape.

  python tools/coreset_bench.py [--repeats 5] [--host-centres 32]"""
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
from eoe_amd import coreset                    # noqa: E402

SHAPES = ((45_000, 512, 450), (45_000, 512, 4_500), (5_000, 512, 500))


def wall_ms(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def torch_kcenter(x, m):
    n = x.shape[0]
    idx = torch.zeros(m, dtype=torch.int64, device=x.device)
    chosen = torch.zeros(n, dtype=torch.bool, device=x.device)
    chosen[0] = True
    d2min = ((x - x[0]) ** 2).sum(1)
    for t in range(1, m):
        c = d2min.masked_fill(chosen, -1.0).argmax()
        idx[t] = c
        chosen[c] = True
        d2min = torch.minimum(d2min, ((x - x[c]) ** 2).sum(1))
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-centres", type=int, default=32)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for n, D, m in SHAPES:
        x = torch.randn((n, D), generator=g, device="cuda")
        xh = x.cpu().numpy()
        mh = min(m, a.host_centres)

        def fused():
            return coreset.kcenter(x, m).idx

        def torch_ops():
            return torch_kcenter(x, m)

        ours, theirs = fused().cpu().numpy(), torch_ops().cpu().numpy()
        same = ours == theirs
        agree = {"torch_ops_centres_equal": float(same.mean()), "torch_ops_first_difference": int(np.argmin(same)) if not same.all() else -1,
                 "host_numpy_centres_equal": float((ours[:mh] == coreset.kcenter_np(xh, mh)[0]).mean())}
        for _ in range(2):
            fused(), torch_ops()
        t = {"kcenter": [], "torch_ops": [], "host_numpy": [], "read": []}
        for i in range(a.repeats):
            t["kcenter"].append(wall_ms(fused))
            t["torch_ops"].append(wall_ms(torch_ops))
            t["read"].append(wall_ms(x.sum, calls=20))
            if i == 0:
                t0 = time.perf_counter()
                coreset.kcenter_np(xh, mh)
                t["host_numpy"].append((time.perf_counter() - t0) * 1e3 * m / mh)
        med = {k: float(np.median(v)) for k, v in t.items()}
        matrix = 4.0 * n * D
        print(json.dumps({"case": "kcenter", "n": n, "D": D, "m": m, "box": torch.cuda.get_device_name(0),
                          **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          "us_per_centre": round(med["kcenter"] * 1e3 / m, 3),
                          "pass_tbs": round(matrix * m / (med["kcenter"] * 1e-3) / 1e12, 3),
                          "read_tbs": round(matrix / (med["read"] * 1e-3) / 1e12, 3),
                          "speedup_vs_torch_ops": round(med["torch_ops"] / med["kcenter"], 3),
                          "speedup_vs_host_numpy": round(med["host_numpy"] / med["kcenter"], 1),
                          "host_numpy_centres": mh, **agree}), flush=True)


if __name__ == "__main__":
    main()
