"""Times the bootstrap of AUC, AP and FPR at 95 % TPR (eoe_amd.metrics.bootstrap, csrc/bootstrap.hip) with B = 2000 replicates on
GPU-resident scores at 10 000 and at 90 000 scores, with K = 1 and K = 5 score columns, at roughly 10 % positives -- on the same box in
the same run:

  hip_kernels   `eoe_bootstrap_counts` alone (a memset and four launches) into preallocated buffers; device events around a window
                of back-to-back calls.
  device_call   `metrics.bootstrap(labels, scores, 2000)` as the trainer calls it: host labels, the one upload, the buffers, the
                kernels, the one copy back, the `Bootstrap`; wall clock.
  host_call     what a user would do otherwise with this package: copy the scores to the host, then the vectorised NumPy statement
                (`metrics.bootstrap` on the arrays: Philox in uint64 arrays, `bincount`, `reduceat`, `cumsum`); wall clock, the
                device-to-host copy included.
  torch_call    the same work composed from torch ops on the device: a stable `argsort` per column, then per batch of replicates
                `torch.randint` draws, one `bincount`, a gather into sorted order, `cumsum`s, the sums, a `searchsorted` for the
                threshold, and one copy back of the 3 K B numbers; wall clock.  It uses torch's generator: the work is comparable, the
                bits are not (its tables are checked for their ranges and their means only).
A warm-up, then repeats alternating the variants; medians over the repeats, and every repeat's value under `all_ms`.  The scores are
HSC-like (uniform in [0, 1), the positives shifted up; columns 1.. are column 0 plus noise).  The device and the host route are compared
(equal integers, APs within 4 n 2^-53) before anything is timed.  One JSON line per case.

  python tools/bootstrap_bench.py [--repeats 5] [--host-repeats 5] [--window 0.2] [--replicates 2000]"""
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
from eoe_amd import metrics                    # noqa: E402
from eoe_amd._lib import check, lib            # noqa: E402


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


def torch_bootstrap(la, sc, B, tpr, gen):
    """the bootstrap's three tables [K, B] from torch ops on the device, with torch's own draws; returns host arrays"""
    K = sc.shape[0]
    pos, neg = torch.nonzero(la == 1).reshape(-1), torch.nonzero(la == 0).reshape(-1)
    m, n0 = int(pos.numel()), int(neg.numel())
    N = m + n0
    used = torch.cat([pos, neg])
    target = m - metrics.place_for_tpr(tpr, m)
    cols = []
    for k in range(K):
        su = sc[k][used]
        perm = torch.argsort(su, stable=True)
        ss = su[perm]
        start = torch.ones(N, dtype=torch.bool, device=sc.device)
        start[1:] = ss[1:] != ss[:-1]
        idx = torch.arange(N, device=sc.device)
        gstart = torch.cummax(torch.where(start, idx, torch.zeros_like(idx)), 0).values          # the group's first position
        cols.append((perm, gstart, (perm < m).to(torch.int64)))
    u2 = torch.empty(K, B, dtype=torch.int64, device=sc.device)
    fps = torch.empty(K, B, dtype=torch.int64, device=sc.device)
    ap = torch.empty(K, B, dtype=torch.float64, device=sc.device)
    step = max(1, (1 << 22) // N)
    for b0 in range(0, B, step):
        R = min(step, B - b0)
        rows = torch.arange(R, device=sc.device).reshape(-1, 1) * N
        hit = torch.cat([(rows + torch.randint(m, (R, m), device=sc.device, generator=gen)).reshape(-1),
                         (rows + m + torch.randint(n0, (R, n0), device=sc.device, generator=gen)).reshape(-1)])
        c = torch.bincount(hit, minlength=R * N).reshape(R, N)
        for k, (perm, gstart, is_pos) in enumerate(cols):
            cs = c[:, perm]
            cp = cs * is_pos
            cn = cs - cp
            p_in, n_in = torch.cumsum(cp, 1), torch.cumsum(cn, 1)
            p_lt, n_lt = (p_in - cp)[:, gstart], (n_in - cn)[:, gstart]
            u2[k, b0:b0 + R] = (cp * n_lt + cn * (m - p_lt)).sum(1)
            tps, fpc = (m - p_lt).double(), (n0 - n_lt).double()
            ap[k, b0:b0 + R] = (cp.double() / m * (tps / (tps + fpc).clamp_min(1.0))).sum(1)
            at = torch.searchsorted(p_in, torch.full((R, 1), target, dtype=torch.int64, device=sc.device), right=True)
            fps[k, b0:b0 + R] = n0 - n_lt.gather(1, at.clamp_max(N - 1)).reshape(-1)
    return u2.cpu().numpy(), fps.cpu().numpy(), ap.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--replicates", type=int, default=2000)
    ap.add_argument("--host-repeats", type=int, default=None, help="repeats of host_call (default: --repeats); it takes seconds to minutes")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    B, tpr = a.replicates, 0.95
    for n in (10_000, 90_000):
        for K in (1, 5):
            y = (rng.random(n) < 0.1).astype(np.int64)
            base = rng.random(n) + 0.3 * y
            s = np.stack([base + 0.05 * j * rng.standard_normal(n) for j in range(K)]).astype(np.float32)
            sc, la = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
            T = K * (B + 1)
            out = torch.empty(3 * T + 2, dtype=torch.int64, device="cuda")
            scratch = torch.empty(lib.eoe_bootstrap_scratch_bytes(n, K, B), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0)

            def hip_kernels():
                check(lib.eoe_bootstrap_counts(sc.data_ptr(), la.data_ptr(), n, K, B, 0, tpr, out.data_ptr(), out.data_ptr() + 8 * T,
                                               out.data_ptr() + 16 * T, out.data_ptr() + 24 * T, scratch.data_ptr(), st), "eoe_bootstrap_counts")

            device_call = lambda: metrics.bootstrap(y, sc, B, 0, tpr)                       # noqa: E731
            host_call = lambda: metrics.bootstrap(y, sc.cpu().numpy(), B, 0, tpr)           # noqa: E731
            torch_call = lambda: torch_bootstrap(la, sc, B, tpr, gen)                       # noqa: E731

            dev, host = device_call(), host_call()                                          # the warm-up of both, and the check
            assert np.array_equal(dev.counts["u2"], host.counts["u2"]) and np.array_equal(dev.counts["fps"], host.counts["fps"])
            assert np.abs(dev.counts["ap"] - host.counts["ap"]).max() <= 4 * n * 2.0 ** -53
            hip_kernels()
            torch.cuda.synchronize()
            assert out[:T].cpu().numpy().tobytes() == dev.counts["u2"].tobytes()
            tu2, tfps, tap = torch_call()
            m, n0 = dev.n_pos, dev.n_neg
            assert tu2.min() >= 0 and tu2.max() <= 2 * m * n0 and tfps.min() >= 0 and tfps.max() <= n0 and tap.min() > 0 and tap.max() <= 1 + 1e-9
            # another generator, the same distribution: the means agree within a few standard errors of a mean over B replicates
            for mine, theirs in ((dev.auc_reps, tu2 / (2.0 * m * n0)), (dev.ap_reps, tap), (dev.fpr_reps, tfps / float(n0))):
                tol = 6 * np.sqrt((mine.var(axis=1) + theirs.var(axis=1)) / B) + 1e-12
                assert (np.abs(mine.mean(axis=1) - theirs.mean(axis=1)) <= tol).all(), (mine.mean(axis=1), theirs.mean(axis=1), tol)
            variants = {"hip_kernels": lambda: window_ms(hip_kernels, a.window), "device_call": lambda: wall_ms(device_call, 5),
                        "torch_call": lambda: wall_ms(torch_call, 2), "host_call": lambda: wall_ms(host_call, 1)}
            hip_kernels(), device_call(), torch_call()
            t = {k: [] for k in variants}
            host_repeats = a.repeats if a.host_repeats is None else a.host_repeats
            for r in range(a.repeats):
                for k, fn in variants.items():
                    if k != "host_call" or r < host_repeats:
                        t[k].append(fn())
            med = {k: float(np.median(v)) for k, v in t.items()}
            print(json.dumps({"case": "eval_bootstrap", "n": n, "columns": K, "replicates": B, "n_pos": m, "n_neg": n0,
                              "box": torch.cuda.get_device_name(0),
                              **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                              "hip_kernels_gdraws_per_s": float(K) * B * (m + n0) / (med["hip_kernels"] * 1e-3) / 1e9,
                              "speedup_device_call_vs_host_call": med["host_call"] / med["device_call"],
                              "speedup_device_call_vs_torch_call": med["torch_call"] / med["device_call"],
                              "all_ms": {k: [round(x, 5) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
