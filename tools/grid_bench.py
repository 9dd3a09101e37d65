"""Times one generation's worth of the evolve experiment's figures (eoe_amd.imgrid, csrc/grid.hip) for a uniform 32 x 32 pool and
for a ragged pool shown through crop 224 (cells downsampled to 128), on the same box in the same run: 20 individual strips of oesize
8 (`nrow=16`), the raw grid, the grid sorted by fitness and one marked selection grid with its separator (23 pictures).

  device        `image_grid(pool, ids, ...)` and the one copy of each finished uint8 picture back to the host, as `logger.logimg` does
                it (PNG encoding left out on both sides: it is the same work on the same bytes); wall clock around a synchronise.
  device_kernels the same calls with the pictures left on the device (the launch pairs and their table uploads, no copy back);
                device events over a window.
  host          the host way: copy the listed rows back (the windows of a ragged pool are cut on the host from a host copy of the
                set, which is not charged), float ToTensor, the numpy path of `image_grid`; wall clock.
A warm-up, then repeats alternating the variants; medians.  The two paths' pictures are compared first.  One JSON line per pool.

  python tools/grid_bench.py [--repeats 5] [--window 0.2]"""
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
from eoe_amd.data import RaggedImageSet        # noqa: E402
from eoe_amd.evolve import OEPool              # noqa: E402
from eoe_amd.imgrid import image_grid          # noqa: E402

POP, OESIZE = 20, 8


def figures(pop):
    """(ids, kwargs) of one generation's pictures"""
    flat = [i for ind in pop for i in ind]
    figs = [(ind, dict(nrow=16)) for ind in pop]
    figs.append((flat, dict(nrow=OESIZE)))
    figs.append(([i for ind in sorted(pop, key=sum) for i in ind], dict(nrow=OESIZE)))
    mark = [j for i in range(0, POP, 3) for j in range(i * OESIZE, (i + 1) * OESIZE)]
    figs.append((flat + flat, dict(nrow=OESIZE, row_sep_at=(16, POP), mark=mark)))
    return figs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    uniform = torch.from_numpy(rng.integers(0, 256, (4000, 32, 32, 3), dtype=np.uint8))
    ragged = RaggedImageSet([rng.integers(0, 256, (256, int(w), 3) if k % 2 else (int(w), 256, 3), dtype=np.uint8)
                             for k, w in enumerate(rng.integers(256, 400, 200))])
    for case, dev_pool, host_pool in (("uniform32", OEPool(uniform.cuda()), OEPool(uniform)),
                                      ("ragged_crop224", OEPool(ragged.to("cuda"), crop=224), OEPool(ragged, crop=224))):
        pop = [[int(i) for i in rng.integers(0, len(dev_pool), OESIZE)] for _ in range(POP)]
        figs = figures(pop)

        def kernels():
            return [image_grid(dev_pool, ids, **kw) for ids, kw in figs]

        def device():
            return [image_grid(dev_pool, ids, **kw).cpu().numpy() for ids, kw in figs]

        def host():
            out = []
            for ids, kw in figs:
                if host_pool.crop is None:
                    u8 = dev_pool.images[torch.as_tensor(dev_pool.rows(ids), device="cuda")].cpu()       # copy the rows back
                else:
                    u8 = torch.from_numpy(host_pool._windows_host(host_pool.rows(ids)))
                x = torch.from_numpy(np.ascontiguousarray(u8.numpy().transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
                out.append(image_grid(x, **kw).numpy())
            return out

        got, want = device(), host()
        differing = sum(int((g != w).sum()) for g, w in zip(got, want))
        nbytes = sum(g.size for g in got)
        for _ in range(2):
            kernels(), device(), host()
        t = {"device": [], "device_kernels": [], "host": []}
        for _ in range(a.repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            calls = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            while time.perf_counter() - t0 < a.window:
                kernels()
                calls += 1
            end.record()
            end.synchronize()
            t["device_kernels"].append(start.elapsed_time(end) / calls)
            for name, fn, n in (("device", device, 5), ("host", host, 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e3 / n)
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"case": case, "pictures": len(figs), "picture_bytes": nbytes, "differing_bytes": differing,
                          "box": torch.cuda.get_device_name(0), **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                          "speedup_device_vs_host": med["host"] / med["device"],
                          "all_ms": {k: [round(x, 4) for x in v] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
