"""Times one candidate search of the evolve experiment over an OE pool of MIXED sizes (eoe_amd.evolve.OEPool with crop=,
csrc/evolve.hip) at the reference's pool size, P = 100 candidates against K = 1 (mutation) and K = 2 (mating) parent images, on images
shaped like ImageNet after Resize(256) (256 x 341, 341 x 256 and a few other shapes) with the 224 x 224 centre window, three ways on
the same box in the same run:

  ragged     (a) `eoe_pool_sqdist_ragged_u8` + `eoe_pool_rank`: the windows are read straight out of the arena.
  composed   (b) what the parent commit could do: `eoe_ragged_crop_flip_u8` of the K + P centre windows into a scratch tensor, then
                 `eoe_pool_sqdist_u8` + `eoe_pool_rank` on it: (K + P) * 150 528 bytes written and read again, two more launches.
  host       (c) the windows cropped on the device, copied back, and summed and sorted in numpy int64.
`*_kernels_ms`: device events around a window of back-to-back calls, list uploads included (every variant uploads its origins).
`*_call_ms`: the whole call as the operators use it -- `OEPool.distances` for (a); for (b) the same host work, `data.crop_flip_u8`
and a tensor pool's `distances` with its workspace kept -- with the one copy of distances + order back to the host; wall clock.  (c)
has only the wall clock.  A warm-up, then repeats alternating the variants; medians and the min-max spread over the repeats.  The three
must agree bit for bit before anything is timed.  One JSON line per K.

  python tools/ragged_evolve_bench.py [--repeats 5] [--window 0.2]"""
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
from eoe_amd.data import RaggedImageSet, crop_flip_u8        # noqa: E402
from eoe_amd.evolve import OEPool              # noqa: E402

P, CROP = 100, 224
SHAPES = [(256, 341), (341, 256), (256, 256), (256, 384), (256, 455), (384, 256), (256, 307), (321, 256)]
N_SET = 320                                    # 40 images of each shape: about 90 MB, beyond the L2s, inside the Infinity Cache


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
    rs = RaggedImageSet([rng.integers(0, 256, (*SHAPES[i % len(SHAPES)], 3), dtype=np.uint8) for i in range(N_SET)], device="cuda")
    pool = OEPool(rs, crop=CROP)
    D, st = pool.features, torch.cuda.current_stream().cuda_stream
    for K in (1, 2):
        parents = [int(i) for i in rng.integers(0, N_SET, K)]
        cands = [int(i) for i in rng.integers(0, N_SET, P)]
        rows = np.asarray(parents + cands)
        win = np.ascontiguousarray(np.concatenate([rows[:, None], pool._origins[rows]], axis=1), dtype=np.int32)
        out = torch.empty(K * P * 12, dtype=torch.uint8, device="cuda")
        dist, order = out[:K * P * 8].view(torch.int64), out[K * P * 8:].view(torch.int32)
        # ---- (a)
        need = ctypes.c_size_t(0)
        check(lib.eoe_pool_sqdist_ragged_workspace(CROP, CROP, 3, K, P, ctypes.byref(need)), "eoe_pool_sqdist_ragged_workspace")
        ws_a = torch.empty(need.value, dtype=torch.uint8, device="cuda")

        def ragged_kernels():
            check(lib.eoe_pool_sqdist_ragged_u8(rs.arena.data_ptr(), rs.arena.numel(), rs.offsets.data_ptr(), rs.sizes_dev.data_ptr(), N_SET, 3,
                                                CROP, CROP, win.ctypes.data, K, win[K:].ctypes.data, P, dist.data_ptr(), ws_a.data_ptr(),
                                                ws_a.numel(), st), "eoe_pool_sqdist_ragged_u8")
            check(lib.eoe_pool_rank(dist.data_ptr(), K, P, order.data_ptr(), st), "eoe_pool_rank")

        ragged_call = lambda: pool.distances(parents, cands)                                   # noqa: E731
        # ---- (b)
        check(lib.eoe_pool_sqdist_workspace(D, K, P, ctypes.byref(need)), "eoe_pool_sqdist_workspace")
        ws_b = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        params_host = torch.from_numpy(np.ascontiguousarray(np.concatenate([win, np.zeros((K + P, 1), np.int32)], axis=1)))
        params = torch.empty_like(params_host, device="cuda")
        scratch = torch.empty((K + P, CROP, CROP, 3), dtype=torch.uint8, device="cuda")
        qi, ci = np.arange(K, dtype=np.int32), np.arange(K, K + P, dtype=np.int32)

        def composed_kernels():
            params.copy_(params_host, non_blocking=True)
            check(lib.eoe_ragged_crop_flip_u8(rs.arena.data_ptr(), rs.offsets.data_ptr(), rs.sizes_dev.data_ptr(), N_SET, 3, params.data_ptr(),
                                              scratch.data_ptr(), K + P, CROP, CROP, 1, st), "eoe_ragged_crop_flip_u8")
            check(lib.eoe_pool_sqdist_u8(scratch.data_ptr(), K + P, D, qi.ctypes.data, K, ci.ctypes.data, P, dist.data_ptr(), ws_b.data_ptr(),
                                         ws_b.numel(), st), "eoe_pool_sqdist_u8")
            check(lib.eoe_pool_rank(dist.data_ptr(), K, P, order.data_ptr(), st), "eoe_pool_rank")

        def composed_call():
            # what `OEPool.distances` would do with (b) inside it: the same host work for the origins, the public wrappers, one copy back
            r = np.concatenate([pool.rows(parents), pool.rows(cands)])
            p4 = np.concatenate([r[:, None], pool._origins[r], np.zeros((K + P, 1), np.int64)], axis=1).astype(np.int32)
            wins = crop_flip_u8(rs, torch.from_numpy(p4).cuda(), (CROP, CROP), True)
            inner = OEPool(wins)
            inner._workspace = ws_b
            return inner.distances(range(K), range(K, K + P))

        # ---- (c)
        def host_call():
            params.copy_(params_host, non_blocking=True)
            check(lib.eoe_ragged_crop_flip_u8(rs.arena.data_ptr(), rs.offsets.data_ptr(), rs.sizes_dev.data_ptr(), N_SET, 3, params.data_ptr(),
                                              scratch.data_ptr(), K + P, CROP, CROP, 1, st), "eoe_ragged_crop_flip_u8")
            flat = scratch.cpu().numpy().reshape(K + P, -1).astype(np.int64)
            d = np.stack([((flat[K:] - row) ** 2).sum(axis=1) for row in flat[:K]])
            return d, np.argsort(d, axis=1, kind="stable").astype(np.int32)

        # the three agree bit for bit
        ra, rb, rc = ragged_call(), composed_call(), host_call()
        assert ra[0].tobytes() == rb[0].tobytes() == rc[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() == rc[1].tobytes()
        for _ in range(3):
            ragged_kernels(), composed_kernels(), ragged_call(), composed_call()
        t = {"ragged_kernels": [], "composed_kernels": [], "ragged_call": [], "composed_call": [], "host_call": []}
        for _ in range(a.repeats):
            t["ragged_kernels"].append(window_ms(ragged_kernels, a.window))
            t["composed_kernels"].append(window_ms(composed_kernels, a.window))
            t["ragged_call"].append(wall_ms(ragged_call, 50))
            t["composed_call"].append(wall_ms(composed_call, 50))
            t["host_call"].append(wall_ms(host_call, 2))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"case": "ragged_candidate_search", "crop": CROP, "P": P, "K": K, "window_bytes": D, "n_set": N_SET,
                          "arena_mb": round(rs.arena.numel() / 1e6, 1), "box": torch.cuda.get_device_name(0),
                          **{f"{k}_ms": round(v, 5) for k, v in med.items()},
                          "spread_ms": {k: [round(min(v), 5), round(max(v), 5)] for k, v in t.items()},
                          "ragged_kernels_gbs": (P + K) * D / (med["ragged_kernels"] * 1e-3) / 1e9,
                          "speedup_kernels_vs_composed": med["composed_kernels"] / med["ragged_kernels"],
                          "speedup_call_vs_composed": med["composed_call"] / med["ragged_call"],
                          "speedup_call_vs_host": med["host_call"] / med["ragged_call"]}), flush=True)


if __name__ == "__main__":
    main()
