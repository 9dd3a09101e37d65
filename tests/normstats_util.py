"""Inputs and the tolerance rule of the normalisation-statistics tests (fixture g20_normstats, made by
tests/golden/make_golden_normstats.py from the reference's own code).

Inputs are pure functions of a name (oracle.fill), so the fixture holds only results and the GPU box regenerates the same bits.

Tolerance rule: every comparison is against the fixture's fp64 twin, and the allowance is K_NOISE_PARITY (the project's constant,
tests/test_gpu_parity_big.py) times the distance of the reference's OWN fp32 run to that twin on the same case, measured and
stored by the golden script ("noise/..." keys, asserted non-zero there).  One floor: fitted statistics are handed to kernels as
fp32 numbers, so they cannot be asked for more than one ulp of representation, 2^-23 relative."""
import numpy as np

from oracle import fill as ofill

from test_gpu_parity_big import K_NOISE_PARITY      # the project's constant (3): one definition

STATS_FLOOR = 2.0 ** -23        # relative: one fp32 ulp


def stats_allowance(g, case: str, key: str) -> float:
    return max(K_NOISE_PARITY * float(g[f"noise/stats/{case}/{key}"]), STATS_FLOOR)


def stats_ratio(got, g, case: str, key: str) -> float:
    """relative distance of a fitted statistic to the fp64 twin, in units of its allowance (<= 1 passes)"""
    want = np.asarray(g[f"stats/{case}/{key}64"], np.float64)
    dev = np.max(np.abs(np.asarray(got, np.float64) - want) / np.abs(want))
    return float(dev / stats_allowance(g, case, key))


def op_ratio(got, g, size: str, scale: str, affine: int) -> float:
    """largest per-element distance to the twin relative to max(1, |twin|), in units of 3 x the reference's fp32 noise"""
    want = g[f"op/{size}/{scale}/{affine}/y64"]
    dev = np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want)))
    return float(dev / (K_NOISE_PARITY * float(g[f"noise/op/{size}/{scale}/{affine}"])))


def check_stats_dict(stats: dict, g, case: str, mode: int, what: str = "") -> str:
    """assert a fit_statistics-style dict against the fixture; returns the printable ratios"""
    if mode == 0:
        r = {"mean": stats_ratio(stats["mean"], g, case, "mean"), "std": stats_ratio(stats["std"], g, case, "std")}
    else:
        c = len(stats["mean"])
        assert stats["mean"] == [stats["mean"][0]] * c and stats["std"] == [stats["std"][0]] * c
        r = {"tmin": stats_ratio(stats["mean"][0], g, case, "tmin"), "range": stats_ratio(stats["std"][0], g, case, "range"),
             "tmax": stats_ratio(stats["mean"][0] + stats["std"][0], g, case, "tmax")}
    msg = f"[{what}{case} mode {mode}] deviation / allowance: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items())
    assert stats["mode"] == mode and all(v <= 1.0 for v in r.values()), msg
    return msg


def running_stats_np(x: np.ndarray, batch: int = 2):
    """the yardstick for fitted mean / std: the reference's running statistics over consecutive groups of `batch` images, written
    out on float64 images [m, C, H, W].  Per group: the count goes up by one, the mean moves by (group mean - mean) / count, and the
    spread gains the group's mean of (value - new mean) * (value - old mean); std = sqrt(spread / count).  Returns (mean, std) per
    channel"""
    channels = x.shape[1]
    avg, spread, groups = np.zeros(channels), np.zeros(channels), 0
    for start in range(0, x.shape[0], batch):
        vals = np.moveaxis(x[start:start + batch], 1, -1).reshape(-1, channels)        # every pixel of the group, per channel
        groups += 1
        before = avg
        avg = before + (vals.mean(axis=0) - before) / groups
        spread = spread + ((vals - avg) * (vals - before)).mean(axis=0)
    return avg, np.sqrt(spread / groups)


def torch_gcn_normalize(x, scale: str = "l1", shift=None, range=None, inplace: bool = False):
    """the yardstick for the operator: global contrast normalisation and the per-channel affine in stock torch ops, on any device
    and dtype, as a chain of whole-batch passes (row mean, subtract, row scale, divide, subtract, divide).  `inplace` overwrites
    x (what tools/norm_bench.py times); otherwise x is left alone.  tests/test_cpu_normstats.py pins it to the fixture's twins."""
    import torch
    y = x if inplace else x.clone()
    rows = y.view(y.shape[0], -1)
    rows.sub_(rows.mean(dim=1, keepdim=True))
    if scale == "l1":
        spread = rows.abs().mean(dim=1, keepdim=True)
    elif scale == "l2":
        spread = rows.square().sum(dim=1, keepdim=True).sqrt() / rows.shape[1]
    else:
        raise ValueError(scale)
    rows.div_(spread)
    if shift is not None:
        per_channel = lambda v: torch.as_tensor(v, dtype=y.dtype, device=y.device).view(1, -1, 1, 1)      # noqa: E731
        y.sub_(per_channel(shift)).div_(per_channel(range))
    return y


def stats_set(name: str) -> np.ndarray:
    """the uint8 NHWC image sets of the statistics cases"""
    if name == "ramp37":
        base = ofill.fill_int("g20/ramp37", (37, 32, 32, 3), 0, 96)
        ramp = (np.arange(37) * 4)[:, None, None, None]                 # image i is brighter by 4 i: up to 95 + 144 = 239
        return (base + ramp).astype(np.uint8)
    if name == "gray40":
        return ofill.fill_int("g20/gray40", (40, 28, 28, 1), 0, 256).astype(np.uint8)
    if name == "rect9":
        base = ofill.fill_int("g20/rect9", (9, 64, 48, 3), 0, 200)
        return (base + (np.arange(3) * 20)[None, None, None, :]).astype(np.uint8)
    raise KeyError(name)


def stats_index(name: str):
    """ascending row list of a case (None = the whole set)"""
    if name == "ramp37_idx20":
        pick = np.sort(np.argsort(ofill.uniform_pm1("g20/idx20", 37))[:20])
        return "ramp37", pick.astype(np.int64)
    return name, None


STATS_CASES = ("ramp37", "gray40", "rect9", "ramp37_idx20")
OP_SHAPES = {"32": (6, 3, 32, 32), "28": (5, 1, 28, 28), "224": (2, 3, 224, 224)}
TRAJ_STEPS, TRAJ_HALF = 10, 16


def op_input(size: str) -> np.ndarray:
    return ofill.fill(f"g20/op/{size}", OP_SHAPES[size], std=0.25, mean=0.5)


def traj_batch(i: int):
    """16 normal + 16 OE images of 32 x 32 in [0, 1] (uniform, std 0.25 around 0.5: inside [0.06, 0.94])"""
    x = ofill.fill(f"g20/traj/b{i}", (2 * TRAJ_HALF, 3, 32, 32), std=0.25, mean=0.5)
    y = np.array([0] * TRAJ_HALF + [1] * TRAJ_HALF, dtype=np.int64)
    return x, y
