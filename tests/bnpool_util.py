"""Case tables, fp64 references and the tolerance table of the BatchNorm / pooling / junction kernel tests (tests/test_gpu_bnpool.py
on the GPU, tests/test_cpu_bnpool.py without one): eoe_bn_stats, eoe_bn_stats_partials, eoe_bn_act_pool_*, eoe_bn_act_maxpool_*,
eoe_colsum_f32 of csrc/conv.hip and eoe_maxpool_*, eoe_avgpool_*, eoe_add_relu_fwd / eoe_relu_bwd of csrc/cbam.hip.

Inputs are pure functions of a name (oracle.fill).  Every reference is the stock formula in fp64 on exactly the values the kernel
reads: oracle.models.batch_norm, F.leaky_relu, F.max_pool2d(return_indices=True) and torch autograd.  With EOE_Y16 the kernels read
a 16-bit copy of y while the statistics come from the unrounded y; the reference then normalises the rounded values with the
unrounded statistics, straight-through for the gradient (the rule of test_gpu_resnet.test_stem_conv_bn_relu_maxpool_fused).

Input conditions.  y lies on the grid of multiples of 2^-6, so equal taps of a window are bit-equal and tie alike in fp32 and fp64
(the first maximum wins); gamma holds positive and negative entries and exact zeros (the whole window ties: tap 0 wins); with slope
0 about half of every window ties at 0.  tests/test_cpu_bnpool.py asserts for every case that the fp32 evaluation picks the winners
and the signs of z = gamma * xhat + beta that fp64 picks -- zero disagreements, nothing is excluded from any comparison.

Tolerance rule (that of tests/rowops_util.py).  Where an older test fixes a tolerance for a quantity it is reused (TOL_* below, each
with its source); 16-bit outputs get 2 * EPS16 relative on top.  For what no older test reaches -- the statistics themselves, column
sums over tens of thousands of rows, C = 4092, statistics around a large mean -- the yardstick is the reference formula evaluated in
fp32 torch on the CPU: its distance to the fp64 value divided by the quantity's natural scale, the largest such ratio over all cases
of the regime (REF_ERR32, measured by `python tests/bnpool_util.py` and asserted by tests/test_cpu_bnpool.py).  A kernel may be
K_KERNEL = 4 times as far away (it sums in another order and may contract to FMA), plus FLOOR_ULPS fp32 ulps of that scale, plus
FLT_MIN.  Nothing is measured against a kernel."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill as ofill, models as omodels

ULP32 = 2.0 ** -23
FLT_MIN = 2.0 ** -126
K_KERNEL = 4.0
FLOOR_ULPS = 4.0
EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # tests/gpu_util.py
DTYPES = (torch.bfloat16, torch.float16)
GRID = 64.0                                                             # y lies on multiples of 1 / GRID
MOMENTUM = 0.1

# ------------------------------------------------------------------------------------------------ reused tolerances (rtol, atol)
TOL_BN_FWD = (1e-4, 1e-4)                  # test_gpu_cnn.test_bn_act_vs_oracle: "bn+lrelu forward", "bn eval"
TOL_BN_GRAD = (1e-3, 1e-4)                 # ... "bn+lrelu dy", "dgamma", "dbeta"
TOL_AVG_FWD = (1e-6, 1e-6)                 # test_gpu_resnet.test_add_relu_and_avgpool: "avgpool(relu(a+b))"
TOL_AVG_BWD = (1e-6, 1e-7)                 # ... "da", "db"


def tol16(base, dtype):
    """a 16-bit output: 2 * EPS16 relative on top (as rowops_util.tol_ln_y16); dtype None: the fp32 tolerance"""
    return base if dtype is None else (base[0] + 2 * EPS16[dtype], base[1])


# ------------------------------------------------------------------------------------------------ measured reference errors
# key -> largest |fp32-CPU value - fp64 value| / scale over every case of the regime (the scale is named with each spec below).
# The comment holds the figure `python tests/bnpool_util.py` printed and the resulting kernel bound K_KERNEL * value + FLOOR_ULPS
# * ULP32, both in units of the scale.
REF_ERR32 = {
    "bwd4092/dbeta":            7.8e-08,        # measured 7.789e-08 (0.65 ulp) -> kernel bound 6.6 ulp of the scale
    "bwd4092/dgamma":           1.1e-07,        # measured 1.034e-07 (0.87 ulp) -> kernel bound 7.7 ulp of the scale
    "bwd4092/dy":               1.1e-06,        # measured 1.054e-06 (8.84 ulp) -> kernel bound 40.9 ulp of the scale
    "bwdbig/dbeta":             1.5e-07,        # measured 1.438e-07 (1.21 ulp) -> kernel bound 9.0 ulp of the scale
    "bwdbig/dgamma":            1.5e-07,        # measured 1.479e-07 (1.24 ulp) -> kernel bound 9.0 ulp of the scale
    "colsum/1":                 3.7e-08,        # measured 3.668e-08 (0.31 ulp) -> kernel bound 5.2 ulp of the scale
    "colsum/3":                 5.4e-08,        # measured 5.336e-08 (0.45 ulp) -> kernel bound 5.8 ulp of the scale
    "colsum/70000":             4.6e-08,        # measured 4.522e-08 (0.38 ulp) -> kernel bound 5.5 ulp of the scale
    "partials/mean":            3.2e-08,        # measured 3.195e-08 (0.27 ulp) -> kernel bound 5.1 ulp of the scale
    "partials/rmean":           1.1e-07,        # measured 1.098e-07 (0.92 ulp) -> kernel bound 7.7 ulp of the scale
    "partials/rstd":            1.6e-07,        # measured 1.530e-07 (1.28 ulp) -> kernel bound 9.4 ulp of the scale
    "partials/rvar":            9.4e-08,        # measured 9.330e-08 (0.78 ulp) -> kernel bound 7.2 ulp of the scale
    "stats/mean":               6.2e-08,        # measured 6.167e-08 (0.52 ulp) -> kernel bound 6.1 ulp of the scale
    "stats/rmean":              1.5e-07,        # measured 1.409e-07 (1.18 ulp) -> kernel bound 9.0 ulp of the scale
    "stats/rstd":               1.7e-07,        # measured 1.680e-07 (1.41 ulp) -> kernel bound 9.7 ulp of the scale
    "stats/rvar":               1.3e-07,        # measured 1.201e-07 (1.01 ulp) -> kernel bound 8.4 ulp of the scale
    "stats_bigmean/mean":       1.2e-07,        # measured 1.132e-07 (0.95 ulp) -> kernel bound 8.0 ulp of the scale
    "stats_bigmean/rmean":      1.5e-07,        # measured 1.465e-07 (1.23 ulp) -> kernel bound 9.0 ulp of the scale
    "stats_bigmean/rstd":       1.4e-07,        # measured 1.301e-07 (1.09 ulp) -> kernel bound 8.7 ulp of the scale
    "stats_bigmean/rvar":       9.7e-08,        # measured 9.640e-08 (0.81 ulp) -> kernel bound 7.3 ulp of the scale
}


def bound_factor(key):
    return K_KERNEL * REF_ERR32[key] + FLOOR_ULPS * ULP32


# ------------------------------------------------------------------------------------------------ comparing
def meas(key, scale):
    return ("meas", key, scale)


def tol(rt):
    return ("tol", rt[0], rt[1])


def _np64(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().float().cpu().double().numpy() if v.dtype != torch.float64 else v.detach().cpu().numpy()
    return np.asarray(v, np.float64)


def _amax(t):
    return float(np.abs(_np64(t)).max())


def deviation(got, ref, spec):
    """(largest error / allowance, message) of one quantity; a non-finite result counts as infinitely far"""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not np.isfinite(g).all():
        return float("inf"), "non-finite values in the result"
    err = np.abs(g - r)
    if spec[0] == "tol":
        allow = spec[2] + spec[1] * np.abs(r) + FLT_MIN
    else:
        allow = bound_factor(spec[1]) * np.broadcast_to(_np64(spec[2]), r.shape) + FLT_MIN
    ratio = err / allow
    i = int(np.argmax(ratio)) if ratio.size else 0
    return float(ratio.max()) if ratio.size else 0.0, (f"max err/allowance {float(ratio.max()):.3f} at flat index {i} (got "
                                                       f"{g.flatten()[i]:.9g}, ref {r.flatten()[i]:.9g}, allowed {allow.flatten()[i]:.3e})")


def compare(what, got: dict, ref: dict, specs: dict, names=None, verbose=True):
    """assert every quantity of `names` (or of `specs`) against the fp64 reference; prints each figure before it asserts"""
    bad = []
    for name in (names or specs):
        ratio, msg = deviation(got[name], ref[name], specs[name])
        if verbose:
            print(f"[{what}] {name}: {msg}")
        if not ratio <= 1.0:
            bad.append(f"{name}: {msg}")
    assert not bad, f"{what}: " + "; ".join(bad)


def measure_into(table: dict, got32: dict, ref: dict, specs: dict):
    """fold the fp32-CPU evaluation's scaled errors of one case into `table` (key -> largest so far)"""
    for name, spec in specs.items():
        if spec[0] != "meas":
            continue
        err = np.abs(_np64(got32[name]) - _np64(ref[name]))
        scale = np.broadcast_to(_np64(spec[2]), err.shape)
        with np.errstate(divide="ignore", invalid="ignore"):          # a zero scale asks for the exact value
            err = np.maximum(err - FLT_MIN, 0.0)
            ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
        table[spec[1]] = max(table.get(spec[1], 0.0), float(ratio.max()))


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def round16(a: np.ndarray, dtype) -> np.ndarray:
    """fp32 array holding the values rounded to the 16-bit dtype (None: left alone)"""
    return a if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def grid_fill(name, shape, std=1.0, mean=0.0):
    """oracle.fill rounded to the grid of multiples of 2^-6 (exact in fp32 and, at these magnitudes, in fp16)"""
    return (np.round(ofill.fill(name, shape, std=std, mean=mean).astype(np.float64) * GRID) / GRID).astype(np.float32)


def gamma_beta(tag, C):
    """gamma: negative at c % 4 == 1, exactly 0 at c % 8 == 2 (there beta is 0 at c % 16 == 2: z == 0 everywhere, and nonzero at
    c % 16 == 10), positive elsewhere; |gamma| in [0.5, 1.5] so that no two grid values of y collapse into one z"""
    g = 0.5 + np.abs(ofill.fill(f"bnpool/{tag}/g", (C,), std=1.0 / math.sqrt(3.0)))
    b = ofill.fill(f"bnpool/{tag}/b", (C,), std=0.5)
    c = np.arange(C)
    g[c % 4 == 1] *= -1.0
    g[c % 8 == 2] = 0.0
    b[c % 16 == 2] = 0.0
    return g.astype(np.float32), b.astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1 / 2. statistics
EPS_BN = 1e-4
# (M, C): VEC = 1 | cpb = 1 | the boundary of the four-loads-in-flight loop (step 64: 1024 = 4 full iterations) | gy > 512 |
# gx * gy > 1024 | the channel tail of the 16-column finalize
STATS_CASES = ((37, 1), (37, 3), (37, 5), (2, 4), (300, 4), (1023, 64), (1024, 64), (1025, 64), (33000, 256), (4200, 4096), (500, 20))
STATS_BIGMEAN = (2000, 64)                 # per-channel mean = 8 x std
PARTIALS_R = (1, 63, 1024, 1025, 2049, 3000)
PARTIALS_C = (4, 20)


def stats_launch(M, C):
    """(vec, cpb, gx, gy, capped by gx*gy, capped by 512) of eoe_bn_stats' launch arithmetic, restated for the table's claims"""
    vec = 4 if C % 4 == 0 else 1
    cols = C // vec
    cpb = 1
    while cpb < 64 and cpb < cols:
        cpb *= 2
    rpb = 256 // cpb
    gy = -(-M // (rpb * 16))
    gx = -(-cols // cpb)
    cap1 = gy * gx > 1024
    if cap1:
        gy = 1024 // gx
    cap2 = gy > 512
    if cap2:
        gy = 512
    return vec, cpb, gx, max(gy, 1), cap1, cap2


def running0(tag, C):
    return (ofill.fill(f"bnpool/{tag}/rm", (C,), std=0.3), ofill.fill(f"bnpool/{tag}/rv", (C,), std=0.2, mean=1.5))


def stats_eval(y, rm0, rv0, dt, eps=EPS_BN):
    """training-mode statistics through oracle.models.batch_norm: mean, rstd and the updated running buffers"""
    x, rm, rv = _t(y, dt), _t(rm0, dt).clone(), _t(rv0, dt).clone()
    omodels.batch_norm(x, None, None, rm, rv, True, MOMENTUM, eps)
    mu = x.mean(dim=0)
    var = ((x - mu[None]) ** 2).mean(dim=0)
    return {"mean": mu, "rstd": 1.0 / torch.sqrt(var + eps), "rmean": rm, "rvar": rv}


def stats_specs(regime, ref):
    """scales: the mean in units of the spread plus its own size (1 / rstd + |mean|); rstd and the running variance relative; the
    running mean its own size or the momentum's share of the mean's scale"""
    s_mean = 1.0 / _np64(ref["rstd"]) + np.abs(_np64(ref["mean"]))
    return {"mean": meas(f"{regime}/mean", s_mean), "rstd": meas(f"{regime}/rstd", _np64(ref["rstd"])),
            "rmean": meas(f"{regime}/rmean", np.maximum(np.abs(_np64(ref["rmean"])), MOMENTUM * s_mean)),
            "rvar": meas(f"{regime}/rvar", _np64(ref["rvar"]))}


@functools.lru_cache(maxsize=None)
def stats_case(M, C, bigmean=False):
    tag = f"stats/{M}x{C}" + ("/big" if bigmean else "")
    if bigmean:
        sd = 0.5 + 1.5 * np.abs(ofill.fill(f"bnpool/{tag}/sd", (C,), std=1.0 / math.sqrt(3.0)))
        y = (ofill.fill(f"bnpool/{tag}/y", (M, C), std=1.0, mean=8.0) * sd[None]).astype(np.float32)
    else:
        y = ofill.fill(f"bnpool/{tag}/y", (M, C), std=1.0, mean=0.3)
    rm0, rv0 = running0(tag, C)
    ref = stats_eval(y, rm0, rv0, torch.float64)
    return {"y": y, "rm0": rm0, "rv0": rv0, "ref": ref, "got32": stats_eval(y, rm0, rv0, torch.float32),
            "specs": stats_specs("stats_bigmean" if bigmean else "stats", ref)}


def partials_eval(part, M, rm0, rv0, dt, eps=EPS_BN):
    """the statistics of partial rows [R][2][C] (column sums and sums of squares): mean = S / M, var = Q / M - mean^2"""
    p, rm, rv = _t(part, dt), _t(rm0, dt), _t(rv0, dt)
    mu = p[:, 0].sum(0) / M
    var = torch.clamp(p[:, 1].sum(0) / M - mu * mu, min=0.0)
    return {"mean": mu, "rstd": 1.0 / torch.sqrt(var + eps), "rmean": (1 - MOMENTUM) * rm + MOMENTUM * mu,
            "rvar": (1 - MOMENTUM) * rv + MOMENTUM * var * (M / max(M - 1, 1))}


@functools.lru_cache(maxsize=None)
def partials_case(R, C):
    """the rows an NT GEMM with `colstats` leaves: per 64 rows of a y [64 R, C] the fp32 column sums and sums of squares"""
    tag = f"partials/{R}x{C}"
    M = 64 * R
    y = ofill.fill(f"bnpool/{tag}/y", (M, C), std=1.0, mean=0.3).astype(np.float64).reshape(R, 64, C)
    part = np.stack([y.sum(1), (y * y).sum(1)], axis=1).astype(np.float32)          # [R, 2, C]
    rm0, rv0 = running0(tag, C)
    ref = partials_eval(part, M, rm0, rv0, torch.float64)
    return {"part": part, "M": M, "rm0": rm0, "rv0": rv0, "ref": ref, "got32": partials_eval(part, M, rm0, rv0, torch.float32),
            "specs": stats_specs("partials", ref)}


# ------------------------------------------------------------------------------------------------ 3 - 5. BatchNorm + act + pool
def out_hw(H, W, pool):
    """pool: ('win', P) the P x P / stride P window of eoe_bn_act_pool, or ('max', k, stride, pad) of eoe_bn_act_maxpool"""
    if pool[0] == "win":
        return H // pool[1], W // pool[1]
    _, k, s, p = pool
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _nchw(a, dt):
    return _t(a, dt).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def bn_act_eval(c, dt):
    """forward and every gradient of pool(leaky_relu(bn(y))) in dtype `dt`.  out / idx / z are NHWC, `flat` is the NCHW flatten
    [n, C Ho Wo], dy is [n H W, C]; idx holds the kernel's tap code ky * k + kx (for ('win', P): the tap inside the P x P window)"""
    n, H, W, C = c["y"].shape
    pool, eps, slope = c["pool"], c["eps"], c["slope"]
    yv = _nchw(c["y"], dt).requires_grad_(True)
    x = yv if c["yq"] is None else yv + (_nchw(c["yq"], dt) - yv).detach()
    if c["gamma"] is None:
        g, b = torch.ones(C, dtype=dt, requires_grad=True), torch.zeros(C, dtype=dt, requires_grad=True)
    else:
        g, b = _t(c["gamma"], dt).requires_grad_(True), _t(c["beta"], dt).requires_grad_(True)
    if not c["training"]:
        rm, rv = _t(c["rm"], dt), _t(c["rv"], dt)
        z = omodels.batch_norm(x, g, b, rm, rv, False, MOMENTUM, eps)
        mu, var = rm, rv
    else:
        mu = yv.mean(dim=(0, 2, 3))
        var = ((yv - mu.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        if c["yq"] is None:
            z = omodels.batch_norm(x, g, b, torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt), True, MOMENTUM, eps)
        else:
            z = (x - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    a = F.leaky_relu(z, slope)
    k, s, p = (pool[1], pool[1], 0) if pool[0] == "win" else pool[1:]
    if k == 1 and s == 1:
        out, tap = a, torch.zeros(a.shape, dtype=torch.int64)
    else:
        out, ix = F.max_pool2d(a, k, s, p, return_indices=True)
        Ho, Wo = out.shape[2:]
        ky = ix // W - (torch.arange(Ho).view(1, 1, Ho, 1) * s - p)
        kx = ix % W - (torch.arange(Wo).view(1, 1, 1, Wo) * s - p)
        assert int(ky.min()) >= 0 and int(ky.max()) < k and int(kx.min()) >= 0 and int(kx.max()) < k
        tap = ky * k + kx
    (out * _nchw(c["dout"], dt)).sum().backward()
    return {"out": _nhwc(out), "out16": _nhwc(out), "flat": out.detach().reshape(n, -1), "idx": _nhwc(tap).to(torch.uint8), "z": _nhwc(z),
            "dy": _nhwc(yv.grad).reshape(n * H * W, C), "dgamma": g.grad, "dbeta": b.grad,
            "mean": mu.detach(), "rstd": (1.0 / torch.sqrt(var + eps)).detach()}


@functools.lru_cache(maxsize=None)
def bn_act_case(tag, n, H, W, C, pool, slope, training=True, affine=True, ydtype=None, eps=EPS_BN):
    """inputs (numpy fp32), fp64 reference and fp32-CPU evaluation of one BatchNorm + activation + pool case.  ydtype: the kernel
    reads y rounded to that 16-bit type (EOE_Y16); `yq` holds those values in fp32"""
    y = grid_fill(f"bnpool/{tag}/y", (n, H, W, C), std=1.0, mean=0.25)
    Ho, Wo = out_hw(H, W, pool)
    c = {"y": y, "yq": None if ydtype is None else round16(y, ydtype), "pool": pool, "slope": slope, "training": training, "eps": eps,
         "gamma": None, "beta": None, "dout": ofill.fill(f"bnpool/{tag}/dout", (n, Ho, Wo, C), std=1.0)}
    if affine:
        c["gamma"], c["beta"] = gamma_beta(tag, C)
    c["rm"], c["rv"] = running0(tag, C)
    c["ref"] = bn_act_eval(c, torch.float64)
    c["got32"] = bn_act_eval(c, torch.float32)
    return c


def stats32(c):
    """what a test hands to the kernel as `stats` [2 C]: the fp64 (mean, rstd) of the reference rounded to fp32"""
    return torch.cat([c["ref"]["mean"], c["ref"]["rstd"]]).float()


def act_specs(c, out_dtype=None, dy_dtype=None, regime=None):
    """reused tolerances; regime 'bwd4092' measures dy / dgamma / dbeta (scale: the channel's largest |dy|, the largest column sum),
    regime 'bwdbig' measures dgamma / dbeta (tens of thousands of rows)"""
    ref = c["ref"]
    s = {"out": tol(TOL_BN_FWD), "flat": tol(tol16(TOL_BN_FWD, out_dtype)), "out16": tol(tol16(TOL_BN_FWD, out_dtype)),
         "dy": tol(tol16(TOL_BN_GRAD, dy_dtype)), "dgamma": tol(TOL_BN_GRAD), "dbeta": tol(TOL_BN_GRAD)}
    if regime is not None:
        for k in ("dgamma", "dbeta"):
            s[k] = meas(f"{regime}/{k}", _amax(ref[k]))
    if regime == "bwd4092" and dy_dtype is None:
        s["dy"] = meas("bwd4092/dy", np.abs(_np64(ref["dy"])).max(0, keepdims=True))
    return s


# 3. forward of eoe_bn_act_pool on non-square maps
FWD_SHAPES = ((3, 6, 10), (2, 1, 4))
FWD_C = (4, 12, 48)
FWD_SLOPES = (0.0, 0.01, 1.0)
FWD_YKINDS = (None, torch.bfloat16, torch.float16)


def fwd_cases():
    """(n, H, W, C, P, slope, affine, ydtype): every C x pool x y type on each map (the 1 x 4 map takes pool 1 only), the slopes
    rotating so that each meets every C, pool and y type; gamma = beta = NULL at C = 12 with an fp32 y"""
    out = []
    for si, (n, H, W) in enumerate(FWD_SHAPES):
        for pi, P in enumerate((1, 2)):
            if H % P or W % P:
                continue
            for ci, C in enumerate(FWD_C):
                for yi, yd in enumerate(FWD_YKINDS):
                    out.append((n, H, W, C, P, FWD_SLOPES[(si + pi + ci + yi) % 3], not (C == 12 and yd is None), yd))
    return out


def fwd_case(n, H, W, C, P, slope, affine, yd):
    return bn_act_case(f"fwd/{n}x{H}x{W}x{C}/p{P}", n, H, W, C, ("win", P), slope, True, affine, yd)


# 4. backward of eoe_bn_act_pool.  C -> map: q = (C/4) / gcd(C/4, 256) workgroups at least
#   4: q 1, 180 / 45 items: one partly idle workgroup           12: q 3, 72 / 18 items: one partly idle workgroup and two empty ones
#   20: q 5, 7700 items on a grid of 30 x 256 (pool 1): not a multiple of the stride, and the apply pass reloads its quad
#   1028: q 257, more quads than threads, 257 workgroups for 25 of work      4092: q 1023, the largest C / 4 the entry point takes
#   4096: 1024 quads, q 4: a workgroup holds a quad at most once
BWD_MAPS = {4: (3, 6, 10), 12: (2, 2, 6), 20: (5, 14, 22), 1028: (2, 2, 6), 4092: (2, 2, 2), 4096: (2, 2, 6)}
BWD_BIG = (9, 64, 60, 64)                  # 552960 items > 2 * 1024 * 256: two positions per iteration and the 1024-row cap
# option sets (P flips with the parity of the C index, so that every MODE x P x YT runs):
#   (P, nchw_flat, dy dtype, training, accumulate, dgamma / dbeta given, y dtype)
BWD_OPTIONS = ((1, 0, None, True, 0, True, None),
               (2, 1, torch.float16, False, 1, True, torch.float16),
               (2, 0, torch.bfloat16, True, 0, False, torch.bfloat16),
               (1, 1, None, True, 1, True, None),
               (2, 0, torch.bfloat16, False, 0, True, None))


def bwd_cases():
    """(n, H, W, C, P, flat, dy dtype, training, accumulate, dgb, y dtype, slope)"""
    out = []
    for ci, (C, (n, H, W)) in enumerate(BWD_MAPS.items()):
        for oi, (P, flat, dyd, training, acc, dgb, yd) in enumerate(BWD_OPTIONS):
            if ci % 2:
                P = 3 - P
            out.append((n, H, W, C, P, flat, dyd, training, acc, dgb, yd, (0.0, 0.01)[(ci + oi) % 2]))
    out.append(BWD_BIG + (1, 0, None, True, 0, True, None, 0.01))
    return out


def bwd_case(n, H, W, C, P, flat, dyd, training, acc, dgb, yd, slope):
    c = dict(bn_act_case(f"bwd/{n}x{H}x{W}x{C}/p{P}", n, H, W, C, ("win", P), slope, training, True, yd))
    regime = "bwd4092" if C == 4092 else "bwdbig" if (n, H, W, C) == BWD_BIG else None
    c["specs"] = act_specs(c, None, dyd, regime)
    c["pre"] = None
    if acc:                                # what dgamma / dbeta hold before an accumulating call
        c["pre"] = {k: ofill.fill(f"bnpool/bwd/pre_{k}/{C}", (C,), std=1.0, mean=3.0) for k in ("dgamma", "dbeta")}
        c["ref"], c["got32"] = dict(c["ref"]), dict(c["got32"])
        for k, v in c["pre"].items():
            c["ref"][k] = c["ref"][k] + _t(v, torch.float64)
            c["got32"][k] = c["got32"][k] + _t(v, torch.float32)
        if regime is not None:
            c["specs"] = act_specs(c, None, dyd, regime)
    return c


def bwd_launch(n, H, W, C, P):
    """(items, q, workgroups of the reduce pass, workgroups of the apply pass) of eoe_bn_act_pool_bwd's launch arithmetic"""
    cc = C // 4
    items = n * (H // P) * (W // P) * cc
    grid = min(max(-(-items // 256), 1), 4096)
    q = cc // math.gcd(cc, 256)
    g0 = max(min(grid, 1024) // q * q, q)
    return items, q, g0, grid


# 5. eoe_bn_act_maxpool: (k, stride, pad, H, W)
MAXPOOL_GEOS = ((3, 2, 1, 6, 10),          # the s2k3 kernel on a non-square map
                (3, 2, 1, 7, 9),           # odd map: the generic kernel with S = 2
                (3, 2, 0, 8, 6),           # Ho != H / 2: generic, and the last row and column fall in no window
                (3, 1, 1, 5, 7),           # S = 1
                (2, 3, 0, 8, 7),           # run-time stride, pixels between the windows
                (2, 2, 1, 5, 6))           # windows hanging into the padding
MAXPOOL_C = (4, 12, 64)
MAXPOOL_N = 2
EPS_MAXPOOL = 1e-5                         # the stem's BatchNorm


def maxpool_slope(gi, ci):
    return (0.0, 0.01)[(gi + ci) % 2]


def maxpool_case(gi, C, training, yd=None):
    k, s, p, H, W = MAXPOOL_GEOS[gi]
    slope = maxpool_slope(gi, MAXPOOL_C.index(C))
    return bn_act_case(f"maxpool/{gi}/{C}", MAXPOOL_N, H, W, C, ("max", k, s, p), slope, training, True, yd, EPS_MAXPOOL)


def is_s2k3(k, s, p, H, W):
    Ho, Wo = out_hw(H, W, ("max", k, s, p))
    return k == 3 and s == 2 and p == 1 and H % 2 == 0 and W % 2 == 0 and Ho == H // 2 and Wo == W // 2


def unwon_pixels(c):
    """[n, H, W, C] bool: pixels that win no window (their upstream gradient is empty)"""
    n, H, W, C = c["y"].shape
    k, s, p = c["pool"][1:]
    won = torch.zeros(n, C, H * W, dtype=torch.bool)
    Ho, Wo = out_hw(H, W, c["pool"])
    tap = c["ref"]["idx"].permute(0, 3, 1, 2).long()
    ih = tap // k + torch.arange(Ho).view(1, 1, Ho, 1) * s - p
    iw = tap % k + torch.arange(Wo).view(1, 1, 1, Wo) * s - p
    won.scatter_(2, (ih * W + iw).reshape(n, C, -1), True)
    return ~won.reshape(n, C, H, W).permute(0, 2, 3, 1)


def all_act_cases():
    """(what, case) of every BatchNorm + activation + pool case of the tables, each evaluation once"""
    seen = {}
    for a in fwd_cases():
        seen[("fwd",) + a] = fwd_case(*a)
    for a in bwd_cases():
        seen[("bwd",) + a] = bwd_case(*a)
    for gi in range(len(MAXPOOL_GEOS)):
        for C in MAXPOOL_C:
            for training in (True, False):
                for yd in (None,) + DTYPES:
                    seen[("maxpool", gi, C, training, yd)] = maxpool_case(gi, C, training, yd)
    return list(seen.items())


# ------------------------------------------------------------------------------------------------ 6. eoe_colsum_f32, accumulate
COLSUM_C = (4, 1028, 4092)
COLSUM_ROWS = (1, 3, 70000)
COLSUM_PERIOD = 61


@functools.lru_cache(maxsize=None)
def colsum_case(rows, C):
    """x [rows, C] repeats a table of COLSUM_PERIOD (a prime) grid rows, so the 70000 x 4092 matrix (1.1 GB) is built where it is
    needed from 1 MB and its fp64 column sums are counts x table rows, exact; `pre` is what `out` holds before the call"""
    table = grid_fill(f"bnpool/colsum/{C}", (COLSUM_PERIOD, C), std=1.0, mean=0.25)
    pre = ofill.fill(f"bnpool/colsum/pre/{C}", (C,), std=1.0, mean=3.0)
    counts = np.bincount(np.arange(rows) % COLSUM_PERIOD, minlength=COLSUM_PERIOD).astype(np.float64)
    ref = {"out": torch.from_numpy(pre.astype(np.float64) + (table.astype(np.float64) * counts[:, None]).sum(0))}
    x32 = colsum_matrix(torch.from_numpy(table), rows)
    got32 = {"out": torch.from_numpy(pre) + x32.sum(0)}
    specs = {"out": meas(f"colsum/{rows}", _amax(ref["out"]))}
    return {"table": table, "pre": pre, "ref": ref, "got32": got32, "specs": specs}


def colsum_matrix(table: torch.Tensor, rows):
    return table.repeat(-(-rows // COLSUM_PERIOD), 1)[:rows].contiguous()


# ------------------------------------------------------------------------------------------------ 7. eoe_maxpool, exact
PLAIN_GEOS = ((2, 2, 0, 6, 10), (3, 1, 1, 5, 7), (2, 3, 0, 8, 7), (3, 2, 0, 8, 6))
PLAIN_C = (4, 20)
PLAIN_N = 2


@functools.lru_cache(maxsize=None)
def plain_maxpool_case(gi, C):
    """x = relu of a grid fill (about half of it ties at 0); dout on the grid as well, so that the sum over the windows a pixel
    won is exact in fp32 in any order"""
    k, s, p, H, W = PLAIN_GEOS[gi]
    x = np.maximum(grid_fill(f"bnpool/plain/{gi}/{C}/x", (PLAIN_N, H, W, C), std=1.0), 0.0).astype(np.float32)
    Ho, Wo = out_hw(H, W, ("max", k, s, p))
    dout = grid_fill(f"bnpool/plain/{gi}/{C}/dout", (PLAIN_N, Ho, Wo, C), std=1.0)
    xt = _nchw(x, torch.float64).requires_grad_(True)
    out, ix = F.max_pool2d(xt, k, s, p, return_indices=True)
    (out * _nchw(dout, torch.float64)).sum().backward()
    ky = ix // W - (torch.arange(Ho).view(1, 1, Ho, 1) * s - p)
    kx = ix % W - (torch.arange(Wo).view(1, 1, 1, Wo) * s - p)
    return {"x": x, "dout": dout, "out": _nhwc(out).float(), "idx": _nhwc(ky * k + kx).to(torch.uint8), "dx": _nhwc(xt.grad).float()}


# ------------------------------------------------------------------------------------------------ 8. eoe_avgpool
AVGPOOL_CASES = ((1, 1, 16), (3, 49, 32), (2, 1000, 512))          # (n, HW, C)
AVGPOOL_REFUSED_C = (48, 8, 320)           # C / 4 = 12 does not divide 256; C % 16 != 0; C / 4 = 80 is no multiple of 64


@functools.lru_cache(maxsize=None)
def avgpool_case(n, HW, C):
    """x = relu of a grid fill: the maximum of a (image, channel) column ties, the first position wins (numpy's argmax)"""
    x = np.maximum(grid_fill(f"bnpool/avg/{n}x{HW}x{C}/x", (n, HW, C), std=1.0), 0.0).astype(np.float32)
    dout = ofill.fill(f"bnpool/avg/{n}x{HW}x{C}/dout", (n, C), std=1.0)
    ref = {"mean": torch.from_numpy(x.astype(np.float64).mean(1)), "max": torch.from_numpy(x.max(1)),
           "argmax": torch.from_numpy(x.argmax(1).astype(np.int32)),
           "dx": torch.from_numpy(np.broadcast_to(dout.astype(np.float64)[:, None, :] / HW, (n, HW, C)).copy())}
    return {"x": x, "dout": dout, "ref": ref, "specs": {"mean": tol(TOL_AVG_FWD), "dx": tol(TOL_AVG_BWD)}}


# ------------------------------------------------------------------------------------------------ 9. add + ReLU, exact
JUNCTION_GRID_CAP = 8192                   # workgroups of 256 threads, one quad each (cbam.hip grid_for)
JUNCTION_COUNTS = (4, 1028, JUNCTION_GRID_CAP * 256 * 4 + 4)          # the last: one quad past the grid cap


@functools.lru_cache(maxsize=None)
def junction_case(count):
    """a, b on the grid; b = -a on every third element (a + b == 0 exactly), both -0.0 on every 97th"""
    a = grid_fill(f"bnpool/junction/{count}/a", (count,), std=1.0)
    b = grid_fill(f"bnpool/junction/{count}/b", (count,), std=1.0)
    i = np.arange(count)
    b[i % 3 == 0] = -a[i % 3 == 0]
    a[i % 97 == 1] = -0.0
    b[i % 97 == 1] = -0.0
    dout = ofill.fill(f"bnpool/junction/{count}/dout", (count,), std=1.0)
    out = np.maximum(a + b, np.float32(0.0))
    return {"a": a, "b": b, "dout": dout, "out": torch.from_numpy(out), "g": torch.from_numpy(np.where(out > 0, dout, np.float32(0.0)))}


# ------------------------------------------------------------------------------------------------ the measurement
def all_measured_cases():
    """(what, ref, got32, specs) of every case that has a measured bound"""
    for M, C in STATS_CASES:
        c = stats_case(M, C)
        yield f"stats {M}x{C}", c["ref"], c["got32"], c["specs"]
    c = stats_case(*STATS_BIGMEAN, bigmean=True)
    yield "stats bigmean", c["ref"], c["got32"], c["specs"]
    for R in PARTIALS_R:
        for C in PARTIALS_C:
            c = partials_case(R, C)
            yield f"partials {R}x{C}", c["ref"], c["got32"], c["specs"]
    for a in bwd_cases():
        c = bwd_case(*a)
        yield f"bwd {a}", c["ref"], c["got32"], c["specs"]
    for rows in COLSUM_ROWS:
        for C in COLSUM_C:
            c = colsum_case(rows, C)
            yield f"colsum {rows}x{C}", c["ref"], c["got32"], c["specs"]


def measure() -> dict:
    table = {}
    for _, ref, got32, specs in all_measured_cases():
        measure_into(table, got32, ref, specs)
    return table


if __name__ == "__main__":
    for k, v in sorted(measure().items()):
        print(f'    "{k}": {v:.3e},    # {v / ULP32:.2f} ulp -> kernel bound {(K_KERNEL * v + FLOOR_ULPS * ULP32) / ULP32:.1f} ulp')
