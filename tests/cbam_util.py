"""Case tables, inputs, fp64 references and the tolerance table of the CBAM gate kernel tests (tests/test_gpu_cbam.py on the GPU,
tests/test_cpu_cbam.py without one): eoe_cgate_fwd / _bwd, eoe_sgate_fwd / _bwd and the fused unit eoe_cbam_junction_fwd / _bwd /
_bwd_data of csrc/cbam.hip.

References.  `autograd` runs oracle.models._ChannelGate / _SpatialGate (the two sub-modules of oracle.models._CBAM) under torch
autograd with explicit weights from oracle.fill: out, dx, g (= dres), the seven parameter gradients and the running buffers; the
fused unit is relu(SpatialGate(ChannelGate(x)) + res) of the same two modules.  `restate` writes the same unit out by hand, forward
and backward: it yields what the kernels save (pooled, argmax_c, hidden, scale, comp, argmax_p, z, mean / rstd, sp) and what the
fused backward keeps in scratch (the per-pixel record {sp, dcomp0, dcomp1}, datt, the dscale slices), and tests/test_cpu_cbam.py
holds it against `autograd` in fp64.  Both run in fp64 for the reference and in fp32 for the yardstick below.

Inputs.  x and res lie on the grid of multiples of 2^-6 (bnpool_util.grid_fill), |x| < 1.74; `plant` writes into x: a channel plane
that is all zero in image 0 (the whole plane ties: argmax_c 0), a channel of the last image whose maximum 4.0 occurs twice, at
pixels of different row lanes of chan_reduce_kernel, two pixels whose channels are all 0 (argmax_p 0, for the fused unit too: 0 * sc
ties as well) and a pixel whose maximum 4.0 sits in channels 2, 6, 66 and C - 1 (other 16-lane sub-lanes, and the same sub-lane's
next round).  tests/test_cpu_cbam.py asserts per case that fp32 picks the argmax_c, argmax_p, hidden > 0 and out > 0 that fp64 picks:
zero disagreements, nothing is excluded from any comparison.

Tolerance rule (that of tests/bnpool_util.py).  Reused where an older test fixes one: TOL_* below.  A 16-bit copy equals the kernel's
own fp32 output cast, bit for bit.  Everything else -- every saved intermediate, and the parameter gradients of the cases older tests
do not reach (n > 5, HW > 196 or C > 512: sums over 3136 pixels, 300 images, 2.1 M pixels, 4096 channels) -- is held against the
fp32-CPU evaluation of the same formulas: its distance to fp64 over the quantity's natural scale (for a sum: the sum of the absolute
values of its terms, propagated through the formulas that follow), the largest ratio per regime in REF_ERR32.  A kernel may be
K_KERNEL = 4 times as far away plus FLOOR_ULPS fp32 ulps of the scale.  Nothing is measured against a kernel."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill as ofill, models as omodels
from bnpool_util import (DTYPES, FLOOR_ULPS, FLT_MIN, K_KERNEL, ULP32, _np64, _t, grid_fill, meas, measure_into, round16,      # noqa: F401
                         tol)

EPS_BN = 1e-5                              # oracle.models._BasicConv: BatchNorm2d(1, eps 1e-5, momentum 0.01)
MOMENTUM = 0.01
GAMMA, BETA = 0.7, -0.1                    # test_gpu_resnet.test_cbam_vs_oracle_shapes
RM0, RV0, NBT0 = 0.3, 1.7, 41              # the running buffers before the call
BIG = 4.0                                  # the planted maximum
SLICES = 8                                 # EOE_CBAM_DSCALE_SLICES

# ------------------------------------------------------------------------------------------------ reused tolerances
TOL_Y = (1e-4, 1e-5)                       # test_gpu_resnet.test_cbam_vs_oracle_shapes: "y"
TOL_DX = (1e-3, 1e-4)                      # ... "dx"
TOL_PGRAD = 2e-4                           # ... rel_rms of every parameter gradient
TOL_EXACT = (0.0, 0.0)                     # g = dout * [out > 0]; the max planes of x

PARAM_GRADS = ("dw1", "db1", "dw2", "db2", "dw", "dgamma", "dbeta")
SAVED = ("pooled", "hidden", "scale", "comp", "z", "mean", "rstd", "rmean", "rvar", "sp", "record", "datt", "slices")

# ------------------------------------------------------------------------------------------------ measured reference errors
# key -> largest |fp32-CPU value - fp64 value| / scale over every case of the regime ("small": n <= 5, HW <= 196, C <= 512, what the
# older tests reach; "big": the rest).  The comment holds the figure `python tests/cbam_util.py` printed and the resulting kernel
# bound K_KERNEL * value + FLOOR_ULPS * ULP32, both in units of the scale.  Measured on the CPU only.
REF_ERR32 = {
    "big/comp":       1.5e-07,        # measured 1.439e-07 (1.21 ulp) -> kernel bound 9.0 ulp of the scale
    "big/datt":       8.9e-06,        # measured 8.863e-06 (74.35 ulp) -> kernel bound 302.6 ulp of the scale
    "big/db1":        2.3e-08,        # measured 2.235e-08 (0.19 ulp) -> kernel bound 4.8 ulp of the scale
    "big/db2":        1.8e-06,        # measured 1.776e-06 (14.89 ulp) -> kernel bound 64.4 ulp of the scale
    "big/dbeta":      1.2e-08,        # measured 1.156e-08 (0.10 ulp) -> kernel bound 4.4 ulp of the scale
    "big/dgamma":     2.5e-08,        # measured 2.461e-08 (0.21 ulp) -> kernel bound 4.8 ulp of the scale
    "big/dw":         9.4e-08,        # measured 9.368e-08 (0.79 ulp) -> kernel bound 7.2 ulp of the scale
    "big/dw1":        2.3e-08,        # measured 2.252e-08 (0.19 ulp) -> kernel bound 4.8 ulp of the scale
    "big/dw2":        7.2e-06,        # measured 7.127e-06 (59.78 ulp) -> kernel bound 245.6 ulp of the scale
    "big/hidden":     1.7e-07,        # measured 1.667e-07 (1.40 ulp) -> kernel bound 9.7 ulp of the scale
    "big/mean":       5.7e-08,        # measured 5.674e-08 (0.48 ulp) -> kernel bound 5.9 ulp of the scale
    "big/pooled":     4.1e-08,        # measured 4.015e-08 (0.34 ulp) -> kernel bound 5.4 ulp of the scale
    "big/record":     5.5e-07,        # measured 5.476e-07 (4.59 ulp) -> kernel bound 22.5 ulp of the scale
    "big/rmean":      7.6e-08,        # measured 7.503e-08 (0.63 ulp) -> kernel bound 6.6 ulp of the scale
    "big/rstd":       7.6e-08,        # measured 7.519e-08 (0.63 ulp) -> kernel bound 6.6 ulp of the scale
    "big/rvar":       5.7e-08,        # measured 5.670e-08 (0.48 ulp) -> kernel bound 5.9 ulp of the scale
    "big/scale":      2.1e-07,        # measured 2.016e-07 (1.69 ulp) -> kernel bound 11.0 ulp of the scale
    "big/slices":     2.1e-07,        # measured 2.075e-07 (1.74 ulp) -> kernel bound 11.0 ulp of the scale
    "big/sp":         5.5e-07,        # measured 5.476e-07 (4.59 ulp) -> kernel bound 22.5 ulp of the scale
    "big/z":          2.2e-07,        # measured 2.136e-07 (1.79 ulp) -> kernel bound 11.4 ulp of the scale
    "small/comp":     1.1e-07,        # measured 1.030e-07 (0.86 ulp) -> kernel bound 7.7 ulp of the scale
    "small/datt":     9.0e-06,        # measured 8.952e-06 (75.10 ulp) -> kernel bound 306.0 ulp of the scale
    "small/hidden":   5.7e-08,        # measured 5.667e-08 (0.48 ulp) -> kernel bound 5.9 ulp of the scale
    "small/mean":     5.4e-08,        # measured 5.337e-08 (0.45 ulp) -> kernel bound 5.8 ulp of the scale
    "small/pooled":   4.0e-08,        # measured 3.953e-08 (0.33 ulp) -> kernel bound 5.3 ulp of the scale
    "small/record":   3.5e-07,        # measured 3.461e-07 (2.90 ulp) -> kernel bound 15.7 ulp of the scale
    "small/rmean":    6.9e-08,        # measured 6.804e-08 (0.57 ulp) -> kernel bound 6.3 ulp of the scale
    "small/rstd":     1.1e-07,        # measured 1.042e-07 (0.87 ulp) -> kernel bound 7.7 ulp of the scale
    "small/rvar":     4.3e-08,        # measured 4.258e-08 (0.36 ulp) -> kernel bound 5.4 ulp of the scale
    "small/scale":    2.0e-07,        # measured 1.977e-07 (1.66 ulp) -> kernel bound 10.7 ulp of the scale
    "small/slices":   4.4e-07,        # measured 4.347e-07 (3.65 ulp) -> kernel bound 18.8 ulp of the scale
    "small/sp":       3.5e-07,        # measured 3.461e-07 (2.90 ulp) -> kernel bound 15.7 ulp of the scale
    "small/z":        1.4e-07,        # measured 1.309e-07 (1.10 ulp) -> kernel bound 8.7 ulp of the scale
}


def bound_factor(key):
    return K_KERNEL * REF_ERR32[key] + FLOOR_ULPS * ULP32


def rel_rms(got, ref):                     # gpu_util.rel_rms
    g, r = _np64(got), _np64(ref)
    return float(np.sqrt(np.mean((g - r) ** 2)) / (np.sqrt(np.mean(r ** 2)) + 1e-30))


def rms(r):
    return ("rms", r)


def deviation(got, ref, spec):
    """bnpool_util.deviation over this file's REF_ERR32, plus ("rms", r): rel_rms(got, ref) <= r"""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if not np.isfinite(g).all():
        return float("inf"), "non-finite values in the result"
    if spec[0] == "rms":
        v = rel_rms(g, r)
        return v / spec[1], f"rel rms {v:.3e} (allowed {spec[1]:.1e})"
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
    """assert every quantity of `names` (or of `got`) against the fp64 reference; prints each figure before it asserts"""
    bad = []
    for name in (names or got):
        ratio, msg = deviation(got[name], ref[name], specs[name])
        if verbose:
            print(f"[{what}] {name}: {msg}")
        if not ratio <= 1.0:
            bad.append(f"{name}: {msg}")
    assert not bad, f"{what}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ launch arithmetic, restated
def chan_cpb(C):
    return C // 4 if C // 4 < 64 else 64


def cgate_accepts(C, Ch):
    """check_cgate of csrc/cbam.hip"""
    if not (C >= 16 and C % 16 == 0 and C <= 4096 and 1 <= Ch <= 256):
        return False
    cpb = chan_cpb(C)
    return 256 % cpb == 0 and (C // 4) % cpb == 0


def junction_nz(n, HW, C):
    """the slices eoe_cbam_junction_bwd cuts an image's pixels into (the launcher's two-line rule)"""
    nz = 1
    while nz < SLICES and n * (C // 4 // chan_cpb(C)) * nz < 1024 and HW // (nz * 2) >= 64:
        nz *= 2
    return nz


def sgate_bwd_accepts(H, W):
    return (H + 6) * (W + 6) <= 8192


def plane_exceeds_stage(H, W):
    """sgate_conv_bwd_weight_kernel: the padded plane [(H+6)(W+6)][2] against the [256][49] + [4][49] stage"""
    return (H + 6) * (W + 6) * 2 > (256 + 4) * 49


# ------------------------------------------------------------------------------------------------ case tables
# channel gate (n, H, W, C, Ch): HW = 1 | C = 16, Ch = 1 | C = 32 | HW = 63 / 64 / 65 around rpb = 64 | HW = 127 / 128 / 129 around
# U * rpb = 128 of the C = 64 pooling | HW = 3 < rpb = 4 | odd Ch | C = 4096, Ch = 256 | n = 17 | n = 70
CGATE_CASES = ((1, 1, 1, 16, 1), (2, 3, 5, 16, 1), (3, 7, 9, 32, 2), (2, 1, 63, 16, 1), (2, 1, 64, 16, 1), (2, 1, 65, 16, 1),
               (2, 1, 127, 64, 4), (2, 8, 16, 64, 4), (2, 3, 43, 64, 4), (2, 1, 3, 256, 16), (2, 5, 7, 256, 3), (1, 2, 2, 4096, 256),
               (17, 3, 3, 64, 4), (70, 2, 2, 128, 8))
CGATE_REFUSED_C = (8, 48, 80, 96, 320, 4112)
CGATE_REFUSED_CH = (0, 257)
# spatial gate (n, H, W, C): one pixel | W > 7 > H | C no multiple of 64 | the window exactly | H > 7 > W, three rounds of a sub-lane
SGATE_SMALL = ((1, 1, 1, 4), (2, 3, 11, 4), (2, 6, 6, 68), (3, 7, 7, 64), (1, 13, 4, 132))
# (H+6)(W+6) = 8192 exactly | plane larger than stage | either side of plane = stage | n > 64 | P = 2 116 800: a second grid-stride
# round in every pixel, conv, sigmoid and elementwise kernel, all 512 BatchNorm-backward partials
SGATE_LARGE = ((2, 58, 122, 4), (1, 84, 84, 8), (1, 74, 74, 4), (1, 73, 74, 4), (70, 9, 5, 16), (300, 84, 84, 4))
SGATE_REFUSED_BWD = (1, 58, 123, 4)
# fused unit (n, H, W, C, Ch) -> nz by junction_nz: 1 | 1 | 2 | 8, per 64 | 8, per 128 | 8, short last slice (1023 = 7 * 128 + 127) |
# 8, per 392: the network's own map | 2 | 1, C = 512 | 8, P = 141 120 > 131 072 || added to the issue's table, which by the launcher's
# rule reaches nz 1, 2 and 8 only: 4, per 64 | 4 because n * nz reaches 1024 (HW alone would give 8)
FUSED_CASES = ((2, 3, 5, 16, 1), (3, 7, 7, 64, 4), (2, 8, 16, 64, 4), (2, 16, 32, 64, 4), (2, 32, 32, 64, 4), (2, 31, 33, 64, 4),
               (1, 56, 56, 64, 4), (300, 8, 16, 64, 4), (2, 5, 5, 512, 32), (45, 56, 56, 16, 1),
               (2, 16, 16, 64, 4), (300, 16, 32, 16, 1))
FUSED_EVAL = ((2, 3, 5, 16, 1), (3, 7, 7, 64, 4), (2, 31, 33, 64, 4))          # these run over the running statistics as well
FUSED_DATA_ONLY = (1, 58, 123, 16, 1)      # the full backward refuses it


# seed names: a case whose fp32 and fp64 evaluations disagree on a winner or a ReLU mask gets another name until they agree
SEEDS = {("fused", 300, 16, 32, 16, 1): "/b"}


def regime(n, HW, C):
    return "small" if n <= 5 and HW <= 196 and C <= 512 else "big"


# ------------------------------------------------------------------------------------------------ inputs
def plant(x, C):
    """the ties (module docstring), in place on x [n, HW, C]; skipped where the map has no room"""
    n, HW, _ = x.shape
    rpb = 256 // chan_cpb(C) if C >= 16 else 64
    if HW >= 4:
        x[n - 1, 0, :] = 0.0
        x[n - 1, HW - 1, :] = 0.0
    if HW >= 3:
        x[n - 1, 1, 1] = x[n - 1, rpb if HW > rpb else 2, 1] = BIG
    hw = HW // 2
    for ch in (2, 6, 66, C - 1):
        if ch < C and 0 < hw < HW - 1:
            x[0, hw, ch] = BIG
    x[0, :, 0] = 0.0


def weights(tag, C, Ch, affine):
    """fp32 arrays; the MLP and the 7 x 7 conv at fan-in scale (the gates stay away from saturation)"""
    w = {"w": ofill.fill(f"cbam/{tag}/w", (1, 2, 7, 7), std=2.0 / np.sqrt(98.0)),
         "gamma": np.float32([GAMMA]) if affine else None, "beta": np.float32([BETA]) if affine else None}
    if Ch:
        w.update(w1=ofill.fill(f"cbam/{tag}/w1", (Ch, C), std=1.0 / np.sqrt(C)), b1=ofill.fill(f"cbam/{tag}/b1", (Ch,), std=0.1, mean=0.1),
                 w2=ofill.fill(f"cbam/{tag}/w2", (C, Ch), std=1.0 / np.sqrt(Ch)), b2=ofill.fill(f"cbam/{tag}/b2", (C,), std=0.1))
    return w


def modules(c, dt):
    """(ChannelGate or None, SpatialGate or None) of oracle.models, loaded with the case's weights and running buffers"""
    cg = sg = None
    w = c["w"]
    with torch.no_grad():
        if c["part"] != "sgate":
            cg = omodels._ChannelGate(c["C"], c["C"] // c["Ch"]).to(dt)
            assert tuple(cg.mlp[0].weight.shape) == (c["Ch"], c["C"])
            for p, k in ((cg.mlp[0].weight, "w1"), (cg.mlp[0].bias, "b1"), (cg.mlp[1].weight, "w2"), (cg.mlp[1].bias, "b2")):
                p.copy_(_t(w[k], dt))
        if c["part"] != "cgate":
            sg = omodels._SpatialGate().to(dt)
            bn = sg.spatial.bn
            sg.spatial.conv.weight.copy_(_t(w["w"], dt))
            if c["affine"]:
                bn.weight.copy_(_t(w["gamma"], dt))
                bn.bias.copy_(_t(w["beta"], dt))
            else:
                bn.weight = bn.bias = None
            bn.running_mean.fill_(float(np.float32(RM0)))
            bn.running_var.fill_(float(np.float32(RV0)))
            bn.num_batches_tracked.fill_(NBT0)
            sg.train(c["training"])
    return cg, sg


def _nchw(a, c, dt):
    return _t(a, dt).reshape(c["n"], c["H"], c["W"], c["C"]).permute(0, 3, 1, 2).contiguous()


def _flat(t, c):
    return t.detach().permute(0, 2, 3, 1).reshape(c["n"], c["H"] * c["W"], c["C"])


def autograd(c, dt):
    """the oracle modules under torch autograd in dtype dt"""
    cg, sg = modules(c, dt)
    x = _nchw(c["x"], c, dt).requires_grad_(True)
    y = x if cg is None else cg(x)
    y = y if sg is None else sg(y)
    r = None
    if c["res"] is not None:
        r = _nchw(c["res"], c, dt).requires_grad_(True)
        y = torch.relu(y + r)
    (y * _nchw(c["dout"], c, dt)).sum().backward()
    o = {"out": _flat(y, c), "dx": _flat(x.grad, c)}
    if r is not None:
        o["g"] = _flat(r.grad, c)
    if cg is not None:
        o.update(dw1=cg.mlp[0].weight.grad, db1=cg.mlp[0].bias.grad, dw2=cg.mlp[1].weight.grad, db2=cg.mlp[1].bias.grad)
    if sg is not None:
        bn = sg.spatial.bn
        o.update(dw=sg.spatial.conv.weight.grad.reshape(98), rmean=bn.running_mean.detach().clone(), rvar=bn.running_var.detach().clone(),
                 nbt=int(bn.num_batches_tracked))
        if c["affine"]:
            o.update(dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    return o


def first_argmax(v, dim):
    """index of the first maximum along dim (int32): what the kernels promise"""
    size = v.shape[dim]
    idx = torch.arange(size).view([size if d == dim else 1 for d in range(v.dim())])
    return torch.where(v == v.amax(dim, keepdim=True), idx, size).amin(dim).to(torch.int32)


@torch.no_grad()
def restate(c, dt, scales=False):
    """the unit written out by hand in dtype dt, forward and backward ([n, HW, C] layout).  With `scales`, o['scales'][name] holds the
    natural scale of each measured quantity: for a sum the sum of its terms' absolute values, carried through what follows it"""
    n, H, W, C, Ch = c["n"], c["H"], c["W"], c["C"], c["Ch"]
    HW = H * W
    use_c, use_s = c["part"] != "sgate", c["part"] != "cgate"
    w = {k: None if v is None else _t(v, dt) for k, v in c["w"].items()}
    x, dout = _t(c["x"], dt), _t(c["dout"], dt)
    o, S = {}, {}
    xc = x
    if use_c:
        pooled = torch.stack([x.mean(1), x.amax(1)], 1)                                   # [n, 2, C]
        am_c = first_argmax(x, 1)
        hidden = torch.relu(pooled @ w["w1"].t() + w["b1"])                               # [n, 2, Ch]
        hs = hidden[:, 0] + hidden[:, 1]
        sc = torch.sigmoid(hs @ w["w2"].t() + 2 * w["b2"])                                # [n, C]
        xc = x * sc[:, None, :]
        o.update(pooled=pooled, argmax_c=am_c, hidden=hidden, scale=sc)
        S["pooled"] = torch.stack([x.abs().mean(1), torch.zeros(n, C, dtype=dt)], 1)      # the max plane of x: exact
        S["hidden"] = pooled.abs() @ w["w1"].abs().t() + w["b1"].abs()
        S["scale"] = sc + 0.25 * (hs @ w["w2"].abs().t() + 2 * w["b2"].abs())
    y = xc
    if use_s:
        comp = torch.stack([xc.amax(2), xc.mean(2)], 2)                                   # [n, HW, 2]
        am_p = first_argmax(xc, 2)
        cimg = comp.reshape(n, H, W, 2).permute(0, 3, 1, 2)
        z = F.conv2d(cimg, w["w"], padding=3)[:, 0]                                       # [n, H, W]
        if c["training"]:
            mu = z.mean()
            var = ((z - mu) ** 2).mean()
            cnt = z.numel()
            o.update(rmean=(1 - MOMENTUM) * float(np.float32(RM0)) + MOMENTUM * mu,
                     rvar=(1 - MOMENTUM) * float(np.float32(RV0)) + MOMENTUM * var * (cnt / max(cnt - 1, 1)))
        else:
            mu, var = torch.tensor(float(np.float32(RM0)), dtype=dt), torch.tensor(float(np.float32(RV0)), dtype=dt)
            o.update(rmean=mu.clone(), rvar=var.clone())
        rstd = 1.0 / torch.sqrt(var + EPS_BN)
        ga = w["gamma"][0] if c["affine"] else torch.tensor(1.0, dtype=dt)
        be = w["beta"][0] if c["affine"] else torch.tensor(0.0, dtype=dt)
        xh = ((z - mu) * rstd).reshape(n, HW)
        sp = torch.sigmoid(xh * ga + be)                                                  # [n, HW]
        y = xc * sp[..., None]
        o.update(comp=comp, argmax_p=am_p, z=z.reshape(n, HW), mean=mu, rstd=rstd, sp=sp)
        S["comp"] = comp.abs().amax() if use_c else torch.stack([torch.zeros(n, HW, dtype=dt), x.abs().mean(2)], 2)
        S["z"] = F.conv2d(cimg.abs(), w["w"].abs(), padding=3)[:, 0].reshape(n, HW)
        S["mean"] = 1.0 / rstd + mu.abs()                                                 # as bnpool_util.stats_specs
        S["rstd"], S["rvar"] = rstd, o["rvar"]
        S["rmean"] = torch.maximum(o["rmean"].abs(), MOMENTUM * S["mean"])
        S["sp"] = torch.tensor(1.0, dtype=dt)
    has_res = c["res"] is not None
    out = torch.relu(y + _t(c["res"], dt)) if has_res else y
    g = dout * (out > 0) if has_res else dout
    o["out"] = out
    if has_res:
        o["g"] = g
    dxc = g
    if use_s:
        dsp = (g * xc).sum(2)
        gs = dsp * sp * (1 - sp)
        o.update(dbeta=gs.sum().reshape(1), dgamma=(gs * xh).sum().reshape(1))
        m0, m1 = gs.mean(), (gs * xh).mean()
        dz = ga * rstd * (gs - m0 - xh * m1) if c["training"] else ga * rstd * gs
        dzs = ga.abs() * rstd * ((gs.abs() + m0.abs() + (xh * m1).abs()) if c["training"] else gs.abs())
        dzi, dzsi = dz.reshape(n, 1, H, W), dzs.reshape(n, 1, H, W)
        dcomp = F.conv_transpose2d(dzi, w["w"], padding=3).permute(0, 2, 3, 1).reshape(n, HW, 2)
        o["dw"] = torch.nn.grad.conv2d_weight(cimg.contiguous(), (1, 2, 7, 7), dzi, padding=3).reshape(98)
        o["record"] = torch.cat([sp[..., None], dcomp], 2)                                # [n, HW, 3]
        dxc = g * sp[..., None] + (torch.arange(C) == am_p[..., None]) * dcomp[..., 0:1] + dcomp[..., 1:2] / C
        S["dgamma"], S["dbeta"] = (gs * xh).abs().sum(), gs.abs().sum()
        S["dw"] = torch.nn.grad.conv2d_weight(cimg.abs().contiguous(), (1, 2, 7, 7), dzsi, padding=3).reshape(98)
        sdc = F.conv_transpose2d(dzsi, w["w"].abs(), padding=3).permute(0, 2, 3, 1).reshape(n, HW, 2)
        S["record"] = torch.cat([torch.ones(n, HW, 1, dtype=dt), sdc], 2)
    dx = dxc
    if use_c:
        t = dxc * x
        if c["part"] == "fused":
            nz = junction_nz(n, HW, C)
            per = -(-HW // nz)
            o["slices"] = torch.stack([t[:, k * per:min(HW, (k + 1) * per)].sum(1) for k in range(nz)])          # [nz, n, C]
            S["slices"] = torch.stack([t[:, k * per:min(HW, (k + 1) * per)].abs().sum(1) for k in range(nz)])
        s1 = sc * (1 - sc)
        datt, datts = t.sum(1) * s1, t.abs().sum(1) * s1
        on = (hidden > 0).to(dt)
        dhidden, dhiddens = (datt @ w["w2"])[:, None, :] * on, (datts @ w["w2"].abs())[:, None, :] * on
        dpooled = dhidden @ w["w1"]
        o.update(datt=datt, dw1=torch.einsum("nkj,nkc->jc", dhidden, pooled), db1=dhidden.sum((0, 1)), dw2=datt.t() @ hs, db2=2 * datt.sum(0))
        S.update(datt=datts, dw1=torch.einsum("nkj,nkc->jc", dhiddens, pooled.abs()), db1=dhiddens.sum((0, 1)), dw2=datts.t() @ hs,
                 db2=2 * datts.sum(0))
        dx = dxc * sc[:, None, :] + dpooled[:, 0][:, None, :] / HW + (torch.arange(HW)[None, :, None] == am_c[:, None, :]) * dpooled[:, 1][:, None, :]
    o["dx"] = dx
    if scales:
        o["scales"] = S
    return o


def case_specs(c):
    """name -> spec of everything a test may compare"""
    r, S = c["regime"], c["ref"]["scales"]
    s = {"out": tol(TOL_Y), "dx": tol(TOL_DX), "g": tol(TOL_EXACT)}
    for k in PARAM_GRADS:
        if k in c["ref"]:
            s[k] = rms(TOL_PGRAD) if r == "small" else meas(f"big/{k}", S[k])
    for k in SAVED:
        if k in S:
            s[k] = meas(f"{r}/{k}", S[k])
    return s


@functools.lru_cache(maxsize=None)
def case(part, n, H, W, C, Ch=0, training=True, affine=True, res=True, seed=""):
    """inputs (numpy fp32), the fp64 reference, the fp32-CPU evaluation and the specs of one case; part: 'cgate' | 'sgate' | 'fused'
    (the channel gate takes no res; the fused unit always does)"""
    tag = f"{part}/{n}x{H}x{W}x{C}x{Ch}{seed}{SEEDS.get((part, n, H, W, C, Ch), '')}"
    HW = H * W
    x = grid_fill(f"cbam/{tag}/x", (n, HW, C), std=1.0)
    plant(x, C)
    c = {"part": part, "n": n, "H": H, "W": W, "C": C, "Ch": Ch, "training": training, "affine": affine, "x": x,
         "res": grid_fill(f"cbam/{tag}/res", (n, HW, C), std=1.0) if res else None,
         "dout": ofill.fill(f"cbam/{tag}/dout", (n, HW, C), std=1.0), "w": weights(tag, C, Ch, affine), "regime": regime(n, HW, C),
         "nz": junction_nz(n, HW, C) if part == "fused" else None}
    c["ref"] = {**restate(c, torch.float64, scales=True), **autograd(c, torch.float64)}
    c["got32"] = {**restate(c, torch.float32), **autograd(c, torch.float32)}
    c["specs"] = case_specs(c)
    return c


def sgate_options(shape):
    """(training, affine) sets of a spatial-gate shape: all four on the small ones"""
    return ((True, True), (False, True), (True, False), (False, False)) if shape in SGATE_SMALL else ((True, True),)


def all_cases(heavy=True):
    """(what, case) of every case of the tables; heavy = False leaves out those above a million elements"""
    def light(n, H, W, C):
        return heavy or n * H * W * C <= 1 << 20
    for a in CGATE_CASES:
        yield f"cgate {a}", case("cgate", *a, res=False)
    for a in SGATE_SMALL + SGATE_LARGE:
        if light(*a):
            for training, affine in sgate_options(a):
                for res in (True, False):
                    yield f"sgate {a} train={training} affine={affine} res={res}", case("sgate", *a, 0, training, affine, res)
    for a in FUSED_CASES + (FUSED_DATA_ONLY,):
        if light(*a[:4]):
            for training in (True, False) if a in FUSED_EVAL or a == FUSED_DATA_ONLY else (True,):
                yield f"fused {a} train={training}", case("fused", *a, training)
    a = FUSED_CASES[1]
    yield f"fused {a} affine=False", case("fused", *a, True, False)


def measure() -> dict:
    table = {}
    for _, c in all_cases():
        measure_into(table, c["got32"], c["ref"], c["specs"])
    return table


if __name__ == "__main__":
    for k, v in sorted(measure().items()):
        print(f'    "{k}": {v:.3e},    # {v / ULP32:.2f} ulp -> kernel bound {(K_KERNEL * v + FLOOR_ULPS * ULP32) / ULP32:.1f} ulp')
