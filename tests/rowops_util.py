"""Case tables, fp64 references and the tolerance table of the row-kernel tests (tests/test_gpu_rowops.py on the GPU,
tests/test_cpu_rowops.py without one): LayerNorm forward / backward, embed + ln_pre, and the six objective heads.

Inputs are pure functions of a name (oracle.fill).  Every reference is oracle.models.layer_norm / oracle.objectives.* evaluated
in fp64 on the same fp32 (or 16-bit-rounded) inputs.

Tolerance rule.  Where an older test already fixes a tolerance for a quantity it is reused (TOL_* below, each with its source).
For the regimes no older test reaches -- column sums over thousands of rows, LayerNorm around a large mean, LayerNorm row
statistics, HSC at small norms and at d = 1, DSAD next to the origin, saturated BCE / focal logits -- the yardstick is the
reference formula itself: the oracle's function evaluated in fp32 torch on the CPU, its distance to the fp64 value divided by the
quantity's natural scale, the largest such ratio over all cases of the regime (REF_ERR32, measured by `python tests/rowops_util.py`
and asserted by tests/test_cpu_rowops.py).  A kernel may be K_KERNEL = 4 times as far away (it sums in another order, wave tree
against sequential, and may contract to FMA), plus FLOOR_ULPS fp32 ulps of that scale, plus FLT_MIN (below the smallest normal
number fp32 has no relative precision and a kernel may flush)."""
import functools
import math

import numpy as np
import torch

from oracle import fill as ofill, models as omodels, objectives as oobj

ULP32 = 2.0 ** -23
FLT_MIN = 2.0 ** -126
K_KERNEL = 4.0
FLOOR_ULPS = 4.0
EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # tests/gpu_util.py
DTYPES = (torch.bfloat16, torch.float16)

# ------------------------------------------------------------------------------------------------ reused tolerances (rtol, atol)
TOL_LN_Y32 = (1e-5, 1e-5)                  # test_gpu_ops.test_layernorm: "layernorm fwd f32"
TOL_LN_DX = (1e-4, 1e-4)                   # ... "layernorm bwd dx"


def tol_ln_y16(dtype):                     # ... "layernorm fwd 16-bit"
    return (2 * EPS16[dtype], 1e-5)


def tol_ln_dx16(dtype):                    # ... "layernorm bwd dx16"
    return (2 * EPS16[dtype], 1e-4)


def tol_ln_colsum(rows):                   # ... "layernorm bwd dgamma / dbeta / column sums of dx"
    return (1e-4, 1e-4 * math.sqrt(rows))


TOL_HSC_GRAD = (1e-5, 1e-9)                # test_gpu_ops.test_hsc_bce: hsc and bce gradients
TOL_HSC_SCORE = (1e-5, 1e-7)               # ... hsc and bce scores
TOL_LOSS_REL = 2e-6                        # ... |loss - ref| <= 2e-6 max(1, |ref|)  (hsc, bce)
TOL_N4_LOSS_REL = 2e-5                     # test_other_objectives_n4_vs_golden: dsad / dsvdd / focal loss, relative
# the gradient tolerances of that test are absolute at its weights (n = 16, upstream 1); a row's gradient is proportional to
# inv_count x upstream, so the absolute part is restated per unit of that weight (x 16)
TOL_DSAD_GRAD = (2e-4, 1e-6 * 16)
TOL_DSVDD_GRAD = (1e-5, 1e-7 * 16)
TOL_DSVDD_SCORE = (1e-5, 0.0)
TOL_FOCAL_GRAD = (5e-4, 1e-7 * 16)
TOL_FOCAL_SCORE = (1e-5, 0.0)
# test_clip_objective_n2_vs_golden_and_oracle, oracle part (n = 301, upstream 3): loss 1e-4 absolute, gradient (5e-4, 1e-6) -> per
# unit of inv_count x upstream 1e-6 * 301 / 3 = 1e-4; score (2e-4, 2e-6)
TOL_CLIP_LOSS_ABS = 1e-4
TOL_CLIP_GRAD = (5e-4, 1e-4)
TOL_CLIP_SCORE = (2e-4, 2e-6)

# ------------------------------------------------------------------------------------------------ measured reference errors
# key -> largest |fp32-CPU value - fp64 value| / scale over every case of the regime (the scale is named with each spec below).
# The comment holds the figure `python tests/rowops_util.py` printed and the resulting kernel bound K_KERNEL * value + FLOOR_ULPS
# * ULP32, both in units of the scale.
REF_ERR32 = {
    "bce/grad": 1.7e-07,                          # measured 1.647e-07 (1.38 ulp) -> kernel bound 9.7 ulp of the scale
    "bce/rows": 4.4e-08,                          # measured 4.389e-08 (0.37 ulp) -> kernel bound 5.5 ulp of the scale
    "dsad/grad": 2.3e-07,                         # measured 2.256e-07 (1.89 ulp) -> kernel bound 11.7 ulp of the scale
    "dsad/rows": 9.6e-08,                         # measured 9.509e-08 (0.80 ulp) -> kernel bound 7.2 ulp of the scale
    "elem/score0": 6.8e-08,                       # measured 6.791e-08 (0.57 ulp) -> kernel bound 6.3 ulp of the scale
    "elem/score1": 4.2e-08,                       # measured 4.140e-08 (0.35 ulp) -> kernel bound 5.4 ulp of the scale
    "focal/grad": 2.3e-07,                        # measured 2.282e-07 (1.91 ulp) -> kernel bound 11.7 ulp of the scale
    "focal/rows": 7.2e-08,                        # measured 7.124e-08 (0.60 ulp) -> kernel bound 6.4 ulp of the scale
    "hsc/dist": 8.9e-08,                          # measured 8.852e-08 (0.74 ulp) -> kernel bound 7.0 ulp of the scale
    "hsc/grad": 1.6e-07,                          # measured 1.555e-07 (1.30 ulp) -> kernel bound 9.4 ulp of the scale
    "hsc/rows": 9.3e-08,                          # measured 9.290e-08 (0.78 ulp) -> kernel bound 7.1 ulp of the scale
    "hsc/score": 9.7e-08,                         # measured 9.651e-08 (0.81 ulp) -> kernel bound 7.3 ulp of the scale
    "ln/mean": 4.8e-08,                           # measured 4.760e-08 (0.40 ulp) -> kernel bound 5.6 ulp of the scale
    "ln/rstd": 1.7e-07,                           # measured 1.636e-07 (1.37 ulp) -> kernel bound 9.7 ulp of the scale
    "ln_bigmean/dbeta": 3.5e-08,                  # measured 3.461e-08 (0.29 ulp) -> kernel bound 5.2 ulp of the scale
    "ln_bigmean/dgamma": 1.8e-06,                 # measured 1.730e-06 (14.51 ulp) -> kernel bound 64.4 ulp of the scale
    "ln_bigmean/dx": 3.3e-07,                     # measured 3.291e-07 (2.76 ulp) -> kernel bound 15.1 ulp of the scale
    "ln_bigmean/dxsum": 1.6e-07,                  # measured 1.520e-07 (1.28 ulp) -> kernel bound 9.4 ulp of the scale
    "ln_bigmean/mean": 1.5e-07,                   # measured 1.427e-07 (1.20 ulp) -> kernel bound 9.0 ulp of the scale
    "ln_bigmean/rstd": 1.3e-07,                   # measured 1.239e-07 (1.04 ulp) -> kernel bound 8.4 ulp of the scale
    "ln_bigmean/y": 2.5e-06,                      # measured 2.473e-06 (20.75 ulp) -> kernel bound 87.9 ulp of the scale
    "ln_many/4100x1024/dbeta": 1.3e-07,           # measured 1.242e-07 (1.04 ulp) -> kernel bound 8.4 ulp of the scale
    "ln_many/4100x1024/dgamma": 2.3e-07,          # measured 2.229e-07 (1.87 ulp) -> kernel bound 11.7 ulp of the scale
    "ln_many/4100x1024/dxsum": 2.3e-07,           # measured 2.270e-07 (1.90 ulp) -> kernel bound 11.7 ulp of the scale
    "ln_many/9000x256/dbeta": 1.8e-07,            # measured 1.771e-07 (1.49 ulp) -> kernel bound 10.0 ulp of the scale
    "ln_many/9000x256/dgamma": 2.0e-07,           # measured 1.921e-07 (1.61 ulp) -> kernel bound 10.7 ulp of the scale
    "ln_many/9000x256/dxsum": 1.8e-07,            # measured 1.728e-07 (1.45 ulp) -> kernel bound 10.0 ulp of the scale
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
    """assert every quantity of `specs` (or of `names`) against the fp64 reference; prints each figure before it asserts"""
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
            err = np.maximum(err - FLT_MIN, 0.0)                      # what the bound grants below the smallest normal number
            ratio = np.where(scale > 0, err / scale, np.where(err == 0, 0.0, np.inf))
        table[spec[1]] = max(table.get(spec[1], 0.0), float(ratio.max()))


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def round16(a: np.ndarray, dtype) -> np.ndarray:
    """fp32 array holding values already rounded to the 16-bit dtype (None: left alone)"""
    return a if dtype is None else torch.from_numpy(a).to(dtype).float().numpy()


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_MANY = ((9000, 256), (4100, 1024))          # several rows per wave: grid 512 with 2-3 rows a wave; NV = 4 with a few second rows
LN_STRIDED = ((5, 7, 256), (5, 7, 768))        # (n, L, D): the class-token rows of [n*L, D], ldx = ld_out = L*D
LN_INST = (33, 512)                            # the four instantiations x the output selections; accumulate
LN_BIGMEAN = (64, 768)                         # mean 8, std 0.25: two-pass variance
LN_SELECTIONS = ("dx", "dxsum", "dgb", "all")


def ln_eval(x, g, b, dy, res, dt):
    """LayerNorm and its backward in dtype `dt` by autograd through oracle.models.layer_norm; dx includes `res` (None: none)"""
    xt, gt, bt = _t(x, dt).requires_grad_(True), _t(g, dt).requires_grad_(True), _t(b, dt).requires_grad_(True)
    y = omodels.layer_norm(xt, gt, bt)
    (y * _t(dy, dt)).sum().backward()
    mu = xt.detach().mean(dim=-1)
    var = ((xt.detach() - mu[:, None]) ** 2).mean(dim=-1)
    dx = xt.grad if res is None else xt.grad + _t(res, dt)
    return {"y": y.detach(), "mean": mu, "rstd": 1.0 / torch.sqrt(var + 1e-5), "dx": dx, "dx16": dx, "y16": y.detach(),
            "dgamma": gt.grad, "dbeta": bt.grad, "dxsum": dx.sum(0)}


@functools.lru_cache(maxsize=None)
def ln_case(tag: str, rows: int, D: int, dy_dtype=None, with_res: bool = True, mean: float = 0.5, std: float = 2.0, pick: int = 1):
    """inputs (numpy fp32), fp64 reference and fp32-CPU evaluation of one LayerNorm case.  pick = L: the rows are every L-th row
    of a [rows*L, D] fill (the strided cases); `xfull` / `resfull` hold the whole buffers"""
    xfull = ofill.fill(f"rowops/{tag}/x", (rows * pick, D), std=std, mean=mean)
    resfull = ofill.fill(f"rowops/{tag}/res", (rows * pick, D), std=1.0) if with_res else None
    x = np.ascontiguousarray(xfull[::pick])
    res = np.ascontiguousarray(resfull[::pick]) if with_res else None
    g = ofill.fill(f"rowops/{tag}/g", (D,), std=0.2, mean=1.0)
    b = ofill.fill(f"rowops/{tag}/b", (D,), std=0.2)
    dy = round16(ofill.fill(f"rowops/{tag}/dy", (rows, D), std=1.0), dy_dtype)
    ref = ln_eval(x, g, b, dy, res, torch.float64)
    got32 = ln_eval(x, g, b, dy, res, torch.float32)
    return {"x": x, "xfull": xfull, "res": res, "resfull": resfull, "g": g, "b": b, "dy": dy, "ref": ref, "got32": got32}


def stats32(ref):
    """the row statistics a backward test hands to the kernel: the fp64 values rounded to fp32, [rows, 2] = (mean, rstd)"""
    return torch.stack([ref["mean"], ref["rstd"]], dim=1).float()


def _amax(t):
    return float(_np64(t).__abs__().max())


def ln_specs(kind: str, rows: int, D: int, ref: dict, dtype=None) -> dict:
    """kind: 'plain' (reused tolerances), 'many' (column sums measured), 'bigmean' (everything measured).
    Scales of the measured quantities: the largest fp64 magnitude of the quantity (column sums, y, dx) and, for the row
    statistics, the row's largest |x - mean| ... restated through rstd: mean in units of 1/rstd, rstd relative"""
    s = {"y": tol(TOL_LN_Y32), "dx": tol(TOL_LN_DX), "dgamma": tol(tol_ln_colsum(rows)), "dbeta": tol(tol_ln_colsum(rows)),
         "dxsum": tol(tol_ln_colsum(rows)),
         "mean": meas("ln/mean", 1.0 / _np64(ref["rstd"]) + np.abs(_np64(ref["mean"]))), "rstd": meas("ln/rstd", _np64(ref["rstd"]))}
    if dtype is not None:
        s["y16"], s["dx16"] = tol(tol_ln_y16(dtype)), tol(tol_ln_dx16(dtype))
    if kind == "many":
        for k in ("dgamma", "dbeta", "dxsum"):
            s[k] = meas(f"ln_many/{rows}x{D}/{k}", _amax(ref[k]))
    if kind == "bigmean":
        for k in ("y", "dx", "dgamma", "dbeta", "dxsum"):
            s[k] = meas(f"ln_bigmean/{k}", _amax(ref[k]))
        s["mean"], s["rstd"] = meas("ln_bigmean/mean", s["mean"][2]), meas("ln_bigmean/rstd", s["rstd"][2])
    return s


def ln_cases_all():
    """(what, case, specs) of every LayerNorm case of the tables, for the CPU checks"""
    out = []
    for rows, D in LN_MANY:
        for dt in DTYPES:
            c = ln_case(f"many{rows}", rows, D, dt)
            out.append((f"ln many {rows}x{D} {dt}", c, ln_specs("many", rows, D, c["ref"], dt)))
    for n, L, D in LN_STRIDED:
        for dt in DTYPES:
            for with_res in (True, False):
                c = ln_case(f"strided{D}", n, D, dt, with_res, pick=L)
                out.append((f"ln strided n={n} L={L} D={D} {dt} res={with_res}", c, ln_specs("plain", n, D, c["ref"], dt)))
    rows, D = LN_INST
    for dt in (None,) + DTYPES:
        for with_res in (True, False):
            c = ln_case("inst", rows, D, dt, with_res)
            out.append((f"ln inst {dt} res={with_res}", c, ln_specs("plain", rows, D, c["ref"], dt)))
    rows, D = LN_BIGMEAN
    for dt in DTYPES:
        c = ln_case("bigmean", rows, D, dt, True, 8.0, 0.25)
        out.append((f"ln bigmean {dt}", c, ln_specs("bigmean", rows, D, c["ref"], dt)))
    return out


# ------------------------------------------------------------------------------------------------ embed + ln_pre
# every D with n < 4 and with n > 4, n % 4 != 0; every (n, L) with at least two D
EMBED_CASES = ((256, 1, 2), (256, 5, 64), (256, 9, 17), (512, 3, 50), (512, 9, 17), (768, 1, 2), (768, 3, 50), (768, 5, 64),
               (1024, 1, 2), (1024, 3, 50), (1024, 5, 64), (1024, 9, 17))          # (D, n, L)


def embed_eval(c, dt):
    tok, cls, pos = (_t(c[k], dt).requires_grad_(True) for k in ("tok", "cls", "pos"))
    g, b = _t(c["g"], dt).requires_grad_(True), _t(c["b"], dt).requires_grad_(True)
    n, L, D = c["dims"]
    x0 = (torch.cat([cls.reshape(1, 1, D).expand(n, 1, D), tok.reshape(n, L - 1, D)], dim=1) + pos).reshape(n * L, D)
    y = omodels.layer_norm(x0, g, b)
    (y * _t(c["dy"], dt)).sum().backward()
    xd = x0.detach()
    mu = xd.mean(dim=-1)
    var = ((xd - mu[:, None]) ** 2).mean(dim=-1)
    return {"x0": xd, "y": y.detach(), "mean": mu, "rstd": 1.0 / torch.sqrt(var + 1e-5), "dtok": tok.grad, "dcls": cls.grad,
            "dpos": pos.grad, "dgamma": g.grad, "dbeta": b.grad}


@functools.lru_cache(maxsize=None)
def embed_case(D: int, n: int, L: int):
    tag = f"rowops/embed/{D}/{n}/{L}"
    c = {"dims": (n, L, D), "tok": ofill.fill(tag + "/tok", (n * (L - 1), D), std=1.0), "cls": ofill.fill(tag + "/cls", (D,), std=1.0),
         "pos": ofill.fill(tag + "/pos", (L, D), std=0.5, mean=0.25), "g": ofill.fill(tag + "/g", (D,), std=0.2, mean=1.0),
         "b": ofill.fill(tag + "/b", (D,), std=0.2), "dy": ofill.fill(tag + "/dy", (n * L, D), std=1.0)}
    # what the accumulating outputs hold before the call
    c["pre"] = {"dcls": ofill.fill(tag + "/pre_dcls", (D,), std=1.0, mean=2.0), "dpos": ofill.fill(tag + "/pre_dpos", (L, D), std=1.0, mean=-2.0),
                "dgamma": ofill.fill(tag + "/pre_dg", (D,), std=1.0, mean=3.0), "dbeta": ofill.fill(tag + "/pre_db", (D,), std=1.0, mean=-3.0)}
    c["ref"] = embed_eval(c, torch.float64)
    c["got32"] = embed_eval(c, torch.float32)
    for k, v in c["pre"].items():
        c["ref"][k] = c["ref"][k] + _t(v, torch.float64)
        c["got32"][k] = c["got32"][k] + _t(v, torch.float32)
    return c


def embed_specs(c, dtype=None) -> dict:
    """x0 is one fp32 addition: compared bit for bit by the tests.  y as LayerNorm forward; the sums over n images (dpos, dcls)
    and over n*L rows (dgamma, dbeta) by the column-sum rule of test_layernorm at their own row counts"""
    n, L, D = c["dims"]
    ref = c["ref"]
    s = {"y": tol(TOL_LN_Y32), "dpos": tol(tol_ln_colsum(n)), "dcls": tol(tol_ln_colsum(n)), "dgamma": tol(tol_ln_colsum(n * L)),
         "dbeta": tol(tol_ln_colsum(n * L)),
         "mean": meas("ln/mean", 1.0 / _np64(ref["rstd"]) + np.abs(_np64(ref["mean"]))), "rstd": meas("ln/rstd", _np64(ref["rstd"]))}
    if dtype is not None:
        s["dtok"] = tol(tol_ln_dx16(dtype))
    return s


# ------------------------------------------------------------------------------------------------ objective heads
ROW_N = (1, 4, 5, 257)                    # wave-per-row heads, four rows a workgroup: one row, a full workgroup, one past it, many
ROW_D = (1, 63, 64, 65, 100, 512)         # below, at and one past the 64 lanes; ragged; several strides
CLIP_D = (63, 64, 65, 100, 512)
CLIP_T = (2, 5, 64)
ELEM_N = (1, 255, 256, 257, 1000)         # elementwise heads, 256 a workgroup
UPSTREAM = 1.5                            # the factor on the loss before backward
GRAD_SCALE = 256.0
HSC_NORMS = (1e-3, 1e-2, 1.0, 30.0)
EDGE_LOGITS = (0.0, 1e-4, -1e-4, 5.0, -5.0, 17.0, -17.0, 40.0, -40.0, 90.0, -90.0, 200.0, -200.0)
FOCAL_GAMMA, FOCAL_EPS = 2.0, 1e-7


def inv_count_of(n):
    """every other case runs with an explicit inv_count (1 / (4 n), the data-parallel convention), the rest with the default 1 / n"""
    return None if n % 2 else 1.0 / (4 * n)


def row_labels(tag, n):
    y = ofill.fill_int(f"rowops/{tag}/y", (n,), 0, 2)
    if n >= 2:
        y[0], y[1] = 0, 1                 # both classes in every batch
    return y


def _rows(t):
    return t[:, None] if t.dim() == 1 else t


def hsc_eval(f, y, nominal, inv, up, dt):
    """per-row dist / score / loss, mean loss and gradient of the HSC head (closed form of the oracle: autograd through sqrt is NaN at
    an all-zero row)"""
    ft, yt = _t(f, dt), torch.from_numpy(y)
    inv = 1.0 / f.shape[0] if inv is None else inv
    rows = oobj.hsc_losses(ft, yt, nominal)
    return {"dist": oobj.hsc_dists(ft), "score": oobj.hsc_score(ft), "rows": rows, "loss": (rows.sum() * inv).reshape(1),
            "grad": oobj.hsc_loss_grad(ft, yt, nominal, inv) * up}


def hsc_specs(f, y, nominal, inv, up, ref, regime) -> dict:
    """regime 'plain': the tolerances of test_hsc_bce.  regime 'edge' (small norms, d = 1): the kernel and the fp32 reference compute
    sqrt(ss + 1) - 1 and 1 - exp(-dist), so dist carries an ABSOLUTE error of a few ulps of root = sqrt(ss + 1) and the score of a few
    ulps of 1; -log(score + 1e-9) and the anomalous gradient factor -e / (1 - e) turn that into (absolute error) / score.  Scales:
        dist: root          score: 1          row loss: nominal root, anomalous root / score + |loss|
        gradient row: max |g| of the row x (nominal 1, anomalous 1 + root (1 + 1 / score));  all-zero rows are exact (tests)"""
    n = f.shape[0]
    inv = 1.0 / n if inv is None else inv
    if regime == "plain":
        lref = abs(float(ref["loss"]))
        return {"loss": ("tol", 0.0, TOL_LOSS_REL * max(1.0, lref * (1.0 / (n * inv)))), "grad": tol(TOL_HSC_GRAD), "score": tol(TOL_HSC_SCORE)}
    ss = (np.asarray(f, np.float64) ** 2).sum(1)
    root = np.sqrt(ss + 1)
    score = np.maximum(_np64(ref["score"]), FLT_MIN)
    anom, zero = (y != nominal), (ss == 0)
    rows = np.abs(_np64(ref["rows"]))
    s_rows = np.where(zero, rows + 1.0, np.where(anom, root / score + rows, root))
    gmax = np.abs(_np64(ref["grad"])).max(1)
    s_grad = gmax * np.where(anom, 1 + root * (1 + 1 / score), 1.0)
    return {"dist": meas("hsc/dist", root), "score": meas("hsc/score", 1.0), "rows": meas("hsc/rows", s_rows),
            "loss": meas("hsc/rows", float((s_rows * inv).sum())), "grad": meas("hsc/grad", np.broadcast_to(s_grad[:, None], f.shape))}


@functools.lru_cache(maxsize=None)
def hsc_case(n, d, nominal, regime="plain"):
    if regime == "plain":
        f = ofill.fill(f"rowops/hsc/f{n}x{d}", (n, d), std=0.08)
        y = row_labels(f"hsc/{n}x{d}", n)
    else:                                 # each norm in both label classes, plus an all-zero row in each
        u = ofill.fill(f"rowops/hsc/edge{d}", (2 * len(HSC_NORMS) + 2, d), std=1.0).astype(np.float64)
        u /= np.sqrt((u * u).sum(1, keepdims=True))
        mag = np.array([m for m in HSC_NORMS for _ in (0, 1)] + [0.0, 0.0])
        f = (u * mag[:, None]).astype(np.float32)
        y = np.array([0, 1] * (len(HSC_NORMS) + 1), dtype=np.int64)
        n = f.shape[0]
    inv, up = inv_count_of(n), UPSTREAM
    ref = hsc_eval(f, y, nominal, inv, up, torch.float64)
    return {"f": f, "y": y, "nominal": nominal, "inv": inv, "up": up, "ref": ref, "got32": hsc_eval(f, y, nominal, inv, up, torch.float32),
            "specs": hsc_specs(f, y, nominal, inv, up, ref, regime)}


def hsc_cases_all():
    out = [(n, d, nom, "plain") for n in ROW_N for d in ROW_D if d >= 63 for nom in (0, 1)]
    out += [(n, 1, nom, "edge1") for n in ROW_N for nom in (0, 1)]                 # d = 1: small norms by construction
    out += [(0, d, nom, "edge") for d in (1, 100) for nom in (0, 1)]
    return out


def hsc_case_of(n, d, nom, regime):
    if regime == "edge1":                 # the plain fill at d = 1, judged by the edge rule
        c = dict(hsc_case(n, d, nom, "plain"))
        c["specs"] = hsc_specs(c["f"], c["y"], nom, c["inv"], c["up"], c["ref"], "edge")
        return c
    return hsc_case(n, d, nom, regime)


def dsad_eval(f, y, nominal, inv, up, dt):
    ft, yt = _t(f, dt), torch.from_numpy(y)
    inv = 1.0 / f.shape[0] if inv is None else inv
    rows = oobj.dsad_losses(ft, yt, nominal)
    return {"rows": rows, "loss": (rows.sum() * inv).reshape(1), "grad": oobj.dsad_loss_grad(ft, yt, nominal, inv) * up}


@functools.lru_cache(maxsize=None)
def dsad_case(n, d, nominal, regime="plain"):
    """'edge': anomalous rows at |f|^2 ~ 1e-3 and one all-zero row in each class (loss 1 / 1e-9 to fp32 rounding, gradient exactly 0);
    everything there is a ratio of a sum of squares, so the scales are the row's own |loss| and largest |gradient|"""
    if regime == "plain":
        f = ofill.fill(f"rowops/dsad/f{n}x{d}", (n, d), std=0.08)
        y = row_labels(f"dsad/{n}x{d}", n)
    else:
        f = ofill.fill(f"rowops/dsad/edge{d}", (10, d), std=math.sqrt(1e-3 / d))
        f[4:6] = 0.0
        f[6:] *= 30.0
        y = np.array([0, 1] * 5, dtype=np.int64)
        n = 10
    inv, up = inv_count_of(n), UPSTREAM
    ref = dsad_eval(f, y, nominal, inv, up, torch.float64)
    w = (1.0 / n if inv is None else inv)
    if regime == "plain":
        specs = {"loss": ("tol", TOL_N4_LOSS_REL, 0.0), "rows": ("tol", TOL_N4_LOSS_REL, 0.0),
                 "grad": ("tol", TOL_DSAD_GRAD[0], TOL_DSAD_GRAD[1] * w * up)}
    else:
        rows = np.abs(_np64(ref["rows"]))
        gmax = np.abs(_np64(ref["grad"])).max(1)
        specs = {"rows": meas("dsad/rows", rows), "loss": meas("dsad/rows", float((rows * w).sum())),
                 "grad": meas("dsad/grad", np.broadcast_to(gmax[:, None], f.shape))}
    return {"f": f, "y": y, "nominal": nominal, "inv": inv, "up": up, "ref": ref, "got32": dsad_eval(f, y, nominal, inv, up, torch.float32),
            "specs": specs}


def dsad_cases_all():
    return [(n, d, nom, "plain") for n in ROW_N for d in ROW_D for nom in (0, 1)] + [(0, d, nom, "edge") for d in (1, 100) for nom in (0, 1)]


def dsvdd_eval(f, c, inv, up, dt):
    ft, ct = _t(f, dt), _t(c, dt)
    inv = 1.0 / f.shape[0] if inv is None else inv
    rows = oobj.dsvdd_score(ft, ct)
    return {"score": rows, "loss": (rows.sum() * inv).reshape(1), "grad": oobj.dsvdd_loss_grad(ft, ct, inv) * up}


@functools.lru_cache(maxsize=None)
def dsvdd_case(n, d):
    f = ofill.fill(f"rowops/dsvdd/f{n}x{d}", (n, d), std=0.08)
    c = ofill.fill(f"rowops/dsvdd/c{d}", (d,), std=0.1, mean=0.05)
    inv, up = inv_count_of(n), UPSTREAM
    w = (1.0 / n if inv is None else inv)
    specs = {"loss": ("tol", TOL_N4_LOSS_REL, 0.0), "score": tol(TOL_DSVDD_SCORE), "grad": ("tol", TOL_DSVDD_GRAD[0], TOL_DSVDD_GRAD[1] * w * up)}
    return {"f": f, "c": c, "inv": inv, "up": up, "ref": dsvdd_eval(f, c, inv, up, torch.float64),
            "got32": dsvdd_eval(f, c, inv, up, torch.float32), "specs": specs}


def dsvdd_cases_all():
    return [(n, d) for n in ROW_N for d in ROW_D]


def elem_eval(head, x, y, inv, up, dt):
    """bce / focal on logits x [n]: per-element losses, mean loss, gradient, and the score for both nominal labels"""
    xt, yt = _t(x, dt), torch.from_numpy(y)
    inv = 1.0 / x.shape[0] if inv is None else inv
    if head == "bce":
        rows, grad = oobj.bce_losses(xt, yt), oobj.bce_loss_grad(xt, yt, inv)
    else:
        rows, grad = oobj.focal_losses(xt, yt, FOCAL_GAMMA, FOCAL_EPS), oobj.focal_loss_grad(xt, yt, FOCAL_GAMMA, FOCAL_EPS, inv)
    return {"rows": rows, "loss": (rows.sum() * inv).reshape(1), "grad": grad * up, "score0": oobj.bce_score(xt, 0).reshape(-1),
            "score1": oobj.bce_score(xt, 1).reshape(-1)}


def edge_logit_table():
    """every edge logit with both labels"""
    x = np.array([v for v in EDGE_LOGITS for _ in (0, 1)], dtype=np.float32)
    y = np.array([0, 1] * len(EDGE_LOGITS), dtype=np.int64)
    return x, y


def focal_edge_distance(x, y):
    """distance of each (logit, label) to the two clamp edges of pt = clamp(exp(-b), eps, 1 - eps), in fp64.  The upper edge 1 - eps
    is within 1e-7 of 1, so in exp(-b) itself every saturated logit would be 'close' to it; the distance is therefore taken where the
    edges are far apart, on b = -log(exp(-b)): |b - b_edge| / b_edge for b_edge = -log(eps) and -log(1 - eps)"""
    b = _np64(oobj.bce_losses(_t(x, torch.float64), torch.from_numpy(y)))
    edges = np.array([-math.log(FOCAL_EPS), -math.log1p(-FOCAL_EPS)])
    return np.abs(b[:, None] - edges[None, :]) / edges[None, :]


@functools.lru_cache(maxsize=None)
def elem_case(head, n, regime="plain"):
    """'edge' (n ignored): EDGE_LOGITS x both labels.  Scales there: a loss element's own bce value b (the focal weight is <= 1; its
    cancellation 1 - pt costs ulps of 1, not of the tiny result); a gradient element's max(sigmoid, label) -- the size of the two
    terms of sigmoid(x) - y, whose difference keeps their absolute error (the focal bracket is of order 1); sigmoid itself for the
    score with nominal_label 0 and 1 for 1 - sigmoid"""
    if regime == "plain":
        x = ofill.fill(f"rowops/{head}/x{n}", (n,), std=2.0)
        y = row_labels(f"{head}/{n}", n)
    else:
        x, y = edge_logit_table()
        n = x.shape[0]
    inv, up = inv_count_of(n), UPSTREAM
    w = (1.0 / n if inv is None else inv)
    ref = elem_eval(head, x, y, inv, up, torch.float64)
    if regime == "plain" and head == "bce":
        lref = abs(float(ref["loss"])) / (n * w)
        specs = {"loss": ("tol", 0.0, TOL_LOSS_REL * max(1.0, lref) * n * w), "grad": tol(TOL_HSC_GRAD), "score0": tol(TOL_HSC_SCORE),
                 "score1": tol(TOL_HSC_SCORE)}
    elif regime == "plain":
        specs = {"loss": ("tol", TOL_N4_LOSS_REL, 0.0), "grad": ("tol", TOL_FOCAL_GRAD[0], TOL_FOCAL_GRAD[1] * w * up),
                 "score0": tol(TOL_FOCAL_SCORE), "score1": tol(TOL_HSC_SCORE)}
    else:
        b = _np64(oobj.bce_losses(_t(x, torch.float64), torch.from_numpy(y)))
        s = _np64(torch.sigmoid(_t(x, torch.float64)))
        specs = {"rows": meas(f"{head}/rows", b), "loss": meas(f"{head}/rows", float((b * w).sum())),
                 "grad": meas(f"{head}/grad", np.maximum(s, y.astype(np.float64)) * w * up),
                 "score0": meas("elem/score0", s), "score1": meas("elem/score1", 1.0)}
    return {"x": x, "y": y, "inv": inv, "up": up, "ref": ref, "got32": elem_eval(head, x, y, inv, up, torch.float32), "specs": specs}


def elem_cases_all():
    return [(h, n, "plain") for h in ("bce", "focal") for n in ELEM_N] + [(h, 0, "edge") for h in ("bce", "focal")]


def clip_eval(f, y, t, nominal, loo, inv, up, dt):
    ft, tt, yt = _t(f, dt).requires_grad_(True), _t(t, dt), torch.from_numpy(y)
    inv = 1.0 / f.shape[0] if inv is None else inv
    rows = oobj.clip_losses(ft, yt, tt, nominal, loo)
    loss = rows.sum() * inv
    (loss * up).backward()
    return {"loss": loss.detach().reshape(1), "grad": ft.grad, "score": oobj.clip_score(ft.detach(), tt)}


@functools.lru_cache(maxsize=None)
def clip_case(n, d, T, loo, nominal):
    """|f| stays of order sqrt(d) (std 1); one label that is neither class where n >= 4; for T >= 3 prompt 2 repeats prompt 1 (a tie
    among the leave_one_out candidates) and the first sample is aligned with it, so the tie is the maximum there.  The tied prompts
    are identical rows, so either pick gives the same loss and gradient: the first maximum is what the fp64 reference takes"""
    f = ofill.fill(f"rowops/clip/f{n}x{d}", (n, d), std=1.0)
    t = ofill.fill(f"rowops/clip/t{T}x{d}", (T, d), std=1.0).astype(np.float64)
    t = (t / np.sqrt((t * t).sum(1, keepdims=True)) * 0.2 + 0.05).astype(np.float32)          # as test_clip_objective_n2_vs_golden_and_oracle
    y = row_labels(f"clip/{n}x{d}", n)
    if T >= 3:
        t[2] = t[1]
        f[0] = f[0] * 0.25 + 40.0 * t[1]
        y[0] = nominal
    if n >= 4:
        y[3] = 7
    inv, up = inv_count_of(n), UPSTREAM
    w = (1.0 / n if inv is None else inv)
    specs = {"loss": ("tol", 0.0, TOL_CLIP_LOSS_ABS * n * w), "grad": ("tol", TOL_CLIP_GRAD[0], TOL_CLIP_GRAD[1] * w * up), "score": tol(TOL_CLIP_SCORE)}
    return {"f": f, "t": t, "y": y, "nominal": nominal, "loo": loo, "inv": inv, "up": up, "ref": clip_eval(f, y, t, nominal, loo, inv, up, torch.float64),
            "got32": clip_eval(f, y, t, nominal, loo, inv, up, torch.float32), "specs": specs}


def clip_cases_all():
    return [(n, d, T, loo, nom) for n in ROW_N for d in CLIP_D for T in CLIP_T for loo in (False, True) for nom in (0, 1)]


# ------------------------------------------------------------------------------------------------ the measurement
def all_cases():
    """(what, ref, got32, specs) of every case of every table"""
    for what, c, specs in ln_cases_all():
        yield what, c["ref"], c["got32"], specs
    for D, n, L in EMBED_CASES:
        c = embed_case(D, n, L)
        for dt in DTYPES:
            yield f"embed D={D} n={n} L={L} {dt}", c["ref"], c["got32"], embed_specs(c, dt)
    for args in hsc_cases_all():
        c = hsc_case_of(*args)
        yield f"hsc {args}", c["ref"], c["got32"], c["specs"]
    for args in dsad_cases_all():
        c = dsad_case(*args)
        yield f"dsad {args}", c["ref"], c["got32"], c["specs"]
    for args in dsvdd_cases_all():
        c = dsvdd_case(*args)
        yield f"dsvdd {args}", c["ref"], c["got32"], c["specs"]
    for args in elem_cases_all():
        c = elem_case(*args)
        yield f"{args}", c["ref"], c["got32"], c["specs"]
    for args in clip_cases_all():
        c = clip_case(*args)
        yield f"clip {args}", c["ref"], c["got32"], c["specs"]


def measure() -> dict:
    table = {}
    for _, ref, got32, specs in all_cases():
        measure_into(table, got32, ref, specs)
    return table


if __name__ == "__main__":
    for k, v in sorted(measure().items()):
        print(f'    "{k}": {v:.3e},    # {v / ULP32:.2f} ulp -> kernel bound {(K_KERNEL * v + FLOOR_ULPS * ULP32) / ULP32:.1f} ulp')
