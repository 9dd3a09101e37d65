"""Case table, inputs, rounding model and fp32 restatement of the long-sequence attention tests (tests/test_gpu_attention_long.py on the
GPU, tests/test_cpu_attention_long.py without one): attn_long_fwd / attn_long_bwd of csrc/attention_long.hip, 64 < L <= LONG_MAX_L.

The fp64 references, the comparison functions and every tolerance are tests/attention_util.py's, imported unchanged (FWD_ABS_V,
FWD_CLOSE, BWD_ABS_THIRD, BWD_REL_RMS and the dbias form); nothing is introduced here.

Regimes.  unit, peaked: attention_util's.  offset: its mean 4, with std 0.75 (see below).  late64 / late128, the non-causal form of its
`late`: unit q, k, v plus a constant C along the direction (1, ..., 1) / 8 of every head on ALL queries and on the keys >= 64 (>= 128)
only, so a query has its largest logit, by about C^2 / 8, in a key block that comes after one (two) blocks have been accumulated: the
running maximum moves and the accumulator and row sum must be rescaled.

Two inputs were changed for the one-third condition (attention_util's docstring; a condition on the inputs, no tolerance moved):
  * offset with attention_util's std 1 gave rel_rms / 3 EPS16 = 0.346 over these longer rows; std 0.75 is used (every logit still lies
    near 128, above the overflow point of an unsubtracted expf);
  * late128 with LATE_C = 16 at L = 129 leaves ONE late key, which takes all but e^-32 of every row: dS underflows the 16-bit formats and
    the dQ / dK thirds of the fp64 reference are of the order 1e-13 (model error / allowance 248).  late128 uses C = 8 (LATE_C_LONG);
    late64 keeps LATE_C = 16.

ROUNDING MODEL (model_long), written from the header of csrc/attention_long.hip: fp64 with
  forward   per 64-key block the UNNORMALISED e = exp(s - running maximum) rounded to 16 bit before its product with V, the
            accumulator rescaled when the maximum moves, the row sum from the unrounded e, out = O / l rounded;
  backward  P = softmax normalised and rounded before dO^T P (dV); dS = P (dP - delta) / 8 with delta = sum_key P dP from unrounded
            values, rounded before K^T dS^T (dQ) and Q^T dS (dK); dQ, dK, dV rounded;
  dbias     the Q third from the unrounded dQ, the K third exactly 0, the V third the column sums of dO.

restate32_long: an fp32 restatement of the kernels' block structure on flat memory (reads behind the end give zero, as the kernels'
buffer resources do), (image, head) units in DESCENDING order (no order is promised on a GPU, and this one lets a write past an image's
last row land on rows that were already written), with one deliberate error when `mutant` is named (MUTANTS).

Measured model error / allowance, the largest over the table (`python tests/attention_long_util.py` prints these lines):
    long   late128 backward per third / 8 EPS16 max|ref|      0.190
    long   late128 dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.009
    long   late128 forward / (4 EPS16, 6 EPS16)               0.102
    long   late128 forward / 6 EPS16 max|v|                   0.098
    long   late128 rel_rms / 3 EPS16                          0.227
    long   late64  backward per third / 8 EPS16 max|ref|      0.185
    long   late64  dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.006
    long   late64  forward / (4 EPS16, 6 EPS16)               0.131
    long   late64  forward / 6 EPS16 max|v|                   0.127
    long   late64  rel_rms / 3 EPS16                          0.225
    long   offset  backward per third / 8 EPS16 max|ref|      0.302
    long   offset  dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.017
    long   offset  forward / (4 EPS16, 6 EPS16)               0.128
    long   offset  forward / 6 EPS16 max|v|                   0.125
    long   offset  rel_rms / 3 EPS16                          0.310
    long   peaked  backward per third / 8 EPS16 max|ref|      0.152
    long   peaked  dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.020
    long   peaked  forward / (4 EPS16, 6 EPS16)               0.132
    long   peaked  forward / 6 EPS16 max|v|                   0.132
    long   peaked  rel_rms / 3 EPS16                          0.199
    long   unit    backward per third / 8 EPS16 max|ref|      0.172
    long   unit    dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.034
    long   unit    forward / (4 EPS16, 6 EPS16)               0.093
    long   unit    forward / 6 EPS16 max|v|                   0.090
    long   unit    rel_rms / 3 EPS16                          0.204
"""
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # `python tests/attention_long_util.py`
import attention_util as au          # noqa: E402
from attention_util import (BWD_ABS_THIRD, BWD_REL_RMS, DBIAS_ABS, DBIAS_RTOL, DTYPES, EPS16, FWD_ABS_V, FWD_CLOSE, LATE_C, SCALE,          # noqa: E402,F401
                            bwd_failures, bwd_ratios, dbias_failures, dbias_start, fwd_failures, fwd_ratios, merge_heads, split_heads)

LONG_MIN_L, LONG_MAX_L = 65, 640                                         # eoe_amd.ops.ATTN_SHORT_MAX_L + 1, ATTN_LONG_MAX_L
BLOCK = 64                                                               # keys (and queries) per block

# ------------------------------------------------------------------------------------------------ case table
UNIT_L = (65, 66, 127, 128, 129, 145, 191, 192, 193, 197, 256, 257, 577)
SHAPE = (2, 2)                                                           # (n, heads)
MAG_L = (65, 128, 129, 197)
LATE_L = (129, 197)
LATE_FROM = {"late64": 64, "late128": 128}
LATE_C_LONG = {"late64": LATE_C, "late128": 8.0}
REGIMES = dict(au.REGIMES, offset=(0.75, 4.0))          # (std, mean) of q and k; v and dO: std 1
GRID = ((1, 1), (1, 12), (7, 3), (257, 1))
GRID_L = (65, 197)
NEIGHBOUR_L = (65, 197)


def long_table():
    """(regime, n, L, heads) of every case that is compared with fp64"""
    t = [("unit",) + (SHAPE[0], L, SHAPE[1]) for L in UNIT_L]
    t += [(r, SHAPE[0], L, SHAPE[1]) for r in ("peaked", "offset") for L in MAG_L]
    t += [(r, SHAPE[0], L, SHAPE[1]) for r in LATE_FROM for L in LATE_L]
    t += [("unit", n, L, h) for n, h in GRID for L in GRID_L]
    return list(dict.fromkeys(t))


def long_inputs(regime, n, L, heads, dtype):
    """(qkv [n L, 3 D], dout [n L, D]) in the 16-bit dtype"""
    D = heads * 64
    late = regime in LATE_FROM
    std, mean = REGIMES["unit" if late else regime]
    name = f"attn/long/{regime}/{n}x{L}x{heads}"
    x = torch.cat([au.r16(name + "/q", (n * L, D), std, dtype, mean), au.r16(name + "/k", (n * L, D), std, dtype, mean),
                   au.r16(name + "/v", (n * L, D), 1.0, dtype)], dim=1)
    if late:
        x = x.float().reshape(n, L, 3 * D)
        x[:, :, :D] += LATE_C_LONG[regime] / 8.0
        x[:, LATE_FROM[regime]:, D:2 * D] += LATE_C_LONG[regime] / 8.0
        x = x.reshape(n * L, 3 * D).to(dtype)
    return x.contiguous(), au.r16(name + "/do", (n * L, D), 1.0, dtype)


@functools.lru_cache(maxsize=None)
def long_case(regime, n, L, heads, dtype):
    """inputs and fp64 results of one case (attention_util.vit_case's fields); nothing in it is ever modified"""
    qkv, dout = long_inputs(regime, n, L, heads, dtype)
    x = qkv.double().requires_grad_(True)
    out = au.attn_ref64(x, n, L, heads)
    (out * dout.double()).sum().backward()
    D = heads * 64
    return {"dims": (n, L, heads), "dtype": dtype, "qkv": qkv, "dout": dout, "out": out.detach(), "dqkv": x.grad,
            "dbias": x.grad.sum(0), "docol": dout.double().sum(0), "vmax": float(qkv[:, 2 * D:].float().abs().max()),
            "gscale": float(x.grad.abs().max())}


# ------------------------------------------------------------------------------------------------ the rounding model
def _r(x, dtype):
    return x.to(dtype).double()


def model_long(c):
    """fp64 with the documented roundings of attn_long_fwd / attn_long_bwd: {'out', 'dqkv', 'dbias'}"""
    n, L, heads = c["dims"]
    dt = c["dtype"]
    q, k, v = split_heads(c["qkv"].double(), n, L, heads, 3)
    do = split_heads(c["dout"].double(), n, L, heads, 1)[0]
    s = q @ k.transpose(-1, -2) * SCALE
    o = torch.zeros(n, heads, L, 64, dtype=torch.float64)
    m = torch.full((n, heads, L, 1), float("-inf"), dtype=torch.float64)
    l = torch.zeros(n, heads, L, 1, dtype=torch.float64)
    for k0 in range(0, L, BLOCK):
        sb = s[..., k0:k0 + BLOCK]
        mnew = torch.maximum(m, sb.max(-1, keepdim=True).values)
        alpha, e = torch.exp(m - mnew), torch.exp(sb - mnew)
        l = l * alpha + e.sum(-1, keepdim=True)
        o = o * alpha + _r(e, dt) @ v[:, :, k0:k0 + BLOCK]
        m = mnew
    out = _r(merge_heads((o / l)[None], n, L, heads), dt)
    p = torch.softmax(s, dim=-1)
    p16 = _r(p, dt)
    dp = do @ v.transpose(-1, -2)
    ds16 = _r(p * (dp - (p * dp).sum(-1, keepdim=True)) * SCALE, dt)
    dq, dk, dv = ds16 @ k, ds16.transpose(-1, -2) @ q, p16.transpose(-1, -2) @ do
    acc = merge_heads(torch.stack([dq, dk, dv]), n, L, heads)
    D = heads * 64
    dbias = torch.cat([acc[:, :D].sum(0), torch.zeros(D, dtype=torch.float64), c["docol"]])
    return {"out": out, "dqkv": _r(acc, dt), "dbias": dbias}


# ------------------------------------------------------------------------------------------------ fp32 restatement and its mutants
MUTANTS = ("key_mask_edge", "no_rescale", "query_tail", "img_head_swap", "no_scale_ds")


def restate32_long(qkv, dout, n, L, heads, dtype, mutant=None, dbias_start=None):
    """attn_long_fwd + attn_long_bwd in fp32 on the CPU, one unit per (image, head) on flat memory, 64-key blocks, outputs pre-filled with
    NaN.  mutant (one deliberate error):
        key_mask_edge   the last key block masks keys > L instead of >= L: the row behind the image is a key (behind the last image: zeros)
        no_rescale      accumulator and row sum are not rescaled when the running maximum moves
        query_tail      the last query block stores all its 64 rows: out rows behind L, the next image's, are overwritten
        img_head_swap   img = unit % heads, h = unit / heads
        no_scale_ds     dS without the factor 1/8"""
    assert mutant is None or mutant in MUTANTS
    D = heads * 64
    ld = 3 * D
    qf, dof = qkv.float().reshape(-1), dout.float().reshape(-1)
    out = torch.full((n * L * D,), float("nan"))
    dqkv = torch.full((n * L * ld,), float("nan"))
    bseg = heads * n * 64
    part = torch.zeros(3 * bseg)
    Lk = L + 1 if mutant == "key_mask_edge" else L
    Lpad = (L + BLOCK - 1) // BLOCK * BLOCK
    Lq = Lpad if mutant == "query_tail" else L                # rows the forward stores; queries >= L are read as zeros
    for b in reversed(range(n * heads)):
        img, h = (b % heads, b // heads) if mutant == "img_head_swap" else (b // heads, b % heads)
        qb = img * L * ld + h * 64
        q, k, v = au._gather(qf, qb, L, ld), au._gather(qf, qb + D, Lk, ld), au._gather(qf, qb + 2 * D, Lk, ld)
        do = au._gather(dof, img * L * D + h * 64, L, D)
        qq = torch.cat([q, torch.zeros(Lq - L, 64)])
        s = (qq @ k.t()) * SCALE
        o, m, l = torch.zeros(Lq, 64), torch.full((Lq, 1), float("-inf")), torch.zeros(Lq, 1)
        for k0 in range(0, Lk, BLOCK):
            sb = s[:, k0:k0 + BLOCK]
            mnew = torch.maximum(m, sb.max(-1, keepdim=True).values)
            alpha = torch.ones_like(m) if mutant == "no_rescale" and k0 > 0 else torch.exp(m - mnew)
            e = torch.exp(sb - mnew)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + e.to(dtype).float() @ v[k0:k0 + BLOCK]
            m = mnew
        au._scatter(out, (img * L) * D + h * 64, Lq, D, (o / l).to(dtype).float())
        # backward: the statistics of pass 1 (lse, delta), then P = exp(s - lse)
        s = s[:L]
        lse = torch.logsumexp(s, dim=-1, keepdim=True)
        p = torch.exp(s - lse)
        p16 = p.to(dtype).float()
        dp = do @ v.t()
        ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * (1.0 if mutant == "no_scale_ds" else SCALE)
        ds16 = ds.to(dtype).float()
        dq, dk, dv = ds16 @ k, (ds16.t() @ q)[:L], (p16.t() @ do)[:L]
        for t, g in enumerate((dq, dk, dv)):
            au._scatter(dqkv, qb + t * D, L, ld, g.to(dtype).float())
        for t, colsum in enumerate((dq.sum(0), torch.zeros(64), do.sum(0))):
            au._scatter(part, t * bseg + (h * n + img) * 64, 1, 64, colsum[None])
    res = {"out": out.reshape(n * L, D).to(dtype), "dqkv": dqkv.reshape(n * L, ld).to(dtype)}
    if dbias_start is not None:
        res["dbias"] = dbias_start + part.reshape(3, heads, n, 64).sum(2).reshape(3 * D)
    return res


def restatement_failures(c, mutant=None):
    """everything the comparison functions find wrong with restate32_long's results of case c"""
    n, L, heads = c["dims"]
    start = dbias_start(heads)
    r = restate32_long(c["qkv"], c["dout"], n, L, heads, c["dtype"], mutant, start)
    return (fwd_failures(r["out"], c["out"], c["vmax"], c["dtype"]) + bwd_failures(r["dqkv"], c["dqkv"], heads, c["dtype"])
            + dbias_failures(r["dbias"], c, start))


# ------------------------------------------------------------------------------------------------ the measurement
def measure():
    """{(regime, quantity): largest rounding-model error / allowance over the table, both dtypes}"""
    table = {}

    def fold(key, value):
        table[key] = max(table.get(key, 0.0), value)

    for regime, n, L, heads in long_table():
        for dt in DTYPES:
            c = long_case(regime, n, L, heads, dt)
            m = model_long(c)
            a, b = fwd_ratios(m["out"], c["out"], c["vmax"], dt)
            fold((regime, "forward / 6 EPS16 max|v|"), a / FWD_ABS_V)
            fold((regime, "forward / (4 EPS16, 6 EPS16)"), b)
            a, b = bwd_ratios(m["dqkv"], c["dqkv"], heads, dt)
            fold((regime, "backward per third / 8 EPS16 max|ref|"), a / BWD_ABS_THIRD)
            fold((regime, "rel_rms / 3 EPS16"), b / BWD_REL_RMS)
            atol = DBIAS_ABS * EPS16[dt] * c["gscale"] * math.sqrt(n * L)
            fold((regime, "dbias / (1e-3, 8 EPS16 scale sqrt(n L))"),
                 float(((m["dbias"] - c["dbias"]).abs() / (atol + DBIAS_RTOL * c["dbias"].abs())).max()))
    return table


if __name__ == "__main__":
    for (regime, what), v in sorted(measure().items()):
        print(f"    long   {regime:7s} {what:42s} {v:.3f}")
