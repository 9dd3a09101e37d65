"""Case tables, inputs, references, tolerances and comparison functions of the attention tests (tests/test_gpu_attention.py on the
GPU, tests/test_cpu_attention.py without one): attn_fwd / attn_bwd of csrc/attention.hip (both backward kernels) and the causal
attn_causal_fwd of csrc/clip_text.hip.

Inputs are pure functions of a name (oracle.fill), rounded to the 16-bit dtype first exactly as gpu_util.t16 does (r16 below is
t16 without the upload); every reference sees those rounded values.

References.
  * attn_ref64 / vit_case: fp64 softmax(q k^T / 8) v per (image, head), gradients by fp64 autograd, dbias = column sums of the fp64
    dqkv.  causal=True adds CLIP's mask.
  * model_vit / model_causal, the ROUNDING MODEL: fp64 with the kernels' documented roundings -- P to 16 bit before P.V and P^T.dO,
    dS (scale included) to 16 bit before its two products, outputs to 16 bit; the causal form rounds the unnormalised exp(s - m)
    relative to the RUNNING maximum of its 64-key blocks and rescales, as the kernel's online softmax does.  CPU only: the yardstick
    of the tolerances.
  * restate32: an fp32 restatement of one workgroup per (image, head) on flat memory (reads behind the end give zero, as the
    kernels' buffer resources do), with the same roundings, and with one deliberate error when `mutant` is named (MUTANTS).  CPU
    only: the evidence that the comparison functions below notice a subtly wrong kernel.

Regimes.  unit: q, k, v, dO std 1 (test_gpu_ops.test_attention's).  peaked: q, k std 3, logit std about 9, most rows put more than
half their mass on one key.  offset: q, k mean 4 std 1, every logit near 128, above the overflow point of an unsubtracted fp32 expf
(88.7), spread across keys about 4.  late (causal only, L = 128): q and the keys >= 64 carry LATE_C along one direction, so every
query >= 64 has its largest logit, by about LATE_C^2 / 8, in the second 64-key block: the running maximum jumps after the first
block has been accumulated.

Tolerances: all reused, none measured on a kernel.
  forward    |err| <= 6 EPS16 max|v|                     test_gpu_clip_text.test_attn_causal_matches_fp64_and_is_causal
             and assert_close(4 EPS16, 6 EPS16)          test_gpu_ops.test_attention (the ViT kernels only)
  backward   |err| <= 8 EPS16 max|ref of the third|      test_attention's (8 EPS16, 8 EPS16 scale) with the scale taken per third
             rel_rms < 3 EPS16 over the whole tensor     test_attention
  dbias      (1e-3, 8 EPS16 scale sqrt(n L))             test_attention ("attention bwd bias sums")
The one-third condition (test_cpu_attention.test_rounding_model_uses_at_most_a_third_of_every_tolerance): over every case of the
tables below, both dtypes, the rounding model's distance to fp64 is at most one third of each of these allowances.  It is a
condition on the INPUTS: a case that breaks it is changed, the tolerance is not.

Measured model error / allowance, the largest over the table (`python tests/attention_util.py` prints these lines):
    causal late   forward / 6 EPS16 max|v|                   0.144
    causal offset forward / 6 EPS16 max|v|                   0.139
    causal peaked forward / 6 EPS16 max|v|                   0.141
    vit    offset backward per third / 8 EPS16 max|ref|      0.274
    vit    offset dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.020
    vit    offset forward / (4 EPS16, 6 EPS16)               0.182
    vit    offset forward / 6 EPS16 max|v|                   0.195
    vit    offset rel_rms / 3 EPS16                          0.323
    vit    peaked backward per third / 8 EPS16 max|ref|      0.155
    vit    peaked dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.024
    vit    peaked forward / (4 EPS16, 6 EPS16)               0.174
    vit    peaked forward / 6 EPS16 max|v|                   0.191
    vit    peaked rel_rms / 3 EPS16                          0.199
    vit    unit   backward per third / 8 EPS16 max|ref|      0.187
    vit    unit   dbias / (1e-3, 8 EPS16 scale sqrt(n L))    0.041
    vit    unit   forward / (4 EPS16, 6 EPS16)               0.179
    vit    unit   forward / 6 EPS16 max|v|                   0.180
    vit    unit   rel_rms / 3 EPS16                          0.232
"""
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # `python tests/attention_util.py`
from oracle import fill as ofill          # noqa: E402

EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # tests/gpu_util.py
DTYPES = (torch.bfloat16, torch.float16)
SCALE = 0.125                                                            # 1 / sqrt(64)
EXPF_OVERFLOW = 88.7                                                     # fp32 expf overflows above this

# ------------------------------------------------------------------------------------------------ tolerances (sources: docstring)
FWD_ABS_V = 6.0                  # x EPS16 x max|v|
FWD_CLOSE = (4.0, 6.0)           # x EPS16: (rtol, atol)
BWD_ABS_THIRD = 8.0              # x EPS16 x max|ref| of the third
BWD_REL_RMS = 3.0                # x EPS16
DBIAS_RTOL, DBIAS_ABS = 1e-3, 8.0        # atol = DBIAS_ABS x EPS16 x scale x sqrt(n L)

# ------------------------------------------------------------------------------------------------ case tables
REGIMES = {"unit": (1.0, 0.0), "peaked": (3.0, 0.0), "offset": (1.0, 4.0)}          # (std, mean) of q and k; v and dO: std 1
EVERY_L = tuple(range(1, 65))
EVERY_SHAPE = (2, 2)                                                     # (n, heads)
MAG_L = (1, 15, 16, 17, 32, 33, 48, 49, 50, 63, 64)
NEIGHBOUR_L = (1, 17, 64)
NEIGHBOUR_CAUSAL_L = (1, 65, 128)
GRID = ((1, 1), (1, 12), (7, 3), (257, 1), (3, 12))
GRID_L = (17, 50)
DBIAS_N = (1, 2, 257)
DBIAS_HEADS = 2
DBIAS_L = (16, 50)
CAUSAL_L = (64, 65, 128)
CAUSAL_HEADS = (1, 8)
CAUSAL_N = 2
LATE_L, LATE_C = 128, 16.0
PAD_ROWS = 5                                                             # sentinel / NaN rows around a view


def vit_table():
    """(regime, n, L, heads) of every ViT-kernel case that is compared with fp64"""
    t = [("unit",) + (EVERY_SHAPE[0], L, EVERY_SHAPE[1]) for L in EVERY_L]
    t += [(r, EVERY_SHAPE[0], L, EVERY_SHAPE[1]) for r in ("peaked", "offset") for L in MAG_L]
    t += [("unit", n, L, h) for n, h in GRID for L in GRID_L]
    t += [("unit", n, L, DBIAS_HEADS) for n in DBIAS_N for L in DBIAS_L]
    return list(dict.fromkeys(t))


def causal_table():
    t = [(r, CAUSAL_N, L, h) for r in ("peaked", "offset") for L in CAUSAL_L for h in CAUSAL_HEADS]
    return t + [("late", CAUSAL_N, LATE_L, h) for h in CAUSAL_HEADS]


# ------------------------------------------------------------------------------------------------ inputs
def r16(name, shape, std, dtype, mean=0.0):
    """gpu_util.t16 without the upload: the fill rounded to the 16-bit dtype (a CPU tensor of that dtype)"""
    return torch.from_numpy(ofill.fill(name, shape, std=std, mean=mean)).to(dtype)


def vit_inputs(regime, n, L, heads, dtype, tag="vit"):
    """(qkv [n L, 3 D], dout [n L, D]) in the 16-bit dtype"""
    D = heads * 64
    std, mean = REGIMES[regime]
    name = f"attn/{tag}/{regime}/{n}x{L}x{heads}"
    qkv = torch.cat([r16(name + "/q", (n * L, D), std, dtype, mean), r16(name + "/k", (n * L, D), std, dtype, mean),
                     r16(name + "/v", (n * L, D), 1.0, dtype)], dim=1)
    return qkv.contiguous(), r16(name + "/do", (n * L, D), 1.0, dtype)


def causal_inputs(regime, n, L, heads, dtype):
    """qkv [n L, 3 D] of a causal case.  'late': unit q, k, v plus LATE_C along the direction (1, ..., 1) / 8 of every head, on all
    queries and on the keys >= 64 only"""
    if regime != "late":
        return vit_inputs(regime, n, L, heads, dtype, tag="causal")[0]
    D = heads * 64
    x = vit_inputs("unit", n, L, heads, dtype, tag="causal_late")[0].float().reshape(n, L, 3 * D)
    x[:, :, :D] += LATE_C / 8.0
    x[:, 64:, D:2 * D] += LATE_C / 8.0
    return x.reshape(n * L, 3 * D).to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------ fp64 references
def split_heads(x, n, L, heads, parts):
    """[n L, parts * heads * 64] -> parts tensors [n, heads, L, 64]"""
    return x.reshape(n, L, parts, heads, 64).permute(2, 0, 3, 1, 4)


def merge_heads(x, n, L, heads):
    """[parts, n, heads, L, 64] -> [n L, parts * heads * 64]"""
    parts = x.shape[0]
    return x.permute(1, 3, 0, 2, 4).reshape(n * L, parts * heads * 64)


def causal_mask(L, dtype=torch.float64):
    return torch.full((L, L), float("-inf"), dtype=dtype).triu(1)


def logits64(qkv, n, L, heads, causal=False):
    q, k, _ = split_heads(qkv.double(), n, L, heads, 3)
    s = q @ k.transpose(-1, -2) * SCALE
    return s + causal_mask(L) if causal else s


def attn_ref64(qkv, n, L, heads, causal=False):
    """fp64 softmax(q k^T / 8 [+ causal mask]) v per (image, head): [n L, D]"""
    v = split_heads(qkv.double(), n, L, heads, 3)[2]
    o = torch.softmax(logits64(qkv, n, L, heads, causal), dim=-1) @ v
    return merge_heads(o[None], n, L, heads)


@functools.lru_cache(maxsize=None)
def vit_case(regime, n, L, heads, dtype):
    """inputs and fp64 results of one ViT-kernel case; nothing in it is ever modified"""
    qkv, dout = vit_inputs(regime, n, L, heads, dtype)
    x = qkv.double().requires_grad_(True)
    out = attn_ref64(x, n, L, heads)
    (out * dout.double()).sum().backward()
    D = heads * 64
    return {"dims": (n, L, heads), "dtype": dtype, "qkv": qkv, "dout": dout, "out": out.detach(), "dqkv": x.grad,
            "dbias": x.grad.sum(0), "docol": dout.double().sum(0), "vmax": float(qkv[:, 2 * D:].float().abs().max()),
            "gscale": float(x.grad.abs().max())}


@functools.lru_cache(maxsize=None)
def causal_case(regime, n, L, heads, dtype):
    qkv = causal_inputs(regime, n, L, heads, dtype)
    D = heads * 64
    return {"dims": (n, L, heads), "dtype": dtype, "qkv": qkv, "out": attn_ref64(qkv, n, L, heads, causal=True),
            "vmax": float(qkv[:, 2 * D:].float().abs().max())}


# ------------------------------------------------------------------------------------------------ the rounding model
def _r(x, dtype):
    return x.to(dtype).double()


def model_vit(c):
    """fp64 with the documented roundings of attn_fwd / attn_bwd: {'out', 'dqkv', 'dbias'}.  dbias as the four-wave kernel forms it:
    the Q third from the unrounded dQ, the K third exactly 0, the V third the column sums of dO"""
    n, L, heads = c["dims"]
    dt = c["dtype"]
    q, k, v = split_heads(c["qkv"].double(), n, L, heads, 3)
    do = split_heads(c["dout"].double(), n, L, heads, 1)[0]
    p = torch.softmax(q @ k.transpose(-1, -2) * SCALE, dim=-1)
    p16 = _r(p, dt)
    out = _r(merge_heads((p16 @ v)[None], n, L, heads), dt)
    dp = do @ v.transpose(-1, -2)
    ds16 = _r(p * (dp - (p * dp).sum(-1, keepdim=True)) * SCALE, dt)
    dq, dk, dv = ds16 @ k, ds16.transpose(-1, -2) @ q, p16.transpose(-1, -2) @ do
    acc = merge_heads(torch.stack([dq, dk, dv]), n, L, heads)
    D = heads * 64
    dbias = torch.cat([acc[:, :D].sum(0), torch.zeros(D, dtype=torch.float64), c["docol"]])
    return {"out": out, "dqkv": _r(acc, dt), "dbias": dbias}


def model_causal(c):
    """fp64 with the roundings of attn_causal_fwd: per 64-key block the unnormalised exp(s - running max) is rounded to 16 bit
    before its product with V, the accumulator is rescaled when the maximum moves, the row sum stays unrounded"""
    n, L, heads = c["dims"]
    dt = c["dtype"]
    v = split_heads(c["qkv"].double(), n, L, heads, 3)[2]
    s = logits64(c["qkv"], n, L, heads, causal=True)
    o = torch.zeros(n, heads, L, 64, dtype=torch.float64)
    m = torch.full((n, heads, L, 1), float("-inf"), dtype=torch.float64)
    l = torch.zeros(n, heads, L, 1, dtype=torch.float64)
    for k0 in range(0, L, 64):
        q0 = k0                                   # queries below the block see none of its keys: the kernel skips them
        sb = s[:, :, q0:, k0:k0 + 64]
        mnew = torch.maximum(m[:, :, q0:], sb.max(-1, keepdim=True).values)
        alpha = torch.exp(m[:, :, q0:] - mnew)
        e = torch.exp(sb - mnew)
        l[:, :, q0:] = l[:, :, q0:] * alpha + e.sum(-1, keepdim=True)
        o[:, :, q0:] = o[:, :, q0:] * alpha + _r(e, dt) @ v[:, :, k0:k0 + 64]
        m[:, :, q0:] = mnew
    return {"out": _r(merge_heads((o / l)[None], n, L, heads), dt)}


# ------------------------------------------------------------------------------------------------ comparing
def _d(t):
    return t.detach().float().cpu().double() if t.dtype != torch.float64 else t.detach().cpu()


def _worst(err, allow):
    ratio = err / allow
    i = int(ratio.argmax())
    return f"max err/allowance {float(ratio.max()):.3f} at flat index {i} (err {float(err.flatten()[i]):.3e})"


def fwd_failures(got, ref, vmax, dtype, frac=1.0, close=True):
    """what is wrong with a forward result: [] if nothing.  frac scales every allowance (1/3: the one-third condition).
    close=False leaves out test_attention's assert_close form (the causal kernel's own test has the first form only)"""
    g, r, eps = _d(got), _d(ref), EPS16[dtype]
    if g.shape != r.shape:
        return [f"out: shape {tuple(g.shape)} for {tuple(r.shape)}"]
    if not torch.isfinite(g).all():
        return ["out: non-finite values"]
    bad, err = [], (g - r).abs()
    if float(err.max()) > frac * FWD_ABS_V * eps * vmax:
        bad.append(f"out: |err| {float(err.max()):.3e} > {frac:.3g} x 6 EPS16 max|v| = {frac * FWD_ABS_V * eps * vmax:.3e}")
    allow = frac * (FWD_CLOSE[1] * eps + FWD_CLOSE[0] * eps * r.abs())
    if close and bool((err > allow).any()):
        bad.append("out: (4 EPS16, 6 EPS16): " + _worst(err, allow))
    return bad


def fwd_ratios(got, ref, vmax, dtype):
    """(err / (EPS16 max|v|), largest err / assert_close allowance)"""
    g, r, eps = _d(got), _d(ref), EPS16[dtype]
    err = (g - r).abs()
    return float(err.max()) / (eps * vmax), float((err / (FWD_CLOSE[1] * eps + FWD_CLOSE[0] * eps * r.abs())).max())


def rel_rms(got, ref):                       # gpu_util.rel_rms
    g, r = _d(got), _d(ref)
    return float((g - r).pow(2).mean().sqrt() / (r.pow(2).mean().sqrt() + 1e-30))


def bwd_ratios(got, ref, heads, dtype):
    """(largest per-third err / (EPS16 max|ref third|), rel_rms / EPS16)"""
    g, r, eps, D = _d(got), _d(ref), EPS16[dtype], heads * 64
    per = [float((g[:, t * D:(t + 1) * D] - r[:, t * D:(t + 1) * D]).abs().max()) / (eps * float(r[:, t * D:(t + 1) * D].abs().max()) + 1e-300)
           for t in range(3)]
    return max(per), rel_rms(g, r) / eps


def bwd_failures(got, ref, heads, dtype, frac=1.0):
    g, r, eps, D = _d(got), _d(ref), EPS16[dtype], heads * 64
    if g.shape != r.shape:
        return [f"dqkv: shape {tuple(g.shape)} for {tuple(r.shape)}"]
    if not torch.isfinite(g).all():
        return ["dqkv: non-finite values"]
    bad = []
    for t, name in enumerate(("dQ", "dK", "dV")):
        gt, rt = g[:, t * D:(t + 1) * D], r[:, t * D:(t + 1) * D]
        err, allow = float((gt - rt).abs().max()), frac * BWD_ABS_THIRD * eps * float(rt.abs().max())
        if err > allow:
            bad.append(f"{name}: |err| {err:.3e} > {frac:.3g} x 8 EPS16 max|ref| = {allow:.3e}")
    rr = rel_rms(g, r)
    if not rr < frac * BWD_REL_RMS * eps:
        bad.append(f"dqkv: rel_rms {rr:.3e} (= {rr / eps:.2f} EPS16), limit {frac:.3g} x 3 EPS16")
    return bad


def dbias_failures(got, c, start, frac=1.0, k_exact=True):
    """got = start + column sums (fp32 [3 D]) against case c.  Every third against the fp64 column sums of dqkv, the V third also
    against the fp64 column sums of dO; k_exact: the K third still holds the bits of `start` (the four-wave kernel adds exactly 0)"""
    n, L, heads = c["dims"]
    D, eps = heads * 64, EPS16[c["dtype"]]
    g, s0 = _d(got), _d(start)
    if not torch.isfinite(g).all():
        return ["dbias: non-finite values"]
    bad = []
    atol = DBIAS_ABS * eps * c["gscale"] * math.sqrt(n * L)
    for what, ref in (("column sums of dqkv", s0 + c["dbias"]), ("V third: column sums of dO", None)):
        if ref is None:
            gg, ref = g[2 * D:], s0[2 * D:] + c["docol"]
        else:
            gg = g
        err, allow = (gg - ref).abs(), frac * (atol + DBIAS_RTOL * ref.abs())
        if bool((err > allow).any()):
            bad.append(f"dbias, {what}: " + _worst(err, allow))
    if k_exact and not torch.equal(got[D:2 * D].detach().cpu().view(torch.int32), start[D:2 * D].detach().cpu().view(torch.int32)):
        bad.append("dbias: the K third changed")
    return bad


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def bitwise_failures(got, want, what):
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{what}: {tuple(got.shape)} {got.dtype} for {tuple(want.shape)} {want.dtype}"]
    ne = bits(got) != bits(want)
    return [f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits, first at {ne.nonzero()[0].tolist()}"] if bool(ne.any()) else []


def finite_failures(got, what):
    return [] if bool(torch.isfinite(got.detach().float()).all()) else [f"{what}: non-finite values"]


# ------------------------------------------------------------------------------------------------ fp32 restatement and its mutants
MUTANTS = ("key_mask", "no_max", "no_scale_ds", "img_head_swap", "dbias_k_from_v")


def _gather(flat, base, rows, pitch):
    idx = base + torch.arange(rows)[:, None] * pitch + torch.arange(64)[None, :]
    ok = idx < flat.numel()
    return torch.where(ok, flat[idx.clamp(max=flat.numel() - 1)], torch.zeros((), dtype=flat.dtype))


def _scatter(flat, base, rows, pitch, val):
    idx = base + torch.arange(rows)[:, None] * pitch + torch.arange(64)[None, :]
    ok = idx < flat.numel()
    flat[idx[ok]] = val[ok]


def restate32(qkv, dout, n, L, heads, dtype, mutant=None, dbias_start=None):
    """attn_fwd + attn_bwd (four-wave form of dbias) in fp32 on the CPU, one 'workgroup' per (image, head) on flat memory, outputs
    pre-filled with NaN.  mutant (one deliberate error):
        key_mask        keys <= L instead of < L: the next image's first row is read (behind the last image: zeros)
        no_max          softmax without the max subtraction
        no_scale_ds     dS without the factor 1/8
        img_head_swap   img = block % heads, h = block / heads
        dbias_k_from_v  the K third of dbias takes the V sums"""
    assert mutant is None or mutant in MUTANTS
    D = heads * 64
    ld = 3 * D
    qf, dof = qkv.float().reshape(-1), dout.float().reshape(-1)
    out = torch.full((n * L * D,), float("nan"))
    dqkv = torch.full((n * L * ld,), float("nan"))
    bseg = heads * n * 64
    part = torch.zeros(3 * bseg)
    Lk = L + 1 if mutant == "key_mask" else L
    for b in range(n * heads):
        img, h = (b % heads, b // heads) if mutant == "img_head_swap" else (b // heads, b % heads)
        qb = img * L * ld + h * 64
        q, k, v = _gather(qf, qb, L, ld), _gather(qf, qb + D, Lk, ld), _gather(qf, qb + 2 * D, Lk, ld)
        do = _gather(dof, img * L * D + h * 64, L, D)
        s = (q @ k.t()) * SCALE
        if mutant == "no_max":
            e = torch.exp(s)
            p = e / e.sum(-1, keepdim=True)
        else:
            p = torch.softmax(s, dim=-1)
        p16 = p.to(dtype).float()
        _scatter(out, (img * L) * D + h * 64, L, D, (p16 @ v).to(dtype).float())
        dp = do @ v.t()
        ds = p * (dp - (p * dp).sum(-1, keepdim=True)) * (1.0 if mutant == "no_scale_ds" else SCALE)
        ds16 = ds.to(dtype).float()
        dq, dk, dv = ds16 @ k, (ds16.t() @ q)[:L], (p16.t() @ do)[:L]
        for t, g in enumerate((dq, dk, dv)):
            _scatter(dqkv, qb + t * D, L, ld, g.to(dtype).float())
        docol = do.sum(0)
        for t, colsum in enumerate((dq.sum(0), docol if mutant == "dbias_k_from_v" else torch.zeros(64), docol)):
            _scatter(part, t * bseg + (h * n + img) * 64, 1, 64, colsum[None])
    res = {"out": out.reshape(n * L, D).to(dtype), "dqkv": dqkv.reshape(n * L, ld).to(dtype)}
    if dbias_start is not None:
        res["dbias"] = dbias_start + part.reshape(3, heads, n, 64).sum(2).reshape(3 * D)
    return res


def dbias_start(heads):
    """what dbias holds before a call: non-zero, no two thirds alike"""
    return torch.from_numpy(ofill.fill(f"attn/dbias_start/{heads}", (3 * heads * 64,), std=1.0, mean=2.0))


def restatement_failures(c, mutant=None):
    """everything the comparison functions find wrong with restate32's results of case c"""
    n, L, heads = c["dims"]
    start = dbias_start(heads)
    r = restate32(c["qkv"], c["dout"], n, L, heads, c["dtype"], mutant, start)
    return (fwd_failures(r["out"], c["out"], c["vmax"], c["dtype"]) + bwd_failures(r["dqkv"], c["dqkv"], heads, c["dtype"])
            + dbias_failures(r["dbias"], c, start))


# ------------------------------------------------------------------------------------------------ the measurement
def measure():
    """{(kind, regime, quantity): largest rounding-model error / allowance over the tables, both dtypes}"""
    table = {}

    def fold(key, value):
        table[key] = max(table.get(key, 0.0), value)

    for regime, n, L, heads in vit_table():
        for dt in DTYPES:
            c = vit_case(regime, n, L, heads, dt)
            m = model_vit(c)
            a, b = fwd_ratios(m["out"], c["out"], c["vmax"], dt)
            fold(("vit", regime, "forward / 6 EPS16 max|v|"), a / FWD_ABS_V)
            fold(("vit", regime, "forward / (4 EPS16, 6 EPS16)"), b)
            a, b = bwd_ratios(m["dqkv"], c["dqkv"], heads, dt)
            fold(("vit", regime, "backward per third / 8 EPS16 max|ref|"), a / BWD_ABS_THIRD)
            fold(("vit", regime, "rel_rms / 3 EPS16"), b / BWD_REL_RMS)
            atol = DBIAS_ABS * EPS16[dt] * c["gscale"] * math.sqrt(n * L)
            fold(("vit", regime, "dbias / (1e-3, 8 EPS16 scale sqrt(n L))"),
                 float(((m["dbias"] - c["dbias"]).abs() / (atol + DBIAS_RTOL * c["dbias"].abs())).max()))
    for regime, n, L, heads in causal_table():
        for dt in DTYPES:
            c = causal_case(regime, n, L, heads, dt)
            a, _ = fwd_ratios(model_causal(c)["out"], c["out"], c["vmax"], dt)
            fold(("causal", regime, "forward / 6 EPS16 max|v|"), a / FWD_ABS_V)
    return table


if __name__ == "__main__":
    for (kind, regime, what), v in sorted(measure().items()):
        print(f"    {kind:6s} {regime:6s} {what:42s} {v:.3f}")
