"""Case tables, inputs, references, tolerances and comparison functions of the GEMM edge tests (tests/test_gpu_gemm_edges.py on the
GPU, tests/test_cpu_gemm_edges.py without one): eoe_gemm_nt (csrc/gemm.hip, gemm256.hip, gemm_w8.hip: ten routes behind launch_nt) and
eoe_gemm_tn / eoe_gemm_tn_grouped (csrc/gemm_tn.hip).

Inputs are pure functions of a name (oracle.fill), rounded to the 16-bit dtype first exactly as gpu_util.t16 does; the name holds the
dtype, because the magnitudes do (below).  Every reference sees the rounded values.

References.
  * nt_ref64: the contract of include/eoe_hip.h in fp64: v = acc alpha + bias, then NONE (C = v, C += v with `accumulate`), GELU (pre = v,
    act = gelu of pre ROUNDED to 16 bit), RESIDUAL (v + aux, aux fp32 at ldaux), GELU_BWD (v gelu'(aux), aux 16 bit at ldaux); column sums
    of the epilogue result added to what colsum held; colstats = (sum, sum of squares) of the result per 64 output rows.
    tn_ref64: C = [C +] alpha A^T B.
  * nt_model / tn_model, the ROUNDING MODEL: the same in fp64 with the kernels' documented roundings: v rounded to fp32, the 16-bit
    stores, fp32 C.  The column sums are taken from the fp32 values the epilogue holds BEFORE the 16-bit store (gemm_common.h: `cs[c] +=
    v[c]` stands in front of pack8 in all three epilogues), not from the stored ones.  CPU only: the yardstick of the input scales.
  * restate32: an fp32 restatement on flat, strided memory with canaries (operand reads behind a buffer's end give zero, as the kernels'
    buffer resources do; rows of A past M and rows of B past N are zero), with one deliberate error when `mutant` is named (MUTANTS).
    CPU only: the evidence that the comparison functions notice a subtly wrong kernel.

Magnitudes.  A has std 0.25; B has std sigma / (0.25 sqrt K) so that acc has std sigma whatever K is: sigma = 0.02 and bias std 0.02
(NONE, RESIDUAL), 0.0035 and 0.003 (GELU: the pre-activation's absolute allowance 1e-4 does not grow with K), 0.008 (GELU_BWD, whose saved
pre-activation has std 1).  All of them x 8 for fp16, whose EPS16 is 8 times smaller.  These follow from the one-third condition: a 16-bit
store alone is off by up to EPS16 |x|, which is a third of (2 EPS16 |x| + atol) only where |x| <= atol / EPS16.

Tolerances: all reused from tests/test_gpu_ops.py, none measured on a kernel.
  fp32 out      (2e-6, 2e-5 sqrt K)        test_gemm_nt_plain, line 60
  16-bit out    (2 EPS16, 1e-4 sqrt K)     test_gemm_nt_plain, line 63
  accumulate    (2e-6, 2e-5 sqrt K)        test_gemm_nt_plain, line 67
  residual      (2e-6, 1e-4)               test_gemm_nt_strided_and_epilogues, line 80
  GELU pre      (2 EPS16, 1e-4)            line 84
  GELU act      (2 EPS16, 1e-4) against gelu64 of the STORED pre-activation, line 85
  GELU_BWD      (2 EPS16, 2e-4)            line 91
  column sums   (1e-4, 1e-3) at M <= 256, line 92; atol x sqrt(M / 200) above (200 = the row count the figure was set at; an fp32 sum's
                error grows no faster for these inputs)
  colstats      (1e-5, 1e-4) sums, (1e-5, 1e-3) sums of squares, test_gemm_nt_colstats_and_bn_stats_partials, lines 113-114
  TN            (2e-6, 3e-5 sqrt T), line 143; (4e-6, 6e-5 sqrt T) after an accumulate, line 145
One check is not a reused tolerance but the number format itself: the GELU activation is the 16-bit value NEAREST to gelu of the stored
pre-activation, |act - gelu64(pre16)| <= half a 16-bit spacing at gelu64(pre16) plus 2^-16 relative for the fp32 evaluation (v_exp_f32 and
v_rcp_f32 are 1 ulp each: about 2^-21).  It is the only check that tells the activation of the unrounded pre-activation (mutant
gelu_unrounded) from the contract: that error is at most another half spacing, inside (2 EPS16, 1e-4) at any magnitude.
GELU without aux_out has no stored pre-activation to compare with: it must equal the pair's activation bit for bit.

The one-third condition (test_cpu_gemm_edges.test_rounding_model_uses_at_most_a_third_of_every_tolerance): over every case of the tables,
both dtypes, the rounding model's distance to fp64 is at most one third of each of these allowances.  It is a condition on the INPUTS: a
case that breaks it gets other input scales, the tolerance stays.

The tables (nt_table, tn_table).  Every route of the issue's table runs every M, N and K listed for it, every kind of list A that the route
admits, and both stride sets (minimal; lda = K + 64, ldb = K + 8, ldc = N + 8, ldaux = N + 16: all multiples of 8, which the fast epilogues
need).  The values are PAIRED CYCLICALLY, not multiplied out: every (M, N) pair of a route appears with both stride sets (the eight-wave
route: with these two and with lda = K + 64, ldc = N + 64), and along that list K and the kind are dealt out least-used-first (per N, then
per K, then overall), so that no kind or K is tied to one N and every kind meets every K the list has room for (the full product of the first row alone is 13 000 launches).  Every kind of
GENERIC_KINDS runs once through `epilogue_generic` on the two-workgroup, persistent and 160 x 256 x 32 routes, forced in turn by
N % 16 != 0 (not at N = 2048), by ldc % 8 != 0 and by a C pointer 8 bytes off; the GELU pair with each forcing.  Routes whose reach depends
on the CU count (the 160 x 256 x 32 kernel; the eight-wave kernel's fall-backs choose 128- or 160-row tiles by it) get M and the expected
code from `dispatch(case, ncu)`, a Python restatement of nt_route's conditions (gemm.hip) that only builds tables: the CPU tests hold it
against the real rule, asked through eoe_gemm_nt_route, on every row at 64 to 304 CUs, and the GPU tests assert that the route asked for is
the route that ran (`nt_last_kernel`).
The gather forms (the route "gather" of NT_KERNELS: the implicit patch matrix of a convolution, in eoe_gemm_nt and eoe_gemm_tn_grouped) are
outside these tables: tests/conv_gather_util.py has theirs, bitwise on integer inputs, with the data-movement kernels of csrc/conv.hip.
The wide-tile and stream-K TN forms need workload-sized groups (216 tiles of 256 x 128 on 256 CUs) and keep their present tests
(test_gemm_tn_wide_tiles, test_gemm_tn_grouped_stream_k); nothing here shrinks them.

Measured model error / allowance, the largest over the tables at 256 CUs (`python tests/gemm_util.py` prints these lines):
    nt 16-bit out / (2 EPS16, 1e-4 sqrt K)                   0.195
    nt GELU activation / (2 EPS16, 1e-4)                     0.189
    nt GELU pre-activation / (2 EPS16, 1e-4)                 0.274
    nt GELU_BWD / (2 EPS16, 2e-4)                            0.272
    nt accumulate / (2e-6, 2e-5 sqrt K)                      0.001
    nt colstats squares / (1e-5, 1e-3)                       0.000
    nt colstats sums / (1e-5, 1e-4)                          0.001
    nt column sums / (1e-4, 1e-3 sqrt(M / 200))              0.000
    nt fp32 out / (2e-6, 2e-5 sqrt K)                        0.000
    nt residual / (2e-6, 1e-4)                               0.001
    tn accumulate / (4e-6, 6e-5 sqrt T)                      0.002
    tn fp32 out / (2e-6, 3e-5 sqrt T)                        0.006
"""
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # `python tests/gemm_util.py`
from oracle import fill as ofill          # noqa: E402

EPS16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}          # tests/gpu_util.py
MANT16 = {torch.bfloat16: 7, torch.float16: 10}
MINEXP16 = {torch.bfloat16: -126, torch.float16: -14}
DTYPES = (torch.bfloat16, torch.float16)
DTNAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
PAD_ROWS = 5                                                             # canary / NaN rows around a view
CANARY32 = 12345.678                                                     # NaN-free: an add into it shows
CANARY16_BITS = 0x3E5B                                                   # a fixed, finite bit pattern in both 16-bit formats
DEFAULT_CUS = 256

# ------------------------------------------------------------------------------------------------ tolerances (sources: docstring)
TOL_F32 = (2e-6, 2e-5)                   # atol x sqrt K
TOL_16 = (2.0, 1e-4)                     # rtol x EPS16, atol x sqrt K
TOL_RES = (2e-6, 1e-4)
TOL_GELU = (2.0, 1e-4)                   # rtol x EPS16
TOL_GELU_BWD = (2.0, 2e-4)               # rtol x EPS16
TOL_COLSUM = (1e-4, 1e-3)                # atol x sqrt(M / 200) above M = 256
COLSUM_ROWS = 200
TOL_STATS = ((1e-5, 1e-4), (1e-5, 1e-3))
TOL_TN = (2e-6, 3e-5)                    # atol x sqrt T
TOL_TN_ACC = (4e-6, 6e-5)
NEAREST_SLOP = 2.0 ** -16

# EOE_NT_KERNEL_* of include/eoe_hip.h (eoe_amd._lib.NT_KERNELS mirrors them; test_cpu_gemm_edges compares the two lists with the header)
NT_KERNELS = ("none", "persistent_256x128", "persistent_256x96", "narrow_256x64", "persistent_narrow", "two_wg_128", "two_wg_160",
              "wide_160x256x32", "one_wave_160x256", "one_wave_256x256", "eight_wave", "eight_wave_stream_k", "split_k", "gather")
CODE = {n: i for i, n in enumerate(NT_KERNELS)}
TILE = {"persistent_256x128": (256, 128), "persistent_256x96": (256, 96), "narrow_256x64": (256, 64), "persistent_narrow": (256, 64),
        "two_wg_128": (128, 128), "two_wg_160": (160, 128), "wide_160x256x32": (160, 256), "one_wave_160x256": (160, 256),
        "one_wave_256x256": (256, 256), "eight_wave": (256, 256), "split_k": (128, 128)}
FLAGS = {"two_wg_128": 1 | 8 | 16, "two_wg_160": 1 | 8 | 32, "persistent_256x128": 1 | 4 | 64, "persistent_256x96": 1 | 4 | 48,
         "narrow_256x64": 1, "persistent_narrow": 1 | 4 | 64, "one_wave_160x256": 1 | 128, "one_wave_256x256": 1 | 256,
         "eight_wave": 1 | 262144, "wide_160x256x32": 1, "split_k": 1}

# kind -> (epilogue, 16-bit or fp32 C, bias, alpha, accumulate, aux_out kept, column sums: None / "ws" / "atomic", colstats)
KINDS = {
    "none_f32": ("none", "f32", False, 1.0, False, False, None, False),
    "none_f32_bias": ("none", "f32", True, 1.0, False, False, None, False),
    "none_16": ("none", "16", False, 1.0, False, False, None, False),
    "none_16_bias": ("none", "16", True, 1.0, False, False, None, False),
    "none_f32_alpha": ("none", "f32", True, 0.5, False, False, None, False),
    "none_16_alpha": ("none", "16", True, 0.5, False, False, None, False),
    "acc_bias": ("none", "f32", True, 1.0, True, False, None, False),
    "acc_alpha": ("none", "f32", False, 0.5, True, False, None, False),
    "residual_alpha": ("residual", "f32", True, 0.5, False, False, None, False),
    "residual": ("residual", "f32", True, 1.0, False, False, None, False),
    "gelu": ("gelu", "16", True, 1.0, False, True, None, False),
    "gelu_nopre": ("gelu", "16", True, 1.0, False, False, None, False),
    "gelu_nobias": ("gelu", "16", False, 1.0, False, True, None, False),
    "gelu_bwd_ws": ("gelu_bwd", "16", False, 1.0, False, False, "ws", False),
    "gelu_bwd_atomic": ("gelu_bwd", "16", False, 1.0, False, False, "atomic", False),
    "none_f32_colsum": ("none", "f32", True, 1.0, False, False, "ws", False),
    "colstats": ("none", "f32", True, 1.0, False, False, None, True),
}
LIST_A = ("none_f32", "none_f32_bias", "none_16", "none_16_bias", "none_f32_alpha", "none_16_alpha", "acc_bias", "residual_alpha", "gelu",
          "gelu_nopre", "gelu_bwd_ws", "gelu_bwd_atomic")
GENERIC_KINDS = ("none_16_bias", "acc_bias", "residual_alpha", "gelu", "gelu_bwd_ws", "gelu_bwd_atomic")        # each kind once through epilogue_generic
NARROW_KINDS = ("none_f32", "none_16", "none_f32_bias", "none_16_bias", "none_f32_alpha", "acc_bias", "colstats")
W8_KINDS = ("none_16_bias", "none_16", "gelu", "gelu_nopre")
W8_REFUSED = ("none_f32_bias", "acc_bias", "none_f32_colsum")                                                 # + K = 64
SPLITK_KINDS = ("none_16", "none_f32_bias", "residual")
EPI_CODE = {"none": 0, "gelu": 1, "residual": 2, "gelu_bwd": 3}


def kind_of(c):
    return dict(zip(("epi", "out", "bias", "alpha", "accumulate", "aux_out", "colsum", "colstats"), KINDS[c["kind"]]))


# ------------------------------------------------------------------------------------------------ the dispatcher's reach (tables only)
def fast_ok(c):
    """epilogue_fast_ok of gemm_common.h"""
    return c["N"] % 16 == 0 and c["ldc"] % 8 == 0 and c["ldaux"] % 8 == 0 and c["c_off_bytes"] % 16 == 0


def direct_ok(c):
    k = kind_of(c)
    if not fast_ok(c) or k["colstats"]:
        return False
    if k["epi"] in ("gelu", "gelu_bwd"):
        return k["out"] == "16"
    if k["epi"] == "residual":
        return k["out"] == "f32"
    return True


def w8_applies(c):
    k = kind_of(c)
    if k["epi"] not in ("none", "gelu") or k["out"] == "f32" or k["accumulate"] or k["colsum"] or k["colstats"] or c["split_k"]:
        return False
    if c["N"] % 256 or c["K"] // 64 < 2 or c["M"] < 256 or not fast_ok(c):
        return False
    return ((c["M"] - 1) * c["ldc"] + c["N"]) * 2 + 256 * c["ldc"] * 2 < 0x7fffffff and (c["M"] + 256) * c["lda"] * 2 + c["K"] * 2 < 0x7fffffff


def _cdiv(a, b):
    return -(-a // b)


def dispatch(c, ncu=DEFAULT_CUS):
    """nt_route of gemm.hip for gather == 0 without the opt-in stream-K bits: the name of the route (the gather branches:
    conv_gather_util.route_form)"""
    f, k = c["flags"], kind_of(c)
    M, N, K = c["M"], c["N"], c["K"]
    if k["epi"] == "none" and N <= 64:
        return "persistent_narrow" if f & 64 else "narrow_256x64"
    if f & (128 | 256) and direct_ok(c):
        return "one_wave_256x256" if f & 256 else "one_wave_160x256"
    big = K >= 4096 and N >= 2048
    if c["split_k"] and not (f & 8192 or M > 1024 or K // 64 < 24 or k["epi"] not in ("none", "residual") or k["colsum"] or k["colstats"]
                             or k["accumulate"] or N % 16 or c["ldc"] % 4 or (k["epi"] == "residual" and c["ldaux"] % 4)):
        nk, S = K // 64, 8
        while S > 1 and nk % S:
            S //= 2
        if S >= 2 and nk // S >= 3 and S * M * N <= 2 * ncu * 65536:
            return "split_k"
    if not f & (131072 | 4 | 8 | 512) and M >= 2048 and w8_applies(c):
        tiles = _cdiv(M, 256) * (N // 256)
        if f & 262144 or tiles * 100 >= _cdiv(tiles, ncu) * ncu * 85:
            return "eight_wave"
    if not f & (4096 | 4 | 8 | 512) and not k["colstats"] and N % 256 == 0 and N >= 2048 and K % 32 == 0 and M >= 2048:
        tiles, slots = _cdiv(M, 160) * (N // 256), 2 * ncu
        if tiles * 10 >= _cdiv(tiles, slots) * slots * 9:
            return "wide_160x256x32"
    gelu_wide = k["epi"] == "gelu" and N >= 2048 and K <= 1024 and not f & 1024
    if (f & 512 or gelu_wide) and not f & (4 | 8) and direct_ok(c) and M >= 2048 and N >= 512:
        cost = {mi: _cdiv(_cdiv(M, 32 * mi) * _cdiv(N, 256), ncu) * (mi * (K // 64 + 2) + 30) for mi in (5, 8)}
        return "one_wave_256x256" if cost[8] < cost[5] else "one_wave_160x256"
    if big and not f & (4 | 8) and direct_ok(c) and M >= 2048:
        return "one_wave_256x256"
    if not k["colstats"] and (f & 8 or (not big and not f & 4)):
        slots = 2 * ncu
        c4, c5 = _cdiv(_cdiv(M, 128) * _cdiv(N, 128), slots) * 128, _cdiv(_cdiv(M, 160) * _cdiv(N, 128), slots) * 160
        return "two_wg_160" if f & 32 or (not f & 16 and c5 <= c4) else "two_wg_128"
    t4, t3 = _cdiv(M, 256) * _cdiv(N, 128), _cdiv(M, 256) * _cdiv(N, 96)
    force = (f >> 4) & 7
    use3 = force == 3 if force else _cdiv(t3, ncu) * 3 * 10 <= _cdiv(t4, ncu) * 4 * 9
    return "persistent_256x96" if use3 else "persistent_256x128"


# ------------------------------------------------------------------------------------------------ case tables
def nt_case(route, kind, M, N, K, strides="min", flags=None, c_off_bytes=0, split_k=False, ncu=DEFAULT_CUS, **ld):
    """one row: route names the kernel the row is FOR (its flags); `expect` the route launch_nt takes (another one where the row is a
    refusal that must fall back)"""
    out16 = KINDS[kind][1] == "16"
    if strides == "min":
        d = dict(lda=K, ldb=K, ldc=N, ldaux=N)
    elif strides == "pad":
        d = dict(lda=K + 64, ldb=K + 8, ldc=N + 8, ldaux=N + 16)
    elif strides == "third":                         # the class-token-only block's pattern: one row in three
        d = dict(lda=3 * K, ldb=K, ldc=3 * N, ldaux=3 * N)
    elif strides == "w8":
        d = dict(lda=K + 64, ldb=K, ldc=N + 64, ldaux=N + 64)
    d.update(ld)
    if KINDS[kind][0] not in ("residual", "gelu_bwd"):
        d["ldaux"] = 0                                             # no aux: ops.gemm_nt passes 0
    c = dict(route=route, flags=FLAGS[route] if flags is None else flags, kind=kind, M=M, N=N, K=K, strides=strides,
             c_off_bytes=c_off_bytes, split_k=split_k, out16=out16, **d)
    c["expect"] = dispatch(c, ncu)
    c["code"] = CODE[c["expect"]]
    c["id"] = f"{route}-{kind}-{M}x{N}x{K}-{strides}-ldc{c['ldc']}" + (f"-off{c_off_bytes}" if c_off_bytes else "")
    return c


def _cycle(route, Ms, Ns, Ks, kinds, admit=lambda c: True, ncu=DEFAULT_CUS, stride_sets=("min", "pad"), **kw):
    """every (M, N) pair with every stride set.  K and the kind are dealt out least-used-first along that list: K the one this N has met
    least often, the kind (among those the route admits at the shape) the one that has met this N, then this K, then any row least
    often; ties go round in list order.  So no kind or K is tied to one N, and every kind meets every K the list has room for"""
    rows, j, used = [], 0, {}
    n = lambda *key: used.get(key, 0)                         # noqa: E731
    for strides in stride_sets:
        for M in Ms:
            for N in Ns:
                K = min(Ks, key=lambda K: (n("NK", N, K), n("K", K), (Ks.index(K) - j) % len(Ks)))
                cand = [c for c in (nt_case(route, kind, M, N, K, strides, ncu=ncu, **kw) for kind in kinds) if admit(c)]
                c = min(cand, key=lambda c: (n("kN", c["kind"], N), n("kK", c["kind"], K), n("k", c["kind"]), (kinds.index(c["kind"]) - j) % len(kinds)))
                for key in (("NK", N, K), ("K", K), ("kN", c["kind"], N), ("kK", c["kind"], K), ("k", c["kind"])):
                    used[key] = n(*key) + 1
                rows.append(c)
                j += 1
    return rows


def _generic(route, M, N, K, kinds, ncu=DEFAULT_CUS, n_odd=None):
    """each kind once through epilogue_generic: forced by N % 16 != 0, by ldc % 8 != 0, by a C pointer 8 bytes off"""
    rows = []
    for i, kind in enumerate(kinds):
        how = i % 3 if n_odd is not None else 1 + i % 2
        if how == 0:
            rows.append(nt_case(route, kind, M, n_odd, K, "min", ncu=ncu))
        elif how == 1:
            rows.append(nt_case(route, kind, M, N, K, "pad", ncu=ncu, ldc=N + 4))
        else:
            rows.append(nt_case(route, kind, M, N, K, "pad", ncu=ncu, c_off_bytes=8))
    # and every forcing once on the kind that writes two outputs
    if n_odd is not None:
        rows.append(nt_case(route, "gelu", M, n_odd, K, "min", ncu=ncu))
    rows.append(nt_case(route, "gelu", M, N, K, "pad", ncu=ncu, ldc=N + 4))
    rows.append(nt_case(route, "gelu", M, N, K, "pad", ncu=ncu, c_off_bytes=8))
    return rows


TWO_WG_M, TWO_WG_N, RING_K = (1, 63, 65, 81, 127, 129, 159, 161, 333), (72, 128, 136, 144, 264), (64, 128, 256)
PERS_M, PERS_N = (1, 255, 257, 300), (96, 104, 128, 200)
NARROW_M, NARROW_N, NARROW_K = (1, 255, 257, 600), (8, 24, 48, 64), (64, 192)
ONE_WAVE_M, ONE_WAVE_N = (159, 161, 257, 333), (16, 240, 256, 272)
W8_M, W8_N, W8_K = (2048, 2049, 2303, 2305), (256, 512), (128, 192, 256)
WIDE_N, WIDE_K = 2048, (64, 256)
SPLITK_M, SPLITK_N, SPLITK_K = (1, 7, 129, 1024), (16, 144, 768), (1536, 3072)
BIG_M = 2048                                    # from here on a case is compared with fp64 on sampled rows only


def wide_rows(ncu):
    """(ragged M, whole M) at which launch_nt's rule sends every kind of list A to the 160 x 256 x 32 kernel at N = 2048, or None: its
    tiles must fill >= 90 % of the 2 x #CU slots in every round, and the eight-wave kernel (>= 85 % of #CU 256 x 256 tiles) goes first"""
    for t in range(2 * ncu // (WIDE_N // 256), 12, -1):
        Ms = (t * 160 - 37, t * 160)
        if all(dispatch(nt_case("wide_160x256x32", kind, M, WIDE_N, 64, ncu=ncu), ncu) == "wide_160x256x32" for M in Ms for kind in LIST_A):
            return Ms
    return None


@functools.lru_cache(maxsize=None)
def nt_table(ncu=DEFAULT_CUS):
    """{route: [case, ...]}"""
    t = {}
    for route in ("two_wg_128", "two_wg_160"):
        t[route] = _cycle(route, TWO_WG_M, TWO_WG_N, RING_K, LIST_A, ncu=ncu)
        t[route] += _generic(route, 161, 144, 128, GENERIC_KINDS, ncu, n_odd=136)
    t["two_wg_128"] += [nt_case("two_wg_128", kind, M, 128, 128, "third", ncu=ncu) for M in (7, 130)
                        for kind in ("none_16_bias", "residual", "gelu", "gelu_bwd_ws")]
    for route in ("persistent_256x128", "persistent_256x96"):
        t[route] = _cycle(route, PERS_M, PERS_N, RING_K, LIST_A + ("colstats",),
                          admit=lambda c: c["kind"] != "colstats" or fast_ok(c), ncu=ncu)
        t[route] += [nt_case(route, "colstats", M, N, 128, s, ncu=ncu) for M, N, s in ((300, 96, "min"), (257, 128, "pad"))]
        t[route] += _generic(route, 257, 96, 128, GENERIC_KINDS, ncu, n_odd=104)
    for route in ("narrow_256x64", "persistent_narrow"):
        t[route] = _cycle(route, NARROW_M, NARROW_N, NARROW_K, NARROW_KINDS,
                          admit=lambda c: c["kind"] != "colstats" or fast_ok(c), ncu=ncu)
        t[route] += [nt_case(route, "colstats", M, N, 64, s, ncu=ncu) for M, N, s in ((600, 48, "min"), (257, 64, "pad"))]
    for route in ("one_wave_160x256", "one_wave_256x256"):
        t[route] = _cycle(route, ONE_WAVE_M, ONE_WAVE_N, RING_K, LIST_A,
                          admit=lambda c: c["expect"] == c["route"], ncu=ncu)
        t[route] += [nt_case(route, kind, 257, 272, 128, "pad", ncu=ncu) for kind in LIST_A if not any(c["kind"] == kind for c in t[route])]
        t[route].append(nt_case(route, "none_16_bias", 161, 264, 128, ncu=ncu))            # refused (N % 16): must fall back and be right
    # minimal, the general padded set, and lda = K + 64 with ldc = N + 64: eoe_w8_applies bounds a_reach and c_bytes by both
    t["eight_wave"] = _cycle("eight_wave", W8_M, W8_N, W8_K, W8_KINDS, ncu=ncu, stride_sets=("min", "pad", "w8"))
    t["eight_wave"] += [nt_case("eight_wave", kind, 2049, 256, 128, ncu=ncu) for kind in W8_REFUSED]
    t["eight_wave"].append(nt_case("eight_wave", "none_16_bias", 2049, 256, 64, ncu=ncu))
    Ms = wide_rows(ncu)
    t["wide_160x256x32"] = []
    if Ms:
        for i, kind in enumerate(LIST_A):
            t["wide_160x256x32"].append(nt_case("wide_160x256x32", kind, Ms[i % 2], WIDE_N, WIDE_K[(i // 2) % 2], ncu=ncu))
        t["wide_160x256x32"] += [nt_case("wide_160x256x32", kind, Ms[0], WIDE_N, 64, "pad", ncu=ncu) for kind in ("gelu", "gelu_bwd_ws", "residual_alpha")]
        t["wide_160x256x32"] += _generic("wide_160x256x32", Ms[0], WIDE_N, 64, GENERIC_KINDS, ncu)      # (N % 16 != 0 cannot reach this kernel)
    # N <= 64 without an epilogue is the narrow kernel's: RESIDUAL takes those shapes
    sk = _cycle("split_k", SPLITK_M, SPLITK_N, SPLITK_K, SPLITK_KINDS, admit=lambda c: c["expect"] == c["route"], ncu=ncu, split_k=True)
    sk += [nt_case("split_k", "none_16", 129, 144, 1472, split_k=True, ncu=ncu), nt_case("split_k", "residual", 1025, 144, 1536, "pad", split_k=True, ncu=ncu),
           nt_case("split_k", "residual", 129, 24, 1536, "pad", split_k=True, ncu=ncu)]
    t["split_k"] = sk
    return t


TN_T, TN_MN = (1, 63, 64, 65, 200), ((8, 8), (136, 264), (256, 128))
TN_FLAGS = (0, 2, 4)


def tn_case(T, M, N, strides, accumulate):
    d = dict(lda=M, ldb=N, ldc=N) if strides == "min" else dict(lda=M + 8, ldb=3 * N, ldc=N + 4)
    return dict(T=T, M=M, N=N, strides=strides, accumulate=accumulate, alpha=0.5 if accumulate else 1.0,
                id=f"tn-{T}x{M}x{N}-{strides}" + ("-acc" if accumulate else ""), **d)


def tn_table():
    return [tn_case(T, M, N, s, acc) for T in TN_T for M, N in TN_MN for s in ("min", "pad") for acc in (False, True)]


def tn_group():
    """one grouped launch mixing strided and contiguous problems (same T, accumulate, alpha)"""
    return [tn_case(65, 136, 264, "pad", False), tn_case(65, 256, 128, "min", False), tn_case(65, 8, 8, "pad", False)]


# ------------------------------------------------------------------------------------------------ inputs
def r16(name, shape, std, dtype, mean=0.0):
    """gpu_util.t16 without the upload"""
    return torch.from_numpy(ofill.fill(name, shape, std=std, mean=mean)).to(dtype)


def _f32(name, shape, std, mean=0.0):
    return torch.from_numpy(ofill.fill(name, shape, std=std, mean=mean))


SIGMA = {"none": (0.02, 0.02), "residual": (0.02, 0.02), "gelu": (0.0035, 0.003), "gelu_bwd": (0.008, 0.0)}       # (acc std, bias std)
A_STD = 0.25


@functools.lru_cache(maxsize=64)
def _nt_inputs(kind, M, N, K, dtype):
    k = dict(zip(("epi", "out", "bias", "alpha", "accumulate", "aux_out", "colsum", "colstats"), KINDS[kind]))
    f = 8.0 if dtype == torch.float16 else 1.0
    sig, sbias = SIGMA[k["epi"]]
    name = f"gemm/nt/{DTNAME[dtype]}/{k['epi']}/{M}x{N}x{K}"
    x = {"a": r16(name + "/a", (M, K), A_STD, dtype), "b": r16(name + "/b", (N, K), f * sig / (A_STD * math.sqrt(K)), dtype),
         "bias": _f32(name + "/bias", (N,), f * sbias, mean=f * sbias / 2) if k["bias"] else None, "aux": None, "c0": None, "colsum0": None}
    if k["epi"] == "residual":
        x["aux"] = _f32(name + "/res", (M, N), 1.0)
    if k["epi"] == "gelu_bwd":
        x["aux"] = r16(name + "/pre", (M, N), 1.0, dtype)
    if k["accumulate"]:
        x["c0"] = _f32(name + "/c0", (M, N), 1.0)
    if k["colsum"]:
        x["colsum0"] = _f32(name + "/colsum0", (N,), 1.0, mean=2.0)
    return x


def nt_inputs(c, dtype):
    """dense inputs of a case (nothing in them is ever modified): a [M, K], b [N, K] 16 bit; bias [N] fp32 or None; aux [M, N] (fp32
    residual / 16-bit saved pre-activation) or None; c0 [M, N] fp32 (accumulate) or None; colsum0 [N] or None"""
    return _nt_inputs(c["kind"], c["M"], c["N"], c["K"], dtype)


def tn_inputs(c, dtype):
    name = f"gemm/tn/{DTNAME[dtype]}/{c['T']}x{c['M']}x{c['N']}"
    return {"a": r16(name + "/a", (c["T"], c["M"]), 1.0, dtype), "b": r16(name + "/b", (c["T"], c["N"]), 1.0, dtype),
            "c0": _f32(name + "/c0", (c["M"], c["N"]), 1.0)}


# ------------------------------------------------------------------------------------------------ fp64 references and the rounding model
def gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_grad64(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


def _r16(x, dtype):
    return x.to(dtype).double()


def _r32(x):
    return x.float().double()


def _nt_eval(c, dtype, x, rows, model):
    k = kind_of(c)
    sel = slice(None) if rows is None else rows
    acc = x["a"][sel].double() @ x["b"].double().t()
    v = acc * k["alpha"] + (x["bias"].double() if k["bias"] else 0.0)
    if model:
        v = _r32(v)
    r = {}
    if k["epi"] == "gelu":
        r["pre"] = _r16(v, dtype) if model else v
        r["C"] = gelu64(_r16(v, dtype))                           # the contract: gelu of the ROUNDED pre-activation
        if model:
            r["C"] = _r16(r["C"], dtype)
        return r
    if k["epi"] == "residual":
        v = v + x["aux"][sel].double()
    if k["epi"] == "gelu_bwd":
        v = v * gelu_grad64(x["aux"][sel].double())
    if model:
        v = _r32(v)
    if rows is None:
        if k["colsum"]:
            r["colsum"] = x["colsum0"].double() + v.sum(0)
        if k["colstats"]:
            R = _cdiv(c["M"], 64)
            pad = torch.zeros(R * 64 - c["M"], c["N"], dtype=torch.float64)
            g = torch.cat([v, pad]).reshape(R, 64, c["N"])
            r["stats"] = torch.stack([g.sum(1), (g * g).sum(1)], dim=1)
    if k["accumulate"]:
        v = x["c0"][sel].double() + v
    r["C"] = (_r16(v, dtype) if k["out"] == "16" else _r32(v)) if model else v
    return r


def nt_ref64(c, dtype, rows=None):
    """{'C', 'pre' (GELU), 'colsum', 'stats' [ceil(M/64), 2, N]} in fp64; rows: only these rows of C / pre (no column sums then)"""
    return _nt_eval(c, dtype, nt_inputs(c, dtype), rows, False)


def nt_model(c, dtype, rows=None):
    return _nt_eval(c, dtype, nt_inputs(c, dtype), rows, True)


def tn_ref64(c, dtype, model=False):
    x = tn_inputs(c, dtype)
    v = c["alpha"] * (x["a"].double().t() @ x["b"].double())
    if model:
        v = _r32(v)
    if c["accumulate"]:
        v = x["c0"].double() + v
    return {"C": _r32(v) if model else v}


# ------------------------------------------------------------------------------------------------ flat, strided memory with canaries
def canary(n, kind):
    """n canary elements: fp32 -> CANARY32, 16-bit dtype -> the fixed bit pattern"""
    if kind == torch.float32:
        return torch.full((n,), CANARY32, dtype=torch.float32)
    return torch.full((n,), CANARY16_BITS, dtype=torch.int16).view(kind)


def layout(rows, cols, ld, off_elems=0):
    """(numel, start): a [rows, cols] view at leading dimension ld inside a flat buffer with PAD_ROWS rows of ld before and behind it"""
    start = PAD_ROWS * ld + off_elems
    return start + (rows - 1) * ld + cols + PAD_ROWS * ld + 8, start


def embed(dense, ld, fill, off_elems=0):
    """the flat buffer that holds `dense` at leading dimension ld: gaps and pad rows hold `fill` ('nan' for an input, 'canary' for an
    output that the kernel overwrites; an output the kernel adds into passes its start values as `dense`)"""
    rows, cols = dense.shape
    n, start = layout(rows, cols, ld, off_elems)
    flat = torch.full((n,), float("nan"), dtype=dense.dtype) if fill == "nan" else canary(n, dense.dtype)
    view = flat.as_strided((rows, cols), (ld, 1), start)
    view.copy_(dense)
    return flat, start


def view_of(flat, rows, cols, ld, start):
    return flat.as_strided((rows, cols), (ld, 1), start)


def canary_failures(flat, rows, cols, ld, start, what):
    """everything outside the [rows, cols] view must still hold the canary's bits"""
    want = canary(flat.numel(), flat.dtype)
    ne = bits(flat) != bits(want)
    view_of(ne, rows, cols, ld, start).fill_(False)
    if not bool(ne.any()):
        return []
    i = int(ne.nonzero()[0])
    r, col = divmod(i - start, ld) if i >= start else (-1 - (start - 1 - i) // ld, (i - start) % ld)
    return [f"canary:{what}: {int(ne.sum())} elements outside the view were written, first at row {r}, column {col}"]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------ comparing
def _d(t):
    return t.detach().float().cpu().double() if t.dtype != torch.float64 else t.detach().cpu()


def close_failures(what, got, ref, rtol, atol, frac=1.0):
    g, r = _d(got), _d(ref)
    if g.shape != r.shape:
        return [f"value:{what}: shape {tuple(g.shape)} for {tuple(r.shape)}"]
    if not bool(torch.isfinite(g).all()):
        return [f"value:{what}: non-finite values"]
    err, allow = (g - r).abs(), frac * (atol + rtol * r.abs())
    if bool((err > allow).any()):
        ratio = err / allow
        i = int(ratio.argmax())
        return [f"value:{what}: ({rtol:.3g}, {atol:.3g}) x {frac:.3g}: max err/allowance {float(ratio.max()):.3f} at flat index {i} "
                f"(err {float(err.flatten()[i]):.3e}), {int((err > allow).sum())} of {err.numel()} out"]
    return []


def ratio(got, ref, rtol, atol):
    g, r = _d(got), _d(ref)
    return float(((g - r).abs() / (atol + rtol * r.abs())).max()) if g.numel() else 0.0


def spacing16(x, dtype):
    """the distance between neighbouring 16-bit values around |x| (fp64 tensor)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -200))).clamp_min(MINEXP16[dtype])
    return torch.pow(2.0, e - MANT16[dtype])


def nearest_failures(act, pre16, dtype):
    """the activation is the 16-bit value nearest to gelu of the STORED pre-activation"""
    ref = gelu64(_d(pre16))
    err, allow = (_d(act) - ref).abs(), 0.5 * spacing16(ref, dtype) + NEAREST_SLOP * ref.abs()
    n = int((err > allow).sum())
    return [f"act_nearest: {n} of {err.numel()} activations are not the 16-bit value nearest to gelu(stored pre-activation); "
            f"max err / half spacing {float((err / allow).max()):.2f}"] if n else []


def colsum_atol(M):
    return TOL_COLSUM[1] * (math.sqrt(M / COLSUM_ROWS) if M > 256 else 1.0)


def nt_tols(c, dtype):
    """{'C': (rtol, atol), 'pre': ..., 'colsum': ..., 'stats0', 'stats1'} of a case"""
    k, eps, sk = kind_of(c), EPS16[dtype], math.sqrt(c["K"])
    t = {}
    if k["epi"] == "gelu":
        t["pre"] = (TOL_GELU[0] * eps, TOL_GELU[1])
        t["C"] = (TOL_GELU[0] * eps, TOL_GELU[1])
    elif k["epi"] == "residual":
        t["C"] = TOL_RES
    elif k["epi"] == "gelu_bwd":
        t["C"] = (TOL_GELU_BWD[0] * eps, TOL_GELU_BWD[1])
    elif k["out"] == "16":
        t["C"] = (TOL_16[0] * eps, TOL_16[1] * sk)
    else:
        t["C"] = (TOL_F32[0], TOL_F32[1] * sk)
    t["colsum"] = (TOL_COLSUM[0], colsum_atol(c["M"]))
    t["stats0"], t["stats1"] = TOL_STATS
    return t


def nt_failures(c, dtype, got, ref, frac=1.0, pair_act=None):
    """what is wrong with the results `got` of case c ({'C', 'pre', 'colsum', 'stats'}: dense tensors, `ref` from nt_ref64 on the same
    rows): [] if nothing.  pair_act: the activation of the same case with aux_out kept (kind gelu_nopre: must be equal bit for bit)"""
    k, t, bad = kind_of(c), nt_tols(c, dtype), []
    if k["epi"] == "gelu":
        if k["aux_out"]:
            bad += close_failures("pre", got["pre"], ref["pre"], *t["pre"], frac)
            if not bad:
                bad += close_failures("act", got["C"], gelu64(_d(got["pre"])), *t["C"], frac)
                bad += nearest_failures(got["C"], got["pre"], dtype)
        else:
            assert pair_act is not None, "GELU without aux_out is compared with the pair's activation"
            if not torch.equal(bits(got["C"]), bits(pair_act)):
                bad.append("value:act: GELU without aux_out differs in its bits from the pair's activation")
    else:
        bad += close_failures("C", got["C"], ref["C"], *t["C"], frac)
    if k["colsum"] and "colsum" in ref:
        bad += close_failures("colsum", got["colsum"], ref["colsum"], *t["colsum"], frac)
    if k["colstats"] and "stats" in ref:
        bad += close_failures("stats sums", got["stats"][:, 0], ref["stats"][:, 0], *t["stats0"], frac)
        bad += close_failures("stats squares", got["stats"][:, 1], ref["stats"][:, 1], *t["stats1"], frac)
    return bad


def tn_failures(c, got, ref, frac=1.0):
    rtol, a = TOL_TN_ACC if c["accumulate"] else TOL_TN
    return close_failures("C", got, ref["C"], rtol, a * math.sqrt(c["T"]), frac)


def sample_rows(M, tile_rows, seed):
    """the first and last 8 rows of every row-tile boundary plus 240 seeded random rows"""
    edges = [r for b in list(range(0, M, tile_rows)) + [M] for r in range(b - 8, b + 8) if 0 <= r < M]
    return torch.unique(torch.cat([torch.tensor(edges), torch.from_numpy(np.random.RandomState(seed).randint(0, M, 240))]))


# ------------------------------------------------------------------------------------------------ fp32 restatement and its mutants
MUTANTS = {                                       # name -> the check meant for it (the prefix of a failure line)
    "rows_past_m": "canary:C", "cols_past_n": "canary:C", "c_stride_n": "canary:C", "auxout_stride_n": "canary:aux_out",
    "res_at_ldc": "value:C", "pre_at_ldc": "value:C", "gelu_unrounded": "act_nearest", "alpha_after_bias": "value:C",
    "bias_off_by_one": "value:C", "acc_overwrites": "value:C", "colsum_overwrites": "value:colsum", "colsum_rows_past_m": "value:colsum",
    "colsum_last_part_dropped": "value:colsum", "k_last_dropped": "value:C", "k_first_twice": "value:C", "a_stride_k": "value:C",
    "tn_b_stride_n": "value:C", "tn_t_tail_dropped": "value:C"}


def _gather2(flat, start, rows, cols, ld):
    """[rows, cols] read from flat memory; behind the end (or in front of the start): zero"""
    idx = start + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]
    ok = (idx < flat.numel()) & (idx >= 0)
    return torch.where(ok, flat[idx.clamp(0, flat.numel() - 1)].float(), torch.zeros(()))


def _scatter2(flat, start, ld, val, rows_ok=None):
    rows, cols = val.shape
    idx = start + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]
    ok = idx < flat.numel()
    if rows_ok is not None:
        ok &= rows_ok[:, None]
    flat[idx[ok]] = val.to(flat.dtype)[ok]


def nt_memory(c, dtype):
    """the flat buffers of a case as the GPU test lays them out: {'a', 'b', 'aux', 'C', 'aux_out', 'colsum', 'bias'} -> (flat, start)"""
    k, x = kind_of(c), nt_inputs(c, dtype)
    M, N = c["M"], c["N"]
    odt = dtype if k["out"] == "16" else torch.float32
    coff = c["c_off_bytes"] // (2 if k["out"] == "16" else 4)
    m = {"a": embed(x["a"], c["lda"], "nan"), "b": embed(x["b"], c["ldb"], "nan")}
    if x["aux"] is not None:
        m["aux"] = embed(x["aux"], c["ldaux"], "nan")
    if k["accumulate"]:
        m["C"] = embed(x["c0"], c["ldc"], "canary", coff)
    else:
        n, start = layout(M, N, c["ldc"], coff)
        m["C"] = (canary(n, odt), start)
    if k["aux_out"]:
        n, start = layout(M, N, c["ldc"], coff)
        m["aux_out"] = (canary(n, dtype), start)
    if k["colsum"]:
        m["colsum"] = embed(x["colsum0"][None], N, "canary")
    if k["bias"]:
        m["bias"] = embed(x["bias"][None], N, "nan")
    return m


# ------------------------------------------------------------------------------------------------ the arguments of the C call
def sk_workspace_bytes(ncu):
    """EOE_NT_STREAMK_WORKSPACE_BYTES of include/eoe_hip.h"""
    return 8192 + ncu * 2 * 256 * 256 * 4


def nt_args(c, dtype, addr, sk_bytes):
    """the eoe_gemm_args of case c, filled as ops.gemm_nt fills them, for eoe_gemm_nt and eoe_gemm_nt_route alike.  addr: name -> address of
    the first element of 'a', 'b', 'C' and of what the kind has of 'bias', 'aux', 'aux_out', 'colsum', and of the workspaces 'colsum_ws' (the
    partial rows of a kind with column sums "ws"), 'colstats_ws' and 'sk_ws' (sk_bytes long; attached where ops.gemm_nt attaches it: with
    split_k, or at M >= 2048 and N % 256 == 0)"""
    from eoe_amd import _lib
    k, M, N = kind_of(c), c["M"], c["N"]
    has = lambda n, on: addr[n] if on else None               # noqa: E731
    g = _lib.GemmArgs(addr["a"], addr["b"], addr["C"], has("bias", k["bias"]), has("aux", k["epi"] in ("residual", "gelu_bwd")),
                      has("aux_out", k["aux_out"]), has("colsum", k["colsum"]), M, N, c["K"], c["lda"], c["ldb"], c["ldc"], c["ldaux"],
                      {torch.float16: _lib.EOE_F16, torch.bfloat16: _lib.EOE_BF16}[dtype], EPI_CODE[k["epi"]],
                      0 if k["out"] == "16" else 1, 1 if k["accumulate"] else 0, float(k["alpha"]))
    part_bytes = _cdiv(M, 64) * N * 4                           # EOE_NT_COLSUM_WORKSPACE_BYTES
    if k["colsum"] == "ws":
        g.workspace, g.workspace_bytes = addr["colsum_ws"], part_bytes
    if k["colstats"]:
        g.workspace, g.workspace_bytes, g.colstats = addr["colstats_ws"], 2 * part_bytes, 1
    g.split_k = 1 if c["split_k"] else 0
    if c["split_k"] or (M >= 2048 and N % 256 == 0):
        g.sk_workspace, g.sk_workspace_bytes = addr["sk_ws"], sk_bytes
    return g


def nt_starts(c, dtype):
    """name -> (first element, element size) of every view nt_memory lays out for case c, without building the buffers"""
    k = kind_of(c)
    M, N, K = c["M"], c["N"], c["K"]
    osz = 2 if k["out"] == "16" else 4
    coff = c["c_off_bytes"] // osz
    s = {"a": (layout(M, K, c["lda"])[1], 2), "b": (layout(N, K, c["ldb"])[1], 2), "C": (layout(M, N, c["ldc"], coff)[1], osz)}
    if k["epi"] in ("residual", "gelu_bwd"):
        s["aux"] = (layout(M, N, c["ldaux"])[1], 4 if k["epi"] == "residual" else 2)
    if k["aux_out"]:
        s["aux_out"] = (layout(M, N, c["ldc"], coff)[1], 2)
    if k["colsum"]:
        s["colsum"] = (layout(1, N, N)[1], 4)
    if k["bias"]:
        s["bias"] = (layout(1, N, N)[1], 4)
    return s


def fake_addresses(c, dtype, sk_off=0):
    """addresses for eoe_gemm_nt_route, which reads nothing behind them: every buffer of nt_memory at a 256-byte aligned base of its own, its
    view where nt_starts has it (so C is as far off 16 bytes as on the GPU); the workspaces aligned, the stream-K one sk_off bytes off"""
    addr = {n: (i + 1) << 32 | start * es for i, (n, (start, es)) in enumerate(sorted(nt_starts(c, dtype).items()))}
    addr.update(colsum_ws=20 << 32, colstats_ws=21 << 32, sk_ws=(22 << 32) + sk_off)
    return addr


def restate32(c, dtype, mem, mutant=None):
    """eoe_gemm_nt in fp32 on the flat buffers of nt_memory (C, aux_out and colsum are written in place), one deliberate error when
    `mutant` is named:
        rows_past_m              the rows >= M of the last row tile are stored
        cols_past_n              the columns >= N of the last column tile are stored
        c_stride_n               C written at stride N, not ldc
        auxout_stride_n          aux_out written at stride N, not ldc
        res_at_ldc               the residual read at ldc, not ldaux
        pre_at_ldc               GELU_BWD's saved pre-activation read at ldc, not ldaux
        gelu_unrounded           gelu of the fp32 pre-activation, not of its 16-bit rounding
        alpha_after_bias         (acc + bias) alpha
        bias_off_by_one          the bias of column n - 1 in the N tail (behind the last multiple of 16; the last 4 columns if there is none)
        acc_overwrites           accumulate stores v instead of C + v
        colsum_overwrites        colsum = sums instead of colsum += sums
        colsum_rows_past_m       the column sums run over the whole last row tile
        colsum_last_part_dropped the partial row of the last 64 output rows is left out
        k_last_dropped           the last 64-deep k-tile is not accumulated
        k_first_twice            the first k-tile is accumulated twice
        a_stride_k               A read at stride K, not lda
    returns {'stats'} for colstats"""
    assert mutant is None or mutant in MUTANTS
    k = kind_of(c)
    M, N, K = c["M"], c["N"], c["K"]
    tm, tn = TILE[c["expect"]]
    Mt, Nt = _cdiv(M, tm) * tm, _cdiv(N, tn) * tn
    a = _gather2(mem["a"][0], mem["a"][1], Mt, K, K if mutant == "a_stride_k" else c["lda"])
    a[M:] = 0.0                                                  # rows past M: behind the buffer resource's end
    b = _gather2(mem["b"][0], mem["b"][1], Nt, K, c["ldb"])
    b[N:] = 0.0
    k0, k1 = 0, (K - 64 if mutant == "k_last_dropped" else K)
    acc = a[:, k0:k1] @ b[:, k0:k1].t()
    if mutant == "k_first_twice":
        acc = acc + a[:, :64] @ b[:, :64].t()
    bias = torch.zeros(Nt)
    if k["bias"]:
        bias[:N] = mem["bias"][0][mem["bias"][1]:mem["bias"][1] + N]
        if mutant == "bias_off_by_one":
            t0 = N - N % 16 if N % 16 else N - 4
            bias[t0:N] = mem["bias"][0][mem["bias"][1] + t0 - 1:mem["bias"][1] + N - 1]
    alpha = torch.tensor(k["alpha"], dtype=torch.float32)
    v = (acc + bias) * alpha if mutant == "alpha_after_bias" else acc * alpha + bias
    rows_st = Mt if mutant == "rows_past_m" else M
    cols_st = Nt if mutant == "cols_past_n" else N
    ldc = N if mutant == "c_stride_n" else c["ldc"]
    Cf, Cs = mem["C"]
    res = {}
    if k["epi"] == "gelu":
        pre16 = v.to(dtype)
        src = v if mutant == "gelu_unrounded" else pre16.float()
        act = (src * torch.sigmoid(1.702 * src)).to(dtype)
        if k["aux_out"]:
            _scatter2(mem["aux_out"][0], mem["aux_out"][1], N if mutant == "auxout_stride_n" else c["ldc"], pre16[:rows_st, :cols_st])
        _scatter2(Cf, Cs, ldc, act[:rows_st, :cols_st])
        return res
    if k["epi"] == "residual":
        v = v + _gather2(mem["aux"][0], mem["aux"][1], Mt, Nt, c["ldc"] if mutant == "res_at_ldc" else c["ldaux"])
    if k["epi"] == "gelu_bwd":
        pre = _gather2(mem["aux"][0], mem["aux"][1], Mt, Nt, c["ldc"] if mutant == "pre_at_ldc" else c["ldaux"])
        s = torch.sigmoid(1.702 * pre)
        v = v * (s * (1 + 1.702 * pre * (1 - s)))
    if k["colsum"]:
        rows_cs = Mt if mutant == "colsum_rows_past_m" else M
        if mutant == "colsum_last_part_dropped":
            rows_cs = (_cdiv(M, 64) - 1) * 64
        sums = v[:rows_cs, :N].sum(0)
        cf, cs0 = mem["colsum"]
        cf[cs0:cs0 + N] = sums if mutant == "colsum_overwrites" else cf[cs0:cs0 + N] + sums
    if k["colstats"]:
        R = _cdiv(M, 64)
        g = torch.cat([v[:M, :N], torch.zeros(R * 64 - M, N)]).reshape(R, 64, N)
        res["stats"] = torch.stack([g.sum(1), (g * g).sum(1)], dim=1)
    if k["accumulate"] and mutant != "acc_overwrites":
        v = v + _gather2(Cf, Cs, Mt, Nt, ldc)
    _scatter2(Cf, Cs, ldc, v[:rows_st, :cols_st])
    return res


def nt_memory_failures(c, dtype, mem, extra=None, pair_act=None, rows=None):
    """canaries and values of the flat buffers after a launch (or a restatement) of case c"""
    k = kind_of(c)
    M, N = c["M"], c["N"]
    bad = canary_failures(*mem["C"][:1], M, N, c["ldc"], mem["C"][1], "C")
    got = {"C": view_of(mem["C"][0], M, N, c["ldc"], mem["C"][1])}
    if k["aux_out"]:
        bad += canary_failures(mem["aux_out"][0], M, N, c["ldc"], mem["aux_out"][1], "aux_out")
        got["pre"] = view_of(mem["aux_out"][0], M, N, c["ldc"], mem["aux_out"][1])
    if k["colsum"]:
        bad += canary_failures(mem["colsum"][0], 1, N, N, mem["colsum"][1], "colsum")
        got["colsum"] = mem["colsum"][0][mem["colsum"][1]:mem["colsum"][1] + N]
    if extra:
        got.update(extra)
    ref = nt_ref64(c, dtype, rows)
    if rows is not None:
        got = {n: (t[rows] if n in ("C", "pre") else t) for n, t in got.items()}
        pair_act = pair_act[rows] if pair_act is not None else None
        ref.update(nt_ref64_sums(c, dtype))
    return bad + nt_failures(c, dtype, got, ref, pair_act=pair_act)


@functools.lru_cache(maxsize=8)
def _sums_cached(kind, M, N, K, dtype):
    c = dict(kind=kind, M=M, N=N, K=K)
    r = _nt_eval(c, dtype, _nt_inputs(kind, M, N, K, dtype), None, False)
    return {n: r[n] for n in ("colsum", "stats") if n in r}


def nt_ref64_sums(c, dtype):
    """the fp64 column sums / colstats of a case that is otherwise compared on sampled rows"""
    k = kind_of(c)
    return _sums_cached(c["kind"], c["M"], c["N"], c["K"], dtype) if (k["colsum"] or k["colstats"]) else {}


def case_rows(c):
    """None (every row) below BIG_M, else the sampled rows a case is compared with fp64 on"""
    return sample_rows(c["M"], TILE[c["expect"]][0], c["M"] + c["N"]) if c["M"] >= BIG_M else None


def restatement_failures(c, dtype, mutant=None):
    """everything the comparison functions find wrong with restate32's results of case c (canaries everywhere; values on case_rows)"""
    mem = nt_memory(c, dtype)
    extra = restate32(c, dtype, mem, mutant)
    pair_act = None
    if c["kind"] == "gelu_nopre":
        pc = dict(c, kind="gelu")
        pm = nt_memory(pc, dtype)
        restate32(pc, dtype, pm, None)
        pair_act = view_of(pm["C"][0], c["M"], c["N"], c["ldc"], pm["C"][1])
    return nt_memory_failures(c, dtype, mem, extra, pair_act, case_rows(c))


def tn_memory(c, dtype):
    x = tn_inputs(c, dtype)
    m = {"a": embed(x["a"], c["lda"], "nan"), "b": embed(x["b"], c["ldb"], "nan")}
    if c["accumulate"]:
        m["C"] = embed(x["c0"], c["ldc"], "canary")
    else:
        n, start = layout(c["M"], c["N"], c["ldc"])
        m["C"] = (canary(n, torch.float32), start)
    return m


def tn_restate32(c, dtype, mem, mutant=None):
    """eoe_gemm_tn in fp32 on flat memory.  tn_b_stride_n: B read at stride N, not ldb; tn_t_tail_dropped: the rows of the reduction behind
    the last multiple of 64 are left out"""
    T, M, N = c["T"], c["M"], c["N"]
    a = _gather2(mem["a"][0], mem["a"][1], T, M, c["lda"])
    b = _gather2(mem["b"][0], mem["b"][1], T, N, N if mutant == "tn_b_stride_n" else c["ldb"])
    Tt = T - T % 64 if mutant == "tn_t_tail_dropped" else T
    v = torch.tensor(c["alpha"], dtype=torch.float32) * (a[:Tt].t() @ b[:Tt])
    if c["accumulate"]:
        v = v + _gather2(mem["C"][0], mem["C"][1], M, N, c["ldc"])
    _scatter2(mem["C"][0], mem["C"][1], c["ldc"], v)


def tn_memory_failures(c, dtype, mem):
    bad = canary_failures(mem["C"][0], c["M"], c["N"], c["ldc"], mem["C"][1], "C")
    return bad + tn_failures(c, view_of(mem["C"][0], c["M"], c["N"], c["ldc"], mem["C"][1]), tn_ref64(c, dtype))


def tn_restatement_failures(c, dtype, mutant=None):
    mem = tn_memory(c, dtype)
    tn_restate32(c, dtype, mem, mutant)
    return tn_memory_failures(c, dtype, mem)


# the case on which each mutant must be rejected (kind, M, N, K, strides of the two-workgroup 128-row route unless said otherwise)
def mutant_cases():
    two = lambda kind, M=161, N=136, K=128, s="pad", **kw: nt_case("two_wg_128", kind, M, N, K, s, **kw)          # noqa: E731
    return {"rows_past_m": [two("none_16_bias"), two("none_f32", s="min")], "cols_past_n": [two("none_16_bias"), two("gelu")],
            "c_stride_n": [two("none_f32_bias"), two("gelu")], "auxout_stride_n": [two("gelu")],
            "res_at_ldc": [two("residual_alpha")], "pre_at_ldc": [two("gelu_bwd_ws")],
            "gelu_unrounded": [two("gelu"), two("gelu", s="min", N=144)], "alpha_after_bias": [two("none_f32_alpha"), two("residual_alpha")],
            "bias_off_by_one": [two("none_16_bias"), two("none_f32_bias", N=144)], "acc_overwrites": [two("acc_bias")],
            "colsum_overwrites": [two("gelu_bwd_ws"), two("gelu_bwd_atomic")], "colsum_rows_past_m": [two("gelu_bwd_ws"), two("none_f32_colsum")],
            "colsum_last_part_dropped": [two("gelu_bwd_ws"), two("gelu_bwd_ws", M=129)],
            "k_last_dropped": [two("none_16_bias", K=256), two("none_f32", K=64)], "k_first_twice": [two("none_16_bias", K=256), two("gelu_bwd_ws")],
            "a_stride_k": [two("none_16_bias"), nt_case("two_wg_128", "none_16_bias", 7, 128, 128, "third")],
            "tn_b_stride_n": [tn_case(65, 136, 264, "pad", False), tn_case(63, 8, 8, "pad", True)],
            "tn_t_tail_dropped": [tn_case(65, 136, 264, "pad", False), tn_case(63, 8, 8, "min", False), tn_case(200, 256, 128, "min", True)]}


# ------------------------------------------------------------------------------------------------ the measurement
def measure(ncu=DEFAULT_CUS, big=True):
    """{quantity: largest rounding-model error / allowance over the tables, both dtypes}"""
    table = {}

    def fold(key, value):
        table[key] = max(table.get(key, 0.0), value)

    for cases in nt_table(ncu).values():
        for c in cases:
            if c["M"] >= BIG_M and not big:
                continue
            rows = case_rows(c)
            for dt in DTYPES:
                k, t = kind_of(c), nt_tols(c, dt)
                m, r = nt_model(c, dt, rows), nt_ref64(c, dt, rows)
                if k["epi"] == "gelu":
                    fold("nt GELU pre-activation / (2 EPS16, 1e-4)", ratio(m["pre"], r["pre"], *t["pre"]))
                    fold("nt GELU activation / (2 EPS16, 1e-4)", ratio(m["C"], gelu64(m["pre"]), *t["C"]))
                else:
                    name = {"residual": "nt residual / (2e-6, 1e-4)", "gelu_bwd": "nt GELU_BWD / (2 EPS16, 2e-4)"}.get(
                        k["epi"], "nt accumulate / (2e-6, 2e-5 sqrt K)" if k["accumulate"] else
                        ("nt 16-bit out / (2 EPS16, 1e-4 sqrt K)" if k["out"] == "16" else "nt fp32 out / (2e-6, 2e-5 sqrt K)"))
                    fold(name, ratio(m["C"], r["C"], *t["C"]))
                if "colsum" in r:
                    fold("nt column sums / (1e-4, 1e-3 sqrt(M / 200))", ratio(m["colsum"], r["colsum"], *t["colsum"]))
                if "stats" in r:
                    fold("nt colstats sums / (1e-5, 1e-4)", ratio(m["stats"][:, 0], r["stats"][:, 0], *t["stats0"]))
                    fold("nt colstats squares / (1e-5, 1e-3)", ratio(m["stats"][:, 1], r["stats"][:, 1], *t["stats1"]))
    for c in tn_table():
        for dt in DTYPES:
            rtol, a = TOL_TN_ACC if c["accumulate"] else TOL_TN
            fold("tn accumulate / (4e-6, 6e-5 sqrt T)" if c["accumulate"] else "tn fp32 out / (2e-6, 3e-5 sqrt T)",
                 ratio(tn_ref64(c, dt, model=True)["C"], tn_ref64(c, dt)["C"], rtol, a * math.sqrt(c["T"])))
    return table


def measure_lines(ncu=DEFAULT_CUS):
    return [f"    {what:56s} {v:.3f}" for what, v in sorted(measure(ncu).items())]


if __name__ == "__main__":
    print("\n".join(measure_lines()))
