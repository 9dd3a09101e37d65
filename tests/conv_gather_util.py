"""Case tables, inputs and references of the convolution front end's edge tests (tests/test_gpu_conv_gather.py on the GPU,
tests/test_cpu_conv_gather.py without one): the implicit patch matrix of eoe_gemm_nt (csrc/gemm.hip: gather modes 1, 2 and the narrow
mode 3 over gemm_nt64_kernel, gemm_nt128_kernel and the persistent gemm_nt_kernel), of eoe_gemm_tn_grouped (csrc/gemm_tn.hip: modes 1 and
2, split over T or not) and the data-movement entry points of csrc/conv.hip.  tests/gemm_util.py has the GEMMs without gather.

Everything here is ADDRESSING, and addressing is compared BITWISE.  Inputs are small integers (activations, weights and dy in -2 .. 2,
pure functions of a name through oracle.fill.fill_int), exact in both 16-bit types; every product and partial sum is then an integer (a
multiple of 0.5 with alpha = 0.5) below 2^24, so the fp32 accumulators are exact in any summation order and the expected output is known
to the bit.  The exactness condition -- for every accumulator the kernels form, the sum of |terms| < 2^24: |A| |B| of the GEMM, the prior C
of `accumulate`, the colstats sums and sums of squares per 64 rows, the col2im tap sums, the TN partials -- is asserted on the CPU for every
case of every table (exactness_failures).  16-bit outputs are the round-to-nearest-even of the exact value.  Images of the mean / std paths
take mean in small integers and std in powers of two: (v - mean) / std is exact in fp32 and its 16-bit rounding is the only rounding.

The reference is `unfold`: patch[(img, ho, wo), (ky kw + kx) cpad + c] = x[img, ho s + ky - p, wo s + kx - p, c] or 0, written from that
definition in int64 numpy, then a matrix product; test_cpu_conv_gather holds it against torch.nn.functional.conv2d in fp64.  It calls
neither the kernels nor oracle code derived from them.  `mutant` names one deliberate error (MUTANTS); `applies` says, from the geometry
alone, whether a mutant can change a case, and the CPU tier asserts that it then DOES change the expected output, and that every kernel
of the tables has a case for every mutant of its family (kernel_mutants).

The identity probe: the activation holds a position code (a hash of (img, h, w, c) in +-1 .. 120, never 0), the other operand is
one-hot (NT: weight row j = unit vector at column k0 + j; TN: dy row t0 + j = unit vector j), so the output IS the implicit patch matrix,
window by window; it is compared bitwise with the unfold and with eoe_im2col's output for the same geometry.

Memory is laid out as gemm_util lays it out (flat buffers, PAD_ROWS canary rows around every output, canaries in every stride gap, NaN
around and between the rows of every input).  Inside K, the narrow mode's B columns behind kh kw C hold the finite value B_TAIL (3), not
zero and not NaN: the implicit A must deliver zeros there by itself (0 x NaN is NaN in an MFMA, so NaN cannot stand inside K).

Mode 2 (the packed 3-channel first layer) reads the physically padded NHWC4 image of eoe_stem_pack_image through a window of
2 ceil(kh / 2) rows x 8 pixels x 4 channels without masks (the packed weights are zero where ky >= kh, kx >= kw, c = 3): its patch
matrix is `unfold` of the padded image with that window and pad 0, on the Ho x Wo grid of the layer.

Findings: none so far -- every case of these tables passed bit for bit on its first run on an MI355X (256 CUs); no kernel was changed.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_util as gu          # noqa: E402
from oracle import fill as ofill          # noqa: E402

DTYPES, DTNAME, DEFAULT_CUS = gu.DTYPES, gu.DTNAME, gu.DEFAULT_CUS
EXACT = 1 << 24
B_TAIL = 3
NT_FLAGS_BASE = 1                 # EOE_NT_DEFAULT_FLAGS (gemm_util.FLAGS carries the same bit 0 in every entry)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ geometries
# name -> (kh, kw, stride, pad, H, W): the issue's list; every map but the single pixel has H != W
GEOS = {"3s1_9x7": (3, 3, 1, 1, 9, 7), "3s2_10x13": (3, 3, 2, 1, 10, 13), "5s1_6x11": (5, 5, 1, 2, 6, 11), "1s2_9x6": (1, 1, 2, 0, 9, 6),
        "7s2_14x10": (7, 7, 2, 3, 14, 10), "3s1_1x5": (3, 3, 1, 1, 1, 5), "3s1_5x1": (3, 3, 1, 1, 5, 1), "3s1_1x1": (3, 3, 1, 1, 1, 1),
        "3s3_11x8": (3, 3, 3, 1, 11, 8), "2x3s1_7x9": (2, 3, 1, 1, 7, 9), "4s1_6x5": (4, 4, 1, 1, 6, 5), "3s1_17x16": (3, 3, 1, 1, 17, 16)}
GEO_ORDER = ("3s1_9x7", "3s2_10x13", "5s1_6x11", "1s2_9x6", "7s2_14x10", "3s1_1x5", "3s1_5x1", "3s1_1x1", "3s3_11x8", "2x3s1_7x9")
assert all(H != W or H == 1 for (_, _, _, _, H, W) in GEOS.values())


def geo(name, n):
    kh, kw, s, p, H, W = GEOS[name]
    return dict(name=name, n=n, kh=kh, kw=kw, s=s, p=p, H=H, W=W, Ho=(H + 2 * p - kh) // s + 1, Wo=(W + 2 * p - kw) // s + 1)


def stem_geo(kh, kw, s, p, H, W, n, slack=(0, 0)):
    """the packed first layer: the layer's own geometry, the padded image (Hp, Wp as the header of eoe_stem_pack_image asks, plus
    `slack`) and `g2`, the geometry the gather-2 kernels see (pad 0, the 2 ceil(kh/2) x 8 window)"""
    Ho, Wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    khp = 2 * cdiv(kh, 2)
    Hp = max(H + p, (Ho - 1) * s + khp) + slack[0]
    Wp = max(W + p, (Wo - 1) * s + 8) + slack[1]
    Wp += Wp % 2
    g = dict(name=f"stem{kh}x{kw}s{s}_{H}x{W}", n=n, kh=kh, kw=kw, s=s, p=p, H=H, W=W, Ho=Ho, Wo=Wo, Hp=Hp, Wp=Wp)
    g["g2"] = dict(name=g["name"] + "/packed", n=n, kh=khp, kw=8, s=s, p=0, H=Hp, W=Wp, Ho=Ho, Wo=Wo, kh_arg=kh, kw_arg=kw)
    return g


# ------------------------------------------------------------------------------------------------ inputs
def ints(name, shape, lo=-2, hi=2):
    return ofill.fill_int("conv_gather/" + name, shape, lo, hi + 1)


def position_code(name, shape):
    """a hash of the flat index (= of (img, h, w, c)) in +-(1 .. 120): never 0, so a zero in the output is a padding tap"""
    return ofill.fill_int("conv_gather/code/" + name, shape, 1, 121) * (2 * ofill.fill_int("conv_gather/sign/" + name, shape, 0, 2) - 1)


def t16(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).to(dtype)


def rne16(exact, dtype):
    """round-to-nearest-even of exact values (fp64 array, each exactly an fp32 number) to the 16-bit type"""
    f = exact.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), exact), "the exact value is no fp32 number"
    return torch.from_numpy(f).to(dtype)


# ------------------------------------------------------------------------------------------------ the reference and its mutants
MUTANTS = ("hw_swapped", "howo_swapped", "pad_one_axis", "stride_one_axis", "kx_major", "wrap_lr", "img_square", "taps_reversed",
           "c_mod_cpad", "tail_nonzero")


def applies(mutant, g, C, cpad=None, Kp=None):
    """can this mutant change the patch matrix of geometry g at all (from the geometry alone, never from an outcome)"""
    taps, cp = g["kh"] * g["kw"], cpad or C
    # on a single pixel under a padded odd kernel the only tap that sees data is the centre one, a fixed point of both tap permutations
    centre_only = g["H"] * g["W"] == 1 and g["kh"] == g["kw"] == 2 * g["p"] + 1
    return {"hw_swapped": g["H"] != g["W"],
            "howo_swapped": g["Ho"] != g["Wo"],
            "pad_one_axis": g["p"] > 0,
            "stride_one_axis": g["s"] > 1 and g["Wo"] > 1,
            "kx_major": g["kh"] > 1 and g["kw"] > 1 and not centre_only,
            "wrap_lr": g["p"] > 0 and g["kw"] > 1 and g["n"] * g["H"] * g["W"] > 1,
            "img_square": g["Ho"] != g["Wo"] and (g["n"] >= 2 or g["Ho"] < g["Wo"]),
            "taps_reversed": taps > 1 and not centre_only,
            "c_mod_cpad": taps > 1,
            "tail_nonzero": (Kp or taps * cp) > taps * cp}[mutant]


def unfold(x, g, Kp=None, cpad=None, mutant=None, rows=None):
    """the patch matrix [n Ho Wo (or `rows`), Kp] of x [n, H, W, C] (int64) from the convolution's definition; column = tap cpad + c, zero
    for c >= C and behind the last tap.  mutant: one deliberate error --
        hw_swapped       the tensor addressed as [n, W, H, C]
        howo_swapped     the row decoded on a Wo x Ho grid
        pad_one_axis     the padding applied to h only
        stride_one_axis  the stride applied to h only
        kx_major         tap = kx kh + ky
        wrap_lr          a tap in the left / right padding reads the neighbouring row's pixel instead of 0
        img_square       img = row / (Ho Ho)
        taps_reversed    tap -> taps - 1 - tap
        c_mod_cpad       the column decoded with the other channel count (C where cpad is right, C + 1 where C is)
        tail_nonzero     the columns behind the last tap hold 1"""
    assert mutant is None or mutant in MUTANTS
    n, H, W, C = x.shape
    assert (n, H, W) == (g["n"], g["H"], g["W"])
    kh, kw, s, p, Ho, Wo = g["kh"], g["kw"], g["s"], g["p"], g["Ho"], g["Wo"]
    taps, cp = kh * kw, cpad or C
    if mutant == "c_mod_cpad":
        cp = C + 1 if cp == C else C
    Kp = Kp or taps * (cpad or C)
    m = np.arange(n * Ho * Wo, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    per = Ho * Ho if mutant == "img_square" else Ho * Wo
    img, rem = m // per, m % per
    dWo = Ho if mutant == "howo_swapped" else Wo
    ho, wo = rem // dWo, rem % dWo
    xH, xW = (W, H) if mutant == "hw_swapped" else (H, W)
    px = x.reshape(n * H * W, C)
    out = np.zeros((len(m), Kp), dtype=np.int64)
    if mutant == "tail_nonzero":
        out[:, min(Kp, taps * cp):] = 1
    cc = min(C, cp)
    for ky in range(kh):
        for kx in range(kw):
            tap = kx * kh + ky if mutant == "kx_major" else ky * kw + kx
            if mutant == "taps_reversed":
                tap = taps - 1 - tap
            h = ho * s + ky - p
            w = wo * (1 if mutant == "stride_one_axis" else s) + kx - (0 if mutant == "pad_one_axis" else p)
            ok = (h >= 0) & (h < xH) & (img < n)
            if mutant != "wrap_lr":
                ok &= (w >= 0) & (w < xW)
            pix = (img * xH + h) * xW + w
            ok &= (pix >= 0) & (pix < n * H * W)
            vals = np.where(ok[:, None], px[np.clip(pix, 0, n * H * W - 1), :cc], 0)
            c0 = tap * cp
            width = max(0, min(cc, Kp - c0))
            out[:, c0:c0 + width] = vals[:, :width]
    return out


def pack_ref(w, cpad, Kp, mutant=None):
    """eoe_conv_pack_weight from its contract: w [cout, cin, kh, kw] -> (w16 [cout, Kp], w16t [Kp, cout], w16d [cin taps, cout] with
    the taps REVERSED).  Mutants: kx_major, taps_reversed (w16 / w16t reversed, w16d not), c_mod_cpad, tail_nonzero"""
    cout, cin, kh, kw = w.shape
    taps = kh * kw
    cp = cpad
    if mutant == "c_mod_cpad":
        cp = cin + 1 if cpad == cin else cin
    w16 = np.zeros((cout, Kp), dtype=np.int64)
    if mutant == "tail_nonzero":
        w16[:, min(Kp, taps * cp):] = 1
    w16d = np.zeros((cin * taps, cout), dtype=np.int64)
    for ky in range(kh):
        for kx in range(kw):
            tap = kx * kh + ky if mutant == "kx_major" else ky * kw + kx
            td = taps - 1 - tap
            if mutant == "taps_reversed":
                tap, td = taps - 1 - tap, tap
            c0 = tap * cp
            width = max(0, min(cin, cp, Kp - c0))
            w16[:, c0:c0 + width] = w[:, :width, ky, kx]
            w16d[np.arange(cin) * taps + td, :] = w[:, :, ky, kx].T
    return w16, w16.T.copy(), w16d


def stem_pack_image_ref(x, g, cpad=4):
    """eoe_stem_pack_image from its contract: x [n, 3, H, W] (already normalised) -> [n, Hp, Wp, cpad], pixel (h, w) at (h + pad, w + pad)"""
    n, _, H, W = x.shape
    out = np.zeros((n, g["Hp"], g["Wp"], cpad), dtype=x.dtype)
    out[:, g["p"]:g["p"] + H, g["p"]:g["p"] + W, :3] = x.transpose(0, 2, 3, 1)
    return out


def stem_pack_weight_ref(w):
    """w [cout, 3, kh, kw] -> [cout, ceil(kh/2) 64], column = ky 32 + kx 4 + c"""
    cout, _, kh, kw = w.shape
    out = np.zeros((cout, cdiv(kh, 2) * 2, 8, 4), dtype=w.dtype)
    out[:, :kh, :kw, :3] = w.transpose(0, 2, 3, 1)
    return out.reshape(cout, -1)


def col2im_ref(dp, g, C):
    """dx [n, H, W, C] = the transpose of unfold applied to dp [n Ho Wo, >= taps C] (int64), tap by tap; and sum |terms|"""
    n, H, W = g["n"], g["H"], g["W"]
    dx, mag = np.zeros((n * H * W, C), dtype=np.int64), np.zeros((n * H * W, C), dtype=np.int64)
    m = np.arange(n * g["Ho"] * g["Wo"])
    img, rem = m // (g["Ho"] * g["Wo"]), m % (g["Ho"] * g["Wo"])
    ho, wo = rem // g["Wo"], rem % g["Wo"]
    for ky in range(g["kh"]):
        for kx in range(g["kw"]):
            h, w = ho * g["s"] + ky - g["p"], wo * g["s"] + kx - g["p"]
            ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            pix = ((img * H + h) * W + w)[ok]
            c0 = (ky * g["kw"] + kx) * C
            np.add.at(dx, pix, dp[ok, c0:c0 + C])
            np.add.at(mag, pix, np.abs(dp[ok, c0:c0 + C]))
    return dx.reshape(n, H, W, C), int(mag.max(initial=0))


# ------------------------------------------------------------------------------------------------ eoe_gemm_nt with gather: the tables
# kind -> (16-bit or fp32 C, bias, alpha, accumulate, colstats): the arguments ops.py passes with `gather`
KINDS = {"f32": ("f32", False, 1.0, False, False), "16": ("16", False, 1.0, False, False), "f32_bias": ("f32", True, 1.0, False, False),
         "16_bias": ("16", True, 1.0, False, False), "f32_alpha": ("f32", True, 0.5, False, False), "16_alpha": ("16", False, 0.5, False, False),
         "acc": ("f32", True, 1.0, True, False), "acc_alpha": ("f32", False, 0.5, True, False), "colstats": ("f32", True, 1.0, False, True),
         "colstats16": ("16", False, 1.0, False, True)}
KIND_LIST = ("f32", "16_bias", "acc", "colstats", "f32_alpha", "16", "acc_alpha", "colstats16", "f32_bias", "16_alpha")
# kernel -> (template, the nt_last_form it must report: mi 16 + ni, row tile)
KERNELS = {"nt64_g1": ("gemm_nt64_kernel<T,1>", 0, 256), "nt64_g2": ("gemm_nt64_kernel<T,2>", 0, 256),
           "nt128_mi4": ("gemm_nt128_kernel<T,NONE,4,1>", 64, 128), "nt128_mi5": ("gemm_nt128_kernel<T,NONE,5,1>", 80, 160),
           "pers_ni4_g1": ("gemm_nt_kernel<T,NONE,4,..,1>", 4, 256), "pers_ni2_g1": ("gemm_nt_kernel<T,NONE,2,..,1>", 2, 256),
           "pers_ni2_g2": ("gemm_nt_kernel<T,NONE,2,..,2>", 2, 256), "pers_ni4_g2": ("gemm_nt_kernel<T,NONE,4,..,2>", 4, 256),
           "pers_ni2_g3": ("gemm_nt_kernel<T,NONE,2,..,3>", 2, 256), "pers_ni4_g3": ("gemm_nt_kernel<T,NONE,4,..,3>", 4, 256)}
# the mutants that can apply to a kernel family (mode 2 has pad 0 and its own column order; c_mod_cpad is the pack kernels')
GATHER_MUTANTS = ("hw_swapped", "howo_swapped", "pad_one_axis", "stride_one_axis", "kx_major", "wrap_lr", "img_square", "taps_reversed")
STEM_MUTANTS = ("hw_swapped", "howo_swapped", "stride_one_axis", "kx_major", "img_square", "taps_reversed")
NARROW_MUTANTS = GATHER_MUTANTS + ("tail_nonzero",)


def kernel_mutants(kernel):
    """the mutants that can apply to a kernel of KERNELS"""
    return {"1": GATHER_MUTANTS, "2": STEM_MUTANTS, "3": NARROW_MUTANTS}[kernel[-1]] if kernel.startswith(("nt64", "pers")) else GATHER_MUTANTS
BIG_M = 2048                      # from here on a case is compared on sampled rows only (gemm_util.sample_rows)


def kind_of(c):
    return dict(zip(("out", "bias", "alpha", "accumulate", "colstats"), KINDS[c["kind"]]))


def nt128_rows_mi(M, N, ncu):
    """nt128_rows_mi(p, ncu, false) of gemm.hip"""
    slots = 2 * ncu
    c4, c5 = cdiv(cdiv(M, 128) * cdiv(N, 128), slots) * 128, cdiv(cdiv(M, 160) * cdiv(N, 128), slots) * 160
    return 5 if c5 < c4 else 4


def route_form(c, ncu=DEFAULT_CUS):
    """the gather branches of nt_route (gemm.hip) with the plain epilogue: (kernel name, mi 16 + ni)"""
    mode, N, f = c["mode"], c["N"], c["flags"]
    if N <= 64 and mode in (1, 2) and not f & 64:
        return f"nt64_g{mode}", 0
    if mode == 1 and N >= 128 and not f & 2048:
        mi = 4 if kind_of(c)["colstats"] else nt128_rows_mi(c["M"], N, ncu)
        return f"nt128_mi{mi}", mi * 16
    ni = 2 if N <= 64 else 4
    return f"pers_ni{ni}_g{mode}", ni


def nt_case(kernel, mode, g, C, N, kind, ldc_pad=False, flags=0, K=None, heavy=False, ncu=DEFAULT_CUS):
    gg = g["g2"] if mode == 2 else g                     # what the kernel sees
    taps = gg["kh"] * gg["kw"]
    Kmin = taps * C
    K = K or (cdiv(Kmin, 64) * 64 if mode == 3 else Kmin)
    c = dict(kernel=kernel, mode=mode, g=g, gg=gg, C=C, N=N, kind=kind, flags=NT_FLAGS_BASE | flags, K=K, Kmin=Kmin,
             M=gg["n"] * gg["Ho"] * gg["Wo"], ldb=K + 8 if ldc_pad else K, ldc=N + 8 if ldc_pad else N, heavy=heavy)
    c["expect"], c["form"] = route_form(c, ncu)
    c["id"] = f"{kernel}-{g['name']}-n{g['n']}-C{C}-N{N}-K{K}-{kind}-ldc{c['ldc']}"
    return c


def _kind_for(i, N, kinds=KIND_LIST):
    for j in range(len(kinds)):
        k = kinds[(i + j) % len(kinds)]
        if not KINDS[k][4] or N % 16 == 0:               # colstats needs N % 16 == 0
            return k


def _n_for(gname, target, tile):
    """a batch whose M passes `target` rows and ends inside an image relative to the row tile"""
    hw = geo(gname, 1)["Ho"] * geo(gname, 1)["Wo"]
    n = max(2, cdiv(target, hw))
    while (n * hw) % 32 == 0:
        n += 1
    return n


def _deal(kernel, mode, Cs, Ns, targets, geos=GEO_ORDER, flags=0, ncu=DEFAULT_CUS, first=0):
    """the geometries dealt out over C, N, the kinds, the M targets and the two stride sets cyclically"""
    tile, rows = KERNELS[kernel][2], []
    for i, gn in enumerate(geos, first):
        N = Ns[i % len(Ns)]
        rows.append(nt_case(kernel, mode, geo(gn, _n_for(gn, targets[i % len(targets)], tile)), Cs[i % len(Cs)], N, _kind_for(i, N),
                            ldc_pad=i % 2 == 1, flags=flags, ncu=ncu))
    return rows


# (kh, kw, stride, pad, H, W) of the packed first layer: kh in {3, 7, 8} (odd: half-empty last k-tile), kw in {3, 7, 8}, stride in {2, 4}
STEMS = ((3, 7, 2, 1, 10, 13), (7, 3, 4, 3, 21, 14), (8, 8, 2, 3, 13, 20), (7, 7, 2, 3, 14, 10), (3, 8, 4, 1, 9, 23), (8, 3, 2, 0, 12, 9))


def _stems(kernel, Ns, flags=0, ncu=DEFAULT_CUS, which=range(len(STEMS)), targets=(150, 300)):
    rows = []
    for i in which:
        kh, kw, s, p, H, W = STEMS[i]
        hw = ((H + 2 * p - kh) // s + 1) * ((W + 2 * p - kw) // s + 1)
        n = max(2, cdiv(targets[i % 2], hw))
        n += (n * hw) % 32 == 0
        N = Ns[i % len(Ns)]
        rows.append(nt_case(kernel, 2, stem_geo(kh, kw, s, p, H, W, n, slack=(i % 2, 2 * (i % 3 == 0))), 4, N, _kind_for(i, N),
                            ldc_pad=i % 2 == 1, flags=flags, ncu=ncu))
    return rows


def second_tile_rows(ncu, ni=4):
    """row tiles of 256 at N = 1024 so that the persistent kernel's tiles exceed its grid (persistent_grid = min(tiles, #CUs))"""
    return cdiv(ncu, 1024 // (32 * ni)) + 1


@functools.lru_cache(maxsize=None)
def nt_table(ncu=DEFAULT_CUS):
    """{kernel: [case, ...]}; `expect` / `form` come from route_form, which the CPU tier holds against eoe_gemm_nt_route"""
    t = {}
    t["nt64_g1"] = _deal("nt64_g1", 1, (64, 128), (8, 40, 64), (150, 300), ncu=ncu)
    t["nt64_g2"] = _stems("nt64_g2", (8, 40, 64), ncu=ncu)
    t["nt128_mi4"] = _deal("nt128_mi4", 1, (64, 128), (128, 136, 192), (100, 130, 200, 270, 350), ncu=ncu)
    # 160-row tiles need more 128-row tiles than the 2 x #CU slots hold: one case sized from the CU count (N = 256)
    n5 = cdiv(ncu * 128 + 1, 35)
    t["nt128_mi5"] = [nt_case("nt128_mi5", 1, geo("3s2_10x13", n5), 64, 256, "16_bias", heavy=True, ncu=ncu)]
    t["pers_ni4_g1"] = _deal("pers_ni4_g1", 1, (64, 128), (72, 96), (150, 300), ncu=ncu)
    t["pers_ni4_g1"] += _deal("pers_ni4_g1", 1, (64,), (128,), (300,), geos=("3s2_10x13", "2x3s1_7x9"), flags=2048, ncu=ncu, first=3)
    t["pers_ni2_g1"] = _deal("pers_ni2_g1", 1, (64,), (40, 64), (300,), geos=("3s2_10x13", "5s1_6x11"), flags=64, ncu=ncu)
    t["pers_ni2_g2"] = _stems("pers_ni2_g2", (64, 24), flags=64, ncu=ncu, which=(0, 1))
    t["pers_ni4_g2"] = _stems("pers_ni4_g2", (72,), ncu=ncu, which=(1, 2, 4))
    # narrow channels: every C with 3x3 and 5x5 (K rounded up to 64: tail taps), 4x4x8 = 128 (no tail), and one K a whole tile longer
    for kernel, Ns in (("pers_ni2_g3", (8, 40, 64)), ("pers_ni4_g3", (72, 128, 136))):
        rows = []
        for i, (gn, C) in enumerate([(gn, C) for C in (8, 16, 32) for gn in ("3s2_10x13", "5s1_6x11")] +
                                    [("4s1_6x5", 8), ("3s1_9x7", 8), ("2x3s1_7x9", 16), ("3s1_1x5", 32), ("3s1_5x1", 8), ("3s1_1x1", 16),
                                     ("3s3_11x8", 32), ("1s2_9x6", 8), ("7s2_14x10", 8)]):
            N = Ns[i % len(Ns)]
            g = geo(gn, _n_for(gn, (150, 300)[i % 2], 256))
            rows.append(nt_case(kernel, 3, g, C, N, _kind_for(i, N), ldc_pad=i % 2 == 1, ncu=ncu,
                                K=cdiv(g["kh"] * g["kw"] * C, 64) * 64 + 64 if gn == "3s1_9x7" else None))
        t[kernel] = rows
    # the persistent kernel's second tile per workgroup (the tap cursor restarts): modes 1, 2, 3 at N = 1024
    rt = second_tile_rows(ncu) * 256 - 250
    t["pers_ni4_g1"].append(nt_case("pers_ni4_g1", 1, geo("3s2_10x13", cdiv(rt, 35)), 64, 1024, "16_bias", flags=2048, heavy=True, ncu=ncu))
    t["pers_ni4_g2"].append(nt_case("pers_ni4_g2", 2, stem_geo(3, 7, 2, 1, 20, 27, cdiv(rt, 120)), 4, 1024, "16", heavy=True, ncu=ncu))
    t["pers_ni4_g3"].append(nt_case("pers_ni4_g3", 3, geo("3s2_10x13", cdiv(rt, 35)), 8, 1024, "16_bias", heavy=True, ncu=ncu))
    return t


def nt_cases(ncu=DEFAULT_CUS, heavy=None):
    return [c for cs in nt_table(ncu).values() for c in cs if heavy is None or c["heavy"] == heavy]


def case_rows(c):
    return gu.sample_rows(c["M"], KERNELS[c["expect"]][2], c["M"] + c["N"]).numpy() if c["M"] >= BIG_M else None


# ------------------------------------------------------------------------------------------------ eoe_gemm_nt with gather: inputs, expected
def stem_weight(c):
    g = c["g"]
    return ints(f"stemw/{g['name']}/{c['N']}", (c["N"], 3, g["kh"], g["kw"]))


@functools.lru_cache(maxsize=16)
def _nt_inputs(cid):
    c = _BY_ID[cid]
    g, gg, C, N, K = c["g"], c["gg"], c["C"], c["N"], c["K"]
    if c["mode"] == 2:
        a = stem_pack_image_ref(ints(f"img/{g['name']}/{g['n']}", (g["n"], 3, g["H"], g["W"])), g)
        b = stem_pack_weight_ref(stem_weight(c))
    else:
        a = ints(f"x/{g['name']}/{g['n']}/{C}", (g["n"], g["H"], g["W"], C))
        b = ints(f"w/{g['name']}/{N}/{K}", (N, K))
        b[:, c["Kmin"]:] = B_TAIL                             # inside K, behind the last tap: A must be zero there by itself
    return {"a": a, "b": b, "bias": ints(f"bias/{cid}", (N,)), "c0": ints(f"c0/{cid}", (c["M"], N)) if kind_of(c)["accumulate"] else None}


_BY_ID = {}


def nt_inputs(c):
    """int64 arrays: a = what the kernel's A pointer sees [n, H, W, C], b [N, K], bias [N], c0 [M, N]; never modified"""
    _BY_ID[c["id"]] = c
    return _nt_inputs(c["id"])


def nt_patch(c, x=None, rows=None, mutant=None):
    """the implicit patch matrix [M (or rows), K] of a case (of tensor x: default its own A)"""
    x = nt_inputs(c)["a"] if x is None else x
    return unfold(x, c["gg"], Kp=c["K"], mutant=mutant, rows=rows)


def nt_expected(c, rows=None, mutant=None):
    """{'C' exact fp64 [M (rows), N], 'mag': the largest sum of |terms| of any accumulator, 'stats' [ceil(M/64), 2, N]}"""
    k, x = kind_of(c), nt_inputs(c)
    p = nt_patch(c, rows=rows, mutant=mutant).astype(np.float64)
    b = x["b"].astype(np.float64)
    v = p @ b.T * k["alpha"] + (x["bias"] if k["bias"] else 0)
    mag = float((np.abs(p) @ np.abs(b).T).max()) * k["alpha"] + (float(np.abs(x["bias"]).max()) if k["bias"] else 0)
    r = {}
    if k["colstats"] and rows is None:
        R = cdiv(c["M"], 64)
        gq = np.concatenate([v, np.zeros((R * 64 - c["M"], c["N"]))]).reshape(R, 64, c["N"])
        r["stats"] = np.stack([gq.sum(1), (gq * gq).sum(1)], axis=1)
        mag = max(mag, float(np.abs(gq).sum(1).max()), float((gq * gq).sum(1).max()), float((gq * gq).max()))
    if k["accumulate"]:
        sel = slice(None) if rows is None else rows
        v = v + x["c0"][sel]
        mag += float(np.abs(x["c0"]).max())
    r["C"], r["mag"] = v, mag
    return r


def nt_memory(c, dtype):
    """the flat buffers of a case: {'a', 'b', 'C', 'bias'} -> (flat, start); inputs NaN-padded, C in canaries"""
    k, x = kind_of(c), nt_inputs(c)
    a = x["a"]
    m = {"a": gu.embed(t16(a.reshape(-1, max(8, a.shape[-1])), dtype), max(8, a.shape[-1]), "nan"), "b": gu.embed(t16(x["b"], dtype), c["ldb"], "nan")}
    odt = dtype if k["out"] == "16" else torch.float32
    if k["accumulate"]:
        m["C"] = gu.embed(torch.from_numpy(x["c0"].astype(np.float32)), c["ldc"], "canary")
    else:
        n, start = gu.layout(c["M"], c["N"], c["ldc"])
        m["C"] = (gu.canary(n, odt), start)
    if k["bias"]:
        m["bias"] = gu.embed(torch.from_numpy(x["bias"].astype(np.float32))[None], c["N"], "nan")
    return m


def geometry(gg, C):
    from eoe_amd import _lib
    # (mode 2: the layer's own kh, kw over the padded image, as ops.py passes them)
    return _lib.ConvGeometry(gg["n"], gg["H"], gg["W"], C, gg.get("kh_arg", gg["kh"]), gg.get("kw_arg", gg["kw"]), gg["s"], gg["p"], gg["Ho"],
                             gg["Wo"])


def nt_args(c, dtype, addr, N=None, out_f32=None, plain=False):
    """the eoe_gemm_args of a case as ops.py fills them for a convolution.  addr: 'a', 'b', 'C' (+ 'bias', 'colstats_ws');
    plain: no bias / alpha / accumulate / colstats (the identity probe, with its own N and an fp32 C)"""
    from eoe_amd import _lib
    k = kind_of(c)
    N = N or c["N"]
    f32 = (k["out"] == "f32") if out_f32 is None else out_f32
    g = _lib.GemmArgs(addr["a"], addr["b"], addr["C"], None if plain or not k["bias"] else addr["bias"], None, None, None,
                      c["M"], N, c["K"], 0, c["ldb"], N if plain else c["ldc"], 0,
                      {torch.float16: _lib.EOE_F16, torch.bfloat16: _lib.EOE_BF16}[dtype], 0, 1 if f32 else 0,
                      0 if plain else int(k["accumulate"]), 1.0 if plain else float(k["alpha"]))
    g.gather = 2 if c["mode"] == 2 else 1
    g.geo = geometry(c["gg"], c["C"])
    if k["colstats"] and not plain:
        g.workspace, g.workspace_bytes, g.colstats = addr["colstats_ws"], 2 * cdiv(c["M"], 64) * N * 4, 1
    return g


def fake_addr(c):
    return {"a": 1 << 32, "b": 2 << 32, "C": 3 << 32, "bias": 4 << 32, "colstats_ws": 5 << 32}


def nt_failures(c, dtype, mem, stats=None, rows=None):
    """canaries and bits of a case's outputs after a launch"""
    k = kind_of(c)
    M, N = c["M"], c["N"]
    bad = gu.canary_failures(mem["C"][0], M, N, c["ldc"], mem["C"][1], "C")
    got = gu.view_of(mem["C"][0], M, N, c["ldc"], mem["C"][1])
    exp = nt_expected(c, rows)
    want = rne16(exp["C"], dtype) if k["out"] == "16" else torch.from_numpy(exp["C"].astype(np.float32))
    if rows is not None:
        got = got[torch.from_numpy(rows)]
    ne = gu.bits(got) != gu.bits(want)
    if bool(ne.any()):
        i, j = (int(v) for v in ne.nonzero()[0])
        bad.append(f"bits:C: {int(ne.sum())} of {ne.numel()} differ, first at row {i if rows is None else int(rows[i])}, column {j}: "
                   f"{float(got[i, j])} for {float(want[i, j])}")
    if k["colstats"]:
        full = nt_expected(c) if rows is not None else exp
        ws = torch.from_numpy(full["stats"].astype(np.float32))
        if not torch.equal(gu.bits(stats), gu.bits(ws)):
            bad.append(f"bits:colstats: {int((gu.bits(stats) != gu.bits(ws)).sum())} of {ws.numel()} partial sums differ")
    return bad


def probe_windows(c, N):
    return list(range(0, c["K"], N))


def probe_b(c, k0, N, dtype):
    """weight row j = the unit vector at column k0 + j (rows past K: zero)"""
    b = torch.zeros(N, c["K"], dtype=dtype)
    j = torch.arange(min(N, c["K"] - k0))
    b[j, k0 + j] = 1
    return b


def probe_activation(c):
    """the position code in the layout the case's A pointer sees (mode 2: packed, border and channel 3 zero)"""
    g = c["g"]
    if c["mode"] == 2:
        return stem_pack_image_ref(position_code(c["id"], (g["n"], 3, g["H"], g["W"])), g)
    return position_code(c["id"], (g["n"], g["H"], g["W"], c["C"]))


# ------------------------------------------------------------------------------------------------ eoe_gemm_tn_grouped with gather
TN_TILE = (256, 128)              # BM x BN of gemm_tn_grouped_kernel


def tn_case(mode, g, C, N, accumulate=False, ws="none", ldc_pad=False, split=False):
    gg = g["g2"] if mode == 2 else g
    M = gg["kh"] * gg["kw"] * C
    T = gg["n"] * gg["Ho"] * gg["Wo"]
    c = dict(mode=mode, g=g, gg=gg, C=C, N=N, M=M, T=T, accumulate=accumulate, alpha=0.5 if accumulate else 1.0, ws=ws, split=split,
             ldb=N + 8 if ldc_pad else N, ldc=N + 4 if ldc_pad else N)
    c["id"] = f"tn{mode}-{g['name']}-n{g['n']}-C{C}-N{N}-{ws}" + ("-acc" if accumulate else "") + f"-ldc{c['ldc']}"
    return c


def tn_splits(c, ncu):
    """(splits, t_per_split) of eoe_gemm_tn_grouped for a single problem"""
    tiles, T, splits = cdiv(c["M"], TN_TILE[0]) * cdiv(c["N"], TN_TILE[1]), c["T"], 1
    if tiles * 8 < ncu * 5:
        splits = max(1, min(ncu // tiles, T // 512, 256))
    t_per = cdiv(cdiv(T, splits), 64) * 64
    return cdiv(T, t_per), t_per


@functools.lru_cache(maxsize=None)
def tn_table():
    rows = []
    Cs, Ns, targets = (8, 24, 64), (8, 64, 136), (40, 150, 64 * 3 + 9)
    for i, gn in enumerate(GEO_ORDER):
        hw = geo(gn, 1)["Ho"] * geo(gn, 1)["Wo"]
        n = max(2, cdiv(targets[i % 3], hw))
        n += (n * hw) % 64 == 0
        rows.append(tn_case(1, geo(gn, n), Cs[i % 3], Ns[(i + i // 3) % 3], accumulate=i % 3 == 2, ldc_pad=i % 2 == 1))
    rows.append(tn_case(1, geo("3s1_9x7", 3), 64, 136))                                   # M = 576: three column tiles of 256, the last partial
    for i, (kh, kw, s, p, H, W) in enumerate(STEMS):
        hw = ((H + 2 * p - kh) // s + 1) * ((W + 2 * p - kw) // s + 1)
        rows.append(tn_case(2, stem_geo(kh, kw, s, p, H, W, max(2, cdiv(targets[i % 3], hw)), slack=(i % 2, 2 * (i % 3 == 0))), 4, Ns[i % 3],
                            accumulate=i % 3 == 1, ldc_pad=i % 2 == 0))
    # split over T (T >= 1024 and few tiles): n = 4 on a 17 x 16 output; t_per_split = 576 is no multiple of 272
    g = geo("3s1_17x16", 4)
    rows += [tn_case(1, g, 8, 64, ws="ws", split=True), tn_case(1, g, 24, 8, ws="ws", accumulate=True, ldc_pad=True, split=True),
             tn_case(1, g, 8, 64, ws="unpack", split=True), tn_case(1, g, 24, 136, ws="unpack", accumulate=True, split=True),
             tn_case(1, g, 64, 64, ws="none", split=True), tn_case(1, g, 8, 136, ws="none", accumulate=True, ldc_pad=True, split=True),
             tn_case(2, stem_geo(3, 7, 2, 1, 33, 65, 2), 4, 64, ws="ws", split=True),
             tn_case(1, geo("3s1_9x7", 3), 8, 64, ws="unpack"), tn_case(1, geo("2x3s1_7x9", 2), 24, 8, ws="unpack", accumulate=True)]
    return rows


@functools.lru_cache(maxsize=16)
def _tn_inputs(cid):
    c = _BY_ID[cid]
    g = c["g"]
    if c["mode"] == 2:
        a = stem_pack_image_ref(ints(f"img/{g['name']}/{g['n']}", (g["n"], 3, g["H"], g["W"])), g)
    else:
        a = ints(f"x/{g['name']}/{g['n']}/{c['C']}", (g["n"], g["H"], g["W"], c["C"]))
    out_shape = (c["N"], c["C"], c["gg"]["kh"], c["gg"]["kw"]) if c["ws"] == "unpack" else (c["M"], c["N"])
    return {"a": a, "b": ints(f"dy/{cid}", (c["T"], c["N"])), "c0": ints(f"c0/{cid}", out_shape)}


def tn_inputs(c):
    _BY_ID[c["id"]] = c
    return _tn_inputs(c["id"])


def tn_expected(c, ncu=DEFAULT_CUS, mutant=None):
    """{'C' exact: [M, N], or with unpack_dw the weight gradient [cout, cin, kh, kw]; 'mag'}; the TN partials are sums over a subset of
    the same terms, so the bound over all of T covers every split"""
    x = tn_inputs(c)
    p = unfold(x["a"], c["gg"], mutant=mutant).astype(np.float64)
    b = x["b"].astype(np.float64)
    v = c["alpha"] * (p.T @ b)
    mag = c["alpha"] * float((np.abs(p).T @ np.abs(b)).max())
    if c["ws"] == "unpack":
        taps = c["gg"]["kh"] * c["gg"]["kw"]
        v = v.reshape(taps, c["C"], c["N"]).transpose(2, 1, 0).reshape(c["N"], c["C"], c["gg"]["kh"], c["gg"]["kw"])
    if c["accumulate"]:
        v = v + x["c0"]
        mag += float(np.abs(x["c0"]).max())
    return {"C": v, "mag": mag}


def tn_memory(c, dtype):
    x = tn_inputs(c)
    a = x["a"]
    m = {"a": gu.embed(t16(a.reshape(-1, max(8, a.shape[-1])), dtype), max(8, a.shape[-1]), "nan"), "b": gu.embed(t16(x["b"], dtype), c["ldb"], "nan")}
    rows, cols, ld = tn_out_view(c)
    if c["accumulate"]:
        m["C"] = gu.embed(torch.from_numpy(x["c0"].astype(np.float32)).reshape(rows, cols), ld, "canary")
    else:
        n, start = gu.layout(rows, cols, ld)
        m["C"] = (gu.canary(n, torch.float32), start)
    return m


def tn_out_view(c):
    """(rows, cols, ld) of the output: the [M, N] matrix at ldc, or unpack_dw's dense [cout, cin kh kw]"""
    return (c["N"], c["M"], c["M"]) if c["ws"] == "unpack" else (c["M"], c["N"], c["ldc"])


def tn_args(c, dtype, addr, ws_ptr, ws_bytes, N=None, plain=False):
    from eoe_amd import _lib
    N = N or c["N"]
    g = _lib.GemmArgs(addr["a"], addr["b"], addr["C"], None, None, None, None, c["M"], N, c["T"], 0, N if plain else c["ldb"],
                      N if plain else c["ldc"], 0, {torch.float16: _lib.EOE_F16, torch.bfloat16: _lib.EOE_BF16}[dtype], 0, 1,
                      0 if plain else int(c["accumulate"]), 1.0 if plain else c["alpha"])
    if c["ws"] != "none" and not plain:
        g.workspace, g.workspace_bytes = ws_ptr, ws_bytes
    g.gather = c["mode"]
    g.geo = geometry(c["gg"], c["C"])
    g.unpack_dw = 1 if (c["ws"] == "unpack" and not plain) else 0
    return g


def tn_failures(c, mem, ncu):
    rows, cols, ld = tn_out_view(c)
    bad = gu.canary_failures(mem["C"][0], rows, cols, ld, mem["C"][1], "C")
    got = gu.view_of(mem["C"][0], rows, cols, ld, mem["C"][1])
    want = torch.from_numpy(tn_expected(c, ncu)["C"].astype(np.float32)).reshape(rows, cols)
    ne = gu.bits(got) != gu.bits(want)
    if bool(ne.any()):
        i, j = (int(v) for v in ne.nonzero()[0])
        bad.append(f"bits:C: {int(ne.sum())} of {ne.numel()} differ, first at ({i}, {j}): {float(got[i, j])} for {float(want[i, j])}")
    return bad


# ------------------------------------------------------------------------------------------------ conv.hip entry points: the tables
def im2col_cases():
    """(kind, cin, geometry, Kp extra tiles, normalise)"""
    rows = []
    for i, gn in enumerate(GEO_ORDER):
        rows.append(dict(kind=1, cin=(1, 3, 5)[i % 3], g=geo(gn, 2 + i % 2), extra=64 * (i % 2), norm=i % 2 == 0))
        rows.append(dict(kind=(0, 2)[i % 2], cin=(8, 24, 64)[i % 3], g=geo(gn, 2 + i % 2), extra=64 * ((i + 1) % 2), norm=False))
    for r in rows:
        r["Kp"] = cdiv(r["g"]["kh"] * r["g"]["kw"] * r["cin"], 64) * 64 + r["extra"]
        r["id"] = f"im2col-kind{r['kind']}-cin{r['cin']}-{r['g']['name']}-Kp{r['Kp']}" + ("-norm" if r["norm"] else "")
    return rows


def norm_params(cin):
    """mean in small integers, std in powers of two: (v - mean) / std is exact in fp32"""
    return np.array([(c % 5) - 2 for c in range(cin)], dtype=np.float64), np.array([2.0 ** ((c % 3) - 1) for c in range(cin)])


def col2im_cases():
    rows = []
    for i, gn in enumerate(GEO_ORDER):
        C = (4, 12, 64)[i % 3]
        g = geo(gn, 2 + i % 2)
        rows.append(dict(g=g, C=C, Kp=g["kh"] * g["kw"] * C + (0, 8, 60)[i % 3], accumulate=i % 2,
                         id=f"col2im-{gn}-C{C}-acc{i % 2}"))
    return rows


def pack_jobs(count):
    """mixed shapes: cout in {8, 64, 72}, cin in {3, 8, 64} with cpad in {cin, 8, 64}, Kp with a 64-tile tail, w16t / w16d null or not"""
    shapes = [(8, 3, 8, 3, 3), (64, 8, 8, 5, 5), (72, 64, 64, 3, 3), (72, 3, 3, 2, 3), (8, 8, 64, 1, 1), (64, 3, 8, 7, 7), (72, 8, 8, 4, 4)]
    jobs = []
    for i in range(count):
        cout, cin, cpad, kh, kw = shapes[i % len(shapes)]
        jobs.append(dict(cout=cout, cin=cin, cpad=cpad, kh=kh, kw=kw, Kp=cdiv(kh * kw * cpad, 64) * 64 + 64 * (i % 2),
                         t=i % 4 in (0, 1), d=i % 4 in (0, 2), w=ints(f"packw/{i}", (cout, cin, kh, kw))))
    return jobs


# ------------------------------------------------------------------------------------------------ the exactness condition
def exactness_failures(ncu=DEFAULT_CUS):
    bad = []
    for c in nt_cases(ncu):
        rows = case_rows(c)
        e = nt_expected(c, rows)
        if rows is not None and kind_of(c)["colstats"]:
            e["mag"] = max(e["mag"], nt_expected(c)["mag"])
        if not e["mag"] < EXACT:
            bad.append((c["id"], e["mag"]))
    for c in tn_table():
        e = tn_expected(c, ncu)
        if not e["mag"] < EXACT:
            bad.append((c["id"], e["mag"]))
    for r in col2im_cases():
        dp = ints("dp/" + r["id"], (r["g"]["n"] * r["g"]["Ho"] * r["g"]["Wo"], r["Kp"]))
        mag = col2im_ref(dp, r["g"], r["C"])[1] + 2
        if not mag < EXACT:
            bad.append((r["id"], mag))
    return bad
