"""GPU: the CBAM gate kernels of csrc/cbam.hip -- eoe_cgate_fwd / _bwd, eoe_sgate_fwd / _bwd and the fused unit
eoe_cbam_junction_fwd / _bwd / _bwd_data -- against fp64, called through the C ABI on the current stream, at the shapes where they take
another path: every row-lane count of chan_reduce_kernel and HW on either side of its unrolled loop, Ch = 1 / odd / 256, n = 1 / 17 / 70
for the image slices, non-square maps and maps inside one 7 x 7 window, the padded plane of sgate_conv_bwd_weight_kernel at exactly
64 KiB and on either side of its stage, nz = 1 / 2 / 4 / 8 pixel slices with a short last one, second grid-stride rounds, every option
of the entry points, and planted ties.  Cases, references and tolerances: tests/cbam_util.py.  Every output and every scratch is
pre-filled with NaN and carries a guard of a sentinel past its end that must survive bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cbam_util as cu            # noqa: E402

NAN = float("nan")
SENTINEL = 12345.678
ISENTINEL = 0x5A5A5A5A
GUARD = 64
EOE_ERR_ARG = 1
SGATE_RED = 2 + 2 * 512                    # EOE_SGATE_RED
BN_SCRATCH_1 = (1024 + 3) * 2              # EOE_BN_SCRATCH(1)


@pytest.fixture(scope="module")
def L():
    from eoe_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def stream():
    import eoe_amd.ops as o
    return o._stream


def cu_(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def full(shape, value, dtype=torch.float32):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def p(t):
    return None if t is None else t.data_ptr()


def refused(L, rc):
    assert rc == EOE_ERR_ARG, rc
    assert L.lib.eoe_last_error()


class Bufs:
    """buffers whose body starts as NaN (integers: -1, or `fill`) and whose GUARD trailing elements hold a sentinel"""

    def __init__(self):
        self.items = []

    def new(self, shape, dtype=torch.float32, fill=None):
        numel = int(np.prod(shape))
        integer = dtype in (torch.int32, torch.int64)
        t = torch.empty(numel + GUARD, dtype=dtype, device="cuda")
        t[:numel] = fill if fill is not None else (-1 if integer else NAN)
        t[numel:] = ISENTINEL if integer else SENTINEL
        self.items.append((t, numel))
        return t[:numel].view(tuple(shape))

    def guards_intact(self):
        for t, numel in self.items:
            want = torch.full((GUARD,), ISENTINEL if t.dtype in (torch.int32, torch.int64) else SENTINEL, dtype=t.dtype, device="cuda")
            assert torch.equal(t[numel:], want), f"a write past the end of a {t.dtype} buffer of {numel} elements"

    def bodies_untouched(self, value=SENTINEL):
        for t, numel in self.items:
            v = ISENTINEL if t.dtype in (torch.int32, torch.int64) else value
            assert bool((t[:numel] == torch.tensor(v).to(t.dtype).item()).all())


def code(L, dtype):
    return 0 if dtype is None else L.EOE_F16 if dtype == torch.float16 else L.EOE_BF16


def weights(c):
    return {k: None if v is None else cu_(v) for k, v in c["w"].items()}


# ------------------------------------------------------------------------------------------------ argument blocks
def cgate_args(L, c, B, x, w):
    n, HW, Cc, Ch = c["n"], c["H"] * c["W"], c["C"], c["Ch"]
    s = {"pooled": B.new((n, 2, Cc)), "argmax_c": B.new((n, Cc), torch.int32), "hidden": B.new((n, 2, Ch)), "scale": B.new((n, Cc))}
    out = B.new((n, HW, Cc)) if c["part"] == "cgate" else None
    a = L.CGateArgs(p(x), p(out), p(w["w1"]), p(w["b1"]), p(w["w2"]), p(w["b2"]), p(s["pooled"]), p(s["argmax_c"]), p(s["hidden"]),
                    p(s["scale"]), n, HW, Cc, Ch)
    return a, s, out


def sgate_args(L, c, B, x, w, res=None, out16=None, dtype=None, out=True):
    n, H, W, Cc = c["n"], c["H"], c["W"], c["C"]
    s = {"comp": B.new((n, H * W, 2)), "argmax_p": B.new((n, H * W), torch.int32), "z": B.new((n, H * W)), "stats": B.new((2,)),
         "sp": B.new((n, H * W)), "rmean": B.new((1,), fill=cu.RM0), "rvar": B.new((1,), fill=cu.RV0),
         "nbt": B.new((1,), torch.int64, fill=cu.NBT0), "sums": B.new((BN_SCRATCH_1,))}
    o = B.new((n, H * W, Cc)) if out else None
    a = L.SGateArgs(p(x), p(o), p(w["w"]), p(w["gamma"]), p(w["beta"]), p(s["rmean"]), p(s["rvar"]), p(s["nbt"]), p(s["comp"]),
                    p(s["argmax_p"]), p(s["z"]), p(s["stats"]), p(s["sp"]), p(s["sums"]), n, H, W, Cc, cu.EPS_BN, cu.MOMENTUM,
                    int(c["training"]), p(res), p(out16), code(L, dtype))
    return a, s, o


def saved(s):
    """what the forward saved, under the reference's names"""
    got = {k: v for k, v in s.items() if k in ("pooled", "hidden", "scale", "comp", "z", "sp", "rmean", "rvar")}
    if "stats" in s:
        got.update(mean=s["stats"][0], rstd=s["stats"][1])
    return got


def check_saved(c, s, what):
    ref = c["ref"]
    cu.compare(what, saved(s), ref, c["specs"])
    for k in ("argmax_c", "argmax_p"):
        if k in s:
            assert torch.equal(s[k].cpu(), ref[k]), f"{what}: {k} differs in {int((s[k].cpu() != ref[k]).sum())} places"
    if "nbt" in s:
        assert int(s["nbt"].item()) == ref["nbt"]


# ------------------------------------------------------------------------------------------------ 1. the channel gate
@pytest.mark.parametrize("n,H,W,Cc,Ch", cu.CGATE_CASES)
def test_cgate(L, stream, n, H, W, Cc, Ch):
    """HW = 1; C = 16 / 32 (64 / 32 row lanes); HW = 63 / 64 / 65 around rpb = 64 and 127 / 128 / 129 around U * rpb = 128; HW = 3 below
    rpb = 4 (lanes at -inf with position 0 join the merge); Ch = 1, odd, 256; C = 4096; n = 17 and 70 over the 16 image slices of the
    weight-gradient kernel.  Everything saved, out, dx and the four parameter gradients; the positions of the maxima exactly"""
    c = cu.case("cgate", n, H, W, Cc, Ch, res=False)
    B, x, w = Bufs(), cu_(c["x"]), weights(c)
    a, s, out = cgate_args(L, c, B, x, w)
    L.check(L.lib.eoe_cgate_fwd(C.byref(a), stream()), "eoe_cgate_fwd")
    check_saved(c, s, f"cgate fwd {n}x{H}x{W}x{Cc}/{Ch}")
    cu.compare("cgate fwd", {"out": out}, c["ref"], c["specs"])
    HW = H * W
    g = {"dx": B.new((n, HW, Cc)), "dw1": B.new((Ch, Cc)), "db1": B.new((Ch,)), "dw2": B.new((Cc, Ch)), "db2": B.new((Cc,))}
    dscale, dpooled, dhidden, dout = B.new((n, Cc)), B.new((n, 2, Cc)), B.new((n, 2, Ch)), cu_(c["dout"])
    a.out = None
    b = L.CGateBwdArgs(a, p(dout), p(g["dx"]), p(dscale), p(dpooled), p(dhidden), p(g["dw1"]), p(g["db1"]), p(g["dw2"]), p(g["db2"]))
    L.check(L.lib.eoe_cgate_bwd(C.byref(b), stream()), "eoe_cgate_bwd")
    g["datt"] = dscale
    cu.compare("cgate bwd", g, c["ref"], c["specs"])
    B.guards_intact()


def test_cgate_refuses_and_writes_nothing(L, stream):
    """C below 16, above 4096, or with a thread-column count that does not divide 256 or C / 4; Ch = 0 and 257"""
    for Cc, Ch in [(Cc, 4) for Cc in cu.CGATE_REFUSED_C] + [(64, Ch) for Ch in cu.CGATE_REFUSED_CH]:
        assert not cu.cgate_accepts(Cc, Ch)
        n, HW, B = 2, 3, Bufs()
        t = [B.new(sh, dt, fill=ISENTINEL if dt == torch.int32 else SENTINEL) for sh, dt in
             (((n, HW, Cc), torch.float32), ((n, 2, Cc), torch.float32), ((n, Cc), torch.int32), ((n, 2, max(Ch, 1)), torch.float32),
              ((n, Cc), torch.float32), ((n, HW, Cc), torch.float32), ((max(Ch, 1), Cc), torch.float32), ((Cc,), torch.float32))]
        out, pooled, am, hidden, scale, dx, dw, db = t
        x, wt = full((n, HW, Cc), 1.0), full((Cc * 260,), 0.5)
        a = L.CGateArgs(p(x), p(out), p(wt), p(wt), p(wt), p(wt), p(pooled), p(am), p(hidden), p(scale), n, HW, Cc, Ch)
        refused(L, L.lib.eoe_cgate_fwd(C.byref(a), stream()))
        b = L.CGateBwdArgs(a, p(x), p(dx), p(scale), p(pooled), p(hidden), p(dw), p(db), p(dw), p(db))
        refused(L, L.lib.eoe_cgate_bwd(C.byref(b), stream()))
        torch.cuda.synchronize()
        B.bodies_untouched()
        B.guards_intact()


# ------------------------------------------------------------------------------------------------ 2. the spatial gate
def run_sgate(L, stream, c, what, dtypes):
    n, H, W, Cc = c["n"], c["H"], c["W"], c["C"]
    x, w, ref = cu_(c["x"]), weights(c), c["ref"]
    res = None if c["res"] is None else cu_(c["res"])
    for dtype in dtypes:
        B = Bufs()
        out16 = None if dtype is None else B.new((n, H * W, Cc), dtype)
        a, s, out = sgate_args(L, c, B, x, w, res, out16, dtype)
        L.check(L.lib.eoe_sgate_fwd(C.byref(a), stream()), "eoe_sgate_fwd")
        check_saved(c, s, f"sgate fwd {what} out16={dtype}")
        cu.compare("sgate fwd", {"out": out}, ref, c["specs"])
        if out16 is not None:
            assert torch.equal(out16, out.to(dtype)), "the 16-bit copy is not the fp32 output rounded"
        B.guards_intact()
    dout, affine = cu_(c["dout"]), c["affine"]
    got = {"dx": B.new((n, H * W, Cc)), "dw": B.new((98,))}
    if affine:
        got.update(dgamma=B.new((1,)), dbeta=B.new((1,)))
    if res is not None:
        got["g"] = B.new((n, H * W, Cc))
        L.check(L.lib.eoe_relu_bwd(p(dout), p(out), p(got["g"]), out.numel(), stream()), "eoe_relu_bwd")
        dout = got["g"]
    dscale, dcomp, red, wpart = B.new((n, H * W)), B.new((n, H * W, 2)), B.new((SGATE_RED,)), B.new((n, 98))
    a.out = a.running_mean = a.running_var = a.num_batches_tracked = a.res = a.out16 = None
    b = L.SGateBwdArgs(a, p(dout), p(got["dx"]), p(dscale), p(dcomp), p(red), p(got["dw"]), p(got.get("dgamma")), p(got.get("dbeta")),
                       p(wpart))
    L.check(L.lib.eoe_sgate_bwd(C.byref(b), stream()), "eoe_sgate_bwd")
    got["record"] = torch.cat([s["sp"][..., None], dcomp], 2)
    cu.compare(f"sgate bwd {what}", got, ref, c["specs"])
    assert bool(torch.isfinite(wpart).all())
    B.guards_intact()


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("n,H,W,Cc", cu.SGATE_SMALL)
def test_sgate_small(L, stream, n, H, W, Cc, res):
    """one pixel; 3 x 11 and 13 x 4 (rows and columns counted apart, the map narrower than the window one way); 6 x 6 inside one
    window; 7 x 7; C = 68 and 132 (a sub-lane's tail round).  Training and eval, affine and gamma = beta = NULL, with the residual
    junction (out16 bf16 / fp16 / NULL) and without; everything saved, out, g, dx, dw, dgamma, dbeta, the running buffers"""
    for training, affine in cu.sgate_options((n, H, W, Cc)):
        c = cu.case("sgate", n, H, W, Cc, 0, training, affine, res)
        run_sgate(L, stream, c, f"{n}x{H}x{W}x{Cc} train={training} affine={affine} res={res}", cu.DTYPES + (None,) if res else (None,))


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("n,H,W,Cc", cu.SGATE_LARGE)
def test_sgate_large(L, stream, n, H, W, Cc, res):
    """58 x 122: (H+6)(W+6) = 8192, exactly 64 KiB of dynamic LDS, non-square; 84 x 84 and 74 x 74: the padded plane larger than the
    stage that reuses it, 73 x 74 just below; n = 70 for the 64-image walk of sgate_wpart_sum_kernel; 300 x 84 x 84: a second
    grid-stride round in every pixel, conv, sigmoid and elementwise kernel and all 512 BatchNorm-backward partials"""
    c = cu.case("sgate", n, H, W, Cc, 0, True, True, res)
    run_sgate(L, stream, c, f"{n}x{H}x{W}x{Cc} res={res}", (torch.bfloat16,) if res else (None,))


def test_sgate_refuses_and_writes_nothing(L, stream):
    """58 x 123 by the backward only (the forward takes it); C = 6, H = 0, gamma without beta by both"""
    n, H, W, Cc = cu.SGATE_REFUSED_BWD
    c = cu.case("sgate", n, H, W, Cc, 0, True, True, False)
    B, x, w = Bufs(), cu_(c["x"]), weights(c)
    a, s, out = sgate_args(L, c, B, x, w)
    L.check(L.lib.eoe_sgate_fwd(C.byref(a), stream()), "eoe_sgate_fwd")
    check_saved(c, s, "sgate fwd 58x123")
    cu.compare("sgate fwd 58x123", {"out": out}, c["ref"], c["specs"])
    B.guards_intact()

    def attempt(n, H, W, Cc, gamma=True, beta=True, fwd=True):
        B2 = Bufs()
        px = max(n * H * W, 1)
        t = [B2.new(sh, dt, fill=ISENTINEL if dt != torch.float32 else SENTINEL) for sh, dt in
             (((px, Cc), torch.float32), ((px, 2), torch.float32), ((px,), torch.int32), ((px,), torch.float32), ((2,), torch.float32),
              ((px,), torch.float32), ((1,), torch.float32), ((1,), torch.float32), ((1,), torch.int64), ((px, Cc), torch.float32),
              ((98,), torch.float32), ((1,), torch.float32), ((1,), torch.float32), ((max(n, 1), 98), torch.float32),
              ((SGATE_RED,), torch.float32), ((px, 2), torch.float32), ((px,), torch.float32))]
        out, comp, am, z, stats, sp, rm, rv, nbt, dx, dw, dg, db, wpart, red, dcomp, dscale = t
        xx, sums, one = full((px, Cc), 1.0), full((BN_SCRATCH_1,), 0.0), full((1,), 1.0)
        a2 = L.SGateArgs(p(xx), p(out), p(w["w"]), p(one) if gamma else None, p(one) if beta else None, p(rm), p(rv), p(nbt), p(comp), p(am),
                         p(z), p(stats), p(sp), p(sums), n, H, W, Cc, cu.EPS_BN, cu.MOMENTUM, 1, None, None, 0)
        if fwd:
            refused(L, L.lib.eoe_sgate_fwd(C.byref(a2), stream()))
        b2 = L.SGateBwdArgs(a2, p(xx), p(dx), p(dscale), p(dcomp), p(red), p(dw), p(dg), p(db), p(wpart))
        refused(L, L.lib.eoe_sgate_bwd(C.byref(b2), stream()))
        torch.cuda.synchronize()
        B2.bodies_untouched()
        B2.guards_intact()

    attempt(n, H, W, Cc, fwd=False)
    attempt(2, 3, 5, 6)
    attempt(2, 0, 5, 4)
    attempt(2, 3, 5, 4, gamma=True, beta=False)


# ------------------------------------------------------------------------------------------------ 3. the fused unit
def fused_forward(L, stream, c, x, w, res, dtype):
    B = Bufs()
    n, HW, Cc = c["n"], c["H"] * c["W"], c["C"]
    out16 = None if dtype is None else B.new((n, HW, Cc), dtype)
    cg, s, _ = cgate_args(L, c, B, x, w)
    sg, s2, out = sgate_args(L, c, B, None, w, res, out16, dtype)
    s.update(s2)
    L.check(L.lib.eoe_cbam_junction_fwd(C.byref(cg), C.byref(sg), stream()), "eoe_cbam_junction_fwd")
    return B, cg, sg, s, out, out16


def fused_backward(L, stream, c, cg, sg, out, data_only):
    """(got, scratch) of eoe_cbam_junction_bwd or of its data-only form, every output and scratch NaN before the call"""
    B = Bufs()
    n, HW, Cc, Ch = c["n"], c["H"] * c["W"], c["C"], c["Ch"]
    dout = cu_(c["dout"])
    got = {"g": B.new((n, HW, Cc)), "dx": B.new((n, HW, Cc))}
    sc = {"dsc": B.new((cu.SLICES, n, Cc)), "dpooled": B.new((n, 2, Cc)), "dhidden": B.new((n, 2, Ch)), "dsp": B.new((n, HW)),
          "dcomp": B.new((n, HW, 4)), "red": B.new((SGATE_RED,))}
    sg.out = sg.running_mean = sg.running_var = sg.num_batches_tracked = sg.res = sg.out16 = None
    if data_only:
        L.check(L.lib.eoe_cbam_junction_bwd_data(C.byref(cg), C.byref(sg), p(dout), p(out), p(got["g"]), p(got["dx"]), p(sc["dsc"]),
                                                 p(sc["dpooled"]), p(sc["dhidden"]), p(sc["dsp"]), p(sc["dcomp"]), p(sc["red"]), stream()),
                "eoe_cbam_junction_bwd_data")
    else:
        got.update(dw1=B.new((Ch, Cc)), db1=B.new((Ch,)), dw2=B.new((Cc, Ch)), db2=B.new((Cc,)), dw=B.new((98,)))
        if c["affine"]:
            got.update(dgamma=B.new((1,)), dbeta=B.new((1,)))
        sc["wpart"] = B.new((n, 98))
        cb = L.CGateBwdArgs(cg, None, p(got["dx"]), p(sc["dsc"]), p(sc["dpooled"]), p(sc["dhidden"]), p(got["dw1"]), p(got["db1"]),
                            p(got["dw2"]), p(got["db2"]))
        sb = L.SGateBwdArgs(sg, None, None, p(sc["dsp"]), p(sc["dcomp"]), p(sc["red"]), p(got["dw"]), p(got.get("dgamma")),
                            p(got.get("dbeta")), p(sc["wpart"]))
        L.check(L.lib.eoe_cbam_junction_bwd(C.byref(cb), C.byref(sb), p(dout), p(out), p(got["g"]), stream()), "eoe_cbam_junction_bwd")
    return B, got, sc


def check_fused_scratch(c, got, sc, s):
    """the per-pixel record {sp, dcomp0, dcomp1, argmax bits}, datt in slice 0, the partial slices 1 .. nz - 1, and the slices past nz
    still NaN: none of them may leak into a result"""
    nz = c["nz"]
    got = dict(got)
    got["record"], got["datt"] = sc["dcomp"][..., :3], sc["dsc"][0]
    assert torch.equal(sc["dcomp"][..., 3].contiguous().view(torch.int32), s["argmax_p"])
    if nz > 1:
        part = {"slices": sc["dsc"][1:nz]}
        ref = {"slices": c["ref"]["slices"][1:]}
        spec = c["specs"]["slices"]
        cu.compare(f"fused slices nz={nz}", part, ref, {"slices": (spec[0], spec[1], cu._np64(spec[2])[1:])})
    assert bool(torch.isnan(sc["dsc"][nz:]).all()), "a dscale slice past nz was written"
    return got


def run_fused(L, stream, c, what, dtypes):
    x, res, w = cu_(c["x"]), cu_(c["res"]), weights(c)
    for dtype in dtypes:
        B, cg, sg, s, out, out16 = fused_forward(L, stream, c, x, w, res, dtype)
        check_saved(c, s, f"fused fwd {what} out16={dtype}")
        cu.compare("fused fwd", {"out": out}, c["ref"], c["specs"])
        if out16 is not None:
            assert torch.equal(out16, out.to(dtype)), "the 16-bit copy is not the fp32 output rounded"
        B.guards_intact()
    full_ok = cu.sgate_bwd_accepts(c["H"], c["W"])
    if full_ok:
        Bf, got, sc = fused_backward(L, stream, c, cg, sg, out, False)
        cu.compare(f"fused bwd {what}", check_fused_scratch(c, got, sc, s), c["ref"], c["specs"])
        assert bool(torch.isfinite(sc["wpart"]).all())
        Bf.guards_intact()
    Bd, gd, scd = fused_backward(L, stream, c, cg, sg, out, True)
    if full_ok:
        assert torch.equal(gd["g"], got["g"]) and torch.equal(gd["dx"], got["dx"]), "the data-only backward differs from the full one"
    cu.compare(f"fused data-only bwd {what}", check_fused_scratch(c, gd, scd, s), c["ref"], c["specs"])
    if not c["training"]:
        assert bool(torch.isnan(scd["red"]).all()), "the data-only backward over the running statistics must not touch red"
    Bd.guards_intact()


@pytest.mark.parametrize("n,H,W,Cc,Ch", cu.FUSED_CASES)
def test_cbam_junction(L, stream, n, H, W, Cc, Ch):
    """nz = 1 (15 and 49 pixels), 2 (8 x 16), 4 (16 x 16), 8 (16 x 32: 64 pixels a slice, 32 x 32: 128, 31 x 33: a short last slice,
    56 x 56: the network's map); n = 300 (nz held at 2 by the map, at 4 by n); C = 512; 45 x 56 x 56: a second round of the 16-lane
    pixel kernels.  Forward with out16 bf16 / fp16 / NULL, the full backward with every scratch NaN before it, and the data-only
    backward: g and dx bit-equal to the full one; over the running statistics as well on FUSED_EVAL"""
    for training in (True, False) if (n, H, W, Cc, Ch) in cu.FUSED_EVAL else (True,):
        c = cu.case("fused", n, H, W, Cc, Ch, training)
        run_fused(L, stream, c, f"{n}x{H}x{W}x{Cc}/{Ch} train={training}", cu.DTYPES + (None,) if c["regime"] == "small" else (torch.float16,))


def test_cbam_junction_without_gamma(L, stream):
    """gamma = beta = NULL: dgamma / dbeta not asked for"""
    c = cu.case("fused", *cu.FUSED_CASES[1], True, False)
    run_fused(L, stream, c, "affine=False", (torch.bfloat16,))


@pytest.mark.parametrize("training", [True, False])
def test_cbam_junction_data_only_above_the_lds_cap(L, stream, training):
    """58 x 123: the full backward refuses the map and writes nothing, the data-only form takes it -- against fp64, over the batch
    statistics and over the running statistics (sgate_bn_bwd_apply_kernel<true>)"""
    c = cu.case("fused", *cu.FUSED_DATA_ONLY, training)
    run_fused(L, stream, c, f"58x123 train={training}", (None,))
    n, HW, Cc, Ch = c["n"], c["H"] * c["W"], c["C"], c["Ch"]
    x, res, w = cu_(c["x"]), cu_(c["res"]), weights(c)
    B, cg, sg, s, out, _ = fused_forward(L, stream, c, x, w, res, None)
    B2 = Bufs()
    t = [B2.new(sh, fill=SENTINEL) for sh in ((n, HW, Cc), (n, HW, Cc), (cu.SLICES, n, Cc), (n, 2, Cc), (n, 2, Ch), (n, HW), (n, HW, 4),
                                               (SGATE_RED,), (Ch, Cc), (Ch,), (Cc, Ch), (Cc,), (98,), (1,), (1,), (n, 98))]
    g, dx, dsc, dpooled, dhidden, dsp, dcomp, red, dw1, db1, dw2, db2, dw, dg, db, wpart = t
    cb = L.CGateBwdArgs(cg, None, p(dx), p(dsc), p(dpooled), p(dhidden), p(dw1), p(db1), p(dw2), p(db2))
    sb = L.SGateBwdArgs(sg, None, None, p(dsp), p(dcomp), p(red), p(dw), p(dg), p(db), p(wpart))
    refused(L, L.lib.eoe_cbam_junction_bwd(C.byref(cb), C.byref(sb), p(cu_(c["dout"])), p(out), p(g), stream()))
    torch.cuda.synchronize()
    B2.bodies_untouched()
    B2.guards_intact()
