"""GPU: the BatchNorm + activation + pooling kernels of csrc/conv.hip and the plain pooling / junction kernels of csrc/cbam.hip
against fp64, called through the C ABI on the current stream, at the shapes where they take another path: channel counts whose
quad count does not divide 256 (q > 1 workgroups forced), more quads than threads, idle workgroups, the 1024-row cap, non-square
maps, the generic overlapping max-pool backward at S = 1 / 2 / run-time stride, every option of the entry points.  Cases,
references and tolerances: tests/bnpool_util.py.  Every output is pre-filled with NaN (or a sentinel that must survive bit for
bit), and so is the reduction scratch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnpool_util as bu            # noqa: E402

NAN = float("nan")
SENTINEL = 12345.678
EOE_ERR_ARG = 1


@pytest.fixture(scope="module")
def L():
    from eoe_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def stream():
    import eoe_amd.ops as o
    return o._stream


def cu(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def full(shape, value, dtype=torch.float32):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def p(t):
    return None if t is None else t.data_ptr()


def scratch(C):
    """EOE_BN_SCRATCH(C) floats of NaN: a partial row a later kernel reads must have been written"""
    return full(((1024 + 3) * 2 * C,), NAN)


def code(L, dtype, y16=False):
    c = L.EOE_F32 if dtype is None else L.EOE_F16 if dtype == torch.float16 else L.EOE_BF16
    return c | (L.EOE_Y16 if y16 else 0)


def y_of(c, yd):
    """the y buffer the kernel reads: fp32, or the 16-bit copy"""
    return cu(c["y"]) if yd is None else cu(c["yq"], yd)


def refused(L, rc):
    assert rc == EOE_ERR_ARG, rc
    assert L.lib.eoe_last_error()


def untouched(*ts):
    return all(bool((t == 77).all()) if t.dtype == torch.uint8 else bool((t == torch.tensor(SENTINEL).to(t.dtype).item()).all()) for t in ts)


# ------------------------------------------------------------------------------------------------ 1. eoe_bn_stats
def run_stats(L, stream, c, M, C, training=1, eps=bu.EPS_BN):
    y, stats = cu(c["y"]), full((2 * C,), NAN)
    rm, rv = cu(c["rm0"]), cu(c["rv0"])
    nbt, red = torch.full((1,), 41, dtype=torch.int64, device="cuda"), scratch(C)
    L.check(L.lib.eoe_bn_stats(p(y), p(red), p(stats), p(rm), p(rv), p(nbt), M, C, eps, bu.MOMENTUM, training, stream()), "eoe_bn_stats")
    return {"mean": stats[:C], "rstd": stats[C:], "rmean": rm, "rvar": rv}, nbt


@pytest.mark.parametrize("M,C", bu.STATS_CASES)
def test_bn_stats_training(L, stream, M, C):
    """(37, 1 / 3 / 5): VEC = 1.  (2, 4), (300, 4): cpb = 1.  (1023 / 1024 / 1025, 64): the boundary of the four-loads-in-flight
    loop.  (33000, 256): gy capped at 512.  (4200, 4096): gx * gy capped at 1024.  (500, 20): the channel tail of the 16-column
    finalize.  Statistics, running buffers (momentum 0.1, unbiased variance) and num_batches_tracked"""
    c = bu.stats_case(M, C)
    got, nbt = run_stats(L, stream, c, M, C)
    assert int(nbt.item()) == 42
    bu.compare(f"bn_stats {M}x{C}", got, c["ref"], c["specs"])


def test_bn_stats_large_mean(L, stream):
    """per-channel mean = 8 x std: E[y^2] - E[y]^2 keeps the spread only while the partial rows stay in double (with float rows rstd
    was 1.6 times its bound away)"""
    M, C = bu.STATS_BIGMEAN
    c = bu.stats_case(M, C, bigmean=True)
    got, _ = run_stats(L, stream, c, M, C)
    bu.compare("bn_stats large mean", got, c["ref"], c["specs"])


def test_bn_stats_eval_reads_the_running_buffers(L, stream):
    """eval: stats = (running_mean, 1 / sqrt(running_var + eps)); the buffers and the counter stay untouched"""
    M, C = 300, 20
    c = bu.stats_case(500, 20)
    got, nbt = run_stats(L, stream, c, M, C, training=0)
    assert int(nbt.item()) == 41
    assert torch.equal(got["rmean"].cpu(), torch.from_numpy(c["rm0"])) and torch.equal(got["rvar"].cpu(), torch.from_numpy(c["rv0"]))
    assert torch.equal(got["mean"].cpu(), torch.from_numpy(c["rm0"]))
    want = 1.0 / torch.sqrt(torch.from_numpy(c["rv0"]).double() + bu.EPS_BN)
    bu.compare("bn_stats eval", got, {"rstd": want}, {"rstd": bu.meas("stats/rstd", want)})


# ------------------------------------------------------------------------------------------------ 2. eoe_bn_stats_partials
@pytest.mark.parametrize("C", bu.PARTIALS_C)
@pytest.mark.parametrize("R", bu.PARTIALS_R)
def test_bn_stats_partials(L, stream, R, C):
    """R <= 1024 rows go straight to the finalize; above, fold_partials pairs rows r and r + 1024 (1025: one pair; 2049: two
    partners for row 0, an odd tail; 3000: most rows with three, the rest with two)"""
    c = bu.partials_case(R, C)
    part, stats = cu(c["part"]), full((2 * C,), NAN)
    rm, rv = cu(c["rm0"]), cu(c["rv0"])
    nbt, red = torch.zeros(1, dtype=torch.int64, device="cuda"), scratch(C)
    L.check(L.lib.eoe_bn_stats_partials(p(part), R, p(red), p(stats), p(rm), p(rv), p(nbt), c["M"], C, bu.EPS_BN, bu.MOMENTUM,
                                        stream()), "eoe_bn_stats_partials")
    assert int(nbt.item()) == 1
    bu.compare(f"bn_stats_partials {R}x{C}", {"mean": stats[:C], "rstd": stats[C:], "rmean": rm, "rvar": rv}, c["ref"], c["specs"])


# ------------------------------------------------------------------------------------------------ 3. eoe_bn_act_pool_fwd
def pool_fwd(L, stream, c, yd, dtype, mode):
    """one forward call; mode: '16' (16-bit NHWC), 'f32', 'f32+16' (fp32 NHWC and out16), 'flat16', 'flatf32'"""
    n, H, W, C = c["y"].shape
    P = c["pool"][1]
    Ho, Wo = H // P, W // P
    flat, f32 = mode.startswith("flat"), "f32" in mode
    out = full((n, C * Ho * Wo) if flat else (n, Ho, Wo, C), NAN, torch.float32 if f32 else dtype)
    out16 = full((n, Ho, Wo, C), NAN, dtype) if mode == "f32+16" else None
    g = None if c["gamma"] is None else cu(c["gamma"])
    b = None if c["beta"] is None else cu(c["beta"])
    y, st = y_of(c, yd), cu(bu.stats32(c))
    L.check(L.lib.eoe_bn_act_pool_fwd(p(y), p(st), p(g), p(b), p(out), p(out16), n, H, W, C, P, int(flat), int(f32),
                                      c["slope"], code(L, dtype, yd is not None), stream()), "eoe_bn_act_pool_fwd")
    got = {"flat" if flat else "out" if f32 else "out16": out}
    if out16 is not None:
        got["out16"] = out16
    return got


@pytest.mark.parametrize("n,H,W,C,P,slope,affine,yd", bu.fwd_cases())
def test_bn_act_pool_fwd(L, stream, n, H, W, C, P, slope, affine, yd):
    """non-square maps (6 x 10, 1 x 4), pool 1 / 2, C = 4 / 12 / 48, slope 0 / 0.01 / 1, gamma = beta = NULL, y fp32 or 16-bit
    (EOE_Y16), and all five output forms in both 16-bit dtypes"""
    c = bu.fwd_case(n, H, W, C, P, slope, affine, yd)
    for dtype in (bu.DTYPES if yd is None else (yd,)):
        for mode in ("16", "f32", "f32+16", "flat16", "flatf32"):
            got = pool_fwd(L, stream, c, yd, dtype, mode)
            specs = bu.act_specs(c, None if mode == "flatf32" else dtype)
            bu.compare(f"fwd {mode} {dtype}", got, c["ref"], specs, tuple(got))


def test_bn_act_pool_fwd_refuses_and_writes_nothing(L, stream):
    """out16 with a 16-bit or a flat output, odd H with pool 2, C % 4 != 0"""
    c = bu.fwd_case(2, 1, 4, 4, 1, 0.0, True, None)
    y, st, g, b = cu(c["y"]), cu(bu.stats32(c)), cu(c["gamma"]), cu(c["beta"])
    out, out16 = full((64,), SENTINEL), full((64,), SENTINEL, torch.bfloat16)
    f = L.lib.eoe_bn_act_pool_fwd
    refused(L, f(p(y), p(st), p(g), p(b), p(out), p(out16), 2, 1, 4, 4, 1, 0, 0, 0.0, L.EOE_BF16, stream()))
    refused(L, f(p(y), p(st), p(g), p(b), p(out), p(out16), 2, 1, 4, 4, 1, 1, 1, 0.0, L.EOE_BF16, stream()))
    refused(L, f(p(y), p(st), p(g), p(b), p(out), None, 2, 1, 4, 4, 2, 0, 1, 0.0, L.EOE_BF16, stream()))
    refused(L, f(p(y), p(st), p(g), p(b), p(out), None, 2, 1, 2, 6, 1, 0, 1, 0.0, L.EOE_BF16, stream()))
    torch.cuda.synchronize()
    assert untouched(out, out16)


# ------------------------------------------------------------------------------------------------ 4. eoe_bn_act_pool_bwd
@pytest.mark.parametrize("n,H,W,C,P,flat,dyd,training,acc,dgb,yd,slope", bu.bwd_cases())
def test_bn_act_pool_bwd(L, stream, n, H, W, C, P, flat, dyd, training, acc, dgb, yd, slope):
    """the reduce pass at q = (C/4) / gcd(C/4, 256) forced workgroups -- C = 4 (q 1, one partly idle workgroup), 12 (q 3: one partly
    idle and two empty workgroups), 20 (q 5: 7700 items, no multiple of the grid stride; the apply pass reloads its quad), 1028
    (q 257: more quads than threads, whole idle workgroups), 4092 (q 1023), 4096 (1024 quads, q 4), 64 on 9 x 64 x 60 (two positions
    per iteration, the 1024-row cap) -- each with pool 1 / 2, NHWC / NCHW-flat dout, fp32 / 16-bit dy, training / eval (running
    statistics), accumulate 0 / 1, dgamma = dbeta = NULL, y fp32 / EOE_Y16"""
    c = bu.bwd_case(n, H, W, C, P, flat, dyd, training, acc, dgb, yd, slope)
    Ho, Wo = H // P, W // P
    dout = cu(c["dout"])
    if flat:
        dout = dout.permute(0, 3, 1, 2).contiguous()
    dy = full((n * H * W, C), NAN, torch.float32 if dyd is None else dyd)
    dg = db = None
    if dgb:
        dg = cu(c["pre"]["dgamma"]) if acc else full((C,), NAN)
        db = cu(c["pre"]["dbeta"]) if acc else full((C,), NAN)
    dtype = dyd or yd or torch.bfloat16
    y, st, g, b, red = y_of(c, yd), cu(bu.stats32(c)), cu(c["gamma"]), cu(c["beta"]), scratch(C)
    L.check(L.lib.eoe_bn_act_pool_bwd(p(y), p(st), p(g), p(b), p(dout), p(red),
                                      p(dy), int(dyd is None), p(dg), p(db), n, H, W, C, P, flat, int(training), acc, slope,
                                      code(L, dtype, yd is not None), stream()), "eoe_bn_act_pool_bwd")
    got = {"dy": dy}
    if dgb:
        got.update(dgamma=dg, dbeta=db)
    bu.compare("bn_act_pool_bwd", got, c["ref"], c["specs"], tuple(got))


def test_bn_act_pool_bwd_without_gamma(L, stream):
    """gamma = beta = NULL (gamma 1, beta 0), dgamma / dbeta still asked for"""
    n, H, W, C = 3, 6, 10, 12
    c = bu.bn_act_case("bwd/nogamma", n, H, W, C, ("win", 2), 0.01, True, False, None)
    dy, dg, db = full((n * H * W, C), NAN), full((C,), NAN), full((C,), NAN)
    y, st, dout, red = cu(c["y"]), cu(bu.stats32(c)), cu(c["dout"]), scratch(C)
    L.check(L.lib.eoe_bn_act_pool_bwd(p(y), p(st), None, None, p(dout), p(red), p(dy), 1, p(dg), p(db),
                                      n, H, W, C, 2, 0, 1, 0, 0.01, L.EOE_BF16, stream()), "eoe_bn_act_pool_bwd")
    bu.compare("bwd gamma NULL", {"dy": dy, "dgamma": dg, "dbeta": db}, c["ref"], bu.act_specs(c), ("dy", "dgamma", "dbeta"))


# ------------------------------------------------------------------------------------------------ 5. eoe_bn_act_maxpool
@pytest.mark.parametrize("C", bu.MAXPOOL_C)
@pytest.mark.parametrize("gi", range(len(bu.MAXPOOL_GEOS)))
def test_bn_act_maxpool(L, stream, gi, C):
    """(k, stride, pad) on H x W: (3, 2, 1) on 6 x 10 the s2k3 kernel on a non-square map; (3, 2, 1) on 7 x 9 generic S = 2; (3, 2, 0)
    on 8 x 6 generic, last row and column in no window; (3, 1, 1) on 5 x 7 S = 1; (2, 3, 0) on 8 x 7 run-time stride, pixels between
    windows; (2, 2, 1) on 5 x 6 windows hanging into the padding.  Forward: out, out16, idx (exact).  Backward: training and eval,
    dy in bf16 / fp16 / fp32 (dtype EOE_F32), y fp32 and EOE_Y16; a pixel that won no window gets the mean terms / exactly 0"""
    k, s, pad, H, W = bu.MAXPOOL_GEOS[gi]
    n = bu.MAXPOOL_N
    Ho, Wo = bu.out_hw(H, W, ("max", k, s, pad))
    for training in (True, False):
        for yd in (None,) + bu.DTYPES:
            c = bu.maxpool_case(gi, C, training, yd)
            y, st, g, b = y_of(c, yd), cu(bu.stats32(c)), cu(c["gamma"]), cu(c["beta"])
            idx = None
            for dtype in (bu.DTYPES if yd is None else (yd,)):
                out, out16 = full((n, Ho, Wo, C), NAN), full((n, Ho, Wo, C), NAN, dtype)
                idx = torch.full((n, Ho, Wo, C), 255, dtype=torch.uint8, device="cuda")
                L.check(L.lib.eoe_bn_act_maxpool_fwd(p(y), p(st), p(g), p(b), p(out), p(out16), p(idx), n, H, W, C, k, s, pad, c["slope"],
                                                     code(L, dtype, yd is not None), stream()), "eoe_bn_act_maxpool_fwd")
                bu.compare(f"maxpool fwd {dtype} y={yd}", {"out": out, "out16": out16}, c["ref"], bu.act_specs(c, dtype), ("out", "out16"))
                assert torch.equal(idx.cpu(), c["ref"]["idx"]), f"winner taps differ in {int((idx.cpu() != c['ref']['idx']).sum())} places"
            dout = cu(c["dout"])
            for dyd in ((None,) + bu.DTYPES if yd is None else (yd,)):
                dy = full((n * H * W, C), NAN, torch.float32 if dyd is None else dyd)
                dg, db, red = full((C,), NAN), full((C,), NAN), scratch(C)
                L.check(L.lib.eoe_bn_act_maxpool_bwd(p(y), p(st), p(g), p(b), p(dout), p(idx), p(red), p(dy), p(dg), p(db), n, H, W, C,
                                                     k, s, pad, int(training), c["slope"], code(L, dyd, yd is not None), stream()),
                        "eoe_bn_act_maxpool_bwd")
                bu.compare(f"maxpool bwd train={training} dy={dyd} y={yd}", {"dy": dy, "dgamma": dg, "dbeta": db}, c["ref"],
                           bu.act_specs(c, None, dyd), ("dy", "dgamma", "dbeta"))
                if not training:
                    zero = (c["ref"]["dy"] == 0)
                    assert bool((dy.float().cpu()[zero] == 0).all()), "eval: a pixel without a won window must get exactly 0"


def test_bn_act_maxpool_bwd_refuses_y16_with_f32(L, stream):
    c = bu.maxpool_case(0, 4, True, torch.float16)
    k, s, pad, H, W = bu.MAXPOOL_GEOS[0]
    n, C = bu.MAXPOOL_N, 4
    dy, dg, db = full((n * H * W, C), SENTINEL), full((C,), SENTINEL), full((C,), SENTINEL)
    y, st, g, b, dout, idx, red = (y_of(c, torch.float16), cu(bu.stats32(c)), cu(c["gamma"]), cu(c["beta"]), cu(c["dout"]), cu(c["ref"]["idx"]),
                                   scratch(C))
    rc = L.lib.eoe_bn_act_maxpool_bwd(p(y), p(st), p(g), p(b), p(dout),
                                      p(idx), p(red), p(dy), p(dg), p(db), n, H, W, C, k, s, pad, 1, 0.0,
                                      L.EOE_F32 | L.EOE_Y16, stream())
    refused(L, rc)
    torch.cuda.synchronize()
    assert untouched(dy, dg, db)


# ------------------------------------------------------------------------------------------------ 6. eoe_colsum_f32
@pytest.mark.parametrize("C", bu.COLSUM_C)
@pytest.mark.parametrize("rows", bu.COLSUM_ROWS)
def test_colsum_f32_accumulates(L, stream, rows, C):
    """accumulate = 1 at q = 1 / 257 / 1023 forced workgroups, with one row, three rows (idle workgroups) and 70000 rows (many
    iterations per thread)"""
    c = bu.colsum_case(rows, C)
    x = bu.colsum_matrix(cu(c["table"]), rows)
    out, red = cu(c["pre"]), scratch(C)
    L.check(L.lib.eoe_colsum_f32(p(x), p(out), p(red), rows, C, 1, stream()), "eoe_colsum_f32")
    bu.compare(f"colsum {rows}x{C}", {"out": out}, c["ref"], c["specs"])


# ------------------------------------------------------------------------------------------------ 7. eoe_maxpool, exact
@pytest.mark.parametrize("C", bu.PLAIN_C)
@pytest.mark.parametrize("gi", range(len(bu.PLAIN_GEOS)))
def test_maxpool_plain_exact(L, stream, gi, C):
    """(2, 2, 0) on 6 x 10, (3, 1, 1) on 5 x 7, (2, 3, 0) on 8 x 7, (3, 2, 0) on 8 x 6; ties after a ReLU: values, 16-bit copies, winner
    taps and gradients bit for bit"""
    k, s, pad, H, W = bu.PLAIN_GEOS[gi]
    n = bu.PLAIN_N
    c = bu.plain_maxpool_case(gi, C)
    Ho, Wo = bu.out_hw(H, W, ("max", k, s, pad))
    x = cu(c["x"])
    for dtype in bu.DTYPES:
        out, out16 = full((n, Ho, Wo, C), NAN), full((n, Ho, Wo, C), NAN, dtype)
        idx = torch.full((n, Ho, Wo, C), 255, dtype=torch.uint8, device="cuda")
        L.check(L.lib.eoe_maxpool_fwd(p(x), p(out), p(out16), p(idx), n, H, W, C, k, s, pad, code(L, dtype), stream()), "eoe_maxpool_fwd")
        assert torch.equal(out.cpu(), c["out"]) and torch.equal(out16.cpu(), c["out"].to(dtype)) and torch.equal(idx.cpu(), c["idx"])
        dx, dout = full((n, H, W, C), NAN), cu(c["dout"])
        L.check(L.lib.eoe_maxpool_bwd(p(dout), p(idx), p(dx), n, H, W, C, k, s, pad, stream()), "eoe_maxpool_bwd")
        assert torch.equal(dx.cpu(), c["dx"])


# ------------------------------------------------------------------------------------------------ 8. eoe_avgpool
@pytest.mark.parametrize("n,HW,C", bu.AVGPOOL_CASES)
def test_avgpool(L, stream, n, HW, C):
    """one position (every row lane but one idle), 49 positions on 32 row lanes (the tail loop only), 1000 positions on 4 row lanes
    (the eight-loads-in-flight loop and its tail); the mean, the scratch's max plane and argmax (first position of the maximum), and the backward"""
    c = bu.avgpool_case(n, HW, C)
    x, pooled, arg = cu(c["x"]), full((n, 2, C), NAN), torch.full((n, C), -1, dtype=torch.int32, device="cuda")
    L.check(L.lib.eoe_avgpool_fwd(p(x), p(pooled), p(arg), n, HW, C, stream()), "eoe_avgpool_fwd")
    bu.compare("avgpool fwd", {"mean": pooled[:, 0]}, c["ref"], c["specs"], ("mean",))
    assert torch.equal(pooled[:, 1].cpu(), c["ref"]["max"]) and torch.equal(arg.cpu(), c["ref"]["argmax"])
    dx, dout = full((n, HW, C), NAN), cu(c["dout"])
    L.check(L.lib.eoe_avgpool_bwd(p(dout), p(dx), n, HW, C, stream()), "eoe_avgpool_bwd")
    bu.compare("avgpool bwd", {"dx": dx}, c["ref"], c["specs"], ("dx",))


@pytest.mark.parametrize("C", bu.AVGPOOL_REFUSED_C)
def test_avgpool_refuses_channel_counts_it_cannot_take(L, stream, C):
    x, pooled, arg = full((2, 3, C), 1.0), full((2, 2, C), SENTINEL), torch.full((2 * C * 4,), 77, dtype=torch.uint8, device="cuda")
    refused(L, L.lib.eoe_avgpool_fwd(p(x), p(pooled), p(arg), 2, 3, C, stream()))
    torch.cuda.synchronize()
    assert untouched(pooled, arg)


# ------------------------------------------------------------------------------------------------ 9. add + ReLU, exact
@pytest.mark.parametrize("count", bu.JUNCTION_COUNTS)
def test_add_relu_and_relu_bwd_exact(L, stream, count):
    """one quad, 257 quads, one quad past the grid cap (a second grid-stride iteration for one thread); a + b == 0 and -0.0 inputs;
    the backward's mask is out > 0"""
    c = bu.junction_case(count)
    a, b = cu(c["a"]), cu(c["b"])
    for dtype in bu.DTYPES:
        out, out16 = full((count,), NAN), full((count,), NAN, dtype)
        L.check(L.lib.eoe_add_relu_fwd(p(a), p(b), p(out), p(out16), code(L, dtype), count, stream()), "eoe_add_relu_fwd")
        assert torch.equal(out.cpu(), c["out"]) and torch.equal(out16.cpu(), c["out"].to(dtype))
    g, dout = full((count,), NAN), cu(c["dout"])
    L.check(L.lib.eoe_relu_bwd(p(dout), p(out), p(g), count, stream()), "eoe_relu_bwd")
    assert torch.equal(g.cpu(), c["g"])


def test_add_relu_refuses_a_count_that_is_no_multiple_of_four(L, stream):
    a, out, out16 = full((8,), 1.0), full((8,), SENTINEL), full((8,), SENTINEL, torch.bfloat16)
    refused(L, L.lib.eoe_add_relu_fwd(p(a), p(a), p(out), p(out16), L.EOE_BF16, 6, stream()))
    refused(L, L.lib.eoe_relu_bwd(p(a), p(a), p(out), 6, stream()))
    torch.cuda.synchronize()
    assert untouched(out, out16)
