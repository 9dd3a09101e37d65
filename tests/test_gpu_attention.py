"""GPU: the attention kernels of csrc/attention.hip (attn_fwd, both attn_bwd kernels) and the causal forward of csrc/clip_text.hip
against fp64 at every length 1..64, at peaked and offset logits, next to NaN and sentinel rows, over the grid edges, and the dbias
shortcut.  Cases, references, tolerances and the comparison functions: tests/attention_util.py (checked without a GPU, mutants
included, by tests/test_cpu_attention.py).  Every output starts as NaN or as a sentinel; a test loops over its lengths and reports
every failing one together."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_util as au            # noqa: E402
from gpu_util import DTYPES            # noqa: E402

NAN = float("nan")
SENTINEL = 1234.0
KERNELS = {"four_wave": 0, "one_wave": 1}          # attn_flags bit 0


@pytest.fixture(scope="module")
def ops():
    import eoe_amd.ops as o
    return o


@pytest.fixture
def attn_flags():
    """sets the backward kernel selection; the value found is restored afterwards"""
    from eoe_amd import _lib
    prev = _lib.get_option("attn_flags")
    yield lambda v: _lib.set_option("attn_flags", v)
    _lib.set_option("attn_flags", prev)


@pytest.fixture(params=list(KERNELS))
def bwd_kernel(request, attn_flags):
    attn_flags(KERNELS[request.param])
    return request.param


def full(shape, value, dtype):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def fwd(ops, qkv, n, L, heads, out=None):
    out = full((n * L, heads * 64), SENTINEL, qkv.dtype) if out is None else out
    return ops.attn_fwd(qkv, out, n, L, heads)


def bwd(ops, qkv, dout, n, L, heads, dbias=None, dqkv=None):
    dqkv = full((n * L, 3 * heads * 64), NAN, qkv.dtype) if dqkv is None else dqkv
    if dbias is not None:          # the wrapper's reused partial rows: one the finish kernel reads must have been written by this call
        ops.scratch("attn_bias_part", (n * 3 * heads * 64,), torch.float32, qkv.device).fill_(NAN)
    return ops.attn_bwd(qkv, dout, dqkv, n, L, heads, dbias=dbias)


def tagged(tag, failures):
    return [f"{tag}: {f}" for f in failures]


def report(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


def check_case(ops, c, forward=True, backward=True):
    n, L, heads = c["dims"]
    dt = c["dtype"]
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    bad = []
    if forward:
        bad += au.fwd_failures(fwd(ops, qkv, n, L, heads), c["out"], c["vmax"], dt)
    if backward:
        bad += au.bwd_failures(bwd(ops, qkv, dout, n, L, heads), c["dqkv"], heads, dt)
    return bad


# ------------------------------------------------------------------------------------------------ 1. every length
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_at_every_length(ops, dtype):
    n, heads = au.EVERY_SHAPE
    report([m for L in au.EVERY_L for m in tagged(f"L={L}", check_case(ops, au.vit_case("unit", n, L, heads, dtype), backward=False))])


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_at_every_length(ops, dtype, bwd_kernel):
    n, heads = au.EVERY_SHAPE
    report([m for L in au.EVERY_L for m in tagged(f"L={L}", check_case(ops, au.vit_case("unit", n, L, heads, dtype), forward=False))])


# ------------------------------------------------------------------------------------------------ 2. magnitudes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", ["peaked", "offset"])
def test_magnitudes(ops, dtype, regime, bwd_kernel):
    n, heads = au.EVERY_SHAPE
    report([m for L in au.MAG_L for m in tagged(f"L={L}", check_case(ops, au.vit_case(regime, n, L, heads, dtype)))])


# ------------------------------------------------------------------------------------------------ 3. kernel against kernel
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_wave_and_four_wave_backward_agree(ops, dtype, attn_flags):
    """dqkv to the bit (same products in the same k order); dbias within its tolerance (the four-wave kernel sums per-wave partials,
    takes the V third from dO and adds exact zeros to the K third)"""
    n, heads = au.EVERY_SHAPE
    bad = []
    for regime, lengths in (("unit", au.EVERY_L), ("peaked", au.MAG_L), ("offset", au.MAG_L)):
        for L in lengths:
            c = au.vit_case(regime, n, L, heads, dtype)
            qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
            start = au.dbias_start(heads)
            res = {}
            for name, flag in KERNELS.items():
                attn_flags(flag)
                db = start.cuda()
                res[name] = (bwd(ops, qkv, dout, n, L, heads, dbias=db), db)
            tag = f"{regime} L={L}"
            bad += tagged(tag, au.bitwise_failures(res["one_wave"][0], res["four_wave"][0], "dqkv, one wave against four"))
            for name in KERNELS:
                bad += tagged(f"{tag} {name}", au.dbias_failures(res[name][1], c, start, k_exact=(name == "four_wave")))
            a, b = res["one_wave"][1].double().cpu(), res["four_wave"][1].double().cpu()
            allow = au.DBIAS_ABS * au.EPS16[dtype] * c["gscale"] * math.sqrt(n * L) + au.DBIAS_RTOL * b.abs()
            if bool(((a - b).abs() > allow).any()):
                bad.append(f"{tag}: dbias of the two kernels differs by {float((a - b).abs().max()):.3e}")
    report(bad)


# ------------------------------------------------------------------------------------------------ 4. neighbours
def framed(t, value):
    """a copy of t as a view into a larger buffer with PAD_ROWS rows of `value` before and after; (buffer, view)"""
    pad = au.PAD_ROWS
    buf = full((t.shape[0] + 2 * pad, t.shape[1]), value, t.dtype)
    buf[pad:pad + t.shape[0]] = t
    return buf, buf[pad:pad + t.shape[0]]


def frame_failures(buf, value, what):
    pad = au.PAD_ROWS
    want = full((pad, buf.shape[1]), value, buf.dtype)
    return au.bitwise_failures(buf[:pad], want, f"{what}: rows before") + au.bitwise_failures(buf[-pad:], want, f"{what}: rows behind")


@pytest.mark.parametrize("dtype", DTYPES)
def test_outputs_leave_their_neighbours_alone_and_inputs_ignore_theirs(ops, dtype, bwd_kernel):
    n, heads = au.EVERY_SHAPE
    bad = []
    for L in au.NEIGHBOUR_L:
        c = au.vit_case("unit", n, L, heads, dtype)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        out, dqkv = fwd(ops, qkv, n, L, heads), bwd(ops, qkv, dout, n, L, heads)
        # outputs as views between sentinel rows
        obuf, oview = framed(torch.zeros_like(out), SENTINEL)
        gbuf, gview = framed(torch.zeros_like(dqkv), SENTINEL)
        oview.fill_(SENTINEL), gview.fill_(NAN)
        fwd(ops, qkv, n, L, heads, out=oview), bwd(ops, qkv, dout, n, L, heads, dqkv=gview)
        bad += tagged(f"L={L}", frame_failures(obuf, SENTINEL, "out") + frame_failures(gbuf, SENTINEL, "dqkv")
                      + au.bitwise_failures(oview, out, "out as a view") + au.bitwise_failures(gview, dqkv, "dqkv as a view"))
        # inputs as views between NaN rows
        _, qview = framed(qkv, NAN)
        _, dview = framed(dout, NAN)
        bad += tagged(f"L={L}", au.bitwise_failures(fwd(ops, qview, n, L, heads), out, "out from qkv between NaN rows")
                      + au.bitwise_failures(bwd(ops, qview, dview, n, L, heads), dqkv, "dqkv from inputs between NaN rows"))
        # image 1 all NaN: image 0 as in a run of its own
        q2, d2 = qkv.clone(), dout.clone()
        q2[L:], d2[L:] = NAN, NAN
        out0, dqkv0 = fwd(ops, qkv[:L], 1, L, heads), bwd(ops, qkv[:L], dout[:L], 1, L, heads)
        o2, g2 = fwd(ops, q2, n, L, heads), bwd(ops, q2, d2, n, L, heads)
        bad += tagged(f"L={L}, image 1 NaN", au.finite_failures(o2[:L], "out of image 0") + au.finite_failures(g2[:L], "dqkv of image 0")
                      + au.bitwise_failures(o2[:L], out0, "out of image 0") + au.bitwise_failures(g2[:L], dqkv0, "dqkv of image 0"))
    report(bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_sequence_ignores_a_nan_neighbour(ops, dtype):
    heads, bad = 2, []
    for L in au.NEIGHBOUR_CAUSAL_L:
        qkv = au.causal_inputs("peaked", 2, L, heads, dtype).cuda()
        alone = ops.attn_causal_fwd(qkv[:L], full((L, heads * 64), SENTINEL, dtype), 1, L, heads)
        q2 = qkv.clone()
        q2[L:] = NAN
        buf, view = framed(torch.zeros(2 * L, heads * 64, dtype=dtype, device="cuda"), SENTINEL)
        ops.attn_causal_fwd(q2, view, 2, L, heads)
        bad += tagged(f"L={L}", au.finite_failures(view[:L], "out of sequence 0") + au.bitwise_failures(view[:L], alone, "out of sequence 0")
                      + frame_failures(buf, SENTINEL, "out"))
    report(bad)


# ------------------------------------------------------------------------------------------------ 5. grid
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,heads", au.GRID)
def test_grid(ops, dtype, n, heads, bwd_kernel):
    bad, D = [], heads * 64
    for L in au.GRID_L:
        c = au.vit_case("unit", n, L, heads, dtype)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        start = au.dbias_start(heads)
        db = start.cuda()
        out, dqkv = fwd(ops, qkv, n, L, heads), bwd(ops, qkv, dout, n, L, heads, dbias=db)
        bad += tagged(f"L={L}", au.fwd_failures(out, c["out"], c["vmax"], dtype) + au.bwd_failures(dqkv, c["dqkv"], heads, dtype)
                      + au.dbias_failures(db, c, start, k_exact=(bwd_kernel == "four_wave")))
        if n > 1:          # images permuted: so are out and dqkv, to the bit
            perm = torch.arange(n - 1, -1, -1, device="cuda").roll(n // 3)
            qp, dp = qkv.reshape(n, L, 3 * D)[perm].reshape(n * L, 3 * D), dout.reshape(n, L, D)[perm].reshape(n * L, D)
            bad += tagged(f"L={L}, images permuted",
                          au.bitwise_failures(fwd(ops, qp, n, L, heads), out.reshape(n, L, D)[perm].reshape(n * L, D), "out")
                          + au.bitwise_failures(bwd(ops, qp, dp, n, L, heads), dqkv.reshape(n, L, 3 * D)[perm].reshape(n * L, 3 * D), "dqkv"))
        if heads > 1:      # whole heads permuted in q, k, v and dout alike: so are the 64-column blocks of out and of each third of dqkv
            perm = torch.arange(heads - 1, -1, -1, device="cuda").roll(heads // 3)
            qp = qkv.reshape(n * L, 3, heads, 64)[:, :, perm].reshape(n * L, 3 * D).contiguous()
            dp = dout.reshape(n * L, heads, 64)[:, perm].reshape(n * L, D).contiguous()
            bad += tagged(f"L={L}, heads permuted",
                          au.bitwise_failures(fwd(ops, qp, n, L, heads), out.reshape(n * L, heads, 64)[:, perm].reshape(n * L, D), "out")
                          + au.bitwise_failures(bwd(ops, qp, dp, n, L, heads), dqkv.reshape(n * L, 3, heads, 64)[:, :, perm].reshape(n * L, 3 * D), "dqkv"))
    report(bad)


# ------------------------------------------------------------------------------------------------ 6. dbias
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", au.DBIAS_N)
def test_dbias(ops, dtype, n, bwd_kernel):
    """accumulates into a non-zero start; K third untouched (four-wave kernel), V third the column sums of dO, Q third and everything
    else against fp64; dqkv the same with and without dbias; a second identical call gives the same bits"""
    heads, bad = au.DBIAS_HEADS, []
    for L in au.DBIAS_L:
        c = au.vit_case("unit", n, L, heads, dtype)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        start = au.dbias_start(heads)
        plain = bwd(ops, qkv, dout, n, L, heads)
        db1, db2 = start.cuda(), start.cuda()
        g1, g2 = bwd(ops, qkv, dout, n, L, heads, dbias=db1), bwd(ops, qkv, dout, n, L, heads, dbias=db2)
        bad += tagged(f"L={L}", au.dbias_failures(db1, c, start, k_exact=(bwd_kernel == "four_wave"))
                      + au.bwd_failures(g1, c["dqkv"], heads, dtype)
                      + au.bitwise_failures(g1, plain, "dqkv with dbias against without") + au.bitwise_failures(g2, g1, "dqkv of a second call")
                      + au.bitwise_failures(db2, db1, "dbias of a second call"))
    report(bad)


# ------------------------------------------------------------------------------------------------ 7. refusals
def refused(call):
    from eoe_amd import _lib
    with pytest.raises((_lib.EoeError, ValueError)):
        call()


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_the_outputs_alone(ops, dtype):
    """every one of these returns before any launch"""
    from eoe_amd import _lib
    n, heads, D = 2, 2, 128
    qkv, dout = au.vit_inputs("unit", n, 4, heads, dtype)
    qkv, dout = qkv.cuda(), dout.cuda()
    out, dqkv, db = full((n * 4, D), SENTINEL, dtype), full((n * 4, 3 * D), SENTINEL, dtype), full((3 * D,), SENTINEL, torch.float32)
    big = full((n * 130, 3 * D), 1.0, dtype)
    refused(lambda: ops.attn_fwd(qkv, out, n, 0, heads))
    refused(lambda: ops.attn_bwd(qkv, dout, dqkv, n, 0, heads, dbias=db))
    refused(lambda: ops.attn_causal_fwd(qkv, out, n, 0, heads))
    refused(lambda: ops.attn_fwd(big, out, n, 65, heads))
    refused(lambda: ops.attn_bwd(big, big, dqkv, n, 65, heads, dbias=db))
    refused(lambda: ops.attn_causal_fwd(big, out, n, 129, heads))
    refused(lambda: ops.attn_fwd(qkv, out, n, 4, 0))
    refused(lambda: ops.attn_bwd(qkv, dout, dqkv, n, 4, 0))
    refused(lambda: ops.attn_causal_fwd(qkv, out, n, 4, 0))
    # fp32 tensors: through the wrappers, and with the C ABI's fp32 code
    q32, d32 = qkv.float(), dout.float()
    o32, g32 = full((n * 4, D), SENTINEL, torch.float32), full((n * 4, 3 * D), SENTINEL, torch.float32)
    refused(lambda: ops.attn_fwd(q32, o32, n, 4, heads))
    refused(lambda: ops.attn_bwd(q32, d32, g32, n, 4, heads))
    refused(lambda: ops.attn_causal_fwd(q32, o32, n, 4, heads))
    s = ops._stream()
    assert _lib.lib.eoe_attn_fwd(q32.data_ptr(), o32.data_ptr(), n, 4, heads, _lib.EOE_F32, s) != 0
    assert _lib.lib.eoe_attn_bwd(q32.data_ptr(), d32.data_ptr(), g32.data_ptr(), None, None, n, 4, heads, _lib.EOE_F32, s) != 0
    assert _lib.lib.eoe_attn_causal_fwd(q32.data_ptr(), o32.data_ptr(), n, 4, heads, _lib.EOE_F32, s) != 0
    # dbias without its scratch
    assert _lib.lib.eoe_attn_bwd(qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), db.data_ptr(), None, n, 4, heads, ops.dtype_code(dtype), s) != 0
    torch.cuda.synchronize()
    for t in (out, dqkv, db, o32, g32):
        report(au.bitwise_failures(t, torch.full_like(t, SENTINEL), "an output of a refused call"))


# ------------------------------------------------------------------------------------------------ 8. causal, at magnitude
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", ["peaked", "offset", "late"])
def test_causal_at_magnitude(ops, dtype, regime):
    bad = []
    for r, n, L, heads in au.causal_table():
        if r != regime:
            continue
        c = au.causal_case(regime, n, L, heads, dtype)
        buf, view = framed(torch.zeros(n * L, heads * 64, dtype=dtype, device="cuda"), SENTINEL)
        view.fill_(SENTINEL)
        ops.attn_causal_fwd(c["qkv"].cuda(), view, n, L, heads)
        bad += tagged(f"L={L} heads={heads}", au.fwd_failures(view, c["out"], c["vmax"], dtype, close=False) + frame_failures(buf, SENTINEL, "out"))
    report(bad)
