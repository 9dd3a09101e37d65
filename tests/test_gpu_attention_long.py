"""GPU: the long-sequence attention kernels of csrc/attention_long.hip (attn_long_fwd, attn_long_bwd, 64 < L <= 640) against fp64 over
the table of tests/attention_long_util.py, next to NaN and sentinel rows, run twice for their bits, their refusals, and the block
driver's choice between them and the short kernels.  Cases, rounding model and mutants: tests/attention_long_util.py (checked without
a GPU by tests/test_cpu_attention_long.py); references, comparison functions and tolerances: tests/attention_util.py, unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_long_util as lu       # noqa: E402
import attention_util as au            # noqa: E402
from gpu_util import DTYPES            # noqa: E402

NAN = float("nan")
SENTINEL = 1234.0


@pytest.fixture(scope="module")
def ops():
    import eoe_amd.ops as o
    return o


def full(shape, value, dtype):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def fwd(ops, qkv, n, L, heads, out=None):
    out = full((n * L, heads * 64), SENTINEL, qkv.dtype) if out is None else out
    return ops.attn_long_fwd(qkv, out, n, L, heads)


def bwd(ops, qkv, dout, n, L, heads, dbias=None, dqkv=None):
    dqkv = full((n * L, 3 * heads * 64), NAN, qkv.dtype) if dqkv is None else dqkv
    if dbias is not None:          # the wrapper's reused partial rows: one the finish kernel reads must have been written by this call
        ops.scratch("attn_bias_part", (n * 3 * heads * 64,), torch.float32, qkv.device).fill_(NAN)
    return ops.attn_long_bwd(qkv, dout, dqkv, n, L, heads, dbias=dbias)


def tagged(tag, failures):
    return [f"{tag}: {f}" for f in failures]


def report(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


def check_case(ops, c):
    n, L, heads = c["dims"]
    dt = c["dtype"]
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    start = au.dbias_start(heads)
    db = start.cuda()
    bad = au.fwd_failures(fwd(ops, qkv, n, L, heads), c["out"], c["vmax"], dt)
    bad += au.bwd_failures(bwd(ops, qkv, dout, n, L, heads, dbias=db), c["dqkv"], heads, dt)
    return bad + au.dbias_failures(db, c, start)


# ------------------------------------------------------------------------------------------------ 1. the table against fp64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", ["unit", "peaked", "offset", "late64", "late128"])
def test_forward_and_backward_against_fp64(ops, dtype, regime):
    cases = [t for t in lu.long_table() if t[0] == regime]
    assert cases
    report([m for t in cases for m in tagged(f"n={t[1]} L={t[2]} heads={t[3]}", check_case(ops, lu.long_case(*t, dtype)))])


# ------------------------------------------------------------------------------------------------ 2. neighbours
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
def test_neighbouring_rows_are_neither_read_nor_written(ops, dtype):
    """inputs sit between NaN rows, outputs between sentinel rows: the results are those of the plain call to the bit, no NaN leaks and
    the sentinels keep their bits"""
    n, heads = lu.SHAPE
    bad = []
    for L in lu.NEIGHBOUR_L:
        c = lu.long_case("unit", n, L, heads, dtype)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        plain_out, plain_dqkv = fwd(ops, qkv, n, L, heads), bwd(ops, qkv, dout, n, L, heads)
        _, qv = framed(qkv, NAN)
        _, dv = framed(dout, NAN)
        obuf, ov = framed(full((n * L, heads * 64), SENTINEL, dtype), SENTINEL)
        gbuf, gv = framed(full((n * L, 3 * heads * 64), SENTINEL, dtype), SENTINEL)
        fwd(ops, qv, n, L, heads, out=ov)
        bwd(ops, qv, dv, n, L, heads, dqkv=gv)
        tag = f"L={L}"
        bad += tagged(tag, au.finite_failures(ov, "out") + au.finite_failures(gv, "dqkv"))
        bad += tagged(tag, au.bitwise_failures(ov, plain_out, "out in a frame") + au.bitwise_failures(gv, plain_dqkv, "dqkv in a frame"))
        bad += tagged(tag, frame_failures(obuf, SENTINEL, "out") + frame_failures(gbuf, SENTINEL, "dqkv"))
    report(bad)


# ------------------------------------------------------------------------------------------------ 3. two runs, the same bits
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_give_identical_bits(ops, dtype):
    bad = []
    for regime, n, L, heads in (("unit", 2, 197, 2), ("late64", 2, 129, 2), ("unit", 7, 65, 3), ("unit", 1, 197, 12), ("unit", 2, 577, 2)):
        c = lu.long_case(regime, n, L, heads, dtype)
        qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
        runs = []
        for _ in range(2):
            db = au.dbias_start(heads).cuda()
            runs.append((fwd(ops, qkv, n, L, heads), bwd(ops, qkv, dout, n, L, heads, dbias=db), db))
        for what, a, b in zip(("out", "dqkv", "dbias"), *runs):
            bad += tagged(f"{regime} n={n} L={L} heads={heads}", au.bitwise_failures(a, b, what + ", second run against first"))
    report(bad)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_come_before_any_launch_and_leave_the_outputs_alone(ops):
    dt = torch.float16
    heads = 2
    D = heads * 64
    assert ops.ATTN_LONG_MAX_L == lu.LONG_MAX_L >= 577 and ops.ATTN_SHORT_MAX_L + 1 == lu.LONG_MIN_L
    for n, L, h, dtype in ((2, 64, heads, dt), (2, lu.LONG_MAX_L + 1, heads, dt), (2, 65, 0, dt), (2, 65, heads, torch.float32)):
        qkv = torch.zeros((n * L, 3 * D), dtype=dtype, device="cuda")
        dout = torch.zeros((n * L, D), dtype=dtype, device="cuda")
        out, dqkv = full((n * L, D), SENTINEL, dtype), full((n * L, 3 * D), SENTINEL, dtype)
        db = full((3 * D,), SENTINEL, torch.float32)
        with pytest.raises((RuntimeError, ValueError)):
            ops.attn_long_fwd(qkv, out, n, L, h)
        with pytest.raises((RuntimeError, ValueError)):
            ops.attn_long_bwd(qkv, dout, dqkv, n, L, h, dbias=db)
        torch.cuda.synchronize()
        for what, t in (("out", out), ("dqkv", dqkv), ("dbias", db)):
            assert not au.bitwise_failures(t, torch.full_like(t, SENTINEL), what), (n, L, h, dtype)
    # and the short entry points still refuse what is now the long kernels'
    qkv = torch.zeros((2 * 65, 3 * D), dtype=dt, device="cuda")
    out = full((2 * 65, D), SENTINEL, dt)
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv, out, 2, 65, heads)
    torch.cuda.synchronize()
    assert not au.bitwise_failures(out, torch.full_like(out, SENTINEL), "out")


# ------------------------------------------------------------------------------------------------ 5. the block driver's choice
def _fused_block(ops, n, L, heads, dtype):
    """one block through eoe_vit_block_fwd / _bwd (VitBlockFunction); returns what the call leaves behind: the saved qkv and attention
    output, the d(out-projection input) copy and dqkv of the backward, and the 16-bit transposed out-projection weight"""
    from oracle import fill as ofill
    D, M = heads * 64, n * L

    def P(name, shape, std, mean=0.0):
        return torch.from_numpy(ofill.fill(f"attn/long/block/{name}", shape, std=std, mean=mean)).cuda().requires_grad_(True)

    params = [P("ln1_g", (D,), 0.1, 1.0), P("ln1_b", (D,), 0.1), P("w_in", (3 * D, D), D ** -0.5), P("b_in", (3 * D,), 0.1),
              P("w_out", (D, D), D ** -0.5), P("b_out", (D,), 0.1), P("ln2_g", (D,), 0.1, 1.0), P("ln2_b", (D,), 0.1),
              P("w_fc", (4 * D, D), D ** -0.5), P("b_fc", (4 * D,), 0.1), P("w_proj", (D, 4 * D), (4 * D) ** -0.5), P("b_proj", (D,), 0.1)]
    x = P(f"x{L}", (M, D), 1.0)
    y = ops.VitBlockFunction.apply(x, n, heads, *params, False)
    ws = y.grad_fn.saved_tensors[1]
    _, ptr = ops._block_ws(M, D, x.device, dtype)          # the layout of the saved activations
    base = min(ptr.values())

    def saved(key, cols):
        o = ptr[key] - base
        return ws[o:o + M * cols * 2].view(dtype).reshape(M, cols)

    qkv, att = saved("qkv", 3 * D).clone(), saved("att", D).clone()
    y.backward(torch.from_numpy(ofill.fill(f"attn/long/block/dy{L}", (M, D), std=1.0)).cuda())
    torch.cuda.synchronize()
    par = ops._vit_sweeps[(x.device.index, ops._stream())].parity
    d_mid16 = ops.scratch(f"d16_c{par}", (M, D), dtype, x.device).clone()
    dqkv = ops.scratch(f"dqkv{par}", (M, 3 * D), dtype, x.device).clone()
    w_out_t = ops.shadow.get(params[4], True, True)[1]
    return {"y": y.detach().clone(), "qkv": qkv, "att": att, "d_mid16": d_mid16, "dqkv": dqkv, "w_out_t": w_out_t,
            "grads": [p.grad.clone() for p in params] + [x.grad.clone()]}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [64, 65])
def test_block_driver_runs_the_kernels_its_length_names(ops, dtype, L):
    """the attention step of eoe_vit_block_fwd / _bwd, isolated: the block's attention output carries the bits of the separate attention
    op on the block's own qkv, and its dqkv those of the separate backward on the d att that the same dgrad GEMM forms from the block's
    own buffers.  L = 64: the short ops.attn_fwd / attn_bwd, the path of the code before the long kernels; L = 65: the long ones"""
    n, heads = 3, 4          # D = 256: the narrowest row the LayerNorm kernels take
    D, M = heads * 64, n * L
    prev = ops.compute_dtype()
    ops.set_compute_dtype(dtype)
    try:
        r = _fused_block(ops, n, L, heads, dtype)
        short = L <= ops.ATTN_SHORT_MAX_L
        att = full((M, D), SENTINEL, dtype)
        (ops.attn_fwd if short else ops.attn_long_fwd)(r["qkv"], att, n, L, heads)
        bad = au.bitwise_failures(r["att"], att, "attention output of the fused block against the separate op")
        datt = full((M, D), NAN, dtype)
        ops.gemm_nt(r["d_mid16"], r["w_out_t"], datt)
        dqkv = full((M, 3 * D), NAN, dtype)
        (ops.attn_bwd if short else ops.attn_long_bwd)(r["qkv"], datt, dqkv, n, L, heads)
        bad += au.bitwise_failures(r["dqkv"], dqkv, "dqkv of the fused block against the separate op")
        # and the whole block twice: the same bits
        r2 = _fused_block(ops, n, L, heads, dtype)
        bad += au.bitwise_failures(r2["y"], r["y"], "x_out, second run against first")
        for i, (a, b) in enumerate(zip(r2["grads"], r["grads"])):
            bad += au.bitwise_failures(a, b, f"gradient {i}, second run against first") + au.finite_failures(a, f"gradient {i}")
    finally:
        ops.set_compute_dtype(prev)
    report(bad)
