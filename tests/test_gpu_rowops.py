"""GPU: the row kernels of csrc/elementwise.hip (LayerNorm forward / backward, embed + ln_pre, the six objective heads) against
fp64 at the shapes where they take another path: several rows per wave, strided rows, every template instantiation and output
selection, accumulate, NV = 1 .. 4, n below / off the wave count, d around the 64 lanes, edge magnitudes.  Cases, references and
tolerances: tests/rowops_util.py.  Every output is pre-filled with NaN (or a sentinel that must survive bit for bit), and so is
the reused reduction scratch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_util as ru            # noqa: E402
from gpu_util import DTYPES         # noqa: E402

NAN = float("nan")
SENTINEL = 12345.678


@pytest.fixture(scope="module")
def ops():
    import eoe_amd.ops as o
    return o


def cu(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def full(shape, value, dtype=torch.float32):
    return torch.full(tuple(shape), value, dtype=dtype, device="cuda")


def p(t):
    return None if t is None else t.data_ptr()


def poison_scratch(ops, name, count):
    """the reused scratch of the wrapper (same key), filled with NaN: a partial row the finish kernel reads must have been written"""
    dev = torch.zeros(1, device="cuda").device
    ops.scratch(name, (count,), torch.float32, dev).fill_(NAN)


def ln_forward(ops, x, c, rows, D, ldx, out_dtype, with_stats=True):
    out = full((rows, D), NAN, out_dtype)
    stats = full((rows, 2), NAN) if with_stats else None
    ops.layernorm_fwd(x, cu(c["g"]), cu(c["b"]), rows, D, ldx, out, stats)
    got = {"y" if out_dtype == torch.float32 else "y16": out}
    if with_stats:
        got["mean"], got["rstd"] = stats[:, 0], stats[:, 1]
    return got


def ln_backward(ops, c, rows, D, dy_dtype, sel="all", want_dx16=None, pre=None, x=None, ldx=None, dx=None, ld_out=None, dres=None):
    """one eoe_layernorm_bwd through the wrapper.  sel: which reduction outputs are asked for; pre: what they hold before the call"""
    ldx, ld_out = ldx or D, ld_out or D
    x = cu(c["x"]) if x is None else x
    dy = cu(c["dy"], dy_dtype)
    if dres is None and c["res"] is not None:
        dres = cu(c["res"])
    dx = full((rows, D), NAN) if dx is None else dx
    dx16 = full((rows, D), NAN, want_dx16) if want_dx16 is not None else None
    outs = {}
    if sel in ("dgb", "all"):
        outs["dgamma"] = cu(pre["dgamma"]) if pre else full((D,), 0.0)
        outs["dbeta"] = cu(pre["dbeta"]) if pre else full((D,), 0.0)
    if sel in ("dxsum", "all"):
        outs["dxsum"] = cu(pre["dxsum"]) if pre else full((D,), 0.0)
    poison_scratch(ops, "ln_red", ops.LN_SCRATCH_ROWS * 3 * D)
    ops.layernorm_bwd(dy, x, cu(ru.stats32(c["ref"])), cu(c["g"]), rows, D, ldx, dx, ld_out, dres=dres, dx16=dx16, **outs)
    got = dict(outs, dx=dx)
    if dx16 is not None:
        got["dx16"] = dx16
    return got


# ------------------------------------------------------------------------------------------------ 1. LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D", ru.LN_MANY)
def test_layernorm_many_rows_per_wave(ops, dtype, rows, D):
    """rows > 4096: the 512-workgroup cap, and a wave's register accumulation of dgamma / dbeta / dxsum over several rows"""
    c = ru.ln_case(f"many{rows}", rows, D, dtype)
    specs = ru.ln_specs("many", rows, D, c["ref"], dtype)
    x = cu(c["x"])
    ru.compare("fwd f32", ln_forward(ops, x, c, rows, D, D, torch.float32), c["ref"], specs, ("y", "mean", "rstd"))
    ru.compare("fwd 16-bit", ln_forward(ops, x, c, rows, D, D, dtype), c["ref"], specs, ("y16",))
    got = ln_backward(ops, c, rows, D, dtype, want_dx16=dtype)
    ru.compare("bwd", got, c["ref"], specs, ("dx", "dx16", "dgamma", "dbeta", "dxsum"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,L,D", ru.LN_STRIDED)
def test_layernorm_strided_class_token_rows(ops, dtype, n, L, D):
    """the call of VitHeadFunction: x and dx_out / dres at stride L*D, y / dy / dx16 compact, the other rows of dx_out untouched"""
    c = ru.ln_case(f"strided{D}", n, D, dtype, True, pick=L)
    specs = ru.ln_specs("plain", n, D, c["ref"], dtype)
    x = cu(c["xfull"])
    for out_dtype in (torch.float32, dtype):
        for with_stats in (True, False):
            got = ln_forward(ops, x, c, n, D, L * D, out_dtype, with_stats)
            ru.compare(f"fwd {out_dtype} stats={with_stats}", got, c["ref"], specs, tuple(got))
    # backward with dres at the ld_out stride (its other rows hold other values: a D-stride read would pick them up)
    dx = full((n * L, D), SENTINEL)
    got = ln_backward(ops, c, n, D, dtype, x=x, ldx=L * D, dx=dx, ld_out=L * D, dres=cu(c["resfull"]))
    got["dx"] = dx.view(n, L, D)[:, 0]
    ru.compare("bwd dres", got, c["ref"], specs, ("dx", "dgamma", "dbeta", "dxsum"))
    assert bool((dx.view(n, L, D)[:, 1:] == SENTINEL).all()), "rows other than the class-token rows were written"
    # backward with a compact dx16, no dres
    c2 = ru.ln_case(f"strided{D}", n, D, dtype, False, pick=L)
    dx = full((n * L, D), SENTINEL)
    got = ln_backward(ops, c2, n, D, dtype, want_dx16=dtype, x=x, ldx=L * D, dx=dx, ld_out=L * D)
    got["dx"] = dx.view(n, L, D)[:, 0]
    ru.compare("bwd dx16", got, c2["ref"], specs, ("dx", "dx16", "dgamma", "dbeta", "dxsum"))
    assert bool((dx.view(n, L, D)[:, 1:] == SENTINEL).all()), "rows other than the class-token rows were written"


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("dy_dtype", [None] + DTYPES, ids=["dy_f32", "dy_bf16", "dy_f16"])
def test_layernorm_bwd_instantiations_and_output_selections(ops, dy_dtype, with_res):
    """fp32 / 16-bit dy x with / without dres, each with no reduction output (the early return), dxsum only, dgamma + dbeta only,
    and all of them; dx does not depend on the selection"""
    rows, D = ru.LN_INST
    c = ru.ln_case("inst", rows, D, dy_dtype, with_res)
    specs = ru.ln_specs("plain", rows, D, c["ref"], dy_dtype)
    first = None
    for sel in ru.LN_SELECTIONS:
        got = ln_backward(ops, c, rows, D, dy_dtype or torch.float32, sel=sel)
        assert set(got) == {"dx": {"dx"}, "dxsum": {"dx", "dxsum"}, "dgb": {"dx", "dgamma", "dbeta"},
                            "all": {"dx", "dgamma", "dbeta", "dxsum"}}[sel]
        ru.compare(f"sel {sel}", got, c["ref"], specs, tuple(got))
        first = got["dx"] if first is None else first
        assert torch.equal(got["dx"], first), f"dx differs between the output selections ({sel})"


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_bwd_adds_into_its_reduction_outputs(ops, dtype):
    rows, D = ru.LN_INST
    c = ru.ln_case("inst", rows, D, dtype, True)
    specs = ru.ln_specs("plain", rows, D, c["ref"], dtype)
    pre = {k: ru.ofill.fill(f"rowops/acc/{k}", (D,), std=1.0, mean=3.0) for k in ("dgamma", "dbeta", "dxsum")}
    got = ln_backward(ops, c, rows, D, dtype, pre=pre)
    want = {k: c["ref"][k] + torch.from_numpy(pre[k]).double() for k in pre}
    ru.compare("accumulate", got, want, specs, tuple(pre))


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_large_mean(ops, dtype):
    """mean 8, std 0.25: a one-pass variance E[x^2] - E[x]^2 would lose the spread"""
    rows, D = ru.LN_BIGMEAN
    c = ru.ln_case("bigmean", rows, D, dtype, True, 8.0, 0.25)
    specs = ru.ln_specs("bigmean", rows, D, c["ref"], dtype)
    x = cu(c["x"])
    ru.compare("fwd f32", ln_forward(ops, x, c, rows, D, D, torch.float32), c["ref"], specs, ("y", "mean", "rstd"))
    ru.compare("fwd 16-bit", ln_forward(ops, x, c, rows, D, D, dtype), c["ref"], specs, ("y16",))
    got = ln_backward(ops, c, rows, D, dtype, want_dx16=dtype)
    ru.compare("bwd", got, c["ref"], specs, ("dx", "dx16", "dgamma", "dbeta", "dxsum"))


# ------------------------------------------------------------------------------------------------ 2. embed + ln_pre
@pytest.mark.parametrize("D,n,L", ru.EMBED_CASES)
def test_embed_lnpre_fwd(ops, D, n, L):
    from eoe_amd import _lib
    c = ru.embed_case(D, n, L)
    x0, y, stats = full((n * L, D), NAN), full((n * L, D), NAN), full((n * L, 2), NAN)
    ins = [cu(c[k]) for k in ("tok", "cls", "pos", "g", "b")]
    _lib.check(_lib.lib.eoe_embed_lnpre_fwd(*[p(t) for t in ins], p(x0), p(y), p(stats), n, L, D, 1e-5, ops._stream()), "eoe_embed_lnpre_fwd")
    assert torch.equal(x0.cpu(), c["got32"]["x0"]), "x0 is one fp32 addition per element"
    ru.compare("embed fwd", {"y": y, "mean": stats[:, 0], "rstd": stats[:, 1]}, c["ref"], ru.embed_specs(c), ("y", "mean", "rstd"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,n,L", ru.EMBED_CASES)
def test_embed_lnpre_bwd(ops, dtype, D, n, L):
    """partial rows + finish kernel (scratch given) and atomics (scratch NULL): both against fp64, both adding into dcls / dpos /
    dgamma / dbeta, and the same dtok bits"""
    from eoe_amd import _lib
    c = ru.embed_case(D, n, L)
    specs = ru.embed_specs(c, dtype)
    ins = [cu(c["dy"]), cu(c["got32"]["x0"]), cu(ru.stats32(c["ref"])), cu(c["g"])]
    dev = ins[0].device
    dtoks = []
    for with_scratch in (True, False):
        dtok = full((n * (L - 1), D), NAN, dtype)
        acc = {k: cu(c["pre"][k]) for k in ("dcls", "dpos", "dgamma", "dbeta")}
        part = None
        if with_scratch:
            part = ops.scratch("embed_ln_part", (L * 2 * D,), torch.float32, dev)
            part.fill_(NAN)
        _lib.check(_lib.lib.eoe_embed_lnpre_bwd(*[p(t) for t in ins], p(dtok), p(acc["dcls"]), p(acc["dpos"]), p(acc["dgamma"]), p(acc["dbeta"]),
                                                p(part), n, L, D, ops.dtype_code(dtype), ops._stream()), "eoe_embed_lnpre_bwd")
        ru.compare(f"embed bwd scratch={with_scratch}", dict(acc, dtok=dtok), c["ref"], specs, ("dtok", "dcls", "dpos", "dgamma", "dbeta"))
        dtoks.append(dtok)
    assert torch.equal(dtoks[0], dtoks[1]), "dtok differs between the partial-row and the atomics path"


# ------------------------------------------------------------------------------------------------ 3. objective heads
def labels_cu(y):
    return torch.from_numpy(y).cuda()


def backward_of(loss_fn, feats, up):
    f = feats.clone().requires_grad_(True)
    loss = loss_fn(f)
    (loss * up).backward()
    return loss.detach().reshape(1), f.grad


def scaled_gradient_is_exact(ops, loss_fn, feats, up, grad):
    """under set_grad_scale(S) the head hands out S x the gradient, bit for bit (S is a power of two)"""
    ops.set_grad_scale(ru.GRAD_SCALE)
    try:
        _, g = backward_of(loss_fn, feats, up)
    finally:
        ops.set_grad_scale(1.0)
    assert torch.equal(g, grad * ru.GRAD_SCALE), "the scaled gradient is not S x the unscaled one"


def test_hsc_head(ops):
    from eoe_amd import _lib
    for args in ru.hsc_cases_all():
        c = ru.hsc_case_of(*args)
        f, y = cu(c["f"]), labels_cu(c["y"])
        n, d = f.shape
        fn = lambda t: ops.hsc_loss(t, y, c["nominal"], c["inv"])          # noqa: E731
        loss, grad = backward_of(fn, f, c["up"])
        got = {"loss": loss, "grad": grad, "score": ops.hsc_score(f)}
        if "rows" in c["specs"]:
            got["score"], got["dist"], got["rows"] = full((n,), NAN), full((n,), NAN), full((n,), NAN)
            _lib.check(_lib.lib.eoe_hsc_fwd(p(f), p(y), c["nominal"], None, p(got["score"]), p(got["dist"]), p(got["rows"]), n, d, 1.0,
                                            ops._stream()), "eoe_hsc_fwd")
            zero = np.flatnonzero((c["f"] == 0).all(1))
            for z in zero:                    # the exact expectations of test_hsc_bce for an all-zero row
                assert float(grad[z].abs().max()) == 0.0 and float(got["dist"][z]) == 0.0 and float(got["score"][z]) == 0.0
                want = 0.0 if c["y"][z] == c["nominal"] else 20.7233
                assert abs(float(got["rows"][z]) - want) < 1e-3
        ru.compare(f"hsc {args}", got, c["ref"], c["specs"])
    scaled_gradient_is_exact(ops, fn, f, c["up"], grad)


def test_dsad_head(ops):
    from eoe_amd import _lib
    for args in ru.dsad_cases_all():
        c = ru.dsad_case(*args)
        f, y = cu(c["f"]), labels_cu(c["y"])
        n, d = f.shape
        fn = lambda t: ops.dsad_loss(t, y, c["nominal"], c["inv"])          # noqa: E731
        loss, grad = backward_of(fn, f, c["up"])
        rows = full((n,), NAN)
        _lib.check(_lib.lib.eoe_dsad_fwd(p(f), p(y), c["nominal"], None, p(rows), n, d, 1.0, ops._stream()), "eoe_dsad_fwd")
        for z in np.flatnonzero((c["f"] == 0).all(1)):
            assert float(grad[z].abs().max()) == 0.0
            if c["y"][z] != c["nominal"]:
                assert float(rows[z]) == float(np.float32(1.0) / np.float32(1e-9))
        ru.compare(f"dsad {args}", {"loss": loss, "grad": grad, "rows": rows}, c["ref"], c["specs"])
    scaled_gradient_is_exact(ops, fn, f, c["up"], grad)


def test_dsvdd_head(ops):
    for args in ru.dsvdd_cases_all():
        c = ru.dsvdd_case(*args)
        f, center = cu(c["f"]), cu(c["c"])
        fn = lambda t: ops.dsvdd_loss(t, center, c["inv"])          # noqa: E731
        loss, grad = backward_of(fn, f, c["up"])
        ru.compare(f"dsvdd {args}", {"loss": loss, "grad": grad, "score": ops.dsvdd_score(f, center)}, c["ref"], c["specs"])
    scaled_gradient_is_exact(ops, fn, f, c["up"], grad)


@pytest.mark.parametrize("head", ["bce", "focal"])
def test_elementwise_heads(ops, head):
    """bce and focal at sizes around the 256-thread workgroup and at the edge logits (exp(-b) below eps, inside the clamp window,
    above 1 - eps; expf overflow): everything finite, the focal gradient without its pt term exactly where fp64 clamps"""
    from eoe_amd import _lib
    for args in [a for a in ru.elem_cases_all() if a[0] == head]:
        c = ru.elem_case(*args)
        x, y = cu(c["x"]).reshape(-1, 1), labels_cu(c["y"])
        n = x.shape[0]
        if head == "bce":
            fn = lambda t: ops.bce_loss(t, y, c["inv"])          # noqa: E731
        else:
            fn = lambda t: ops.focal_loss(t, y, c["inv"], ru.FOCAL_GAMMA, ru.FOCAL_EPS)          # noqa: E731
        loss, grad = backward_of(fn, x, c["up"])
        got = {"loss": loss, "grad": grad.reshape(-1)}
        for nominal in (0, 1):
            score, rows = full((n,), NAN), full((n,), NAN)
            if head == "bce":
                _lib.check(_lib.lib.eoe_bce_fwd(p(x), p(y), nominal, None, p(score), p(rows), n, 1.0, ops._stream()), "eoe_bce_fwd")
            else:
                _lib.check(_lib.lib.eoe_focal_fwd(p(x), p(y), nominal, None, p(score), p(rows), n, 1.0, ru.FOCAL_GAMMA, ru.FOCAL_EPS,
                                                  ops._stream()), "eoe_focal_fwd")
            got[f"score{nominal}"], got["rows"] = score, rows
        ru.compare(f"{args}", got, c["ref"], c["specs"])
    scaled_gradient_is_exact(ops, fn, x, c["up"], grad)


@pytest.mark.parametrize("T", ru.CLIP_T)
def test_clip_head(ops, T):
    from eoe_amd import _lib
    for args in [a for a in ru.clip_cases_all() if a[2] == T]:
        n, d, _, loo, nominal = args
        c = ru.clip_case(*args)
        f, t, y = cu(c["f"]), cu(c["t"]), labels_cu(c["y"])
        fn = lambda v: ops.clip_loss(v, y, t, nominal, loo, c["inv"])          # noqa: E731
        loss, grad = backward_of(fn, f, c["up"])
        ru.compare(f"clip {args}", {"loss": loss, "grad": grad, "score": ops.clip_score(f, t)}, c["ref"], c["specs"])
        if n >= 4:                            # a label that is neither class: no loss, no gradient
            rows = full((n,), NAN)
            _lib.check(_lib.lib.eoe_clip_fwd(p(f), p(t), p(y), nominal, int(loo), None, None, p(rows), n, d, T, 1.0, ops._stream()), "eoe_clip_fwd")
            assert float(rows[3]) == 0.0 and float(grad[3].abs().max()) == 0.0 and bool(torch.isfinite(rows).all())
    scaled_gradient_is_exact(ops, fn, f, c["up"], grad)
