"""GPU: LayerNorm forward / backward and embed + ln_pre (csrc/elementwise.hip) through the C ABI at widths that are multiples of 64 but
not of 256 -- the last 256-column group of a row then has 16, 32 or 48 active lanes -- against oracle.models.layer_norm in fp64.  Cases:
tests/vit_narrow_util.py; references and every tolerance: tests/rowops_util.py, unchanged.

Guard words: every output is NaN before the call and carries a NaN margin behind its last row and, where the row stride exceeds D, behind
column D - 1 of every row; the margins must come back untouched, so a tail lane that writes past D is caught.  The inputs' margins hold NaN
too: a tail lane that READS past D poisons the row's statistics."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rowops_util as ru            # noqa: E402
import vit_narrow_util as nu        # noqa: E402
from gpu_util import DTYPES         # noqa: E402

NAN = float("nan")
G = nu.GUARD


@pytest.fixture(scope="module")
def ops():
    import eoe_amd.ops as o
    return o


def cu(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def p(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """a [rows, ld] buffer of NaN with G more NaN behind it; `.view` is its [rows, :cols] part"""

    def __init__(self, rows, cols, dtype=torch.float32, ld=None, fill=NAN):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.flat = torch.full((rows * self.ld + G,), NAN, dtype=dtype, device="cuda")
        self.body = self.flat[:rows * self.ld].view(rows, self.ld)
        if fill == fill:                   # not NaN: the part the kernel adds into
            self.body[:, :cols] = fill

    @property
    def view(self):
        return self.body[:, :self.cols]

    def ptr(self):
        return self.flat.data_ptr()

    def assert_margins(self, what):
        assert bool(torch.isnan(self.flat[self.rows * self.ld:]).all()), f"{what}: written behind the last row"
        if self.ld > self.cols:
            assert bool(torch.isnan(self.body[:, self.cols:]).all()), f"{what}: written behind column D - 1 of a row"


def padded(a, ld, dtype=None):
    """[rows, D] values in a [rows, ld] device buffer whose margin is NaN"""
    rows, D = a.shape
    t = torch.full((rows, ld), NAN, dtype=torch.float32)
    t[:, :D] = torch.from_numpy(a)
    return cu(t, dtype)


def ln_forward(ops, c, rows, D, out_dtype, ldx=None, with_stats=True):
    from eoe_amd import _lib
    ldx = ldx or D
    x = padded(c["x"], ldx)
    out = Guarded(rows, D, out_dtype)
    stats = Guarded(rows, 2) if with_stats else None
    out_f32 = 1 if out_dtype == torch.float32 else 0
    code = _lib.EOE_BF16 if out_f32 else ops.dtype_code(out_dtype)
    g, b = cu(c["g"]), cu(c["b"])          # (named: a temporary's memory is handed to the next allocation)
    _lib.check(_lib.lib.eoe_layernorm_fwd(p(x), ldx, p(g), p(b), out.ptr(), stats.ptr() if stats else None, rows, D, 1e-5,
                                          code, out_f32, ops._stream()), "eoe_layernorm_fwd")
    out.assert_margins("y")
    got = {"y" if out_f32 else "y16": out.view}
    if with_stats:
        stats.assert_margins("stats")
        got["mean"], got["rstd"] = stats.view[:, 0], stats.view[:, 1]
    return got


def ln_backward(ops, c, rows, D, dy_dtype, code_dtype, sel="all", want_dx16=False, ld=None, with_scratch=True):
    """one eoe_layernorm_bwd.  dy_dtype None: fp32 dy.  ld: ldx = ld_out (x, dres and dx_out at that row stride, NaN margins)"""
    from eoe_amd import _lib
    ld = ld or D
    x = padded(c["x"], ld)
    dres = padded(c["res"], ld) if c["res"] is not None else None
    dy = cu(c["dy"], dy_dtype)
    dx = Guarded(rows, D, ld=ld)
    dx16 = Guarded(rows, D, code_dtype) if want_dx16 else None
    outs = {k: Guarded(1, D, fill=0.0) for k in {"dx": (), "dxsum": ("dxsum",), "dgb": ("dgamma", "dbeta"), "all": ("dgamma", "dbeta", "dxsum")}[sel]}
    red = None
    if with_scratch and outs:
        red = torch.full((ops.LN_SCRATCH_ROWS * 3 * D,), NAN, device="cuda")          # EOE_LN_SCRATCH(D): a partial row read must have been written
    o = lambda k: outs[k].ptr() if k in outs else None                                 # noqa: E731
    stats, g = cu(ru.stats32(c["ref"])), cu(c["g"])
    _lib.check(_lib.lib.eoe_layernorm_bwd(p(dy), 1 if dy_dtype is None else 0, p(x), ld, p(stats), p(g), p(dres),
                                          dx.ptr(), ld, dx16.ptr() if dx16 else None, o("dgamma"), o("dbeta"), o("dxsum"), p(red), rows, D,
                                          ops.dtype_code(code_dtype), ops._stream()), "eoe_layernorm_bwd")
    got = {"dx": dx.view}
    dx.assert_margins("dx")
    if dx16:
        dx16.assert_margins("dx16")
        got["dx16"] = dx16.view
    for k, b in outs.items():
        b.assert_margins(k)
        got[k] = b.view[0]
    return got


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", nu.LN_ROWS)
@pytest.mark.parametrize("D", nu.LN_WIDTHS)
def test_layernorm_narrow(ops, D, rows, dtype):
    """forward (fp32 and 16-bit out, with the statistics) and the full backward (16-bit dy, dres, dx16, every reduction output)"""
    c = nu.ln_narrow_case(rows, D, dtype)
    specs = ru.ln_specs("plain", rows, D, c["ref"], dtype)
    ru.compare("fwd f32", ln_forward(ops, c, rows, D, torch.float32), c["ref"], specs, ("y", "mean", "rstd"))
    ru.compare("fwd 16-bit", ln_forward(ops, c, rows, D, dtype, with_stats=False), c["ref"], specs, ("y16",))
    got = ln_backward(ops, c, rows, D, dtype, dtype, want_dx16=True)
    ru.compare("bwd", got, c["ref"], specs, ("dx", "dx16", "dgamma", "dbeta", "dxsum"))


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("dy_dtype", [None] + list(DTYPES), ids=["dy_f32", "dy_bf16", "dy_f16"])
@pytest.mark.parametrize("D", nu.LN_WIDTHS)
def test_layernorm_bwd_narrow_instantiations_and_output_selections(ops, D, dy_dtype, with_res):
    """fp32 / 16-bit dy x with / without dres, each with no reduction output (the early return), dxsum only, dgamma + dbeta only and all
    of them, with and without dx16; the atomics path (no scratch) once.  dx does not depend on the selection"""
    rows = nu.LN_INST_ROWS
    c = nu.ln_narrow_case(rows, D, dy_dtype, with_res)
    code_dtype = dy_dtype or torch.bfloat16
    specs = ru.ln_specs("plain", rows, D, c["ref"], code_dtype)
    first = None
    for i, sel in enumerate(ru.LN_SELECTIONS):
        got = ln_backward(ops, c, rows, D, dy_dtype, code_dtype, sel=sel, want_dx16=bool(i & 1))
        ru.compare(f"sel {sel}", got, c["ref"], specs, tuple(got))
        first = got["dx"] if first is None else first
        assert torch.equal(got["dx"], first), f"dx differs between the output selections ({sel})"
    got = ln_backward(ops, c, rows, D, dy_dtype, code_dtype, sel="all", with_scratch=False)
    ru.compare("atomics", got, c["ref"], specs, tuple(got))
    assert torch.equal(got["dx"], first)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", nu.LN_WIDTHS)
def test_layernorm_narrow_strided_rows(ops, D, dtype):
    """ldx = ld_out = D + 64 > D: x, dres and dx_out at the wider stride, y / dy / dx16 compact; the 64 columns behind every row -- where a
    tail group's idle lanes would land -- hold NaN before and after"""
    rows, ld = nu.LN_STRIDED_ROWS, D + nu.LN_MARGIN
    for with_res in (True, False):
        c = nu.ln_narrow_strided_case(D, dtype, with_res)
        specs = ru.ln_specs("plain", rows, D, c["ref"], dtype)
        for out_dtype in (torch.float32, dtype):
            got = ln_forward(ops, c, rows, D, out_dtype, ldx=ld)
            ru.compare(f"fwd {out_dtype}", got, c["ref"], specs, tuple(got))
        got = ln_backward(ops, c, rows, D, dtype, dtype, want_dx16=not with_res, ld=ld)
        ru.compare(f"bwd res={with_res}", got, c["ref"], specs, tuple(got))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", (9, 4100))
def test_width_256_keeps_the_bits_of_the_untailed_path(ops, rows, dtype):
    """D = 256 has no tail.  The library serves one D by one code path, so the guarded calls above and the plain calls the model makes
    (ops.layernorm_fwd / layernorm_bwd, what tests/test_gpu_rowops.py holds to fp64) run the same instantiation: equal bits, run to run"""
    D = 256
    c = nu.ln_narrow_case(rows, D, dtype)
    x, g, b = cu(c["x"]), cu(c["g"]), cu(c["b"])
    for out_dtype in (torch.float32, dtype):
        out, stats = torch.full((rows, D), NAN, dtype=out_dtype, device="cuda"), torch.full((rows, 2), NAN, device="cuda")
        ops.layernorm_fwd(x, g, b, rows, D, D, out, stats)
        got = ln_forward(ops, c, rows, D, out_dtype)
        assert torch.equal(got["y" if out_dtype == torch.float32 else "y16"], out)
        assert torch.equal(got["mean"], stats[:, 0]) and torch.equal(got["rstd"], stats[:, 1])
    plain = {k: torch.zeros(D, device="cuda") for k in ("dgamma", "dbeta", "dxsum")}
    dx, dx16 = torch.full((rows, D), NAN, device="cuda"), torch.full((rows, D), NAN, dtype=dtype, device="cuda")
    ops.layernorm_bwd(cu(c["dy"], dtype), x, cu(ru.stats32(c["ref"])), g, rows, D, D, dx, D, dres=cu(c["res"]), dx16=dx16, **plain)
    for _ in range(2):
        got = ln_backward(ops, c, rows, D, dtype, dtype, want_dx16=True)
        assert torch.equal(got["dx"], dx) and torch.equal(got["dx16"], dx16)
        for k, v in plain.items():
            assert torch.equal(got[k], v), k


# ------------------------------------------------------------------------------------------------ embed + ln_pre
@pytest.mark.parametrize("D,n,L", nu.EMBED_CASES)
def test_embed_lnpre_fwd_narrow(ops, D, n, L):
    from eoe_amd import _lib
    c = ru.embed_case(D, n, L)
    x0, y, stats = Guarded(n * L, D), Guarded(n * L, D), Guarded(n * L, 2)
    ins = [cu(c[k]) for k in ("tok", "cls", "pos", "g", "b")]
    _lib.check(_lib.lib.eoe_embed_lnpre_fwd(*[p(t) for t in ins], x0.ptr(), y.ptr(), stats.ptr(), n, L, D, 1e-5, ops._stream()), "eoe_embed_lnpre_fwd")
    for name, buf in (("x0", x0), ("y", y), ("stats", stats)):
        buf.assert_margins(name)
    assert torch.equal(x0.view.cpu(), c["got32"]["x0"]), "x0 is one fp32 addition per element"
    ru.compare("embed fwd", {"y": y.view, "mean": stats.view[:, 0], "rstd": stats.view[:, 1]}, c["ref"], ru.embed_specs(c), ("y", "mean", "rstd"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,n,L", nu.EMBED_CASES)
def test_embed_lnpre_bwd_narrow(ops, dtype, D, n, L):
    """partial rows + finish kernel (scratch given) and atomics (scratch NULL): both against fp64, both adding into dcls / dpos /
    dgamma / dbeta, and the same dtok bits"""
    from eoe_amd import _lib
    c = ru.embed_case(D, n, L)
    specs = ru.embed_specs(c, dtype)
    ins = [cu(c["dy"]), cu(c["got32"]["x0"]), cu(ru.stats32(c["ref"])), cu(c["g"])]
    dtoks = []
    for with_scratch in (True, False):
        dtok = Guarded(n * (L - 1), D, dtype)
        acc = {"dcls": Guarded(1, D), "dpos": Guarded(L, D), "dgamma": Guarded(1, D), "dbeta": Guarded(1, D)}
        for k, buf in acc.items():
            buf.view.copy_(cu(c["pre"][k]).reshape(buf.view.shape))
        part = torch.full((L * 2 * D,), NAN, device="cuda") if with_scratch else None
        _lib.check(_lib.lib.eoe_embed_lnpre_bwd(*[p(t) for t in ins], dtok.ptr(), acc["dcls"].ptr(), acc["dpos"].ptr(), acc["dgamma"].ptr(),
                                                acc["dbeta"].ptr(), p(part), n, L, D, ops.dtype_code(dtype), ops._stream()), "eoe_embed_lnpre_bwd")
        dtok.assert_margins("dtok")
        got = {"dtok": dtok.view, "dpos": acc["dpos"].view}
        for k, buf in acc.items():
            buf.assert_margins(k)
            if k != "dpos":
                got[k] = buf.view[0]
        ru.compare(f"embed bwd scratch={with_scratch}", got, c["ref"], specs, ("dtok", "dcls", "dpos", "dgamma", "dbeta"))
        dtoks.append(dtok.view.clone())
    assert torch.equal(dtoks[0], dtoks[1]), "dtok differs between the partial-row and the atomics path"
