"""GPU: explaining the BatchNorm CNNs (CNN32, CNN28).  The first-layer data gradient back to the image (eoe_conv_image_dgrad) against its
float64 statement under a derived bound, the eval-mode BatchNorm backward through `conv_bn_act_pool` and `BnActFunction` against float64
autograd, `explain.input_gradient` against autograd through the fp64 oracle, its side effects, and the trainer option.  Case tables,
floors, bars and the measured distances: tests/explain_cnn_util.py."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bnpool_util as bu                                          # noqa: E402
import explain_cnn_util as cu                                     # noqa: E402
from gpu_util import DTYPES, assert_close                         # noqa: E402
from oracle import models as omodels                              # noqa: E402

EOE_ERR_ARG = 1


def guarded(shape):
    """an fp32 output tensor with cu.GUARD elements of NaN behind it: (the view to write, the guard)"""
    n = int(np.prod(shape))
    buf = torch.full((n + cu.GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[:n].view(shape), buf[n:]


def guard_intact(guard):
    return bool(torch.isnan(guard).all())


@pytest.fixture(autouse=True)
def _restore():
    import eoe_amd
    from eoe_amd import ops
    old, old_scale, old_parity = eoe_amd.compute_dtype(), ops.grad_scale(), ops._parity
    yield
    eoe_amd.set_compute_dtype(old)
    ops.set_grad_scale(old_scale)
    eoe_amd.set_parity_mode(old_parity)


# ------------------------------------------------------------------------------------------------ the kernel alone
def image_dgrad(dy, w, std, scale_inv, n, cin, cout, Hi, k, stride, pad, code):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    dx, guard = guarded((n, cin, Hi, Hi))
    check(lib.eoe_conv_image_dgrad(dy.data_ptr(), w.data_ptr(), ops._p(std), scale_inv, dx.data_ptr(), n, cin, cout, Hi, Hi, k, k, stride,
                                   pad, code, ops._stream()), "eoe_conv_image_dgrad")
    torch.cuda.synchronize()
    assert guard_intact(guard)
    return dx.cpu()


@pytest.mark.parametrize("n", cu.DGRAD_N)
@pytest.mark.parametrize("cin,cout,k,stride,pad,Hi", cu.DGRAD_CASES)
def test_conv_image_dgrad_against_its_float64_statement(cin, cout, k, stride, pad, Hi, n):
    """dy in fp16, bf16 and fp32, std NULL and given, scale_inv 1 and 1 / 256; the reference is the float64 statement on the same
    rounded dy and the fp32 weights, the bound per element (k k cout + 4) 2^-24 (scale_inv / std[c]) sum |dy w|; two runs give the
    same bytes; the guard behind dx stays intact"""
    from eoe_amd import _lib, ops
    from eoe_amd.explain import conv_image_dgrad_np
    dy32, w = cu.dgrad_case(cin, cout, k, stride, pad, Hi, n)
    wd = torch.from_numpy(w).cuda()
    stdt = torch.tensor(cu.DGRAD_STD[:cin])
    for dt, code in ((torch.float16, _lib.EOE_F16), (torch.bfloat16, _lib.EOE_BF16), (torch.float32, _lib.EOE_F32)):
        dyd = torch.from_numpy(dy32).to(dt).cuda()
        dyq = dyd.float().cpu().numpy()
        for std in (None, stdt):
            for scale_inv in cu.DGRAD_SCALE_INV:
                stdn = None if std is None else std.numpy()
                got = image_dgrad(dyd, wd, None if std is None else std.cuda(), scale_inv, n, cin, cout, Hi, k, stride, pad, code)
                ref = conv_image_dgrad_np(dyq, w, n, Hi, Hi, stride, pad, stdn, scale_inv)
                bound = cu.dgrad_bound(dyq, w, n, Hi, stride, pad, stdn, scale_inv)
                err = np.abs(got.double().numpy() - ref)
                worst = float((err / np.maximum(bound, 1e-300)).max())
                print(f"[{cin}->{cout} k{k} s{stride} p{pad} {Hi} n{n} {dt} std={std is not None} x{scale_inv:g}] err / bound {worst:.3f}")
                assert (err <= bound).all(), worst
                again = image_dgrad(dyd, wd, None if std is None else std.cuda(), scale_inv, n, cin, cout, Hi, k, stride, pad, code)
                assert torch.equal(got, again)
        # the wrapper: the same bytes
        via = ops.conv_image_dgrad(dyd, wd, n, Hi, Hi, stride, pad, std=stdt.cuda(), scale_inv=cu.DGRAD_SCALE_INV[-1])
        assert torch.equal(via.cpu(), got)
    if (k, stride, pad, Hi) == (3, 2, 0, 6):
        assert (got[:, :, -1, :] == 0).all() and (got[:, :, :, -1] == 0).all()


def test_conv_image_dgrad_refuses_what_it_does_not_serve_and_takes_no_images():
    from eoe_amd import _lib, ops
    lib = _lib.lib
    dy, w = torch.zeros(3 * 32 * 32 * 32, device="cuda"), torch.zeros(64 * 3 * 49, device="cuda")
    dx = torch.full((3 * 3 * 32 * 32,), 12345.0, device="cuda")

    def call(n=3, cin=3, cout=32, Hi=32, Wi=32, kh=5, kw=5, stride=1, pad=2, code=_lib.EOE_F32, dyp=None):
        return lib.eoe_conv_image_dgrad(dy.data_ptr() if dyp is None else dyp, w.data_ptr(), None, 1.0, dx.data_ptr(), n, cin, cout, Hi, Wi,
                                        kh, kw, stride, pad, code, ops._stream())
    bad = (dict(cin=2), dict(cin=4), dict(cout=30), dict(cout=0), dict(kh=5, kw=3), dict(kh=4, kw=4, pad=1), dict(kh=9, kw=9, pad=4),
           dict(stride=3), dict(stride=0), dict(pad=5), dict(pad=-1), dict(code=0), dict(code=7), dict(n=-1), dict(Hi=0),
           dict(Hi=2, Wi=2, kh=7, kw=7, pad=2), dict(dyp=dy.data_ptr() + 4), dict(dyp=dy.data_ptr() + 2, code=_lib.EOE_F16))
    for kw_ in bad:
        assert call(**kw_) == EOE_ERR_ARG, kw_
        assert lib.eoe_last_error()
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((dx == 12345.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dx == 0).all())


# ------------------------------------------------------------------------------------------------ eval-mode BatchNorm backward
def _unit_inputs(tag, C, flat_out):
    """a conv unit in front of BatchNorm with C channels: C = 16 CNN28's conv1 (image), 32 CNN32's conv1 (image), 128 CNN32's conv3"""
    from oracle import fill
    cin, Hi, image = {16: (1, 28, True), 32: (3, 32, True), 128: (64, 8, False)}[C]
    n = 3
    f = lambda name, shape, **k: torch.from_numpy(fill.fill(f"explain_cnn/bn/{tag}/{C}/{name}", shape, **k).astype(np.float32))   # noqa: E731
    x = f("x", (n, cin, Hi, Hi))
    Ho = Hi // 2
    p = dict(x=x, w=f("w", (C, cin, 5, 5), std=(cin * 25) ** -0.5), cb=f("cb", (C,), std=0.02), g=f("g", (C,), std=0.05, mean=1.0),
             b=f("b", (C,), std=0.02), rm=f("rm", (C,), std=0.3, mean=0.1), rv=0.6 + f("rv", (C,), std=0.8).abs(),
             dout=f("dout", (n, C * Ho * Ho) if flat_out else (n, Ho, Ho, C)))
    return p, image, n, Hi


@pytest.mark.parametrize("flat_out", [False, True])
@pytest.mark.parametrize("C", [16, 32, 128])
def test_eval_mode_batchnorm_backward_through_the_conv_unit(C, flat_out, monkeypatch):
    """`_bn_act_pool_bwd` with training=False (dy = gamma rstd g over the running statistics) reached through `conv_bn_act_pool` in
    parity mode (fp32 convolution, so that the winners of the pool windows are the oracle's), pool 2: its dy, dgamma and dbeta against
    float64 autograd through oracle.models.batch_norm in eval mode, at bnpool_util.TOL_BN_GRAD = (1e-3, 1e-4) -- what
    tests/test_gpu_bnpool.py holds the training form's dy, dgamma and dbeta to.  The running buffers stay bit-equal."""
    import eoe_amd
    from eoe_amd import ops
    eoe_amd.set_parity_mode(True)
    p, image, n, Hi = _unit_inputs("unit", C, flat_out)
    # float64 reference
    r = {k: v.double().requires_grad_(k in ("w", "cb", "g", "b")) for k, v in p.items()}
    y = F.conv2d(r["x"], r["w"], r["cb"], stride=1, padding=2)
    y.retain_grad()
    out = F.max_pool2d(F.leaky_relu(omodels.batch_norm(y, r["g"], r["b"], r["rm"], r["rv"], False, 0.1, 1e-4), 0.01), 2, 2)
    dout = r["dout"].reshape(out.shape) if flat_out else r["dout"].permute(0, 3, 1, 2)
    (out * dout).sum().backward()
    ref = {"dy": y.grad.permute(0, 2, 3, 1).reshape(-1, C), "dgamma": r["g"].grad, "dbeta": r["b"].grad}
    # the unit
    d = {k: v.cuda() for k, v in p.items()}
    for k in ("w", "cb", "g", "b"):
        d[k].requires_grad_()
    rm0, rv0, nbt = d["rm"].clone(), d["rv"].clone(), torch.full((), 7, dtype=torch.int64, device="cuda")
    xin = d["x"] if image else d["x"].permute(0, 2, 3, 1).contiguous()
    cfg = ops.ConvUnit(training=False, eps=1e-4, momentum=0.1, pool=2, is_image=image, mean=None, std=None, flat_out=flat_out)
    seen = {}
    real = ops._bn_act_pool_bwd
    monkeypatch.setattr(ops, "_bn_act_pool_bwd", lambda *a, **k: seen.setdefault("out", real(*a, **k)))
    o = ops.conv_bn_act_pool(xin, d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], nbt, cfg)
    assert_close(o.cpu(), (out.detach().reshape(n, -1) if flat_out else out.detach().permute(0, 2, 3, 1)), rtol=1e-4, atol=1e-4, what="forward")
    o.backward(d["dout"])
    torch.cuda.synchronize()
    dy, dg, db = seen["out"]
    got = {"dy": dy, "dgamma": dg, "dbeta": db}
    assert dy.dtype == torch.float32 and torch.equal(d["g"].grad, dg) and torch.equal(d["b"].grad, db)
    bu.compare(f"eval bn bwd C={C} flat={flat_out}", got, ref, {k: bu.tol(bu.TOL_BN_GRAD) for k in got})
    assert torch.equal(d["rm"], rm0) and torch.equal(d["rv"], rv0) and int(nbt) == 7


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flat_out", [False, True])
@pytest.mark.parametrize("C", [16, 32, 128])
def test_eval_mode_batchnorm_backward_writes_a_16_bit_dy_on_the_fast_path(C, flat_out, dtype, monkeypatch):
    """the same units on the fast path (16-bit convolution GEMM, dy in the compute dtype): the dy, dgamma and dbeta `_bn_act_pool_bwd`
    returns against float64 autograd through oracle.models.batch_norm in eval mode on the very y the kernel read (the fp32 convolution
    output the forward saved; eval mode never saves a 16-bit y, which needs the GEMM's batch statistics), so the convolution's 16-bit
    rounding is on both sides.  dy at bnpool_util.tol16(TOL_BN_GRAD, dtype), dgamma and dbeta at TOL_BN_GRAD: what tests/test_gpu_bnpool.py
    holds the training form's 16-bit dy to."""
    import eoe_amd
    from eoe_amd import ops
    eoe_amd.set_compute_dtype(dtype)
    eoe_amd.set_parity_mode(False)
    p, image, n, Hi = _unit_inputs("unit", C, flat_out)
    d = {k: v.cuda() for k, v in p.items()}
    for k in ("w", "cb", "g", "b"):
        d[k].requires_grad_()
    nbt = torch.full((), 7, dtype=torch.int64, device="cuda")
    xin = d["x"] if image else d["x"].permute(0, 2, 3, 1).contiguous()
    cfg = ops.ConvUnit(training=False, eps=1e-4, momentum=0.1, pool=2, is_image=image, mean=None, std=None, flat_out=flat_out)
    seen = {}
    real = ops._bn_act_pool_bwd

    def spy(*a, **k):
        seen["y"], seen["out"] = a[0], real(*a, **k)
        return seen["out"]
    monkeypatch.setattr(ops, "_bn_act_pool_bwd", spy)
    ops.conv_bn_act_pool(xin, d["w"], d["cb"], d["g"], d["b"], d["rm"], d["rv"], nbt, cfg).backward(d["dout"])
    torch.cuda.synchronize()
    dy, dg, db = seen["out"]
    assert dy.dtype == dtype and seen["y"].dtype == torch.float32 and seen["y"].shape == (n * Hi * Hi, C)
    # float64 reference on the saved y
    r = {k: p[k].double().requires_grad_(k in ("g", "b")) for k in ("g", "b", "rm", "rv", "dout")}
    y = seen["y"].cpu().double().reshape(n, Hi, Hi, C).permute(0, 3, 1, 2).requires_grad_()
    out = F.max_pool2d(F.leaky_relu(omodels.batch_norm(y, r["g"], r["b"], r["rm"], r["rv"], False, 0.1, 1e-4), 0.01), 2, 2)
    dout = r["dout"].reshape(out.shape) if flat_out else r["dout"].permute(0, 3, 1, 2)
    (out * dout).sum().backward()
    ref = {"dy": y.grad.permute(0, 2, 3, 1).reshape(-1, C), "dgamma": r["g"].grad, "dbeta": r["b"].grad}
    specs = {"dy": bu.tol(bu.tol16(bu.TOL_BN_GRAD, dtype)), "dgamma": bu.tol(bu.TOL_BN_GRAD), "dbeta": bu.tol(bu.TOL_BN_GRAD)}
    bu.compare(f"eval bn bwd fast C={C} flat={flat_out} {dtype}", {"dy": dy, "dgamma": dg, "dbeta": db}, ref, specs)
    assert int(nbt) == 7


def test_eval_mode_batchnorm1d_backward():
    """BnActFunction at [3, 64] with training=False against float64 autograd, bnpool_util.TOL_BN_GRAD as above"""
    from eoe_amd import ops
    from oracle import fill
    C = 64
    f = lambda name, shape, **k: torch.from_numpy(fill.fill(f"explain_cnn/bn1d/{name}", shape, **k).astype(np.float32))   # noqa: E731
    p = dict(y=f("y", (3, C)), g=f("g", (C,), std=0.05, mean=1.0), b=f("b", (C,), std=0.02), rm=f("rm", (C,), std=0.3, mean=0.1),
             rv=0.6 + f("rv", (C,), std=0.8).abs(), dout=f("dout", (3, C)))
    r = {k: v.double().requires_grad_(k in ("y", "g", "b")) for k, v in p.items()}
    (F.leaky_relu(omodels.batch_norm(r["y"], r["g"], r["b"], r["rm"], r["rv"], False, 0.1, 1e-4), 0.01) * r["dout"]).sum().backward()
    d = {k: v.cuda() for k, v in p.items()}
    for k in ("y", "g", "b"):
        d[k].requires_grad_()
    nbt = torch.full((), 7, dtype=torch.int64, device="cuda")
    rm0, rv0 = d["rm"].clone(), d["rv"].clone()
    ops.BnActFunction.apply(d["y"], d["g"], d["b"], d["rm"], d["rv"], nbt, (False, 1e-4, 0.1)).backward(d["dout"])
    got = {"dy": d["y"].grad, "dgamma": d["g"].grad, "dbeta": d["b"].grad}
    ref = {"dy": r["y"].grad, "dgamma": r["g"].grad, "dbeta": r["b"].grad}
    bu.compare("eval bn1d bwd", got, ref, {k: bu.tol(bu.TOL_BN_GRAD) for k in got})
    assert torch.equal(d["rm"], rm0) and torch.equal(d["rv"], rv0) and int(nbt) == 7
    # asked for the input's gradient alone: the same dy, no parameter gradient
    y2 = d["y"].detach().clone().requires_grad_()
    o = ops.BnActFunction.apply(y2, d["g"].detach(), d["b"].detach(), d["rm"], d["rv"], nbt, (False, 1e-4, 0.1))
    (gy,) = torch.autograd.grad(o, y2, d["dout"])
    assert torch.equal(gy, d["y"].grad)


# ------------------------------------------------------------------------------------------------ end to end
def eoe_cnn(name, bias, norm, fc2_gain=1.0, bn1d_var_gain=1.0):
    import eoe_amd.models as emodels
    m = cu.build(emodels, name, bias, fc2_gain, bn1d_var_gain).cuda().train()
    if norm:
        m.set_normalize(*cu.normalize_of(name, True))
    return m


def input_grad_distance(name, bias, norm, dtype, scale, parity=False):
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype(dtype)
    eoe_amd.set_parity_mode(parity)
    ops.set_grad_scale(scale)
    ref = cu.oracle_grad(name, bias, norm)
    got = explain.input_gradient(eoe_cnn(name, bias, norm), cu.images_of(name).cuda(), explain.score_fn("hsc"))
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    return cu.distance(got.cpu(), ref)


@pytest.mark.parametrize("dtype,scale", cu.DTYPE_SCALES)
@pytest.mark.parametrize("name,bias,norm", cu.CASES)
def test_input_gradient_against_autograd_through_the_fp64_oracle(name, bias, norm, dtype, scale):
    """fast mode: the worst image's relative rms distance; fp16 at gradient scale 1 and at 256 meets the same bar, so the scale is
    undone exactly.  Floors, bars and the measured table: explain_cnn_util.FLOOR / INPUT_GRAD_BAR / INPUT_GRAD_MEASURED"""
    dist = input_grad_distance(name, bias, norm, dtype, scale)
    fl = cu.FLOOR[dtype][(name, bias, norm)]
    print(f"[{name} bias={bias} norm={norm} {dtype} scale={scale:g}] input-gradient rel rms {dist:.3e} (the case's floor {fl:.3e})")
    assert dist <= cu.INPUT_GRAD_BAR[dtype][name] and dist <= cu.CEILING_FACTOR * fl, dist


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,bias,norm", cu.CASES)
def test_input_gradient_in_parity_mode(name, bias, norm, dtype):
    dist = input_grad_distance(name, bias, norm, dtype, 1.0, parity=True)
    print(f"[parity {name} bias={bias} norm={norm} {dtype}] input-gradient rel rms {dist:.3e}")
    assert dist <= cu.PARITY_BAR[name] and dist <= cu.PARITY_CEILING, dist


@pytest.mark.parametrize("scale", [1.0, 256.0])
@pytest.mark.parametrize("name,gain,var_gain", cu.SATURATED_CASES)
def test_a_saturated_score_still_has_a_gradient(name, gain, var_gain, scale):
    """fc2 x gain (bias, Normalize fused): the HSC score is 1 in fp32 to within an ulp and d score / d out of order exp(-|out|), down to
    1e-30: fp16's dy chain flushes such a gradient behind any fixed seed, the per-image power-of-two seed carries it.  Every image's
    gradient must be finite and not 0, at gradient scale 1 and 256.  fc2 x 64 runs with bn1d1's running variance raised so that
    exp(-|out|) is an fp32 number at all: explain_cnn_util.SATURATED_CASES has the reasoning and the figures."""
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype(torch.float16)
    ops.set_grad_scale(scale)
    m = eoe_cnn(name, True, True, fc2_gain=gain, bn1d_var_gain=var_gain)
    x = cu.images_of(name).cuda()
    with torch.no_grad():
        score = explain.score_fn("hsc")(m.eval()(x))
    got = explain.input_gradient(m, x, explain.score_fn("hsc"))
    print(f"[{name} gain={gain:g} var x{var_gain:g} scale={scale:g}] scores {score.tolist()}, per-image |grad| max {got.abs().flatten(1).amax(1).tolist()}")
    assert float(score.min()) > 0.999
    assert torch.isfinite(got).all() and bool((got.abs().flatten(1).amax(1) > 0).all())


def test_input_gradient_leaves_no_trace():
    """CNN32 with bias: no parameter gets a .grad, a registered gradient arena keeps its bytes, the running buffers and
    num_batches_tracked stay bit-equal, the train / eval flags and requires_grad come back, two calls give the same bytes, and a
    training step behind the call has the loss and gradient bits of one without it"""
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype(torch.float16)
    ops.set_grad_scale(256.0)
    imgs = cu.images_of("CNN32").cuda()
    lbls = torch.tensor([0, 1, 1], device="cuda")

    def step(m):
        loss = eoe_amd.hsc_loss(m(imgs), lbls, 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, \
            {n: b.detach().clone() for n, b in m.named_buffers()}

    loss0, grads0, bufs0 = step(eoe_cnn("CNN32", True, True))
    m = eoe_cnn("CNN32", True, True)
    m.bn2d2.eval()                                                     # a mixed set of flags must come back as it was
    m.fc2.bias.requires_grad_(False)
    flags = {n: mod.training for n, mod in m.named_modules()}
    req = {n: p.requires_grad for n, p in m.named_parameters()}
    arena = {}
    for n, p in m.named_parameters():                                  # what parallel.GradArena registers: a poisoned view per parameter
        arena[n] = torch.full_like(p, 12345.0)
        p._eoe_grad_buf = arena[n]
    before = {n: b.detach().clone() for n, b in m.named_buffers()}
    a = explain.input_gradient(m, imgs, explain.score_fn("hsc"))
    b = explain.input_gradient(m, imgs, explain.score_fn("hsc"))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not imgs.requires_grad and a.abs().sum() > 0
    assert all(p.grad is None for p in m.parameters())
    assert all(bool((t == 12345.0).all()) for t in arena.values())
    assert all(torch.equal(before[n], buf) for n, buf in m.named_buffers()) and int(m.bn2d1.num_batches_tracked) == 7
    assert {n: mod.training for n, mod in m.named_modules()} == flags and m.training
    assert {n: p.requires_grad for n, p in m.named_parameters()} == req
    for p in m.parameters():
        del p._eoe_grad_buf
    m.bn2d2.train()
    m.fc2.bias.requires_grad_(True)
    loss1, grads1, bufs1 = step(m)
    assert torch.equal(loss0, loss1) and set(grads0) == set(grads1)
    for n in grads0:
        assert torch.equal(grads0[n], grads1[n]), n
    for n in bufs0:
        assert torch.equal(bufs0[n], bufs1[n]), n


# ------------------------------------------------------------------------------------------------ trainer
def _task(name):
    """a small resident set for CNN32 (RGB 32 x 32) / CNN28 (grayscale 28 x 28) on the pattern of test_gpu_explain.small_task, the
    encoder trained for one epoch"""
    import eoe_amd
    import eoe_amd.models as emodels
    from eoe_amd.data import ResidentImageSource
    from eoe_amd.training import TRAINER
    ch, res = cu.IMAGE[name]
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, res), torch.linspace(0, 1, res), indexing="ij")

    def make(k, n):
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)[..., :ch]
        img = (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, res, res, ch), generator=g)).clamp(0, 255).to(torch.uint8)
        return img if ch == 3 else img[..., 0]
    test_y = torch.tensor([0, 1] * 8)
    test = torch.stack([make(int(y), 1)[0] for y in test_y])
    kw = dict(crop=res, mean=(0.5,) * ch, std=(0.25,) * ch, seed=3)
    ds = ResidentImageSource(make(0, 32), make(1, 32), test, test_y, grayscale=(ch == 1), **kw)
    torch.manual_seed(0)
    m0 = getattr(emodels, name)(bias=True)
    tr = TRAINER["hsc"](m0, dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"])
    model, _ = tr.train_cls(copy.deepcopy(m0), ds, 0, "only", 0)
    return ds, m0, model


@pytest.mark.parametrize("name", cu.MODELS)
def test_trainer_explains_a_cnn_and_changes_nothing_when_off(name, tmp_path):
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    ds, m0, model = _task(name)
    res = cu.IMAGE[name][1]
    kw = dict(dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"])
    on = TRAINER["hsc"](m0, logger=JsonLogger(str(tmp_path / "on")), extremes=2, explain=True, **kw)
    off = TRAINER["hsc"](m0, logger=JsonLogger(str(tmp_path / "off")), extremes=2, explain=False, **kw)
    never = TRAINER["hsc"](m0, logger=JsonLogger(str(tmp_path / "never")), extremes=2, **kw)
    res_on, res_off, res_never = (t.eval_cls(model, ds, 0, "only", 0) for t in (on, off, never))
    key = "eval_cls0_it0"
    assert list(on.explanations) == [key] and off.explanations == {} and never.explanations == {}
    maps = on.explanations[key]
    ex = on.extremes[key]
    rows = sum(min(2, len(r)) for r in (ex.most[0][0], ex.least[0][0], ex.most[1][0], ex.least[1][0]) if len(r))
    assert maps.shape == (rows, res, res) and rows == 8 and maps.dtype == torch.float32 and torch.isfinite(maps).all() and maps.max() > 0
    assert all(p.grad is None for p in model.parameters())
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off", "never")}
    extra = sorted(set(files["on"]) - set(files["off"]))
    assert files["off"] == files["never"] and set(files["off"]) <= set(files["on"])
    assert extra and all(f.startswith("eval_cls0-only_it0_extremes_heat") for f in extra) and any(f.endswith(".png") for f in extra), files
    for f in files["off"]:
        if os.path.isfile(tmp_path / "off" / f):
            assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "never" / f).read_bytes() == (tmp_path / "on" / f).read_bytes(), f
    assert on.extremes[key].as_dict() == off.extremes[key].as_dict() == never.extremes[key].as_dict()
    assert [(r.auc, p.avg_prec) for r, p in (res_on, res_off)] == [(res_never[0].auc, res_never[1].avg_prec)] * 2
    # attention is refused before scoring: no loader is asked for
    att = TRAINER["hsc"](m0, extremes=2, attention=True, **kw)
    asked = []
    real = ds.loaders
    ds.loaders = lambda *a, **k: (asked.append(1), real(*a, **k))[1]
    try:
        with pytest.raises(NotImplementedError, match="attention=True needs a ViT encoder"):
            att.eval_cls(model, ds, 0, "only", 0)
    finally:
        del ds.loaders
    assert not asked
    eoe_amd.set_compute_dtype(old)
