"""Grad-CAM on the device: the map kernels (csrc/gradcam.hip) against the numpy statements within a derived bound, the data-only CBAM
junction backward against the full one in bytes, WideResNet in two halves, and `explain.grad_cam` against autograd through the fp64
oracle, with what it must leave untouched."""
import copy
import os

import numpy as np
import pytest
import torch

import gradcam_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _modes():
    import eoe_amd
    from eoe_amd import ops
    dt, par, gs = eoe_amd.compute_dtype(), ops.parity_mode(), ops.grad_scale()
    yield
    eoe_amd.set_compute_dtype(dt)
    eoe_amd.set_parity_mode(par)
    ops.set_grad_scale(gs)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n,h,w,C", gu.MAP_CASES)
def test_map_kernels_against_numpy(n, h, w, C):
    from eoe_amd import explain
    A, dA = gu.act_case(n, h, w, C)
    a, d = torch.from_numpy(A).cuda(), torch.from_numpy(dA).cuda()
    alpha = explain.cam_weights(d).cpu().numpy().astype(np.float64)
    mean = dA.astype(np.float64).mean(axis=(1, 2))
    assert (np.abs(alpha - mean) <= (h * w + 1) * gu.U * np.abs(dA.astype(np.float64)).mean(axis=(1, 2)) + 1e-45).all()
    for mode in gu.MODES:
        got = explain.cam_map(a, d, mode)
        again = explain.cam_map(a, d, mode)
        assert torch.equal(got, again)                                    # two runs, equal bytes
        g = got.cpu().numpy()
        want = explain.cam_np(A, dA, mode)
        err, bound = np.abs(g.astype(np.float64) - want), gu.cam_bound(A, dA, mode)
        print(f"cam_map n={n} {h}x{w}x{C} {mode}: max err {err.max():.3e}, smallest slack {(bound - err).min():.3e}")
        assert (err <= bound + 1e-45).all(), (mode, float((err - bound).max()))
        if n > 1:
            assert (g[0] == 0).all() and g[1].min() > 0                   # exact zeros where relu clips
        zero = explain.cam_map(a, torch.zeros_like(d), mode)
        assert (zero == 0).all()


@pytest.mark.parametrize("hw,HW", gu.UPSAMPLE_CASES)
def test_upsample_against_numpy(hw, HW):
    from eoe_amd import explain
    (h, w), (H, W) = hw, HW
    for n in gu.N_IMAGES:
        m = gu.act_case(n, h, w, 4, "up")[0][..., 0].copy()
        dev = torch.from_numpy(m).cuda()
        got = explain.cam_upsample(dev, H, W)
        assert torch.equal(got, explain.cam_upsample(dev, H, W))
        g = got.cpu().numpy()
        err = np.abs(g.astype(np.float64) - explain.bilinear_np(m, H, W))
        print(f"cam_upsample n={n} {h}x{w} -> {H}x{W}: max err {err.max():.3e}")
        assert g.shape == (n, H, W) and (err <= gu.upsample_bound(m, H, W) + 1e-45).all()
        if (h, w) == (H, W):
            assert np.array_equal(g, m)
        if (h, w) == (1, 1):
            assert (g == m.reshape(n, 1, 1)).all()


def test_non_finite_entries_propagate():
    from eoe_amd import explain
    A, dA = gu.act_case(1, 3, 5, 64)
    A[0, 1, 2, 7] = np.nan
    a, d = torch.from_numpy(A).cuda(), torch.from_numpy(dA).cuda()
    gc = explain.cam_map(a, d, "gradcam").cpu().numpy()
    assert np.isnan(gc[0, 1, 2]) and np.isfinite(gc[0, 0, 0])
    A[0, 2, 4, 1], dA[0, 2, 4, 1] = 1.0, np.inf
    a, d = torch.from_numpy(A).cuda(), torch.from_numpy(dA).cuda()
    hi = explain.cam_map(a, d, "hirescam").cpu().numpy()
    assert np.isnan(hi[0, 1, 2]) and np.isposinf(hi[0, 2, 4]) and np.isfinite(hi[0, 0, 0])
    up = explain.cam_upsample(torch.from_numpy(hi).cuda(), 12, 20).cpu().numpy()
    assert np.isnan(up).any() and np.isfinite(up[0, 0, 0])


def test_kernels_refuse_bad_arguments_and_take_n_zero():
    from eoe_amd import _lib
    lib = _lib.lib
    a = torch.zeros((2, 3, 3, 8), device="cuda")
    alpha, m, out = torch.zeros((2, 8), device="cuda"), torch.zeros((2, 3, 3), device="cuda"), torch.zeros((2, 6, 6), device="cuda")
    p = lambda t: t.data_ptr()
    bad = [lib.eoe_cam_weights(None, p(alpha), 2, 3, 3, 8, None), lib.eoe_cam_weights(p(a), p(alpha), 2, 3, 3, 6, None),
           lib.eoe_cam_weights(p(a) + 4, p(alpha), 2, 3, 3, 8, None), lib.eoe_cam_weights(p(a), p(alpha), 1 << 20, 64, 64, 512, None),
           lib.eoe_cam_weights(p(a), p(alpha), 2, 0, 3, 8, None),
           lib.eoe_cam_map(p(a), p(a), p(alpha), None, 2, 3, 3, 8, 0, None), lib.eoe_cam_map(p(a), p(a), None, p(m), 2, 3, 3, 8, 0, None),
           lib.eoe_cam_map(p(a), None, p(alpha), p(m), 2, 3, 3, 8, 1, None), lib.eoe_cam_map(p(a), p(a), p(alpha), p(m), 2, 3, 3, 8, 2, None),
           lib.eoe_cam_map(p(a), p(a), p(alpha), p(m), 2, 3, 3, 10, 0, None), lib.eoe_cam_map(p(a) + 8, p(a), p(alpha), p(m), 2, 3, 3, 8, 0, None),
           lib.eoe_cam_upsample(p(m), p(out), 2, 3, 3, 2, 6, None), lib.eoe_cam_upsample(p(m), p(out), 2, 3, 3, 6, 2, None),
           lib.eoe_cam_upsample(None, p(out), 2, 3, 3, 6, 6, None), lib.eoe_cam_upsample(p(m), p(out), 1 << 20, 3, 3, 64, 64, None)]
    assert all(rc != 0 for rc in bad), bad
    out.fill_(5.0)
    assert lib.eoe_cam_weights(p(a), p(alpha), 0, 3, 3, 8, None) == 0 and lib.eoe_cam_map(p(a), p(a), p(alpha), p(m), 0, 3, 3, 8, 0, None) == 0
    assert lib.eoe_cam_upsample(p(m), p(out), 0, 3, 3, 6, 6, None) == 0
    torch.cuda.synchronize()
    assert (out == 5.0).all()


# ------------------------------------------------------------------------------------------------ the CBAM junction
def _junction(n, H, W, C, params_need_grad):
    """(out, dx, g) of CbamJunctionFunction in eval mode on the case's inputs; the parameters require a gradient (the full backward) or
    not (the data-only one)"""
    from eoe_amd import ops_resnet
    from eoe_amd.models.cbam import CBAM
    cb = CBAM(C, 16)
    cb.load_state_dict(gu.oracle_cbam(C).state_dict())
    cb = cb.cuda().eval()
    for prm in cb.parameters():
        prm.requires_grad_(params_need_grad)
    x, res, dout = (t.cuda() for t in gu.junction_case(n, H, W, C))
    x.requires_grad_(), res.requires_grad_()
    out = ops_resnet.cbam_junction(x, res, cb, False)
    dx, g = torch.autograd.grad(out, (x, res), dout)
    torch.cuda.synchronize()
    return out.detach(), dx, g, cb


@pytest.mark.parametrize("n,H,W,C", gu.JUNCTION_CASES)
def test_junction_data_backward_equals_the_full_one(n, H, W, C):
    out1, dx1, g1, _ = _junction(n, H, W, C, False)
    out0, dx0, g0, cb = _junction(n, H, W, C, True)
    assert torch.equal(out0, out1) and torch.equal(dx0, dx1) and torch.equal(g0, g1)
    assert dx1.abs().sum() > 0 and torch.isfinite(dx1).all()
    assert all(prm.grad is None for prm in cb.parameters())
    out_r, dx_r, g_r = gu.junction_oracle(n, H, W, C)
    for got, ref in ((dx1, dx_r), (g1, g_r)):
        assert float((got.cpu().double() - ref).abs().max()) <= gu.JUNCTION_BIG_TOL * float(ref.abs().max())


def test_junction_data_backward_beyond_the_cap():
    """96 x 96: the full backward refuses the map (its weight-gradient kernel holds a padded plane in LDS), the data-only one runs it"""
    from eoe_amd import _lib
    n, H, W, C = gu.JUNCTION_BIG
    with pytest.raises(_lib.EoeError, match="feature map too large"):
        _junction(n, H, W, C, True)
    out, dx, g, _ = _junction(n, H, W, C, False)
    out_r, dx_r, g_r = gu.junction_oracle(n, H, W, C)
    for name, got, ref in (("out", out, out_r), ("dx", dx, dx_r), ("g", g, g_r)):
        err = float((got.cpu().double() - ref).abs().max()) / float(ref.abs().max())
        print(f"junction 96x96x64 {name}: max err / max |ref| = {err:.3e}")
        assert err <= gu.JUNCTION_BIG_TOL, name


# ------------------------------------------------------------------------------------------------ the encoder
_models = {}


def eoe_wrn(res):
    """the package's WideResNet(res) with the oracle's deterministic state, on the device, in train mode (as a trainer holds it)"""
    from eoe_amd.models import WideResNet
    if res not in _models:
        m = WideResNet(res=res)
        m.load_state_dict(gu.oracle_wrn(res).state_dict())
        _models[res] = m
    return copy.deepcopy(_models[res]).cuda().train()


@pytest.mark.parametrize("res", gu.RESOLUTIONS)
@pytest.mark.parametrize("dtype", ["fp16", "bf16", "parity"])
def test_head_of_features_is_forward(res, dtype):
    import eoe_amd
    eoe_amd.set_compute_dtype("bf16" if dtype == "bf16" else "fp16")
    eoe_amd.set_parity_mode(dtype == "parity")
    m = eoe_wrn(res).eval()
    x = gu.images_of(res).cuda()
    with torch.no_grad():
        want = m(x)
        for k, layer in enumerate(gu.LAYERS, start=1):
            a = m.features(x, layer)
            assert a.shape == (gu.N_MODEL, res >> (k + 1), res >> (k + 1), 32 << k) and a.dtype == torch.float32
            assert torch.equal(m.head(a, layer), want) and torch.equal(m.head(m.features(x, k), k), want), layer
    # through a detached leaf with the tape on, as grad_cam runs it
    with torch.no_grad():
        a = m.features(x, "layer2")
    leaf = m.leaf_of(a)
    assert leaf.requires_grad and leaf.is_leaf and (dtype == "parity" or leaf._eoe16 is a._eoe16)
    assert torch.equal(m.head(leaf, "layer2").detach(), want)


@pytest.mark.parametrize("res", gu.RESOLUTIONS)
@pytest.mark.parametrize("dtype", ["parity", "fp16", "bf16"])
def test_grad_cam_against_the_oracle(res, dtype):
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype("bf16" if dtype == "bf16" else "fp16")
    eoe_amd.set_parity_mode(dtype == "parity")
    ops.set_grad_scale(256.0 if dtype == "fp16" else 1.0)
    key = "parity" if dtype == "parity" else (torch.float16 if dtype == "fp16" else torch.bfloat16)
    m = eoe_wrn(res)
    x = gu.images_of(res).cuda()
    worst, failed = 0.0, []
    for layer in gu.LAYERS:
        ref = gu.oracle_maps(res, layer)
        for mode in gu.MODES:
            got = explain.grad_cam(m, x, explain.score_fn("hsc"), layer=layer, mode=mode)
            assert got.shape == (gu.N_MODEL, res, res) and got.dtype == torch.float32
            err = gu.map_error(got.cpu().numpy(), ref[mode])
            print(f"grad_cam {dtype} res={res} {layer} {mode}: {err:.3e}   (recorded {gu.MEASURED[key].get((res, layer, mode))})")
            worst = max(worst, err)
            limit = gu.PARITY_CEILING if dtype == "parity" else gu.bar(key)
            if limit is None or not err <= limit:
                failed.append((layer, mode, err, limit))
    assert not failed, failed
    assert m.training and all(p.grad is None and p.requires_grad for p in m.parameters())


def test_saturated_score_keeps_finite_nonzero_maps():
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype("fp16")
    ops.set_grad_scale(256.0)
    m = eoe_wrn(32)
    x = gu.images_of(32).cuda()
    with torch.no_grad():
        m.eval()
        norm = m(x).norm(dim=1).min()
        m.train()
        m.fc.weight.mul_(24.0 / norm), m.fc.bias.mul_(24.0 / norm)
        m.eval()
        score = explain.score_fn("hsc")(m(x))
        m.train()
    assert bool((1 - score < 1e-6).all()), score
    for layer in ("layer1", "layer4"):
        for mode in gu.MODES:
            maps = explain.grad_cam(m, x, explain.score_fn("hsc"), layer=layer, mode=mode)
            assert torch.isfinite(maps).all() and bool((maps.flatten(1).amax(1) > 0).all()), (layer, mode)


@pytest.mark.parametrize("grads_set", [False, True])
def test_grad_cam_touches_nothing_else(grads_set):
    """a registered gradient arena, every .grad, every running buffer and num_batches_tracked keep their bytes; flags and requires_grad
    come back; two calls give the same bytes.  (With the full junction backward the arena views of the CBAM parameters were written.)"""
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype("fp16")
    ops.set_grad_scale(256.0)
    m = eoe_wrn(32)
    m.layer2[0].bn1.eval()
    m.fc.bias.requires_grad_(False)
    flags = {n: mod.training for n, mod in m.named_modules()}
    req = {n: p.requires_grad for n, p in m.named_parameters()}
    arena = {}
    for n, p in m.named_parameters():                                  # what parallel.GradArena registers: a view per parameter
        arena[n] = torch.full_like(p, 12345.0)
        p._eoe_grad_buf = arena[n]
        if grads_set:
            p.grad = torch.full_like(p, -7.0)
    before = {n: b.detach().clone() for n, b in m.named_buffers()}
    x = gu.images_of(32).cuda()
    a = explain.grad_cam(m, x, explain.score_fn("hsc"), layer="layer1")
    b = explain.grad_cam(m, x, explain.score_fn("hsc"), layer="layer1")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and a.abs().sum() > 0 and not x.requires_grad
    assert all(bool((t == 12345.0).all()) for t in arena.values())
    if grads_set:
        assert all(bool((p.grad == -7.0).all()) for p in m.parameters())
    else:
        assert all(p.grad is None for p in m.parameters())
    assert all(torch.equal(before[n], buf) for n, buf in m.named_buffers()) and int(m.bn1.num_batches_tracked) == 7
    assert {n: mod.training for n, mod in m.named_modules()} == flags and m.training
    assert {n: p.requires_grad for n, p in m.named_parameters()} == req and "forward" not in vars(m)


def test_training_is_untouched():
    """one HSC Adam step before and one after a grad_cam call: the losses and parameter bytes of the same two steps without the call"""
    import eoe_amd
    from eoe_amd import explain, ops
    from eoe_amd.optim import FusedAdam
    eoe_amd.set_compute_dtype("fp16")
    ops.set_grad_scale(256.0)
    x = gu.images_of(32).cuda()
    lbls = torch.tensor([0, 1, 1], device="cuda")

    def two_steps(with_call):
        m = eoe_wrn(32)
        opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.0, amsgrad=False)
        losses = []
        for i in range(2):
            opt.zero_grad()
            loss = eoe_amd.hsc_loss(m(x), lbls, 0)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
            if with_call and i == 0:
                assert explain.grad_cam(m, x, explain.score_fn("hsc"), layer="layer1").abs().sum() > 0
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}, {n: b.detach().clone() for n, b in m.named_buffers()}

    l0, p0, b0 = two_steps(False)
    l1, p1, b1 = two_steps(True)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    assert all(torch.equal(p0[n], p1[n]) for n in p0) and all(torch.equal(b0[n], b1[n]) for n in b0)


# ------------------------------------------------------------------------------------------------ trainer
def _task():
    from eoe_amd.data import LabelledImageSet
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 32), indexing="ij")

    def make(k, n):
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)
        return (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, 32, 32, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    cls = torch.tensor([0, 1] * 8)
    imgs = torch.stack([make(int(c), 1)[0] for c in cls])
    lset = LabelledImageSet(imgs, cls, imgs, cls, make(1, 16), ["a", "b"], 32, mean=(0.5,) * 3, std=(0.25,) * 3)
    return lset.source([0])


def test_trainer_keeps_and_logs_the_maps(tmp_path):
    import eoe_amd
    from eoe_amd import explain, ops
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    eoe_amd.set_compute_dtype("bf16")
    ds = _task()
    model = eoe_wrn(32).cpu()
    kw = dict(dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["a"])
    on = TRAINER["hsc"](model, logger=JsonLogger(str(tmp_path / "on")), extremes=2, cam=True, cam_layer="layer3", **kw)
    off = TRAINER["hsc"](model, logger=JsonLogger(str(tmp_path / "off")), extremes=2, **kw)
    res_on, res_off = on.eval_cls(copy.deepcopy(model), ds, 0, "a", 0), off.eval_cls(copy.deepcopy(model), ds, 0, "a", 0)
    key = "eval_cls0_it0"
    assert list(on.cams) == [key] and off.cams == {}
    maps = on.cams[key]
    rows, per, _ = on._extreme_rows(on.extremes[key])
    assert maps.shape == (len(rows), 32, 32) and len(rows) == 8 and maps.dtype == torch.float32 and torch.isfinite(maps).all() and maps.max() > 0
    # equal to a direct call on the same rows
    m = copy.deepcopy(model).cuda().eval()
    on._normalize_hook(m, ds)
    imgs, lbls, _ = ds.test_inputs(rows)
    prev = ops.grad_scale()
    ops.set_grad_scale(ops.default_grad_scale())
    direct = explain.grad_cam(m, on._test_time_inputs(imgs.cuda(), lbls, 0), explain.score_fn(on, None, 0), layer="layer3")
    ops.set_grad_scale(prev)
    assert torch.equal(direct, maps)
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off")}
    extra = sorted(set(files["on"]) - set(files["off"]))
    assert set(files["off"]) <= set(files["on"])
    assert extra and all(f.startswith("eval_cls0-a_it0_extremes_cam") for f in extra) and any(f.endswith(".png") for f in extra), files
    assert (res_on[0].auc, res_on[1].avg_prec) == (res_off[0].auc, res_off[1].avg_prec)

    class NoLoaders:
        nominal_label = 0

        def test_inputs(self, rows):
            raise AssertionError

        def loaders(self, *a, **k):
            raise AssertionError("no loader may be asked for")
    with pytest.raises(NotImplementedError, match="no WideResNet"):
        on.eval_cls(CNN32(), NoLoaders(), 0, "a", 0)
