"""GPU: explaining an anomaly score (csrc/explain.hip, eoe_amd/explain.py).  The last hop of the ViT input gradient against
torch.nn.functional.fold, the tower's input gradient against autograd through the fp64 oracle at the four geometries of
tests/vit_narrow_util.py, its side effects, the saliency and overlay kernels against their numpy statements, and the trainer option.
Case tables and the measured distances: tests/explain_util.py."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import explain_util as xu                                         # noqa: E402
import vit_narrow_util as nu                                      # noqa: E402
from gpu_util import DTYPES, EPS16, assert_close                  # noqa: E402
from oracle import models as omodels, objectives, trainer as otrainer   # noqa: E402


@pytest.fixture(autouse=True)
def _restore():
    import eoe_amd
    from eoe_amd import ops
    old, old_cls, old_scale = eoe_amd.compute_dtype(), ops.VIT_CLS_ONLY_LAST, ops.grad_scale()
    yield
    eoe_amd.set_compute_dtype(old)
    ops.VIT_CLS_ONLY_LAST = old_cls
    ops.set_grad_scale(old_scale)


def guarded(shape, dtype=torch.float32):
    """an output tensor with xu.GUARD elements of NaN (0xFF bytes) behind it: (the view to write, the guard)"""
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        buf = torch.full((n + xu.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    else:
        buf = torch.full((n + xu.GUARD,), float("nan"), dtype=dtype, device="cuda")
    return buf[:n].view(shape), buf[n:]


def guard_intact(guard):
    return bool((guard == 0xA5).all()) if guard.dtype == torch.uint8 else bool(torch.isnan(guard).all())


# ------------------------------------------------------------------------------------------------ the last hop
def unpatchify(dp, std, scale_inv, n, res, patch):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    dx, guard = guarded((n, 3, res, res))
    check(lib.eoe_unpatchify_grad(dp.data_ptr(), ops._p(std), scale_inv, dx.data_ptr(), n, res, patch, ops._stream()),
          "eoe_unpatchify_grad")
    torch.cuda.synchronize()
    assert guard_intact(guard)
    return dx.cpu()


@pytest.mark.parametrize("res,patch,n", xu.UNPATCHIFY_CASES)
def test_unpatchify_grad_is_fold_times_scale_over_std(res, patch, n):
    dp = xu.dpatches_case(res, patch, n)
    ref = xu.fold_reference(dp, res, patch, n)
    dpd = torch.from_numpy(dp).cuda()
    # no Normalize, a power-of-two scale: the rearranged values, bit for bit
    for scale_inv in (1.0, 1.0 / 256.0):
        assert torch.equal(unpatchify(dpd, None, scale_inv, n, res, patch), ref * scale_inv)
    std = torch.tensor(xu.UNPATCHIFY_STD)
    for scale_inv in (1.0, 1.0 / 256.0, 0.3):
        got = unpatchify(dpd, std.cuda(), scale_inv, n, res, patch)
        assert_close(got, ref.double() * scale_inv / std.double().view(1, 3, 1, 1), rtol=1e-6, atol=0.0, what=f"unpatchify {res}/{patch} x{scale_inv}")


def test_embed_backward_with_an_image_gradient_leaves_the_other_gradients_bit_equal():
    from eoe_amd import ops
    import eoe_amd
    eoe_amd.set_compute_dtype(torch.float16)
    n, res, patch, D = 3, 48, 16, 192
    L = (res // patch) ** 2 + 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn((n, 3, res, res), generator=g).cuda()
    params = [torch.randn(s, generator=g).mul_(0.1).cuda().requires_grad_() for s in ((D, 3, patch, patch), (D,), (L, D), (D,), (D,))]
    dy = torch.randn((n * L, D), generator=g).cuda()
    mean, std = torch.tensor(xu.NORM_MEAN).cuda(), torch.tensor(xu.NORM_STD).cuda()
    outs = []
    for need in (False, True):
        xin = x.clone().requires_grad_(need)
        y = ops.VitEmbedFunction.apply(xin, *params, patch, mean, std)
        grads = torch.autograd.grad(y, ([xin] if need else []) + params, dy)
        outs.append([t.clone() for t in grads])
    without, with_x = outs
    assert with_x[0].shape == x.shape and torch.isfinite(with_x[0]).all() and with_x[0].abs().sum() > 0
    for a, b in zip(without, with_x[1:]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the tower's input gradient
def eoe_tower(key, norm):
    from eoe_amd.models import ClipViTB32Custom
    geo = nu.TOWERS[key]
    m = ClipViTB32Custom(layers=geo["layers"], input_resolution=geo["input_resolution"], patch_size=geo["patch_size"], width=geo["width"],
                         output_dim=geo["output_dim"])
    omodels.deterministic_init(m, tag="explain", width=geo["width"], layers=geo["layers"])
    m = m.cuda().train()
    if norm:
        m.feature_model.set_normalize(xu.NORM_MEAN, xu.NORM_STD)
    return m


def tower_batch(key):
    return otrainer.synthetic_batch(f"explain/{key}", 1, 2, nu.TOWERS[key]["input_resolution"])


@pytest.fixture(scope="module")
def oracle_grad():
    """d hsc_score / d image through oracle.models.ClipViTNet in fp64, once per (geometry, Normalize)"""
    cache = {}

    def get(key, norm):
        if (key, norm) not in cache:
            geo = nu.TOWERS[key]
            m = omodels.ClipViTNet(layers=geo["layers"], width=geo["width"], heads=geo["width"] // 64, output_dim=geo["output_dim"],
                                   input_resolution=geo["input_resolution"], patch_size=geo["patch_size"])
            omodels.deterministic_init(m, tag="explain", width=geo["width"], layers=geo["layers"])
            m = m.double().eval()
            x = tower_batch(key)[0].double().requires_grad_()
            inp = x
            if norm:
                inp = (x - torch.tensor(xu.NORM_MEAN).double().view(1, 3, 1, 1)) / torch.tensor(xu.NORM_STD).double().view(1, 3, 1, 1)
            (g,) = torch.autograd.grad(objectives.hsc_score(m(inp)).sum(), x)
            cache[(key, norm)] = g
        return cache[(key, norm)]
    return get


def input_grad_distance(ref, key, dtype, cls_only, norm, scale):
    """the worst image's relative rms distance of input_gradient to `ref`"""
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype(dtype)
    ops.VIT_CLS_ONLY_LAST = cls_only
    ops.set_grad_scale(scale)
    got = explain.input_gradient(eoe_tower(key, norm), tower_batch(key)[0].cuda(), explain.score_fn("hsc"))
    assert got.shape == ref.shape and got.dtype == torch.float32 and torch.isfinite(got).all()
    d = (got.cpu().double() - ref).flatten(1)
    return float((d.pow(2).mean(1).sqrt() / ref.flatten(1).pow(2).mean(1).sqrt()).max())


CASES = [(dt, 1.0) for dt in DTYPES] + [(torch.float16, 256.0)]


@pytest.mark.parametrize("dtype,scale", CASES)
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("key", list(nu.TOWERS))
def test_input_gradient_against_autograd_through_the_fp64_oracle(oracle_grad, key, cls_only, norm, dtype, scale):
    """per-image relative rms distance to the fp64 gradient; fp16 with the gradient scale at 1 and at 256 meets the same bar, so the
    scale is undone exactly.  Bars and the measured table: explain_util.INPUT_GRAD_BAR / INPUT_GRAD_MEASURED"""
    dist = input_grad_distance(oracle_grad(key, norm), key, dtype, cls_only, norm, scale)
    print(f"[{key} {dtype} cls_only={cls_only} norm={norm} scale={scale:g}] input-gradient rel rms {dist:.3e} = {dist / EPS16[dtype]:.2f} EPS16")
    assert dist <= xu.INPUT_GRAD_BAR[dtype] * EPS16[dtype], dist


def test_input_gradient_leaves_no_trace():
    """no parameter gets a .grad, the train / eval flags come back, two calls give the same bytes, and a training step behind the call has
    the bits of one without it"""
    import eoe_amd
    from eoe_amd import explain, ops
    eoe_amd.set_compute_dtype(torch.float16)
    ops.set_grad_scale(256.0)
    imgs, lbls = tower_batch("ti_short")
    imgs, lbls = imgs.cuda(), lbls.cuda()

    def step(m):
        loss = eoe_amd.hsc_loss(m(imgs), lbls, 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    loss0, grads0 = step(eoe_tower("ti_short", True))
    m = eoe_tower("ti_short", True)
    m.feature_model.ln_post.eval()                                     # a mixed set of flags must come back as it was
    flags = {n: mod.training for n, mod in m.named_modules()}
    a = explain.input_gradient(m, imgs, explain.score_fn("hsc"))
    b = explain.input_gradient(m, imgs, explain.score_fn("hsc"))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not imgs.requires_grad
    assert all(p.grad is None for p in m.parameters())
    assert {n: mod.training for n, mod in m.named_modules()} == flags and m.training
    loss1, grads1 = step(m)
    assert torch.equal(loss0, loss1) and set(grads0) == set(grads1)
    for n in grads0:
        assert torch.equal(grads0[n], grads1[n]), n


# ------------------------------------------------------------------------------------------------ saliency
@pytest.mark.parametrize("mode", ["max", "l2", "gradxinput"])
@pytest.mark.parametrize("n,C,H,W,pool", xu.SALIENCY_CASES + ((3, 3, 28, 28, None), (2, 1, 5, 7, None)))
def test_saliency_map_against_its_numpy_statement(n, C, H, W, pool, mode):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    from eoe_amd.explain import MODES, saliency, saliency_np
    g, x = xu.saliency_case(n, C, H, W)
    ref = torch.from_numpy(saliency_np(g, x, mode, pool))
    gd, xd = torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda()
    s, guard = guarded((n, H, W))
    for _ in range(2):
        check(lib.eoe_saliency_map(gd.data_ptr(), xd.data_ptr() if mode == "gradxinput" else None, s.data_ptr(), n, C, H, W, MODES[mode],
                                   pool or 0, ops._stream()), "eoe_saliency_map")
    torch.cuda.synchronize()
    assert guard_intact(guard)
    got = s.cpu()
    assert torch.equal(got, saliency(gd, xd, mode, pool).cpu())           # the wrapper, and the same bytes on every run
    if pool is None and (mode == "max" or (mode == "gradxinput" and C == 1)):
        assert torch.equal(got, ref)
    else:
        assert_close(got, ref, rtol=xu.SALIENCY_RTOL, atol=0.0, what=f"saliency {mode} {(n, C, H, W, pool)}")
    if pool:
        blocks = got.reshape(n, H // pool, pool, W // pool, pool)
        assert torch.equal(blocks, blocks[:, :, :1, :, :1].expand_as(blocks))     # every block carries ONE value


def test_saliency_smooth_is_the_blur_of_the_multi_scale_modes():
    from eoe_amd.explain import saliency
    from eoe_amd.msm import blur_np
    g, _ = xu.saliency_case(3, 3, 28, 28)
    got = saliency(torch.from_numpy(g).cuda(), mode="max", smooth=2.0).cpu()
    ref = blur_np(np.abs(g).max(1)[:, None], 2.0)[:, 0]
    assert_close(got, torch.from_numpy(ref), rtol=1e-5, atol=1e-6, what="smoothed saliency")


# ------------------------------------------------------------------------------------------------ overlay
@pytest.mark.parametrize("alpha", xu.OVERLAY_ALPHAS)
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", xu.OVERLAY_SIZES)
def test_heat_overlay_against_its_numpy_statement(H, W, C, u8, alpha):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    from eoe_amd.explain import overlay, overlay_np
    maps, pics = xu.overlay_case(H, W, C, u8)
    ref = overlay_np(maps, pics, alpha)
    md, pd = torch.from_numpy(maps).cuda(), torch.from_numpy(pics).cuda()
    out, guard = guarded((4, H, W, 3), torch.uint8)
    check(lib.eoe_heat_overlay_u8(md.data_ptr(), pd.data_ptr(), 1 if u8 else 0, out.data_ptr(), 4, C, H, W, alpha, ops._stream()),
          "eoe_heat_overlay_u8")
    torch.cuda.synchronize()
    assert guard_intact(guard)
    got = out.cpu().numpy()
    assert np.array_equal(got, overlay(md, pd, alpha).cpu().numpy())
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    share = float((diff != 0).mean())
    print(f"[{H}x{W} C={C} u8={u8} alpha={alpha}] bytes that differ: {share:.2e}, max {diff.max()}")
    assert diff.max() <= 1 and share <= xu.OVERLAY_MAX_DIFF_SHARE
    t = xu.heat_levels(maps)[..., None]
    assert (diff[np.broadcast_to((t == 0) | (t == 1), diff.shape)] == 0).all()
    base = pics if u8 else np.floor(pics.transpose(0, 2, 3, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(got[2], np.repeat(base[2], 3, 2) if C == 1 else base[2])            # the constant map: the picture unchanged


# ------------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def small_task():
    """the resident 32-px set and ViT-Ti tower of test_hsc_trainer_runs_a_vit_ti_tower_on_a_resident_32px_set, trained for one epoch"""
    import eoe_amd
    from eoe_amd.data import ResidentImageSource
    from eoe_amd.models import ClipViTB32Custom
    from eoe_amd.training import TRAINER
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 32), indexing="ij")

    def make(k, n):
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)
        return (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, 32, 32, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    test_y = torch.tensor([0, 1] * 8)
    test = torch.stack([make(int(y), 1)[0] for y in test_y])
    ds = ResidentImageSource(make(0, 32), make(1, 32), test, test_y, crop=32, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), seed=3)
    torch.manual_seed(0)
    m0 = ClipViTB32Custom(width=192, layers=1, input_resolution=32, patch_size=8, output_dim=64)
    tr = TRAINER["hsc"](m0, dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"])
    model, _ = tr.train_cls(copy.deepcopy(m0), ds, 0, "only", 0)
    eoe_amd.set_compute_dtype(old)
    return ds, m0, model


def test_test_inputs_are_the_loaders_batches_bit_for_bit(small_task):
    ds = small_task[0]
    _, loader = ds.loaders(5)
    for imgs, lbls, idx in loader:
        got = ds.test_inputs(idx)
        assert torch.equal(got[0], imgs) and torch.equal(got[1], lbls) and torch.equal(got[2], idx)
    whole = torch.cat([b[0] for b in loader])
    rows = [9, 2, 15, 2]
    got = ds.test_inputs(rows)
    assert torch.equal(got[0], whole[rows]) and torch.equal(got[1], ds.test_y[rows])


def test_test_pictures_are_the_test_images_without_the_normalize(small_task):
    ds = small_task[0]
    rows = [9, 2, 15, 2]
    assert ds.mean is not None                                          # this source carries Normalize in its batches
    pics, imgs = ds.test_pictures(rows), ds.test_images(rows)
    want = ds.test[rows].permute(0, 3, 1, 2).float().cpu() / 255.0     # crop = the whole 32 x 32 image
    assert pics.shape == imgs.shape and float(pics.min()) >= 0.0 and float(pics.max()) <= 1.0
    assert (pics.cpu() - want).abs().max().item() <= 1e-6
    assert float(imgs.min()) < -0.5 and torch.equal(ds.test_images(rows), imgs)          # test_images still normalised afterwards


def test_trainer_explains_its_extremes_and_changes_nothing_when_off(small_task, tmp_path):
    """`explain=True` against `explain=False` on this commit: the option adds its own files and changes no other (that `extremes` itself
    changes nothing is held by the existing extremes tests); the maps against a recomputation by hand; the logged heat picture against
    image_grid(overlay(maps, the pictures in the [0, 1] scale)) for a source that carries mean / std in its batches"""
    import eoe_amd
    from eoe_amd import explain, ops
    from eoe_amd.imgrid import image_grid
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger

    class Keeping(JsonLogger):
        def logimg(self, name, *a, **k):
            self.pictures = getattr(self, "pictures", {})
            self.pictures[name] = super().logimg(name, *a, **k)
            return self.pictures[name]
    eoe_amd.set_compute_dtype("bf16")
    ds, m0, model = small_task
    kw = dict(dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"], extremes=3)
    on = TRAINER["hsc"](m0, logger=Keeping(str(tmp_path / "on")), explain=True, **kw)
    off = TRAINER["hsc"](m0, logger=JsonLogger(str(tmp_path / "off")), **kw)
    on.eval_cls(model, ds, 0, "only", 0)
    off.eval_cls(model, ds, 0, "only", 0)
    key = "eval_cls0_it0"
    assert list(on.explanations) == [key] and off.explanations == {}
    assert on.extremes[key].as_dict() == off.extremes[key].as_dict()
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off")}
    extra = sorted(set(files["on"]) - set(files["off"]))
    assert set(files["off"]) <= set(files["on"]) and extra and all(f.startswith("eval_cls0-only_it0_extremes_heat") for f in extra), files
    for f in files["off"]:
        if os.path.isfile(tmp_path / "off" / f):
            assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "on" / f).read_bytes(), f
    # the maps, recomputed by hand for the same rows
    ex = on.extremes[key]
    lists = [r for r in (ex.most[0][0], ex.least[0][0], ex.most[1][0], ex.least[1][0]) if len(r)]
    per = min(len(r) for r in lists)
    rows = np.concatenate([r[:per] for r in lists])
    maps = on.explanations[key]
    assert maps.shape == (len(rows), 32, 32) and maps.dtype == torch.float32 and torch.isfinite(maps).all() and maps.max() > 0
    # the logged picture: the heat over the pictures in ToTensor's scale, not over the normalised loader output
    pics = ds.test[torch.as_tensor(rows)].permute(0, 3, 1, 2).float() / 255.0
    assert float(ds.test_images(rows).min()) < 0.0
    heat = explain.overlay(maps, pics.to(maps.device), on.EXPLAIN_ALPHA)
    want = image_grid(heat, None, nrow=per, pad=2, maxres=128).cpu().numpy()
    got = on.logger.pictures["eval_cls0-only_it0_extremes_heat"]
    assert got.shape == want.shape and got.std() > 10
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert (diff != 0).mean() <= xu.OVERLAY_MAX_DIFF_SHARE, (diff.max(), (diff != 0).mean())
    model = model.cuda()
    ops.set_grad_scale(ops.default_grad_scale())
    grad = explain.input_gradient(model, ds.test_inputs(rows)[0], explain.score_fn("hsc"))
    assert torch.equal(explain.saliency(grad, mode="max", pool=8), maps)
    assert all(p.grad is None for p in model.parameters())
    model.cpu()


def test_trainer_explain_refuses_a_source_without_test_inputs_before_scoring(small_task):
    from eoe_amd.data import ListSource
    from eoe_amd.training import TRAINER
    ds, m0, model = small_task
    batches = [(torch.zeros(2, 3, 32, 32), torch.tensor([0, 1]))]

    class Counting(ListSource):
        asked = 0

        def loaders(self, *a, **k):
            Counting.asked += 1
            return super().loaders(*a, **k)
    tr = TRAINER["hsc"](m0, dataset=Counting(batches, batches), classes=["only"], extremes=2, explain=True)
    with pytest.raises(NotImplementedError, match="test_inputs"):
        tr.eval_cls(model, tr.ds, 0, "only", 0)
    assert Counting.asked == 0
