"""GPU: image towers whose width is a multiple of 64 but not of 256 -- ViT-Ti's 192 (3 heads), ViT-S's 384 (6 heads), one head at width 64
and five at 320 -- against the CPU oracle of the same geometry and against the reference's own module (tests/golden/g28_vit_narrow.npz).
The LayerNorm and embed kernels predicate the last 256-column group of a row there (csrc/elementwise.hip); the GEMMs see N = 192 / 576 /
1152 and the attention kernels 1, 3, 5 and 6 heads.  Geometries: tests/vit_narrow_util.py.  The bars are tests/test_gpu_vit_long.py's:
TRAJ_TOL on the loss and the scores, FEATURES_RMS = 20 EPS16 on the rel rms of encoder features, 30 EPS16 + 1e-3 on every gradient norm."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_narrow_util as nu                                     # noqa: E402
from gpu_util import DTYPES, EPS16, rel_rms                      # noqa: E402
from oracle import fill, models as omodels, objectives, trainer as otrainer   # noqa: E402
from test_gpu_model import TRAJ_TOL                              # noqa: E402

FEATURES_RMS = 20.0          # x EPS16: test_vit_trajectory_vs_golden's bar on the encoder output ("encoder-after rel rms")


@pytest.fixture(autouse=True)
def _restore():
    import eoe_amd
    from eoe_amd import ops
    old, old_cls = eoe_amd.compute_dtype(), ops.VIT_CLS_ONLY_LAST
    yield
    eoe_amd.set_compute_dtype(old)
    ops.VIT_CLS_ONLY_LAST = old_cls


@pytest.fixture(scope="module")
def oracle_step():
    """features, loss, scores and parameter gradients of one HSC step of the CPU oracle, computed once per (geometry, freeze); n = 3: one
    nominal, two outlier-exposure images"""
    cache = {}

    def get(key, freeze):
        k = (key, freeze)
        if k not in cache:
            geo = nu.TOWERS[key]
            m = omodels.ClipViTNet(freeze=freeze, layers=geo["layers"], width=geo["width"], heads=geo["width"] // 64, output_dim=geo["output_dim"],
                                   input_resolution=geo["input_resolution"], patch_size=geo["patch_size"])
            omodels.deterministic_init(m, tag="vitnarrow", width=geo["width"], layers=geo["layers"])
            m.freeze_parts()
            imgs, lbls = otrainer.synthetic_batch(f"vitnarrow/{key}", 1, 2, geo["input_resolution"])
            feats = m(imgs)
            loss = objectives.hsc_loss(feats, lbls, 0)
            loss.backward()
            cache[k] = dict(imgs=imgs, lbls=lbls, feats=feats.detach(), loss=loss.item(), scores=objectives.hsc_score(feats.detach()).numpy(),
                            gnorm={n: p.grad.double().norm().item() for n, p in m.named_parameters() if p.grad is not None})
        return cache[k]
    return get


def eoe_model(geo, freeze=False):
    from eoe_amd.models import ClipViTB32Custom
    m = ClipViTB32Custom(freeze=freeze, layers=geo["layers"], input_resolution=geo["input_resolution"], patch_size=geo["patch_size"],
                         width=geo["width"], output_dim=geo["output_dim"])
    omodels.deterministic_init(m, tag="vitnarrow", width=geo["width"], layers=geo["layers"])
    m = m.cuda().train()
    if freeze:
        m.freeze_parts()
    return m


def check_step(ref, m, dtype, freeze):
    import eoe_amd
    feats = m(ref["imgs"].cuda())
    loss = eoe_amd.hsc_loss(feats, ref["lbls"].cuda(), 0)
    loss.backward()
    tol = TRAJ_TOL[dtype]
    rf = rel_rms(feats.detach(), ref["feats"])
    dl = abs(loss.item() - ref["loss"]) / max(1.0, abs(ref["loss"]))
    ds = np.abs(eoe_amd.hsc_score(feats.detach()).cpu().numpy() - ref["scores"]).max()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    print(f"[{dtype} frozen={freeze}] features rel rms {rf:.2e}; loss dev {dl:.2e}; score dev {ds:.2e}")
    assert torch.isfinite(feats).all() and rf < FEATURES_RMS * EPS16[dtype], rf
    assert dl <= tol and ds <= tol, (dl, ds)
    assert set(grads) == set(ref["gnorm"]), set(grads) ^ set(ref["gnorm"])
    worst = 0.0
    for n, g in grads.items():
        r = ref["gnorm"][n]
        dev = abs(g.double().norm().item() - r) / max(r, 1e-12)
        worst = max(worst, dev)
        print(f"   {n}: grad-norm deviation {dev:.2e}")
        assert dev <= 30 * EPS16[dtype] + 1e-3, (n, dev, r)
    print(f"   worst grad-norm deviation {worst:.2e}")
    if freeze:
        assert all(n.startswith("final_linear") for n in grads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("freeze,cls_only", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("key", list(nu.TOWERS))
def test_narrow_tower_against_the_oracle(oracle_step, key, freeze, cls_only, dtype):
    """one HSC step at (64, 16, 192): short attention, 3 heads; (144, 16, 384): long attention, 6 heads; (32, 16, 64): one head, rows of
    the tail group alone; (32, 16, 320): one full group + 16 lanes"""
    import eoe_amd
    from eoe_amd import ops
    eoe_amd.set_compute_dtype(dtype)
    ops.VIT_CLS_ONLY_LAST = cls_only
    ref = oracle_step(key, freeze)
    assert ref["imgs"].shape[0] == 3
    check_step(ref, eoe_model(nu.TOWERS[key], freeze), dtype, freeze)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vit_ti_width_against_the_reference_fixture(golden, dtype):
    """the reference's own VisualTransformer at (64, 16, 192, 2, 3, 64): output and per-tensor gradient norms"""
    import eoe_amd
    from eoe_amd.models import VisualTransformer
    eoe_amd.set_compute_dtype(dtype)
    g = golden("g28_vit_narrow")
    geo = tuple(int(v) for v in g["geometry"])
    assert geo == nu.G28_GEOMETRY
    m = omodels.deterministic_init(VisualTransformer(*geo), tag="g28", width=geo[2], layers=geo[3]).cuda().train()
    x = torch.from_numpy(fill.fill("g28/x", (2, 3, geo[0], geo[0]), std=1.0)).cuda()
    dy = torch.from_numpy(fill.fill("g28/dy", (2, geo[5]), std=1.0)).cuda()
    out = m(x)
    (out * dy).sum().backward()
    dev = rel_rms(out.detach(), torch.from_numpy(g["out"]))
    print(f"[{dtype}] output rel rms {dev:.2e}")
    assert dev < FEATURES_RMS * EPS16[dtype], dev
    for n, p in m.named_parameters():
        ref = float(g[f"gnorm/{n}"])
        d = abs(p.grad.double().norm().item() - ref) / max(ref, 1e-12)
        print(f"   {n}: grad-norm deviation {d:.2e}")
        assert d <= 30 * EPS16[dtype] + 1e-3, (n, d, ref)


def test_vit_ti_clip_state_dict_loads_strictly_and_encodes_like_the_oracle():
    import eoe_amd
    from eoe_amd.models.clip import CLIP, build_model
    eoe_amd.set_compute_dtype(torch.float16)
    # embed_dim 64; vision 64 / 16, width 192, two layers; a small text tower
    src = CLIP(64, 64, 2, 192, 16, 77, 1000, 128, 2, 1)
    omodels.deterministic_init(src.visual, tag="vitnarrow/clip", width=192, layers=2)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    model = build_model(sd).cuda()
    v = model.visual
    assert (v.input_resolution, v.patch_size, v.positional_embedding.shape[0], len(v.transformer.resblocks)) == (64, 16, 17, 2)
    assert v.conv1.weight.shape[0] == 192 and v.transformer.resblocks[0].n_head == 3
    oracle = omodels.deterministic_init(omodels.VisualTransformer(64, 16, 192, 2, 3, 64), tag="vitnarrow/clip", width=192, layers=2)
    x = torch.from_numpy(fill.fill("vitnarrow/clip/x", (2, 3, 64, 64), std=1.0))
    with torch.no_grad():
        got, ref = model.encode_image(x.cuda()).cpu(), oracle(x)
    dev = rel_rms(got, ref)
    assert torch.isfinite(got).all() and dev < FEATURES_RMS * EPS16[torch.float16], dev


def test_hsc_trainer_runs_a_vit_ti_tower_on_a_resident_32px_set():
    """the training loop end to end at width 192: two epochs over a small resident image set at 32 x 32 / patch 8 (17 tokens)"""
    import copy
    import eoe_amd
    from eoe_amd.data import ResidentImageSource
    from eoe_amd.models import ClipViTB32Custom
    from eoe_amd.training import TRAINER
    eoe_amd.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 32), indexing="ij")

    def make(k, n):                        # a class-dependent low-frequency pattern + noise, uint8 [n, 32, 32, 3]
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)
        return (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, 32, 32, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    test_y = torch.tensor([0, 1] * 8)
    test = torch.stack([make(int(y), 1)[0] for y in test_y])
    ds = ResidentImageSource(make(0, 32), make(1, 32), test, test_y, crop=32, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), seed=3)
    torch.manual_seed(0)
    m0 = ClipViTB32Custom(width=192, layers=1, input_resolution=32, patch_size=8, output_dim=64)
    tr = TRAINER["hsc"](m0, dataset=ds, epochs=2, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"])
    model, roc = tr.train_cls(copy.deepcopy(m0), ds, 0, "only", 0)
    assert len(tr.last_losses) == 2 * 2 and all(np.isfinite(tr.last_losses)), tr.last_losses
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert roc is not None and 0.0 <= roc.auc <= 1.0
