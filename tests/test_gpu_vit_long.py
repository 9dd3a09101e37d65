"""GPU: image towers with more than 64 tokens (the attention kernels of csrc/attention_long.hip inside eoe_vit_block_fwd / _bwd) against the
CPU oracle of the same geometry and against the reference's own module (tests/golden/g27_vit_long.npz): 144 / 16 (82 tokens, width 256)
and ViT-B/16's own 224 / 16 (197 tokens, width 768).  The bars are test_gpu_model.test_vit_trajectory_vs_golden's: TRAJ_TOL (imported) on
the loss and the scores, FEATURES_RMS = 20 EPS16 on the rel rms of encoder features, 30 EPS16 + 1e-3 on every gradient norm."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DTYPES, EPS16, rel_rms                     # noqa: E402
from oracle import fill, models as omodels, objectives, trainer as otrainer   # noqa: E402
from test_gpu_model import TRAJ_TOL                              # noqa: E402

FEATURES_RMS = 20.0          # x EPS16: test_vit_trajectory_vs_golden's bar on the encoder output ("encoder-after rel rms")
SMALL = dict(input_resolution=144, patch_size=16, width=256, layers=2, output_dim=64)          # 82 tokens, 4 heads
B16 = dict(input_resolution=224, patch_size=16, width=768, layers=2, output_dim=512)           # 197 tokens, 12 heads


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
    """features, loss, scores and parameter gradients of one HSC step of the CPU oracle, computed once per (geometry, n, freeze)"""
    cache = {}

    def get(key, geo, n_half, freeze):
        k = (key, n_half, freeze)
        if k not in cache:
            m = omodels.ClipViTNet(freeze=freeze, layers=geo["layers"], width=geo["width"], heads=geo["width"] // 64, output_dim=geo["output_dim"],
                                   input_resolution=geo["input_resolution"], patch_size=geo["patch_size"])
            omodels.deterministic_init(m, tag="vitlong", width=geo["width"], layers=geo["layers"])
            m.freeze_parts()
            imgs, lbls = otrainer.synthetic_batch(f"vitlong/{key}", n_half, n_half + (1 if key == "small" else 0), geo["input_resolution"])
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
    omodels.deterministic_init(m, tag="vitlong", width=geo["width"], layers=geo["layers"])
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
        assert dev <= 30 * EPS16[dtype] + 1e-3, (n, dev, r)
    print(f"   worst grad-norm deviation {worst:.2e}")
    if freeze:
        assert all(n.startswith("final_linear") for n in grads)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("freeze,cls_only", [(False, False), (False, True), (True, True)])
def test_tower_of_82_tokens_against_the_oracle(oracle_step, dtype, freeze, cls_only):
    import eoe_amd
    from eoe_amd import ops
    eoe_amd.set_compute_dtype(dtype)
    ops.VIT_CLS_ONLY_LAST = cls_only
    ref = oracle_step("small", SMALL, 1, freeze)          # n = 3: one nominal, two outlier-exposure images
    assert ref["imgs"].shape[0] == 3
    check_step(ref, eoe_model(SMALL, freeze), dtype, freeze)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tower_of_vit_b16_against_the_oracle(oracle_step, dtype):
    import eoe_amd
    eoe_amd.set_compute_dtype(dtype)
    ref = oracle_step("b16", B16, 1, False)
    assert ref["imgs"].shape[0] == 2
    check_step(ref, eoe_model(B16), dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tower_of_82_tokens_against_the_reference_fixture(golden, dtype):
    """the reference's own VisualTransformer at (144, 16, 256, 2, 4, 64): output and per-tensor gradient norms"""
    import eoe_amd
    from eoe_amd.models import VisualTransformer
    eoe_amd.set_compute_dtype(dtype)
    g = golden("g27_vit_long")
    geo = tuple(int(v) for v in g["geometry"])
    m = omodels.deterministic_init(VisualTransformer(*geo), tag="g27", width=geo[2], layers=geo[3]).cuda().train()
    x = torch.from_numpy(fill.fill("g27/x", (2, 3, geo[0], geo[0]), std=1.0)).cuda()
    dy = torch.from_numpy(fill.fill("g27/dy", (2, geo[5]), std=1.0)).cuda()
    out = m(x)
    (out * dy).sum().backward()
    dev = rel_rms(out.detach(), torch.from_numpy(g["out"]))
    print(f"[{dtype}] output rel rms {dev:.2e}")
    assert dev < FEATURES_RMS * EPS16[dtype], dev
    for n, p in m.named_parameters():
        ref = float(g[f"gnorm/{n}"])
        d = abs(p.grad.double().norm().item() - ref) / max(ref, 1e-12)
        assert d <= 30 * EPS16[dtype] + 1e-3, (n, d, ref)


def test_reduced_vit_b16_state_dict_loads_strictly_and_encodes_like_the_oracle():
    import eoe_amd
    from eoe_amd.models.clip import CLIP, build_model
    eoe_amd.set_compute_dtype(torch.float16)
    # embed_dim 512; vision 224 / 16, width 768, two layers; a small text tower
    src = CLIP(512, 224, 2, 768, 16, 77, 1000, 128, 2, 1)
    omodels.deterministic_init(src.visual, tag="vitlong/clip", width=768, layers=2)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    model = build_model(sd).cuda()
    v = model.visual
    assert (v.input_resolution, v.patch_size, v.positional_embedding.shape[0], len(v.transformer.resblocks)) == (224, 16, 197, 2)
    oracle = omodels.deterministic_init(omodels.VisualTransformer(224, 16, 768, 2, 12, 512), tag="vitlong/clip", width=768, layers=2)
    x = torch.from_numpy(fill.fill("vitlong/clip/x", (2, 3, 224, 224), std=1.0))
    with torch.no_grad():
        got, ref = model.encode_image(x.cuda()).cpu(), oracle(x)
    dev = rel_rms(got, ref)
    assert torch.isfinite(got).all() and dev < FEATURES_RMS * EPS16[torch.float16], dev


def test_unsupported_geometries_are_refused_at_construction():
    from eoe_amd.models import VisualTransformer
    from eoe_amd import ops
    for args, word in (((224, 14, 1024, 2, 16, 768), "patch"), ((224, 16, 1280, 2, 20, 512), "width"), ((224, 16, 768, 2, 8, 512), "head"),
                       ((448, 16, 768, 2, 12, 512), str(ops.ATTN_LONG_MAX_L))):
        with pytest.raises(NotImplementedError, match=word):
            VisualTransformer(*args)
    VisualTransformer(384, 16, 768, 1, 12, 512)          # 577 tokens: ViT-B/16 at 384
