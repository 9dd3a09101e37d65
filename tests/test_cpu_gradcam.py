"""Grad-CAM without a GPU: the numpy statements against torch in float64, the refusals and their order (a refusal that came behind a
launch would fail here as "no GPU"), and the trainer's option checks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gradcam_util as gu


def test_cam_np_against_einsum():
    from eoe_amd.explain import cam_np
    for (n, h, w, C) in gu.MAP_CASES:
        A, dA = gu.act_case(n, h, w, C)
        a, d = torch.from_numpy(A).double(), torch.from_numpy(dA).double()
        want = {"gradcam": torch.relu(torch.einsum("nhwc,nc->nhw", a, d.mean(dim=(1, 2)))), "hirescam": torch.relu((a * d).sum(dim=3))}
        for mode in gu.MODES:
            got = cam_np(A, dA, mode)
            assert got.dtype == np.float32 and got.shape == (n, h, w)
            # cam_np rounds alpha to fp32 as the kernel stores it: within the bound the kernel itself is held to
            assert (np.abs(got.astype(np.float64) - want[mode].numpy()) <= gu.cam_bound(A, dA, mode) + 1e-30).all(), (n, h, w, C, mode)
            if n > 1:
                assert (got[0] == 0).all() and got[1].min() > 0          # the image built negative everywhere is clipped to exact zeros
    with pytest.raises(ValueError, match="mode"):
        cam_np(A, dA, "nope")


def test_cam_np_keeps_a_nan_and_zero_gradient_gives_zero():
    from eoe_amd.explain import cam_np
    A, dA = gu.act_case(1, 3, 5, 64)
    for mode in gu.MODES:
        assert (cam_np(A, np.zeros_like(dA), mode) == 0).all()
    A[0, 1, 2, 7] = np.nan
    assert np.isnan(cam_np(A, dA, "hirescam")[0, 1, 2]) and np.isnan(cam_np(A, dA, "gradcam")[0, 1, 2])
    assert np.isfinite(cam_np(A, dA, "hirescam")[0, 0, 0])


def test_bilinear_np_against_interpolate():
    from eoe_amd.explain import bilinear_np, grad_cam_np
    for (h, w), (H, W) in gu.UPSAMPLE_CASES:
        m = np.abs(gu.act_case(3, h, w, 4, "up")[0][..., 0]).astype(np.float64)
        want = F.interpolate(torch.from_numpy(m)[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0].numpy()
        got = bilinear_np(m, H, W)
        assert got.dtype == np.float32 and got.shape == (3, H, W)
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23 * np.abs(m).max(), ((h, w), (H, W))
        if (h, w) == (H, W):
            assert np.array_equal(got, m.astype(np.float32))
        if (h, w) == (1, 1):
            assert (got == got[:, :1, :1]).all()
    with pytest.raises(ValueError, match="smaller"):
        bilinear_np(np.zeros((1, 4, 4)), 3, 4)
    A, dA = gu.act_case(3, 7, 7, 64)
    a, d = torch.from_numpy(A).double(), torch.from_numpy(dA).double()
    want = F.interpolate(torch.relu((a * d).sum(dim=3))[:, None], size=(30, 30), mode="bilinear", align_corners=False)[:, 0].numpy()
    assert np.abs(grad_cam_np(A, dA, "hirescam", 30, 30) - want).max() <= 2.0 ** -23 * want.max()


def test_cpu_tensors_go_through_the_numpy_statements():
    from eoe_amd import explain
    A, dA = gu.act_case(3, 7, 7, 64)
    m = explain.cam_map(torch.from_numpy(A), torch.from_numpy(dA), "gradcam")
    assert np.array_equal(m.numpy(), explain.cam_np(A, dA, "gradcam"))
    up = explain.cam_upsample(m, 30, 30)
    assert np.array_equal(up.numpy(), explain.bilinear_np(m.numpy(), 30, 30))
    assert explain.overlay(up, torch.zeros((3, 3, 30, 30))).shape == (3, 30, 30, 3)          # a form overlay takes


def test_refusals_and_their_order():
    from eoe_amd import explain, ops_resnet
    from eoe_amd.models import CNN32, WideResNet
    from eoe_amd.models.custom import WideResNetCustom
    sf = explain.score_fn("hsc")
    x = torch.zeros((2, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="no WideResNet"):
        explain.grad_cam(CNN32(), x, sf)
    with pytest.raises(NotImplementedError, match="no WideResNet"):
        explain.grad_cam(torch.nn.Linear(4, 4), x, sf)
    wrn = WideResNet(res=32)
    for kw in (dict(layer="layer5"), dict(layer=4), dict(mode="cam")):
        with pytest.raises(ValueError, match="is none of"):
            explain.grad_cam(wrn, x, sf, **kw)
    with pytest.raises(ValueError, match="smaller"):
        explain.grad_cam(wrn, x, sf, layer="layer1", size=(4, 4))
    # a model found, the layer and the mode known: the CPU images are refused as the model refuses them, and everything comes back
    wrn.layer2[0].bn1.eval()
    wrn.fc.bias.requires_grad_(False)
    flags = {n: m.training for n, m in wrn.named_modules()}
    req = {n: p.requires_grad for n, p in wrn.named_parameters()}
    for layer in gu.LAYERS:
        with pytest.raises(RuntimeError, match="runs on the GPU only"):
            explain.grad_cam(wrn, x, sf, layer=layer)
    assert {n: m.training for n, m in wrn.named_modules()} == flags and wrn.training
    assert {n: p.requires_grad for n, p in wrn.named_parameters()} == req
    assert "forward" not in vars(wrn)                                 # the cut forward is gone again
    wrapped = WideResNetCustom()                                      # the tower inside a wrapper: found, cut, and put back
    with pytest.raises(RuntimeError, match="GPU only"):
        explain.grad_cam(wrapped, torch.zeros((1, 3, 224, 224)), sf)
    assert "forward" not in vars(wrapped.feature_model) and wrapped.training
    # the unfused CBAM forms have no data-only backward: refused below layer4, served at layer4 (here: as far as the CPU refusal)
    was = ops_resnet.FUSE_CBAM
    try:
        ops_resnet.FUSE_CBAM = False
        with pytest.raises(NotImplementedError, match="data-only"):
            explain.grad_cam(wrn, x, sf, layer="layer3")
        with pytest.raises(RuntimeError, match="runs on the GPU only"):
            explain.grad_cam(wrn, x, sf, layer="layer4")
    finally:
        ops_resnet.FUSE_CBAM = was
    wrn.layer4[1].cbam.no_spatial = True
    with pytest.raises(NotImplementedError, match="data-only"):
        explain.grad_cam(wrn, x, sf, layer="layer3")


def test_features_and_head_refuse_like_forward():
    from eoe_amd.models import WideResNet
    wrn = WideResNet(res=32)
    with pytest.raises(ValueError, match="is none of"):
        wrn.features(torch.zeros((1, 3, 32, 32)), "layer0")
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        wrn.features(torch.zeros((1, 3, 32, 32)), "layer2")
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        wrn.head(torch.zeros((1, 4, 4, 128)), 2)


def test_trainer_options():
    from eoe_amd.models import CNN32, WideResNet
    from eoe_amd.models.clip_vit import VisualTransformer
    from eoe_amd.training import TRAINER

    class Source:
        def test_inputs(self, rows):
            raise AssertionError("no input is asked for by the check")

        def loaders(self, *a, **k):
            raise AssertionError("no loader is asked for by the check")

    wrn = WideResNet(res=32)
    with pytest.raises(ValueError, match="extremes must be at least 1"):
        TRAINER["hsc"](wrn, cam=True)
    with pytest.raises(ValueError, match="cam_layer"):
        TRAINER["hsc"](wrn, extremes=1, cam=True, cam_layer="layer9")
    with pytest.raises(ValueError, match="cam_mode"):
        TRAINER["hsc"](wrn, extremes=1, cam=True, cam_mode="x")
    off = TRAINER["hsc"](wrn)
    assert off.with_cam is False and off.cams == {}
    tr = TRAINER["hsc"](wrn, extremes=2, cam=True, cam_layer="layer3", cam_mode="hirescam", device="cpu")
    assert tr.with_cam and tr.cam_layer == "layer3" and tr.cam_mode == "hirescam"
    tr._check_explainable(wrn, Source(), "cam", "")
    vit = VisualTransformer(32, 16, 64, 1, 1, 32)
    for model in (CNN32(), vit, torch.nn.Linear(4, 4)):
        with pytest.raises(NotImplementedError, match="no WideResNet"):
            tr._check_explainable(model, Source(), "cam", "")
    with pytest.raises(NotImplementedError, match="test_inputs"):
        tr._check_explainable(wrn, object(), "cam", "")
    # the options that existed keep their behaviour: the WideResNet refusal under "explain" and its wording, a ViT accepted
    with pytest.raises(NotImplementedError, match="outside a CNN32 or CNN28"):
        tr._check_explainable(wrn, Source())
    with pytest.raises(NotImplementedError, match="needs a ViT encoder"):
        tr._check_explainable(wrn, Source(), "attention", "whose attention could be rolled out")
    tr._check_explainable(vit, Source())
    tr._check_explainable(vit, Source(), "attention", "whose attention could be rolled out")
    # eval_cls refuses before any loader is asked for
    with pytest.raises(NotImplementedError, match="no WideResNet"):
        tr.eval_cls(CNN32(), Source(), 0, "only", 0)


def test_abi_lists_the_new_entry_points():
    from eoe_amd import _lib
    names = _lib.header_symbols()
    for f in ("eoe_cam_weights", "eoe_cam_map", "eoe_cam_upsample", "eoe_cbam_junction_bwd_data"):
        assert f in names and f in _lib.SIGNATURES and hasattr(_lib.lib, f)
    assert (_lib.EOE_CAM_GRADCAM, _lib.EOE_CAM_HIRESCAM) == (0, 1)
