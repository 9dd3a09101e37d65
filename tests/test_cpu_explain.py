"""CPU: the explanation entry points exist and refuse bad arguments before any launch, the numpy statements of the saliency and overlay
kernels on hand-worked examples, every differentiable score against oracle.objectives, and the refusals of eoe_amd.explain and the
trainer.  Case tables: tests/explain_util.py."""
import numpy as np
import pytest
import torch

import explain_util as xu
from oracle import fill, objectives

NEW_SYMBOLS = ("eoe_unpatchify_grad", "eoe_saliency_map", "eoe_heat_overlay_u8")
P, Q, R = 0x1000, 0x2000, 0x3000              # non-null, 16-byte aligned addresses nothing reads: every call below fails its checks first


def test_the_three_entry_points_are_exported_and_the_abi_version_stays():
    from eoe_amd import _lib
    assert _lib.lib.eoe_abi_version() == 5 and _lib.ABI_VERSION == 5
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(_lib.lib, name)
    assert (_lib.EOE_SALIENCY_MAX, _lib.EOE_SALIENCY_L2, _lib.EOE_SALIENCY_GRADXINPUT) == (0, 1, 2)


def test_unpatchify_grad_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_unpatchify_grad, lib.eoe_last_error
    assert f(None, None, 1.0, Q, 1, 32, 16, None) == 1 and b"null" in err()
    assert f(P, None, 1.0, None, 1, 32, 16, None) == 1 and b"null" in err()
    assert f(P, None, 1.0, Q, 1, 32, 6, None) == 1 and b"patch % 4" in err()
    assert f(P, None, 1.0, Q, 1, 32, 0, None) == 1 and b"patch % 4" in err()
    assert f(P, None, 1.0, Q, 1, 40, 16, None) == 1 and b"res % patch" in err()
    assert f(P, None, 1.0, Q, 1, 32768, 32768, None) == 1 and b"at most 1024" in err()
    assert f(P, None, 1.0, Q, -1, 32, 16, None) == 1 and b"negative" in err()
    assert f(P, None, float("nan"), Q, 1, 32, 16, None) == 1 and b"scale_inv" in err()
    assert f(P + 4, None, 1.0, Q, 1, 32, 16, None) == 1 and b"16-byte aligned" in err()
    assert f(P, None, 1.0, Q, 1 << 20, 224, 32, None) == 1 and b"32-bit indexing" in err()
    assert f(P, None, 1.0, Q, 0, 32, 16, None) == 0                     # an empty batch: nothing to launch


def test_saliency_map_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_saliency_map, lib.eoe_last_error
    assert f(None, None, R, 1, 3, 8, 8, 0, 0, None) == 1 and b"null" in err()
    assert f(P, None, None, 1, 3, 8, 8, 0, 0, None) == 1 and b"null" in err()
    assert f(P, None, R, 1, 3, 8, 8, 2, 0, None) == 1 and b"gradxinput needs x" in err()
    assert f(P, None, R, 1, 3, 8, 8, 3, 0, None) == 1 and b"mode" in err()
    for ch in (0, 2, 4):
        assert f(P, None, R, 1, ch, 8, 8, 0, 0, None) == 1 and b"C must be 1 or 3" in err()
    assert f(P, None, R, 1, 3, 8, 8, 0, 3, None) == 1 and b"does not divide" in err()
    assert f(P, None, R, 1, 3, 8, 12, 0, 8, None) == 1 and b"does not divide" in err()
    assert f(P, None, R, 1, 3, 8, 8, 0, -1, None) == 1 and b"pool" in err()
    assert f(P, None, R, 1, 3, 0, 8, 0, 0, None) == 1 and b"maps of" in err()
    assert f(P, None, R, 1 << 16, 3, 224, 224, 0, 0, None) == 1 and b"32-bit indexing" in err()
    assert f(P, None, R, 0, 3, 8, 8, 0, 0, None) == 0


def test_heat_overlay_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_heat_overlay_u8, lib.eoe_last_error
    assert f(None, Q, 0, R, 1, 3, 8, 8, 0.5, None) == 1 and b"null" in err()
    assert f(P, None, 0, R, 1, 3, 8, 8, 0.5, None) == 1 and b"null" in err()
    assert f(P, Q, 0, None, 1, 3, 8, 8, 0.5, None) == 1 and b"null" in err()
    for ch in (0, 2, 4):
        assert f(P, Q, 1, R, 1, ch, 8, 8, 0.5, None) == 1 and b"C must be 1 or 3" in err()
    for alpha in (-0.01, 1.01, float("nan")):
        assert f(P, Q, 0, R, 1, 3, 8, 8, alpha, None) == 1 and b"alpha must be in [0, 1]" in err()
    assert f(P, Q, 0, R, 1, 3, 8, 0, 0.5, None) == 1 and b"maps of" in err()
    assert f(P, Q, 0, R, 1 << 16, 3, 224, 224, 0.5, None) == 1 and b"32-bit indexing" in err()
    assert f(P, Q, 0, R, 0, 3, 8, 8, 0.5, None) == 0


def test_saliency_np_on_a_hand_worked_2x2_example():
    from eoe_amd.explain import saliency, saliency_np
    g = np.array([[[[1, -2], [3, 0]], [[-4, 1], [0, 0]], [[2, 2], [-5, 1]]]], dtype=np.float32)
    x = np.full_like(g, 0.5)
    assert np.array_equal(saliency_np(g, mode="max"), np.array([[[4, 2], [5, 1]]], np.float32))
    np.testing.assert_allclose(saliency_np(g, mode="l2"), np.array([[[np.sqrt(21), 3], [np.sqrt(34), 1]]]), rtol=1e-7)
    assert np.array_equal(saliency_np(g, x, mode="gradxinput"), np.array([[[3.5, 2.5], [4, 0.5]]], np.float32))
    assert np.array_equal(saliency_np(g, mode="max", pool=2), np.full((1, 2, 2), 3.0, np.float32))
    assert np.array_equal(saliency_np(g[:, :1], mode="max"), np.abs(g[:, 0]))
    # CPU tensors take the numpy route
    assert np.array_equal(saliency(torch.from_numpy(g), mode="max", pool=2).numpy(), np.full((1, 2, 2), 3.0, np.float32))
    with pytest.raises(ValueError, match="does not divide"):
        saliency_np(np.zeros((1, 3, 4, 6), np.float32), pool=4)
    with pytest.raises(ValueError, match="gradxinput needs x"):
        saliency(torch.from_numpy(g), mode="gradxinput")
    with pytest.raises(ValueError, match="none of"):
        saliency(torch.from_numpy(g), mode="sum")


def test_overlay_np_on_hand_worked_2x2_examples():
    from eoe_amd.explain import overlay, overlay_np
    pic = np.empty((1, 2, 2, 3), np.uint8)
    pic[...] = (100, 200, 48)
    m = np.array([[[0, 1], [2, 4]]], np.float32)                       # t = 0, 1/4, 1/2, 1
    want = np.array([[[[100, 200, 48], [139, 150, 36]], [[178, 100, 24], [255, 0, 0]]]], np.uint8)
    assert np.array_equal(overlay_np(m, pic, 1.0), want)
    assert np.array_equal(overlay_np(m, pic, 1.0, dtype=np.float64), want)
    assert np.array_equal(overlay_np(m, pic, 0.0), pic)
    # a constant map: t = 0 everywhere, the picture unchanged; fp32 pictures in ToTensor's scale give the same bytes
    assert np.array_equal(overlay_np(np.full((1, 2, 2), 7.0, np.float32), pic, 0.6), pic)
    picf = np.ascontiguousarray((pic.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    assert np.array_equal(overlay_np(np.full((1, 2, 2), 7.0, np.float32), picf, 0.6), pic)
    assert np.array_equal(overlay_np(m, picf, 1.0), want)
    # a NaN entry is cold and does not move the range: t = 0, 0, 1/2, 1
    mn = np.array([[[np.nan, 1], [2, 3]]], np.float32)
    assert np.array_equal(overlay_np(mn, pic, 1.0), np.array([[[[100, 200, 48], [100, 200, 48]], [[178, 100, 24], [255, 0, 0]]]], np.uint8))
    assert np.array_equal(overlay_np(np.full((1, 2, 2), np.inf, np.float32), pic, 1.0), pic)
    # one channel fills the three
    gray = np.full((1, 2, 2, 1), 100, np.uint8)
    assert np.array_equal(overlay_np(m, gray, 1.0)[0, :, :, 0], want[0, :, :, 0]) and np.array_equal(overlay_np(m, gray, 0.0), np.repeat(gray, 3, 3))
    assert np.array_equal(overlay(torch.from_numpy(m), torch.from_numpy(pic), 1.0).numpy(), want)
    with pytest.raises(ValueError, match="alpha"):
        overlay_np(m, pic, 1.5)
    with pytest.raises(ValueError, match="do not fit"):
        overlay_np(m, pic[:, :1], 0.5)


@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", xu.OVERLAY_SIZES)
def test_the_overlay_inputs_avoid_ties_and_fp32_stays_within_the_share_of_float64(H, W, C, u8):
    """floor(v + 0.5) in fp32 and in float64 can differ only where v is within rounding of a half-integer: the chosen inputs have no
    exact tie, and overlay_np's two precisions differ on at most OVERLAY_MAX_DIFF_SHARE of the bytes, by one grey level"""
    from eoe_amd.explain import overlay_np
    maps, pics = xu.overlay_case(H, W, C, u8)
    t = xu.heat_levels(maps)[..., None]
    img = pics.astype(np.float64) if u8 else pics.astype(np.float64).transpose(0, 2, 3, 1) * 255.0
    img = np.repeat(img, 3, axis=3) if C == 1 else img
    for alpha in xu.OVERLAY_ALPHAS:
        v = img * (1 - alpha * t) + np.array([255.0, 0.0, 0.0]) * alpha * t
        hot = (alpha * t) > 0                                              # at t = 0 the value is the byte itself
        dist = np.abs(v - np.floor(v) - 0.5)
        assert not hot.any() or dist[np.broadcast_to(hot, v.shape)].min() > 0.0
        a, b = overlay_np(maps, pics, alpha), overlay_np(maps, pics, alpha, dtype=np.float64)
        diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
        assert diff.max() <= 1 and (diff != 0).mean() <= xu.OVERLAY_MAX_DIFF_SHARE, (diff.max(), (diff != 0).mean())
        exact = np.broadcast_to((t == 0) | (t == 1), diff.shape)
        assert (diff[exact] == 0).all()


@pytest.mark.parametrize("name", ["hsc", "bce", "focal", "dsad", "dsvdd", "clip"])
def test_every_score_fn_equals_the_oracle_score(name):
    from eoe_amd import explain
    n, d = 5, (1 if name in ("bce", "focal") else 24)
    f = torch.from_numpy(fill.fill(f"explain/score/{name}", (n, d), std=1.0)).double()
    center = None
    if name == "dsvdd":
        center = torch.from_numpy(fill.fill("explain/score/center", (1, d), std=1.0)).double()
    if name == "clip":
        center = torch.from_numpy(fill.fill("explain/score/text", (3, d), std=1.0)).double()
    want = {"hsc": lambda: objectives.hsc_score(f), "dsad": lambda: objectives.hsc_score(f), "bce": lambda: objectives.bce_score(f, 0),
            "focal": lambda: objectives.bce_score(f, 0), "dsvdd": lambda: objectives.dsvdd_score(f, center),
            "clip": lambda: objectives.clip_score(f, center)}[name]()
    x = f.clone().requires_grad_()
    got = explain.score_fn(name, center)(x)
    assert got.shape == (n,) and (got - want).abs().max().item() <= 1e-6
    (g,) = torch.autograd.grad(got.sum(), x)
    assert torch.isfinite(g).all() and g.abs().sum() > 0
    if name in ("bce", "focal"):
        flipped = explain.score_fn(name, nominal_label=1)(f)
        assert (flipped - objectives.bce_score(f, 1)).abs().max().item() <= 1e-6


def test_score_fn_reads_a_trainer_and_refuses_what_it_does_not_know():
    from eoe_amd import explain
    from eoe_amd.training import TRAINER
    f = torch.from_numpy(fill.fill("explain/score/trainer", (5, 8), std=1.0))
    for name, cls in TRAINER.items():
        if name in ("dsvdd", "clip"):
            with pytest.raises(ValueError, match="needs its center"):
                explain.score_fn(cls)
        else:
            assert explain.score_fn(cls)(f[:, :1] if name in ("bce", "focal") else f).shape == (5,)
    tr = TRAINER["dsvdd"](torch.nn.Linear(2, 2))
    tr.center = torch.zeros(1, 8)
    assert torch.equal(explain.score_fn(tr)(f), (f ** 2).sum(-1))
    with pytest.raises(ValueError, match="no differentiable score"):
        explain.score_fn("autoencoder")


def test_input_gradient_refuses_a_batchnorm_model_and_the_trainer_explain_without_extremes():
    from eoe_amd import explain
    from eoe_amd.training import TRAINER
    bn = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4)).train()
    with pytest.raises(NotImplementedError, match="eval-mode BatchNorm"):
        explain.input_gradient(bn, torch.zeros(1, 3, 8, 8), explain.score_fn("hsc"))
    assert bn.training and bn[1].training                                # refused before the mode was touched
    with pytest.raises(ValueError, match="extremes must be at least 1"):
        TRAINER["hsc"](torch.nn.Linear(2, 2), explain=True, extremes=0)
    with pytest.raises(ValueError, match="extremes must be at least 1"):
        TRAINER["hsc"](torch.nn.Linear(2, 2), explain=True)
    tr = TRAINER["hsc"](torch.nn.Linear(2, 2), explain=True, extremes=2)
    assert tr.with_explain and tr.explanations == {} and not TRAINER["hsc"](torch.nn.Linear(2, 2)).with_explain


def test_the_input_gradient_bars_follow_from_the_measured_table():
    """twice the worst measured value, rounded up to one digit, and every measurement below the ceiling past which it is a defect"""
    import math
    from gpu_util import EPS16
    for dt, table in xu.INPUT_GRAD_MEASURED.items():
        worst = max(table.values())
        assert worst * EPS16[dt] <= xu.input_grad_ceiling(EPS16[dt])
        mag = 10 ** math.floor(math.log10(2 * worst))
        assert xu.INPUT_GRAD_BAR[dt] == math.ceil(2 * worst / mag) * mag
