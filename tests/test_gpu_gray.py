"""GPU tier: the 1-channel device input path of the 28 x 28 tasks (`main/train_fmnist.py:31-38`, `main/train_mnist.py`) --
eoe_grayscale_u8 against Pillow's bytes (fixture g22), the one-channel crop / flip / augment against Pillow and the oracle, the
resident source with grayscale= / flip=, a CNN28 trainer run on it, and every other input-pipeline function on 1-channel input."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gray_util as gu                     # noqa: E402
import normstats_util as nu                # noqa: E402
from oracle import augment as oaug         # noqa: E402
from oracle import fill as ofill           # noqa: E402

NOISE_TOL = 2e-6        # tests/test_gpu_augment.py::test_augment_kernel_vs_oracle: device logf / cosf vs numpy on a 0.001-scaled term


def _unit(u8_nhwc: torch.Tensor) -> torch.Tensor:
    """ToTensor of a uint8 NHWC set, computed on the host with a true fp32 division (torch's device division by a scalar multiplies
    by the reciprocal, which is one ulp off for some bytes): fp32 NCHW in [0, 1]"""
    x = u8_nhwc.cpu().numpy().astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def _formula(x: torch.Tensor) -> torch.Tensor:
    """the integer formula in torch, uint8 [..., 3] -> uint8 [..., 1]"""
    w = torch.tensor(gu.L_WEIGHTS, dtype=torch.int64, device=x.device)
    return (((x.to(torch.int64) * w).sum(-1, keepdim=True) + 0x8000) >> 16).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------ 1. Grayscale(1)
def test_grayscale_equals_pillow(golden):
    from eoe_amd.data import grayscale_u8
    g = golden("g22_gray")
    colour = torch.from_numpy(gu.colour_set()).cuda()
    got = grayscale_u8(colour)
    assert got.shape == (gu.N_IMG, 32, 32, 1) and got.dtype == torch.uint8
    got = got.cpu().numpy()[..., 0]
    assert got[0].ravel()[:5].tolist() == [255, 0, 76, 150, 29]                    # white, black, red, green, blue
    n_b = len(gu.boundary_pixels())
    assert np.array_equal(got[1].ravel()[:n_b], g["L"][1].ravel()[:n_b])           # the rounding boundaries
    assert np.array_equal(got, g["L"])
    # a pixel count that is no multiple of the 16 pixels a thread takes: 3 * 5 * 7 = 105 = 6 * 16 + 9
    small = torch.from_numpy(ofill.fill_int("g22/small", (3, 5, 7, 3), 0, 256).astype(np.uint8)).cuda()
    assert torch.equal(grayscale_u8(small), _formula(small))
    # a contiguous view that does not start on a 16-byte boundary (105 bytes into the allocation), and fewer pixels than one thread's
    assert torch.equal(grayscale_u8(small[1:]), _formula(small[1:]))
    assert torch.equal(grayscale_u8(small[:1, :1, :5]), _formula(small[:1, :1, :5]))
    # a non-contiguous input is made contiguous (the wrapper's docstring): every other column
    view = colour[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(grayscale_u8(view), _formula(view))
    assert torch.equal(colour.cpu(), torch.from_numpy(gu.colour_set()))            # out of place
    with pytest.raises(ValueError, match="3 channels, not 1"):
        grayscale_u8(colour[..., :1])


# ------------------------------------------------------------------------------------------------------------ 2. one-channel crop / flip / augment
def _ulps(got: np.ndarray, want: np.ndarray) -> float:
    """largest distance in units of the fp32 spacing at the expected value"""
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -100)))))


@pytest.mark.parametrize("flip_first", [True, False])
@pytest.mark.parametrize("case", list(gu.CROP_CASES))
def test_one_channel_crop_flip_and_augment(golden, case, flip_first):
    from eoe_amd.data import augment_batch, crop_flip_u8, grayscale_u8
    g = golden("g22_gray")
    out_hw = gu.CROP_CASES[case][1]
    src = gu.case_source(case, g["L"])
    rows, want = g[f"{case}/rows"], g[f"{case}/ff{int(flip_first)}"]
    src_d = torch.from_numpy(src[..., None].copy()).cuda()
    src3_d = src_d.expand(-1, -1, -1, 3).contiguous()                              # three equal planes: L(v, v, v) = v
    mean, std = [0.2861], [0.3530]
    for bs in (len(rows), 1, 5):
        p = torch.from_numpy(rows[:bs].copy()).cuda()
        # crop / flip: Pillow's bytes
        u8 = crop_flip_u8(src_d, p, out_hw, flip_first)
        assert u8.shape == (bs,) + out_hw + (1,) and u8.dtype == torch.uint8
        assert np.array_equal(u8.cpu().numpy()[..., 0], want[:bs]), (case, bs)
        # the 3-channel kernel on the same rows is what it was: Grayscale commutes with crop and flip
        u8_3 = crop_flip_u8(src3_d, p, out_hw, flip_first)
        assert u8_3.shape == (bs,) + out_hw + (3,) and torch.equal(grayscale_u8(u8_3), u8)
        # ToTensor: u8 / 255, then Normalize: two fp32 operations, each to 1 ulp
        w255 = want[:bs].astype(np.float32) / np.float32(255.0)
        x = augment_batch(src_d, p, out_hw, None, None, flip_first, 0.0, 0)
        assert x.shape == (bs, 1) + out_hw and x.dtype == torch.float32
        assert _ulps(x.cpu().numpy()[:, 0], w255) <= 1.0
        x = augment_batch(src_d, p, out_hw, mean, std, flip_first, 0.0, 0).cpu().numpy()
        wn = (w255 - np.float32(mean[0])) / np.float32(std[0])
        print(f"[{case} ff={int(flip_first)} bs={bs}] normalised, no noise: {_ulps(x[:, 0], wn):.2f} ulp")
        assert _ulps(x[:, 0], wn) <= 1.0
        # with noise: the oracle's restatement on three equal planes, plane 0 (element e < Ho * Wo: the 1-channel counters)
        x = augment_batch(src_d, p, out_hw, mean, std, flip_first, 0.001, 5).cpu().numpy()
        wo = oaug.augment_batch(src3_d.cpu().numpy(), rows[:bs], out_hw[0], out_hw[1], mean * 3, std * 3, flip_first, 0.001, 5)[:, :1]
        dev = float(np.abs(x - wo).max())
        print(f"[{case} ff={int(flip_first)} bs={bs}] noise 0.001: max deviation from the oracle {dev:.3e} (allowed {NOISE_TOL:g})")
        assert dev < NOISE_TOL
        # and the 3-channel augment of the same call has that plane 0 too
        x3 = augment_batch(src3_d, p, out_hw, mean * 3, std * 3, flip_first, 0.001, 5).cpu().numpy()
        assert x3.shape == (bs, 3) + out_hw and float(np.abs(x3[:, :1] - wo).max()) < NOISE_TOL
    if case == "c32":
        # the real colour set: crop / flip in colour, then Grayscale == Grayscale once, then the one-channel crop / flip
        colour = torch.from_numpy(gu.colour_set()).cuda()
        p = torch.from_numpy(rows.copy()).cuda()
        a = grayscale_u8(crop_flip_u8(colour, p, out_hw, flip_first))
        assert torch.equal(a, crop_flip_u8(grayscale_u8(colour), p, out_hw, flip_first))
        assert np.array_equal(a.cpu().numpy()[..., 0], want)
    with pytest.raises(ValueError, match="one value per channel"):
        augment_batch(src_d, p, out_hw, [0.5] * 3, [0.2] * 3, flip_first, 0.0, 0)


# ------------------------------------------------------------------------------------------------------------ 3. the resident source
BATCH = 16


def _sets():
    """40 gray 28 x 28 normal images (the g20 statistics case 'gray40'), 24 colour 32 x 32 OE images, 16 gray test images"""
    normal = torch.from_numpy(nu.stats_set("gray40"))
    oe = torch.from_numpy(gu.colour_set())
    test = torch.from_numpy(ofill.fill_int("g22/test", (16, 28, 28), 0, 256).astype(np.uint8))
    ty = torch.cat([torch.zeros(8, dtype=torch.int64), torch.ones(8, dtype=torch.int64)])
    return normal, oe, test, ty


def _epoch_with_draws(ds):
    drawn, real = [], ds._params
    ds._params = lambda idx, Hs, Ws: (drawn.append(real(idx, Hs, Ws)), drawn[-1])[1]
    train, test = ds.loaders(BATCH)
    return [(x, y, i) for x, y, i in train], test, drawn


def test_resident_source_grayscale(golden):
    from eoe_amd.data import ResidentImageSource
    normal, oe, test, ty = _sets()
    ds = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, seed=3, mean=[0.5], std=[0.25])
    assert ds.normal.shape == (40, 28, 28, 1) and ds.oe.shape == (24, 32, 32, 1) and ds.test.shape == (16, 28, 28, 1)
    assert np.array_equal(ds.oe.cpu().numpy()[..., 0], golden("g22_gray")["L"])    # converted once, Pillow's bytes
    batches, tst, drawn = _epoch_with_draws(ds)
    assert [b[0].shape for b in batches] == [(2 * BATCH, 1, 28, 28), (2 * BATCH, 1, 28, 28), (16, 1, 28, 28)]
    for x, y, i in batches:
        n = y.shape[0] // 2
        assert x.is_cuda and x.dtype == torch.float32 and torch.isfinite(x).all()
        assert y[:n].eq(0).all() and y[n:].eq(1).all()
        assert i[:n].max() < 40 and i[n:].min() >= 40 and i[n:].max() < 40 + 24        # OE indices offset by the normal set
    assert sorted(torch.cat([b[2][: b[1].shape[0] // 2] for b in batches]).tolist()) == list(range(40))
    assert len(tst) == 1 and tst[0][0].shape == (16, 1, 28, 28)
    want = (_unit(ds.test).numpy() - np.float32(0.5)) / np.float32(0.25)           # centre crop of a 28 x 28 image: the image
    assert np.array_equal(tst[0][0].cpu().numpy(), want)
    # the host draws what a 3-channel source of the same sizes draws from the same seed
    three = ResidentImageSource(normal.expand(-1, -1, -1, 3).contiguous(), oe, test.unsqueeze(-1).expand(-1, -1, -1, 3).contiguous(), ty,
                                crop=28, padding=3, seed=3, mean=[0.5] * 3, std=[0.25] * 3)
    b3, _, drawn3 = _epoch_with_draws(three)
    assert len(drawn) == len(drawn3) == 6 and all(torch.equal(a, b) for a, b in zip(drawn, drawn3))
    assert all(torch.equal(a[2], b[2]) for a, b in zip(batches, b3)) and b3[0][0].shape == (2 * BATCH, 3, 28, 28)
    assert {int(v) for d in drawn for v in d[:, 3]} == {0, 1}
    assert max(int(d[:, 2].max()) for d in drawn[1::2]) > 3                         # the OE half draws from its own 32-wide range
    # the normal half of the 3-channel source has three equal planes; plane 0 has the 1-channel batch's draws and noise counters.
    # Two kernels: each is within NOISE_TOL of the oracle (test above, tests/test_gpu_augment.py), so within twice that of each other
    nb = BATCH
    assert float((b3[0][0][:nb, :1] - batches[0][0][:nb]).abs().max()) < 2 * NOISE_TOL

    # the MNIST chain: no flip, no crop, no noise -> the source bytes / 255
    gray_oe = torch.from_numpy(gu.gray_set())
    mn = ResidentImageSource(normal, gray_oe, test, ty, crop=28, padding=0, noise_std=0.0, flip=False, grayscale=True, seed=3)
    mb, _, md = _epoch_with_draws(mn)
    assert all(int(d[:, 1:].abs().max()) == 0 for d in md)                          # origin (0, 0), flip 0
    for x, y, i in mb:
        n = y.shape[0] // 2
        assert torch.equal(x[:n].cpu(), _unit(normal[i[:n]]))
        assert torch.equal(x[n:].cpu(), _unit(gray_oe[i[n:] - 40].unsqueeze(-1)))
    # flip=False with the crop: flips are zeros, and the images are unflipped crops
    nf = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, noise_std=0.0, flip=False, grayscale=True, seed=3)
    fb, _, fd = _epoch_with_draws(nf)
    assert all(int(d[:, 3].abs().max()) == 0 for d in fd)
    d0 = fd[0]
    ref = oaug.augment_batch(np.repeat(normal.numpy(), 3, axis=-1), d0.numpy(), 28, 28, None, None, True, 0.0, 0)[:, :1]
    assert np.array_equal(fb[0][0][:nb].cpu().numpy(), ref)

    with pytest.raises(ValueError, match="color_jitter"):
        ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, color_jitter=(0.01,) * 4)


def test_resident_source_grayscale_statistics(golden):
    """normalize= on a 1-channel set: one-element statistics, the float64 running statistics of the normal subset"""
    from eoe_amd.data import ResidentImageSource
    from eoe_amd.normalize import GcnNormalize
    normal, oe, test, ty = _sets()
    g20 = golden("g20_normstats")
    ds = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, normalize="normalize")
    assert len(ds.mean) == 1 and len(ds.std) == 1 and ds.ds_statistics == {"mean": ds.mean, "std": ds.std, "mode": 0}
    print("\n   " + nu.check_stats_dict(ds.ds_statistics, g20, "gray40", 0, "source "))
    # a subset of the rows: the helper's recurrence in float64 on those images; the allowance is the floor of the rule in
    # normstats_util (one fp32 ulp, relative: the statistics reach the kernels as fp32 numbers)
    rows = torch.arange(1, 40, 3)
    sub = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, normalize="normalize", normal_index=rows)
    m, s = nu.running_stats_np(normal[rows].permute(0, 3, 1, 2).numpy().astype(np.float32).__truediv__(np.float32(255)).astype(np.float64))
    assert m.shape == (1,) and abs(sub.mean[0] - m[0]) <= nu.STATS_FLOOR * abs(m[0]) and abs(sub.std[0] - s[0]) <= nu.STATS_FLOOR * abs(s[0])
    assert sub.mean != ds.mean
    x = next(iter(sub.loaders(BATCH)[0]))[0]
    assert x.shape == (2 * len(rows), 1, 28, 28) and torch.isfinite(x).all()
    gcn = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, normalize="gcn-normalize")
    assert isinstance(gcn.normalize, GcnNormalize) and len(gcn.normalize.shift) == 1 and gcn.mean is None
    print("   " + nu.check_stats_dict(gcn.ds_statistics, g20, "gray40", 1, "source "))
    y = gcn.normalize(next(iter(gcn.loaders(BATCH)[0]))[0])
    assert y.shape == (2 * BATCH, 1, 28, 28) and torch.isfinite(y).all()
    # given statistics win and round-trip
    again = ResidentImageSource(normal, oe, test, ty, crop=28, padding=3, grayscale=True, normalize="normalize",
                                ds_statistics=dict(sub.ds_statistics))
    assert again.ds_statistics == sub.ds_statistics and again.mean == sub.mean


# ------------------------------------------------------------------------------------------------------------ 4. end to end
def _scores(logdir):
    with open(f"{logdir}/eval_cls0_it0_anomaly_scores.json") as f:
        return json.load(f)


def test_cnn28_trains_on_the_grayscale_set_and_its_snapshot_scores_identically(tmp_path):
    """every layer connected: LabelledImageSet(grayscale=True, normalize='normalize') -> ResidentImageSource -> the one-channel
    augment kernel -> CNN28 with the fused one-element Normalize -> HSC; the snapshot carries the one-element statistics and
    scores the test split bit for bit again"""
    from eoe_amd.data import LabelledImageSet
    from eoe_amd.models import CNN28
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    normal, oe, test, ty = _sets()
    torch.manual_seed(0)
    mk = lambda: LabelledImageSet(normal, torch.zeros(40, dtype=torch.int64), test, ty, oe, ["normal", "other"], crop=28,   # noqa: E731
                                  padding=3, grayscale=True, normalize="normalize")
    lset = mk()
    assert lset.oe.shape == (24, 32, 32, 1)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    tr = TRAINER["hsc"](CNN28(bias=True), dataset=lset, epochs=2, lr=1e-3, batch_size=BATCH, logger=JsonLogger(d1))
    _, res = tr.run(run_classes=[0])
    assert len(tr.last_losses) == 2 * 3 and all(np.isfinite(tr.last_losses))
    assert len(tr.last_scores) == 2
    for la, sc in tr.last_scores:
        assert la.shape == (2 * 40,) and sc.shape == (2 * 40,) and torch.isfinite(sc).all()
    assert np.isfinite(res["mean_auc"])
    path = f"{d1}/snapshots/snapshot_cls0_it0.pt"
    st = torch.load(path)["ds_statistics"]
    assert st["mode"] == 0 and len(st["mean"]) == 1 and len(st["std"]) == 1 and all(type(v) is float for v in st["mean"] + st["std"])
    assert st == lset.source([0], 0).ds_statistics
    first = _scores(d1)
    assert len(first) == 16 and all(np.isfinite(v) for v in first.values())
    tr2 = TRAINER["hsc"](CNN28(bias=True), dataset=mk(), epochs=2, lr=1e-3, batch_size=BATCH, logger=JsonLogger(d2))
    tr2.run(run_classes=[0], load=[[path]], train=False)
    assert _scores(d2) == first
    assert torch.load(f"{d2}/snapshots/snapshot_cls0_it0.pt")["ds_statistics"] == st


# ------------------------------------------------------------------------------------------------------------ 5. the rest of the pipeline on one channel
def _one_and_three(n=3, hw=12):
    one = torch.from_numpy(ofill.fill_int("g22/c1", (n, hw, hw, 1), 0, 256).astype(np.uint8)).cuda()
    return one, one.expand(-1, -1, -1, 3).contiguous()


def test_resize_works_on_one_channel():
    """WORKS: the passes run over [outer, axis, inner] bytes, the channels are `inner`"""
    from eoe_amd.data import resize_u8
    one, three = _one_and_three()
    for size, filt in (((8, 9), "bilinear"), ((17, 12), "bicubic"), (7, "bilinear"), ((12, 5), "bicubic")):
        a, b = resize_u8(one, size, filt), resize_u8(three, size, filt)
        assert a.shape == b.shape[:3] + (1,) and torch.equal(a, b[..., :1]), (size, filt)
        assert torch.equal(b[..., 0], b[..., 2])


def test_fit_statistics_works_on_one_channel():
    """WORKS: exact integer sums per channel; both modes give one element, equal to each element of the three-equal-planes fit
    (mean / std: the same arithmetic per channel; GCN extremes: the same rationals N (N min - S) / D, numerator and denominator
    scaled by 9, both exact in float64 at this size, so the correctly rounded quotients are equal)"""
    from eoe_amd import fit_statistics
    one, three = _one_and_three(n=5)
    for mode in ("normalize", "gcn-normalize"):
        for index in (None, [0, 2, 3]):
            a, b = fit_statistics(one, index, mode), fit_statistics(three, index, mode)
            assert len(a["mean"]) == 1 and len(a["std"]) == 1 and a["mode"] == b["mode"]
            assert b["mean"] == a["mean"] * 3 and b["std"] == a["std"] * 3, (mode, index)


def test_gcn_normalize_works_on_one_channel():
    """WORKS: against the torch-op chain in float64 (tests/normstats_util.py) to one fp32 ulp relative to max(1, |y|), the bound of
    tests/test_gpu_normstats.py for this operator.  Under 'l1', GCN of three equal planes is GCN of one (same mean, same mean
    absolute deviation), so plane 0 of the 3-channel result meets the same twin"""
    from eoe_amd import gcn_normalize
    one, three = _one_and_three(n=4)
    x1, x3 = _unit(one).cuda(), _unit(three).cuda()
    close = lambda got, want: np.max(np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(1.0, np.abs(want))) <= 2.0 ** -23   # noqa: E731
    for scale in ("l1", "l2"):
        for sh, rg in ((None, None), ([-1.25], [3.5])):
            want = nu.torch_gcn_normalize(x1.cpu().double(), scale, sh, rg).numpy()
            assert close(gcn_normalize(x1, scale, sh, rg), want), (scale, sh)
            if scale == "l1":
                y3 = gcn_normalize(x3, scale, None if sh is None else sh * 3, None if rg is None else rg * 3)
                assert close(y3[:, :1], want), (scale, sh)
    y = x1.clone()
    assert gcn_normalize(y, "l1", [-1.25], [3.5], out=y) is y and torch.equal(y, gcn_normalize(x1, "l1", [-1.25], [3.5]))
    with pytest.raises(ValueError, match="one value per channel"):
        gcn_normalize(x1, "l1", [-1.25] * 3, [3.5] * 3)


@pytest.mark.parametrize("op,magnitude", [("lpf", 2), ("hpf", 2), ("blur", 3)])
def test_msm_filters_work_on_one_channel(op, magnitude):
    """WORKS: the filters run per plane and MinMaxNorm per image; with three equal planes the image extremes are the plane's, so
    plane 0 of the 3-channel result is the 1-channel result, bit for bit (the same per-plane arithmetic)"""
    from eoe_amd.msm import msm_filter
    one, three = _one_and_three(n=4)
    x1, x3 = _unit(one).cuda(), _unit(three).cuda()
    rows = torch.tensor([1, 0, 1, 1], dtype=torch.uint8)
    y1, y3 = msm_filter(x1, op, magnitude, rows), msm_filter(x3, op, magnitude, rows)
    assert y1.shape == x1.shape and torch.equal(y1, y3[:, :1]) and torch.equal(y1[1], x1[1]) and not torch.equal(y1[0], x1[0])


def test_sharpen_works_on_one_channel():
    """WORKS: Pillow's UnsharpMask runs per band; uint8 NHWC with C = 1 equals band 0 of three equal bands and the numpy restatement"""
    from eoe_amd.msm import sharpen_u8, msm_sharpen, unsharp_np
    one, three = _one_and_three(n=4)
    a, b = sharpen_u8(one, 150), sharpen_u8(three, 150)
    assert torch.equal(a, b[..., :1]) and np.array_equal(a.cpu().numpy(), unsharp_np(one.cpu().numpy(), 150))
    assert not torch.equal(a, one)
    assert torch.equal(msm_sharpen(_unit(one).cuda(), 1.5).cpu(), _unit(a))


def test_color_jitter_refuses_one_channel():
    """RAISES: the four ops are defined on RGB (ImageEnhance.Color, hue); no 1-channel chain of the reference has ColorJitter"""
    from eoe_amd.data import color_jitter_u8
    one, _ = _one_and_three()
    with pytest.raises(ValueError, match="3 channels, not 1"):
        color_jitter_u8(one, torch.arange(3), torch.ones(3, 4), torch.zeros((3, 4), dtype=torch.int32))
