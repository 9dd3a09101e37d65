"""GPU tier: the sharpen multi-scale mode (csrc/sharpen.hip) byte-exact against the g18 fixture (the reference's own
PilUnsharpMask) and the numpy restatement of Pillow's UnsharpMask, the crop / flip kernel against the oracle, the resident
source's pre-ToTensor path and the trainer / driver paths that apply sharpen."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import augment as oaug   # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g18_inputs():
    spec = importlib.util.spec_from_file_location("make_golden_sharpen", os.path.join(GOLDEN_DIR, "make_golden_sharpen.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _u8(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def test_sharpen_u8_equals_golden_and_restatement(golden):
    from eoe_amd.msm import sharpen_percent, sharpen_u8, unsharp_np
    g = golden("g18_sharpen")
    gen = _g18_inputs()
    for case, (h, w, c, k, mags) in gen.CASES.items():
        x = gen.images(case)
        xd = torch.from_numpy(x).cuda()
        for mag in mags:
            got = sharpen_u8(xd, sharpen_percent(mag)).cpu().numpy()
            assert np.array_equal(got, unsharp_np(x, sharpen_percent(mag))), (case, mag)
            if case == "rgb224":
                got = got[:, ::gen.GRID, ::gen.GRID]
            assert np.array_equal(got, g[f"out/{case}/{mag}"]), (case, mag)


@pytest.mark.parametrize("shape", [(256, 32, 32, 3), (37, 28, 28, 1), (5, 224, 224, 3), (3, 224, 224, 1), (9, 3, 3, 3), (7, 5, 7, 1),
                                   (2, 40, 37, 3), (3, 130, 97, 3)])
def test_sharpen_u8_general_radius_and_threshold(shape):
    from eoe_amd.msm import sharpen_u8, unsharp_np
    x = _u8(shape, shape[0] + shape[1])
    xd = x.cuda()
    # 6400-25600: the ImageNet driver's magnitudes 64, 128, 256 (d * percent up to 255 * 25600)
    for percent, radius, threshold in ((400, 2.0, 3), (150, 0.5, 0), (3200, 3.3, 10), (100, 10.0, 3), (250, 0.0, 3), (6400, 2.0, 3),
                                       (12800, 2.0, 3), (25600, 2.0, 3)):
        if shape[1] * shape[2] > 4096 and radius == 10.0:
            continue                          # the restatement is slow on wide windows of big planes; 3x3 / 5x7 / 28^2 cover it
        got = sharpen_u8(xd, percent, radius=radius, threshold=threshold).cpu().numpy()
        assert np.array_equal(got, unsharp_np(x.numpy(), percent, radius, threshold)), (shape, percent, radius, threshold)
    assert torch.equal(xd.cpu(), x), "the input is not modified"


@pytest.mark.parametrize("shape", [(64, 3, 32, 32), (8, 1, 28, 28), (4, 3, 224, 224)])
def test_msm_sharpen_on_the_tensor_grid_equals_tensor_of_pillow(shape):
    from eoe_amd.msm import msm_sharpen, sharpen_percent, unsharp_np
    n, c, h, w = shape
    u8 = _u8((n, h, w, c), 3 + h)
    x = u8.permute(0, 3, 1, 2).float().div(255)                         # ToTensor's bits
    xd = x.cuda()
    for mag in (1, 4, 32, 64, 128, 256):
        got = msm_sharpen(xd, mag).cpu()
        want = torch.from_numpy(unsharp_np(u8.numpy(), sharpen_percent(mag))).permute(0, 3, 1, 2).float().div(255)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (shape, mag)


@pytest.mark.parametrize("shape", [(64, 3, 32, 32), (6, 3, 224, 224)])
def test_unselected_rows_and_magnitude_zero_are_bit_copies(shape):
    from eoe_amd.msm import msm_sharpen, sharpen_u8
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g).cuda()                          # off the k / 255 grid on purpose
    rows = torch.arange(shape[0], device="cuda") % 3 == 1
    full, part = msm_sharpen(x, 4), msm_sharpen(x, 4, rows)
    assert torch.equal(part[~rows].view(torch.int32), x[~rows].view(torch.int32))
    assert torch.equal(part[rows].view(torch.int32), full[rows].view(torch.int32))
    assert torch.equal(msm_sharpen(x, 0).view(torch.int32), x.view(torch.int32))
    u8 = _u8((shape[0], shape[2], shape[3], shape[1]), 2).cuda()
    full, part = sharpen_u8(u8, 400), sharpen_u8(u8, 400, rows)
    assert torch.equal(part[~rows], u8[~rows]) and torch.equal(part[rows], full[rows]) and not torch.equal(full, u8)
    assert torch.equal(sharpen_u8(u8, 0), u8)


@pytest.mark.parametrize("Hs,crop,pad,flip_first", [(32, 32, 4, True), (40, 32, 0, False), (17, 9, 3, True), (17, 9, 3, False)])
def test_crop_flip_u8_matches_oracle_geometry(Hs, crop, pad, flip_first):
    from eoe_amd.data import crop_flip_u8
    rng = np.random.RandomState(1)
    src = rng.randint(0, 256, size=(11, Hs, Hs + 3, 3), dtype=np.uint8)
    n = 37
    params = np.stack([rng.randint(0, 11, n), rng.randint(-pad, Hs + pad - crop + 1, n), rng.randint(-pad, Hs + 3 + pad - crop + 1, n),
                       rng.randint(0, 2, n)], axis=1).astype(np.int32)
    got = crop_flip_u8(torch.from_numpy(src).cuda(), torch.from_numpy(params).cuda(), (crop, crop), flip_first).cpu()
    want = oaug.augment_batch(src, params, crop, crop, None, None, flip_first, 0.0, 0)
    assert torch.equal(got.permute(0, 3, 1, 2).float().div(255), torch.from_numpy(want))


# --------------------------------------------------------------------------------------------------------------- source / trainer
def _resident(seed=0, n=64, n_oe=64, n_test=32, noise_std=0.001):
    from eoe_amd.data import ResidentImageSource
    g = torch.Generator().manual_seed(200 + seed)
    mk = lambda k: torch.randint(0, 256, (k, 32, 32, 3), generator=g, dtype=torch.uint8)
    normal, oe, test = mk(n), mk(n_oe), mk(n_test)
    ty = torch.tensor([0, 1] * (n_test // 2))
    return lambda: ResidentImageSource(normal, oe, test, ty, crop=32, padding=4, mean=[0.4, 0.45, 0.5], std=[0.25, 0.2, 0.3], seed=seed,
                                       noise_std=noise_std)


def _train_batches(src, msms=None, batch_size=32):
    if msms is not None:
        src.pre_tensor_msms(msms)
    tr, _ = src.loaders(batch_size)
    return [(b[0].clone(), b[1].clone()) for b in tr]


def test_resident_source_sharpen_at_magnitude_zero_is_bitwise_the_plain_source():
    from eoe_amd.msm import MSM
    make = _resident(seed=1)
    plain = _train_batches(make())
    m0 = _train_batches(make(), [MSM.load("sharpen+train_nominal--M0"), MSM.load("sharpen+train_oe--M0")])
    m4 = _train_batches(make(), [MSM.load("sharpen+train_nominal--M4")])
    assert len(plain) == len(m0) == 2
    for (a, la), (b, lb), (c, _) in zip(plain, m0, m4):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(la, lb)
        half = a.shape[0] // 2
        assert not torch.equal(a[:half], c[:half]) and torch.equal(a[half:].view(torch.int32), c[half:].view(torch.int32))


def test_resident_source_sharpen_without_noise_equals_msm_sharpen_of_plain_batches():
    from eoe_amd.msm import MSM, msm_sharpen
    make = _resident(seed=2, noise_std=0.0)
    plain_src, sharp_src = make(), make()
    for s in (plain_src, sharp_src):
        s.defer_normalize(True)                                          # [0, 1] batches
    plain = _train_batches(plain_src)
    sharp = _train_batches(sharp_src, [MSM.load("sharpen+train_nominal--M4"), MSM.load("sharpen+train_oe--M2")])
    for (x, y), (got, _) in zip(plain, sharp):
        nominal = (y == 0).cuda()
        want = msm_sharpen(msm_sharpen(x, 4, nominal), 2, ~nominal)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


class _RecordingLogger:
    def __init__(self):
        self.json = {}

    def print(self, msg):
        pass

    warning = logtxt = print

    def logjson(self, name, obj):
        self.json[name] = obj

    def snapshot(self, *a, **k):
        return None


def test_cnn32_hsc_with_train_sharpen_matches_batches_sharpened_by_the_restatement():
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM, sharpen_percent, unsharp_np
    torch.manual_seed(0)
    m0 = CNN32(bias=True)
    normalize = ([0.4, 0.45, 0.5], [0.25, 0.2, 0.3])
    batches, pre = [], []
    for i in range(2):
        u8 = _u8((64, 32, 32, 3), 40 + i)
        y = torch.tensor([0] * 32 + [1] * 32)
        batches.append((u8.permute(0, 3, 1, 2).float().div(255), y, torch.arange(64)))
        s = u8.numpy().copy()
        s[:32] = unsharp_np(s[:32], sharpen_percent(4))
        pre.append((torch.from_numpy(s).permute(0, 3, 1, 2).float().div(255), y, torch.arange(64)))
    out = {}
    for name, bs, ms in (("hip", batches, [MSM.load("sharpen+train_nominal--M4")]), ("np", pre, ())):
        src = ListSource(bs, normalize=normalize)
        tr = HSC(copy.deepcopy(m0), src, ms)
        tr.train_cls(copy.deepcopy(m0), src, 0, "0", 0)
        out[name] = (tr.last_losses[0], torch.cat([s for _, s in tr.last_scores]).cpu())
    assert abs(out["hip"][0] - out["np"][0]) <= 1e-4 * max(1.0, abs(out["np"][0])), out
    assert (out["hip"][1] - out["np"][1]).abs().max() <= 1e-4 * max(1.0, out["np"][1].abs().max().item())


def HSC(model, src, msms, batch_size=64):
    from eoe_amd.training import HSCTrainer
    return HSCTrainer(model, dataset=src, epochs=1, lr=1e-3, batch_size=batch_size, msms=msms, logger=_RecordingLogger())


def test_resident_source_trainer_run_with_train_sharpen():
    """the trainer hands the train sharpen MSMs to the resident source: a finite run whose losses differ from the plain run"""
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM
    make = _resident(seed=4)
    torch.manual_seed(5)
    m0 = CNN32(bias=True)
    losses = {}
    for name, ms in (("plain", ()), ("m0", [MSM.load("sharpen+train_oe--M0")]), ("m8", [MSM.load("sharpen+train_nominal--M8")])):
        src = make()
        tr = HSC(copy.deepcopy(m0), src, ms, batch_size=32)
        tr.train_cls(copy.deepcopy(m0), src, 0, "0", 0)
        assert tr._step_msms == []
        losses[name] = list(tr.last_losses)
    assert np.isfinite(losses["m8"]).all() and losses["m8"] != losses["plain"]
    assert np.allclose(losses["m0"], losses["plain"], rtol=1e-5, atol=1e-6)     # M0 batches are bitwise the plain ones


def test_multiscale_experiment_with_test_sharpen_trains_once_and_changes_only_eval_scores():
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM
    from eoe_amd.training import multiscale_experiment
    make = _resident(seed=7, n=32, n_oe=32, n_test=32)
    trained, scores = {}, {}
    torch.manual_seed(3)
    m0 = CNN32(bias=True)

    def make_trainer(msms, magnitude):
        tr = HSC(copy.deepcopy(m0), make(), msms, batch_size=16)
        orig_train, orig_eval = tr.train_cls, tr.eval_cls

        def train_cls(*a, **k):
            out = orig_train(*a, **k)
            trained[magnitude] = len(tr.last_losses)
            return out

        def eval_cls(*a, **k):
            out = orig_eval(*a, **k)
            scores[magnitude] = np.array(list(tr.logger.json["eval_cls0_it0_anomaly_scores"].values()))
            return out
        tr.train_cls, tr.eval_cls = train_cls, eval_cls
        return tr

    res = multiscale_experiment(make_trainer, [MSM.load("sharpen+test_nominal")], magnitudes=(0, 4))
    assert trained == {0: 2, 4: 0}, trained
    assert res["ms_mode"] == ["sharpen+test_nominal--M4"] and all(np.isfinite(res["aucs"]))
    assert np.isfinite(scores[4]).all() and np.abs(scores[0] - scores[4]).max() > 0
