"""GPU tier: the multi-scale-mode filters (csrc/msm.hip) against fp64 numpy restatements of the reference's torch.fft / kornia
chains, and the trainer / driver paths that apply them."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_NOISE = 3.0
MAGNITUDES = (0, 1, 2, 4, 8, 16, 32)                       # multiscale_cifar.py
IMAGENET_MAGNITUDES = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256)  # multiscale_imagenet.py
# 224^2: the ImageNet list, plus 100 (r = 24: the far end of the branches that 64 enters, lpf direct / hpf complement)
MAGNITUDES_224 = IMAGENET_MAGNITUDES + (100,)


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float32)


def test_224_magnitudes_reach_every_rank_limited_branch():
    """G = c I + s U U^H at 224^2: every (op, kept set / complement) pair runs with r > 0 under MAGNITUDES_224, so the GEMM chain
    is exercised with the c s terms both zero and non-zero for both ops"""
    from eoe_amd.msm import host_operator
    seen = {}
    for op in ("lpf", "hpf"):
        for mag in MAGNITUDES_224:
            if mag <= 0:
                continue
            u, (c, s) = host_operator(op, 224, mag, True)
            assert (c, s) in ((0.0, 1.0), (1.0, -1.0))
            if u.shape[1] > 0:
                seen.setdefault((op, c), []).append((mag, u.shape[1]))
    print("224^2 branches with r > 0 (op, c): [(magnitude, r)]:", seen)
    assert set(seen) == {("lpf", 0.0), ("lpf", 1.0), ("hpf", 0.0), ("hpf", 1.0)}, seen
    assert (64, 96) in seen[("lpf", 0.0)] and (64, 96) in seen[("hpf", 1.0)]


@pytest.mark.parametrize("shape", [(256, 3, 32, 32), (8, 1, 28, 28), (16, 3, 224, 224)])
@pytest.mark.parametrize("op", ["lpf", "hpf"])
def test_fft_filters_match_fp64(shape, op):
    from eoe_amd.msm import fft_filter_np, msm_filter, torch_fft_filter
    x = _images(shape, 11 + shape[-1])
    xd = x.cuda()
    x_before = xd.clone()
    x64 = x.double().numpy()
    for mag in (MAGNITUDES_224 if shape[-1] == 224 else MAGNITUDES):
        got = msm_filter(xd, op, mag).cpu().numpy()
        if mag == 0:
            assert np.array_equal(got.view(np.uint32), x.numpy().view(np.uint32)), "magnitude 0 is a bit copy"
            continue
        want = fft_filter_np(x64, op, mag)
        ref32 = torch_fft_filter(x, op, mag).double().numpy()           # the reference's own fp32 chain (torch CPU fft)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(ref32), nan), (op, mag)
        if nan.all():
            print(f"{op} {shape} magnitude {mag}: all NaN, as the reference")
            continue
        # a fully zeroed spectrum is per image: rows are either all NaN or all finite
        assert not (nan.reshape(shape[0], -1).any(1) & ~nan.reshape(shape[0], -1).all(1)).any()
        dist = np.abs(ref32[~nan] - want[~nan]).max()
        err = np.abs(got[~nan].astype(np.float64) - want[~nan]).max()
        bar = max(K_NOISE * dist, 1e-6)
        print(f"{op} {shape} magnitude {mag}: max err {err:.3e}, dist32 {dist:.3e}, bar {bar:.3e}")
        assert err <= bar, (op, mag, err, dist)
    assert torch.equal(xd, x_before), "the input is not modified"


def test_fully_zeroed_spectrum_gives_nan_rows():
    from eoe_amd.msm import msm_filter
    x = _images((4, 3, 32, 32), 3).cuda()
    for op, mag in (("lpf", 16), ("lpf", 32), ("hpf", 16)):
        assert torch.isnan(msm_filter(x, op, mag)).all(), (op, mag)
    x = _images((2, 3, 224, 224), 4).cuda()
    for op, mag in (("lpf", 112), ("hpf", 256)):
        assert torch.isnan(msm_filter(x, op, mag)).all(), (op, mag)


def _check_row_selection(shape, op, mag):
    from eoe_amd.msm import msm_filter
    x = _images(shape, 7).cuda()
    x_before = x.clone()
    rows = torch.arange(shape[0], device="cuda") % 3 == 1
    full = msm_filter(x, op, mag)
    part = msm_filter(x, op, mag, rows)
    assert torch.equal(x, x_before)
    assert torch.equal(part[~rows].view(torch.int32), x[~rows].view(torch.int32))
    assert torch.equal(part[rows].view(torch.int32), full[rows].view(torch.int32))


@pytest.mark.parametrize("shape", [(64, 3, 32, 32), (8, 1, 28, 28), (6, 3, 224, 224)])
@pytest.mark.parametrize("op", ["lpf", "hpf", "blur"])
def test_row_selection_copies_unselected_rows_bitwise(shape, op):
    _check_row_selection(shape, op, 4)


@pytest.mark.parametrize("op", ["lpf", "hpf", "blur"])
def test_row_selection_at_224_magnitude_64(op):
    """magnitude 64 at 224^2: lpf on the kept set and hpf on the complement (r = 96), blur with 65 taps"""
    _check_row_selection((6, 3, 224, 224), op, 64)


@pytest.mark.parametrize("shape", [(32, 3, 32, 32), (8, 1, 28, 28), (4, 3, 224, 224)])
def test_blur_matches_restatement(shape):
    from eoe_amd.msm import blur_np, blur_taps_k, msm_filter
    x = _images(shape, 5)
    xd = x.cuda()
    for sigma in (1, 2, 4, 8, 16, 32, 64, 128, 256):     # k up to 223 at 224^2; capped at 31 / 27 at 32^2 / 28^2
        got = msm_filter(xd, "blur", sigma).cpu().numpy()
        want = blur_np(x.numpy(), sigma)
        err = np.abs(got - want).max()
        print(f"blur {shape} sigma {sigma} k {blur_taps_k(sigma, shape[-1])}: max err {err:.3e}")
        assert err <= 1e-5, (shape, sigma)
    assert torch.equal(msm_filter(xd, "blur", 0), xd)


@pytest.mark.parametrize("op", ["lpf", "hpf", "blur"])
def test_apply_msms_test_anomalous_at_imagenet_magnitudes(op):
    """`<op>+test_anomalous` on a labelled 224^2 test batch at the ImageNet driver's 64 and 256 (lpf / hpf 256: NaN rows, as the
    reference): the anomalous rows are msm_filter of those rows bit for bit, the nominal rows bit copies"""
    from eoe_amd.msm import MSM, apply_msms, msm_filter
    x = _images((8, 3, 224, 224), 21).cuda()
    x_before = x.clone()
    lbls = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    anom = (lbls != 0).cuda()
    for mag in (64, 256):
        out = apply_msms(x, lbls, [MSM.load(f"{op}+test_anomalous--M{mag}")], "test", 0)
        assert out is not x
        want = msm_filter(x[anom], op, mag)
        assert torch.equal(out[anom].view(torch.int32), want.view(torch.int32)), (op, mag)
        assert torch.equal(out[~anom].view(torch.int32), x[~anom].view(torch.int32)), (op, mag)
    assert torch.equal(x, x_before)


# --------------------------------------------------------------------------------------------------------------- trainer
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


def _resident(seed=0, n=64, n_oe=64, n_test=32):
    from eoe_amd.data import ResidentImageSource
    g = torch.Generator().manual_seed(100 + seed)
    mk = lambda k: torch.randint(0, 256, (k, 32, 32, 3), generator=g, dtype=torch.uint8)
    normal, oe, test = mk(n), mk(n_oe), mk(n_test)
    ty = torch.tensor([0, 1] * (n_test // 2))
    return lambda: ResidentImageSource(normal, oe, test, ty, crop=32, padding=4, mean=[0.4, 0.45, 0.5], std=[0.25, 0.2, 0.3], seed=seed)


def test_cnn32_hsc_resident_source_with_train_msms_matches_fft_fed_batches():
    import eoe_amd
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM, torch_fft_filter
    from eoe_amd.training import HSCTrainer
    make = _resident(seed=3)
    msms = [MSM.load("lpf+train_nominal--M4"), MSM.load("lpf+train_oe--M4")]
    torch.manual_seed(0)
    m0 = CNN32(bias=True)
    # the same raw [0, 1] batches, filtered by the reference's torch.fft chain, Normalize left to the encoder
    raw = make()
    raw.defer_normalize(True)
    tr_batches, te_batches = raw.loaders(64)
    tr_batches = [(torch_fft_filter(b[0].cuda(), "lpf", 4), b[1], b[2]) for b in tr_batches]
    want_src = ListSource(tr_batches, te_batches, normalize=raw.normalize)
    out = {}
    for name, src, ms in (("hip", make(), msms), ("fft", want_src, ())):
        tr = HSCTrainer(copy.deepcopy(m0), dataset=src, epochs=1, lr=1e-3, batch_size=64, msms=ms, logger=_RecordingLogger())
        tr.train_cls(copy.deepcopy(m0), src, 0, "0", 0)
        out[name] = (tr.last_losses[0], torch.cat([s for _, s in tr.last_scores]).cpu())
    assert abs(out["hip"][0] - out["fft"][0]) <= 1e-4 * max(1.0, abs(out["fft"][0])), out
    assert (out["hip"][1] - out["fft"][1]).abs().max() <= 1e-4 * max(1.0, out["fft"][1].abs().max().item())


def test_test_only_msms_leave_training_bitwise_and_change_eval_scores():
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM
    from eoe_amd.training import HSCTrainer
    make = _resident(seed=5)
    torch.manual_seed(1)
    m0 = CNN32(bias=True)
    res = {}
    for mag in (0, 4):
        msms = [MSM("lpf", "test_anomalous", mag), MSM("blur", "test_nominal", mag)]
        log = _RecordingLogger()
        src = make()
        tr = HSCTrainer(copy.deepcopy(m0), dataset=src, epochs=1, lr=1e-3, batch_size=32, msms=msms, logger=log)
        model, _ = tr.train_cls(copy.deepcopy(m0), src, 0, "0", 0)
        tr.eval_cls(model, src, 0, "0", 0)
        res[mag] = (list(tr.last_losses), log.json["eval_cls0_it0_anomaly_scores"])
    assert res[0][0] == res[4][0]                                   # bitwise: the CNN32 step is reproducible
    s0, s4 = np.array(list(res[0][1].values())), np.array(list(res[4][1].values()))
    assert np.isfinite(s4).all() and np.abs(s0 - s4).max() > 0


def test_vit_step_with_lpf_matches_fft_fed_loss():
    import eoe_amd
    from eoe_amd.data import ListSource
    from eoe_amd.models import ClipViTB32Custom
    from eoe_amd.msm import MSM, torch_fft_filter
    from eoe_amd.training import HSCTrainer
    old = eoe_amd.compute_dtype()
    try:
        eoe_amd.set_compute_dtype("fp16")
        x = _images((16, 3, 224, 224), 9)
        y = torch.tensor([0] * 8 + [1] * 8)
        torch.manual_seed(2)
        m0 = ClipViTB32Custom()
        xf = x.clone()
        xf[:8] = torch_fft_filter(x[:8].cuda(), "lpf", 8).cpu()
        losses = {}
        for name, batch, ms in (("hip", x, [MSM.load("lpf+train_nominal--M8")]), ("fft", xf, ())):
            src = ListSource([(batch, y, torch.arange(16))], normalize=([0.48, 0.46, 0.41], [0.27, 0.26, 0.28]))
            tr = HSCTrainer(copy.deepcopy(m0), dataset=src, epochs=1, lr=1e-4, batch_size=16, msms=ms, logger=_RecordingLogger())
            tr.train_cls(copy.deepcopy(m0), src, 0, "0", 0)
            losses[name] = tr.last_losses[0]
    finally:
        eoe_amd.set_compute_dtype(old)
    assert np.isfinite(losses["hip"]) and abs(losses["hip"] - losses["fft"]) <= 1e-3 * max(1.0, abs(losses["fft"])), losses


def test_multiscale_experiment_test_only_trains_once():
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM
    from eoe_amd.training import HSCTrainer, ADTrainer, multiscale_experiment
    make = _resident(seed=7, n=32, n_oe=32, n_test=32)
    trained = {}
    torch.manual_seed(3)
    m0 = CNN32(bias=True)

    def make_trainer(msms, magnitude):
        tr = HSCTrainer(copy.deepcopy(m0), dataset=make(), epochs=1, lr=1e-3, batch_size=16, msms=msms, logger=_RecordingLogger())
        orig = tr.train_cls

        def train_cls(*a, **k):
            out = orig(*a, **k)
            trained[magnitude] = len(tr.last_losses)
            return out
        tr.train_cls = train_cls
        return tr

    res = multiscale_experiment(make_trainer, [MSM.load("lpf+test_anomalous")], magnitudes=(0, 2, 4))
    assert ADTrainer.KEEP_SNAPSHOT_IN_RAM is False
    assert set(res) == {"magnitudes", "aucs", "stds", "ms_mode"} and res["magnitudes"] == [0, 2, 4]
    assert len(res["aucs"]) == 3 and len(res["stds"]) == 3 and all(np.isfinite(res["aucs"]))
    assert trained == {0: 2, 2: 0, 4: 0}, trained
    assert res["ms_mode"] == ["lpf+test_anomalous--M4"]
