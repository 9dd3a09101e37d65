"""CPU tier: the sharpen multi-scale mode -- the numpy restatement of Pillow's UnsharpMask against Pillow itself and the g18
fixture (the reference's own PilUnsharpMask), argument validation of the new entry points, trainer construction, routing and the
resident source's claim of the train sharpen MSMs."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _g18_inputs():
    spec = importlib.util.spec_from_file_location("make_golden_sharpen", os.path.join(GOLDEN_DIR, "make_golden_sharpen.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_box_constants_of_the_default_radius():
    from eoe_amd.msm import sharpen_box
    assert sharpen_box(2.0) == (1, 4473924, 1677722)
    assert sharpen_box(0.0) == (0, 1 << 24, 0)


@pytest.mark.parametrize("hw", [(3, 3), (5, 7), (28, 28), (32, 32), (40, 37), (224, 224)])
def test_unsharp_np_equals_pillow(hw):
    Image = pytest.importorskip("PIL.Image")
    ImageFilter = pytest.importorskip("PIL.ImageFilter")
    from eoe_amd.msm import unsharp_np
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    big = hw == (224, 224)
    for mode in ("L", "RGB"):
        x = rng.integers(0, 256, (*hw, 3 if mode == "RGB" else 1), dtype=np.uint8)
        x[: hw[0] // 2, : hw[1] // 2] = 90 + (x[: hw[0] // 2, : hw[1] // 2] % 5)      # a patch under the threshold
        im = Image.fromarray(x if mode == "RGB" else x[..., 0], mode)
        for percent in ((0, 150, 3200) if big else (0, 50, 100, 150, 400, 800, 1600, 3200)):
            for radius in ((2.0,) if big else (0.5, 1.0, 2.0, 3.3, 10.0)):
                for threshold in (0, 3, 10):
                    want = np.asarray(im.filter(ImageFilter.UnsharpMask(radius, percent, threshold))).reshape(x.shape)
                    got = unsharp_np(x[None], percent, radius, threshold)[0]
                    assert np.array_equal(got, want), (hw, mode, percent, radius, threshold)


def test_unsharp_np_equals_golden(golden):
    from eoe_amd.msm import sharpen_percent, unsharp_np
    g = golden("g18_sharpen")
    gen = _g18_inputs()
    assert np.array_equal(gen.images("rgb224")[:, ::gen.GRID, ::gen.GRID], g["in_grid/224"])
    n = 0
    for case, (h, w, c, k, mags) in gen.CASES.items():
        x = gen.images(case)
        if case != "rgb224":
            assert np.array_equal(x, g[f"in/{case}"])
        for mag in mags:
            got = unsharp_np(x, sharpen_percent(mag))
            if case == "rgb224":
                got = got[:, ::gen.GRID, ::gen.GRID]
            assert np.array_equal(got, g[f"out/{case}/{mag}"]), (case, mag)
            n += 1
    assert n == 6 * 7
    assert np.array_equal(g["out/rgb32/0"], g["in/rgb32"]) and not np.array_equal(g["out/rgb32/4"], g["in/rgb32"])


def test_sharpen_entry_points_validate_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    u8 = lib.eoe_msm_sharpen_u8
    assert u8(None, None, None, 4, 32, 32, 3, 2.0, 100, 3, None) == 1
    assert u8(16, 16, None, 4, 32, 32, 3, 2.0, 100, 3, None) == 1 and b"aliased" in lib.eoe_last_error()
    assert u8(16, 32, None, 4, 32, 32, 2, 2.0, 100, 3, None) == 1 and b"C must be 1 or 3" in lib.eoe_last_error()
    assert u8(16, 32, None, 4, 32, 32, 3, 2.0, -1, 3, None) == 1 and b"percent" in lib.eoe_last_error()
    assert u8(16, 32, None, 4, 32, 32, 3, -0.5, 100, 3, None) == 1 and b"radius" in lib.eoe_last_error()
    assert u8(16, 32, None, 4, 32, 32, 3, float("nan"), 100, 3, None) == 1
    assert u8(16, 32, None, 0, 32, 32, 3, 2.0, 100, 3, None) == 1
    assert u8(16, 32, None, 4, 0, 32, 3, 2.0, 100, 3, None) == 1
    assert u8(16, 32, None, 4, 512, 512, 3, 2.0, 100, 3, None) == 1 and b"65536" in lib.eoe_last_error()
    f32 = lib.eoe_msm_sharpen_f32
    assert f32(None, 32, None, 4, 3, 32, 32, 2.0, 100, 3, None) == 1
    assert f32(16, 32, None, 4, 4, 32, 32, 2.0, 100, 3, None) == 1 and b"C must be 1 or 3" in lib.eoe_last_error()
    assert f32(16, 32, None, 4, 3, 32, 32, 2.0, -100, 3, None) == 1 and b"percent" in lib.eoe_last_error()
    cf = lib.eoe_crop_flip_u8
    assert cf(None, 4, 32, 32, 64, 128, 4, 32, 32, 1, None) == 1
    assert cf(16, 4, 32, 32, None, 128, 4, 32, 32, 1, None) == 1
    assert cf(16, 4, 32, 32, 64, 128, 0, 32, 32, 1, None) == 1
    assert cf(16, 4, 32, 32, 64, 16, 4, 32, 32, 1, None) == 1 and b"alias" in lib.eoe_last_error()


def test_python_wrappers_refuse_cpu_tensors_and_msm_filter_points_to_msm_sharpen():
    from eoe_amd.data import crop_flip_u8
    from eoe_amd.msm import msm_filter, msm_sharpen, sharpen_u8
    with pytest.raises(RuntimeError):
        msm_sharpen(torch.zeros((1, 3, 32, 32)), 4)
    with pytest.raises(RuntimeError):
        sharpen_u8(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), 400)
    with pytest.raises(RuntimeError):
        crop_flip_u8(torch.zeros((1, 32, 32, 3), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int32), (32, 32))
    with pytest.raises(ValueError, match="msm_sharpen"):
        msm_filter(torch.zeros((1, 3, 32, 32)), "sharpen", 4)


def test_gpu_trainer_accepts_sharpen_and_cpu_trainer_refuses_it():
    from eoe_amd.msm import MSM
    from eoe_amd.training import HSCTrainer
    model = torch.nn.Linear(2, 2)
    tr = HSCTrainer(model, dataset=None, msms=[MSM.load("sharpen+train_nominal--M4")], device="cuda")
    assert [str(m) for m in tr.msms] == ["sharpen+train_nominal--M4"]
    HSCTrainer(model, msms=[MSM.load("sharpen+test_anomalous--M2"), MSM.load("lpf+train_oe--M1")], device="cuda:0")
    with pytest.raises(NotImplementedError, match="sharpen"):
        HSCTrainer(model, msms=[MSM.load("sharpen+train_oe--M4")], device="cpu")
    HSCTrainer(model, msms=[MSM.load("blur+train_oe--M4")], device="cpu")


def test_sharpen_routing_follows_the_reference(monkeypatch):
    from eoe_amd import msm
    msms = [msm.MSM("sharpen", "train_nominal", 4), msm.MSM("lpf", "train_oe", 2), msm.MSM("sharpen", "train_oe", 1),
            msm.MSM("sharpen", "test_nominal", 8), msm.MSM("sharpen", "test_anomalous", 3)]
    assert msm.routing(msms, "train") == [("sharpen", 4, True, False), ("lpf", 2, False, True), ("sharpen", 1, False, True)]
    assert msm.routing(msms, "test") == [("sharpen", 8, True, False), ("sharpen", 3, False, True)]
    calls = []

    def fake_sharpen(x, mag, rows=None):
        calls.append(("sharpen", mag, None if rows is None else rows.tolist()))
        return x + 1

    def fake_filter(x, op, mag, rows=None):
        calls.append((op, mag, None if rows is None else rows.tolist()))
        return x + 1

    monkeypatch.setattr(msm, "msm_sharpen", fake_sharpen)
    monkeypatch.setattr(msm, "msm_filter", fake_filter)
    monkeypatch.setattr(msm, "check_supported", lambda m, device=None: None)     # the batch stays on the CPU here
    imgs, lbls = torch.zeros((4, 3, 2, 2)), torch.tensor([0, 0, 1, 1])
    msm.apply_msms(imgs, lbls, msms, "train", 0)
    assert calls == [("sharpen", 4, [True, True, False, False]), ("lpf", 2, [False, False, True, True]),
                     ("sharpen", 1, [False, False, True, True])]
    calls.clear()
    msm.apply_msms(imgs, torch.tensor([1, 0, 1, 0]), msms, "test", 0)
    assert calls == [("sharpen", 8, [False, True, False, True]), ("sharpen", 3, [True, False, True, False])]
    assert msm.sharpen_percent(4) == 400 and msm.sharpen_percent(0) == 0


def test_resident_source_claims_train_sharpen_and_trainer_skips_it():
    from eoe_amd.data import ListSource, ResidentImageSource
    from eoe_amd.msm import MSM
    from eoe_amd.training import HSCTrainer
    u8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    src = ResidentImageSource(u8, u8, u8, torch.tensor([0, 1, 0, 1]), crop=8, device="cpu")
    msms = [MSM("sharpen", "train_nominal", 4), MSM("lpf", "train_nominal", 2), MSM("sharpen", "train_oe", 1),
            MSM("sharpen", "test_nominal", 8)]
    claimed = src.pre_tensor_msms(msms)
    assert claimed[0] is msms[0] and claimed[1] is msms[2] and len(claimed) == 2
    tr = HSCTrainer(torch.nn.Linear(2, 2), msms=msms, device="cuda")
    tr._msm_source(src)
    assert tr._step_msms == [msms[1], msms[3]]
    tr._msm_source(ListSource([]))                   # a source without the hook claims nothing
    assert tr._step_msms == msms
    plain = HSCTrainer(torch.nn.Linear(2, 2), device="cuda")
    plain._msm_source(src)                           # a trainer without MSMs clears an earlier claim on a shared source
    assert plain._step_msms == [] and src._pre_msms == []


def test_header_declares_the_sharpen_entry_points_in_plain_c():
    import shutil
    import subprocess
    hdr = os.path.join(os.path.dirname(GOLDEN_DIR), "..", "include", "eoe_hip.h")
    text = open(hdr).read()
    for name in ("eoe_msm_sharpen_u8", "eoe_msm_sharpen_f32", "eoe_crop_flip_u8"):
        assert f"int {name}(" in text
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    r = subprocess.run([gcc, "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", hdr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
