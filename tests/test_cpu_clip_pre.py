"""CPU tier: CLIP's preprocessing inside the train chain (eoe_augment_resize_batch, eoe_amd.data.augment_resize_batch,
ResidentImageSource(clip_preprocessing=)) -- the oracle chain of tests/clip_pre_util.py against the Pillow fixture g24, today's
Pillow against the fixture, the entry point's declaration and argument refusals, and the host-side refusals of the source (no
kernel runs in this file)."""
import numpy as np
import pytest
import torch

import clip_pre_util as cu
from oracle import augment as oaug


@pytest.mark.parametrize("case", list(cu.FIXTURE_CASES))
def test_oracle_chain_equals_the_pillow_fixture(golden, case):
    g = golden("g24_clip_pre")
    n, S, C, P, filt = cu.FIXTURE_CASES[case]
    crops = cu.fixture_crops(case)
    assert crops.shape == (n, S, S, C) and g[case].shape == (n, P, P, 3) and g[case].dtype == np.uint8
    assert np.array_equal(cu.oracle_resized(crops, P, filt), g[case])
    if C == 1:                                                           # convert("RGB") of an L image: the byte, three times
        assert np.array_equal(g[case][..., 0], g[case][..., 1]) and np.array_equal(g[case][..., 0], g[case][..., 2])
    if S == P:                                                           # the taps round to the identity
        assert np.array_equal(g[case], crops if C == 3 else np.repeat(crops, 3, axis=3))
    # the whole chain with an identity crop is the same thing: the crop stage of the oracle hands the bytes through
    p = np.zeros((n, 4), dtype=np.int32)
    p[:, 0] = np.arange(n)
    assert np.array_equal(cu.oracle_bytes(crops, p, S, P, True, filt), g[case])


def test_todays_pillow_reproduces_the_fixture(golden):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    g = golden("g24_clip_pre")
    if PIL.__version__.split(".")[0] != str(g["pillow_version"]).split(".")[0]:
        pytest.skip(f"fixture made with Pillow {g['pillow_version']}, this is {PIL.__version__}")
    for case, (n, S, C, P, filt) in cu.FIXTURE_CASES.items():
        for crop, want in zip(cu.fixture_crops(case), g[case]):
            im = Image.fromarray(crop[..., 0], mode="L") if C == 1 else Image.fromarray(crop, mode="RGB")
            got = im.resize((P, P), Image.BICUBIC if filt == "bicubic" else Image.BILINEAR).convert("RGB")
            assert np.array_equal(np.asarray(got), want), case


def test_oracle_chain_pads_and_flips_in_front_of_the_filter():
    """the reference inputs of the GPU tier: padded zeros reach the filter, the two flip orders differ, and the fp32 tail is
    oracle.augment.augment_batch's (checked where both exist: S = P, where the resize is the identity)"""
    src = cu.images("odd", 5, 17, 20, 3)
    p = cu.params("odd", 6, 5, 17, 20, 9, 3)
    assert p[:4, 1].tolist() == [-3, -3, 11, 11] and p[:4, 2].tolist() == [-3, 14, -3, 14]
    a, b = cu.oracle_bytes(src, p, 9, 23, True), cu.oracle_bytes(src, p, 9, 23, False)
    assert a.shape == (6, 23, 23, 3) and not np.array_equal(a[p[:, 3] == 1], b[p[:, 3] == 1])
    assert np.array_equal(a[p[:, 3] == 0], b[p[:, 3] == 0])
    assert (cu.oracle_crops(src, p, 9, True)[0, :3, :3] == 0).all() and (a[0, 0, 0] == 0).all()      # the padded corner
    same = cu.oracle_bytes(src, p, 9, 9, True)
    want = oaug.augment_batch(src, p, 9, 9, cu.CLIP_MEAN, cu.CLIP_STD, True, 0.001, 5)
    assert np.array_equal(cu.oracle_f32(same, cu.CLIP_MEAN, cu.CLIP_STD, 0.001, 5), want)


def test_entry_point_is_declared_exported_and_checks_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    name = "eoe_augment_resize_batch"
    assert name in _lib.header_symbols() and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5                    # additive: the ABI version does not move
    bic, lin = _lib.EOE_RESIZE_BICUBIC, _lib.EOE_RESIZE_BILINEAR

    # (src, n_src, Hs, Ws, C, params, crop_h, crop_w, n_px, filter, bounds, kk, mean, std, out, n, flip_first, noise_std, seed, stream);
    # the pointers are never followed: every call below is refused before a launch
    def call(src=16, n_src=4, Hs=32, Ws=32, C=3, params=32, crop_h=32, crop_w=32, n_px=224, filt=bic, bounds=48, kk=64, mean=None,
             std=None, out=128, n=4, seed=0, noise=0.0):
        return lib.eoe_augment_resize_batch(src, n_src, Hs, Ws, C, params, crop_h, crop_w, n_px, filt, bounds, kk, mean, std, out, n, 1,
                                            noise, seed, None)

    assert call(C=2) == 1 and b"C must be 1 or 3, not 2" in lib.eoe_last_error()
    for kw in (dict(src=None), dict(params=None), dict(bounds=None), dict(kk=None), dict(out=None), dict(n=0), dict(n_src=0), dict(Hs=0)):
        assert call(**kw) == 1, kw
    assert call(crop_h=65, crop_w=65) == 1 and b"crop <= 64" in lib.eoe_last_error()              # S > 64
    assert call(n_px=257) == 1 and b"n_px <= 256" in lib.eoe_last_error()                         # P > 256
    assert call(crop_h=32, crop_w=32, n_px=31) == 1 and b"downscale" in lib.eoe_last_error()      # P < S
    assert call(filt=0) == 1 and b"filter" in lib.eoe_last_error()                                # nearest
    assert call(filt=1) == 1 and call(filt=4) == 1                                                # lanczos, box
    assert call(crop_h=32, crop_w=28) == 1 and b"square" in lib.eoe_last_error()
    assert call(n=1 << 22) == 1 and b"2^22" in lib.eoe_last_error()
    assert call(seed=1 << 24) == 1
    assert call(noise=-1.0) == 1
    assert call(mean=48) == 1 and b"both" in lib.eoe_last_error()
    # 3 * P * P >= 2^18 needs P >= 296, which the P <= 256 limit refuses first; both limits are stated
    assert call(n_px=296) == 1
    assert call(filt=lin, crop_h=65, crop_w=65) == 1


def _u8(n, hw, ch=3):
    return torch.from_numpy(cu.images(f"host{hw}x{ch}", n, hw, hw, ch))


def test_source_option_on_the_host():
    """clip_preprocessing= as far as no kernel is involved: defaults, refusals, unchanged draws"""
    from eoe_amd import data
    lab = torch.zeros(4, dtype=torch.int64)
    kw = dict(crop=32, padding=4, device="cpu")
    src = data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=224, **kw)
    assert src.clip_preprocessing == 224 and tuple(src.mean) == data.CLIP_MEAN and tuple(src.std) == data.CLIP_STD
    assert src.normalize is None
    src.defer_normalize(True)
    assert src.normalize == (data.CLIP_MEAN, data.CLIP_STD) and src._norm_args() == (None, None)
    own = data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=224, mean=[.5] * 3, std=[.25] * 3, **kw)
    assert own.mean == [.5] * 3
    off = data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, **kw)
    assert off.clip_preprocessing is None and off.mean is None
    # the draws and their order are those of the source without the option
    a = data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=224, seed=7, **kw)
    b = data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, seed=7, **kw)
    assert torch.equal(a._params(torch.arange(5), 32, 32), b._params(torch.arange(5), 32, 32))
    # where the stage has work: everywhere but on 3 channels that are n_px wide already
    assert a._clip_px(32, 3) == 224 and a._clip_px(224, 3) is None and a._clip_px(224, 1) == 224 and b._clip_px(32, 3) is None
    with pytest.raises(ValueError, match="normalize="):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=224, normalize="normalize", **kw)
    with pytest.raises(ValueError, match="normalize="):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=224,
                                 ds_statistics={"mean": [0.] * 3, "std": [1.] * 3, "mode": 0}, **kw)
    with pytest.raises(ValueError, match="square crop"):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, crop=(32, 28), device="cpu", clip_preprocessing=224)
    with pytest.raises(ValueError, match="square test images"):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), torch.zeros((4, 32, 30, 3), dtype=torch.uint8), lab, clip_preprocessing=224, **kw)
    with pytest.raises(NotImplementedError, match="upsampling"):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=24, **kw)
    with pytest.raises(NotImplementedError, match="at most 64 px"):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 72), lab, clip_preprocessing=224, **kw)
    with pytest.raises(NotImplementedError, match="at most 256 px"):
        data.ResidentImageSource(_u8(8, 32), _u8(6, 32), _u8(4, 32), lab, clip_preprocessing=288, **kw)
    # a claimed pre-tensor sharpen MSM is out of scope together with the option; the other MSMs are not claimed, as before
    from eoe_amd.msm import MSM
    with pytest.raises(NotImplementedError, match="sharpen"):
        a.pre_tensor_msms([MSM.load("sharpen+train_nominal--M4")])
    assert a.pre_tensor_msms([MSM.load("lpf+train_nominal--M4")]) == []
    assert len(b.pre_tensor_msms([MSM.load("sharpen+train_nominal--M4")])) == 1
    # the labelled set hands the option to its tasks
    lset = data.LabelledImageSet(_u8(8, 32), torch.zeros(8), _u8(4, 32), lab, _u8(6, 32), ["a"], 32, device="cpu", padding=4,
                                 clip_preprocessing=224)
    task = lset.source([0], seed=1)
    assert task.clip_preprocessing == 224 and tuple(task.mean) == data.CLIP_MEAN
    with pytest.raises(ValueError, match="normalize="):
        data.LabelledImageSet(_u8(8, 32), torch.zeros(8), _u8(4, 32), lab, _u8(6, 32), ["a"], 32, device="cpu", normalize="normalize",
                              clip_preprocessing=224).source([0])


def test_wrapper_refuses_on_the_host():
    from eoe_amd import data

    class FakeCuda(torch.Tensor):                        # passes the wrapper's device check; nothing is launched before the refusal
        is_cuda = True

    three = torch.zeros((2, 8, 8, 3), dtype=torch.uint8).as_subclass(FakeCuda)
    p = torch.zeros((2, 4), dtype=torch.int32).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="GPU"):
        data.augment_resize_batch(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 4), dtype=torch.int32), 8, 16)
    with pytest.raises(ValueError, match="not 2"):
        data.augment_resize_batch(torch.zeros((2, 8, 8, 2), dtype=torch.uint8).as_subclass(FakeCuda), p, 8, 16)
    with pytest.raises(ValueError, match="square"):
        data.augment_resize_batch(three, p, (8, 6), 16)
    with pytest.raises(ValueError, match="upsample"):
        data.augment_resize_batch(three, p, 8, 6)
    with pytest.raises(ValueError, match="interpolation"):
        data.augment_resize_batch(three, p, 8, 16, interpolation="nearest")
    with pytest.raises(ValueError, match="three values"):
        data.augment_resize_batch(three, p, 8, 16, mean=[0.5], std=[0.5])
