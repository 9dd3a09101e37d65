"""CPU tier: the 1-channel input path (Grayscale(1) and the one-channel crop / flip / augment) -- the g22 fixture against the integer
formula, today's Pillow and the oracle's crop / flip rule; the new entry points' declarations and argument checks; the noise rule
with one channel; the host-side options of the resident source (no kernel runs in this file)."""
import numpy as np
import pytest
import torch

import gray_util as gu
from oracle import augment as oaug
from oracle.fill import _splitmix64


def test_fixture_l_equals_the_integer_formula(golden):
    g = golden("g22_gray")
    colour = gu.colour_set()
    assert g["L"].shape == (gu.N_IMG, 32, 32) and g["L"].dtype == np.uint8
    assert np.array_equal(g["L"], gu.gray_formula(colour))
    assert g["L"][0].ravel()[:5].tolist() == [255, 0, 76, 150, 29]                 # white, black, red, green, blue
    # image 1: sums on k * 65536 - 0x8000 + {-1, 0, 1}: one below the boundary gives k - 1, on it and above it k
    bp = gu.boundary_pixels()
    sums = (bp.astype(np.int64) * np.asarray(gu.L_WEIGHTS)).sum(1)
    d = (sums + 0x8000 + 1) % 65536 - 1
    assert set(d.tolist()) == {-1, 0, 1} and len(bp) >= 48
    k = (sums + 0x8000 - d) // 65536
    assert np.array_equal(g["L"][1].ravel()[:len(bp)], np.where(d < 0, k - 1, k))
    # a rounding to nearest of the real-valued weights would differ somewhere on these pixels only if the formula were another one:
    # truncation without the 0x8000 differs on every d >= 0 pixel
    assert (((sums >> 16) != g["L"][1].ravel()[:len(bp)])[d >= 0]).all()


def test_todays_pillow_reproduces_the_fixture(golden):
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageOps
    g = golden("g22_gray")
    if PIL.__version__.split(".")[0] != str(g["pillow_version"]).split(".")[0]:
        pytest.skip(f"fixture made with Pillow {g['pillow_version']}, this is {PIL.__version__}")
    colour = gu.colour_set()
    got = np.stack([np.asarray(Image.fromarray(c, mode="RGB").convert("L")) for c in colour])
    assert np.array_equal(got, g["L"])
    name = "c32"
    (Ho, Wo), pad = gu.CROP_CASES[name][1:]
    src = gu.case_source(name, g["L"])
    for row, want in zip(g[f"{name}/rows"], g[f"{name}/ff1"]):
        i, t, l, f = (int(v) for v in row)
        im = Image.fromarray(src[i], mode="L")
        im = im.transpose(Image.FLIP_LEFT_RIGHT) if f else im
        im = ImageOps.expand(im, border=pad, fill=0).crop((l + pad, t + pad, l + pad + Wo, t + pad + Ho))
        assert np.array_equal(np.asarray(im), want)


@pytest.mark.parametrize("case", list(gu.CROP_CASES))
def test_fixture_crops_equal_the_oracle_rule(golden, case):
    """Pillow's expand + crop + transpose is the rule oracle/augment.py states (zero padding, both flip orders): the fixture's
    bytes are the oracle's plane 0 on three equal planes, times 255"""
    g = golden("g22_gray")
    (Ho, Wo), pad = gu.CROP_CASES[case][1:]
    src, rows = gu.case_source(case, g["L"]), gu.case_rows(case)
    assert np.array_equal(rows, g[f"{case}/rows"]) and rows.shape == (13, 4)
    assert set(rows[:, 1]) == {-pad, 0, src.shape[1] + pad - Ho} and set(rows[:, 2]) == {-pad, 0, src.shape[2] + pad - Wo}
    assert set(rows[:, 3]) == {0, 1} and rows[:, 0].max() < len(src)
    src3 = np.repeat(src[..., None], 3, axis=-1)
    for ff in (1, 0):
        want = oaug.augment_batch(src3, rows, Ho, Wo, None, None, bool(ff), 0.0, 0)
        assert np.array_equal(np.rint(want * 255.0).astype(np.uint8)[:, 0], g[f"{case}/ff{ff}"]), ff
        assert np.array_equal(want[:, 0], want[:, 2])
    flipped = rows[:, 3] == 1
    assert not np.array_equal(g[f"{case}/ff1"][flipped], g[f"{case}/ff0"][flipped])       # the two orders differ where they should


def test_noise_rule_with_one_channel():
    """element e of slot b draws from splitmix64(seed * 2^40 + b * 2^18 + e) whatever the channel count: with C = 1, e runs over
    [0, Ho * Wo), which are the counters of channel 0 of the 3-channel form"""
    seed, n, Ho, Wo = 5, 3, 4, 7
    three = oaug.noise(seed, n, Ho, Wo)
    e = np.arange(Ho * Wo, dtype=np.uint64)[None, :]
    b = np.arange(n, dtype=np.uint64)[:, None]
    z = _splitmix64((np.uint64(seed) << np.uint64(40)) + (b << np.uint64(18)) + e)
    u1 = ((z >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    u2 = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    one = (np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.283185307179586) * u2)).astype(np.float32).reshape(n, 1, Ho, Wo)
    assert np.array_equal(one[:, 0], three[:, 0])
    assert not np.array_equal(three[:, 0], three[:, 1])
    # so the oracle's augment_batch on three equal planes restates the 1-channel chain in its plane 0
    src = gu.tiny_set()
    rows = gu.case_rows("tiny")
    out3 = oaug.augment_batch(np.repeat(src[..., None], 3, axis=-1), rows, 4, 4, [0.3] * 3, [0.2] * 3, True, 0.001, seed)
    clean = oaug.augment_batch(np.repeat(src[..., None], 3, axis=-1), rows, 4, 4, [0.3] * 3, [0.2] * 3, True, 0.0, seed)
    want = clean[:, 0] + np.float32(0.001) * oaug.noise(seed, len(rows), 4, 4)[:, 0] / np.float32(0.2)
    assert np.abs(out3[:, 0] - want).max() < 1e-6


def test_new_entry_points_are_declared_exported_and_check_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    new = {"eoe_grayscale_u8", "eoe_augment_batch_c", "eoe_crop_flip_u8_c"}
    assert new <= set(_lib.header_symbols()) and new <= set(_lib.SIGNATURES)
    for name in new | {"eoe_augment_batch", "eoe_crop_flip_u8"}:                     # the 3-channel symbols stay
        assert getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5                    # additive: the ABI version does not move
    # eoe_grayscale_u8(src, dst, n_pixels, stream)
    assert lib.eoe_grayscale_u8(None, 32, 4, None) == 1
    assert lib.eoe_grayscale_u8(16, None, 4, None) == 1
    assert lib.eoe_grayscale_u8(16, 32, 0, None) == 1
    assert lib.eoe_grayscale_u8(16, 16, 4, None) == 1 and b"alias" in lib.eoe_last_error()
    # eoe_augment_batch_c(src, n_src, Hs, Ws, C, params, mean, std, out, n, Ho, Wo, flip_first, noise_std, seed, stream)
    assert lib.eoe_augment_batch_c(16, 4, 8, 8, 2, 32, None, None, 64, 4, 8, 8, 1, 0.0, 0, None) == 1
    assert b"C must be 1 or 3, not 2" in lib.eoe_last_error()
    assert lib.eoe_augment_batch_c(None, 4, 8, 8, 1, 32, None, None, 64, 4, 8, 8, 1, 0.0, 0, None) == 1
    assert lib.eoe_augment_batch_c(16, 4, 8, 8, 1, 32, 48, None, 64, 4, 8, 8, 1, 0.0, 0, None) == 1 and b"both" in lib.eoe_last_error()
    assert lib.eoe_augment_batch_c(16, 4, 8, 8, 1, 32, None, None, 64, 4, 8, 8, 1, 0.0, 1 << 24, None) == 1
    # eoe_crop_flip_u8_c(src, n_src, Hs, Ws, C, params, out, n, Ho, Wo, flip_first, stream)
    assert lib.eoe_crop_flip_u8_c(16, 4, 8, 8, 4, 32, 64, 4, 8, 8, 1, None) == 1 and b"C must be 1 or 3, not 4" in lib.eoe_last_error()
    assert lib.eoe_crop_flip_u8_c(16, 4, 8, 8, 1, 32, 16, 4, 8, 8, 1, None) == 1 and b"alias" in lib.eoe_last_error()
    assert lib.eoe_crop_flip_u8_c(16, 4, 8, 8, 1, 32, 64, 0, 8, 8, 1, None) == 1


def _gray(n, hw=28, dims=4):
    t = torch.from_numpy(gu.gray_set()[:n, :hw, :hw].copy())
    return t.unsqueeze(-1) if dims == 4 else t


def test_source_options_on_the_host():
    """grayscale= / flip= of the resident source, as far as no kernel is involved: shapes, refusals, the draw order"""
    from eoe_amd import data
    lab = torch.zeros(4, dtype=torch.int64)
    kw = dict(crop=28, padding=3, device="cpu")
    src = data.ResidentImageSource(_gray(8, dims=3), _gray(6), _gray(4, dims=3), lab, grayscale=True, **kw)
    assert src.normal.shape == (8, 28, 28, 1) and src.oe.shape == (6, 28, 28, 1) and src.test.shape == (4, 28, 28, 1)
    assert src.grayscale and src.flip
    with pytest.raises(ValueError, match="color_jitter"):
        data.ResidentImageSource(_gray(8), _gray(6), _gray(4), lab, grayscale=True, color_jitter=(0.01,) * 4, **kw)
    with pytest.raises(ValueError, match="color_jitter"):
        data.LabelledImageSet(_gray(8), torch.zeros(8), _gray(4), lab, _gray(6), ["a"], 28, device="cpu", grayscale=True,
                              color_jitter=(0.01,) * 4)
    with pytest.raises(ValueError, match=r"\[n, H, W\]"):
        data.ResidentImageSource(torch.zeros((8, 28, 28, 2), dtype=torch.uint8), _gray(6), _gray(4), lab, grayscale=True, **kw)
    with pytest.raises(RuntimeError, match="GPU"):                                   # a colour set needs the kernel: no host path
        data.ResidentImageSource(_gray(8), torch.zeros((6, 32, 32, 3), dtype=torch.uint8), _gray(4), lab, grayscale=True, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        data.grayscale_u8(torch.zeros((2, 4, 4, 3), dtype=torch.uint8))
    # flip=True draws top, left, flip per half, in this order, from the source's generator -- as it always did
    idx = torch.arange(5)
    a = data.ResidentImageSource(_gray(8), _gray(6), _gray(4), lab, grayscale=True, seed=7, **kw)
    g = torch.Generator().manual_seed(7)
    top, left, flip = (torch.randint(-3, 28 + 3 - 28 + 1, (5,), generator=g), torch.randint(-3, 32 + 3 - 28 + 1, (5,), generator=g),
                       torch.randint(0, 2, (5,), generator=g))
    assert torch.equal(a._params(idx, 28, 32), torch.stack([idx, top, left, flip], dim=1).to(torch.int32))
    # flip=False: zeros, and no draw is made for them
    b = data.ResidentImageSource(_gray(8), _gray(6), _gray(4), lab, grayscale=True, flip=False, seed=7, **kw)
    g = torch.Generator().manual_seed(7)
    top, left = torch.randint(-3, 4, (5,), generator=g), torch.randint(-3, 8, (5,), generator=g)
    p = b._params(idx, 28, 32)
    assert torch.equal(p, torch.stack([idx, top, left, torch.zeros(5, dtype=torch.int64)], dim=1).to(torch.int32))
    assert torch.equal(b._params(idx, 28, 28)[:, 1], torch.randint(-3, 4, (5,), generator=g).to(torch.int32))   # the next draw is a top
    # the labelled set hands both options to its tasks and keeps 1-channel sets as they are
    lset = data.LabelledImageSet(_gray(8, dims=3), torch.zeros(8), _gray(4), lab, _gray(6), ["a"], 28, device="cpu", grayscale=True,
                                 flip=False, padding=3)
    assert lset.train.shape == (8, 28, 28, 1)
    task = lset.source([0], seed=1)
    assert task.grayscale and not task.flip and task.padding == 3 and task.normal.data_ptr() == lset.train.data_ptr()
    # given one-element statistics come back as they are
    st = {"mean": [0.3], "std": [0.2], "mode": 0}
    src = data.ResidentImageSource(_gray(8), _gray(6), _gray(4), lab, grayscale=True, normalize="normalize", ds_statistics=st, **kw)
    assert src.mean == [0.3] and src.std == [0.2] and src.ds_statistics == st


def test_wrappers_name_the_channel_count():
    from eoe_amd import data

    class FakeCuda(torch.Tensor):                        # passes the wrappers' device check; nothing is launched before the refusal
        is_cuda = True

    two = torch.zeros((2, 4, 4, 2), dtype=torch.uint8).as_subclass(FakeCuda)
    p = torch.zeros((2, 4), dtype=torch.int32).as_subclass(FakeCuda)
    for call in (lambda: data.augment_batch(two, p, (4, 4)), lambda: data.crop_flip_u8(two, p, (4, 4)),
                 lambda: data.resize_u8(two, (2, 2)), lambda: data.grayscale_u8(two),
                 lambda: data.color_jitter_u8(two, torch.zeros(2), torch.ones(2, 4), torch.zeros(2, 4))):
        with pytest.raises(ValueError, match="not 2"):
            call()
    one = torch.zeros((2, 4, 4, 1), dtype=torch.uint8).as_subclass(FakeCuda)
    with pytest.raises(ValueError, match="3 channels, not 1"):
        data.color_jitter_u8(one, torch.zeros(2), torch.ones(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="3 channels, not 1"):
        data.grayscale_u8(one)
