"""CPU tier of the ragged image sets (eoe_amd.data.RaggedImageSet and what the source does with it on the host): packing, the
Resize rule, the fixture g25 against the oracle's Pillow restatement, the launch plan of the ragged Resize interpreted in numpy, the
crop-origin draws, the construction-time refusals and the entry points' argument checks.  No kernel runs in this file."""
import numpy as np
import pytest
import torch

import ragged_util as ru
from oracle import augment as oaug


def _set(C=3, device=None):
    from eoe_amd import data
    return data.RaggedImageSet(ru.images(C), device=device)


# ------------------------------------------------------------------------------------------------------------- the container
@pytest.mark.parametrize("C", [1, 3])
def test_packing_round_trip(C):
    from eoe_amd import data
    imgs = ru.images(C)
    rs = data.RaggedImageSet(imgs)
    assert len(rs) == len(imgs) and rs.channels == C and not rs.is_uniform and not rs.is_cuda
    assert rs.sizes.dtype == np.int32 and rs.sizes.tolist() == [list(s) for s in ru.SHAPES]
    assert rs.offsets.dtype == torch.int64 and rs.sizes_dev.dtype == torch.int32 and rs.arena.dtype == torch.uint8 and rs.arena.dim() == 1
    assert rs.offsets.tolist() == rs.offsets_host.tolist() and rs.sizes_dev.tolist() == rs.sizes.tolist()
    end = 0
    for i, a in enumerate(imgs):
        o = int(rs.offsets_host[i])
        assert o % 16 == 0 and end <= o < end + 16                       # every image starts at the next multiple of 16 bytes
        end = o + a.size
        assert rs[i].shape == a.shape and np.array_equal(rs[i].numpy(), a)
        assert np.array_equal(rs.arena[o:end].numpy(), a.reshape(-1))
    assert rs.arena.numel() % 16 == 0 and end <= rs.arena.numel() < end + 16
    assert np.array_equal(rs[-1].numpy(), imgs[-1])
    with pytest.raises(IndexError):
        rs[len(imgs)]
    with pytest.raises(ValueError, match="differ in size"):
        rs.as_tensor()
    assert rs.to("cpu") is rs


def test_accepted_and_refused_inputs():
    from eoe_amd import data
    two_d = data.RaggedImageSet([np.zeros((4, 5), np.uint8), torch.ones((3, 2, 1), dtype=torch.uint8)])
    assert two_d.channels == 1 and two_d[0].shape == (4, 5, 1) and two_d[1].shape == (3, 2, 1) and int(two_d[1].sum()) == 6
    strided = np.arange(6 * 8 * 3, dtype=np.uint8).reshape(6, 8, 3)[::2, ::2]                 # a view that is not contiguous
    assert np.array_equal(data.RaggedImageSet([strided])[0].numpy(), strided)
    with pytest.raises(ValueError, match="mixed channel counts"):
        data.RaggedImageSet([np.zeros((4, 5, 3), np.uint8), np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        data.RaggedImageSet([np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(ValueError, match="1 or 3 channels"):
        data.RaggedImageSet([np.zeros((4, 5, 2), np.uint8)])
    with pytest.raises(ValueError, match="at least one"):
        data.RaggedImageSet([])


@pytest.mark.parametrize("shape", [(4, 5, 7, 3), (3, 4, 4, 1), (2, 16, 16, 3)])
def test_from_tensor_is_uniform(shape):
    from eoe_amd import data
    t = torch.arange(int(np.prod(shape)), dtype=torch.int64).remainder(251).to(torch.uint8).reshape(shape)
    rs = data.RaggedImageSet.from_tensor(t)
    assert rs.is_uniform and len(rs) == shape[0] and rs.channels == shape[3]
    assert torch.equal(rs.as_tensor(), t) and torch.equal(rs[1], t[1])
    assert (rs.offsets_host % 16 == 0).all()
    listed = data.RaggedImageSet(list(t.numpy()))                                            # the same set through the constructor
    assert torch.equal(listed.arena, rs.arena) and listed.offsets_host.tolist() == rs.offsets_host.tolist()
    assert torch.equal(data.RaggedImageSet.from_tensor(t[..., 0]).as_tensor(), t[..., :1])   # [n, H, W] is [n, H, W, 1]


def test_resized_hw_known_answers():
    from eoe_amd import data
    for (H, W), want in zip(ru.SHAPES, ru.RESIZED):
        assert data.resized_hw(H, W, ru.TARGET) == want
        assert data.resized_hw(H, W, (ru.TARGET, 24)) == (16, 24)
    # the shapes the reference's sets have: ImageNet's usual 500 x 375 both ways, and the rule's truncation
    assert data.resized_hw(375, 500, 256) == (256, 341) and data.resized_hw(500, 375, 256) == (341, 256)
    assert data.resized_hw(256, 300, 256) == (256, 300) and data.resized_hw(333, 500, 256) == (256, 384)


# --------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filt", ru.FILTERS)
def test_fixture_equals_the_oracle_resize(golden, C, filt):
    g = golden("g25_ragged")
    for i, a in enumerate(ru.images(C)):
        r = g[f"r/{filt}/c{C}/{i}"]
        assert r.dtype == np.uint8 and r.shape == ru.RESIZED[i] + (C,)
        assert np.array_equal(oaug.resize(a, ru.TARGET, filt), r), i
        assert np.array_equal(oaug.resize(a, (ru.TARGET, ru.TARGET), filt), g[f"p/{filt}/c{C}/{i}"]), i
        assert np.array_equal(ru.center_crop(r, ru.TARGET), g[f"cc/{filt}/c{C}/{i}"]), i
        if ru.SHAPES[i] == ru.RESIZED[i]:                                  # Resize returns the image itself
            assert np.array_equal(r, a)


def test_fixture_jitter_equals_the_oracle(golden):
    g = golden("g25_ragged")
    seen = set()
    for k, (i, order, factors, (top, left), flip) in enumerate(ru.JITTER):
        whole = oaug.color_jitter(g[f"r/bilinear/c3/{i}"], np.asarray(factors, np.float32), order)
        assert np.array_equal(ru.crop_flip(whole, top, left, flip, ru.TARGET), g[f"jit/{k}"]), k
        seen.add(order.index(1))
    assert seen == {0, 1, 3}                                               # contrast first, in the middle, last
    assert (g["jit/1"][:2] == 0).all() and (g["jit/1"][:, :3] == 0).all() and (g["jit/2"][14:] == 0).all()    # the zero padding


def test_todays_pillow_reproduces_the_fixture(golden):
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    g = golden("g25_ragged")
    if PIL.__version__.split(".")[0] != str(g["pillow_version"]).split(".")[0]:
        pytest.skip(f"fixture made with Pillow {g['pillow_version']}, this is {PIL.__version__}")
    for filt, pf in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC)):
        for i, a in enumerate(ru.images(3)):
            got = np.asarray(Image.fromarray(a, mode="RGB").resize((ru.TARGET, ru.TARGET), pf))
            assert np.array_equal(got, g[f"p/{filt}/c3/{i}"]), (filt, i)


# ------------------------------------------------------------------------------------------------ the plan of the ragged Resize
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filt", ru.FILTERS)
@pytest.mark.parametrize("size", [ru.TARGET, (ru.TARGET, ru.TARGET), (20, 16)])
def test_resize_plan_interpreted_on_the_host(golden, C, filt, size):
    """the descriptors, offsets and the tap array that the two launches get, run by a numpy restatement of the pass kernel that
    checks every index: the result equals the fixture, so a table that would send the kernel outside an arena fails here"""
    from eoe_amd import data, _lib
    g = golden("g25_ragged")
    rs = _set(C)
    pair = not isinstance(size, int)
    taps = data._TapArena({"bilinear": _lib.EOE_RESIZE_BILINEAR, "bicubic": _lib.EOE_RESIZE_BICUBIC}[filt])
    plan = data.ragged_resize_plan(rs.sizes, C, size, taps, rs.offsets_host, pair)
    assert plan["h"] is not None and plan["v"] is not None
    tap = taps.tensor().numpy()
    pairs = {(h, w) for h, w in ru.SHAPES}
    assert len(taps.seen) <= 2 * len(pairs)                                # one table per distinct (in, out), not per image
    mid, out = np.zeros(plan["mid_bytes"], np.uint8), np.zeros(plan["out_bytes"], np.uint8)
    ru.emulate_pass(rs.arena.numpy(), mid, plan["h"][0], plan["h"][1], tap)
    ru.emulate_pass(mid, out, plan["v"][0], plan["v"][1], tap)
    for i, a in enumerate(ru.images(C)):
        h, w = plan["out_sizes"][i]
        o = int(plan["out_offsets"][i])
        got = out[o:o + h * w * C].reshape(h, w, C)
        if size == ru.TARGET:
            assert o % 16 == 0 and np.array_equal(got, g[f"r/{filt}/c{C}/{i}"]), i
        elif size == (ru.TARGET, ru.TARGET):
            assert o == i * h * w * C and np.array_equal(got, g[f"p/{filt}/c{C}/{i}"]), i
        else:
            assert np.array_equal(got, oaug.resize(a, size, filt)), i
    # identity images are copies: ksize 0 and equal axes in both descriptors of image 3 (16 x 16) under Resize(16)
    if size == ru.TARGET:
        assert plan["h"][1][3].tolist()[1:3] == [16, 16] and plan["h"][1][3, 6] == 0 and plan["v"][1][3, 6] == 0


def test_resize_plan_skips_a_pass_only_when_no_image_needs_it():
    from eoe_amd import data, _lib
    taps = data._TapArena(_lib.EOE_RESIZE_BILINEAR)
    sizes = np.array([[16, 30], [16, 16], [16, 97]], np.int32)            # heights are at the target: only a horizontal pass
    off, _ = data.RaggedImageSet.layout(sizes, 3)
    plan = data.ragged_resize_plan(sizes, 3, (16, 16), taps, off, True)
    assert plan["v"] is None and plan["h"] is not None and plan["h"][0][:, 1].tolist() == [0, 768, 1536]       # straight into the result
    none = data.ragged_resize_plan(sizes, 3, 16, data._TapArena(_lib.EOE_RESIZE_BILINEAR), off, False)
    assert none["h"] is None and none["v"] is None                        # Resize(16) leaves all three alone
    with pytest.raises(ValueError, match="would become"):
        data.ragged_resize_plan(np.array([[400, 2]], np.int32), 3, (0, 4), taps, np.zeros(1, np.int64), True)


# -------------------------------------------------------------------------------------------------------------- draws
def test_crop_origin_draws():
    from eoe_amd import data
    g = torch.Generator().manual_seed(3)
    sizes = np.array([[16, 22]] * 300 + [[44, 16]] * 300 + [[16, 16]] * 20 + [[20, 20]] * 300, np.int32)
    for pad in (0, 3):
        tl = data.ragged_crop_origins(sizes, 16, pad, g)
        assert tl.shape == (len(sizes), 2) and tl.dtype == torch.int64
        hi = torch.from_numpy(sizes.astype(np.int64)) + pad - 16
        assert (tl >= -pad).all() and (tl <= hi).all()                   # inside each image's own legal range
        land, port, exact, square = tl[:300], tl[300:600], tl[600:620], tl[620:]
        assert int(land[:, 1].min()) == -pad and int(land[:, 1].max()) == 6 + pad       # both ends of the landscape image's range
        assert int(port[:, 0].min()) == -pad and int(port[:, 0].max()) == 28 + pad
        if pad == 0:
            assert (land[:, 0] == 0).all() and (port[:, 1] == 0).all() and (exact == 0).all()
        # a square image: the tensor path's range [-pad, 20 + pad - 16], every origin of it reached on both axes
        for a in (0, 1):
            assert set(square[:, a].tolist()) == set(range(-pad, 4 + pad + 1))
    with pytest.raises(ValueError, match="smaller than the crop"):
        data.ragged_crop_origins(np.array([[15, 40]], np.int32), 16, 0, g)


def test_center_origins_are_torchvisions():
    from eoe_amd import data
    sizes = np.array([[16, 22], [17, 16], [21, 19], [44, 16], [13, 16], [12, 30]], np.int32)
    want = [[int(round((h - 16) / 2.0)) if h >= 16 else -((16 - h) // 2), int(round((w - 16) / 2.0))] for h, w in sizes.tolist()]
    assert data.center_origins(sizes, 16).tolist() == want
    assert want[1] == [0, 0] and want[2] == [2, 2] and want[0] == [0, 3] and want[4][0] == -1 and want[5][0] == -2


def _labels(n=9):
    return torch.tensor([0, 1] * n)[:n]


def test_source_draws_on_the_host():
    """the ragged halves draw per image; a tensor half draws what it always drew, also next to a ragged one"""
    from eoe_amd import data
    rs, oe = _set(3), data.RaggedImageSet(ru.oe_images(3))
    small = data.RaggedImageSet([a for a, s, r in zip(ru.images(3), ru.SHAPES, ru.RESIZED) if s == r])         # those Resize(16) leaves alone
    assert [tuple(s) for s in small.sizes.tolist()] == [(16, 16), (17, 16), (16, 97)]
    src = data.ResidentImageSource(small, small, small, _labels(3), crop=16, padding=2, device="cpu", seed=5)
    idx = torch.tensor([2, 0, 1, 2, 2, 1])
    p = src._params_ragged(idx, small.sizes)
    assert p.dtype == torch.int32 and p.shape == (6, 4) and p[:, 0].tolist() == idx.tolist()
    hw = torch.from_numpy(small.sizes.astype(np.int64))[idx]
    assert (p[:, 1] >= -2).all() and (p[:, 1] <= hw[:, 0] + 2 - 16).all() and (p[:, 2] >= -2).all() and (p[:, 2] <= hw[:, 1] + 2 - 16).all()
    assert set(p[:, 3].tolist()) <= {0, 1}
    # the order of the draws: tops, lefts, flips -- restated with the same generator
    g = torch.Generator().manual_seed(5)
    tl = data.ragged_crop_origins(small.sizes[idx.numpy()], 16, 2, g)
    flip = torch.randint(0, 2, (6,), generator=g)
    assert torch.equal(p[:, 1:3].to(torch.int64), tl) and torch.equal(p[:, 3].to(torch.int64), flip)
    noflip = data.ResidentImageSource(small, small, small, _labels(3), crop=16, padding=2, device="cpu", seed=5, flip=False)
    q = noflip._params_ragged(idx, small.sizes)
    assert torch.equal(q[:, :3], p[:, :3]) and (q[:, 3] == 0).all()
    # the tensor path is untouched: same seed, same draws with and without a ragged OE set beside it
    t = torch.zeros((8, 20, 20, 3), dtype=torch.uint8)
    a = data.ResidentImageSource(t, t, t, _labels(8), crop=16, padding=2, device="cpu", seed=9)
    b = data.ResidentImageSource(t, small, small, _labels(3), crop=16, padding=2, device="cpu", seed=9)
    c = data.ResidentImageSource(t, t, t, _labels(8), crop=16, padding=2, device="cpu", seed=9)
    first = a._draw(torch.arange(5), a.normal)
    assert torch.equal(first, b._draw(torch.arange(5), b.normal)) and torch.equal(first, c._params(torch.arange(5), 20, 20))
    assert len(rs) == 9 and len(oe) == 8


# ----------------------------------------------------------------------------------------------------------- refusals
def test_a_too_small_image_is_refused_at_construction():
    from eoe_amd import data
    rs = _set(3)                                                           # raw: image 7 is 9 x 13
    with pytest.raises(ValueError, match=r"normal image 7 of size \(9, 13\)"):
        data.ResidentImageSource(rs, rs, rs, _labels(), crop=16, device="cpu")
    ok = data.RaggedImageSet([a for a in ru.images(3) if min(a.shape[:2]) >= 16])
    with pytest.raises(ValueError, match=r"OE image 7 of size \(9, 13\)"):
        data.ResidentImageSource(ok, rs, ok, _labels(len(ok)), crop=16, device="cpu")
    with pytest.raises(ValueError, match=r"required crop size \(24, 24\) is larger than normal image 3 of size \(16, 16\)"):
        data.ResidentImageSource(ok, ok, ok, _labels(len(ok)), crop=24, padding=3, device="cpu")
    data.ResidentImageSource(ok, ok, ok, _labels(len(ok)), crop=16, device="cpu")            # fits
    data.ResidentImageSource(ok, ok, ok, _labels(len(ok)), crop=22, padding=3, device="cpu")  # fits with the padding
    lset = data.LabelledImageSet(rs, torch.zeros(9), ok, _labels(len(ok)), ok, ["a"], 16, device="cpu")
    with pytest.raises(ValueError, match="image 7"):
        lset.source([0])


def test_the_three_refusals():
    from eoe_amd import data, evolve
    ok = data.RaggedImageSet([a for a in ru.images(3) if min(a.shape[:2]) >= 16])
    t = torch.zeros((4, 16, 16, 3), dtype=torch.uint8)
    lab = _labels(len(ok))
    for sets in ((ok, t, t), (t, ok, t)):
        with pytest.raises(NotImplementedError, match="clip_preprocessing on a RaggedImageSet"):
            data.ResidentImageSource(*sets, _labels(4), crop=16, device="cpu", clip_preprocessing=32)
        with pytest.raises(NotImplementedError, match="grayscale=True on a RaggedImageSet"):
            data.ResidentImageSource(*sets, _labels(4), crop=16, device="cpu", grayscale=True)
    with pytest.raises(NotImplementedError, match="clip_preprocessing on a RaggedImageSet"):
        data.ResidentImageSource(t, t, ok, lab, crop=16, device="cpu", clip_preprocessing=32)
    with pytest.raises(NotImplementedError, match="grayscale=True on a RaggedImageSet"):
        data.LabelledImageSet(ok, torch.zeros(len(ok)), ok, lab, t, ["a"], 16, device="cpu", grayscale=True)
    with pytest.raises(NotImplementedError, match="ONE shape"):
        evolve.OEPool(ok)
    src = data.ResidentImageSource(t, ok, t, _labels(4), crop=16, device="cpu")

    class _Trainer:
        ds, logger = src, None
    with pytest.raises(NotImplementedError, match="ONE shape"):
        evolve.run_evolution(_Trainer(), None, [0])
    # a 1-channel ragged set cannot take ColorJitter; a tensor OE set beside a ragged normal set is fine
    gray = data.RaggedImageSet([a for a in ru.images(1) if min(a.shape[:2]) >= 16])
    with pytest.raises(ValueError, match="RGB"):
        data.ResidentImageSource(gray, gray, gray, lab, crop=16, device="cpu", color_jitter=(0.1, 0.1, 0.1, 0.1))
    # rows are rows: the subset machinery does not look at shapes
    src.set_oe_subset([1, 3, 3])
    with pytest.raises(IndexError):
        src.set_oe_subset([len(ok)])


def test_wrappers_refuse_on_the_host():
    from eoe_amd import data
    rs = _set(3)
    p = torch.zeros((2, 4), dtype=torch.int32)
    for fn in (lambda: data.augment_batch(rs, p, (16, 16)), lambda: data.crop_flip_u8(rs, p, (16, 16)),
               lambda: data.color_jitter_crop_u8(rs, p, (16, 16), torch.ones(2, 4), torch.zeros(2, 4, dtype=torch.int32)),
               lambda: data.resize_u8(rs, 16)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    with pytest.raises(TypeError, match="RaggedImageSet"):
        data.color_jitter_crop_u8(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), p, (4, 4), torch.ones(2, 4), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="3 channels"):
        data.color_jitter_crop_u8(_set(1), p, (4, 4), torch.ones(2, 4), torch.zeros(2, 4, dtype=torch.int32))


def test_entry_points_are_declared_exported_and_check_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    names = ["eoe_ragged_augment_batch", "eoe_ragged_crop_flip_u8", "eoe_ragged_color_jitter_crop_u8", "eoe_ragged_resize_pass_u8"]
    for name in names:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5                    # additive: the ABI version does not move

    # the pointers are never followed: every call below returns before a launch
    def aug(arena=16, offsets=32, sizes=48, n_src=4, C=3, params=64, mean=None, std=None, out=128, n=4, Ho=16, Wo=16, noise=0.0, seed=0):
        return lib.eoe_ragged_augment_batch(arena, offsets, sizes, n_src, C, params, mean, std, out, n, Ho, Wo, 1, noise, seed, None)

    assert aug(n=0) == 0                                                           # an empty batch: nothing to do, no launch
    assert aug(C=2) == 1 and b"C must be 1 or 3, not 2" in lib.eoe_last_error()
    for kw in (dict(arena=None), dict(offsets=None), dict(sizes=None), dict(params=None), dict(out=None), dict(n=-1), dict(n_src=0),
               dict(Ho=0), dict(Wo=0), dict(noise=-1.0), dict(seed=1 << 24), dict(n=1 << 22), dict(Ho=300, Wo=300)):
        assert aug(**kw) == 1, kw
    assert aug(mean=48) == 1 and b"both" in lib.eoe_last_error()

    def crop(arena=16, offsets=32, sizes=48, n_src=4, C=3, params=64, out=128, n=4, Ho=16, Wo=16):
        return lib.eoe_ragged_crop_flip_u8(arena, offsets, sizes, n_src, C, params, out, n, Ho, Wo, 1, None)

    assert crop(n=0) == 0 and crop(C=4) == 1
    for kw in (dict(arena=None), dict(offsets=None), dict(sizes=None), dict(params=None), dict(out=None), dict(n_src=0), dict(Ho=0)):
        assert crop(**kw) == 1, kw
    assert crop(out=16) == 1 and b"alias" in lib.eoe_last_error()

    def jit(arena=16, offsets=32, sizes=48, n_src=4, params=64, factors=80, order=96, scratch=112, out=128, n=4, Ho=16, Wo=16):
        return lib.eoe_ragged_color_jitter_crop_u8(arena, offsets, sizes, n_src, params, factors, order, scratch, out, n, Ho, Wo, 1, None)

    assert jit(n=0) == 0
    for kw in (dict(arena=None), dict(offsets=None), dict(sizes=None), dict(params=None), dict(factors=None), dict(order=None),
               dict(scratch=None), dict(out=None), dict(n_src=0), dict(Wo=0), dict(out=16)):
        assert jit(**kw) == 1, kw

    def rsz(src=16, dst=32, offs=48, desc=64, taps=80, n=4, biggest=100):
        return lib.eoe_ragged_resize_pass_u8(src, dst, offs, desc, taps, n, biggest, None)

    assert rsz(n=0) == 0 and rsz(biggest=0) == 0
    for kw in (dict(src=None), dict(dst=None), dict(offs=None), dict(desc=None), dict(taps=None), dict(n=-1), dict(dst=16)):
        assert rsz(**kw) == 1, kw
