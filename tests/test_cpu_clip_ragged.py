"""CPU tier of CLIP's preprocessing on image sets of mixed sizes (eoe_amd.data.clip_preprocess_ragged, the window of the ragged
Resize): the plan's geometry -- window origins, the source rows the horizontal pass keeps, packed offsets -- the plan interpreted in
numpy against Pillow, and the refusals, which all fire on the host.  No kernel runs in this file."""
import numpy as np
import pytest
import torch

import clip_ragged_util as cu
import ragged_util as ru

P = cu.N_PX


def _plan(rs, n_px=P, window=None):
    from eoe_amd import data, _lib
    taps = data._TapArena(_lib.EOE_RESIZE_BICUBIC)
    win = data.clip_window(rs.sizes, n_px) if window is None else window
    return data.ragged_resize_plan(rs.sizes, 3, n_px, taps, rs.offsets_host, True, win), taps, win


# ------------------------------------------------------------------------------------------------------------------ geometry
def test_window_origins_are_center_origins_on_the_resized_sizes():
    from eoe_amd import data
    sizes = np.array(cu.SHAPES + [(P, P + 9), (P + 9, P), (P, P + 3), (P + 3, P), (P, P + 1), (P + 1, P), (7, 8), (375, 500)], np.int32)
    win = data.clip_window(sizes, P)
    full = np.array([data.resized_hw(h, w, P) for h, w in sizes.tolist()])
    assert [tuple(f) for f in full.tolist()] == [cu.resized_hw(h, w, P) for h, w in sizes.tolist()]
    assert (full.min(axis=1) == P).all()                                    # the shorter side is n_px: the window cuts one axis only
    assert np.array_equal(win[:, :2], data.center_origins(full, P)) and (win[:, 2:] == P).all()
    want = [[cu.origin(h, P), cu.origin(w, P)] for h, w in full.tolist()]
    assert win[:, :2].tolist() == want
    k = len(cu.SHAPES)
    # Python's round, halves to even: 9 / 2 -> 4, 3 / 2 -> 2, 1 / 2 -> 0
    assert win[k:k + 6, :2].tolist() == [[0, 4], [4, 0], [0, 2], [2, 0], [0, 0], [0, 0]]
    assert full[4].tolist() == [8, 17] and win[4, :2].tolist() == [0, 4] and full[1].tolist() == [8, 13] and win[1, :2].tolist() == [0, 2]
    assert full[k + 6].tolist() == [8, 9] and win[k + 6].tolist() == [0, 0, 8, 8]          # 7 x 8: count == axis_in, yet no identity
    assert full[-1].tolist() == [8, 10] and win[-1, :2].tolist() == [0, 1]


def test_plan_rows_offsets_and_descriptors():
    """per image: the horizontal pass runs over exactly the source rows that the vertical window's taps touch, writes the window's
    columns, and the vertical pass is told where source row 0 would lie; the results are packed"""
    from eoe_amd import data, _lib
    imgs = cu.images()
    rs = cu.packed_set(imgs)
    plan, taps, win = _plan(rs)
    n = len(imgs)
    assert plan["out_sizes"].tolist() == [[P, P]] * n and plan["out_bytes"] == n * P * P * 3
    assert plan["out_offsets"].tolist() == [i * P * P * 3 for i in range(n)]
    (h_offs, h_desc, h_big), (v_offs, v_desc, v_big) = plan["h"], plan["v"]
    assert h_desc.dtype == np.int32 and h_offs.dtype == np.int64 and h_desc.shape == (n, 8) and v_desc.shape == (n, 8)
    for i, (H, W) in enumerate(cu.SHAPES):
        Ho, Wo = cu.resized_hw(H, W, P)
        top, left = int(win[i, 0]), int(win[i, 1])
        if H == Ho:
            lo, hi = top, top + P
        else:
            b = data._resize_tables_host(H, Ho, _lib.EOE_RESIZE_BICUBIC)[0].numpy()[top:top + P]
            lo, hi = int(b[:, 0].min()), int((b[:, 0] + b[:, 1]).max())
        assert 0 <= lo < hi <= H
        outer, a_in, a_out, inner, _, _, ks, first = h_desc[i].tolist()
        assert (outer, a_in, a_out, inner, first) == (hi - lo, W, P, 3, left), i
        assert (ks == 0) == (W == Wo)
        assert h_offs[i, 0] == rs.offsets_host[i] + lo * W * 3 and h_offs[i, 1] == plan["mid_offsets"][i]
        assert plan["mid_sizes"][i].tolist() == [hi - lo, P] and plan["mid_offsets"][i] % 16 == 0
        outer, a_in, a_out, inner, _, _, ks, first = v_desc[i].tolist()
        assert (outer, a_in, a_out, inner, first) == (1, H, P, P * 3, top), i
        assert (ks == 0) == (H == Ho)
        assert v_offs[i, 0] == plan["mid_offsets"][i] - lo * P * 3 and v_offs[i, 1] == i * P * P * 3
    # the tall images really lose rows, and one virtual start lies in front of the intermediate
    kept = {s: int(plan["mid_sizes"][i, 0]) for i, s in enumerate(cu.SHAPES)}
    assert kept[(13, 8)] == 8 and kept[(40, 3)] < 40 and kept[(31, 20)] < 31 and kept[(8, 13)] == 8 and kept[(20, 31)] == 20
    assert (v_offs[:, 0] < plan["mid_offsets"]).any()
    assert h_big == max(int(plan["mid_sizes"][i, 0]) * P * 3 for i in range(n)) and v_big == P * P * 3
    assert len(taps.seen) == len({(W, cu.resized_hw(H, W, P)[1]) for H, W in cu.SHAPES if W != cu.resized_hw(H, W, P)[1]}
                                 | {(H, cu.resized_hw(H, W, P)[0]) for H, W in cu.SHAPES if H != cu.resized_hw(H, W, P)[0]})
    # with a tall image first, that start is negative: the offset is signed, and the interpreter finds every read inside
    first_tall = cu.packed_set([ru.image(0, 40, 3, 3), ru.image(1, 11, 5, 3)])
    plan, taps, _ = _plan(first_tall)
    assert plan["v"][0][0, 0] < 0 and plan["mid_offsets"][0] == 0
    cu.run_plan_on_host(first_tall, plan, taps)


def test_reach_is_the_union_of_the_windows_tap_bounds():
    """`_TapArena.reach` reads the union off the window's first and last row; here against the union taken row by row, for up- and
    downsampling pairs and every window of a few widths, both filters"""
    from eoe_amd import data, _lib
    for filt in (_lib.EOE_RESIZE_BICUBIC, _lib.EOE_RESIZE_BILINEAR):
        taps = data._TapArena(filt)
        for n_in, n_out in ((5, 17), (40, 106), (31, 12), (3, 8), (500, 298), (9, 8), (1, 8), (8, 9)):
            b = data._resize_tables_host(n_in, n_out, filt)[0].numpy()
            for count in {1, 2, min(8, n_out), n_out}:
                for first in range(0, n_out - count + 1):
                    rows = b[first:first + count]
                    assert taps.reach(n_in, n_out, first, count) == (int(rows[:, 0].min()), int((rows[:, 0] + rows[:, 1]).max()))
        assert taps.reach(13, 13, 2, 8) == (2, 10)                          # a pass Pillow skips: the window's own positions


def test_plan_without_a_window_is_the_plan_it_was():
    """field eight is 0 everywhere, every row is kept and the layouts are those of the unwindowed Resize"""
    from eoe_amd import data, _lib
    rs = data.RaggedImageSet(ru.images(3))
    for size, pair in ((16, False), ((16, 16), True)):
        plan = data.ragged_resize_plan(rs.sizes, 3, size, data._TapArena(_lib.EOE_RESIZE_BICUBIC), rs.offsets_host, pair)
        for name in ("h", "v"):
            assert (plan[name][1][:, 7] == 0).all()
        assert plan["h"][1][:, 0].tolist() == [h for h, _ in ru.SHAPES] and np.array_equal(plan["h"][0][:, 0], rs.offsets_host)
        assert np.array_equal(plan["v"][0][:, 0], plan["mid_offsets"])
        full = [data.resized_hw(h, w, size) for h, w in ru.SHAPES]
        assert plan["out_sizes"].tolist() == [list(f) for f in full]
        assert plan["mid_sizes"].tolist() == [[h, f[1]] for (h, _), f in zip(ru.SHAPES, full)]
        # ... and a window that is the whole resized image gives the same rows
        whole = np.array([[0, 0, f[0], f[1]] for f in full])
        again = data.ragged_resize_plan(rs.sizes, 3, size, data._TapArena(_lib.EOE_RESIZE_BICUBIC), rs.offsets_host, pair, whole)
        for name in ("h", "v"):
            keep = [0, 1, 2, 3, 6, 7]                                       # the tables are entered in another order, no more
            assert np.array_equal(again[name][0], plan[name][0]) and np.array_equal(again[name][1][:, keep], plan[name][1][:, keep])


def test_plan_of_an_all_identity_set_and_of_single_pass_sets():
    from eoe_amd import data
    same = cu.packed_set([ru.image(i, P, P, 3) for i in range(3)])
    plan, _, win = _plan(same)
    assert plan["h"] is None and plan["v"] is None and win.tolist() == [[0, 0, P, P]] * 3
    assert plan["out_offsets"].tolist() == [0, P * P * 3, 2 * P * P * 3]
    # only horizontal windows: one pass, straight into the result, every source row
    wide = cu.packed_set([ru.image(0, P, 13, 3), ru.image(1, P, P, 3), ru.image(2, 5, 11, 3)])
    plan, _, _ = _plan(wide)
    assert plan["h"] is not None and plan["v"] is not None                  # 5 x 11 needs both passes
    wide = cu.packed_set([ru.image(0, P, 13, 3), ru.image(1, P, P, 3), ru.image(2, P, 40, 3)])
    plan, _, _ = _plan(wide)
    assert plan["v"] is None and plan["h"][0][:, 1].tolist() == [0, P * P * 3, 2 * P * P * 3]
    assert plan["h"][1][:, [0, 2, 6, 7]].tolist() == [[P, P, 0, 2], [P, P, 0, 0], [P, P, 0, 16]]
    # only vertical windows: the vertical pass reads the source images themselves
    tall = cu.packed_set([ru.image(0, 13, P, 3), ru.image(1, P, P, 3)])
    plan, _, _ = _plan(tall)
    assert plan["h"] is None and np.array_equal(plan["v"][0][:, 0], tall.offsets_host)
    assert plan["v"][1][:, [0, 1, 2, 3, 6, 7]].tolist() == [[1, 13, P, P * 3, 0, 2], [1, P, P, P * 3, 0, 0]]
    out = cu.run_plan_on_host(tall, plan, data._TapArena(0)).reshape(2, P, P, 3)
    assert np.array_equal(out[0], ru.image(0, 13, P, 3)[2:2 + P]) and np.array_equal(out[1], ru.image(1, P, P, 3))


# --------------------------------------------------------------------------------------------------- the plan against Pillow
def test_windowed_plan_interpreted_on_the_host_equals_pillow_resize_then_crop():
    """"full resize, then crop" by Pillow against the windowed taps applied to the rows the plan keeps, byte for byte on the case
    table; the interpreter checks every index, and that the vertical pass reads only bytes the horizontal pass wrote"""
    pytest.importorskip("PIL")
    imgs = cu.images()
    rs = cu.packed_set(imgs)
    assert int(rs.offsets_host[0]) == 0 and int(rs.offsets_host[-1]) + imgs[-1].size == rs.arena.numel()
    assert (rs.offsets_host[1:-1] % 16 != 0).any()
    plan, taps, _ = _plan(rs)
    out = cu.run_plan_on_host(rs, plan, taps).reshape(len(imgs), P, P, 3)
    for i, a in enumerate(imgs):
        assert np.array_equal(out[i], cu.pillow_clip(a, P)), cu.SHAPES[i]
    # the same set at aligned starts (what RaggedImageSet(list) packs)
    from eoe_amd import data
    al = data.RaggedImageSet(imgs)
    plan, taps, _ = _plan(al)
    assert np.array_equal(cu.run_plan_on_host(al, plan, taps).reshape(len(imgs), P, P, 3), out)


def test_the_unwindowed_plan_through_the_same_interpreter_equals_pillow():
    """the interpreter is the kernel's addressing with field eight = 0: the whole Resize, as before"""
    pytest.importorskip("PIL")
    from eoe_amd import data, _lib
    imgs = cu.images()
    rs = data.RaggedImageSet(imgs)
    taps = data._TapArena(_lib.EOE_RESIZE_BICUBIC)
    plan = data.ragged_resize_plan(rs.sizes, 3, P, taps, rs.offsets_host, False)
    tap = taps.tensor().numpy()
    mid, res = np.zeros(plan["mid_bytes"], np.uint8), np.zeros(plan["out_bytes"], np.uint8)
    mid_w = np.zeros(plan["mid_bytes"], bool)
    cu.emulate_pass(rs.arena.numpy(), mid, plan["h"][0], plan["h"][1], tap, None, mid_w)
    cu.emulate_pass(mid, res, plan["v"][0], plan["v"][1], tap, mid_w, None)
    for i, a in enumerate(imgs):
        h, w = plan["out_sizes"][i]
        o = int(plan["out_offsets"][i])
        assert np.array_equal(res[o:o + h * w * 3].reshape(h, w, 3), cu.pillow_full(a, P)), cu.SHAPES[i]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_bad_windows_are_refused_on_the_host():
    from eoe_amd import data
    rs = cu.packed_set(cu.images())                                         # on the CPU: nothing below reaches a device
    good = data.clip_window(rs.sizes, P)
    for row, col, val in ((1, 1, -1), (2, 0, -1), (1, 1, 6), (2, 0, 6), (4, 1, 10), (0, 0, 1), (0, 1, 1)):
        bad = good.copy()
        bad[row, col] = val
        with pytest.raises(ValueError, match=f"of image {row} lies outside its resized image"):
            data.resize_window_u8(rs, P, bad, "bicubic")
    zero = good.copy()
    zero[:, 2] = 0
    with pytest.raises(ValueError, match="outside its resized image"):
        data.resize_window_u8(rs, P, zero, "bicubic")
    with pytest.raises(ValueError, match="one height and width"):
        data.resize_window_u8(rs, P, good[:-1], "bicubic")
    mixed = good.copy()
    mixed[3, 2] = P - 1
    with pytest.raises(ValueError, match="one height and width"):
        data.resize_window_u8(rs, P, mixed, "bicubic")
    with pytest.raises(ValueError, match="interpolation"):
        data.resize_window_u8(rs, P, good, "nearest")
    with pytest.raises(TypeError, match="RaggedImageSet"):
        data.resize_window_u8(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), P, good[:2])
    with pytest.raises(ValueError, match="out must be"):
        data.resize_window_u8(rs, P, good, "bicubic", out=torch.zeros((len(rs), P, P, 1), dtype=torch.uint8))
    # a good window on a CPU set: the plan is made, then the launch is refused
    with pytest.raises(RuntimeError, match="GPU"):
        data.resize_window_u8(rs, P, good, "bicubic")
    with pytest.raises(RuntimeError, match="GPU"):
        data.clip_preprocess_ragged(rs, P)
    with pytest.raises(RuntimeError, match="GPU"):
        data.clip_preprocess(rs, P)                                         # dispatches
    gray = data.RaggedImageSet([ru.image(i, h, w, 1) for i, (h, w) in enumerate(cu.SHAPES)])
    with pytest.raises(ValueError, match="RGB only"):
        data.clip_preprocess_ragged(gray, P)
    with pytest.raises(ValueError, match="n_px must be positive"):
        data.clip_preprocess_ragged(rs, 0)
    with pytest.raises(TypeError, match="RaggedImageSet"):
        data.clip_preprocess_ragged(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), P)


def _lab(n):
    return torch.tensor([0, 1] * n)[:n]


def test_source_refusals_fire_at_construction_on_the_host():
    from eoe_amd import data
    big = data.RaggedImageSet([ru.image(i, h, w, 3) for i, (h, w) in enumerate([(10, 14), (14, 10), (12, 12), (10, 10)])])
    t = torch.zeros((4, 10, 10, 3), dtype=torch.uint8)
    t8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    lab = _lab(4)
    # a ragged half whose crop is not n_px: for either half, with or without resize=int
    for sets in ((big, t, t8), (t, big, t8)):
        for kw in (dict(), dict(resize=10)):
            with pytest.raises(NotImplementedError, match="clip_preprocessing on a RaggedImageSet needs crop == n_px"):
                data.ResidentImageSource(*sets, lab, crop=8, device="cpu", clip_preprocessing=16, **kw)
    # test_resize with a ragged test set under the option
    with pytest.raises(ValueError, match="test_resize= cannot be combined with clip_preprocessing"):
        data.ResidentImageSource(t8, t8, big, lab, crop=8, device="cpu", clip_preprocessing=8, test_resize=8)
    with pytest.raises(ValueError, match="test_resize= cannot be combined with clip_preprocessing"):
        data.LabelledImageSet(t8, lab, big, lab, t8, ["a", "b"], 8, device="cpu", clip_preprocessing=8, test_resize=8)
    # 1-channel ragged sets: the ragged CLIP path is RGB only
    gray = data.RaggedImageSet([ru.image(i, h, w, 1) for i, (h, w) in enumerate([(10, 14), (14, 10), (12, 12), (10, 10)])])
    with pytest.raises(ValueError, match="RGB only; the test set has 1 channel"):
        data.ResidentImageSource(t8, t8, gray, lab, crop=8, device="cpu", clip_preprocessing=8)
    with pytest.raises(ValueError, match="RGB only; the normal set has 1 channel"):
        data.ResidentImageSource(gray, t8, t8, lab, crop=8, device="cpu", clip_preprocessing=8)
    with pytest.raises(ValueError, match="RGB only; the OE set has 1 channel"):
        data.ResidentImageSource(t8, gray, t8, lab, crop=8, device="cpu", clip_preprocessing=8)
    # the ragged test set is converted at construction, by a kernel
    with pytest.raises(NotImplementedError, match="applied at construction by a HIP kernel"):
        data.ResidentImageSource(t8, t8, big, lab, crop=8, device="cpu", clip_preprocessing=8)
    with pytest.raises(NotImplementedError, match="applied at construction by a HIP kernel"):
        data.LabelledImageSet(t8, lab, big, lab, t8, ["a", "b"], 8, device="cpu", clip_preprocessing=8)
    with pytest.raises(NotImplementedError, match="needs crop == n_px"):
        data.LabelledImageSet(big, lab, t8, lab, t8, ["a", "b"], 8, device="cpu", clip_preprocessing=16)
    # the refusals that clip_preprocessing always had, now with ragged halves beside them
    with pytest.raises(ValueError, match="normalize="):
        data.ResidentImageSource(big, big, t8, lab, crop=8, device="cpu", clip_preprocessing=8, normalize="normalize")
    with pytest.raises(ValueError, match="normalize="):
        data.ResidentImageSource(big, big, t8, lab, crop=8, device="cpu", clip_preprocessing=8, normalize="normalize",
                                 ds_statistics={"mean": [0, 0, 0], "std": [1, 1, 1]})
    with pytest.raises(ValueError, match="square crop"):
        data.ResidentImageSource(big, big, t8, lab, crop=(8, 6), device="cpu", clip_preprocessing=8)
    with pytest.raises(NotImplementedError, match="only upsampling"):
        data.ResidentImageSource(big, big, t8, lab, crop=10, device="cpu", clip_preprocessing=8)
    with pytest.raises(NotImplementedError, match="grayscale=True on a RaggedImageSet"):
        data.ResidentImageSource(big, big, t8, lab, crop=8, device="cpu", clip_preprocessing=8, grayscale=True)
    with pytest.raises(ValueError, match="required crop size"):                # an image smaller than the crop, still found
        data.ResidentImageSource(big, big, t8, lab, crop=12, device="cpu", clip_preprocessing=12)


def test_ragged_halves_with_the_option_draw_what_they_draw_without_it():
    """crop == n_px on ragged normal / OE sets is accepted (on any device: no kernel runs before the first batch), CLIP's statistics
    are the defaults, three given values win, and the host draws are those of the source without the option"""
    from eoe_amd import data
    from eoe_amd.msm import MSM
    big = data.RaggedImageSet([ru.image(i, h, w, 3) for i, (h, w) in enumerate([(10, 14), (14, 10), (12, 12), (10, 10)])])
    t8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    lab = _lab(4)
    a = data.ResidentImageSource(big, big, t8, lab, crop=8, padding=1, device="cpu", seed=7, clip_preprocessing=8)
    b = data.ResidentImageSource(big, big, t8, lab, crop=8, padding=1, device="cpu", seed=7, mean=data.CLIP_MEAN, std=data.CLIP_STD)
    assert a.clip_preprocessing == 8 and tuple(a.mean) == data.CLIP_MEAN and tuple(a.std) == data.CLIP_STD
    assert isinstance(a.normal, data.RaggedImageSet) and isinstance(a.oe, data.RaggedImageSet)
    idx = torch.tensor([3, 0, 2, 1])
    for _ in range(3):
        assert torch.equal(a._draw(idx, a.normal), b._draw(idx, b.normal)) and torch.equal(a._draw(idx, a.oe), b._draw(idx, b.oe))
    c = data.ResidentImageSource(big, big, t8, lab, crop=8, device="cpu", clip_preprocessing=8, mean=(0.5, 0.5, 0.5), std=(0.2, 0.2, 0.2))
    assert tuple(c.mean) == (0.5, 0.5, 0.5)
    # the stage is the identity on these halves, so a claimed sharpen MSM is not in its way
    assert len(a.pre_tensor_msms([MSM.load("sharpen+train_oe--M4")])) == 1
    # a ragged half beside a tensor half that IS upsampled: each set on its own
    t6 = torch.zeros((4, 6, 6, 3), dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="needs crop == n_px"):
        data.ResidentImageSource(t6, big, t8, lab, crop=6, device="cpu", clip_preprocessing=8)
    lset = data.LabelledImageSet(big, lab, t8, lab, big, ["a", "b"], 8, device="cpu", clip_preprocessing=8, padding=1)
    task = lset.source([0], seed=7)
    assert task.clip_preprocessing == 8 and tuple(task.mean) == data.CLIP_MEAN and isinstance(task.normal, data.RaggedImageSet)


def test_entry_point_and_abi_are_unchanged():
    from eoe_amd import _lib
    assert _lib.ABI_VERSION == 5 and _lib.lib.eoe_abi_version() == 5
    assert len(_lib.SIGNATURES["eoe_ragged_resize_pass_u8"]) == 8
