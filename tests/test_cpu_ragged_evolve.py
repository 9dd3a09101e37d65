"""CPU tier: the candidate search over an OE pool of MIXED sizes -- `OEPool(rs, crop=...)` on its numpy path against exact int64
sums over explicitly built zero-padded CenterCrop windows and against the tensor pool of those windows, the refusals that stay,
`OEPool.from_source`, the argument checks of `eoe_pool_sqdist_ragged_u8` (all made before anything is copied or launched), and the
operators on a ragged pool against a tensor pool of its centre windows."""
import ctypes as C

import numpy as np
import pytest
import torch

import ragged_evolve_util as reu

# crop 16: an image exactly 16 x 16, narrower than the crop (20 x 11), shorter (12 x 30), smaller on both axes (9 x 13), and larger ones
# with odd and even margins (CenterCrop rounds a half margin to even)
SHAPES = [(16, 16), (20, 11), (9, 13), (17, 23), (31, 16), (22, 19), (12, 30), (19, 26)]


def _set(C_):
    from eoe_amd.data import RaggedImageSet
    imgs = reu.mixed_images(f"ragged_evolve/cpu/c{C_}", SHAPES, C_)
    return imgs, RaggedImageSet(imgs)


@pytest.mark.parametrize("channels", [3, 1])
def test_ragged_pool_distances_are_the_center_window_sums(channels):
    from eoe_amd.data import center_origins
    from eoe_amd.evolve import OEPool
    imgs, rs = _set(channels)
    pool = OEPool(rs, crop=16)
    assert pool.images is rs and pool.features == 16 * 16 * channels and len(pool) == len(SHAPES) and pool.crop == (16, 16)
    wins = reu.center_windows(imgs, 16, 16)
    # the helper's origins are torchvision's rule written out; the product's come from data.center_origins
    assert [[reu.center_origin(h, 16), reu.center_origin(w, 16)] for h, w in SHAPES] == center_origins(np.array(SHAPES), 16).tolist()
    assert wins[0].tobytes() == imgs[0].tobytes() and (wins[2][:3] == 0).all() and (wins[2][:, :1] == 0).all()     # 9 x 13: padded all round
    q, c = [0, 2, 5, 1], [1, 2, 3, 2, 4, 5, 6, 7, 0, 2]
    dist, order = pool.distances(q, c)
    want = reu.np_dist(wins[q], wins[c])
    assert dist.dtype == np.int64 and order.dtype == np.int32 and np.array_equal(dist, want)
    assert np.array_equal(order, reu.stable_order(want))
    assert dist[1, 1] == 0 == dist[1, 3] == dist[1, 9] and order[1, :3].tolist() == [1, 3, 9]       # query among the candidates, in list order
    # the same bits as the tensor pool of those windows
    td, to = OEPool(torch.from_numpy(wins)).distances(q, c)
    assert dist.tobytes() == td.tobytes() and order.tobytes() == to.tobytes()
    # a crop given as a pair, and valid_indices as on a tensor pool
    part = OEPool(rs, valid_indices=[7, 3, 1], crop=(12, 20))
    w2 = reu.center_windows(imgs, 12, 20)
    assert part.features == 12 * 20 * channels and part.rows([2, 0]).tolist() == [1, 7]
    assert np.array_equal(part.distances([0], [1, 2, 0])[0], reu.np_dist(w2[[7]], w2[[3, 1, 7]]))
    with pytest.raises(IndexError):
        part.distances([0], [3])


def test_refusals_and_from_source():
    from eoe_amd.data import RaggedImageSet, ResidentImageSource
    from eoe_amd.evolve import OEPool
    imgs, rs = _set(3)
    with pytest.raises(NotImplementedError, match="ONE shape") as e:
        OEPool(rs)
    assert "crop=" in str(e.value)
    t = torch.zeros((4, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="crop="):
        OEPool(t, crop=16)
    with pytest.raises(ValueError):
        OEPool(rs, crop=0)
    with pytest.raises(ValueError):
        OEPool(rs, valid_indices=[len(SHAPES)], crop=16)
    fits = RaggedImageSet([im for im in imgs if min(im.shape[:2]) >= 16])                # the source refuses images below its crop
    labels = torch.tensor([0, 1, 0, 1])
    src = ResidentImageSource(t, fits, t, labels, crop=16, device="cpu")
    pool = OEPool.from_source(src, valid_indices=[1, 2])
    assert pool.images is src.oe and pool.crop == (16, 16) and pool.features == 768 and pool.valid_indices.tolist() == [1, 2]
    plain = OEPool.from_source(ResidentImageSource(t, t, t, labels, crop=8, device="cpu"))
    assert plain.crop is None and plain.features == 768 and len(plain) == 4             # a tensor OE set is compared whole


def test_entry_points_check_their_arguments_before_launching():
    from eoe_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5               # additive: the ABI version does not move
    assert {"eoe_pool_sqdist_ragged_workspace", "eoe_pool_sqdist_ragged_u8"} <= set(_lib.header_symbols())
    need = C.c_size_t(0)
    ws = lambda ch, cw, ch_, K, P: lib.eoe_pool_sqdist_ragged_workspace(ch, cw, ch_, K, P, C.byref(need))      # noqa: E731
    # 224 x 224 x 3 at P = 100: 11 chunks of 14 336 bytes; the (row, top, left) lists and one partial sum per pair and chunk
    assert ws(224, 224, 3, 2, 100) == 0 and need.value >= 102 * 12 + 2 * 100 * 11 * 4
    assert ws(16, 16, 3, 5, 7) == 0 and 12 * 12 <= need.value <= 256               # one chunk: the lists alone
    assert ws(8192, 8192, 1, 1, 1) == 0                                             # 2^26 bytes: the largest window
    for args in ((0, 16, 3, 1, 1), (16, 0, 3, 1, 1), (-1, 16, 3, 1, 1), (8192, 8192, 3, 1, 1), (8193, 8192, 1, 1, 1), (2 ** 31 - 1, 2 ** 31 - 1, 3, 1, 1),
                 (16, 16, 2, 1, 1), (16, 16, 3, 0, 1), (16, 16, 3, 1, 0), (16, 16, 3, 1025, 1)):
        assert ws(*args) == 1, args
    assert lib.eoe_pool_sqdist_ragged_workspace(16, 16, 3, 1, 1, None) == 1
    # fake, never dereferenced device pointers: every call below must return before anything is read, copied or launched
    ARENA, OFFS, SIZES, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    q, c = np.array([[0, 0, 0]], np.int32), np.array([[1, 2, 3], [2, -4, 5], [59, 0, 0]], np.int32)

    def sqdist(q, c, n_set=60, K=None, P=None, crop=(16, 16), ws_bytes=1 << 20, arena=ARENA, arena_bytes=1 << 20, channels=3, out=OUT):
        return lib.eoe_pool_sqdist_ragged_u8(arena, arena_bytes, OFFS, SIZES, n_set, channels, crop[0], crop[1], q.ctypes.data,
                                             len(q) if K is None else K, c.ctypes.data, len(c) if P is None else P, out, WS, ws_bytes, None)

    for bad_row in (60, -1, 2 ** 31 - 1):
        bad = c.copy()
        bad[1, 0] = bad_row
        assert sqdist(q, bad) == 1
        assert b"candidate 1" in lib.eoe_last_error() and b"outside the set of 60 rows" in lib.eoe_last_error()
    assert sqdist(np.array([[60, 0, 0]], np.int32), c) == 1 and b"query 0" in lib.eoe_last_error()
    assert sqdist(np.array([[-3, 0, 0]], np.int32), c) == 1 and b"query 0" in lib.eoe_last_error()
    assert sqdist(q, c, K=0) == 1 and b"K (queries)" in lib.eoe_last_error()
    assert sqdist(q, c, P=0) == 1 and b"P (candidates)" in lib.eoe_last_error()
    assert sqdist(q, c, crop=(0, 16)) == 1 and sqdist(q, c, crop=(16, 0)) == 1                  # a window of 0 bytes
    assert sqdist(q, c, crop=(8192, 8192)) == 1 and b"67108864" in lib.eoe_last_error()        # 3 * 2^26 bytes: more than 2^26
    assert sqdist(q, c, ws_bytes=8) == 1 and b"workspace" in lib.eoe_last_error()
    assert sqdist(q, c, n_set=0) == 1 and sqdist(q, c, channels=4) == 1
    assert sqdist(q, c, arena_bytes=(1 << 20) + 8) == 1 and sqdist(q, c, arena=ARENA + 4) == 1 and sqdist(q, c, arena_bytes=0) == 1
    assert sqdist(q, c, arena=None) == 1 and sqdist(q, c, out=None) == 1
    for null_at in (2, 3, 8, 10, 13):                                   # offsets, sizes, query, cand, workspace
        args = [ARENA, 1 << 20, OFFS, SIZES, 60, 3, 16, 16, q.ctypes.data, 1, c.ctypes.data, 3, OUT, WS, 1 << 20, None]
        args[null_at] = None
        assert lib.eoe_pool_sqdist_ragged_u8(*args) == 1 and b"null" in lib.eoe_last_error()


# ---------------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("name", list(reu.OP_CASES))
def test_operators_choose_the_ids_of_the_window_tensor_pool(name):
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.evolve import OEPool
    imgs = reu.op_images()
    assert min(min(s) for s in reu.OP_SHAPES) == 32 and max(max(s) for s in reu.OP_SHAPES) == 48
    got = reu.run_operator(OEPool(RaggedImageSet(imgs), crop=32), name)
    want = reu.run_operator(OEPool(torch.from_numpy(reu.center_windows(imgs, 32, 32))), name)
    assert got == want and got != [list(i) for i in reu.OP_CASES[name][1]]                  # and the case does change its individuals


def test_driver_searches_a_ragged_pool_with_an_injected_fitness():
    import random
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.evolve import OEPool, run_evolution
    imgs = reu.op_images()
    hist = []
    for pool in (OEPool(RaggedImageSet(imgs), crop=32), OEPool(torch.from_numpy(reu.center_windows(imgs, 32, 32)))):
        np.random.seed(11)
        random.seed(11)
        hist.append(run_evolution(None, pool, [0], 1, fitness_fn=lambda ind: ((sum(ind) * 37) % 101) / 101.0, oesize=2, generation_pool=6,
                                  mutation_pool=20, mutation_chance=0.8, mate_chance=0.5, generations=3))
    assert hist[0] == hist[1] and len(hist[0]["pop"]) == 3 and hist[0]["pop"][0] != hist[0]["pop"][2]
