"""GPU tier: the candidate search over an OE pool of MIXED sizes -- `eoe_pool_sqdist_ragged_u8` at the smallest shapes at which each
of its paths can go wrong (misaligned rows, zero padding, the arena's first and last bytes, chunk edges inside window rows, the largest
partial sums).  Every distance case asserts equality with numpy's exact int64 sums, bitwise equality with the composed path the
kernel replaces (`crop_flip_u8` of the windows, then the uniform pool's kernels) and identical bits on a second call
(`ragged_evolve_util.check_windows` / `check_pool`).  Then the error paths, the operators on the device against the numpy path, and a
two-generation evolution of CNN32 / HSC over a ragged OE set end to end."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ragged_evolve_util as reu                                     # noqa: E402
from oracle import fill as ofill                                     # noqa: E402


def _set(name, shapes, C):
    from eoe_amd.data import RaggedImageSet
    imgs = reu.mixed_images(name, shapes, C)
    return imgs, RaggedImageSet(imgs, device="cuda")


# W * C odd (W = 23, 27, 17, 31) beside even W with an odd centre margin (W = 26, 22: left * C = 15, 9), so the rows of a query and of a
# candidate start at different offsets within a dword; 16 x 16 windows of 48-byte rows: three pieces per window row
MIXED = [(21, 23), (19, 27), (33, 17), (16, 16), (25, 31), (18, 26), (40, 22), (17, 29)]


@pytest.mark.parametrize("channels", [3, 1])
def test_mixed_sizes_with_misaligned_rows(channels):
    imgs, rs = _set(f"ragged_evolve/gpu/mixed{channels}", MIXED, channels)
    q = [0, 5, 2, 5]
    c = [1, 5, 6, 1, 7, 0, 3, 4, 1, 2, 5]
    dist, order = reu.check_pool(rs, imgs, 16, q, c)
    assert dist[1, 1] == 0 == dist[1, 10] == dist[0, 5] == dist[2, 9] and np.array_equal(dist[1], dist[3])
    assert order[1, :2].tolist() == [1, 10]                              # the two zeros in list order
    assert np.array_equal(dist[:, 0], dist[:, 3]) and np.array_equal(dist[:, 0], dist[:, 8])      # a repeated candidate
    reu.check_pool(rs, imgs, (15, 13), [4], c)                           # 39- / 13-byte window rows: every 16-byte piece crosses a row


@pytest.mark.parametrize("channels", [3, 1])
def test_images_equal_to_and_smaller_than_the_crop(channels):
    shapes = [(16, 16), (20, 11), (9, 13), (12, 30), (16, 9), (5, 5), (23, 16)]
    imgs, rs = _set(f"ragged_evolve/gpu/small{channels}", shapes, channels)
    dist, _ = reu.check_pool(rs, imgs, 16, [0, 1, 2, 5], [2, 3, 4, 5, 6, 0, 1, 2])
    assert dist[2, 0] == 0 == dist[2, 7] and dist[0, 5] == 0


def test_explicit_origins_at_the_arena_edges_and_outside_the_images():
    # the last image is 32 x 25 x 3 = 2 400 = 150 * 16 bytes: its final byte is the arena's last byte, with no padding behind it
    shapes = [(18, 21), (23, 19), (32, 25)]
    imgs, rs = _set("ragged_evolve/gpu/edges", shapes, 3)
    assert rs.arena.numel() == int(rs.offsets_host[2]) + 2400
    first_tl, last_br = [0, 0, 0], [2, 32 - 16, 25 - 16]                 # flush with the arena's first byte / its last byte
    part = [[0, -5, -7], [2, 32 - 3, 25 - 4], [1, 23 - 9, -11], [2, -15, 24], [1, 3, 5]]
    outside = [[2, 32, 0], [2, -16, 3], [0, 4, 21], [1, 2, -16], [2, 1000, -1000], [0, -1000, 1000]]
    query = [first_tl, last_br, part[0], outside[0]]
    cand = [last_br, first_tl] + part + outside + [[1, 1, 1]]
    dist = reu.check_windows(rs, imgs, 16, 16, query, cand)
    assert dist[0, 1] == 0 == dist[1, 0]
    own = lambda d: int((reu.window(imgs[d[0]], d[1], d[2], 16, 16).astype(np.int64) ** 2).sum())      # noqa: E731
    for j in range(len(outside)):                                       # against a window wholly outside: the other window's own sum of squares
        for i in range(3):
            assert dist[i, 2 + len(part) + j] == own(query[i]) > 0
        assert dist[3, 2 + len(part) + j] == 0                          # outside against outside
    assert [dist[3, j] for j in range(2 + len(part))] == [own(d) for d in cand[:2 + len(part)]]
    # origins at the ends of int32: nothing to compose them with (the crop kernel adds to its origins), so numpy and a second call
    far = [[2, 2 ** 31 - 1, 0], [0, 0, -2 ** 31], [1, -2 ** 31, 2 ** 31 - 1], [2, 2 ** 31 - 1, 2 ** 31 - 1]]
    rc, got = reu.sqdist_ragged(rs, 16, 16, query[:3], far)
    assert rc == 0 and got.tolist() == [[own(d)] * 4 for d in query[:3]]
    assert got.tobytes() == reu.sqdist_ragged(rs, 16, 16, query[:3], far)[1].tobytes()
    # a window wider than the images: every window row holds padding on both sides
    reu.check_windows(rs, imgs, 7, 40, [[0, 2, -9], [2, 30, -3]], [[1, 0, -10], [2, -3, -8], [0, 2, -9]])


def test_imagenet_windows_with_the_largest_partial_sums():
    from eoe_amd.data import RaggedImageSet
    shapes = [(256, 300), (257, 301), (300, 256)]                        # 224 x 224 x 3 = 150 528 bytes in 672-byte window rows
    imgs = reu.mixed_images("ragged_evolve/gpu/big", shapes, 3)
    imgs[1][...], imgs[2][...] = 255, 0
    rs = RaggedImageSet(imgs, device="cuda")
    # P = 3: 147 chunks of 1 024 bytes per candidate, the most there are; chunk edges fall inside window rows (1 024 / 672)
    dist, _ = reu.check_pool(rs, imgs, 224, [0, 1, 2], [2, 0, 1])
    assert dist[1, 0] == 255 * 255 * 150528 == dist[2, 2] and dist[1, 2] == 0 == dist[2, 0]
    # P = 1 024: the largest chunk (65 536 bytes, partial sum 255^2 * 65 536 = 4 261 478 400 > 2^31), three per candidate
    many = [1] * 1023 + [0]
    dist, order = reu.check_pool(rs, imgs, 224, [2, 0, 1], many)
    assert (dist[0, :1023] == 255 * 255 * 150528).all() and (dist[2, :1023] == 0).all()
    assert order[0, 0] == 1023 and order[0, 1:].tolist() == list(range(1023)) and order[2, -1] == 1023


def test_error_paths_do_not_touch_the_device():
    from eoe_amd._lib import EoeError, lib
    from eoe_amd.evolve import OEPool
    imgs, rs = _set("ragged_evolve/gpu/mixed3", MIXED, 3)
    pool = OEPool(rs, crop=16)
    with pytest.raises(IndexError):
        pool.distances([0], [len(MIXED)])
    out = torch.full((1, 4), -7, dtype=torch.int64, device="cuda")
    for bad in (len(MIXED), -5, 2 ** 31 - 1):
        rc, _ = reu.sqdist_ragged(rs, 16, 16, [[0, 0, 0]], [[1, 0, 0], [2, 1, 1], [bad, 0, 0], [3, 0, 0]], out=out)
        assert rc == 1 and f"outside the set of {len(MIXED)} rows".encode() in lib.eoe_last_error()
    rc, _ = reu.sqdist_ragged(rs, 16, 16, [[0, 0, 0]], [[1, 0, 0], [2, 1, 1], [5, 0, 0], [3, 0, 0]], out=out, n_set=5)    # a row past a SHORTER set
    assert rc == 1
    torch.cuda.synchronize()
    assert (out == -7).all()
    with pytest.raises(EoeError, match="at most 1024"):                 # the pool reports it as an error, not as a wrong order
        pool.distances([0], [1] * 1025)
    reu.check_pool(rs, imgs, 16, [1], [2, 3])                            # and the device is fine afterwards


@pytest.mark.parametrize("name", list(reu.OP_CASES))
def test_operators_on_the_device_choose_the_same_ids(name):
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.evolve import OEPool
    imgs = reu.op_images()
    wins = torch.from_numpy(reu.center_windows(imgs, 32, 32))
    got = {"cuda ragged": reu.run_operator(OEPool(RaggedImageSet(imgs, device="cuda"), crop=32), name),
           "cpu ragged": reu.run_operator(OEPool(RaggedImageSet(imgs), crop=32), name),
           "cuda tensor": reu.run_operator(OEPool(wins.cuda()), name)}
    assert got["cuda ragged"] == got["cpu ragged"] == got["cuda tensor"] != [list(i) for i in reu.OP_CASES[name][1]]


# ---------------------------------------------------------------------------------------------------------------- end to end
N_NORMAL, N_TEST, N_OE = 64, 64, 40


def _source():
    """64 normal and 64 test images (every second anomalous) of 32 x 32 x 3 as tensors, and a ragged OE set of 40 images of 32 to 48 px"""
    from eoe_amd.data import RaggedImageSet, ResidentImageSource
    img = lambda name, n, lo, hi: torch.from_numpy(ofill.fill_int(name, (n, 32, 32, 3), lo, hi).astype(np.uint8))    # noqa: E731
    oe_shapes = [(32 + (5 * i) % 17, 32 + (7 * i + 3) % 17) for i in range(N_OE)]
    oe = RaggedImageSet(reu.mixed_images("ragged_evolve/gpu/oe", oe_shapes, 3, 0, 200))
    test = img("ragged_evolve/gpu/test", N_TEST, 60, 160)
    test[1::2] = img("ragged_evolve/gpu/test_anom", N_TEST // 2, 0, 256)
    labels = torch.zeros(N_TEST, dtype=torch.int64)
    labels[1::2] = 1
    return ResidentImageSource(img("ragged_evolve/gpu/normal", N_NORMAL, 60, 160), oe, test, labels, crop=32, noise_std=0.0, seed=3)


def _record_batches(src):
    seen, real = [], src._epoch

    def epoch(batch_size):
        for b in real(batch_size):
            seen.append((b[1].clone(), b[2].clone()))
            yield b

    src._epoch = epoch
    return seen


def _oe_rows(batch):
    lbls, idcs = batch
    assert int((lbls == 0).sum()) == int((lbls == 1).sum()) and (idcs[lbls == 0] < N_NORMAL).all()
    return (idcs[lbls == 1] - N_NORMAL).tolist()


def test_evolution_over_a_ragged_oe_set_end_to_end(tmp_path):
    import json
    from eoe_amd import OEPool, run_evolution
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(1)
    src = _source()
    assert isinstance(src.oe, RaggedImageSet) and src.oe.is_cuda and not src.oe.is_uniform
    seen = _record_batches(src)
    tr = HSCTrainer(CNN32(bias=True), dataset=src, epochs=1, lr=1e-3, batch_size=32, logger=JsonLogger(str(tmp_path)))
    pool = OEPool.from_source(src)
    assert pool.images is src.oe and pool.crop == (32, 32) and len(pool) == N_OE
    h = run_evolution(tr, pool, [0], 1, oesize=1, generation_pool=4, mutation_pool=20, generations=2, mutation_chance=1.0)
    for k in ("pop", "fit", "mean_fit", "std_fit", "max_fit", "min_fit"):
        assert len(h[k]) == 2, k
    fits = [f for gen in h["fit"] for f in gen]
    assert len(fits) == 8 and all(np.isfinite(f) and 0.0 <= f <= 1.0 for f in fits)
    assert all(len(p) == 4 and all(len(ind) == 1 and 0 <= ind[0] < N_OE for ind in p) for p in h["pop"])
    assert h["pop"][0] != h["pop"][1]                                   # the mutations did search the pool
    # every training saw exactly its individual's image, and the source is whole again afterwards
    assert tr.ds is src and src.oe_subset is None and tr.oe_limit_samples == np.inf
    trained = [sorted({r for b in seen[i:i + 2] for r in _oe_rows(b)}) for i in range(0, len(seen), 2)]
    assert trained[:4] == [[ind[0]] for ind in h["pop"][0]] and all(len(t) == 1 for t in trained) and 4 < len(trained) <= 8
    with open(tmp_path / "evolution.json") as f:
        nodes = json.load(f)
    assert len(trained) == sum(n["fitness"] is not None for n in nodes)
    with open(tmp_path / "evolve_results.json") as f:
        assert json.load(f) == h
