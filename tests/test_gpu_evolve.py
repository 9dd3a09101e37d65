"""GPU tier: the candidate search of the evolve experiment on the device -- `eoe_pool_sqdist_u8` against numpy's exact int64
sums at the smallest shapes at which each of its paths can go wrong, `eoe_pool_rank` on exact ties, the error paths, the
operators on the device path against the numpy path (fixture g21_evolve), the OE subset of the resident source through the batch
indices, `oe_limit_samples` through `run`, and a two-generation evolution of CNN32 / HSC end to end."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evolve_util as eu                                             # noqa: E402
from oracle import fill as ofill                                     # noqa: E402


def _np_dist(u8, q, c):
    flat = u8.reshape(u8.shape[0], -1).astype(np.int64)
    return np.stack([((flat[c] - flat[k]) ** 2).sum(axis=1) for k in q])


def _images(name, shape):
    return ofill.fill_int(name, shape, 0, 256).astype(np.uint8)


def _check(u8, q, c):
    from eoe_amd.evolve import OEPool
    pool = OEPool(torch.from_numpy(u8).cuda())
    dist, order = pool.distances(q, c)
    want = _np_dist(u8, q, c)
    assert dist.dtype == np.int64 and order.dtype == np.int32 and dist.shape == order.shape == (len(q), len(c))
    assert np.array_equal(dist, want)
    assert np.array_equal(order, np.argsort(want, axis=1, kind="stable"))
    again = pool.distances(q, c)
    assert dist.tobytes() == again[0].tobytes() and order.tobytes() == again[1].tobytes()       # two calls, identical bits
    return dist, order


def test_sqdist_exact_100_candidates_one_query():
    u8 = _images("evolve/gpu/cifar", (120, 32, 32, 3))                    # D = 3 072: three chunks of 1 024 bytes per candidate
    cands = ofill.fill_int("evolve/gpu/cands", (100,), 0, 120).tolist()
    _check(u8, [17], cands)


def test_sqdist_exact_repeats_and_query_among_candidates():
    u8 = _images("evolve/gpu/cifar", (120, 32, 32, 3))
    q = [5, 90, 5, 0, 119]
    c = [3, 90, 3, 119, 5, 64, 3, 0, 5]
    dist, order = _check(u8, q, c)
    assert dist[1, 1] == 0 and dist[0, 4] == 0 == dist[2, 8] and np.array_equal(dist[0], dist[2])
    assert order[0].tolist()[:2] == [4, 8]                               # the two zeros in list order, then the rest


@pytest.mark.parametrize("shape", [(9, 7, 9, 3), (9, 28, 28, 1)], ids=["bytewise_189", "grey_784"])
def test_sqdist_exact_odd_and_grey(shape):
    u8 = _images(f"evolve/gpu/{shape[1]}", shape)
    _check(u8, [0, 8, 4], [8, 1, 2, 3, 4, 4, 7])


def test_sqdist_exact_large_images_with_extreme_chunks():
    u8 = _images("evolve/gpu/big", (3, 256, 256, 3))                      # D = 196 608: 192 chunks at P = 3
    u8[1], u8[2] = 255, 0
    dist, _ = _check(u8, [0, 1, 2], [2, 0, 1])
    assert dist[1, 0] == 255 * 255 * 196608 == dist[2, 2]                # every chunk's partial sum is the largest possible
    # 1 024 candidates: the largest chunk (65 536 bytes, partial sum 255^2 * 65 536 = 4 261 478 400 > 2^31), three per candidate
    many = [1] * 1023 + [0]
    dist, order = _check(u8, [2], many)
    assert (dist[0, :1023] == 255 * 255 * 196608).all() and order[0, 0] == 1023 and order[0, 1:].tolist() == list(range(1023))


def test_rank_is_stable_on_exact_ties():
    from eoe_amd._lib import check, lib
    rows = np.array([[5, 3, 5, 3, 3, 9, 0, 5], [7] * 8, [8, 7, 6, 5, 4, 3, 2, 1]], np.int64)
    big = np.concatenate([rows, rows + (1 << 40)], axis=1)               # ties that differ only above 32 bits from the others
    for d in (rows, big, ofill.fill_int("evolve/gpu/rank", (2, 1024), 0, 50)):
        dist = torch.from_numpy(d).cuda()
        order = torch.empty(d.shape, dtype=torch.int32, device="cuda")
        check(lib.eoe_pool_rank(dist.data_ptr(), d.shape[0], d.shape[1], order.data_ptr(), torch.cuda.current_stream().cuda_stream), "rank")
        assert np.array_equal(order.cpu().numpy(), np.argsort(d, axis=1, kind="stable"))
    assert np.argsort(rows[0], kind="stable").tolist() == [6, 1, 3, 4, 0, 2, 7, 5]


def test_error_paths_do_not_touch_the_device():
    from eoe_amd._lib import EoeError, lib
    from eoe_amd.evolve import OEPool
    u8 = _images("evolve/gpu/cifar", (120, 32, 32, 3))
    pool = OEPool(torch.from_numpy(u8).cuda())
    with pytest.raises(IndexError):
        pool.distances([0], [120])
    # straight at the entry point: ids outside the set are refused before the launch and never dereferenced
    imgs, ws = pool.images, torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    q, st = np.array([0], np.int32), torch.cuda.current_stream().cuda_stream
    for bad in ([1, 2, 120, 3], [1, -5, 2, 3], [1, 2, 3, 2 ** 31 - 1]):
        c = np.array(bad, np.int32)
        assert lib.eoe_pool_sqdist_u8(imgs.data_ptr(), 120, 3072, q.ctypes.data, 1, c.ctypes.data, 4, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == 1
        assert b"outside the set of 120 rows" in lib.eoe_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all()
    dist = torch.zeros((1, 1025), dtype=torch.int64, device="cuda")
    order = torch.full((1, 1025), -7, dtype=torch.int32, device="cuda")
    assert lib.eoe_pool_rank(dist.data_ptr(), 1, 1025, order.data_ptr(), st) == 3
    torch.cuda.synchronize()
    assert (order == -7).all()
    with pytest.raises(EoeError, match="at most 1024"):                 # the pool reports it as an error, not as a wrong order
        pool.distances([0], [1] * 1025)
    # and the device is fine afterwards
    _check(u8, [1], [2, 3])


@pytest.mark.parametrize("name", list(eu.CASES))
def test_operators_on_the_device_choose_the_same_ids(golden, name):
    from eoe_amd.evolve import OEPool, mate_individuals, mutate_individual
    g = golden("g21_evolve")
    kind, inds, indp = eu.CASES[name]
    got = {}
    for where in ("cpu", "cuda"):
        pool = OEPool(torch.from_numpy(eu.pool_u8()).to(where))
        cur = [list(i) for i in inds]
        np.random.seed(int(g[f"{name}/seed"]))
        if kind == "mutate":
            mutate_individual(cur[0], pool, eu.POOLSIZE, indp, eu.ONEOFKBEST)
        else:
            mate_individuals(cur[0], cur[1], pool, eu.POOLSIZE, indp, eu.ONEOFKBEST)
        got[where] = cur
    assert got["cuda"] == got["cpu"] == g[f"{name}/out"].tolist()


# ------------------------------------------------------------------------------------------------------ source and trainer
N_NORMAL, N_TEST, N_OE = 64, 64, 40


def _source(mark=None):
    """64 normal, 64 test (every second anomalous) and 40 OE images of 32 x 32 x 3; `mark`: OE rows painted white, all others'
    values kept below 200, so that the pixels tell which OE rows a batch holds"""
    from eoe_amd.data import ResidentImageSource
    img = lambda name, n, lo, hi: torch.from_numpy(ofill.fill_int(name, (n, 32, 32, 3), lo, hi).astype(np.uint8))    # noqa: E731
    oe = img("evolve/gpu/oe", N_OE, 0, 200)
    for r in mark or ():
        oe[r] = 255
    test = img("evolve/gpu/test", N_TEST, 60, 160)
    test[1::2] = img("evolve/gpu/test_anom", N_TEST // 2, 0, 256)
    labels = torch.zeros(N_TEST, dtype=torch.int64)
    labels[1::2] = 1
    return ResidentImageSource(img("evolve/gpu/normal", N_NORMAL, 60, 160), oe, test, labels, crop=32, noise_std=0.0, seed=3)


def _record_batches(src):
    seen, real = [], src._epoch

    def epoch(batch_size):
        for b in real(batch_size):
            seen.append((b[0].detach().clone(), b[1].clone(), b[2].clone()))
            yield b

    src._epoch = epoch
    return seen


def _oe_rows(batch):
    imgs, lbls, idcs = batch
    assert int((lbls == 0).sum()) == int((lbls == 1).sum()) and (idcs[lbls == 0] < N_NORMAL).all()
    return (idcs[lbls == 1] - N_NORMAL).tolist(), imgs[(lbls == 1).to(imgs.device)]


def test_oe_subset_restricts_the_oe_half_of_every_batch():
    src = _source(mark=[13])
    train, _ = src.loaders(24)                                          # 64 normal samples: batches of 24, 24 and a ragged 16
    full = [b for b in train]
    rows = [r for b in full for r in _oe_rows(b)[0]]
    # the full set: 40 rows tiled twice, permuted, the first 64 taken
    assert len(full) == 3 and len(rows) == N_NORMAL and len(set(rows)) > 30 and max(rows.count(r) for r in set(rows)) <= 2
    src.set_oe_subset([13])
    batches = [b for b in train]
    assert [len(b[1]) for b in batches] == [48, 48, 32]
    for b in batches:
        got, imgs = _oe_rows(b)
        assert got == [13] * len(got)                                   # reported as the row of the FULL OE set, offset by the normal set
        assert float(imgs.min()) > 0.999                                # and it IS that image: the white one (the others stay below 0.79)
    src.set_oe_subset([13, 2, 2])
    rows = [r for b in train for r in _oe_rows(b)[0]]
    assert len(rows) == N_NORMAL and set(rows) == {13, 2} and rows.count(2) > rows.count(13)     # rows may repeat: 2 is listed twice
    src.set_oe_subset(None)
    rows = [r for b in train for r in _oe_rows(b)[0]]
    assert len(set(rows)) > 30


def test_trainer_honours_oe_limit_samples():
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    torch.manual_seed(0)
    for limit in ([13, 29], 2):
        src = _source(mark=[13, 29])
        seen = _record_batches(src)
        tr = HSCTrainer(CNN32(bias=True), dataset=src, epochs=1, lr=1e-3, batch_size=32, oe_limit_samples=limit)
        np.random.seed(8)
        want = [13, 29] if isinstance(limit, list) else sorted(int(i) for i in np.random.choice(N_OE, 2, False))
        np.random.seed(8)
        _, res = tr.run()
        assert len(seen) == 2 and 0.0 <= res["mean_auc"] <= 1.0
        rows = [r for b in seen for r in _oe_rows(b)[0]]
        assert len(rows) == N_NORMAL and set(rows) == set(want) and rows.count(want[0]) == N_NORMAL // 2
        if isinstance(limit, list):
            assert all(float(_oe_rows(b)[1].min()) > 0.999 for b in seen)
        assert src.oe_subset.tolist() == want
    # the default never restricts
    src = _source()
    seen = _record_batches(src)
    HSCTrainer(CNN32(bias=True), dataset=src, epochs=1, lr=1e-3, batch_size=32).run()
    assert src.oe_subset is None and len({r for b in seen for r in _oe_rows(b)[0]}) > 30


def test_evolution_end_to_end(tmp_path):
    import json
    from eoe_amd import run_evolution
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(1)
    src = _source()
    seen = _record_batches(src)
    tr = HSCTrainer(CNN32(bias=True), dataset=src, epochs=1, lr=1e-3, batch_size=32, logger=JsonLogger(str(tmp_path)))
    h = run_evolution(tr, None, [0], 1, oesize=1, generation_pool=4, mutation_pool=20, generations=2, mutation_chance=1.0)
    for k in ("pop", "fit", "mean_fit", "std_fit", "max_fit", "min_fit"):
        assert len(h[k]) == 2, k
    fits = [f for gen in h["fit"] for f in gen]
    assert len(fits) == 8 and all(np.isfinite(f) and 0.0 <= f <= 1.0 for f in fits)
    assert all(len(p) == 4 and all(len(ind) == 1 and 0 <= ind[0] < N_OE for ind in p) for p in h["pop"])
    # every training saw exactly its individual's image, and the source is whole again afterwards
    assert tr.ds is src and src.oe_subset is None and tr.oe_limit_samples == np.inf
    trained = [sorted({r for b in seen[i:i + 2] for r in _oe_rows(b)[0]}) for i in range(0, len(seen), 2)]
    assert trained[:4] == [[ind[0]] for ind in h["pop"][0]] and all(len(t) == 1 for t in trained) and 4 < len(trained) <= 8
    with open(tmp_path / "evolution.json") as f:
        nodes = json.load(f)
    assert len(trained) == sum(n["fitness"] is not None for n in nodes)
    with open(tmp_path / "evolve_results.json") as f:
        assert json.load(f) == h
