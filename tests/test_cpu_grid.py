"""Image grids without a GPU: the numpy path of `eoe_amd.imgrid.image_grid` and `JsonLogger.logimg` against the pictures of the
reference's `Logger.logimg` (tests/golden/g26_grid.npz), geometry and refusals, the PNG and header files, `Genealogy.scores_best`,
and that `run_evolution` without `log_images` does what it did before."""
import json
import os
import random

import numpy as np
import pytest
import torch

import evolve_util
import grid_util

SIZES = [(40, 30), (30, 40), (20, 50), (33, 33), (64, 64)]


@pytest.mark.parametrize("name", grid_util.case_names())
def test_fixture_cases_on_the_host_path(name):
    from eoe_amd.imgrid import image_grid
    src, rows, kw, ref, mask, rgb = grid_util.case(name)
    got = image_grid(src, rows, **kw)
    grid_util.compare(name, got, ref, mask, rgb)
    if src.dtype == torch.uint8:                  # the uint8 form is the fp32 form fed u8 / 255, bit for bit
        assert torch.equal(image_grid(grid_util.as_f32(src, rows), **kw), got)


def test_second_pass_takes_the_first_pass_bytes():
    from eoe_amd.imgrid import image_grid, image_grids
    rows, strips, ref = grid_util.second_pass_inputs()
    pool = torch.from_numpy(grid_util.fixture()["in/u8"])
    first = image_grids(pool, rows, nrow=16)
    assert first.shape[0] == len(rows) and all(np.array_equal(first[i].numpy(), s) for i, s in enumerate(strips))
    grid_util.compare("second_pass", image_grid(first, nrow=1, maxres=1024), ref, None, None)


def test_geometry_and_the_empty_picture():
    from eoe_amd.imgrid import grid_geometry, image_grid
    x = torch.zeros(17, 3, 9, 7)
    assert tuple(image_grid(x, nrow=4).shape) == ((9 + 2) * 5 + 2, (7 + 2) * 4 + 2, 3)
    assert tuple(image_grid(x, nrow=32, pad=0).shape) == (9, 7 * 17, 3)                       # xmaps = n < nrow
    assert tuple(image_grid(x, [3], pad=1).shape) == (11, 9, 3)                               # a lone image is padded like any other
    assert tuple(image_grid(x, nrow=4, pad=3, row_sep_at=(16, 1)).shape) == ((9 + 3) * 5 + 3 + 16, (7 + 3) * 4 + 3, 3)
    g = grid_geometry(5, 9, 7, nrow=4, pad=3, row_sep_at=(16, 1))
    assert g["sep_pos"] == (9 + 3) * 1 + 3 // 2 and g["rows"] == g["Hg"] + 16
    assert grid_geometry(4, 130, 100)["ch"] == grid_geometry(4, 130, 100)["cw"] == 128        # one side beyond maxres resizes both
    empty = image_grid(x, [])
    assert tuple(empty.shape) == (0, 0, 3) and empty.dtype == torch.uint8
    assert not image_grid(torch.full((2, 1, 4, 4), 0.5), mark=[0]).numpy()[3:5, 3:5].any()    # a constant image under mark: all 0


def test_refusals_name_the_argument():
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.imgrid import image_grid, image_grids
    x = torch.zeros(4, 3, 5, 5)
    with pytest.raises(ValueError, match="nrow"):
        image_grid(x, nrow=0)
    with pytest.raises(ValueError, match="nrow"):
        image_grid(x, [], nrow=0)
    with pytest.raises(ValueError, match=r"c \(channels\)"):
        image_grid(torch.zeros(4, 2, 5, 5))
    with pytest.raises(ValueError, match="32-bit"):
        image_grid(torch.zeros(1, 1, 2, 2), np.zeros(1 << 29, dtype=np.int64))
    with pytest.raises(IndexError):
        image_grid(x, [4])
    with pytest.raises(IndexError):
        image_grid(x, mark=[4])
    with pytest.raises(ValueError, match="crop"):
        image_grid(RaggedImageSet([np.zeros((4, 5, 3), np.uint8)]))
    with pytest.raises(ValueError, match="crop"):
        image_grid(x, crop=4)
    with pytest.raises(ValueError):
        image_grid(torch.zeros(4, 3, 5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="pictures"):
        image_grids(x, [0, 1])


def test_c_abi_refuses_before_any_launch():
    from eoe_amd import _lib
    lib = _lib.lib
    names = {"eoe_grid_f32", "eoe_grid_u8", "eoe_grid_ragged_u8"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5                    # additive: the ABI version does not move
    # the pointers are never followed: every call below returns before a launch
    f32 = lambda C_=3, n=4, nrow=8, out=0, h=5: lib.eoe_grid_f32(16, 4, C_, h, 5, 16, n, 1, nrow, 2, 128, 0, 0, 0, 16, 16, out, None)   # noqa: E731
    assert f32(nrow=0) == 1 and b"nrow" in lib.eoe_last_error()
    assert f32(C_=2) == 1 and b"C must be 1 or 3" in lib.eoe_last_error()
    assert f32(n=1 << 30, h=32768) == 1 and b"n * cell" in lib.eoe_last_error()
    assert f32(out=7) == 1 and b"out of 7 bytes" in lib.eoe_last_error()
    assert f32(n=0) == 0                                                              # the empty picture: nothing is written
    assert lib.eoe_grid_u8(16, 4, 5, 5, 4, 16, 4, 1, 8, 2, 128, 0, 0, 0, 16, 16, 0, None) == 1 and b"C must" in lib.eoe_last_error()
    assert lib.eoe_grid_ragged_u8(16, 0, 16, 16, 4, 3, 8, 8, 16, 4, 1, 8, 2, 128, 0, 0, 0, 16, 16, 0, None) == 1
    assert b"arena" in lib.eoe_last_error()


def _ragged_images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


def test_ragged_windows_equal_the_uniform_form_on_the_host():
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.evolve import OEPool
    from eoe_amd.imgrid import image_grid
    rs = RaggedImageSet(_ragged_images())
    pool, ids = OEPool(rs, crop=32), [4, 0, 1, 2, 3, 2]
    windows = torch.from_numpy(pool._windows_host(pool.rows(ids)))
    want = image_grid(windows, nrow=4, mark=[[1, 2]])
    assert torch.equal(image_grid(pool, ids, nrow=4, mark=[[1, 2]]), want)
    assert torch.equal(image_grid(rs, ids, crop=32, nrow=4, mark=[[1, 2]]), want)
    # cell 3 is image 2 (20 x 50): CenterCrop(32) pads 6 zero rows above and below, and zero is then the cell's minimum
    cell = want.numpy()[2:2 + 32, 2 + 3 * 34:2 + 3 * 34 + 32]
    assert not cell[:6].any() and not cell[26:].any() and cell[6:26].any()


def test_logimg_writes_png_and_headers(tmp_path):
    from PIL import Image
    from eoe_amd.training.ad_trainer import JsonLogger
    src, rows, kw, ref, mask, rgb = grid_util.case("mark_sep")
    logger = JsonLogger(str(tmp_path))
    img = logger.logimg(os.path.join("selection", "gen001"), src, rows, rowheaders=["a", 2.5], **kw)
    grid_util.compare("mark_sep", img, ref, mask, rgb)
    assert isinstance(img, np.ndarray)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "selection" / "gen001.png").convert("RGB")), img)
    assert json.load(open(tmp_path / "selection" / "gen001.headers.json")) == ["a", "2.5"]
    logger.logimg("plain", src, rows, step=3)
    assert (tmp_path / "plain_v3.png").exists() and not (tmp_path / "plain_v3.headers.json").exists()
    quiet = JsonLogger(None)
    assert np.array_equal(quiet.logimg("x", src, rows, rowheaders=["a"], **kw), img) and not quiet.active


def test_logimg_without_pillow_returns_the_array(tmp_path, monkeypatch):
    import builtins
    from eoe_amd import imgrid
    from eoe_amd.training.ad_trainer import JsonLogger
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("no Pillow")
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_pil)
    monkeypatch.setattr(imgrid, "_PILLOW_WARNED", False)
    src, rows, kw, ref, mask, rgb = grid_util.case("n5_nrow4")
    with pytest.warns(UserWarning, match="Pillow"):
        img = JsonLogger(str(tmp_path)).logimg("a", src, rows, **kw)
    assert np.array_equal(img, ref) and not (tmp_path / "a.png").exists()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                 # warned once
        JsonLogger(str(tmp_path)).logimg("b", src, rows, **kw)


def _tree(entries):
    """a genealogy of (ids, fitness or None) nodes"""
    from eoe_amd.evolve import Genealogy, Individual
    tree = Genealogy()
    for gen, (ids, fit) in enumerate(entries):
        ind = Individual(ids)
        tree.add(ind)
        if fit is not None:
            tree.evaluated(ind, gen, fit)
    return tree


def test_scores_best_on_hand_built_trees():
    tree = _tree([([3, 1], 0.50), ([0, 2], 0.75), ([3, 1], 0.90), ([5, 5], None), ([1, 3], 0.25), ([4, 4], 0.75), ([2, 2], 0.60)])
    # [3, 1] appears twice: the first node (0.50) is kept; [5, 5] was never evaluated
    assert tree.scores_best(k=20) == [0.25, 0.50, 0.60, 0.75, 0.75]                    # k larger than the tree
    assert tree.scores_best(k=2) == [0.75, 0.75]
    assert tree.scores_best(k=2, reverse=True) == [0.25, 0.50]
    fits, nodes = tree.scores_best(k=3, return_nodes=True)
    assert fits == [0.60, 0.75, 0.75] and [n["ids"] for n in nodes] == [[2, 2], [0, 2], [4, 4]]      # equal fitness: id-list order
    assert [n["id"] for n in tree.scores_best(k=1, reverse=True, return_nodes=True)[1]] == [4]
    assert _tree([([1], None)]).scores_best() == [] and tree.scores_best(k=0) == []
    assert all("file" not in n for n in tree.to_json())


def _fitness(ind):
    return ((sum(int(i) * (k + 3) for k, i in enumerate(ind)) * 2654435761) % 1000) / 1000.0


class _Holder:
    def __init__(self, logger):
        self.logger = logger


def _run(tmp, log_images, oesize=2):
    from eoe_amd.evolve import OEPool, run_evolution
    from eoe_amd.training.ad_trainer import JsonLogger
    np.random.seed(11)
    random.seed(11)
    pool = OEPool(torch.from_numpy(evolve_util.pool_u8()))
    history = run_evolution(_Holder(JsonLogger(str(tmp))), pool, [0], fitness_fn=_fitness, oesize=oesize, generation_pool=6,
                            mutation_pool=20, generations=3, mutation_chance=0.7, mate_chance=0.6, log_images=log_images)
    return history, json.load(open(os.path.join(tmp, "evolve_results.json"))), json.load(open(os.path.join(tmp, "evolution.json")))


def test_run_evolution_without_log_images_is_the_parent_commits_run(tmp_path):
    """same seed, same JSON: tests/golden/g26_evolve_off.json holds `evolve_results` and `evolution` of this very call made
    with the commit before `log_images` existed (`_run` is the recipe)"""
    want = json.load(open(os.path.join(os.path.dirname(grid_util.GOLDEN), "g26_evolve_off.json")))
    history, results, tree = _run(str(tmp_path), False)
    assert results == want["evolve_results"] and tree == want["evolution"]
    assert json.loads(json.dumps(history)) == want["evolve_results"]
    pictures = [f for _, _, files in os.walk(tmp_path) for f in files if f.endswith((".png", ".headers.json"))]
    assert pictures == []


@pytest.mark.parametrize("oesize", [2, 1])
def test_run_evolution_with_log_images_on_the_host(tmp_path, oesize):
    from PIL import Image
    from eoe_amd.evolve import OEPool
    from eoe_amd.imgrid import image_grid, image_grids
    off = _run(str(tmp_path / "off"), False, oesize)
    history, results, tree = _run(str(tmp_path / "on"), True, oesize)
    assert results == off[1]                                                           # no draw depends on the figures
    assert [{k: v for k, v in n.items() if k != "file"} for n in tree] == off[2]
    on = tmp_path / "on"
    for g in range(3):
        for name in [f"raw_gen/gen{g:03}.png", f"gen{g:03}.png", f"gen{g:03}.headers.json"]:
            assert (on / name).exists(), name
        for stage in ("selection", "mating", "mutation"):
            assert (on / stage / f"gen{g:03}.png").exists() == (g > 0), (stage, g)
    assert sorted(os.listdir(on / "final")) == ["best.headers.json", "best.png", "best_raw.png", "worst.headers.json", "worst.png",
                                                "worst_raw.png"]
    pool = OEPool(torch.from_numpy(evolve_util.pool_u8()))
    evaluated = [n for n in tree if n["fitness"] is not None]
    assert evaluated and len(os.listdir(on / "individuals")) == len(evaluated)
    for n in evaluated:
        assert n["file"].startswith(str(on / "individuals")) and f"_fit{n['fitness'] * 100:06.3f}.png" in n["file"]
        assert np.array_equal(np.asarray(Image.open(n["file"])), image_grid(pool, n["ids"], nrow=16).numpy())
    assert json.load(open(on / "gen002.headers.json")) == [f"{f * 100:06.3f}" for f in sorted(history["fit"][2])]
    from eoe_amd.evolve import Genealogy
    t = Genealogy()
    t.nodes = tree
    fits, nodes = t.scores_best(20, return_nodes=True)
    two_pass = image_grid(image_grids(pool, [n["ids"] for n in nodes], nrow=16), nrow=20, maxres=1024)
    assert np.array_equal(np.asarray(Image.open(on / "final" / "best_raw.png")), two_pass.numpy())
    assert json.load(open(on / "final" / "best.headers.json")) == [f"{f * 100:06.3f}" for f in fits]
    first = np.asarray(Image.open(on / "selection" / "gen001.png"))
    size = (32 + 2) * (6 if oesize > 1 else 1) + 2
    assert first.shape[0] == 2 * size - 2 + 16 and not first[size - 1:size - 1 + 16].any()     # 16 black rows between before and after
