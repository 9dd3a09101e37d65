"""Image grids on the MI355X (csrc/grid.hip): every case of tests/golden/g26_grid.npz through the kernel under the rules of
tests/grid_util.py, the three source forms against each other, the grid's edge shapes, the evolve experiment's figures and the
trainer's previews."""
import json
import os
import random

import numpy as np
import pytest
import torch

import grid_util
from oracle import fill as ofill

pytestmark = pytest.mark.gpu

SIZES = [(40, 30), (30, 40), (20, 50), (33, 33), (64, 64)]


@pytest.mark.parametrize("name", grid_util.case_names())
def test_fixture_cases_through_the_kernel(name):
    from eoe_amd.imgrid import image_grid
    src, rows, kw, ref, mask, rgb = grid_util.case(name, "cuda")
    got = image_grid(src, rows, **kw)
    assert got.is_cuda and got.dtype == torch.uint8
    grid_util.compare(name, got, ref, mask, rgb)
    if src.dtype == torch.uint8:                  # the uint8 form is bit-equal to the fp32 form fed u8 / 255
        assert torch.equal(image_grid(grid_util.as_f32(src, rows), **kw), got)
    assert torch.equal(image_grid(src.cpu(), rows, **kw), got.cpu()), "the host path yields other bytes"


def test_second_pass_takes_the_first_pass_bytes():
    from eoe_amd.imgrid import image_grid, image_grids
    rows, strips, ref = grid_util.second_pass_inputs()
    pool = torch.from_numpy(grid_util.fixture()["in/u8"]).cuda()
    first = image_grids(pool, rows, nrow=16)                    # all strips: one launch pair, one buffer
    assert first.is_cuda and first.is_contiguous() and first.shape[0] == len(rows)
    assert all(np.array_equal(first[i].cpu().numpy(), s) for i, s in enumerate(strips))
    grid_util.compare("second_pass", image_grid(first, nrow=1, maxres=1024), ref, None, None)


def test_ragged_windows_equal_the_uniform_form():
    """5 images of mixed sizes, crop 32: the arena's centre windows give the bytes of the uniform form applied to
    `OEPool._windows_host` of the same rows -- 20 x 50 and 30 x 40 are narrower than the crop on one side (zero padding)"""
    from eoe_amd.data import RaggedImageSet
    from eoe_amd.evolve import OEPool
    from eoe_amd.imgrid import image_grid
    rng = np.random.default_rng(5)
    rs = RaggedImageSet([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES])
    host, ids = OEPool(rs, crop=32), [4, 0, 1, 2, 3, 2]
    windows = torch.from_numpy(host._windows_host(host.rows(ids))).cuda()
    pool = OEPool(rs.to("cuda"), crop=32)
    for kw in (dict(nrow=4), dict(nrow=4, mark=[[1, 2]], row_sep_at=(16, 1)), dict(nrow=8, maxres=24)):
        want = image_grid(windows, **kw)
        assert torch.equal(image_grid(pool, ids, **kw), want), kw
        assert torch.equal(image_grid(rs.to("cuda"), ids, crop=32, **kw), want), kw
    cell = image_grid(pool, ids, nrow=4, mark=[]).cpu().numpy()[2:2 + 32, 2 + 3 * 34:2 + 3 * 34 + 32]      # image 2 (20 x 50)
    assert not cell[:6].any() and not cell[26:].any() and cell[6:26].any()


def test_grid_edge_shapes():
    """257 cells of 3 x 5 x 5 at nrow = 16: more workgroups than one wave of the reduction's grid, a last row of one cell, rows of
    Wg * 3 = 342 bytes and a picture of 121 * 342 bytes (neither a multiple of 4: the dword stores straddle rows, the last two
    bytes are the byte-store tail).  Every row of cells must be the picture of its own 16 cells, a shape class the fixture pins
    (n16_nrow16, n1_nrow16), and everything else 0."""
    from eoe_amd.imgrid import image_grid
    x = torch.from_numpy(ofill.fill("grid/edge", (257, 3, 5, 5), std=1.0)).cuda()
    full = image_grid(x, nrow=16).cpu().numpy()
    assert full.shape == (7 * 17 + 2, 7 * 16 + 2, 3) and (full.shape[1] * 3) % 4 and full.size % 4
    for r in range(17):
        chunk = image_grid(x, list(range(16 * r, min(16 * r + 16, 257))), nrow=16).cpu().numpy()
        band = full[7 * r:7 * r + 9]
        assert np.array_equal(band[:, :chunk.shape[1]], chunk), r
        assert not band[:, chunk.shape[1]:].any()
    marked = image_grid(x, nrow=16, mark=[[256]]).cpu().numpy()
    assert (marked[7 * 16 + 2, 2:7] == (224, 28, 28)).all() and not marked[7 * 16 + 2:, 9:].any()


def _pool_and_table():
    imgs = torch.from_numpy(ofill.fill_int("grid/pool", (32, 32, 32, 3), 0, 256).astype(np.uint8))
    table = ofill.fill("grid/fitness", (32, 32), std=1.0)
    fitness = lambda ind: float(0.5 + 0.4 * np.tanh(sum(table[k % 32, int(i)] for k, i in enumerate(ind))))      # noqa: E731
    return imgs, fitness


class _Holder:
    def __init__(self, logger):
        self.logger = logger


def test_run_evolution_logs_its_figures(tmp_path):
    from PIL import Image
    from eoe_amd.evolve import Genealogy, OEPool, run_evolution
    from eoe_amd.imgrid import image_grid, image_grids
    from eoe_amd.training.ad_trainer import JsonLogger
    imgs, fitness = _pool_and_table()
    pool = OEPool(imgs.cuda())
    np.random.seed(4)
    random.seed(4)
    run_evolution(_Holder(JsonLogger(str(tmp_path))), pool, [0], fitness_fn=fitness, oesize=3, generation_pool=4, mutation_pool=16,
                  generations=2, mutation_chance=0.8, mate_chance=0.8, log_images=True)
    tree = json.load(open(tmp_path / "evolution.json"))
    evaluated = [n for n in tree if n["fitness"] is not None]
    files = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(tmp_path) for f in fs if not f.endswith(".json"))
    want = ["gen000.png", "gen001.png", "raw_gen/gen000.png", "raw_gen/gen001.png", "selection/gen001.png", "mating/gen001.png",
            "mutation/gen001.png", "final/best.png", "final/best_raw.png", "final/worst.png", "final/worst_raw.png"]
    want += [os.path.relpath(n["file"], tmp_path) for n in evaluated]
    assert files == sorted(want) and len(evaluated) >= 4
    for n in evaluated:                                        # the nodes carry the paths; each file is its individual's strip
        assert os.path.basename(n["file"]).startswith(f"gen{n['generation']:03}_ind") and n["file"].endswith(f"_fit{n['fitness'] * 100:06.3f}.png")
        assert np.array_equal(np.asarray(Image.open(n["file"])), image_grid(pool, n["ids"], nrow=16).cpu().numpy())
    t = Genealogy()
    t.nodes = tree
    fits, nodes = t.scores_best(20, return_nodes=True)
    two_pass = image_grid(image_grids(pool, [n["ids"] for n in nodes], nrow=16), nrow=20, maxres=1024)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "final" / "best_raw.png")), two_pass.cpu().numpy())
    assert json.load(open(tmp_path / "final" / "best.headers.json")) == [f"{f * 100:06.3f}" for f in fits]


def _source():
    from eoe_amd.data import ResidentImageSource
    img = lambda name, n, lo, hi: torch.from_numpy(ofill.fill_int(name, (n, 32, 32, 3), lo, hi).astype(np.uint8))    # noqa: E731
    labels = torch.zeros(64, dtype=torch.int64)
    labels[1::2] = 1
    return ResidentImageSource(img("grid/normal", 64, 60, 160), img("grid/oe", 40, 0, 200), img("grid/test", 64, 0, 256), labels,
                               crop=32, padding=2, seed=3)


def test_preview_leaves_the_source_unchanged():
    plain, asked = _source(), _source()
    x, counts = asked.preview(40, True)
    assert tuple(x.shape) == (80, 3, 32, 32) and x.dtype == torch.float32 and counts == {0: 64, 1: 40}
    xt, ct = asked.preview(20, False)
    assert tuple(xt.shape) == (40, 3, 32, 32) and ct == {0: 32, 1: 32}
    first = next(iter(_source().loaders(10)[1]))[0]            # test batches of 10: label 0 is every second row
    assert torch.equal(xt[:5], first[0::2])
    for a, b in zip(plain.loaders(16)[0], asked.loaders(16)[0]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_previews_do_not_change_the_training(tmp_path):
    from PIL import Image
    from eoe_amd.imgrid import image_grid
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    losses = {}
    for previews in (False, True):
        torch.manual_seed(0)
        d = tmp_path / str(previews)
        tr = HSCTrainer(CNN32(bias=True), dataset=_source(), epochs=1, lr=1e-3, batch_size=32, logger=JsonLogger(str(d)),
                        previews=previews)
        tr.run()
        losses[previews] = list(tr.last_losses)
        pngs = sorted(f for f in os.listdir(d) if f.endswith(".png"))
        assert pngs == (["eval_cls0-0_preview.png", "training_cls0-0_preview.png"] if previews else [])
    assert len(losses[True]) == 2 and losses[True] == losses[False]
    prev, counts = _source().preview(40, True)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "True" / "training_cls0-0_preview.png")),
                          image_grid(prev, nrow=40).cpu().numpy())
    assert json.load(open(tmp_path / "True" / "training_cls0-0_preview.headers.json")) == ["64", "40"]
    assert json.load(open(tmp_path / "True" / "eval_cls0-0_preview.headers.json")) == ["0: 32", "1: 32"]
