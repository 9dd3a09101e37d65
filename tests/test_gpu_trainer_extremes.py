"""GPU tier: `ADTrainer(extremes=k)` on a tiny CNN32 task -- the kept `Extremes`, the logged JSON and the picture against the NumPy
ranking of the scores the same evaluation logs, `ResidentImageSource.test_images`, and the default (0) against a run with the option:
the same files otherwise, the same results."""
import json
import os

import numpy as np
import pytest
import torch

import topk_util
from eoe_amd import metrics

pytestmark = pytest.mark.gpu

K = 5
N_TEST = 40
ROWS = ["nominal most", "nominal least", "anomalous most", "anomalous least"]


def _source(anomalous=None):
    """a resident 32 x 32 task with 40 test images: label 1 at every fourth row (10 of them), or at the listed rows"""
    from eoe_amd.data import ResidentImageSource
    rng = np.random.default_rng(17)
    img = lambda n, lo, hi: torch.from_numpy(rng.integers(lo, hi, (n, 32, 32, 3)).astype(np.uint8))    # noqa: E731
    labels = torch.zeros(N_TEST, dtype=torch.int64)
    labels[list(range(3, N_TEST, 4)) if anomalous is None else anomalous] = 1
    return ResidentImageSource(img(48, 60, 160), img(32, 0, 256), img(N_TEST, 0, 256), labels, crop=32, padding=2, seed=3)


def _run(tmp_path, name, extremes, source=None):
    from eoe_amd.models import CNN32
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(11)
    logdir = str(tmp_path / name)
    kw = {} if extremes is None else {"extremes": extremes}
    tr = HSCTrainer(CNN32(bias=True), dataset=source if source is not None else _source(), epochs=1, lr=1e-3, batch_size=16,
                    logger=JsonLogger(logdir), **kw)
    _, res = tr.run()
    return tr, res, logdir


def _logged_scores(logdir):
    with open(os.path.join(logdir, "eval_cls0_it0_anomaly_scores.json")) as f:
        logged = json.load(f)
    idc = np.array([int(i) for i in logged], dtype=np.int64)
    return idc, np.array(list(logged.values()), dtype=np.float64).astype(np.float32)


def test_test_images_are_the_test_loaders_images_and_draw_nothing():
    src = _source()
    allx = torch.cat([b[0] for b in src.loaders(16)[1]])
    state = src._g.get_state().clone(), src._step
    rows = [39, 0, 7, 7, 12]
    got = src.test_images(rows)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (5, 3, 32, 32) and torch.equal(got, allx[rows])
    assert torch.equal(src.test_images(np.array(rows)), got) and torch.equal(src.test_images(torch.tensor(rows)), got)
    assert torch.equal(src._g.get_state(), state[0]) and src._step == state[1]
    with pytest.raises(IndexError):
        src.test_images([N_TEST])
    with pytest.raises(IndexError):
        src.test_images([-1])


def test_trainer_extremes_agree_with_its_logged_scores_and_the_default_is_untouched(tmp_path):
    from PIL import Image
    from eoe_amd.imgrid import image_grid
    tr, res, logdir = _run(tmp_path, "on", K)
    plain, res_plain, logdir_plain = _run(tmp_path, "off", 0)
    default, res_default, logdir_default = _run(tmp_path, "default", None)
    # ---- the option changes nothing else: results, losses, every other file
    assert res == res_plain == res_default and tr.last_losses == plain.last_losses == default.last_losses
    stem = "eval_cls0-0_it0_extremes"
    added = {"eval_cls0_it0_extremes.json", stem + ".png", stem + ".headers.json"}
    assert set(os.listdir(logdir)) - set(os.listdir(logdir_plain)) == added
    assert sorted(os.listdir(logdir_plain)) == sorted(os.listdir(logdir_default)) == sorted(set(os.listdir(logdir)) - added)
    assert not any("extremes" in f for f in os.listdir(logdir_plain))
    assert plain.extremes == {} and default.extremes == {} and plain.n_extremes == default.n_extremes == 0
    for f in ("eval_cls0_it0_anomaly_scores.json", "results.json"):
        with open(os.path.join(logdir, f), "rb") as a, open(os.path.join(logdir_plain, f), "rb") as b:
            assert a.read() == b.read()
    # ---- extremes=5: the kept object and the JSON equal the NumPy ranking of the scores the evaluation logged
    idc, s = _logged_scores(logdir)
    y = _source().test_y.cpu().numpy()[idc]
    assert idc.tolist() == list(range(N_TEST)) and np.isfinite(s).all()
    want = topk_util.reference(s, y, K)
    assert set(tr.extremes) == {"eval_cls0_it0"}
    ex = tr.extremes["eval_cls0_it0"]
    assert isinstance(ex, metrics.Extremes) and ex.num == (30, 10)
    topk_util.check_extremes(ex, s, want, K, "trainer", remap=idc)
    with open(os.path.join(logdir, "eval_cls0_it0_extremes.json")) as f:
        j = json.load(f)
    assert j == ex.as_dict() and list(j) == ["nominal", "anomalous"]
    for g, name in enumerate(("nominal", "anomalous")):
        assert j[name]["num"] == want[1][g]
        for end, key in enumerate(("most", "least")):
            w = want[0][g][end]
            assert [i for i, _ in j[name][key]] == idc[w].tolist()
            assert [np.float32(v) for _, v in j[name][key]] == s[w].tolist()
    # ---- the picture: four rows of five test images, in the lists' order
    rows = np.concatenate([idc[want[0][g][end]] for g in (0, 1) for end in (0, 1)])
    pic = np.asarray(Image.open(os.path.join(logdir, stem + ".png")))
    assert pic.shape == ((32 + 2) * 4 + 2, (32 + 2) * K + 2, 3)
    assert np.array_equal(pic, image_grid(_source().test_images(rows), nrow=K).cpu().numpy())
    with open(os.path.join(logdir, stem + ".headers.json")) as f:
        assert json.load(f) == [f"{r}: {m}" for r, m in zip(ROWS, (30, 30, 10, 10))]


def test_a_small_and_an_empty_group_shape_the_picture(tmp_path):
    from PIL import Image
    # three anomalous test images: every row is cut to three
    tr, _, logdir = _run(tmp_path, "small", K, _source(anomalous=[4, 9, 30]))
    ex = tr.extremes["eval_cls0_it0"]
    assert ex.num == (37, 3) and len(ex.most[0][0]) == K and len(ex.most[1][0]) == len(ex.least[1][0]) == 3
    assert sorted(ex.most[1][0].tolist()) == [4, 9, 30] and ex.most[1][0].tolist() == ex.least[1][0].tolist()[::-1]
    stem = os.path.join(logdir, "eval_cls0-0_it0_extremes")
    assert np.asarray(Image.open(stem + ".png")).shape == ((32 + 2) * 4 + 2, (32 + 2) * 3 + 2, 3)
    with open(stem + ".headers.json") as f:
        assert json.load(f) == [f"{r}: {m}" for r, m in zip(ROWS, (37, 37, 3, 3))]
    # no anomalous test image: no metrics, the JSON and two rows all the same
    tr, res, logdir = _run(tmp_path, "empty", K, _source(anomalous=[]))
    ex = tr.extremes["eval_cls0_it0"]
    assert ex.num == (N_TEST, 0) and ex.most[1][0].size == 0 and len(ex.least[0][0]) == K and res["cls_aucs"] == [[None]]
    stem = os.path.join(logdir, "eval_cls0-0_it0_extremes")
    assert np.asarray(Image.open(stem + ".png")).shape == ((32 + 2) * 2 + 2, (32 + 2) * K + 2, 3)
    with open(stem + ".headers.json") as f:
        assert json.load(f) == [f"{r}: {N_TEST}" for r in ROWS[:2]]
    with open(os.path.join(logdir, "eval_cls0_it0_extremes.json")) as f:
        assert json.load(f)["anomalous"] == {"most": [], "least": [], "num": 0}
