"""GPU tier: `eoe_feature_knn` (csrc/knn.hip) -- indices and distances against the float64 NumPy statement (`neighbors.knn_np`) bit for
bit on integer-valued features at every tile, chunk and k edge (tests/knn_util.py), the rounding bound on real-valued ones, strided
and unaligned inputs, non-finite rows, repeatability under a dirty scratch, `feature_knn` on both routes, and the trainer's
`neighbors=k` / `knn_baseline=True` on a small CNN32 task."""
import json
import os

import numpy as np
import pytest
import torch

import knn_util
from eoe_amd import metrics, neighbors

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 64


def raw(q, r, k, fill=0xA5, pad=0, shift=0):
    """one `eoe_feature_knn` call.  The outputs sit between guard words pre-filled with SENTINEL, the scratch is pre-filled with the
    byte `fill`.  pad > 0: the rows lie `D + pad` apart and the padding is NaN; shift = 1: the features start 4 bytes past a 16-byte
    boundary (the element-load path).  Returns (idx int32 [nq, k], d2 fp32 [nq, k], counts [2]) on the host."""
    from eoe_amd._lib import check, lib
    (nq, D), nr = q.shape, r.shape[0]

    def place(x):
        n, ld = x.shape[0], D + pad
        buf = torch.full((n * ld + 4 + shift,), float("nan"), dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + n * ld].view(n, ld)
        view[:, :D] = torch.from_numpy(x).cuda()
        return buf, view, ld

    qb, qv, ldq = place(q)
    rb, rv, ldr = place(r)
    idx = torch.full((nq * k + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    d2 = torch.full((nq * k + 2 * GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    counts = torch.full((2 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    scratch = torch.full((lib.eoe_feature_knn_scratch_bytes(nq, nr, D, k),), fill, dtype=torch.uint8, device="cuda")
    check(lib.eoe_feature_knn(qv.data_ptr(), ldq, rv.data_ptr(), ldr, nq, nr, D, k, idx[GUARD:].data_ptr(), d2[GUARD:].data_ptr(),
                              counts[GUARD:].data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "eoe_feature_knn")
    idx, d2, counts = idx.cpu().numpy(), d2.cpu().numpy(), counts.cpu().numpy()
    for name, a, n in (("idx", idx, nq * k), ("d2", d2, nq * k), ("counts", counts, 2)):
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + n:] == SENTINEL).all(), f"{name}: written outside its {n} entries"
    return idx[GUARD:GUARD + nq * k].reshape(nq, k), d2[GUARD:GUARD + nq * k].reshape(nq, k), counts[GUARD:GUARD + 2].tolist()


def test_the_covering_table_holds_every_edge_value():
    assert knn_util.cover_is_complete()


@pytest.mark.parametrize("nq,nr,D,k", knn_util.COVER)
def test_integer_features_give_numpys_stable_argsort_bit_for_bit(nq, nr, D, k):
    q, r = knn_util.exact_features(nq, D, 1000 + nq + D), knn_util.exact_features(nr, D, 2000 + nr + k)
    idx, d2, counts = raw(q, r, k)
    assert counts == [0, 0]
    knn_util.check_exact(idx, d2, q, r, k, f"{nq}x{nr}x{D} k={k}")


@pytest.mark.parametrize("nr,k", [(3, 5), (129, 64), (1025, 16), (2051, 64)])
def test_values_in_minus_one_to_one_at_three_columns_are_almost_all_ties(nr, k):
    q, r = knn_util.exact_features(33, 3, 5, -1, 1), knn_util.exact_features(nr, 3, 6 + nr, -1, 1)
    idx, d2, _ = raw(q, r, k)
    if nr > k:
        assert (np.diff(d2, axis=1) == 0).mean() > 0.5
    knn_util.check_exact(idx, d2, q, r, k, f"ties nr={nr} k={k}")
    if nr < k:
        assert (idx[:, nr:] == -1).all() and np.isposinf(d2[:, nr:]).all()


@pytest.mark.parametrize("nq,nr,D,k", [(33, 1025, 65, 5), (130, 129, 63, 16), (31, 2051, 515, 64), (1, 127, 3, 1)])
def test_strided_and_unaligned_inputs_give_the_bytes_of_contiguous_ones(nq, nr, D, k):
    q, r = knn_util.exact_features(nq, D, 11), knn_util.exact_features(nr, D, 12)
    base = raw(q, r, k)
    knn_util.check_exact(base[0], base[1], q, r, k, "contiguous")
    for pad, shift in ((4 - D % 4 if D % 4 else 4, 0), (1, 0), (0, 1), (3, 1)):
        got = raw(q, r, k, pad=pad, shift=shift)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2] == base[2], (pad, shift)


@pytest.mark.parametrize("nq,nr,D,k", knn_util.REAL_SHAPES)
def test_real_features_stay_within_the_rounding_bound_for_every_row(nq, nr, D, k):
    cases = [(m, 0.0) for m in knn_util.MAGNITUDES] + [(1.0, 100.0)]                   # the last: a common offset, the cancellation case
    for mag, off in cases:
        q, r = knn_util.real_features(nq, D, 21, mag, off), knn_util.real_features(nr, D, 22, mag, off)
        idx, d2, counts = raw(q, r, k)
        assert counts == [0, 0]
        worst = knn_util.check_real(idx, d2, q, r, k, f"{nq}x{nr}x{D} k={k} magnitude {mag} offset {off}")
        print(f"knn real {nq}x{nr}x{D} k={k} mag={mag} off={off}: worst |err| / B = {worst:.4f}")


def test_non_finite_rows_on_both_sides_of_a_chunk_edge():
    nq, nr, D, k = 130, 2051, 65, 16
    q, r = knn_util.exact_features(nq, D, 31), knn_util.exact_features(nr, D, 32)
    for row, col, v in ((0, 0, np.nan), (1023, 64, np.inf), (1024, 3, -np.inf), (1025, 33, np.nan), (2050, 1, np.inf)):
        r[row, col] = v
    for row, col, v in ((0, 64, np.nan), (127, 0, np.inf), (128, 31, -np.inf)):
        q[row, col] = v
    idx, d2, counts = raw(q, r, k)
    assert counts == [3, 5]
    want_idx, want_d2, bad = neighbors.knn_np(q, r, k)
    assert bad == (3, 5)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(d2.astype(np.float64), want_d2)                      # NaN rows compare equal here
    assert not np.isin(idx, [0, 1023, 1024, 1025, 2050]).any()
    for row in (0, 127, 128):
        assert (idx[row] == -1).all() and np.isnan(d2[row]).all()
    # every reference non-finite: nothing to return
    r2 = knn_util.exact_features(3, D, 33)
    r2[:, 0] = np.nan
    idx, d2, counts = raw(q[1:32], r2, 5)
    assert counts == [0, 3] and (idx == -1).all() and np.isposinf(d2).all()


def test_four_runs_over_different_scratch_fills_give_the_same_bytes():
    q, r = knn_util.real_features(130, 65, 41), knn_util.real_features(2051, 65, 42)
    runs = [raw(q, r, 16, fill) for fill in (0x00, 0x00, 0xFF, 0x5A)]
    for other in runs[1:]:
        assert other[0].tobytes() == runs[0][0].tobytes() and other[1].tobytes() == runs[0][1].tobytes() and other[2] == runs[0][2]


def test_feature_knn_on_device_tensors_is_the_raw_route_and_on_cpu_tensors_numpy():
    from eoe_amd._lib import lib
    q, r, k = knn_util.exact_features(33, 65, 51), knn_util.exact_features(1025, 65, 52), 5
    qt, rt = torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda()
    idx, d2, counts = raw(q, r, k)
    got = neighbors.feature_knn(qt, rt, k)
    assert got.idx.dtype == torch.int64 and got.d2.dtype == torch.float32 and got.idx.is_cuda and got.nonfinite == (0, 0)
    assert np.array_equal(got.idx.cpu().numpy(), idx) and got.d2.cpu().numpy().tobytes() == d2.tobytes()
    need = lib.eoe_feature_knn_scratch_bytes(33, 1025, 65, k)
    own = torch.full((need + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    a = neighbors.feature_knn_device(qt, rt, k, scratch=own)
    assert np.array_equal(a[0].cpu().numpy(), idx) and a[1].cpu().numpy().tobytes() == d2.tobytes() and a[2].tolist() == counts
    with pytest.raises(ValueError, match="scratch"):
        neighbors.feature_knn_device(qt, rt, k, scratch=own[:need - 16])
    with pytest.raises(RuntimeError, match="GPU tensors"):
        neighbors.feature_knn_device(qt.cpu(), rt, k)
    strided = torch.full((33, 72), float("nan"), device="cuda")
    strided[:, :65] = qt
    assert np.array_equal(neighbors.feature_knn(strided[:, :65], rt, k).idx.cpu().numpy(), idx)
    cpu = neighbors.feature_knn(qt.cpu(), rt.cpu(), k)
    want = neighbors.knn_np(q, r, k)
    assert np.array_equal(cpu.idx.numpy(), want[0]) and np.array_equal(cpu.d2.numpy(), want[1].astype(np.float32)) and not cpu.idx.is_cuda
    assert np.array_equal(cpu.idx.numpy(), idx)
    score = neighbors.knn_score(got, "mean")
    assert score.is_cuda and np.allclose(score.cpu().numpy(), np.sqrt(want[1]).mean(1), rtol=1e-6)
    assert np.array_equal(neighbors.knn_score(got, "kth").cpu().numpy(), np.sqrt(d2[:, -1]))
    none = neighbors.feature_knn(qt[:0], rt, k)
    assert tuple(none.idx.shape) == (0, k) and none.nonfinite == (0, 0)
    empty = neighbors.feature_knn(qt, rt[:0], k)
    assert (empty.idx == -1).all() and torch.isinf(empty.d2).all()


# ------------------------------------------------------------------------------------------------ source and trainer
ROWS_CLASSES = [0, 1] * 12


def _task():
    """a fresh two-class LabelledImageSet of 24 32 x 32 images (the test split is the training images, so both routes of a source can
    be compared on the same picture) and its task 'class 0 is normal': 12 normal rows, the even ones"""
    from eoe_amd.data import LabelledImageSet
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 32), indexing="ij")

    def make(k, n):
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)
        return (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, 32, 32, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    cls = torch.tensor(ROWS_CLASSES)
    imgs = torch.stack([make(int(c), 1)[0] for c in cls])
    lset = LabelledImageSet(imgs, cls, imgs, cls, make(1, 16), ["a", "b"], 32, mean=(0.5,) * 3, std=(0.25,) * 3)
    return lset.source([0], seed=3)


def _model():
    from eoe_amd.models import CNN32
    torch.manual_seed(0)
    return CNN32(bias=True)


KW = dict(epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["a"])


def test_normal_inputs_are_the_test_route_on_the_normal_rows_and_leave_training_alone():
    import eoe_amd
    from eoe_amd.training import TRAINER
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    ds = _task()
    assert ds.n_normal == 12 and ds.normal_index.tolist() == list(range(0, 24, 2))
    pos = torch.tensor([3, 0, 11, 3])
    imgs, ids = ds.normal_inputs(pos)
    assert ids.tolist() == [6, 0, 22, 6] and imgs.shape == (4, 3, 32, 32) and imgs.dtype == torch.float32 and imgs.is_cuda
    assert torch.equal(imgs, ds.test_images(ids))                                   # the training images ARE the test split here
    assert torch.equal(ds.normal_pictures(pos), ds.test_pictures(ids))
    assert torch.equal(ds.normal_inputs(pos)[0], imgs)                              # no draw: twice the same

    def train(calls):
        d = _task()
        for _ in range(calls):
            d.normal_inputs(torch.arange(12))
            d.normal_pictures([1, 2])
        torch.manual_seed(1)
        tr = TRAINER["hsc"](_model(), dataset=d, **KW)
        model, _ = tr.train_cls(_model(), d, 0, "a", 0)
        return model.state_dict()
    plain, called = train(0), train(3)
    assert plain.keys() == called.keys() and all(torch.equal(plain[n], called[n]) for n in plain)
    eoe_amd.set_compute_dtype(old)


def test_trainer_keeps_and_logs_the_neighbours_and_scores_the_knn_baseline(tmp_path):
    import copy
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    ds = _task()
    torch.manual_seed(1)
    model, _ = TRAINER["hsc"](_model(), dataset=ds, **KW).train_cls(_model(), ds, 0, "a", 0)
    on = TRAINER["hsc"](_model(), dataset=ds, logger=JsonLogger(str(tmp_path / "on")), extremes=3, neighbors=4, knn_baseline=True, **KW)
    off = TRAINER["hsc"](_model(), dataset=ds, logger=JsonLogger(str(tmp_path / "off")), extremes=3, **KW)
    shots = {}
    real = on.logger.logimg
    on.logger.logimg = lambda name, *a, **k: shots.setdefault(name, real(name, *a, **k))
    res_on, res_off = on.eval_cls(copy.deepcopy(model), ds, 0, "a", 0), off.eval_cls(copy.deepcopy(model), ds, 0, "a", 0)
    key = "eval_cls0_it0"
    assert list(on.neighbors) == [key] and off.neighbors == {} and off.knn_results == {}
    neigh = on.neighbors[key]
    rows, per, _ = on._extreme_rows(on.extremes[key])
    assert per == 3 and len(rows) == 12
    assert neigh.idx.shape == (12, 4) and neigh.d2.shape == (12, 4) and neigh.idx.dtype == torch.int64 and neigh.nonfinite == (0, 0)
    # the same search over features recomputed here, in the batches the trainer used
    m = copy.deepcopy(model).cuda().eval()
    on._normalize_hook(m, ds)
    refs = neighbors.embed(m, [(ds.normal_inputs(torch.arange(12))[0],)], trainer=on)
    queries = neighbors.embed(m, [ds.test_inputs(rows)[:2]], trainer=on)
    assert refs.shape == (12, 256) and queries.shape == (12, 256)
    want_idx, want_d2, _ = neighbors.knn_np(queries, refs, 4)
    assert np.array_equal(neigh.idx.cpu().numpy(), want_idx)
    knn_util.check_real(neigh.idx.cpu().numpy(), neigh.d2.cpu().numpy(), queries.cpu().numpy(), refs.cpu().numpy(), 4, "trainer")
    # files: the JSON names dataset rows, the picture holds one image and its four neighbours per row
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off")}
    extra = sorted(set(files["on"]) - set(files["off"]))
    assert set(files["off"]) <= set(files["on"])
    assert extra == ["eval_cls0-a_it0_extremes_neighbors.png", "eval_cls0_it0_extremes_neighbors.json", "eval_cls0_it0_knn.json"], extra
    logged = json.load(open(tmp_path / "on" / "eval_cls0_it0_extremes_neighbors.json"))
    assert logged["k"] == 4 and [r["row"] for r in logged["rows"]] == [int(x) for x in rows]
    normal_rows = ds.normal_index.numpy()
    for r, ids, dist in zip(logged["rows"], want_idx, neigh.dist().cpu().numpy()):
        assert [n[0] for n in r["neighbors"]] == normal_rows[ids].tolist() and [n[1] for n in r["neighbors"]] == [float(x) for x in dist]
    # a normal test image is its own nearest training image (the test split is the training images): distance 0 up to rounding
    own = [i for i, row in enumerate(rows) if ROWS_CLASSES[int(row)] == 0]
    assert own and all(logged["rows"][i]["neighbors"][0][0] == int(rows[i]) for i in own)
    pic = shots["eval_cls0-a_it0_extremes_neighbors"]
    assert pic.shape == ((32 + 2) * 12 + 2, (32 + 2) * 5 + 2, 3) and pic.dtype == np.uint8 and pic.max() > 0
    # the baseline: AUC of the mean distance to the 4 nearest normal features over the whole test split
    test_feats = neighbors.embed(m, [ds.test_inputs(torch.arange(lo, min(lo + 16, 24)))[:2] for lo in (0, 16)], trainer=on)
    _, d2_all, _ = neighbors.knn_np(test_feats, refs, 4)
    score = np.sqrt(d2_all).mean(1)
    res = on.knn_results[0]
    assert res == json.load(open(tmp_path / "on" / "eval_cls0_it0_knn.json"))
    assert (res["k"], res["n_normal"], res["D"]) == (4, 12, 256)
    assert abs(res["auc"] - metrics.roc_auc(ds.test_y.cpu().numpy(), score)) <= 1e-6
    assert abs(res["avg_prec"] - metrics.average_precision(ds.test_y.cpu().numpy(), score)) <= 1e-6
    # nothing else moved
    for f in files["off"]:
        if os.path.isfile(tmp_path / "off" / f):
            assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "on" / f).read_bytes(), f
    assert (res_on[0].auc, res_on[1].avg_prec) == (res_off[0].auc, res_off[1].avg_prec)
    # a classifier head is refused before scoring
    from eoe_amd.models import CNN32
    asked = []
    with pytest.raises(NotImplementedError, match="a classifier head has no embedding"):
        clf = TRAINER["hsc"](CNN32(clf=True), dataset=ds, extremes=3, neighbors=4, **KW)
        clf.compute_anomaly_score = lambda *a, **k: asked.append(1)
        clf.eval_cls(CNN32(clf=True), ds, 0, "a", 0)
    assert not asked
    eoe_amd.set_compute_dtype(old)


def test_a_run_with_the_options_at_their_defaults_leaves_the_same_files_and_results(tmp_path):
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")

    def run(name, **extra):
        torch.manual_seed(2)
        np.random.seed(2)
        tr = TRAINER["hsc"](_model(), dataset=_task(), logger=JsonLogger(str(tmp_path / name)), extremes=3, **extra, **KW)
        out = tr.run(run_seeds=1)[1]
        assert tr.neighbors == {} and tr.knn_results == {}
        return out, sorted(os.path.relpath(os.path.join(d, f), tmp_path / name) for d, _, fs in os.walk(tmp_path / name) for f in fs)
    (res_a, files_a), (res_b, files_b) = run("without"), run("defaults", neighbors=0, knn_baseline=False)
    assert files_a == files_b and "results.json" in files_a and not any("neighbors" in f or "knn" in f for f in files_a)
    assert (tmp_path / "without" / "results.json").read_bytes() == (tmp_path / "defaults" / "results.json").read_bytes()
    assert res_a == res_b
    # with the options on, `run` fills one entry per evaluation and starts the next run empty
    torch.manual_seed(2)
    tr = TRAINER["hsc"](_model(), dataset=_task(), extremes=3, neighbors=4, knn_baseline=True, **KW)
    tr.neighbors["stale"] = None
    res_c = tr.run(run_seeds=1)[1]
    assert list(tr.neighbors) == ["eval_cls0_it0"] and tr.neighbors["eval_cls0_it0"].idx.shape == (12, 4) and list(tr.knn_results) == [0]
    assert res_c["cls_aucs"] == res_a["cls_aucs"]
    eoe_amd.set_compute_dtype(old)
