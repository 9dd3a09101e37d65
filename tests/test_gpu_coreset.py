"""GPU tier: `eoe_feature_coreset` (csrc/coreset.hip) -- centres, radii, assignment and distances against the float64 NumPy statement
(`coreset.kcenter_np`) byte for byte on integer-valued features at every edge of the row map (tests/coreset_util.py), ties, strided
and unaligned rows, non-finite rows, the derived rounding bound at every step on real-valued features, repeatability under a dirty
scratch, consistency with `feature_knn`, `kcenter` on both routes, and the trainer's `knn_coreset` on a small CNN32 task."""
import json
import math
import os

import numpy as np
import pytest
import torch

import coreset_util
from eoe_amd import coreset, neighbors

pytestmark = pytest.mark.gpu

SENTINEL = -7
GUARD = 64


def raw(x, m, start=0, fill=0xA5, pad=0, shift=0):
    """one `eoe_feature_coreset` call.  The five outputs sit between guard words pre-filled with SENTINEL, the scratch is pre-filled
    with the byte `fill`.  pad > 0: the rows lie `D + pad` apart and the padding is NaN; shift = 1: the features start 4 bytes past a
    16-byte boundary (the element-load path).  Returns (idx int32 [m], radius fp32 [m], assign int32 [n], d2min fp32 [n], counts [2])
    on the host."""
    from eoe_amd._lib import check, lib
    n, D = x.shape
    ld = D + pad
    buf = torch.full((n * ld + 4 + shift,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + n * ld].view(n, ld)
    view[:, :D] = torch.from_numpy(x).cuda()
    sizes = {"idx": m, "radius": m, "assign": n, "d2min": n, "counts": 2}
    out = {name: torch.full((size + 2 * GUARD,), SENTINEL, dtype=torch.float32 if name in ("radius", "d2min") else torch.int32, device="cuda")
           for name, size in sizes.items()}
    need = lib.eoe_feature_coreset_scratch_bytes(n, D, m)
    assert need >= 8 * m + 4 * n
    scratch = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    check(lib.eoe_feature_coreset(view.data_ptr(), ld, n, D, m, start, *[out[name][GUARD:].data_ptr() for name in sizes],
                                  scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "eoe_feature_coreset")
    host = {name: t.cpu().numpy() for name, t in out.items()}
    for name, size in sizes.items():
        a = host[name]
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + size:] == SENTINEL).all(), f"{name}: written outside its {size} entries"
    return tuple(host[name][GUARD:GUARD + size] for name, size in sizes.items())


def same_bytes(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def test_the_covering_table_holds_every_edge_value():
    assert coreset_util.cover_is_complete()


@pytest.mark.parametrize("n,D,m,start", coreset_util.COVER)
def test_integer_features_give_numpys_selection_byte_for_byte(n, D, m, start):
    x = coreset_util.exact_features(n, D, 1000 + 7 * n + D)
    idx, radius, assign, d2min, counts = raw(x, m, start)
    assert counts.tolist() == [0, 0]
    coreset_util.check_exact(idx, radius, assign, d2min, x, m, start, f"{n}x{D} m={m} start={start}")


@pytest.mark.parametrize("n", [129, 1025])
def test_values_in_minus_one_to_one_at_three_columns_are_almost_all_ties(n):
    x = coreset_util.exact_features(n, 3, 5 + n, -1, 1)
    idx, radius, assign, d2min, _ = raw(x, n)
    assert (radius == 0).sum() >= n - 27                                             # 27 distinct points: every other row is a duplicate
    assert sorted(idx.tolist()) == list(range(n))
    coreset_util.check_exact(idx, radius, assign, d2min, x, n, 0, f"ties n={n}")


@pytest.mark.parametrize("n,D,m", [(33, 64, 33), (65, 65, 9), (129, 515, 16), (31, 4, 31)])
def test_strided_and_unaligned_rows_give_the_bytes_of_contiguous_ones(n, D, m):
    x = coreset_util.exact_features(n, D, 11 + n)
    x += coreset_util.real_features(n, D, 12 + n, 0.25)                                # real values: the summation order shows in the bytes
    base = raw(x, m, 1)
    for pad in (1, 4):
        for shift in (0, 1):
            assert same_bytes(raw(x, m, 1, pad=pad, shift=shift), base), (pad, shift)
    assert same_bytes(raw(x, m, 1, pad=0, shift=1), base)


def test_non_finite_rows_are_never_centres_and_are_counted():
    n, D = 67, 65
    x = coreset_util.exact_features(n, D, 31)
    bad = {0: np.nan, 40: np.inf, n - 1: -np.inf}
    for row, v in bad.items():
        x[row, (7 * row) % D] = v
    for m in (5, n - 3, n):
        idx, radius, assign, d2min, counts = raw(x, m, 1)
        assert counts.tolist() == [3, 0]
        assert not np.isin(idx, list(bad)).any()
        assert (assign[list(bad)] == -1).all() and np.isnan(d2min[list(bad)]).all()
        coreset_util.check_exact(idx, radius, assign, d2min, x, m, 1, f"non-finite m={m}")
    idx, radius, _, _, _ = raw(x, n, 1)                                               # 64 eligible rows for 67 centres
    assert (idx[:n - 3] >= 0).all() and sorted(idx[:n - 3].tolist()) == [i for i in range(n) if i not in bad]
    assert (idx[n - 3:] == -1).all() and np.isnan(radius[n - 3:]).all()
    for start in bad:                                                                 # a non-finite start row: flagged, and kcenter raises
        assert raw(x, 4, start)[4].tolist() == [3, 1]
        with pytest.raises(ValueError, match="start row"):
            coreset.kcenter(torch.from_numpy(x).cuda(), 4, start)


@pytest.mark.parametrize("D", [3, 64, 515, 2048])
def test_real_features_choose_the_farthest_row_within_the_rounding_bound_at_every_step(D):
    for mag, off in ((1.0, 0.0), (1e3, 1e3)):                                        # the second: where the expansion form would cancel
        x = coreset_util.real_features(1025, D, 21 + D, mag, off)
        idx, radius, assign, d2min, counts = raw(x, 64, 3)
        assert counts.tolist() == [0, 0] and idx[0] == 3
        ratio, err = coreset_util.check_real(idx, radius, d2min, x, f"1025x{D} magnitude {mag} offset {off}")
        print(f"coreset real 1025x{D} mag={mag} off={off}: smallest chosen / farthest = {ratio:.9f}, worst error / gamma = {err:.4f}")
        assert ((assign >= 0) & (assign < 64)).all() and (assign[idx] == np.arange(64)).all()


def test_two_runs_over_different_scratch_fills_give_the_same_bytes():
    x = coreset_util.real_features(2051, 65, 41)
    a, b = raw(x, 300, 5, fill=0x00), raw(x, 300, 5, fill=0xA5)
    assert same_bytes(a, b)


def test_the_whole_set_as_its_own_coreset_gives_feature_knn_the_same_neighbours():
    x, q, k = coreset_util.exact_features(300, 65, 51), coreset_util.exact_features(33, 65, 52), 5
    xt, qt = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    cs = coreset.kcenter(xt, 300)
    assert sorted(cs.idx.tolist()) == list(range(300))
    full, sub = neighbors.feature_knn(qt, xt, k), neighbors.feature_knn(qt, xt[cs.idx], k)
    assert torch.equal(full.d2, sub.d2)                                               # ascending already: the sorted rows
    back = cs.idx[sub.idx]                                                            # rows of x
    assert torch.equal(((qt[:, None, :] - xt[back]) ** 2).sum(-1), full.d2)
    # the same rows wherever no tie decides one: none among the k returned, none between the k-th and the first row left out (equal
    # distances go to the lowest reference index, and the coreset's order is another one)
    more = neighbors.feature_knn(qt, xt, k + 1).d2
    distinct = (more[:, 1:] != more[:, :-1]).all(dim=1)
    assert distinct.any() and torch.equal(back[distinct], full.idx[distinct])


def test_kcenter_on_device_tensors_is_the_raw_route_and_on_cpu_tensors_numpy():
    from eoe_amd._lib import lib
    x = coreset_util.exact_features(130, 65, 61)
    xt = torch.from_numpy(x).cuda()
    want = coreset.kcenter_np(x, 17, 2)
    got = coreset.kcenter(xt, 17, 2)
    assert got.idx.dtype == torch.int64 and got.assign.dtype == torch.int64 and got.radius.dtype == torch.float32 and got.idx.is_cuda
    assert np.array_equal(got.idx.cpu().numpy(), want[0]) and np.array_equal(got.assign.cpu().numpy(), want[2])
    assert np.array_equal(got.d2min.cpu().numpy(), want[3].astype(np.float32)) and got.nonfinite == 0
    assert got.cover() == math.sqrt(want[3].max()) and got.sizes().tolist() == np.bincount(want[2], minlength=17).tolist()
    assert coreset.kcenter(xt, 0.125, 2).idx.tolist() == want[0].tolist()             # ceil(0.125 * 130) = 17
    cpu = coreset.kcenter(xt.cpu(), 17, 2)
    assert not cpu.idx.is_cuda and np.array_equal(cpu.idx.numpy(), want[0]) and cpu.as_dict() == got.as_dict()
    strided = torch.full((130, 72), float("nan"), device="cuda")
    strided[:, :65] = xt
    assert coreset.kcenter(strided[:, :65], 17, 2).idx.tolist() == want[0].tolist()
    need = lib.eoe_feature_coreset_scratch_bytes(130, 65, 17)
    own = torch.full((need + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    assert coreset.kcenter_device(xt, 17, 2, scratch=own)[0].tolist() == want[0].tolist()
    for wrong in (own[:need - 16], own[1:], own.to(torch.int8)):
        with pytest.raises(ValueError, match="scratch"):
            coreset.kcenter_device(xt, 17, 2, scratch=wrong)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        coreset.kcenter_device(xt.cpu(), 17)
    for n, D, m in ((0, 4, 1), (4, 0, 1), (4, 2049, 1), (4, 4, 0), (4, 4, 5), (1 << 24, 4, 1)):
        assert lib.eoe_feature_coreset_scratch_bytes(n, D, m) == 0


def test_the_c_abi_refuses_arguments_outside_its_ranges_before_any_launch():
    from eoe_amd._lib import lib
    x = torch.zeros((4, 4), device="cuda")
    out = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def call(ld=4, n=4, D=4, m=2, start=0):
        p = out.data_ptr()
        return lib.eoe_feature_coreset(x.data_ptr(), ld, n, D, m, start, p, p, p, p, p, scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for kw in (dict(D=0), dict(D=2049), dict(ld=3), dict(n=0), dict(n=1 << 24), dict(m=0), dict(m=5), dict(start=-1), dict(start=4)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ trainer
ROWS_CLASSES = [0, 1] * 12


def _task():
    """the two-class set of 24 32 x 32 images tests/test_gpu_knn.py trains on and its task 'class 0 is normal': 12 normal rows"""
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


def test_trainer_searches_and_scores_against_the_coreset_and_logs_it(tmp_path):
    import eoe_amd
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    shots = {}

    def run(name, **extra):
        torch.manual_seed(2)
        np.random.seed(2)
        tr = TRAINER["hsc"](_model(), dataset=_task(), logger=JsonLogger(str(tmp_path / name)), extremes=3, neighbors=3, knn_baseline=True,
                            **extra, **KW)
        real = tr.logger.logimg
        tr.logger.logimg = lambda nm, *a, **k: shots.setdefault((name, nm), real(nm, *a, **k))
        tr.coresets["stale"] = None
        tr.run(run_seeds=1)
        return tr, sorted(os.listdir(tmp_path / name))
    on, files_on = run("on", knn_coreset=0.25)
    off, files_off = run("off")
    key = "eval_cls0_it0"
    assert list(on.coresets) == [key] and off.coresets == {}
    assert not any("_coreset" in f for f in files_off) and set(files_off) <= set(files_on)
    assert sorted(set(files_on) - set(files_off)) == ["eval_cls0-a_it0_coreset.png", "eval_cls0_it0_coreset.json"]
    cs = on.coresets[key]
    n_normal = 12
    m = math.ceil(0.25 * n_normal)
    assert cs.m == m == 3 and cs.n == n_normal and cs.idx[0] == 0 and cs.nonfinite == 0
    logged = json.load(open(tmp_path / "on" / "eval_cls0_it0_coreset.json"))
    normal_rows = _task().normal_index.numpy()
    centres = logged["centres"]
    assert len(centres) == m and len(set(centres)) == m and set(centres) <= set(normal_rows.tolist())
    assert centres == normal_rows[cs.idx.cpu().numpy()].tolist() and sum(logged["sizes"]) == n_normal and len(logged["radius"]) == m - 1
    near = json.load(open(tmp_path / "on" / "eval_cls0_it0_extremes_neighbors.json"))
    assert near["k"] == 3 and all(len(r["neighbors"]) == 3 and {i for i, _ in r["neighbors"]} <= set(centres) for r in near["rows"])
    res = on.knn_results[0]
    assert res == json.load(open(tmp_path / "on" / "eval_cls0_it0_knn.json"))
    assert res["coreset"]["m"] == m and res["coreset"]["n"] == n_normal
    assert math.isfinite(res["coreset"]["cover"]) and res["coreset"]["cover"] > 0 and res["coreset"]["cover"] == cs.cover()
    assert 0.0 <= res["auc"] <= 1.0 and 0.0 <= res["avg_prec"] <= 1.0
    assert "coreset" not in off.knn_results[0] and (res["k"], res["n_normal"]) == (3, n_normal)
    pic = shots[("on", "eval_cls0-a_it0_coreset")]
    assert pic.dtype == np.uint8 and pic.shape[2] == 3 and pic.max() > 0
    # m is clamped to [neighbors, n_normal]
    few = TRAINER["hsc"](_model(), dataset=_task(), extremes=3, neighbors=3, knn_coreset=1, **KW)
    few.run(run_seeds=1)
    assert few.coresets[key].m == 3
    eoe_amd.set_compute_dtype(old)
