"""GPU tier: per-task normalisation on the device -- `eoe_set_moments_u8` against numpy's exact integer sums, `fit_statistics`
and `gcn_normalize` against the reference's results (fixture g20_normstats; rule in tests/normstats_util.py: K_NOISE_PARITY x the
reference's own fp32-vs-fp64 distance per case, fitted statistics floored at one fp32 ulp), the sources and the trainer in both
modes, and a K = 10 training trajectory behind GCN + Normalize."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import normstats_util as nu                                          # noqa: E402
import parity_util                                                   # noqa: E402
from oracle import fill as ofill, models as omodels                  # noqa: E402


@pytest.fixture(autouse=True)
def _restore_modes():
    import eoe_amd
    old = eoe_amd.compute_dtype()
    yield
    eoe_amd.set_compute_dtype(old)
    eoe_amd.set_parity_mode(False)


def _np_moments(u8):
    v = u8.astype(np.int64)
    m = v.shape[0]
    flat = v.reshape(m, -1)
    chan = np.stack([v.sum(axis=(1, 2)), (v * v).sum(axis=(1, 2))], axis=2)
    S, N = flat.sum(1), flat.shape[1]
    img = np.stack([flat.min(1), flat.max(1), np.abs(N * flat - S[:, None]).sum(1)], axis=1)
    return chan, img


def _case(case):
    name, idx = nu.stats_index(case)
    return nu.stats_set(name), idx


# ------------------------------------------------------------------------------------------------------------ 1. the statistics kernel
@pytest.mark.parametrize("case", nu.STATS_CASES + ("odd", "odd_gray", "big"))
def test_set_moments_equal_numpy_exactly(case):
    from eoe_amd.normalize import set_moments_u8
    if case == "odd":               # N = 189: not a multiple of 16, the byte-wise path
        u8, idx = ofill.fill_int("g20/odd", (5, 7, 9, 3), 0, 256).astype(np.uint8), np.array([4, 0, 2], dtype=np.int64)
    elif case == "odd_gray":
        u8, idx = ofill.fill_int("g20/odd_gray", (3, 5, 5, 1), 0, 256).astype(np.uint8), None
    elif case == "big":             # the MVTec-style image size, saturated values included
        u8, idx = ofill.fill_int("g20/big", (3, 224, 224, 3), 0, 256).astype(np.uint8), None
        u8[1] = 255
        u8[2, :, :, 1] = 0
    else:
        u8, idx = _case(case)
    dev = torch.from_numpy(u8).cuda()
    chan, img = set_moments_u8(dev, idx)
    chan2, img2 = set_moments_u8(dev, idx)
    want_chan, want_img = _np_moments(u8 if idx is None else u8[idx])
    assert chan.dtype == torch.int64 and img.dtype == torch.int64
    assert np.array_equal(chan.cpu().numpy(), want_chan) and np.array_equal(img.cpu().numpy(), want_img)
    assert torch.equal(chan, chan2) and torch.equal(img, img2)                       # run to run, bit for bit


def test_set_moments_bounds():
    """a row outside the set reads nothing and is marked; the Python wrapper refuses it before the launch"""
    from eoe_amd._lib import lib, check
    from eoe_amd.normalize import set_moments_u8
    u8 = torch.from_numpy(nu.stats_set("rect9")).cuda()
    with pytest.raises(IndexError):
        set_moments_u8(u8, [0, 9])
    with pytest.raises(IndexError):
        set_moments_u8(u8, [-1])
    idx = torch.tensor([1, 9, -3, 8], dtype=torch.int64, device="cuda")
    chan = torch.zeros((4, 3, 2), dtype=torch.int64, device="cuda")
    img = torch.zeros((4, 3), dtype=torch.int64, device="cuda")
    check(lib.eoe_set_moments_u8(u8.data_ptr(), 9, 64, 48, 3, idx.data_ptr(), 4, chan.data_ptr(), img.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream), "eoe_set_moments_u8")
    want_chan, want_img = _np_moments(nu.stats_set("rect9")[[1, 8]])
    assert (chan[1] == -1).all() and (chan[2] == -1).all() and (img[1] == -1).all() and (img[2] == -1).all()
    assert np.array_equal(chan[[0, 3]].cpu().numpy(), want_chan) and np.array_equal(img[[0, 3]].cpu().numpy(), want_img)


# ------------------------------------------------------------------------------------------------------------ 2. fit_statistics
@pytest.mark.parametrize("case", nu.STATS_CASES)
def test_fit_statistics_matches_the_reference(golden, case):
    from eoe_amd import fit_statistics
    g = golden("g20_normstats")
    u8, idx = _case(case)
    dev = torch.from_numpy(u8).cuda()
    for mode_str, mode in (("normalize", 0), ("gcn-normalize", 1), ("norm", 0), ("gcn-normalise", 1)):
        st = fit_statistics(dev, idx, mode_str)
        assert set(st) == {"mean", "std", "mode"} and type(st["mode"]) is int and len(st["mean"]) == u8.shape[3]
        assert all(type(v) is float for v in st["mean"] + st["std"])
        print("\n   " + nu.check_stats_dict(st, g, case, mode, "GPU "), end="")
    assert fit_statistics(dev, idx, "normalize") == fit_statistics(dev, idx, "Normalize")


# ------------------------------------------------------------------------------------------------------------ 3. the operator
def _op_input_dev(size):
    return torch.from_numpy(nu.op_input(size)).cuda()


@pytest.mark.parametrize("size", list(nu.OP_SHAPES))
@pytest.mark.parametrize("scale", ["l1", "l2"])
@pytest.mark.parametrize("affine", [0, 1])
def test_gcn_normalize_matches_the_reference(golden, size, scale, affine):
    from eoe_amd import gcn_normalize
    g = golden("g20_normstats")
    x = _op_input_dev(size)
    c = x.shape[1]
    sh, rg = ([float(g["op/shift"])] * c, [float(g["op/range"])] * c) if affine else (None, None)
    y = gcn_normalize(x, scale, sh, rg)
    assert torch.equal(x, _op_input_dev(size))                                        # out of place leaves x alone
    got = y.cpu().numpy()
    ratio = nu.op_ratio(got[:, :, ::8, ::8] if size == "224" else got, g, size, scale, affine)
    print(f"\n   [gcn_normalize {size} {scale} affine={affine}] deviation / (3 x reference noise) = {ratio:.3f}", end="")
    assert ratio <= 1.0
    # in place: the same bits; twice: the same bits
    z = x.clone()
    assert gcn_normalize(z, scale, sh, rg, out=z) is z and torch.equal(z, y)
    assert torch.equal(gcn_normalize(x, scale, sh, rg), y)


def test_gcn_class_form_works_in_place_and_returns_its_argument(golden):
    from eoe_amd import GlobalContrastNormalization, GcnNormalize, gcn_normalize
    g = golden("g20_normstats")
    x = _op_input_dev("28")
    keep = x.clone()
    gcn = GlobalContrastNormalization(scale="l1")
    y = gcn(x)
    assert y is x and not torch.equal(x, keep)
    assert nu.op_ratio(x.cpu().numpy(), g, "28", "l1", 0) <= 1.0
    # the source-side object: out of place, GCN + Normalize in one launch
    op = GcnNormalize([float(g["op/shift"])], [float(g["op/range"])], "l1")
    z = op(keep)
    assert z is not keep and torch.equal(keep, _op_input_dev("28"))
    assert torch.equal(z, gcn_normalize(keep, "l1", [float(g["op/shift"])], [float(g["op/range"])]))
    assert nu.op_ratio(z.cpu().numpy(), g, "28", "l1", 1) <= 1.0


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 1, 9, 9), (2, 3, 72, 72), (1, 3, 224, 224)])
def test_gcn_normalize_other_shapes_vs_fp64(shape):
    """shapes off the fixture: a feature count that is no multiple of 4 (the scalar path), one just past the all-in-registers
    limit, one full 224 x 224 sample compared on every element.  The sums run in fp64, so what is left is the rounding of the
    fp32 output: one ulp, 2^-23 relative to max(1, |y|)"""
    from eoe_amd import gcn_normalize
    from normstats_util import torch_gcn_normalize
    x = ofill.fill(f"g20/other/{shape}", shape, std=0.25, mean=0.5)
    c = shape[1]
    for scale in ("l1", "l2"):
        for sh, rg in ((None, None), ([-1.25] * c, [3.5 + 0.25 * k for k in range(c)])):
            want = torch_gcn_normalize(torch.from_numpy(x).double(), scale, sh, rg).numpy()
            got = gcn_normalize(torch.from_numpy(x).cuda(), scale, sh, rg).cpu().numpy().astype(np.float64)
            assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 2.0 ** -23, (shape, scale, sh)


def test_gcn_constant_sample_is_non_finite_as_in_the_reference():
    from eoe_amd import gcn_normalize
    x = _op_input_dev("28")
    x[2] = 0.5
    y = gcn_normalize(x)
    assert not torch.isfinite(y[2]).any() and torch.isfinite(y[[0, 1, 3, 4]]).all()


# ------------------------------------------------------------------------------------------------------------ 4 / 5. sources and trainer
def _lit_set(n_per_class=24, n_test=16, n_oe=20):
    """two classes of differently lit 32 x 32 images (class 0 dark, class 1 bright and flatter), an OE set, a test split"""
    def imgs(name, n, lo, hi):
        return torch.from_numpy(ofill.fill_int(name, (n, 32, 32, 3), lo, hi).astype(np.uint8))
    train = torch.cat([imgs("g20/lit/dark", n_per_class, 0, 120), imgs("g20/lit/bright", n_per_class, 140, 250)])
    classes = torch.cat([torch.zeros(n_per_class, dtype=torch.int64), torch.ones(n_per_class, dtype=torch.int64)])
    perm = torch.from_numpy(np.argsort(ofill.uniform_pm1("g20/lit/perm", 2 * n_per_class)))     # interleave the classes
    train, classes = train[perm], classes[perm]
    test = torch.cat([imgs("g20/lit/tdark", n_test // 2, 0, 120), imgs("g20/lit/tbright", n_test // 2, 140, 250)])
    test_classes = torch.cat([torch.zeros(n_test // 2, dtype=torch.int64), torch.ones(n_test // 2, dtype=torch.int64)])
    return train, classes, test, test_classes, imgs("g20/lit/oe", n_oe, 0, 256)


def _labelled(normalize, **kw):
    from eoe_amd.data import LabelledImageSet
    train, classes, test, test_classes, oe = _lit_set()
    return LabelledImageSet(train, classes, test, test_classes, oe, ["dark", "bright"], crop=32, normalize=normalize, **kw), train, classes


def test_labelled_set_fits_per_task_and_caches(monkeypatch):
    from eoe_amd import fit_statistics, normalize as norm_mod
    from eoe_amd.normalize import GcnNormalize
    lset, train, classes = _labelled("gcn-normalize")
    calls = []
    real = norm_mod.fit_statistics
    monkeypatch.setattr(norm_mod, "fit_statistics", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    s0, s1 = lset.source([0], seed=0), lset.source([1], seed=0)
    assert len(calls) == 2
    assert s0.ds_statistics != s1.ds_statistics and s0.ds_statistics["mode"] == 1 == s1.ds_statistics["mode"]
    for c, s in ((0, s0), (1, s1)):
        rows = torch.nonzero(classes == c).flatten()
        assert s.ds_statistics == real(train.cuda(), rows, "gcn-normalize")
        assert isinstance(s.normalize, GcnNormalize) and s.normalize.shift == s.ds_statistics["mean"] and s.mean is None
    again = lset.source([0], seed=1)                                       # another seed of the same task: no second fit
    assert len(calls) == 2 and again.ds_statistics == s0.ds_statistics
    both = lset.source([1, 0], seed=0)                                     # another class set: its own fit, keyed by the sorted tuple
    assert len(calls) == 3 and both.ds_statistics == real(train.cuda(), None, "gcn-normalize")
    lset.source([0, 1], seed=0)
    assert len(calls) == 3
    given = {"mean": [-2.0] * 3, "std": [5.0] * 3, "mode": 1}             # a snapshot's statistics win and are not kept
    assert lset.source([0], seed=0, ds_statistics=given).ds_statistics == given
    assert lset.source([0], seed=0).ds_statistics == s0.ds_statistics and len(calls) == 3
    # batches leave the source in the [0, 1] scale
    xb = next(iter(s0.loaders(8)[0]))[0]
    assert float(xb.min()) > -0.01 and float(xb.max()) < 1.01


def _scores(logdir, c):
    with open(f"{logdir}/eval_cls{c}_it0_anomaly_scores.json") as f:
        return json.load(f)


def test_trainer_runs_gcn_mode_and_scores_snapshots_with_their_statistics(tmp_path):
    from eoe_amd.models import CNN32
    from eoe_amd.msm import MSM, msm_filter
    from eoe_amd.normalize import gcn_normalize
    from normstats_util import torch_gcn_normalize
    from eoe_amd.training import HSCTrainer
    from eoe_amd.training.ad_trainer import JsonLogger
    torch.manual_seed(0)
    lset, train, classes = _labelled("gcn-normalize")
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    tr = HSCTrainer(CNN32(bias=True), dataset=lset, epochs=1, lr=1e-3, batch_size=8, logger=JsonLogger(d1))
    _, res = tr.run()
    assert all(np.isfinite(tr.last_losses)) and len(res["cls_aucs"]) == 2
    paths = [f"{d1}/snapshots/snapshot_cls{c}_it0.pt" for c in (0, 1)]
    snaps = [torch.load(p) for p in paths]
    for c, snap in enumerate(snaps):
        st = snap["ds_statistics"]
        assert st["mode"] == 1 and type(st["mean"]) is list and type(st["std"]) is list and type(st["mode"]) is int
        assert all(type(v) is float for v in st["mean"] + st["std"])
        assert st == lset.source([c], 0).ds_statistics
    assert snaps[0]["ds_statistics"] != snaps[1]["ds_statistics"]
    assert tr.load_ds_statistics(paths[1]) == snaps[1]["ds_statistics"] and tr.load_ds_statistics(None) is None
    # score the snapshots again, from the files alone: stored weights with stored statistics, bit for bit the first run's scores.
    # The image set of the second trainer is lit differently in training, so statistics fitted there would differ: only the
    # stored ones can reproduce the scores
    train2, classes2, test, test_classes, oe = _lit_set()
    from eoe_amd.data import LabelledImageSet
    other = LabelledImageSet(255 - train2, classes2, test, test_classes, oe, ["dark", "bright"], crop=32, normalize="gcn-normalize")
    tr2 = HSCTrainer(CNN32(bias=True), dataset=other, epochs=1, lr=1e-3, batch_size=8, logger=JsonLogger(d2))
    tr2.run(load=[[paths[0]], [paths[1]]], train=False)
    for c in (0, 1):
        assert _scores(d1, c) == _scores(d2, c)
        assert torch.load(f"{d2}/snapshots/snapshot_cls{c}_it0.pt")["ds_statistics"] == snaps[c]["ds_statistics"]
    assert other.source([0], 0).ds_statistics != snaps[0]["ds_statistics"]

    # what the encoder receives: GCN + affine of the [0, 1] test batch (the reference's torch-op chain in fp64 is the twin; the
    # allowance is 3 x the distance of that chain in fp32 on the device to the twin)
    ds = lset.source([0], 0)
    seen = []
    model = CNN32(bias=True)
    hook = model.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone()))
    tr.eval_cls(model, ds, 0, "dark", 0)
    raw = [b[0] for b in ds.loaders(8)[1]]
    sh, rg = ds.ds_statistics["mean"], ds.ds_statistics["std"]
    assert len(seen) == len(raw) == 2
    for got, x in zip(seen, raw):
        twin = torch_gcn_normalize(x.cpu().double(), "l1", sh, rg).numpy()
        chain = torch_gcn_normalize(x, "l1", sh, rg).cpu().numpy().astype(np.float64)
        den = np.maximum(1.0, np.abs(twin))
        noise = np.max(np.abs(chain - twin) / den)
        dev = np.max(np.abs(got.cpu().numpy().astype(np.float64) - twin) / den)
        print(f"\n   [encoder input] deviation {dev:.2e}, torch fp32 chain {noise:.2e}", end="")
        assert noise > 0 and dev <= nu.K_NOISE_PARITY * noise
        assert torch.equal(got, gcn_normalize(x, "l1", sh, rg))
    # with an MSM listed the filter runs first, in the [0, 1] scale, then GCN
    seen.clear()
    trm = HSCTrainer(CNN32(bias=True), dataset=lset, epochs=1, lr=1e-3, batch_size=8, msms=[MSM.load("lpf+test_nominal--M4")])
    trm.eval_cls(model, ds, 0, "dark", 0)
    filtered = 0
    for got, b in zip(seen, ds.loaders(8)[1]):
        by_hand = gcn_normalize(msm_filter(b[0], "lpf", 4, b[1] == 0), "l1", sh, rg)
        assert torch.equal(got, by_hand)
        if bool((b[1] == 0).any()):                  # a batch with nominal rows: the filter changed what GCN saw
            assert not torch.equal(got, gcn_normalize(b[0], "l1", sh, rg))
            filtered += 1
    assert filtered >= 1
    hook.remove()


def test_normalize_mode_reuses_the_mean_std_path():
    from eoe_amd.data import ResidentImageSource, normal_subset, ad_targets
    lset, train, classes = _labelled("normalize", padding=2)
    train_np = train.numpy()
    for c in (0, 1):
        src = lset.source([c], seed=3)
        st = src.ds_statistics
        rows = torch.nonzero(classes == c).flatten()
        x = train_np[rows.numpy()].transpose(0, 3, 1, 2).astype(np.float64) / 255.0
        mean, std = nu.running_stats_np(x)
        assert st["mode"] == 0 and np.allclose(st["mean"], mean, rtol=1e-12, atol=0) and np.allclose(st["std"], std, rtol=1e-12, atol=0)
        assert src.normalize is None and src.mean == st["mean"] and src.std == st["std"]
        # the same batches, bit for bit, as a source handed these numbers as mean= / std=
        train_u8, _, test, test_classes, oe = _lit_set()
        ref = ResidentImageSource(train_u8, oe, test, ad_targets(test_classes, [c]), 32, padding=2, mean=st["mean"], std=st["std"], seed=3,
                                  normal_index=normal_subset(classes, [c]))
        (ta, tea), (tb, teb) = src.loaders(8), ref.loaders(8)
        n = 0
        for a, b in zip(ta, tb):
            assert all(torch.equal(u, v) for u, v in zip(a, b))
            n += 1
        assert n == 3 and all(torch.equal(a[0], b[0]) for a, b in zip(tea, teb))
    assert lset.source([0], 0).ds_statistics != lset.source([1], 0).ds_statistics


# ------------------------------------------------------------------------------------------------------------ 6. trajectory
def test_trajectory_behind_gcn_matches_the_reference(golden):
    """CNN32 in its exact-fp32 mode through ADTrainer.train_cls on the fixture's [0, 1] batches, the source reporting a
    GcnNormalize: K = 10 Adam steps against the reference's trajectory (its GCN + Normalize on every batch first)"""
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN32
    from eoe_amd.normalize import GcnNormalize
    from eoe_amd.training import HSCTrainer
    g = golden("g20_normstats")
    gt = {k: g[f"traj/{k}"] for k in ("losses", "scores", "losses64", "scores64")}
    batches = [tuple(torch.from_numpy(a) for a in nu.traj_batch(i)) for i in range(nu.TRAJ_STEPS)]
    op = GcnNormalize([float(g["op/shift"])] * 3, [float(g["op/range"])] * 3, "l1")
    m = omodels.deterministic_init(CNN32(bias=True), tag="cnn32")
    tr = HSCTrainer(m, dataset=ListSource(batches, normalize=op), epochs=1, lr=1e-3, wdk=0.0, milestones=[], batch_size=nu.TRAJ_HALF)
    assert tr._exact_bn_for(m)
    tr.train_cls(m, tr.ds, 0, "0", 0)
    labels, scores = tr.last_scores[0]
    scores = scores.float().cpu().numpy().reshape(nu.TRAJ_STEPS, 2 * nu.TRAJ_HALF)
    assert torch.equal(batches[0][0], torch.from_numpy(nu.traj_batch(0)[0]))          # the source's batches are left alone
    print("\n   " + parity_util.check_trajectory(tr.last_losses, list(scores), gt, nu.K_NOISE_PARITY, what="CNN32 behind GCN, parity mode"))
