"""CPU: the nearest-neighbour entry points exist and refuse bad arguments before any launch, the scratch size grows with every
argument, `neighbors.knn_np` on hand-worked cases (ties, fewer references than k, non-finite rows), `knn_score`, `Neighbors`, and
the refusals of `embed`, of `ResidentImageSource.normal_inputs` and of the trainer's `neighbors` / `knn_baseline` arguments."""
import numpy as np
import pytest
import torch

import knn_util
import ragged_util as ru

NEW_SYMBOLS = ("eoe_feature_knn", "eoe_feature_knn_scratch_bytes")
Q, R, I, D2, C, S = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000      # non-null, 16-byte aligned addresses nothing reads


def test_the_two_entry_points_are_exported_and_the_abi_version_stays():
    from eoe_amd import _lib
    assert _lib.lib.eoe_abi_version() == 5 and _lib.ABI_VERSION == 5
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(_lib.lib, name)
    assert knn_util.cover_is_complete()


def test_feature_knn_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_feature_knn, lib.eoe_last_error
    # eoe_feature_knn(q, ldq, r, ldr, nq, nr, D, k, idx, d2, counts, scratch, stream)
    good = [Q, 8, R, 8, 4, 10, 8, 5, I, D2, C, S, None]
    for i in (0, 2, 8, 9, 10, 11):
        args = list(good)
        args[i] = None
        assert f(*args) == 1 and b"feature_knn" in err() and b"null" in err(), i
    for k in (0, 65, -1):
        args = list(good)
        args[7] = k
        assert f(*args) == 1 and b"k must be" in err(), k
    for D in (0, 2049):
        args = list(good)
        args[1] = args[3] = args[6] = D
        assert f(*args) == 1 and b"D must be" in err(), D
    args = list(good)
    args[1] = 7
    assert f(*args) == 1 and b"ldq" in err()
    args = list(good)
    args[3] = 7
    assert f(*args) == 1 and b"ldr" in err()
    for nr in (1 << 24, -1):
        args = list(good)
        args[5] = nr
        assert f(*args) == 1 and b"nr must be" in err(), nr
    args = list(good)
    args[4] = -1
    assert f(*args) == 1 and b"nq must not be negative" in err()
    args = list(good)
    args[0] = Q + 2
    assert f(*args) == 1 and b"aligned" in err()
    args = list(good)
    args[11] = S + 4
    assert f(*args) == 1 and b"aligned" in err()
    args = list(good)
    args[4] = 0                                                         # no query: nothing to launch
    assert f(*args) == 0
    args[5] = 0
    assert f(*args) == 0


def test_the_scratch_size_is_positive_and_grows_with_every_argument():
    from eoe_amd._lib import lib
    sb = lib.eoe_feature_knn_scratch_bytes
    base = (100, 5000, 512, 5)
    assert sb(*base) > 0 and sb(1, 1, 1, 1) > 0 and sb(0, 0, 1, 1) > 0
    steps = {0: (1, 31, 33, 130, 10000), 1: (1, 127, 1023, 1025, 2051, 45000, (1 << 24) - 1), 2: (1, 64, 515, 2048), 3: (1, 5, 16, 64)}
    for axis, values in steps.items():
        sizes = [sb(*[v if a == axis else base[a] for a in range(4)]) for v in values]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (axis, sizes)
        if axis != 2:                                                   # the width does not enter: the distance matrix is never stored
            assert sizes[-1] > sizes[0], (axis, sizes)
    # the keys: one 8-byte key per (query, chunk of 1 024 references, slot)
    assert sb(10000, 45000, 512, 5) >= 10000 * 44 * 5 * 8
    assert sb(10000, 45000, 512, 5) < 10000 * 45000 * 4 // 50
    for bad in ((-1, 10, 8, 5), (4, 1 << 24, 8, 5), (4, 10, 0, 5), (4, 10, 2049, 5), (4, 10, 8, 0), (4, 10, 8, 65)):
        assert sb(*bad) == 0, bad


def test_knn_np_on_hand_worked_cases():
    from eoe_amd.neighbors import knn_np
    r = np.array([[0, 0], [3, 4], [0, 1], [1, 0], [0, -1], [3, 4]], dtype=np.float32)
    q = np.array([[0, 0], [3, 4]], dtype=np.float32)
    idx, d2, bad = knn_np(q, r, 4)
    assert idx.dtype == np.int64 and d2.dtype == np.float64 and bad == (0, 0)
    assert idx.tolist() == [[0, 2, 3, 4], [1, 5, 2, 3]]                 # the three references at distance 1 and the two at 0: by index
    assert d2.tolist() == [[0, 1, 1, 1], [0, 0, 18, 20]]
    for k in (1, 6):
        i2, dd, _ = knn_np(q, r, k)
        order = [np.argsort(((q[j] - r) ** 2).sum(1), kind="stable")[:k] for j in range(2)]
        assert i2.tolist() == [o.tolist() for o in order]
    # fewer references than k
    idx, d2, _ = knn_np(q, r[:2], 4)
    assert idx.tolist() == [[0, 1, -1, -1], [1, 0, -1, -1]] and d2[:, :2].tolist() == [[0, 25], [0, 25]] and np.isposinf(d2[:, 2:]).all()
    idx, d2, _ = knn_np(q, r[:0], 2)
    assert (idx == -1).all() and np.isposinf(d2).all()
    assert knn_np(q[:0], r, 3)[0].shape == (0, 3)
    # a non-finite reference is never returned, a non-finite query gets nothing
    r2 = r.copy()
    r2[0, 1] = np.nan
    r2[5, 0] = np.inf
    q2 = np.array([[0, 0], [np.nan, 1], [3, 4], [-np.inf, 0]], dtype=np.float32)
    idx, d2, bad = knn_np(q2, r2, 5)
    assert bad == (2, 2)
    assert idx.tolist() == [[2, 3, 4, 1, -1], [-1] * 5, [1, 2, 3, 4, -1], [-1] * 5]
    assert d2[0].tolist() == [1, 1, 1, 25, np.inf] and np.isnan(d2[1]).all() and np.isnan(d2[3]).all()
    for args in ((q, r, 0), (q, r, 65), (q, r, True), (q, r[:, :1], 2), (q[0], r, 2)):
        with pytest.raises(ValueError):
            knn_np(*args)


def test_feature_knn_on_cpu_tensors_is_knn_np_and_the_scores_follow():
    from eoe_amd import neighbors
    q, r = knn_util.exact_features(7, 5, 1), knn_util.exact_features(40, 5, 2)
    got = neighbors.feature_knn(torch.from_numpy(q), torch.from_numpy(r), 6)
    idx, d2, _ = neighbors.knn_np(q, r, 6)
    assert got.idx.dtype == torch.int64 and got.d2.dtype == torch.float32 and got.nonfinite == (0, 0) and got.k == 6
    assert np.array_equal(got.idx.numpy(), idx) and np.array_equal(got.d2.numpy(), d2.astype(np.float32))
    assert np.array_equal(neighbors.feature_knn(q, r, 6).idx.numpy(), idx)            # arrays as well
    knn_util.check_exact(got.idx.numpy(), got.d2.numpy(), q, r, 6)
    knn_util.check_real(got.idx.numpy(), got.d2.numpy(), q, r, 6)
    assert torch.equal(got.dist(), got.d2.sqrt())
    mean, kth = neighbors.knn_score(got, "mean"), neighbors.knn_score(got, "kth")
    assert mean.dtype == torch.float32 and mean.shape == (7,)
    assert np.allclose(mean.numpy(), np.sqrt(d2).mean(1), rtol=1e-6) and np.array_equal(kth.numpy(), np.sqrt(d2[:, 5]).astype(np.float32))
    hand = neighbors.Neighbors(torch.tensor([[1, 0]]), torch.tensor([[9.0, 16.0]]), (0, 0))
    assert neighbors.knn_score(hand, "mean").tolist() == [3.5] and neighbors.knn_score(hand, "kth").tolist() == [4.0]
    with pytest.raises(ValueError, match="mode"):
        neighbors.knn_score(got, "median")
    short = neighbors.feature_knn(torch.from_numpy(q), torch.from_numpy(r[:2]), 3)
    assert torch.isinf(neighbors.knn_score(short, "mean")).all()
    d = short.as_dict(row_ids=[10 + i for i in range(7)], ref_ids=[100, 200])
    assert d["k"] == 3 and d["nonfinite"] == [0, 0] and [x["row"] for x in d["rows"]] == list(range(10, 17))
    assert all(len(x["neighbors"]) == 2 and {n[0] for n in x["neighbors"]} == {100, 200} for x in d["rows"])
    assert d["rows"][0]["neighbors"][0][1] == float(short.dist()[0, 0])
    assert short.as_dict()["rows"][3]["row"] == 3
    with pytest.raises(ValueError, match="row_ids"):
        short.as_dict(row_ids=[1, 2])
    with pytest.raises(ValueError, match="float32"):
        neighbors.feature_knn(torch.from_numpy(q).double(), torch.from_numpy(r), 2)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        neighbors.feature_knn_device(torch.from_numpy(q), torch.from_numpy(r), 2)


def test_embed_concatenates_features_and_refuses_a_classifier_head():
    from eoe_amd import neighbors

    class Feat(torch.nn.Module):
        def __init__(self, out):
            super().__init__()
            self.lin = torch.nn.Linear(12, out)

        def forward(self, x):
            assert not self.training and not torch.is_grad_enabled()
            return self.lin(x.reshape(x.shape[0], -1))
    m = Feat(4).train()
    a, b = torch.randn(3, 3, 2, 2), torch.randn(2, 3, 2, 2)
    f = neighbors.embed(m, [a, (b, torch.zeros(2))])
    assert f.shape == (5, 4) and f.dtype == torch.float32 and not f.requires_grad and m.training
    with torch.no_grad():
        assert torch.equal(f, m.eval()(torch.cat([a, b])))
    with pytest.raises(ValueError, match="a classifier head has no embedding; use an objective with a feature output"):
        neighbors.embed(Feat(1), [a])
    with pytest.raises(ValueError, match="at least one batch"):
        neighbors.embed(m, [])


def test_normal_inputs_refuses_rows_outside_the_set_and_a_ragged_set_under_clip():
    from eoe_amd import data
    big = data.RaggedImageSet([ru.image(i, h, w, 3) for i, (h, w) in enumerate([(10, 14), (14, 10), (12, 12), (10, 10)])])
    t8 = torch.zeros((4, 8, 8, 3), dtype=torch.uint8)
    lab = torch.tensor([0, 1, 0, 1])
    src = data.ResidentImageSource(big, big, t8, lab, crop=8, padding=1, device="cpu", seed=7, clip_preprocessing=8)
    assert src.n_normal == 4
    with pytest.raises(NotImplementedError, match="ragged normal training set has no such copy"):
        src.normal_inputs([0])
    with pytest.raises(NotImplementedError, match="ragged normal"):
        src.normal_pictures([0])
    plain = data.ResidentImageSource(t8, t8, t8, lab, crop=8, device="cpu", normal_index=[1, 3])
    assert plain.n_normal == 2
    for rows in ([2], [-1], [0, 5]):
        with pytest.raises(IndexError, match="outside the normal training set of 2"):
            plain.normal_inputs(rows)


def test_the_trainer_refuses_neighbors_without_extremes_and_a_baseline_without_neighbors():
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    kw = dict(dataset=None, epochs=1, batch_size=4, classes=["a"], device="cpu")
    with pytest.raises(ValueError, match="extremes must be at least 1"):
        TRAINER["hsc"](CNN32(), neighbors=4, **kw)
    with pytest.raises(ValueError, match="neighbors must be at least 1"):
        TRAINER["hsc"](CNN32(), extremes=3, knn_baseline=True, **kw)
    for bad in (65, -1, True, 2.0):
        with pytest.raises(ValueError, match="neighbors must be an integer in"):
            TRAINER["hsc"](CNN32(), extremes=3, neighbors=bad, **kw)
    on = TRAINER["hsc"](CNN32(), extremes=3, neighbors=64, knn_baseline=True, **kw)
    off = TRAINER["hsc"](CNN32(), **kw)
    assert (on.n_neighbors, on.with_knn_baseline, off.n_neighbors, off.with_knn_baseline) == (64, True, 0, False)
    assert on.neighbors == {} and on.knn_results == {} and off.neighbors == {} and off.knn_results == {}

    class NoNormals:
        nominal_label = 0

        def test_inputs(self, rows):
            raise AssertionError

        def loaders(self, *a, **k):
            raise AssertionError("no loader may be asked for")
    with pytest.raises(NotImplementedError, match="needs a source with normal_inputs"):
        on.eval_cls(CNN32(), NoNormals(), 0, "a", 0)
