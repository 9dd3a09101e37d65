"""GPU tier: `eoe_score_extremes` (csrc/topk.hip) -- positions and score bits of both label groups and both ends against NumPy's stable
argsorts (tests/topk_util.py) over every size, score kind, label layout and k; output buffers pre-filled with a sentinel and a dirty
scratch; repeatability byte for byte; the count of non-finite members; `metrics.score_extremes` on device tensors; the refusals."""
import numpy as np
import pytest
import torch

import topk_util
from eoe_amd import metrics

pytestmark = pytest.mark.gpu

SENTINEL = -7


def raw(st, yt, k, fill):
    """one `eoe_score_extremes` call into buffers pre-filled with SENTINEL, the scratch pre-filled with the byte `fill`:
    (idx int32 [2, 2, k], val float32 [2, 2, k], counts [3]) on the host"""
    from eoe_amd._lib import check, lib
    n = st.numel()
    idx = torch.full((2, 2, k), SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((2, 2, k), float(SENTINEL), dtype=torch.float32, device="cuda")
    counts = torch.full((3,), SENTINEL, dtype=torch.int32, device="cuda")
    scratch = torch.full((lib.eoe_score_extremes_scratch_bytes(n, k),), fill, dtype=torch.uint8, device="cuda")
    check(lib.eoe_score_extremes(st.data_ptr(), yt.data_ptr() if yt is not None else None, n, k, idx.data_ptr(), val.data_ptr(),
                                 counts.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "eoe_score_extremes")
    return idx.cpu().numpy(), val.cpu().numpy(), counts.cpu().tolist()


@pytest.mark.parametrize("kind", topk_util.KINDS)
@pytest.mark.parametrize("n", topk_util.NS)
def test_positions_and_score_bits_equal_numpys_stable_argsorts(n, kind):
    s = topk_util.scores(n, kind)
    st = torch.from_numpy(s.copy()).cuda()
    if kind == "tie_run" and n == 1 << 20:                                          # the run of ties really straddles position 2^19
        top = np.flatnonzero(s == np.float32(1.5))
        assert top.size > 1024 and (top < topk_util.HALF).sum() > 20 and (top > topk_util.HALF).sum() > 20
    for how in topk_util.LAYOUTS:
        y = topk_util.labels(n, how)
        yt = None if y is None else torch.from_numpy(y.copy()).cuda()
        want_all = topk_util.reference(s, y, max(topk_util.KS))                     # one pair of argsorts per group; a smaller k is a prefix
        for k in topk_util.KS:
            want = ([(a[:k], b[:k]) for a, b in want_all[0]], want_all[1])
            idx, val, counts = raw(st, yt, k, 0xA5)
            topk_util.check_raw(idx, val, counts, s, want, k, SENTINEL, f"{kind} n={n} {how} k={k}")
        if how in ("mixed", None):                                                  # the public function on the same tensors
            topk_util.check_extremes(metrics.score_extremes(yt, st, 20), s, topk_util.reference(s, y, 20), 20, f"{kind} n={n} {how}")


@pytest.mark.parametrize("n", (257, 65539))
def test_two_runs_give_the_same_bytes_and_a_dirty_scratch_changes_nothing(n):
    from eoe_amd._lib import lib
    for kind in ("quant8", "mixed"):
        s, y = topk_util.scores(n, kind), topk_util.labels(n, "other")
        st, yt = torch.from_numpy(s.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
        for k in (20, 1024):
            runs = [raw(st, yt, k, fill) for fill in (0x00, 0x00, 0xFF, 0x5A)]
            for idx, val, counts in runs[1:]:
                assert idx.tobytes() == runs[0][0].tobytes() and val.tobytes() == runs[0][1].tobytes() and counts == runs[0][2]
            need = lib.eoe_score_extremes_scratch_bytes(n, k)
            own = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            a = metrics.score_extremes_device(yt, st, k, scratch=own)
            b = metrics.score_extremes_device(yt, st, k)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] == runs[0][2]
            m = [min(k, c) for c in a[2][:2]]
            for g in (0, 1):
                assert np.array_equal(a[0][g, :, :m[g]], runs[0][0][g, :, :m[g]]) and (a[0][g, :, m[g]:] == -1).all()
            with pytest.raises(ValueError):
                metrics.score_extremes_device(yt, st, k, scratch=own[:need - 16])


def test_non_finite_members_are_counted_and_refused_others_ignored():
    n = 4097
    s, y = topk_util.scores(n, "mixed"), topk_util.labels(n, "other")
    outside, inside = np.flatnonzero((y != 0) & (y != 1)), np.flatnonzero((y == 0) | (y == 1))
    # under a label outside both groups: ignored
    b = s.copy()
    b[outside[:3]] = [np.nan, np.inf, -np.inf]
    bt, yt = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(y.copy()).cuda()
    idx, val, counts = raw(bt, yt, 20, 0xA5)
    topk_util.check_raw(idx, val, counts, s, topk_util.reference(s, y, 20), 20, SENTINEL, "non-finite outside the groups")
    topk_util.check_extremes(metrics.score_extremes(yt, bt, 20), s, topk_util.reference(s, y, 20), 20, "non-finite outside the groups")
    # among the members: counted, every written position in range, and the public function refuses
    for bad in ([np.nan], [np.inf], [-np.inf], [np.nan, np.inf, -np.inf, np.nan, np.nan]):
        b = s.copy()
        b[inside[5:5 + len(bad)]] = bad
        bt = torch.from_numpy(b.copy()).cuda()
        idx, val, counts = raw(bt, yt, 20, 0xA5)
        assert counts == [int((y == 0).sum()), int((y == 1).sum()), len(bad)]
        assert ((idx == SENTINEL) | ((idx >= 0) & (idx < n))).all()
        with pytest.raises(ValueError):
            metrics.score_extremes(yt, bt, 20)
        with pytest.raises(ValueError):
            metrics.score_extremes(None, bt, 20)


def test_device_refusals_and_host_labels():
    s = torch.tensor([0.1, 0.4, 0.3, 0.2]).cuda()
    y = torch.tensor([0, 1, 1, 0])
    ex = metrics.score_extremes(y, s, k=3)                                          # labels may live on the host
    assert ex.num == (2, 2) and ex.most[0][0].tolist() == [3, 0] and ex.least[1][0].tolist() == [2, 1]
    assert ex == metrics.score_extremes(y.numpy(), s.cpu().numpy(), k=3)
    assert metrics.score_extremes(y, s, k=3, indices=[10, 11, 12, 13]).most[1][0].tolist() == [11, 12]
    for k in (0, 1025, -1):
        with pytest.raises(ValueError):
            metrics.score_extremes(y, s, k=k)
    with pytest.raises(ValueError):
        metrics.score_extremes(y[:3], s)
    with pytest.raises(ValueError):
        metrics.score_extremes(y, s, indices=[1, 2])
    with pytest.raises(ValueError):
        metrics.score_extremes(None, torch.zeros(0).cuda())
    with pytest.raises(ValueError):
        metrics.score_extremes(None, torch.zeros((1 << 20) + 1).cuda())
    with pytest.raises(RuntimeError):
        metrics.score_extremes_device(y, s.cpu())


def test_score_extremes_bad_arguments_launch_nothing():
    from eoe_amd._lib import lib
    n, k = 8, 2
    s = torch.rand(n).cuda()
    idx = torch.full((2, 2, k), SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((2, 2, k), float(SENTINEL), dtype=torch.float32, device="cuda")
    counts = torch.full((3,), SENTINEL, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.eoe_score_extremes_scratch_bytes(n, k), dtype=torch.uint8, device="cuda")
    good = [s.data_ptr(), None, n, k, idx.data_ptr(), val.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
            torch.cuda.current_stream().cuda_stream]
    for i in (0, 4, 5, 6, 7):
        args = list(good)
        args[i] = None
        assert lib.eoe_score_extremes(*args) == 1, i
    for i, v in ((2, 0), (2, (1 << 20) + 1), (3, 0), (3, 1025)):
        args = list(good)
        args[i] = v
        assert lib.eoe_score_extremes(*args) == 1, (i, v)
    torch.cuda.synchronize()
    assert (idx == SENTINEL).all() and (val == SENTINEL).all() and (counts == SENTINEL).all()      # nothing was launched
    assert lib.eoe_score_extremes(*good) == 0
    order = np.argsort(-s.cpu().numpy(), kind="stable")
    assert counts.tolist() == [n, 0, 0] and idx[0, 0].tolist() == order[:k].tolist() and idx[0, 1].tolist() == order[::-1][:k].tolist()
    assert (idx[1] == SENTINEL).all() and (val[1] == SENTINEL).all()
