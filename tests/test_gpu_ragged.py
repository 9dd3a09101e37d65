"""GPU tier of the ragged image sets: the ragged Resize against Pillow's bytes (fixture g25), the ragged crop / augment / jitter
kernels against the uniform kernels run on each image alone (bit for bit) and against the fixture, and a ResidentImageSource /
LabelledImageSet over sets of mixed sizes up to a CNN32 trainer run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ragged_util as ru                   # noqa: E402

S = ru.TARGET


def _ragged(C=3, imgs=None):
    from eoe_amd import data
    return data.RaggedImageSet(ru.images(C) if imgs is None else imgs, device="cuda")


def _resized(golden, C=3, filt="bilinear"):
    """the fixture's Resize(16) results as a ragged set on the device (the crop tests do not depend on the Resize kernel)"""
    g = golden("g25_ragged")
    return _ragged(C, [g[f"r/{filt}/c{C}/{i}"] for i in range(len(ru.SHAPES))])


# ---------------------------------------------------------------------------------------------------------------- 1. Resize
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("filt", ru.FILTERS)
def test_ragged_resize_equals_pillow(golden, C, filt):
    from eoe_amd import data
    g = golden("g25_ragged")
    rs = _ragged(C)
    out = data.resize_u8(rs, S, filt)
    assert isinstance(out, data.RaggedImageSet) and len(out) == len(rs) and out.channels == C and out.is_cuda
    assert [tuple(s) for s in out.sizes.tolist()] == ru.RESIZED and (out.offsets_host % 16 == 0).all()
    assert out.offsets.cpu().tolist() == out.offsets_host.tolist() and out.sizes_dev.cpu().tolist() == out.sizes.tolist()
    for i in range(len(rs)):                                   # the identity and the unchanged images included
        assert np.array_equal(out[i].cpu().numpy(), g[f"r/{filt}/c{C}/{i}"]), i
    sq = data.resize_u8(rs, (S, S), filt)
    assert isinstance(sq, torch.Tensor) and sq.shape == (len(rs), S, S, C) and sq.dtype == torch.uint8 and sq.is_contiguous()
    for i in range(len(rs)):
        assert np.array_equal(sq[i].cpu().numpy(), g[f"p/{filt}/c{C}/{i}"]), i
    # the source arena is untouched
    assert all(np.array_equal(rs[i].cpu().numpy(), a) for i, a in enumerate(ru.images(C)))


def test_ragged_resize_single_pass_and_no_pass(golden):
    """only one axis changes for every image (the other pass is skipped as a whole, identity images are copied), and nothing changes"""
    from eoe_amd import data
    g = golden("g25_ragged")
    keep = [3, 4, 5]                                           # 16 x 16, 17 x 16, 16 x 97: Resize(16) leaves all three alone
    rs = _ragged(3, [ru.image(i, *ru.SHAPES[i], 3) for i in keep])
    assert data.resize_u8(rs, S, "bicubic") is rs
    wide = _ragged(3, [ru.image(i, *ru.SHAPES[i], 3) for i in (3, 5)])                  # heights 16: Resize((16, 16)) is horizontal only
    sq = data.resize_u8(wide, (S, S), "bilinear").cpu().numpy()
    assert np.array_equal(sq[0], g["p/bilinear/c3/3"]) and np.array_equal(sq[1], g["p/bilinear/c3/5"])
    tall = _ragged(1, [ru.image(i, *ru.SHAPES[i], 1) for i in (3, 4)])                  # widths 16: vertical only
    sq = data.resize_u8(tall, (S, S), "bicubic").cpu().numpy()
    assert np.array_equal(sq[0], g["p/bicubic/c1/3"]) and np.array_equal(sq[1], g["p/bicubic/c1/4"])
    same = data.RaggedImageSet.from_tensor(torch.from_numpy(np.stack([g["p/bilinear/c3/0"], g["p/bilinear/c3/1"]]))).to("cuda")
    t = data.resize_u8(same, (S, S), "bilinear")               # nothing to do: the tensor of the set
    assert isinstance(t, torch.Tensor) and np.array_equal(t[1].cpu().numpy(), g["p/bilinear/c3/1"])


# ------------------------------------------------------------------------------------------------------------------ 2. crop
def _alone(rs, i):
    """image i as a 1-image tensor set"""
    return rs[i].unsqueeze(0).contiguous()


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("flip_first", [True, False])
def test_ragged_crop_and_augment_equal_the_uniform_kernels_per_image(golden, C, flip_first):
    """four corner origins of the padded range (padding 3, so negative ones) and an interior one per image, flips alternating"""
    from eoe_amd import data
    rs = _resized(golden, C)
    p = ru.corner_params(ru.RESIZED, S, 3)
    assert (p[:, 1:3] < 0).any() and set(p[:, 3].tolist()) == {0, 1}
    pd = torch.from_numpy(p).cuda()
    mean, std = ([0.4, 0.5, 0.6], [0.2, 0.25, 0.3]) if C == 3 else ([0.45], [0.22])
    u8 = data.crop_flip_u8(rs, pd, (S, S), flip_first)
    f_plain = data.augment_batch(rs, pd, (S, S), None, None, flip_first, 0.0, 0)
    f_norm = data.augment_batch(rs, pd, (S, S), mean, std, flip_first, 0.0, 0)
    assert u8.shape == (len(p), S, S, C) and f_plain.shape == (len(p), C, S, S) and f_plain.dtype == torch.float32
    for i in range(len(rs)):
        rows = torch.from_numpy(np.nonzero(p[:, 0] == i)[0])
        one = _alone(rs, i)
        q = pd[rows].clone()
        q[:, 0] = 0
        assert torch.equal(u8[rows], data.crop_flip_u8(one, q, (S, S), flip_first)), i
        assert torch.equal(f_plain[rows], data.augment_batch(one, q, (S, S), None, None, flip_first, 0.0, 0)), i
        assert torch.equal(f_norm[rows], data.augment_batch(one, q, (S, S), mean, std, flip_first, 0.0, 0)), i
        for r in rows.tolist():                                # and the crop is the crop: the host restatement
            want = ru.crop_flip(rs[i].cpu().numpy(), int(p[r, 1]), int(p[r, 2]), int(p[r, 3]), S, flip_first)
            assert np.array_equal(u8[r].cpu().numpy(), want), (i, r)
    # odd output width: the quad kernel's ragged last quad and its scalar stores
    odd = data.crop_flip_u8(rs, pd, (S - 3, S - 1), flip_first)
    oddf = data.augment_batch(rs, pd, (S - 3, S - 1), mean, std, flip_first, 0.0, 0)
    for r in (0, 7, 26, 44):
        i = int(p[r, 0])
        q = torch.tensor([[0, int(p[r, 1]), int(p[r, 2]), int(p[r, 3])]], dtype=torch.int32, device="cuda")
        assert torch.equal(odd[r:r + 1], data.crop_flip_u8(_alone(rs, i), q, (S - 3, S - 1), flip_first)), r
        assert torch.equal(oddf[r:r + 1], data.augment_batch(_alone(rs, i), q, (S - 3, S - 1), mean, std, flip_first, 0.0, 0)), r


@pytest.mark.parametrize("C", [1, 3])
def test_last_image_of_the_arena_at_its_bottom_right_corner(golden, C):
    from eoe_amd import data
    rs = _resized(golden, C)
    last = len(rs) - 1
    H, W = (int(v) for v in rs.sizes[last])
    assert int(rs.offsets_host[last]) + H * W * C > rs.arena.numel() - 16           # its last byte lies in the arena's last 16
    p = torch.tensor([[last, H - S, W - S, 0], [last, H - S, W - S, 1]], dtype=torch.int32, device="cuda")
    got = data.crop_flip_u8(rs, p, (S, S), True).cpu().numpy()
    img = rs[last].cpu().numpy()
    assert np.array_equal(got[0], img[H - S:, W - S:]) and np.array_equal(got[1], img[:, ::-1][H - S:, W - S:])
    f = data.augment_batch(rs, p, (S, S), None, None, True, 0.0, 0).cpu().numpy()
    assert np.array_equal(f[0], (img[H - S:, W - S:].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 5, 257])
def test_slot_counts_and_noise_on_an_equal_size_set(n, C):
    """RaggedImageSet.from_tensor(t) against the tensor path on t: same params, same seed, noise on -- bit for bit"""
    from eoe_amd import data
    H, W, n_src, pad = 21, 19, 7, 2
    t = torch.from_numpy(np.stack([ru.image(i + 3, H, W, C) for i in range(n_src)])).cuda()
    rs = data.RaggedImageSet.from_tensor(t)
    assert rs.is_cuda and rs.is_uniform and torch.equal(rs.as_tensor(), t)
    k = np.arange(n)
    p = np.stack([(5 * k + 1) % n_src, (7 * k) % (H + 2 * pad - S + 1) - pad, (3 * k + 2) % (W + 2 * pad - S + 1) - pad, (k // 2) % 2],
                 axis=1).astype(np.int32).reshape(n, 4)
    pd = torch.from_numpy(p).cuda()
    mean, std = ([0.4, 0.5, 0.6], [0.2, 0.25, 0.3]) if C == 3 else ([0.45], [0.22])
    got = data.augment_batch(rs, pd, (S, S), mean, std, False, 0.001, 77)
    u8 = data.crop_flip_u8(rs, pd, (S, S), False)
    assert got.shape == (n, C, S, S) and u8.shape == (n, S, S, C)
    if n == 0:
        return                                                 # an empty batch, no launch
    assert torch.equal(got, data.augment_batch(t, pd, (S, S), mean, std, False, 0.001, 77))
    assert torch.equal(u8, data.crop_flip_u8(t, pd, (S, S), False))
    assert not torch.equal(got, data.augment_batch(rs, pd, (S, S), mean, std, False, 0.001, 78))       # the noise is on


@pytest.mark.parametrize("C", [1, 3])
def test_several_workgroups_per_slot(C):
    """an output large enough that several workgroups share a slot (50 x 61: 12 of them with three channels, 4 with one), from images
    whose rows are odd in bytes; the tensor path on the same set is the reference, noise on"""
    from eoe_amd import data
    H, W, n_src = 70, 83, 4
    t = torch.from_numpy(np.stack([ru.image(i + 20, H, W, C) for i in range(n_src)])).cuda()
    rs = data.RaggedImageSet.from_tensor(t)
    p = torch.tensor([[3, -4, -5, 0], [0, 24, 27, 1], [2, 9, 3, 1], [1, 0, 22, 0], [3, 20, -5, 1]], dtype=torch.int32, device="cuda")
    mean, std = ([0.4, 0.5, 0.6], [0.2, 0.25, 0.3]) if C == 3 else ([0.45], [0.22])
    for flip_first in (True, False):
        assert torch.equal(data.augment_batch(rs, p, (50, 61), mean, std, flip_first, 0.001, 9),
                           data.augment_batch(t, p, (50, 61), mean, std, flip_first, 0.001, 9))
        assert torch.equal(data.crop_flip_u8(rs, p, (50, 61), flip_first), data.crop_flip_u8(t, p, (50, 61), flip_first))
    if C == 3:
        factors = torch.tensor([[0.9, 1.2, 0.8, 0.03]] * 5, dtype=torch.float32)
        order = torch.tensor([[0, 1, 2, 3], [1, 3, 0, 2], [3, 2, 1, 0], [2, 0, 3, 1], [0, 2, 1, 3]], dtype=torch.int32)
        whole = data.color_jitter_u8(t, p[:, 0].cpu(), factors, order)
        ident = p.clone()
        ident[:, 0] = torch.arange(5, dtype=torch.int32, device="cuda")
        assert torch.equal(data.color_jitter_crop_u8(rs, p, (50, 61), factors, order, True), data.crop_flip_u8(whole, ident, (50, 61), True))


def test_slot_with_an_index_outside_the_set_is_padding(golden):
    from eoe_amd import data
    rs = _resized(golden, 3)
    p = torch.tensor([[len(rs), 0, 0, 0], [-1, 0, 0, 1], [2, 0, 0, 0]], dtype=torch.int32, device="cuda")
    u8 = data.crop_flip_u8(rs, p, (S, S))
    assert (u8[:2] == 0).all() and torch.equal(u8[2], rs[2])


# ---------------------------------------------------------------------------------------------------------------- 3. jitter
def test_jitter_crop_equals_jitter_then_crop_and_pillow(golden):
    from eoe_amd import data
    g = golden("g25_ragged")
    rs = _resized(golden, 3)
    p = torch.tensor([[i, top, left, flip] for i, _, _, (top, left), flip in ru.JITTER], dtype=torch.int32, device="cuda")
    factors = torch.tensor([f for _, _, f, _, _ in ru.JITTER], dtype=torch.float32)
    order = torch.tensor([o for _, o, _, _, _ in ru.JITTER], dtype=torch.int32)
    got = data.color_jitter_crop_u8(rs, p, (S, S), factors, order, True)
    assert got.shape == (3, S, S, 3) and got.dtype == torch.uint8
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy(), g[f"jit/{k}"]), k
    # every image x every position of the contrast op x both flip orders, at a padded origin, against the two uniform kernels
    orders = [(1, 0, 2, 3), (0, 1, 3, 2), (2, 3, 1, 0), (3, 0, 2, 1)]
    rows, fac, ords = [], [], []
    for i, (H, W) in enumerate(ru.RESIZED):
        for j, o in enumerate(orders):
            rows.append((i, (-2, H - S + 1)[j % 2], (W - S + 2, -1)[j // 2], (i + j) % 2))
            fac.append((0.9 + 0.05 * j, 1.3 - 0.2 * j, 0.6 + 0.3 * j, 0.04 * (j - 1.5)))
            ords.append(o)
    p = torch.tensor(rows, dtype=torch.int32, device="cuda")
    factors, order = torch.tensor(fac, dtype=torch.float32), torch.tensor(ords, dtype=torch.int32)
    for flip_first in (True, False):
        got = data.color_jitter_crop_u8(rs, p, (S, S), factors, order, flip_first)
        for r, (i, top, left, flip) in enumerate(rows):
            whole = data.color_jitter_u8(_alone(rs, i), torch.zeros(1, dtype=torch.int32), factors[r:r + 1], order[r:r + 1])
            q = torch.tensor([[0, top, left, flip]], dtype=torch.int32, device="cuda")
            assert torch.equal(got[r:r + 1], data.crop_flip_u8(whole, q, (S, S), flip_first)), (r, flip_first)
    assert data.color_jitter_crop_u8(rs, p[:0], (S, S), factors[:0], order[:0]).shape == (0, S, S, 3)


# ---------------------------------------------------------------------------------------------------------------- 4. source
def _source(golden, **kw):
    from eoe_amd import data
    ty = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0])
    return data.ResidentImageSource(data.RaggedImageSet(ru.images(3)), data.RaggedImageSet(ru.oe_images(3)), data.RaggedImageSet(ru.images(3)),
                                    ty, crop=S, resize=S, test_resize=S, seed=4, **kw), ty


@pytest.mark.parametrize("jitter", [None, (0.1, 0.2, 0.3, 0.05)])
def test_source_over_ragged_sets(golden, jitter):
    from eoe_amd import data, normalize as norm
    g = golden("g25_ragged")
    src, ty = _source(golden, color_jitter=jitter, noise_std=0.0)
    assert isinstance(src.normal, data.RaggedImageSet) and [tuple(s) for s in src.normal.sizes.tolist()] == ru.RESIZED
    train, test = src.loaders(4)
    assert len(train) == 3
    seen, seen_left = [], set()
    for epoch in range(12):
        for imgs, lbls, idcs in train:
            n = lbls.shape[0] // 2
            assert imgs.is_cuda and imgs.shape == (2 * n, 3, S, S) and imgs.dtype == torch.float32 and torch.isfinite(imgs).all()
            assert lbls[:n].eq(0).all() and lbls[n:].eq(1).all()
            assert idcs[:n].max() < 9 and idcs[n:].min() >= 9 and idcs[n:].max() < 9 + 8
            seen.append(idcs[:n])
            if jitter is not None:
                continue
            # crops of the position-coded image (16 x 97, Resize leaves it alone) decode to a legal origin
            for slot in torch.nonzero(idcs[:n] == ru.CODED).flatten().tolist():
                x = torch.round(imgs[slot] * 255).to(torch.int64).cpu().numpy()
                assert (x[0] == ru.CODED_MARKER).all() and np.array_equal(x[1], np.repeat(np.arange(S)[:, None], S, axis=1))      # top = 0
                cols = x[2][0]
                assert (x[2] == cols[None, :]).all() and (np.array_equal(np.diff(cols), np.ones(S - 1)) or np.array_equal(np.diff(cols), -np.ones(S - 1)))
                assert 0 <= cols.min() and cols.max() <= 96 and cols.max() - cols.min() == S - 1
                seen_left.add(int(cols.min()))
        if epoch == 0:
            assert sorted(torch.cat(seen).tolist()) == list(range(9))                   # every normal image once per epoch
    if jitter is None:
        assert len(seen_left) > 4                                # the origin moves over the long image
    # the test split: CenterCrop(16) of Resize(16), batches as the tensor path builds them
    assert len(test) == 3 and [b[0].shape[0] for b in test] == [4, 4, 1]
    got = torch.cat([b[0] for b in test]).cpu().numpy()
    for i in range(9):
        want = (g[f"cc/bilinear/c3/{i}"].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
        assert np.array_equal(got[i], want), i
    assert torch.equal(torch.cat([b[1] for b in test]), ty) and torch.cat([b[2] for b in test]).tolist() == list(range(9))


def test_source_statistics_are_fitted_over_the_centre_crops(golden):
    from eoe_amd import normalize as norm
    g = golden("g25_ragged")
    rows = [0, 2, 5, 6, 8]
    src, _ = _source(golden, normalize="normalize", normal_index=rows)
    crops = torch.from_numpy(np.stack([g[f"cc/bilinear/c3/{i}"] for i in range(9)])).cuda()
    assert src.ds_statistics == norm.fit_statistics(crops, torch.tensor(rows), "normalize")
    assert src.ds_statistics != norm.fit_statistics(crops, None, "normalize") and list(src.mean) == src.ds_statistics["mean"]
    train, _ = src.loaders(4)
    assert len(train) == 2 and sorted(torch.cat([b[2][: b[1].shape[0] // 2] for b in train]).tolist()) == rows
    gcn, _ = _source(golden, normalize="gcn-normalize")
    assert gcn.ds_statistics == norm.fit_statistics(crops, None, "gcn-normalize")
    src.set_oe_subset([1, 6])
    oe_idcs = torch.cat([b[2][b[1].shape[0] // 2:] for b in src.loaders(4)[0]])
    assert set(oe_idcs.tolist()) <= {9 + 1, 9 + 6}


def _big(i, H, W):
    """a 3-channel image of the trainer test: dark for the normal class, bright for the rest"""
    return ru.image(i, H, W, 3) // 2 + (0 if i % 2 == 0 else 120)


def test_labelled_set_with_ragged_train_and_test_trains_cnn32(tmp_path):
    """every layer connected: LabelledImageSet over ragged train / test / OE sets of about 40 x 52 -> per-image crop draws -> the
    ragged augment kernel -> CNN32 -> HSC; finite losses, and the test scores of two runs are equal"""
    import json
    from eoe_amd import data
    from eoe_amd.training.ad_trainer import JsonLogger
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    shapes = [(40, 52), (52, 40), (41, 49), (38, 55), (44, 44), (32, 61), (47, 33)]
    train = [_big(i, *shapes[i % 7]) for i in range(32)]
    train_y = torch.tensor([i % 2 for i in range(32)])
    test = [_big(i + 1, *shapes[(i + 3) % 7]) for i in range(16)]
    test_y = torch.tensor([(i + 1) % 2 for i in range(16)])
    oe = [_big(2 * i + 1, *shapes[(i + 5) % 7]) for i in range(12)]

    def run(logdir):
        torch.manual_seed(0)
        lset = data.LabelledImageSet(data.RaggedImageSet(train), train_y, data.RaggedImageSet(test), test_y, data.RaggedImageSet(oe),
                                     ["dark", "bright"], crop=32, normalize="normalize")
        tr = TRAINER["hsc"](CNN32(bias=True), dataset=lset, epochs=2, lr=1e-3, wdk=0.0, milestones=[], batch_size=8, logger=JsonLogger(logdir))
        _, res = tr.run(run_classes=[0], run_seeds=1)
        assert len(tr.last_losses) == 2 * 2 and all(np.isfinite(tr.last_losses)) and np.isfinite(res["mean_auc"])
        la, sc = tr.last_scores[-1]                            # the last epoch's step batches: 16 normal + 16 OE samples
        assert la.shape == (32,) and sc.shape == (32,) and torch.isfinite(sc).all()
        with open(f"{logdir}/eval_cls0_it0_anomaly_scores.json") as f:
            scores = json.load(f)
        assert len(scores) == 16 and all(np.isfinite(v) for v in scores.values())
        return scores, sc.clone()

    (test_a, train_a), (test_b, train_b) = run(str(tmp_path / "a")), run(str(tmp_path / "b"))
    assert test_a == test_b and torch.equal(train_a, train_b)
