"""GPU tier of CLIP's preprocessing on image sets of mixed sizes: the windowed ragged Resize (`data.clip_preprocess_ragged`,
`data.resize_window_u8`) against Pillow's bytes and against the composed device path (whole Resize, then the ragged centre crop), the
unwindowed Resize through the changed kernel, `ResidentImageSource` / `LabelledImageSet` with `clip_preprocessing=` over ragged sets,
and one CLIP trainer run fed from raw ragged sets at 224."""
import zlib

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")

import clip_ragged_util as cu              # noqa: E402
import ragged_util as ru                   # noqa: E402

pytestmark = pytest.mark.gpu

P = cu.N_PX
_PILLOW = {}


def _pillow(key, imgs, n_px):
    """Pillow's results, computed once per image list and shared"""
    if key not in _PILLOW:
        want = np.stack([cu.pillow_clip(a, n_px) for a in imgs])
        want.setflags(write=False)
        _PILLOW[key] = want
    return _PILLOW[key]


def _composed(rs, n_px):
    """the device path that existed: the WHOLE bicubic Resize of every image, then the ragged centre crop"""
    from eoe_amd import data
    full = data.resize_u8(rs, n_px, "bicubic")
    tl = torch.from_numpy(data.center_origins(full.sizes, n_px))
    idx = torch.arange(len(full))
    p = torch.stack([idx, tl[:, 0], tl[:, 1], torch.zeros_like(idx)], dim=1).to(torch.int32).cuda()
    return data.crop_flip_u8(full, p, (n_px, n_px), True)


def _sentinel_out(n, n_px, lead=19, value=0xC3):
    """a [n, n_px, n_px, 3] view at an odd address inside a buffer of `value` bytes"""
    count = n * n_px * n_px * 3
    buf = torch.full((count + 64,), value, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + count].view(n, n_px, n_px, 3), lead, count


# ------------------------------------------------------------------------------------------------------------- the window
def test_case_table_equals_pillow_and_the_composed_path():
    from eoe_amd import data
    imgs = cu.images()
    want = _pillow("table", imgs, P)
    rs = cu.packed_set(imgs, "cuda")                          # first image at the arena's start, last at its end, odd starts between
    assert int(rs.offsets_host[0]) == 0 and int(rs.offsets_host[-1]) + imgs[-1].size == rs.arena.numel()
    assert (rs.offsets_host[1:-1] % 16 != 0).any()
    before = rs.arena.clone()
    buf, out, lead, count = _sentinel_out(len(imgs), P)
    got = data.clip_preprocess_ragged(rs, P, out=out)
    assert got is out and got.shape == (len(imgs), P, P, 3) and got.dtype == torch.uint8
    for i in range(len(imgs)):
        assert np.array_equal(got[i].cpu().numpy(), want[i]), cu.SHAPES[i]
    assert (buf[:lead] == 0xC3).all() and (buf[lead + count:] == 0xC3).all()          # nothing in front of or behind the result
    assert torch.equal(rs.arena, before)                                                # the source arena is untouched
    composed = _composed(rs, P)
    assert torch.equal(got, composed)
    again = data.clip_preprocess_ragged(rs, P)                                          # a second call, into memory of its own
    assert again.is_contiguous() and torch.equal(again, got)
    # the same images at the aligned starts of RaggedImageSet(list), and in reverse order
    assert torch.equal(data.clip_preprocess_ragged(data.RaggedImageSet(imgs, device="cuda"), P), got)
    rev = data.clip_preprocess_ragged(cu.packed_set(imgs[::-1], "cuda"), P)
    assert torch.equal(rev, got.flip(0))
    # clip_preprocess dispatches: the same bytes through ToTensor and CLIP's Normalize
    f = data.clip_preprocess(rs, P)
    assert f.shape == (len(imgs), 3, P, P) and torch.equal(f.cpu(), torch.from_numpy(cu.normalized(want, data.CLIP_MEAN, data.CLIP_STD)))


def test_realistic_pair_at_224():
    from eoe_amd import data
    imgs = cu.images(cu.BIG_SHAPES, salt=5)
    want = _pillow("big", imgs, cu.BIG_N_PX)
    rs = data.RaggedImageSet(imgs, device="cuda")
    buf, out, lead, count = _sentinel_out(2, cu.BIG_N_PX, lead=7)
    got = data.clip_preprocess_ragged(rs, cu.BIG_N_PX, out=out)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (buf[:lead] == 0xC3).all() and (buf[lead + count:] == 0xC3).all()
    assert torch.equal(got, _composed(rs, cu.BIG_N_PX))
    assert data.clip_window(rs.sizes, 224).tolist() == [[0, 37, 224, 224], [56, 0, 224, 224]]     # 224 x 298 and 336 x 224


def test_a_set_that_is_n_px_square_already_comes_back_unchanged():
    from eoe_amd import data
    imgs = [ru.image(i, P, P, 3) for i in range(4)]
    rs = data.RaggedImageSet(imgs, device="cuda")
    got = data.clip_preprocess_ragged(rs, P)
    assert got.shape == (4, P, P, 3) and np.array_equal(got.cpu().numpy(), np.stack(imgs))
    buf, out, lead, count = _sentinel_out(4, P)
    assert data.clip_preprocess_ragged(rs, P, out=out) is out and np.array_equal(out.cpu().numpy(), np.stack(imgs))
    assert (buf[:lead] == 0xC3).all() and (buf[lead + count:] == 0xC3).all()


def test_window_argument_errors_leave_the_output_alone():
    from eoe_amd import data
    rs = cu.packed_set(cu.images(), "cuda")
    good = data.clip_window(rs.sizes, P)
    buf, out, _, _ = _sentinel_out(len(rs), P)
    for row, col, val in ((1, 1, -1), (2, 0, -1), (1, 1, 6), (2, 0, 6), (4, 1, 10), (0, 0, 1)):
        bad = good.copy()
        bad[row, col] = val
        with pytest.raises(ValueError, match=f"of image {row} lies outside its resized image"):
            data.resize_window_u8(rs, P, bad, "bicubic", out=out)
    with pytest.raises(ValueError, match="one height and width"):
        data.resize_window_u8(rs, P, good[:-1], "bicubic", out=out)
    with pytest.raises(ValueError, match="out must be"):
        data.resize_window_u8(rs, P, good, "bicubic", out=out.cpu())
    torch.cuda.synchronize()
    assert (buf == 0xC3).all()
    # other windows than the centre one: the four corners of each resized image and a smaller window, against the composed path
    full = data.resize_u8(rs, P, "bicubic")
    for k, (fy, fx, hh, ww) in enumerate([(0, 0, P, P), (1, 1, P, P), (0, 1, 5, 7), (1, 0, 1, 1)]):
        win = np.array([[fy * (h - hh), fx * (w - ww), hh, ww] for h, w in full.sizes.tolist()])
        got = data.resize_window_u8(rs, P, win, "bicubic")
        p = torch.tensor([[i, int(win[i, 0]), int(win[i, 1]), 0] for i in range(len(rs))], dtype=torch.int32, device="cuda")
        assert torch.equal(got, data.crop_flip_u8(full, p, (hh, ww), True)), k
    lin = data.resize_window_u8(rs, P, good, "bilinear")
    full = data.resize_u8(rs, P, "bilinear")
    p = torch.tensor([[i, int(good[i, 0]), int(good[i, 1]), 0] for i in range(len(rs))], dtype=torch.int32, device="cuda")
    assert torch.equal(lin, data.crop_flip_u8(full, p, (P, P), True))


@pytest.mark.parametrize("filt,pil", [("bicubic", "BICUBIC"), ("bilinear", "BILINEAR")])
def test_field_eight_zero_is_the_whole_resize_it_was(filt, pil):
    """`resize_u8` builds descriptors whose eighth field is 0: the bytes are Pillow's, as on the commit before the field had a
    meaning; and a window that is the whole resized image gives the same bytes"""
    from PIL import Image
    from eoe_amd import data
    imgs = cu.images()
    rs = cu.packed_set(imgs, "cuda")
    out = data.resize_u8(rs, P, filt)
    for i, a in enumerate(imgs):
        h, w = cu.resized_hw(a.shape[0], a.shape[1], P)
        assert np.array_equal(out[i].cpu().numpy(), np.asarray(Image.fromarray(a).resize((w, h), getattr(Image, pil)))), cu.SHAPES[i]
    sq = data.resize_u8(rs, (7, 10), filt)
    for i, a in enumerate(imgs):
        assert np.array_equal(sq[i].cpu().numpy(), np.asarray(Image.fromarray(a).resize((10, 7), getattr(Image, pil)))), cu.SHAPES[i]
    whole = np.array([[0, 0, 7, 10]] * len(imgs))
    assert torch.equal(data.resize_window_u8(rs, (7, 10), whole, filt), sq)


# ------------------------------------------------------------------------------------------------------------- the source
TRAIN_SHAPES = [(12, 17), (17, 12), (10, 10), (23, 11), (11, 30), (15, 15), (10, 13), (40, 12)]


def _sets():
    from eoe_amd import data
    normal = data.RaggedImageSet([ru.image(i, h, w, 3) for i, (h, w) in enumerate(TRAIN_SHAPES)])
    oe = data.RaggedImageSet([ru.image(i + 30, h, w, 3) for i, (h, w) in enumerate(TRAIN_SHAPES[::-1][:6])])
    test_imgs = cu.images()
    lab = torch.tensor([i % 2 for i in range(len(test_imgs))])
    return normal, oe, data.RaggedImageSet(test_imgs), test_imgs, lab


def _check_test_batches(tst, test_imgs, lab, bs):
    from eoe_amd import data
    want = torch.from_numpy(cu.normalized(_pillow("table", test_imgs, P), data.CLIP_MEAN, data.CLIP_STD))
    assert isinstance(tst, list) and len(tst) == -(-len(test_imgs) // bs)
    got = torch.cat([b[0] for b in tst])
    assert got.shape == (len(test_imgs), 3, P, P) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got.cpu(), want)                      # the bar of test_gpu_clip_pre.py for its test batches: equal bits
    assert torch.equal(torch.cat([b[1] for b in tst]), lab) and torch.cat([b[2] for b in tst]).tolist() == list(range(len(test_imgs)))


@pytest.mark.parametrize("jitter", [None, (0.1, 0.2, 0.3, 0.05)])
def test_source_over_three_ragged_sets(jitter):
    from eoe_amd import data
    normal, oe, test, test_imgs, lab = _sets()
    kw = dict(crop=P, resize=10, padding=1, seed=3, color_jitter=jitter, interpolation="bilinear")
    src = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=P, **kw)       # construction: refused before
    assert isinstance(src.normal, data.RaggedImageSet) and isinstance(src.oe, data.RaggedImageSet)
    assert isinstance(src.test, torch.Tensor) and src.test.shape == (len(test_imgs), P, P, 3) and src.test.is_cuda
    assert tuple(src.mean) == data.CLIP_MEAN and tuple(src.std) == data.CLIP_STD and src.normalize is None
    uniform_test = torch.zeros((len(test_imgs), P, P, 3), dtype=torch.uint8)
    twin = data.ResidentImageSource(normal, oe, uniform_test, lab, mean=data.CLIP_MEAN, std=data.CLIP_STD, **kw)
    (ta, tst), (tb, _) = src.loaders(4), twin.loaders(4)
    steps = 0
    for _ in range(3):
        for (xa, ya, ia), (xb, yb, ib) in zip(ta, tb):
            assert xa.shape == (8, 3, P, P) and xa.dtype == torch.float32
            assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ia, ib)
            steps += 1
    assert steps == 6
    _check_test_batches(tst, test_imgs, lab, 4)
    # three given values win over CLIP's
    own = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=P, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.4), **kw)
    twin = data.ResidentImageSource(normal, oe, uniform_test, lab, mean=(0.5, 0.4, 0.3), std=(0.2, 0.3, 0.4), **kw)
    assert torch.equal(next(iter(own.loaders(4)[0]))[0], next(iter(twin.loaders(4)[0]))[0])


def test_source_with_only_the_test_set_ragged():
    from eoe_amd import data
    _, _, test, test_imgs, lab = _sets()
    normal = torch.from_numpy(np.stack([ru.image(i, 10, 10, 3) for i in range(8)]))
    oe = torch.from_numpy(np.stack([ru.image(i + 40, 10, 10, 3) for i in range(6)]))
    kw = dict(crop=P, padding=1, seed=5)
    src = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=P, **kw)
    twin = data.ResidentImageSource(normal, oe, torch.zeros((len(lab), P, P, 3), dtype=torch.uint8), lab, mean=data.CLIP_MEAN,
                                    std=data.CLIP_STD, **kw)
    (ta, tst), (tb, _) = src.loaders(3), twin.loaders(3)
    for _ in range(2):
        for (xa, _, ia), (xb, _, ib) in zip(ta, tb):
            assert torch.equal(xa, xb) and torch.equal(ia, ib)
    _check_test_batches(tst, test_imgs, lab, 3)
    # tensor halves that ARE upsampled (6 -> 8, the small-image runners' kernel) beside the ragged test set: each set on its own
    up = data.ResidentImageSource(normal, oe, test, lab, crop=6, clip_preprocessing=P, seed=5)
    x = next(iter(up.loaders(3)[0]))[0]
    assert x.shape == (6, 3, P, P) and torch.isfinite(x).all()
    _check_test_batches(up.loaders(3)[1], test_imgs, lab, 3)
    # resize=(h, w) turns ragged halves into tensors: the tensor path under the option (train_clip_imagenet.py:28)
    rn, ro, _, _, _ = _sets()
    sq = data.ResidentImageSource(rn, ro, test, lab, crop=P, resize=(10, 10), clip_preprocessing=P, seed=5)
    ref = data.ResidentImageSource(data.resize_u8(rn.to("cuda"), (10, 10)), data.resize_u8(ro.to("cuda"), (10, 10)),
                                   torch.zeros((len(lab), P, P, 3), dtype=torch.uint8), lab, crop=P, mean=data.CLIP_MEAN, std=data.CLIP_STD,
                                   seed=5)
    assert isinstance(sq.normal, torch.Tensor) and sq.normal.shape == (8, 10, 10, 3)
    assert torch.equal(next(iter(sq.loaders(4)[0]))[0], next(iter(ref.loaders(4)[0]))[0])


def test_labelled_set_hands_the_option_to_its_tasks():
    from eoe_amd import data
    normal, oe, test, test_imgs, _ = _sets()
    train_classes = torch.arange(len(normal)) % 2
    test_classes = torch.arange(len(test_imgs)) % 2
    lset = data.LabelledImageSet(normal, train_classes, test, test_classes, oe, ["a", "b"], P, resize=10, padding=1, clip_preprocessing=P)
    assert isinstance(lset.test, torch.Tensor) and lset.test.shape == (len(test_imgs), P, P, 3)      # converted once, for every task
    task = lset.source([1], seed=3)
    direct = data.ResidentImageSource(normal, oe, test, data.ad_targets(test_classes, [1]), P, resize=10, padding=1, seed=3,
                                      normal_index=data.normal_subset(train_classes, [1]), clip_preprocessing=P)
    assert task.clip_preprocessing == P and task.test is lset.test
    (t1, s1), (t2, s2) = task.loaders(4), direct.loaders(4)
    got, want = list(t1), list(t2)
    assert len(got) == 1 and got[0][0].shape == (8, 3, P, P)
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][2], want[0][2])
    assert len(s1) == len(s2) and all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(s1, s2))
    _check_test_batches(s1, test_imgs, data.ad_targets(test_classes, [1]), 4)


# ------------------------------------------------------------------------------------------------------------- end to end
def _fake_tokenizer(vocab=1000, ctx=77):
    """clip.tokenize's contract (str -> int64 [1, ctx], [SOT, ids..., EOT, 0...]) with a deterministic word hash"""
    def tok(text):
        ids = [vocab - 2] + [1 + zlib.crc32(w.encode()) % (vocab - 3) for w in text.split()] + [vocab - 1]
        out = torch.zeros(1, ctx, dtype=torch.int64)
        out[0, :len(ids)] = torch.tensor(ids)
        return out
    return tok


def test_clip_trainer_runs_on_raw_ragged_sets_at_224(monkeypatch):
    """the train_clip_cub chain end to end: raw images of mixed sizes, Resize(256) with the aspect ratio kept, ColorJitter,
    RandomCrop(224), CLIP's Normalize; the test split through CLIP's own transform; the smallest CLIP of the trainer tests (2 layers,
    width 256, the "small" text tower), one epoch of one step"""
    from eoe_amd import data
    from eoe_amd.models import CLIP
    from eoe_amd.training import TRAINER, ADTrainer
    monkeypatch.setattr(ADTrainer, "KEEP_SNAPSHOT_IN_RAM", True)
    torch.manual_seed(0)
    shapes = [(300, 400), (400, 300), (260, 260), (375, 500), (500, 333), (256, 300), (280, 610), (330, 270)]
    normal = data.RaggedImageSet([ru.image(i, h, w, 3) // 2 for i, (h, w) in enumerate(shapes)])
    oe = data.RaggedImageSet([ru.image(i + 9, h, w, 3) // 2 + 120 for i, (h, w) in enumerate(shapes[::-1])])
    test = data.RaggedImageSet([ru.image(i + 20, h, w, 3) // 2 + (120 if i % 2 else 0) for i, (h, w) in enumerate(shapes[2:] + shapes[:2])])
    lab = torch.tensor([i % 2 for i in range(8)])
    src = data.ResidentImageSource(normal, oe, test, lab, crop=224, resize=256, seed=1, color_jitter=(0.01,) * 4, clip_preprocessing=224)
    assert src.test.shape == (8, 224, 224, 3) and isinstance(src.normal, data.RaggedImageSet)
    model = CLIP(64, 224, 2, 256, 32, 77, 1000, 128, 2, 2)
    tr = TRAINER["clip"](model, dataset=src, epochs=1, lr=1e-3, batch_size=8, tokenizer=_fake_tokenizer())
    models, res = tr.run(run_classes=[0])
    assert len(tr.last_losses) > 0 and np.isfinite(tr.last_losses).all()
    assert np.isfinite(res["mean_auc"]) and 0.0 <= res["mean_auc"] <= 1.0
    trained = models[0][0].cuda().eval()
    x = next(iter(src.loaders(8)[1]))[0]
    with torch.no_grad():
        scores = tr.compute_anomaly_score(trained(x), tr.center)
    assert scores.shape[0] == 8 and torch.isfinite(scores).all()
