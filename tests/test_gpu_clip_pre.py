"""GPU tier: CLIP's preprocessing inside the train chain -- eoe_augment_resize_batch against the oracle chain of tests/clip_pre_util.py
(bytes exact, fp32 exact without noise) and against the composed GPU chain crop_flip_u8 -> resize_u8 -> channel repeat -> augment_batch
(bitwise, with noise), ResidentImageSource / LabelledImageSet with clip_preprocessing=, and one ADClipTrainer run fed by such a source."""
import zlib

import numpy as np
import pytest
import torch

import clip_pre_util as cu

pytestmark = pytest.mark.gpu

MEAN, STD = cu.CLIP_MEAN, cu.CLIP_STD

# name -> (n_src, Hs, Ws, C, S, P, padding, n, flip_first, filter)
CASES = {
    "cifar": (11, 32, 32, 3, 32, 224, 4, 6, False, "bicubic"),          # main/train_clip_cifar.py
    "fmnist": (11, 28, 28, 1, 28, 224, 3, 6, True, "bicubic"),          # main/train_clip_fmnist.py
    "odd_rgb_ff1": (13, 17, 20, 3, 9, 23, 3, 37, True, "bicubic"),      # P % 4 != 0, two bands, padded zeros in the filter
    "odd_rgb_ff0": (13, 17, 20, 3, 9, 23, 3, 37, False, "bicubic"),
    "odd_l_ff1": (13, 17, 20, 1, 9, 23, 3, 37, True, "bicubic"),
    "odd_l_ff0": (13, 17, 20, 1, 9, 23, 3, 37, False, "bicubic"),
    "bilinear": (13, 17, 20, 3, 9, 23, 3, 37, True, "bilinear"),
    "same12": (5, 16, 16, 3, 12, 12, 2, 7, True, "bicubic"),            # S = P: the identity
    "same12_l": (5, 16, 16, 1, 12, 12, 2, 7, True, "bicubic"),          # ... and only the replication
    "one": (3, 32, 32, 3, 32, 224, 4, 1, True, "bicubic"),              # n = 1
    "five": (7, 28, 32, 1, 28, 224, 3, 5, False, "bicubic"),            # n = 5 at P = 224, a source that is not square
}


def _inputs(name):
    n_src, Hs, Ws, C, S, P, pad, n, ff, filt = CASES[name]
    src = cu.images(name.split("_")[0], n_src, Hs, Ws, C)
    return src, cu.params(name.split("_")[0], n, n_src, Hs, Ws, S, pad)


_ORACLE = {}


def _oracle_bytes(name):
    """computed once per case and shared"""
    if name not in _ORACLE:
        _, _, _, _, S, P, _, _, ff, filt = CASES[name]
        src, p = _inputs(name)
        b = cu.oracle_bytes(src, p, S, P, ff, filt)
        b.setflags(write=False)
        _ORACLE[name] = b
    return _ORACLE[name]


def _composed(src, p, S, P, mean, std, flip_first, noise_std, seed, filt="bicubic"):
    """the chain from the existing kernels: crop_flip_u8 -> resize_u8 -> channel repeat -> augment_batch with identity params"""
    from eoe_amd import data
    u8 = data.resize_u8(data.crop_flip_u8(src, p, (S, S), flip_first), (P, P), filt)
    if u8.shape[3] == 1:
        u8 = u8.repeat(1, 1, 1, 3).contiguous()
    ident = torch.zeros_like(p)
    ident[:, 0] = torch.arange(p.shape[0], dtype=torch.int32, device=p.device)
    return data.augment_batch(u8, ident, (P, P), mean, std, True, noise_std, seed)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_vs_oracle_and_composed_chain(name):
    from eoe_amd.data import augment_resize_batch
    _, _, _, _, S, P, _, n, ff, filt = CASES[name]
    src_np, p_np = _inputs(name)
    src, p = torch.from_numpy(src_np).cuda(), torch.from_numpy(p_np).cuda()
    want_u8 = _oracle_bytes(name)
    # stages 1-4 are integer arithmetic: the bytes are the oracle's
    raw = augment_resize_batch(src, p, S, P, None, None, ff, 0.0, 0, filt)
    assert raw.shape == (n, 3, P, P) and raw.dtype == torch.float32
    got_u8 = torch.round(raw * 255.0).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(got_u8, want_u8)
    assert torch.equal(raw.cpu(), torch.from_numpy(cu.oracle_f32(want_u8)))
    # ... and ToTensor / Normalize are two fp32 operations: bit-exact (as test_augment_kernel_vs_oracle asserts for the same two)
    got = augment_resize_batch(src, p, S, P, MEAN, STD, ff, 0.0, 0, filt)
    assert torch.equal(got.cpu(), torch.from_numpy(cu.oracle_f32(want_u8, MEAN, STD)))
    # with noise: the bar of test_augment_kernel_vs_oracle for the same noise arithmetic
    got = augment_resize_batch(src, p, S, P, MEAN, STD, ff, 0.001, 5, filt)
    diff = (got.cpu() - torch.from_numpy(cu.oracle_f32(want_u8, MEAN, STD, 0.001, 5))).abs().max().item()
    print(f"{name}: max |diff| with noise {diff:.3e}")
    assert diff < 2e-6
    # bitwise the composed GPU chain, with and without noise and Normalize
    assert torch.equal(got, _composed(src, p, S, P, MEAN, STD, ff, 0.001, 5, filt))
    assert torch.equal(augment_resize_batch(src, p, S, P, None, None, ff, 0.001, 9, filt), _composed(src, p, S, P, None, None, ff, 0.001, 9, filt))
    assert torch.equal(raw, _composed(src, p, S, P, None, None, ff, 0.0, 0, filt))


@pytest.mark.parametrize("n,C,S,P,pad", [(256, 3, 32, 224, 4), (256, 1, 28, 224, 3), (2050, 3, 9, 23, 3)])
def test_band_layouts_of_large_batches_equal_the_composed_chain(n, C, S, P, pad):
    """the training batch size (8 bands of 28 rows at P = 224) and a batch so large that a slot is one band: bitwise the composed chain
    (the small cases above, which the oracle checks, run with the most bands)"""
    from eoe_amd.data import augment_resize_batch
    src = torch.from_numpy(cu.images(f"big{C}", 64, S, S + 4, C)).cuda()
    p = torch.from_numpy(cu.params(f"big{n}", n, 64, S, S + 4, S, pad)).cuda()
    got = augment_resize_batch(src, p, S, P, MEAN, STD, False, 0.001, 3)
    assert torch.equal(got, _composed(src, p, S, P, MEAN, STD, False, 0.001, 3))


def test_an_unaligned_output_and_an_index_outside_the_set():
    """an output that is not 16-byte aligned takes the scalar stores; a slot whose index lies outside the set is all padding"""
    from eoe_amd import _lib, data
    src = torch.from_numpy(cu.images("cifar", 11, 32, 32, 3)).cuda()
    p = torch.from_numpy(cu.params("cifar", 3, 11, 32, 32, 32, 4)).cuda()
    want = data.augment_resize_batch(src, p, 32, 224, MEAN, STD, False, 0.001, 5)
    buf = torch.full((want.numel() + 8,), 7.0, device="cuda")
    out = buf[1:1 + want.numel()]
    assert out.data_ptr() % 16 == 4
    bounds, kk = data._cached_resize_tables(32, 224, _lib.EOE_RESIZE_BICUBIC, src.device)
    m, s = torch.tensor(MEAN, device="cuda"), torch.tensor(STD, device="cuda")
    _lib.check(_lib.lib.eoe_augment_resize_batch(src.data_ptr(), 11, 32, 32, 3, p.data_ptr(), 32, 32, 224, _lib.EOE_RESIZE_BICUBIC,
                                                 bounds.data_ptr(), kk.data_ptr(), m.data_ptr(), s.data_ptr(), out.data_ptr(), 3, 0, 0.001, 5,
                                                 torch.cuda.current_stream().cuda_stream), "eoe_augment_resize_batch")
    assert torch.equal(out.view_as(want), want) and buf[0].item() == 7.0 and (buf[1 + want.numel():] == 7.0).all()
    assert data._cached_resize_tables(32, 224, _lib.EOE_RESIZE_BICUBIC, src.device)[0] is bounds          # uploaded once
    for C in (3, 1):
        s8 = torch.from_numpy(cu.images("outside", 4, 12, 12, C)).cuda()
        q = torch.tensor([[1, 0, 0, 0], [4, 0, 0, 0], [-1, 1, 1, 1]], dtype=torch.int32, device="cuda")
        o = data.augment_resize_batch(s8, q, 12, 23, None, None, True, 0.0, 0)
        assert o[0].abs().sum() > 0 and (o[1:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the source
def _rgb_sets():
    lab = torch.cat([torch.zeros(8, dtype=torch.int64), torch.ones(8, dtype=torch.int64)])
    return (torch.from_numpy(cu.images("src/n", 16, 32, 32, 3)), torch.from_numpy(cu.images("src/o", 16, 32, 32, 3)),
            torch.from_numpy(cu.images("src/t", 16, 32, 32, 3)), lab)


def _gray_sets():
    lab = torch.cat([torch.zeros(8, dtype=torch.int64), torch.ones(8, dtype=torch.int64)])
    return (torch.from_numpy(cu.images("src/gn", 16, 28, 28, 1)), torch.from_numpy(cu.images("src/go", 16, 32, 32, 3)),
            torch.from_numpy(cu.images("src/gt", 16, 28, 28, 1)), lab)


def _first_batch_by_hand(twin, b, S, P, mean, std):
    """the first step batch of a source with the draws of `twin` (a source with the same seed and no clip_preprocessing, whose
    generator is consumed here in the order of ResidentImageSource._epoch), put through the composed chain"""
    n = twin.normal.shape[0]
    perm = torch.randperm(n, generator=twin._g)
    oe_order = torch.arange(twin.oe.shape[0])[torch.randperm(twin.oe.shape[0], generator=twin._g)]
    ni, oi = perm[:b], oe_order[:b]
    pn = twin._params(ni, twin.normal.shape[1], twin.normal.shape[2]).cuda()
    po = twin._params(oi, twin.oe.shape[1], twin.oe.shape[2]).cuda()
    seed = (twin.seed * 65521 + 1) % (1 << 23)
    xn = _composed(twin.normal, pn, S, P, mean, std, twin.flip_first, twin.noise_std, 2 * seed)
    xo = _composed(twin.oe, po, S, P, mean, std, twin.flip_first, twin.noise_std, 2 * seed + 1)
    return torch.cat([xn, xo]), torch.cat([ni, oi + n])


def test_source_rgb_train_and_test_batches():
    from eoe_amd import data
    normal, oe, test, lab = _rgb_sets()
    kw = dict(crop=32, padding=4, flip_first=False, seed=3)
    src = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=224, **kw)
    train, tst = src.loaders(8)
    batches = list(train)
    assert len(batches) == 2 and len(train) == 2
    for x, y, idc in batches:
        assert x.shape == (16, 3, 224, 224) and x.dtype == torch.float32 and x.is_cuda
        assert y[:8].eq(0).all() and y[8:].eq(1).all() and idc[:8].max() < 16 and idc[8:].min() >= 16
    twin = data.ResidentImageSource(normal, oe, test, lab, **kw)
    want, idc = _first_batch_by_hand(twin, 8, 32, 224, data.CLIP_MEAN, data.CLIP_STD)
    assert torch.equal(batches[0][0], want) and torch.equal(batches[0][2], idc)
    # test batches: CLIP's own transform on the raw images, one batch at a time
    assert len(tst) == 2 and not isinstance(tst, list)
    got = list(tst)
    want = data.clip_preprocess(test.cuda(), 224)
    assert torch.equal(torch.cat([g[0] for g in got]), want) and got[0][0].shape == (8, 3, 224, 224)
    assert torch.equal(torch.cat([g[1] for g in got]), lab) and torch.equal(torch.cat([g[2] for g in got]), torch.arange(16))
    assert torch.equal(torch.cat([g[0] for g in tst]), want)                                 # iterable again (eval after every epoch)
    # deferred Normalize (what an MSM run asks for): batches in [0, 1] + noise, (mean, std) reported
    src.defer_normalize(True)
    x = next(iter(src.loaders(8)[1]))[0]
    assert src.normalize == (data.CLIP_MEAN, data.CLIP_STD) and 0.0 <= x.min().item() and x.max().item() <= 1.0


def test_source_gray_with_a_colour_oe_set():
    from eoe_amd import data
    normal, oe, test, lab = _gray_sets()
    kw = dict(crop=28, padding=3, seed=5, grayscale=True, resize=28, interpolation="bilinear")
    src = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=224, **kw)
    assert src.oe.shape == (16, 28, 28, 1) and tuple(src.mean) == data.CLIP_MEAN
    train, tst = src.loaders(8)
    x, y, idc = next(iter(train))
    assert x.shape == (16, 3, 224, 224)
    assert torch.isfinite(x).all() and y[:8].eq(0).all() and y[8:].eq(1).all()
    twin = data.ResidentImageSource(normal, oe, test, lab, **kw)
    want, widc = _first_batch_by_hand(twin, 8, 28, 224, data.CLIP_MEAN, data.CLIP_STD)
    assert torch.equal(x, want) and torch.equal(idc, widc)
    got = torch.cat([g[0] for g in tst])
    assert torch.equal(got, data.clip_preprocess(test.cuda().repeat(1, 1, 1, 3).contiguous(), 224))    # the replicated-channel form
    # S = P with one channel is no identity: the byte goes to three channels
    same = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=28, **kw)
    xs = next(iter(same.loaders(8)[0]))[0]
    twin = data.ResidentImageSource(normal, oe, test, lab, **kw)
    assert xs.shape == (16, 3, 28, 28) and torch.equal(xs, _first_batch_by_hand(twin, 8, 28, 28, data.CLIP_MEAN, data.CLIP_STD)[0])


def test_source_identity_stage_and_refusals():
    from eoe_amd import data
    from eoe_amd.msm import MSM
    normal, oe, test, lab = _rgb_sets()
    kw = dict(crop=32, padding=4, seed=3)
    a = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=32, **kw)
    b = data.ResidentImageSource(normal, oe, test, lab, mean=data.CLIP_MEAN, std=data.CLIP_STD, **kw)
    (ta, sa), (tb, sb) = a.loaders(8), b.loaders(8)
    for (xa, ya, ia), (xb, yb, ib) in zip(ta, tb):
        assert xa.shape == (16, 3, 32, 32) and torch.equal(xa, xb) and torch.equal(ia, ib)
    assert isinstance(sa, list) and all(torch.equal(u[0], v[0]) for u, v in zip(sa, sb))
    with pytest.raises(ValueError, match="normalize="):
        data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=224, normalize="normalize", **kw)
    with pytest.raises(ValueError, match="square test images"):
        data.ResidentImageSource(normal, oe, test[:, :, :30].contiguous(), lab, clip_preprocessing=224, **kw)
    with pytest.raises(ValueError, match="square crop"):
        data.ResidentImageSource(normal, oe, test, lab, crop=(32, 28), clip_preprocessing=224)
    src = data.ResidentImageSource(normal, oe, test, lab, clip_preprocessing=224, **kw)
    with pytest.raises(NotImplementedError, match="sharpen"):
        src.pre_tensor_msms([MSM.load("sharpen+train_oe--M4")])
    with pytest.raises(_lib_error(), match="crop <= 64"):
        data.augment_resize_batch(torch.zeros((2, 80, 80, 3), dtype=torch.uint8, device="cuda"),
                                  torch.zeros((2, 4), dtype=torch.int32, device="cuda"), 72, 224)


def _lib_error():
    from eoe_amd import _lib
    return _lib.EoeError


def test_labelled_set_hands_the_option_to_its_tasks():
    from eoe_amd import data
    normal, oe, test, _ = _rgb_sets()
    classes = torch.arange(16) % 2
    lset = data.LabelledImageSet(normal, classes, test, classes, oe, ["a", "b"], 32, padding=4, flip_first=False, clip_preprocessing=224)
    task = lset.source([1], seed=3)
    direct = data.ResidentImageSource(normal, oe, test, data.ad_targets(classes, [1]), 32, padding=4, flip_first=False, seed=3,
                                      normal_index=data.normal_subset(classes, [1]), clip_preprocessing=224)
    (t1, s1), (t2, s2) = task.loaders(8), direct.loaders(8)
    got, want = list(t1), list(t2)
    assert len(got) == 1 and got[0][0].shape == (16, 3, 224, 224)
    assert torch.equal(got[0][0], want[0][0]) and torch.equal(got[0][2], want[0][2])
    for u, v in zip(s1, s2):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])


# ---------------------------------------------------------------------------------------------------------------- end to end
def _fake_tokenizer(vocab=1000, ctx=77):
    """clip.tokenize's contract (str -> int64 [1, ctx], [SOT, ids..., EOT, 0...]) with a deterministic word hash"""
    def tok(text):
        ids = [vocab - 2] + [1 + zlib.crc32(w.encode()) % (vocab - 3) for w in text.split()] + [vocab - 1]
        out = torch.zeros(1, ctx, dtype=torch.int64)
        out[0, :len(ids)] = torch.tensor(ids)
        return out
    return tok


def test_clip_trainer_runs_on_a_clip_preprocessing_source(monkeypatch):
    """the train_clip_cifar chain end to end: 32 x 32 sets, 224 x 224 batches, the smallest CLIP of the trainer tests (2 layers,
    width 256, the g19 "small" text tower) with a 224 / 32 patch grid"""
    from eoe_amd import data
    from eoe_amd.models import CLIP
    from eoe_amd.training import TRAINER, ADTrainer
    monkeypatch.setattr(ADTrainer, "KEEP_SNAPSHOT_IN_RAM", True)
    torch.manual_seed(0)
    normal, oe, test, lab = _rgb_sets()
    src = data.ResidentImageSource(normal, oe, test, lab, crop=32, padding=4, flip_first=False, seed=1, color_jitter=(0.01,) * 4,
                                   clip_preprocessing=224)
    model = CLIP(64, 224, 2, 256, 32, 77, 1000, 128, 2, 2)
    tr = TRAINER["clip"](model, dataset=src, epochs=1, lr=1e-3, batch_size=8, tokenizer=_fake_tokenizer())
    models, res = tr.run(run_classes=[0])
    assert len(tr.last_losses) > 0 and np.isfinite(tr.last_losses).all()
    assert np.isfinite(res["mean_auc"]) and 0.0 <= res["mean_auc"] <= 1.0
    trained = models[0][0].cuda().eval()
    x = next(iter(src.loaders(8)[1]))[0]
    with torch.no_grad():
        scores = tr.compute_anomaly_score(trained(x), tr.center)
    assert scores.shape[0] == 8 and torch.isfinite(scores).all() and (scores >= 0).all() and (scores <= 1).all()
