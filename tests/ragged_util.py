"""Inputs and host-side references of the ragged-set tests (fixture g25_ragged, made by tests/golden/make_golden_ragged.py with Pillow
alone): image sets of mixed sizes through Resize(int) / Resize((h, w)) / CenterCrop / ColorJitter + crop, the chains of the reference's
`main/train_imagenet.py:30-41`, `train_cub.py`, `train_dtd.py`, `train_mvtec.py` and `train_custom.py` at a target of 16 instead of 256.

The images come from an integer formula, not from an RNG, so the fixture script reproduces them anywhere; the fixture holds only
Pillow's results."""
import numpy as np

TARGET = 16                  # Resize(TARGET), CenterCrop(TARGET), RandomCrop(TARGET)
# (H, W) -> what Resize(16) makes of it; the smallest shapes that reach every branch of the rule and of the kernels
SHAPES = [(37, 53), (53, 37), (40, 40), (16, 16), (17, 16), (16, 97), (20, 97), (9, 13), (64, 23)]
RESIZED = [(16, 22), (22, 16), (16, 16), (16, 16), (17, 16), (16, 97), (16, 77), (16, 23), (44, 16)]
FILTERS = ("bilinear", "bicubic")
CODED = 5                    # image 5 (16 x 97, which Resize(16) leaves alone) carries (marker, row, col) in its three channels
CODED_MARKER = 201

# ColorJitter cases: (image, order, factors (b, c, s, h), (top, left) of the 16 x 16 crop, flip) on the bilinear-resized 3-channel set;
# contrast (op 1) first, in the middle and last; the second origin reaches into the zero padding on the top and left, the third on the
# bottom and right
JITTER = [(0, (1, 0, 2, 3), (0.93, 1.21, 0.85, 0.031), (0, 4), 0),
          (6, (2, 1, 3, 0), (1.08, 0.77, 1.3, -0.045), (-2, -3), 1),
          (8, (3, 0, 2, 1), (0.7, 1.6, 0.4, 0.31), (30, 2), 0)]


def image(i: int, H: int, W: int, C: int) -> np.ndarray:
    """uint8 [H, W, C]: image i of the set, a smooth ramp with a texture on it so that neither filter is trivial"""
    r, c, ch = np.arange(H).reshape(H, 1, 1), np.arange(W).reshape(1, W, 1), np.arange(C).reshape(1, 1, C)
    if i == CODED and C == 3:
        return np.concatenate([np.full((H, W, 1), CODED_MARKER), np.broadcast_to(r, (H, W, 1)), np.broadcast_to(c, (H, W, 1))],
                              axis=2).astype(np.uint8)
    v = 31 * i + 5 * r + 3 * c + 41 * ch + 17 * ((r * c + i) % 7) + 9 * ((r + 2 * c) % 5) + 64 * ((r // 4 + c // 5 + ch) % 2)
    return (v % 256).astype(np.uint8)


def images(C: int):
    return [image(i, H, W, C) for i, (H, W) in enumerate(SHAPES)]


def oe_images(C: int):
    """a second set of the same shapes in another order (the OE half of the source tests)"""
    order = [4, 7, 1, 8, 0, 6, 2, 3]
    return [image(i + 11, *SHAPES[i], C) for i in order]


def center_crop(img: np.ndarray, crop: int) -> np.ndarray:
    """torchvision's CenterCrop on an image at least `crop` on both sides"""
    H, W = img.shape[:2]
    top, left = int(round((H - crop) / 2.0)), int(round((W - crop) / 2.0))
    return img[top:top + crop, left:left + crop]


def crop_flip(img: np.ndarray, top: int, left: int, flip: int, S: int, flip_first: bool = True) -> np.ndarray:
    """RandomCrop with zero padding (origin relative to the unpadded image) and the flip in either order, uint8 [S, S, C]"""
    H, W, C = img.shape
    if flip and flip_first:
        img = img[:, ::-1]
    out = np.zeros((S, S, C), dtype=np.uint8)
    ys, xs = np.arange(S) + top, np.arange(S) + left
    vy, vx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    out[np.ix_(vy, vx)] = img[np.ix_(ys[vy], xs[vx])]
    return out[:, ::-1] if flip and not flip_first else out


def corner_params(sizes, S: int, pad: int) -> np.ndarray:
    """int32 [5 n, 4]: for every image the four corner origins of its padded range and one interior origin; flips alternate"""
    rows = []
    for i, (H, W) in enumerate(sizes):
        lo_t, hi_t, lo_l, hi_l = -pad, H + pad - S, -pad, W + pad - S
        for j, (t, l) in enumerate([(lo_t, lo_l), (lo_t, hi_l), (hi_t, lo_l), (hi_t, hi_l), ((lo_t + hi_t) // 2, (lo_l + hi_l + 1) // 2)]):
            rows.append((i, t, l, (i + j) % 2))
    return np.array(rows, dtype=np.int32)


def emulate_pass(src: np.ndarray, dst: np.ndarray, offs: np.ndarray, desc: np.ndarray, taps: np.ndarray):
    """`eoe_ragged_resize_pass_u8` in numpy, with every index checked against the array it goes into (a wrong table fails here, on
    the host, and never reads outside an arena on the device)"""
    for (so, do), (outer, a_in, a_out, inner, b_at, k_at, ks, _) in zip(offs.tolist(), desc.tolist()):
        assert 0 <= so and so + outer * a_in * inner <= len(src), "source image outside its arena"
        assert 0 <= do and do + outer * a_out * inner <= len(dst), "result outside its arena"
        s = src[so:so + outer * a_in * inner].reshape(outer, a_in, inner).astype(np.int64)
        o = dst[do:do + outer * a_out * inner].reshape(outer, a_out, inner)
        if a_in == a_out:
            o[...] = s
            continue
        assert 0 <= b_at and b_at + 2 * a_out <= len(taps) and 0 <= k_at and k_at + a_out * ks <= len(taps), "tables outside the tap array"
        bounds, kk = taps[b_at:b_at + 2 * a_out].reshape(a_out, 2), taps[k_at:k_at + a_out * ks].reshape(a_out, ks)
        for xx in range(a_out):
            xmin, cnt = int(bounds[xx, 0]), int(bounds[xx, 1])
            assert 0 <= xmin and 0 < cnt <= ks and xmin + cnt <= a_in, "taps reach outside the axis"
            acc = (s[:, xmin:xmin + cnt, :] * kk[xx, :cnt].astype(np.int64).reshape(1, cnt, 1)).sum(axis=1) + (1 << 21)
            o[:, xx, :] = np.clip(acc >> 22, 0, 255)
