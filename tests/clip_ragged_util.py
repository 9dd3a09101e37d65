"""Inputs and host-side references of the ragged CLIP-preprocessing tests: CLIP's own transform on RAW images of mixed sizes
(`clip_official/clip/clip.py:58-65`: Resize(n_px, BICUBIC) with the aspect ratio kept, CenterCrop(n_px)), as the test split of the
reference's `main/train_clip_imagenet.py`, `train_clip_cub.py`, `train_clip_dtd.py`, `train_clip_mvtec.py` gets it, at n_px = 8.

The reference for bytes is Pillow itself: `Image.resize((w', h'), BICUBIC)` at torchvision's size rule, then the crop at torchvision's
CenterCrop origin.  The images come from ragged_util's integer formula."""
import numpy as np

import ragged_util as ru

N_PX = 8
# (H, W): what each exercises
SHAPES = [(8, 8),        # identity, no window
          (8, 13),       # identity resize, horizontal window at 2
          (13, 8),       # identity resize, vertical window
          (9, 9),        # downsample, no window
          (5, 11),       # upsample to 8 x 17, window at 4
          (11, 5),       # upsample, vertical window
          (20, 31),      # wide taps
          (31, 20),
          (3, 40),       # extreme aspect
          (40, 3),
          (1, 3)]        # one-pixel short side
BIG_N_PX, BIG_SHAPES = 224, [(375, 500), (500, 333)]


def images(shapes=SHAPES, salt=0):
    return [ru.image(i + salt, H, W, 3) for i, (H, W) in enumerate(shapes)]


def resized_hw(H, W, size):
    """torchvision's `_compute_resized_output_size` for an int, restated here on its own"""
    short, long = (W, H) if W <= H else (H, W)
    if short == size:
        return H, W
    new_long = int(size * long / short)
    return (new_long, size) if W <= H else (size, new_long)


def origin(s, n_px):
    """torchvision's CenterCrop origin on a side of s >= n_px: Python's round, halves to even"""
    return int(round((s - n_px) / 2.0))


def pillow_full(img, n_px):
    """Resize(n_px, BICUBIC) of one uint8 HWC image, by Pillow"""
    from PIL import Image
    h, w = resized_hw(img.shape[0], img.shape[1], n_px)
    return np.asarray(Image.fromarray(img).resize((w, h), Image.BICUBIC))


def pillow_clip(img, n_px):
    """uint8 [n_px, n_px, 3]: CLIP's PIL stage of one raw image, by Pillow"""
    full = pillow_full(img, n_px)
    t, l = origin(full.shape[0], n_px), origin(full.shape[1], n_px)
    return np.ascontiguousarray(full[t:t + n_px, l:l + n_px])


def packed_set(imgs, device=None):
    """a RaggedImageSet whose images lie back to back WITHOUT the alignment gaps: the first image starts the arena, the last one ends
    it, and the starts in between are whatever the byte counts make them (odd for most)"""
    import torch
    from eoe_amd import data
    nbytes = np.array([a.size for a in imgs], dtype=np.int64)
    offsets = np.cumsum(nbytes) - nbytes
    arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs]))
    sizes = np.array([a.shape[:2] for a in imgs], dtype=np.int32)
    rs = data.RaggedImageSet.from_parts(arena, offsets, sizes, 3)
    return rs if device is None else rs.to(device)


def normalized(u8, mean, std):
    """ToTensor -> Normalize on uint8 [n, P, P, 3] -> fp32 NCHW, the two fp32 operations of clip_pre_util.oracle_f32"""
    out = (u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    out = (out - np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)) / np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
    return np.ascontiguousarray(out.astype(np.float32))


def emulate_pass(src, dst, offs, desc, taps, src_written=None, dst_written=None):
    """`eoe_ragged_resize_pass_u8` with its window field in numpy, element by element as the kernel addresses them: the source offset
    is signed and only the sum (offset + position) has to lie in the source.  Every index is checked against the array it goes into;
    with `src_written` (bool, one per source byte) every byte READ must have been written by the pass in front, and `dst_written`
    records what this pass writes -- a horizontal pass that leaves out a row the vertical window needs fails here, on the host."""
    for (so, do), (outer, a_in, a_out, inner, b_at, k_at, ks, first) in zip(offs.tolist(), desc.tolist()):
        assert outer >= 1 and a_out >= 1 and inner >= 1 and first >= 0
        assert 0 <= do and do + outer * a_out * inner <= len(dst), "result outside its arena"
        o = dst[do:do + outer * a_out * inner].reshape(outer, a_out, inner)
        if dst_written is not None:
            assert not dst_written[do:do + outer * a_out * inner].any(), "two images write the same bytes"
            dst_written[do:do + outer * a_out * inner] = True

        def read(r, x):
            at = so + (r * a_in + x) * inner
            assert 0 <= at and at + inner <= len(src), "a read outside the source arena"
            assert src_written is None or src_written[at:at + inner].all(), "a read of bytes the pass in front never wrote"
            return src[at:at + inner].astype(np.int64)

        if ks == 0:
            assert first + a_out <= a_in, "a copied window outside the axis"
            for r in range(outer):
                for x in range(a_out):
                    o[r, x] = read(r, first + x)
            continue
        assert 0 <= b_at and 0 <= k_at and b_at + 2 * (first + a_out) <= len(taps) and k_at + (first + a_out) * ks <= len(taps), \
            "tables outside the tap array"
        for x in range(a_out):
            xx = first + x
            xmin, cnt = int(taps[b_at + 2 * xx]), int(taps[b_at + 2 * xx + 1])
            assert 0 <= xmin and 0 < cnt <= ks and xmin + cnt <= a_in, "taps reach outside the axis"
            k = taps[k_at + xx * ks:k_at + xx * ks + cnt].astype(np.int64)
            for r in range(outer):
                acc = sum(read(r, xmin + j) * k[j] for j in range(cnt)) + (1 << 21)
                o[r, x] = np.clip(acc >> 22, 0, 255)


def run_plan_on_host(rs, plan, taps):
    """both passes of a plan over the set's arena (numpy) -> the flat result; the intermediate's written bytes are tracked"""
    tap = taps.tensor().numpy()
    arena = rs.arena.numpy()
    out = np.full(plan["out_bytes"], 0xA5, np.uint8)
    out_w = np.zeros(plan["out_bytes"], bool)
    if plan["h"] is not None and plan["v"] is not None:
        mid, mid_w = np.full(plan["mid_bytes"], 0x5A, np.uint8), np.zeros(plan["mid_bytes"], bool)
        emulate_pass(arena, mid, plan["h"][0], plan["h"][1], tap, None, mid_w)
        emulate_pass(mid, out, plan["v"][0], plan["v"][1], tap, mid_w, out_w)
    else:
        name = "h" if plan["h"] is not None else "v"
        emulate_pass(arena, out, plan[name][0], plan[name][1], tap, None, out_w)
    assert out_w.all(), "a byte of the packed result is never written"
    return out
