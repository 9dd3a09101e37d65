"""Inputs and host-side references of the ragged candidate-search tests (`eoe_pool_sqdist_ragged_u8`, `OEPool(rs, crop=...)`): image
sets of mixed sizes from `oracle.fill`, their crop windows built EXPLICITLY in numpy (zero canvas, the overlap copied in), exact
int64 distances over them, and the composed device path the kernel replaces (`crop_flip_u8` of the windows into a tensor, then the
uniform `eoe_pool_sqdist_u8` + `eoe_pool_rank`)."""
import ctypes

import numpy as np

from oracle.fill import fill_int


def mixed_images(name: str, shapes, C: int, lo: int = 0, hi: int = 256):
    """uint8 [H, W, C] per shape, pure functions of the name"""
    return [fill_int(f"{name}/{i}", (H, W, C), lo, hi).astype(np.uint8) for i, (H, W) in enumerate(shapes)]


def window(img: np.ndarray, top: int, left: int, ch: int, cw: int) -> np.ndarray:
    """uint8 [ch, cw, C]: the window of `img` whose origin is (top, left) relative to the unpadded image; outside the image: 0"""
    H, W, C = img.shape
    out = np.zeros((ch, cw, C), dtype=np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(top + ch, H), max(left, 0), min(left + cw, W)
    if y0 < y1 and x0 < x1:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = img[y0:y1, x0:x1]
    return out


def center_origin(extent: int, crop: int) -> int:
    """torchvision's CenterCrop on one axis: int(round((extent - crop) / 2.0)) (Python's round), and for a short axis the origin that its
    symmetric padding of (crop - extent) // 2 in front implies"""
    return int(round((extent - crop) / 2.0)) if extent >= crop else -((crop - extent) // 2)


def center_windows(imgs, ch: int, cw: int) -> np.ndarray:
    """uint8 [n, ch, cw, C]: CenterCrop((ch, cw)) of every image, zero-padded"""
    return np.stack([window(im, center_origin(im.shape[0], ch), center_origin(im.shape[1], cw), ch, cw) for im in imgs])


def listed_windows(imgs, desc, ch: int, cw: int) -> np.ndarray:
    """uint8 [len(desc), ch, cw, C] of a list of (row, top, left)"""
    return np.stack([window(imgs[int(r)], int(t), int(l), ch, cw) for r, t, l in desc])


def np_dist(wq: np.ndarray, wc: np.ndarray) -> np.ndarray:
    """int64 [K, P]: exact squared distances of windows [K, ...] to windows [P, ...]"""
    q, c = wq.reshape(len(wq), -1).astype(np.int64), wc.reshape(len(wc), -1).astype(np.int64)
    return np.stack([((c - row) ** 2).sum(axis=1) for row in q])


def np_dist_rows(wins: np.ndarray, q, c) -> np.ndarray:
    """np_dist of windows wins[q] to wins[c], computed once per distinct candidate row (a list may repeat one row 1 023 times)"""
    uc, inv = np.unique(np.asarray(c), return_inverse=True)
    return np_dist(wins[np.asarray(q)], wins[uc])[:, inv.reshape(-1)]


def stable_order(dist: np.ndarray) -> np.ndarray:
    return np.argsort(dist, axis=1, kind="stable").astype(np.int32)


# --------------------------------------------------------------------------------------------------------------- operators
# windows of 32 x 32 x 3: random bytes sit near 3 072 * 10 922 = 33.5 M, far beyond the self-exclusion threshold of 6 502 500, so only
# an individual's own image is excluded and `_pick` always finds its candidates
OP_SHAPES = [(32 + (5 * i) % 17, 32 + (7 * i + 3) % 17) for i in range(30)]
OP_CASES = {"mutate3": ("mutate", [[3, 11, 20]], 0.9), "mutate1": ("mutate", [[7]], 1.0), "mate1": ("mate", [[3], [25]], 1.0),
            "mate3": ("mate", [[3, 11, 20], [5, 17, 29]], 0.5)}


def run_operator(pool, name, seed=5, poolsize=20, oneofkbest=3):
    from eoe_amd.evolve import mate_individuals, mutate_individual
    kind, inds, indp = OP_CASES[name]
    inds = [list(i) for i in inds]
    np.random.seed(seed)
    if kind == "mutate":
        mutate_individual(inds[0], pool, poolsize, indp, oneofkbest)
    else:
        mate_individuals(inds[0], inds[1], pool, poolsize, indp, oneofkbest)
    return inds


def op_images():
    return mixed_images("ragged_evolve/ops", OP_SHAPES, 3)


# ------------------------------------------------------------------------------------------------------------- device side
def sqdist_ragged(rs, ch: int, cw: int, query, cand, out=None, n_set=None):
    """`eoe_pool_sqdist_ragged_u8` called directly on a cuda RaggedImageSet with (row, top, left) lists: (return code, int64 [K, P]
    on the host, or None after an error).  `out`: a pre-filled device tensor to write into"""
    import torch
    from eoe_amd._lib import lib
    query, cand = np.ascontiguousarray(query, dtype=np.int32).reshape(-1, 3), np.ascontiguousarray(cand, dtype=np.int32).reshape(-1, 3)
    K, P = len(query), len(cand)
    need = ctypes.c_size_t(0)
    assert lib.eoe_pool_sqdist_ragged_workspace(ch, cw, rs.channels, K, P, ctypes.byref(need)) == 0
    ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device="cuda")
    if out is None:
        out = torch.empty((K, P), dtype=torch.int64, device="cuda")
    rc = lib.eoe_pool_sqdist_ragged_u8(rs.arena.data_ptr(), rs.arena.numel(), rs.offsets.data_ptr(), rs.sizes_dev.data_ptr(),
                                       len(rs) if n_set is None else n_set, rs.channels, ch, cw, query.ctypes.data, K, cand.ctypes.data, P,
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                      # the host lists stay alive until the stream has passed the call
    return rc, (out.cpu().numpy().reshape(K, P) if rc == 0 else None)


def composed(rs, ch: int, cw: int, query, cand):
    """the path the kernel replaces: `crop_flip_u8` of the K + P windows into a tensor, then the uniform pool's kernels.  Returns
    (int64 [K, P], int32 [K, P], the window tensor on the device)"""
    import torch
    from eoe_amd.data import crop_flip_u8
    from eoe_amd.evolve import OEPool
    desc = np.concatenate([np.asarray(query, np.int32).reshape(-1, 3), np.asarray(cand, np.int32).reshape(-1, 3)])
    params = torch.from_numpy(np.concatenate([desc, np.zeros((len(desc), 1), np.int32)], axis=1)).cuda()
    wins = crop_flip_u8(rs, params, (ch, cw), True)
    K = len(np.asarray(query).reshape(-1, 3))
    dist, order = OEPool(wins).distances(list(range(K)), list(range(K, len(desc))))
    return dist, order, wins


def check_windows(rs, imgs, ch: int, cw: int, query, cand):
    """the three assertions of every distance case on explicit (row, top, left) lists: numpy int64, the composed path bit for bit,
    and the same bits from a second call.  Returns the distances"""
    want = np_dist(listed_windows(imgs, query, ch, cw), listed_windows(imgs, cand, ch, cw))
    rc, got = sqdist_ragged(rs, ch, cw, query, cand)
    assert rc == 0 and got.dtype == np.int64 and np.array_equal(got, want)
    assert got.tobytes() == composed(rs, ch, cw, query, cand)[0].tobytes()
    assert got.tobytes() == sqdist_ragged(rs, ch, cw, query, cand)[1].tobytes()
    return got


def check_pool(rs, imgs, crop, q, c):
    """the same three assertions through `OEPool(rs, crop=crop).distances` (centre windows), and the order: (distances, order)"""
    from eoe_amd.data import center_origins
    from eoe_amd.evolve import OEPool
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    pool = OEPool(rs, crop=crop)
    dist, order = pool.distances(q, c)
    wins = center_windows(imgs, ch, cw)
    want = np_dist_rows(wins, q, c)
    assert dist.dtype == np.int64 and order.dtype == np.int32 and dist.shape == order.shape == (len(q), len(c))
    assert np.array_equal(dist, want) and np.array_equal(order, stable_order(want))
    org = np.stack([center_origins(rs.sizes[:, 0], ch), center_origins(rs.sizes[:, 1], cw)], axis=1)
    desc = lambda rows: np.concatenate([np.asarray(rows).reshape(-1, 1), org[rows]], axis=1)      # noqa: E731
    cd, co, _ = composed(rs, ch, cw, desc(q), desc(c))
    assert dist.tobytes() == cd.tobytes() and order.tobytes() == co.tobytes()
    again = pool.distances(q, c)
    assert dist.tobytes() == again[0].tobytes() and order.tobytes() == again[1].tobytes()
    return dist, order
