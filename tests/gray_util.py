"""Inputs of the 1-channel input-path tests (fixture g22_gray, made by tests/golden/make_golden_gray.py with Pillow).

Inputs are pure functions of a name (oracle.fill), so the fixture holds only results and the GPU box regenerates the same bits."""
import numpy as np

from oracle import fill as ofill

N_IMG = 24
L_WEIGHTS = (19595, 38470, 7471)                 # Pillow's rgb2l (libImaging/Convert.c): (sum + 0x8000) >> 16
BOUNDARY_KS = tuple(range(4, 256, 8))            # image 1 holds sums k * 65536 - 0x8000 + d, d in (-1, 0, 1), for these k
PRIMARIES = ((255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255))


def gray_formula(rgb: np.ndarray) -> np.ndarray:
    """the integer formula on uint8 [..., 3] -> uint8 [...]"""
    v = rgb.astype(np.int64)
    return ((v[..., 0] * L_WEIGHTS[0] + v[..., 1] * L_WEIGHTS[1] + v[..., 2] * L_WEIGHTS[2] + 0x8000) >> 16).astype(np.uint8)


def boundary_pixels() -> np.ndarray:
    """(r, g, b) triples whose weighted sum is exactly k * 65536 - 0x8000 + d: at d = -1 the byte is k - 1, at d = 0 and 1 it is k --
    the places where a rounding that is not Pillow's shows.  The first solution in (r, g) order per target."""
    r, g = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    part = r * L_WEIGHTS[0] + g * L_WEIGHTS[1]
    out = []
    for k in BOUNDARY_KS:
        for d in (-1, 0, 1):
            rest = k * 65536 - 0x8000 + d - part
            ok = (rest >= 0) & (rest % L_WEIGHTS[2] == 0) & (rest // L_WEIGHTS[2] <= 255)
            hit = np.argwhere(ok)
            if len(hit):
                ri, gi = (int(v) for v in hit[0])
                out.append((ri, gi, int(rest[ri, gi] // L_WEIGHTS[2])))
    return np.asarray(out, dtype=np.uint8).reshape(-1, 3)


def colour_set() -> np.ndarray:
    """24 colour images uint8 [24, 32, 32, 3]: image 0 starts with the primaries, image 1 with the rounding boundaries"""
    x = ofill.fill_int("g22/colour", (N_IMG, 32, 32, 3), 0, 256).astype(np.uint8)
    x[0].reshape(-1, 3)[:len(PRIMARIES)] = np.asarray(PRIMARIES, dtype=np.uint8)
    bp = boundary_pixels()
    x[1].reshape(-1, 3)[:len(bp)] = bp
    return x


def gray_set() -> np.ndarray:
    """24 gray images uint8 [24, 28, 28]"""
    return ofill.fill_int("g22/gray", (N_IMG, 28, 28), 0, 256).astype(np.uint8)


def tiny_set() -> np.ndarray:
    """4 gray images of 6 x 5 (a width that is no multiple of 4)"""
    return ofill.fill_int("g22/tiny", (4, 6, 5), 0, 256).astype(np.uint8)


# name -> (source set, (Ho, Wo), padding): the FMNIST chain on its own 28 x 28 images and on the 32 x 32 OE images, a tiny case,
# and an output width (7) that is no multiple of the 4 pixels a thread takes
CROP_CASES = {"g28": ("gray", (28, 28), 3), "c32": ("colour", (28, 28), 3), "tiny": ("tiny", (4, 4), 1), "odd7": ("gray", (5, 7), 2)}


def case_source(name: str, colour_l=None) -> np.ndarray:
    """uint8 [n, H, W] source of a crop case; the colour set enters as its L image (`colour_l`: the fixture's, else the formula)"""
    kind = CROP_CASES[name][0]
    if kind == "gray":
        return gray_set()
    if kind == "tiny":
        return tiny_set()
    return colour_l if colour_l is not None else gray_formula(colour_set())


def case_rows(name: str) -> np.ndarray:
    """int32 [13, 4] = (index, top, left, flip): top and left each at -padding, 0 and the maximum -- every padded border and every
    corner -- with mixed flips, then the four corners again with the other flip"""
    kind, (Ho, Wo), pad = CROP_CASES[name]
    n, Hs, Ws = case_source(name).shape
    tops, lefts = (-pad, 0, Hs + pad - Ho), (-pad, 0, Ws + pad - Wo)
    flips = (0, 1, 1, 1, 0, 0, 0, 1, 1)
    rows = [(t, l, f) for (t, l), f in zip([(t, l) for t in tops for l in lefts], flips)]
    rows += [(tops[0], lefts[0], 1), (tops[0], lefts[2], 0), (tops[2], lefts[0], 1), (tops[2], lefts[2], 0)]
    r = np.asarray([(0,) + row for row in rows], dtype=np.int32)
    r[:, 0] = (np.arange(len(rows)) * 5 + 1) % n
    return r
