"""Inputs of the evolve fixture (tests/golden/g21_evolve.npz), shared by its maker and the tests: pure functions of a name
(oracle.fill), so the fixture holds only seeds and results."""
import numpy as np

from oracle.fill import fill_int

POOL_N, POOL_HW = 60, 32
PARENT, NEAR_DUP = 3, 7                  # image 7 is image 3 with 64 bytes changed by 16: squared distance 64 * (16 / 255)^2 = 0.25
POOLSIZE, ONEOFKBEST = 100, 3            # the reference's defaults (--ev-mutation-pool, --ev-mutation-oneofkbest)
# operator cases: name -> (kind, individuals, indp)
CASES = {
    "mutate1": ("mutate", [[PARENT]], 0.9),
    "mutate4": ("mutate", [[PARENT, 11, 20, 42]], 0.5),
    "mate1": ("mate", [[PARENT], [25]], 0.9),
    "mate4": ("mate", [[PARENT, 11, 20, 42], [5, 17, 33, 58]], 0.5),
}
SELECT_FITS = [0.61, 0.55, 0.79, 0.50, 0.72, 0.66, 0.58, 0.70]      # 8 individuals [i], tournament size 3
SELECT_TOURNSIZE = 3


def pool_u8() -> np.ndarray:
    """60 uint8 images of 32 x 32 x 3: a brightness level per image plus noise of +-48, so that the pairwise distances spread
    from about 75 (equal levels: below the reference's self-exclusion threshold of 100) to 3 000 in the [0, 1] scale; 32 x 32 x 3
    is the smallest image size at which that threshold can be met at all (at 8 x 8 x 3 the largest possible distance is 192)"""
    level = fill_int("evolve/level", (POOL_N, 1, 1, 1), 0, 256)
    noise = fill_int("evolve/noise", (POOL_N, POOL_HW, POOL_HW, 3), -48, 49)
    imgs = np.clip(level + noise, 0, 255).astype(np.uint8)
    dup = imgs[PARENT].copy().reshape(-1)
    dup[:64] = np.where(dup[:64] >= 128, dup[:64] - 16, dup[:64] + 16)
    imgs[NEAR_DUP] = dup.reshape(imgs[PARENT].shape)
    return imgs
