"""Case tables and measured constants of the explanation tests (tests/test_cpu_explain.py, tests/test_gpu_explain.py): the ViT input
gradient's last hop (eoe_unpatchify_grad), the saliency and overlay kernels (csrc/explain.hip) and the tower's input gradient against
autograd through the fp64 oracle."""
import numpy as np
import torch

from oracle import fill

GUARD = 256                                   # elements of NaN behind an output

# eoe_unpatchify_grad: (res, patch, n) -- one patch per image; the smallest patch; g = 7, odd; several blocks; the headline geometry
UNPATCHIFY_CASES = ((32, 32, 1), (8, 4, 3), (28, 4, 2), (48, 16, 3), (224, 32, 2))
UNPATCHIFY_STD = (0.25, 0.5, 2.0)             # none of them 1: a missing 1 / std[c] shows, a swapped channel too

# eoe_saliency_map: (n, C, H, W, pool)
SALIENCY_CASES = ((1, 1, 4, 4, None), (3, 3, 28, 28, 4), (2, 3, 224, 224, 32))
SALIENCY_RTOL = 1e-6                          # sums of <= 1024 non-negative fp32 terms in a fixed tree against one float64 rounding

# eoe_heat_overlay_u8: H x W
OVERLAY_SIZES = ((5, 7), (224, 224))
OVERLAY_ALPHAS = (0.0, 0.6, 1.0)
OVERLAY_MAX_DIFF_SHARE = 0.01                 # of all bytes may differ at all (by one grey level) between two evaluations

# the tower's input gradient: Normalize fused into the patch kernel, std != 1
NORM_MEAN, NORM_STD = (0.1, -0.2, 0.3), (0.5, 2.0, 0.25)

# Per-image relative rms distance of input_gradient to autograd through oracle.models.ClipViTNet in fp64, HSC score, n = 3, measured on
# an MI355X over vit_narrow_util.TOWERS x {cls_only off, on} x {no Normalize, Normalize} (fp16: x {gradient scale 1, 256}); the worst
# image of each case, in units of EPS16[dtype] (tests/test_gpu_explain.py prints every figure before it asserts).  cls_only on and off
# gave the same figures; fp16 at scale 1 and at 256 agreed to the digits shown.  (geometry, Normalize fused) -> EPS16 units.
INPUT_GRAD_MEASURED = {
    torch.bfloat16: {("ti_short", False): 4.82, ("ti_short", True): 3.48, ("s_long", False): 3.52, ("s_long", True): 5.21,
                     ("one_head", False): 6.91, ("one_head", True): 5.22, ("w320", False): 5.39, ("w320", True): 6.83},
    torch.float16: {("ti_short", False): 6.43, ("ti_short", True): 5.30, ("s_long", False): 3.78, ("s_long", True): 4.81,
                    ("one_head", False): 3.96, ("one_head", True): 3.32, ("w320", False): 3.87, ("w320", True): 5.22},
}
# the bar per dtype, in units of EPS16: twice the worst measured value (13.8 and 12.9), rounded up to one digit.  The ceiling a
# measurement may not exceed before it is a defect instead: twice test_gpu_vit_narrow's bar on parameter-gradient norms,
# 2 (30 EPS16 + 1e-3) = 60.5 EPS16 (bf16) and 64.1 EPS16 (fp16); every measured value is a ninth of it or less.
INPUT_GRAD_BAR = {torch.bfloat16: 20.0, torch.float16: 20.0}


def input_grad_ceiling(eps16: float) -> float:
    return 2.0 * (30.0 * eps16 + 1e-3)


def dpatches_case(res, patch, n):
    g = res // patch
    return fill.fill(f"explain/dpatches/{res}/{patch}/{n}", (n * g * g, 3 * patch * patch), std=1.0).astype(np.float32)


def fold_reference(dp: np.ndarray, res, patch, n) -> torch.Tensor:
    """torch.nn.functional.fold of the patch matrix: [n g^2, 3 p^2] -> [n, 3, res, res]"""
    g = res // patch
    cols = torch.from_numpy(dp).reshape(n, g * g, 3 * patch * patch).transpose(1, 2)
    return torch.nn.functional.fold(cols, (res, res), kernel_size=patch, stride=patch)


def saliency_case(n, C, H, W):
    g = fill.fill(f"explain/sal/g/{n}/{C}/{H}/{W}", (n, C, H, W), std=1.0).astype(np.float32)
    x = fill.fill(f"explain/sal/x/{n}/{C}/{H}/{W}", (n, C, H, W), std=1.0, mean=0.5).astype(np.float32)
    return g, x


def overlay_case(H, W, C, u8):
    """(maps [4, H, W], pictures): image 0 and 1 ordinary, image 2 a constant map, image 3 with a NaN and an inf entry.  The values are
    multiples of 1 / 64 (maps) and of 1 / 255 resp. whole bytes (pictures), drawn from a fixed generator; test_cpu_explain.py checks that
    they keep floor(v + 0.5) away from ties."""
    rng = np.random.RandomState(1234 + H * 7 + W * 3 + C + (10 if u8 else 0))
    maps = (rng.randint(0, 641, size=(4, H, W)) / 64.0).astype(np.float32)
    # a known minimum and maximum, 641 / 64 apart: t = k / 641 with 641 prime, so with alpha = 3 / 5 or 1 and whole bytes the blended
    # value is a fraction with an odd denominator -- never a half-integer -- and t = 0 and t = 1 both occur
    maps[:, 0, 0], maps[:, -1, -1] = 0.0, 10.015625
    maps[2] = 3.5
    maps[3, 0, 1], maps[3, 1, 0] = np.nan, np.inf
    bytes_ = rng.randint(0, 256, size=(4, H, W, C)).astype(np.uint8)
    if u8:
        return maps, bytes_
    return maps, np.ascontiguousarray((bytes_.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def heat_levels(maps: np.ndarray) -> np.ndarray:
    """t of every entry in float64, by the rule of eoe_heat_overlay_u8"""
    t = np.zeros(maps.shape, dtype=np.float64)
    for i, m in enumerate(maps):
        fin = np.isfinite(m)
        if fin.any():
            lo, hi = float(m[fin].min()), float(m[fin].max())
            if hi > lo:
                t[i][fin] = (m[fin].astype(np.float64) - lo) / (hi - lo)
    return t
