"""Case tables, references, bounds and measured constants of the Grad-CAM tests (tests/test_cpu_gradcam.py, tests/test_gpu_gradcam.py):
the map kernels of csrc/gradcam.hip against the numpy statements of `eoe_amd.explain`, the data-only CBAM junction backward, and
`explain.grad_cam` on WideResNet + CBAM against autograd through the fp64 oracle."""
import functools

import numpy as np
import torch

from oracle import fill, models as omodels, objectives, trainer as otrainer

U = 2.0 ** -24                                 # the rounding unit of fp32

# ------------------------------------------------------------------------------------------------ the map kernels
CHANNELS = (4, 64, 512)
MAPS = ((1, 1), (2, 2), (3, 5), (7, 7))        # for every C; 56 x 56 at C = 64 on top (more than one workgroup per image in every kernel)
N_IMAGES = (1, 3)
MAP_CASES = [(n, h, w, C) for C in CHANNELS for (h, w) in MAPS for n in N_IMAGES] + [(n, 56, 56, 64) for n in N_IMAGES]
# (h, w) -> (H, W): an integer ratio (x 32), a non-integer one (7 -> 30), the identity, and the constant map of a 1 x 1 source
UPSAMPLE_CASES = (((7, 7), (224, 224)), ((7, 7), (30, 30)), ((3, 5), (3, 5)), ((1, 1), (32, 32)), ((2, 2), (64, 64)), ((3, 5), (10, 7)),
                  ((56, 56), (224, 224)))


def act_case(n, h, w, C, tag="a"):
    """(A, dA) fp32 NHWC, pure functions of the case's name; image 0 of a case with n > 1 has A > 0 and dA < 0, so that both maps of
    it are negative before relu everywhere, image 1 has both positive: no map of it is clipped"""
    name = f"gradcam/{tag}/{n}/{h}/{w}/{C}"
    A = fill.fill(name + "/A", (n, h, w, C), std=1.0).astype(np.float32)
    dA = fill.fill(name + "/dA", (n, h, w, C), std=0.5).astype(np.float32)
    if n > 1:
        A[0], dA[0] = np.abs(A[0]) + 0.125, -np.abs(dA[0]) - 0.125
        A[1], dA[1] = np.abs(A[1]) + 0.125, np.abs(dA[1]) + 0.125
    return A, dA


def cam_bound(A, dA, mode):
    """per entry of the map at the layer's resolution, against `explain.cam_np`.  A sum of k fp32 terms in any fixed order is within
    k 2^-24 sum |terms| of the exact one; every product adds one rounding.  'hirescam': C terms and their products, (C + 1) u sum_c |dA A|.
    'gradcam': alpha is a sum of hw terms and one division, and cam_np rounds its own alpha once more: |alpha - alpha_np| <= (hw + 2) u
    mean_p |dA|, which enters the map through sum_c |A_c|; then the C terms and their products."""
    a, d = np.abs(A.astype(np.float64)), np.abs(dA.astype(np.float64))
    n, h, w, C = a.shape
    if mode == "hirescam":
        return (C + 1) * U * (a * d).sum(axis=3)
    ealpha = (h * w + 2) * U * d.mean(axis=(1, 2))
    return np.einsum("nhwc,nc->nhw", a, ealpha) + (C + 1) * U * np.einsum("nhwc,nc->nhw", a, d.mean(axis=(1, 2)) + ealpha)


def upsample_bound(m, H, W):
    """per entry of the upsampled map, against `explain.bilinear_np` of the same fp32 map.  A weight is one division (l1, relative error
    u) or that and one subtraction (l0 = 1 - l1, absolute error 2 u at most); the product of a row and a column weight, both at most
    1, is then within 5 u absolutely, and the four corners carry it onto max |corner|: 20 u; the six products and three sums of the
    interpolation add one rounding each of a value of at most max |corner|: 9 u.  32 u max |corner| covers both; the maximum over the
    corners is taken by the same index arithmetic with the absolute values (the weights are non-negative, a maximum filter would do
    the same)."""
    from eoe_amd.explain import _bilinear_axis
    a = np.abs(np.asarray(m, dtype=np.float64))
    y0, y1, _ = _bilinear_axis(a.shape[1], H)
    x0, x1, _ = _bilinear_axis(a.shape[2], W)
    c = np.maximum(np.maximum(a[:, y0][:, :, x0], a[:, y0][:, :, x1]), np.maximum(a[:, y1][:, :, x0], a[:, y1][:, :, x1]))
    return 32 * U * c


# ------------------------------------------------------------------------------------------------ the CBAM junction
JUNCTION_CASES = ((2, 8, 8, 64), (1, 2, 2, 256), (3, 1, 1, 512))
JUNCTION_BIG = (1, 96, 96, 64)                 # (H + 6)(W + 6) = 10404 > 8192: beyond the weight-gradient kernel's cap
# the big case against fp64: the longest fp32 sums are the 9216-pixel ones of the channel gate (9216 x 2^-24 = 5.5e-4 in the worst case),
# under the project's parity ceiling
JUNCTION_BIG_TOL = 1e-3


def set_running_stats(model, tag="gradcam"):
    """non-trivial running statistics for every BatchNorm (mean != 0, var != 1), num_batches_tracked = 7; the oracle's and the package's
    modules carry the same buffer names"""
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.from_numpy(fill.fill(f"{tag}/{name}", tuple(buf.shape), std=0.05, mean=0.02)))
            elif name.endswith("running_var"):
                buf.copy_(torch.from_numpy(0.8 + np.abs(fill.fill(f"{tag}/{name}", tuple(buf.shape), std=0.3))))
            elif name.endswith("num_batches_tracked"):
                buf.fill_(7)
    return model


def oracle_cbam(C):
    m = omodels.deterministic_init(omodels._CBAM(C), tag=f"gradcam/cbam{C}")
    return set_running_stats(m, f"gradcam/cbam{C}").eval()


def junction_case(n, H, W, C):
    """x, res, dout fp32 NHWC of one case"""
    name = f"gradcam/junction/{n}/{H}/{W}/{C}"
    return tuple(torch.from_numpy(fill.fill(f"{name}/{k}", (n, H, W, C), std=1.0).astype(np.float32)) for k in ("x", "res", "dout"))


def junction_oracle(n, H, W, C):
    """out, dx, dres of relu(cbam(x) + res) in float64 through autograd, NHWC"""
    x, res, dout = (t.double().permute(0, 3, 1, 2).contiguous().requires_grad_() for t in junction_case(n, H, W, C))
    cb = oracle_cbam(C).double()
    out = torch.relu(cb(x) + res)
    dx, dres = torch.autograd.grad(out, (x, res), dout.detach())
    return tuple(t.detach().permute(0, 2, 3, 1).contiguous() for t in (out, dx, dres))


# ------------------------------------------------------------------------------------------------ the encoder
RESOLUTIONS = (32, 64)
LAYERS = ("layer1", "layer2", "layer3", "layer4")
MODES = ("gradcam", "hirescam")
N_MODEL = 3


@functools.lru_cache(maxsize=None)
def oracle_wrn(res):
    """oracle.models.WideResNet(res) with deterministic weights (SpatialGate BN weights around 1, not the initialisation's 0) and
    non-trivial running statistics, fp32 parameters (the state the package's model loads)"""
    m = omodels.deterministic_init(omodels.WideResNet(res=res), tag=f"gradcam/wrn{res}")
    return set_running_stats(m, f"gradcam/wrn{res}").eval()


def images_of(res):
    return otrainer.synthetic_batch(f"gradcam/x{res}", 1, 2, res)[0]


@functools.lru_cache(maxsize=None)
def oracle_maps(res, layer):
    """{mode: fp32 [3, res, res]} by a forward hook on `layer`, torch.autograd.grad of the summed hsc score and `grad_cam_np`, all in
    float64"""
    from eoe_amd.explain import grad_cam_np
    m = oracle_wrn(res).double()
    try:
        kept = {}
        h = getattr(m, layer).register_forward_hook(lambda mod, inp, out: kept.__setitem__("a", out))
        out = m(images_of(res).double())
        h.remove()
        (dA,) = torch.autograd.grad(objectives.hsc_score(out).sum(), kept["a"])
        A = kept["a"].detach().permute(0, 2, 3, 1).numpy()
        dA = dA.permute(0, 2, 3, 1).numpy()
        return {mode: grad_cam_np(A, dA, mode, res, res) for mode in MODES}
    finally:
        m.float()


def map_error(got, ref):
    """the worst image's largest error relative to that image's largest reference entry; an image whose reference map is all zero must
    be all zero"""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    worst = 0.0
    for i in range(r.shape[0]):
        top = r[i].max()
        err = np.abs(g[i] - r[i]).max()
        worst = max(worst, (0.0 if err == 0 else np.inf) if top == 0 else err / top)
    return worst


PARITY_CEILING = 1e-3                          # the project's parity bar

# ------------------------------------------------------------------------------------------------ measured
# `map_error` of grad_cam against the fp64 oracle, measured on an MI355X (tests/test_gpu_gradcam.py prints every figure before it
# asserts): (res, layer, mode) -> error.  Fast mode has no bar of its own in advance: a max-pool or channel-argmax winner that flips
# under 16-bit rounding moves a whole gradient path; each dtype is held to twice its worst measured case (the convention of
# explain_cnn_util).
MEASURED = {
    "parity": {
        (32, "layer1", "gradcam"): 1.150e-06, (32, "layer1", "hirescam"): 8.747e-07, (32, "layer2", "gradcam"): 9.687e-07, (32, "layer2", "hirescam"): 8.151e-07,
        (32, "layer3", "gradcam"): 9.922e-07, (32, "layer3", "hirescam"): 7.634e-07, (32, "layer4", "gradcam"): 7.673e-07, (32, "layer4", "hirescam"): 7.673e-07,
        (64, "layer1", "gradcam"): 5.812e-07, (64, "layer1", "hirescam"): 7.571e-07, (64, "layer2", "gradcam"): 5.897e-07, (64, "layer2", "hirescam"): 6.492e-07,
        (64, "layer3", "gradcam"): 5.733e-07, (64, "layer3", "hirescam"): 5.698e-07, (64, "layer4", "gradcam"): 5.484e-07, (64, "layer4", "hirescam"): 5.484e-07,
    },
    torch.float16: {
        (32, "layer1", "gradcam"): 1.084e-03, (32, "layer1", "hirescam"): 1.045e-03, (32, "layer2", "gradcam"): 1.184e-03, (32, "layer2", "hirescam"): 1.076e-03,
        (32, "layer3", "gradcam"): 1.160e-03, (32, "layer3", "hirescam"): 9.256e-04, (32, "layer4", "gradcam"): 8.851e-04, (32, "layer4", "hirescam"): 8.851e-04,
        (64, "layer1", "gradcam"): 1.433e-03, (64, "layer1", "hirescam"): 1.981e-03, (64, "layer2", "gradcam"): 1.111e-03, (64, "layer2", "hirescam"): 1.926e-03,
        (64, "layer3", "gradcam"): 1.041e-03, (64, "layer3", "hirescam"): 9.101e-04, (64, "layer4", "gradcam"): 1.027e-03, (64, "layer4", "hirescam"): 1.027e-03,
    },
    torch.bfloat16: {
        (32, "layer1", "gradcam"): 3.076e-02, (32, "layer1", "hirescam"): 1.346e-02, (32, "layer2", "gradcam"): 2.638e-02, (32, "layer2", "hirescam"): 1.135e-02,
        (32, "layer3", "gradcam"): 1.390e-02, (32, "layer3", "hirescam"): 1.156e-02, (32, "layer4", "gradcam"): 1.110e-02, (32, "layer4", "hirescam"): 1.110e-02,
        (64, "layer1", "gradcam"): 1.233e-02, (64, "layer1", "hirescam"): 1.048e-02, (64, "layer2", "gradcam"): 1.095e-02, (64, "layer2", "hirescam"): 1.042e-02,
        (64, "layer3", "gradcam"): 9.466e-03, (64, "layer3", "hirescam"): 1.021e-02, (64, "layer4", "gradcam"): 1.012e-02, (64, "layer4", "hirescam"): 1.012e-02,
    },
}
# parity mode: 5.5e-7 ... 1.2e-6, three orders under the 1e-3 ceiling.  fp16: 8.9e-4 ... 2.0e-3, bf16: 9.5e-3 ... 3.1e-2 -- two to
# eight units of the 16-bit rounding (2^-11, 2^-8) relative to a map's maximum; no case is dominated by a flipped max-pool or argmax
# winner (a flip moves a whole gradient path and would show as an error of the order of the map itself).  The bars, twice the worst
# case per dtype: fp16 3.962e-3 (res 64, layer1, hirescam), bf16 6.152e-2 (res 32, layer1, gradcam).

def bar(dtype):
    vals = MEASURED[dtype].values()
    return 2.0 * max(vals) if vals else None
