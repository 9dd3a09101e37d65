"""Case tables, references and measured constants of the CNN explanation tests (tests/test_cpu_explain_cnn.py,
tests/test_gpu_explain_cnn.py): the first-layer data gradient back to the image (eoe_conv_image_dgrad, csrc/explain.hip), the eval-mode
BatchNorm backward, and `explain.input_gradient` on CNN32 / CNN28 against autograd through the fp64 oracle."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill, models as omodels, objectives, trainer as otrainer

import explain_util as xu

GUARD = xu.GUARD

# eoe_conv_image_dgrad: (cin, cout, k, stride, pad, Hi).  CNN32's conv1, CNN28's conv1, the WideResNet stem on an even and an odd map,
# a map whose last row and column no tap reaches (Ho = 2: rows 0 .. 4 of 6), an image smaller than the kernel
DGRAD_CASES = ((3, 32, 5, 1, 2, 32), (1, 16, 5, 1, 2, 28), (3, 64, 7, 2, 3, 30), (3, 64, 7, 2, 3, 29), (3, 4, 3, 2, 0, 6), (1, 8, 5, 1, 2, 3))
DGRAD_N = (1, 3)
DGRAD_STD = (0.5, 2.0, 0.25)                  # none of them 1 (explain_util.NORM_STD)
DGRAD_SCALE_INV = (1.0, 1.0 / 256.0)


def out_size(Hi, k, stride, pad):
    return (Hi + 2 * pad - k) // stride + 1


def dgrad_case(cin, cout, k, stride, pad, Hi, n):
    """(dy fp32 [n Ho Wo, cout], w fp32 [cout, cin, k, k]) of one case, pure functions of its name"""
    Ho = out_size(Hi, k, stride, pad)
    tag = f"explain_cnn/dgrad/{cin}/{cout}/{k}/{stride}/{pad}/{Hi}/{n}"
    dy = fill.fill(tag + "/dy", (n * Ho * Ho, cout), std=1.0).astype(np.float32)
    w = fill.fill(tag + "/w", (cout, cin, k, k), std=(cin * k * k) ** -0.5).astype(np.float32)
    return dy, w


def dgrad_autograd(dy, w, n, Hi, stride, pad, std=None, scale_inv=1.0):
    """the same gradient by torch.autograd.grad through F.conv2d in float64 (the Normalize (x - 0) / std in front, the seed scaled)"""
    cout, cin, k, _ = w.shape
    Ho = out_size(Hi, k, stride, pad)
    x = torch.zeros((n, cin, Hi, Hi), dtype=torch.float64, requires_grad=True)
    inp = x if std is None else x / torch.tensor(std, dtype=torch.float64).view(1, cin, 1, 1)
    y = F.conv2d(inp, torch.from_numpy(w).double(), None, stride=stride, padding=pad)
    seed = torch.from_numpy(dy).double().reshape(n, Ho, Ho, cout).permute(0, 3, 1, 2) * scale_inv
    (g,) = torch.autograd.grad(y, x, seed)
    return g.numpy()


def dgrad_bound(dy, w, n, Hi, stride, pad, std, scale_inv):
    """per element: (k k cout + 4) 2^-24 (scale_inv / std[c]) sum |dy w| -- the worst case of an fp32 sum of that many terms plus the
    final scaling (1 / std, scale_inv / std and the product: three roundings)"""
    from eoe_amd.explain import conv_image_dgrad_np
    cout, cin, k, _ = w.shape
    mag = conv_image_dgrad_np(np.abs(dy.astype(np.float64)), np.abs(w.astype(np.float64)), n, Hi, Hi, stride, pad, std, scale_inv)
    return (k * k * cout + 4) * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------------ the encoders
MODELS = ("CNN32", "CNN28")
IMAGE = {"CNN32": (3, 32), "CNN28": (1, 28)}
N_IMAGES = 3


def normalize_of(name, norm):
    """(mean, std) of the fused Normalize: explain_util's; one channel of it for CNN28"""
    if not norm:
        return None, None
    c = IMAGE[name][0]
    return tuple(xu.NORM_MEAN[:c]), tuple(xu.NORM_STD[:c])


def set_running_stats(model):
    """non-trivial running statistics (mean != 0, var != 1) for every BatchNorm of a CNN32 / CNN28 -- oracle's or the package's, the
    buffers carry the same names; num_batches_tracked = 7"""
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.copy_(torch.from_numpy(fill.fill(f"explain_cnn/{name}", tuple(buf.shape), std=0.3, mean=0.1)))
            elif name.endswith("running_var"):
                buf.copy_(torch.from_numpy(0.6 + np.abs(fill.fill(f"explain_cnn/{name}", tuple(buf.shape), std=0.8))))
            elif name.endswith("num_batches_tracked"):
                buf.fill_(7)
    return model


def images_of(name):
    ch, res = IMAGE[name]
    x = otrainer.synthetic_batch(f"explain_cnn/{name}", 1, 2, res)[0]
    return x[:, :ch].contiguous()


def build(module, name, bias, fc2_gain=1.0, bn1d_var_gain=1.0):
    """CNN32 / CNN28 of `module` (oracle.models or eoe_amd.models) with deterministic_init and the running statistics above; the
    saturated-score cases multiply fc2's weights by fc2_gain and bn1d1's running variance by bn1d_var_gain"""
    m = getattr(module, name)(bias=bias)
    omodels.deterministic_init(m, tag=f"explain_cnn/{name}")
    set_running_stats(m)
    with torch.no_grad():
        m.fc2.weight.mul_(fc2_gain)
        m.bn1d1.running_var.mul_(bn1d_var_gain)
    return m


# The saturated-score cases: (model, fc2 gain, gain of bn1d1's running variance).  HSC's score is 1 - exp(-(sqrt(|out|^2 + 1) - 1)), its
# derivative of order exp(-|out|).  What a case can ask of an fp32 gradient follows from the format alone: exp(-|out|) is an fp32 number
# only for |out| < 103 (a normal one for |out| < 87), and `input_gradient`'s per-image seed, a power of two clamped to 2^100, brings
# the derivative to order one for |out| < 69.  Beyond that the correctly rounded fp32 derivative is 0 and so is the gradient, whatever
# computes it.  The running statistics are this file's to choose, so with fc2 x 64 bn1d1's running variance is raised by the smallest
# power of 4 that puts the fp64 oracle's |out| below 69 (with bias and the fused Normalize): CNN32 |out| = 1304 ... 1462 at gain 1 of the
# variance, 83 ... 93 at 256, 43 ... 48 at 1024; CNN28 510 ... 543 at 1, 63 ... 68 at 64.  (fc2 x 64 on the statistics of
# set_running_stats alone: measured d score / d out = 0.0 for every image, and a gradient of 0.)  The two cases with smaller gains run
# on the unchanged statistics: |out| = 41 ... 46 and 63 ... 68.
SATURATED_CASES = (("CNN32", 2.0, 1.0), ("CNN28", 8.0, 1.0), ("CNN32", 64.0, 1024.0), ("CNN28", 64.0, 64.0))


def _round(t, dtype):
    return t if dtype is None else t.to(dtype).to(t.dtype)


def _ste(t, dtype):
    """t rounded to `dtype`, straight-through for the gradient"""
    return t if dtype is None else t + (_round(t.detach(), dtype) - t.detach())


def oracle_forward(m, x, dtype=None):
    """oracle.models.CNN32 / CNN28 .forward in eval mode; with `dtype` every convolution's input rounded to it (the weights are rounded
    by the caller)"""
    convs = [(m.conv1, m.bn2d1), (m.conv2, m.bn2d2)] + ([(m.conv3, m.bn2d3)] if hasattr(m, "conv3") else [])
    for conv, bn in convs:
        x = F.max_pool2d(F.leaky_relu(bn(omodels.CNN32._conv(_ste(x, dtype), conv)), 0.01), 2, 2)
    x = x.reshape(x.shape[0], -1)
    x = F.leaky_relu(m.bn1d1(m.fc1(x)), 0.01)
    return m.fc2(x)


@functools.lru_cache(maxsize=None)
def oracle_grad(name, bias, norm, dtype=None, fc2_gain=1.0):
    """d hsc_score / d image through the fp64 oracle in eval mode, [3, C, H, W]; with `dtype` the weights (every matrix and kernel) and
    every convolution's input are rounded to it first: what the 16-bit forward alone costs"""
    m = build(omodels, name, bias, fc2_gain).double().eval()
    if dtype is not None:
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() >= 2:
                    p.copy_(_round(p, dtype))
    x = images_of(name).double().requires_grad_()
    mean, std = normalize_of(name, norm)
    inp = x
    if norm:
        c = x.shape[1]
        inp = (x - torch.tensor(mean).double().view(1, c, 1, 1)) / torch.tensor(std).double().view(1, c, 1, 1)
    out = oracle_forward(m, inp, dtype)
    if dtype is None:
        assert torch.equal(out, m(inp))
    (g,) = torch.autograd.grad(objectives.hsc_score(out).sum(), x)
    return g


def distance(got, ref):
    """the worst image's relative rms distance"""
    d = (got.double() - ref).flatten(1)
    return float((d.pow(2).mean(1).sqrt() / ref.flatten(1).pow(2).mean(1).sqrt()).max())


def floor(name, bias, norm, dtype):
    """the distance the 16-bit forward alone puts between two fp64 evaluations: a max-pool window whose two largest entries lie within
    16-bit rounding of each other sends its gradient to another pixel"""
    return distance(oracle_grad(name, bias, norm, dtype), oracle_grad(name, bias, norm))


CASES = [(n, b, nm) for n in MODELS for b in (False, True) for nm in (False, True)]
DTYPE_SCALES = ((torch.bfloat16, 1.0), (torch.float16, 1.0), (torch.float16, 256.0))

# ------------------------------------------------------------------------------------------------ measured
# Per-image relative rms distance of input_gradient to autograd through the fp64 oracle (HSC score, n = 3, eval mode, the running
# statistics of set_running_stats), the worst image of each case, measured on an MI355X (tests/test_gpu_explain_cnn.py prints every
# figure before it asserts).  fp16 at gradient scale 1 and at 256 agreed to the digits shown.  (model, bias, Normalize fused) -> distance.
INPUT_GRAD_MEASURED = {
    torch.bfloat16: {("CNN32", False, False): 1.364e-01, ("CNN32", False, True): 1.662e-01, ("CNN32", True, False): 1.425e-01,
                     ("CNN32", True, True): 1.668e-01, ("CNN28", False, False): 1.159e-01, ("CNN28", False, True): 9.815e-02,
                     ("CNN28", True, False): 1.220e-01, ("CNN28", True, True): 7.645e-02},
    torch.float16: {("CNN32", False, False): 7.498e-02, ("CNN32", False, True): 1.677e-02, ("CNN32", True, False): 4.080e-02,
                    ("CNN32", True, True): 2.313e-02, ("CNN28", False, False): 2.555e-03, ("CNN28", False, True): 6.561e-02,
                    ("CNN28", True, False): 2.142e-02, ("CNN28", True, True): 1.405e-02},
}
# (every case landed within 6 % of its OWN floor below: the kernels meet the flips the rounded oracle meets, and the 16-bit dy chain adds
# next to nothing)
# parity mode (fp32 convolutions), the same cases, bf16 and fp16 compute alike: the worst over the cases per model (5.7e-7 ... 2.2e-6)
PARITY_MEASURED = {"CNN32": 2.229e-06, "CNN28": 1.662e-06}
# the floors of `floor()`, computed on the CPU (`python tests/explain_cnn_util.py` prints them): (model, bias, Normalize) -> distance
FLOOR = {
    torch.bfloat16: {("CNN32", False, False): 1.342e-01, ("CNN32", False, True): 1.668e-01, ("CNN32", True, False): 1.489e-01,
                     ("CNN32", True, True): 1.669e-01, ("CNN28", False, False): 1.159e-01, ("CNN28", False, True): 9.847e-02,
                     ("CNN28", True, False): 1.220e-01, ("CNN28", True, True): 7.578e-02},
    torch.float16: {("CNN32", False, False): 7.494e-02, ("CNN32", False, True): 1.677e-02, ("CNN32", True, False): 4.080e-02,
                    ("CNN32", True, True): 2.314e-02, ("CNN28", False, False): 2.511e-03, ("CNN28", False, True): 6.564e-02,
                    ("CNN28", True, False): 2.140e-02, ("CNN28", True, True): 1.414e-02},
}

PARITY_CEILING = 1e-3                          # the project's parity bar
CEILING_FACTOR = 3.0                           # fast mode: a measurement beyond 3 x its case's own floor is a defect (the 16-bit dy chain
#                                                adds a second contribution of the floor's kind, and 3 x leaves room for it and no more)
# the bars: twice the worst measured value, per compute dtype and model
INPUT_GRAD_BAR = {torch.bfloat16: {"CNN32": 3.336e-01, "CNN28": 2.440e-01}, torch.float16: {"CNN32": 1.4996e-01, "CNN28": 1.3122e-01}}
PARITY_BAR = {"CNN32": 4.458e-06, "CNN28": 3.324e-06}


if __name__ == "__main__":
    for dt in (torch.bfloat16, torch.float16):
        for case in CASES:
            print(dt, case, f"{floor(*case, dt):.3e}")
