"""Where in an image does its anomaly score come from: input-gradient heat maps for the LayerNorm (ViT) towers and the BatchNorm CNNs
(CNN32, CNN28).

  input_gradient(model, images, score_fn)   d score / d image through the training backward in eval mode (LayerNorm is the same in train
                                            and eval mode; BatchNorm takes its running statistics, `bn_act_pool_bwd_kernel` without batch
                                            statistics), the last hop -- patch embedding back to pixels -- by `eoe_unpatchify_grad`, a
                                            CNN's first convolution back to the image by `eoe_conv_image_dgrad`
  saliency(grad, x, mode, pool, smooth)     the three-channel gradient reduced to one map per image (`eoe_saliency_map`)
  overlay(maps, pictures, alpha)            the map laid over the pictures, uint8 NHWC: a form `imgrid.image_grid` takes
                                            (`eoe_heat_overlay_u8`)
  score_fn(trainer_or_name, ...)            each objective's `compute_anomaly_score` restated with differentiable torch operations
  saliency_np / overlay_np                  the numpy statements of the two kernels (tests, CPU tensors)
  conv_image_dgrad_np                       the float64 numpy statement of `eoe_conv_image_dgrad`

and, from the forward pass alone, attention rollout (Abnar & Zuidema 2020; csrc/rollout.hip):

  attention_probs(qkv, n, L, heads, fuse)   the softmax probabilities of one block fused over its heads, fp32 [n, L, L] (`eoe_attn_probs`)
  attention_rollout(model, images, ...)     R <- A^_l R over the blocks in forward order (`eoe_rollout_step`), the class token's row as a
                                            patch-level map fp32 [n, H, W] (`eoe_rollout_map`): a form `overlay` takes
  attention_probs_np / attention_rollout_np the float64 numpy statements of the two

and, for the WideResNet + CBAM encoder, Grad-CAM (Selvaraju et al. 2017; csrc/gradcam.hip):

  grad_cam(model, images, score_fn, layer, mode, size)
                                            the activation A of `layerK` weighted by the gradient dA of the score at it, rectified and
                                            upsampled onto the image, fp32 [n, H, W]: a form `overlay` takes.  'gradcam'
                                            relu(sum_c mean_p(dA)_c A_c) (`eoe_cam_weights`, `eoe_cam_map`), 'hirescam' relu(sum_c dA_c A_c)
                                            (`eoe_cam_map` alone); `eoe_cam_upsample` is interpolate(bilinear, align_corners=False).  The
                                            backward from the score to the layer runs in eval mode and asks for no parameter gradient:
                                            the conv units skip theirs, the CBAM junction takes `eoe_cbam_junction_bwd_data`
  cam_np / bilinear_np / grad_cam_np        the numpy statements (sums in float64, rounded once)

WideResNet is served by `grad_cam`, not by `input_gradient`: pixel gradients through 17 convolutions, three max / argmax gates per block and
a stride-2 stem are noise, and `input_gradient` (like `explain=True`) keeps refusing it and anything else with a BatchNorm that is not a
CNN32's or CNN28's own.  No BatchNorm encoder has attention to roll out.
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check, lib

MODES = {"max": _lib.EOE_SALIENCY_MAX, "l2": _lib.EOE_SALIENCY_L2, "gradxinput": _lib.EOE_SALIENCY_GRADXINPUT}
FUSE = {"mean": _lib.EOE_FUSE_MEAN, "max": _lib.EOE_FUSE_MAX, "min": _lib.EOE_FUSE_MIN}
CAM_MODES = {"gradcam": _lib.EOE_CAM_GRADCAM, "hirescam": _lib.EOE_CAM_HIRESCAM}
CAM_LAYERS = ("layer1", "layer2", "layer3", "layer4")
HEAT_COLOUR = (255.0, 0.0, 0.0)
OBJECTIVES = ("hsc", "bce", "focal", "dsad", "dsvdd", "clip")


# ------------------------------------------------------------------------------------------------ scores
def _objective_name(trainer_or_name) -> str:
    if isinstance(trainer_or_name, str):
        name = trainer_or_name
    else:
        from .training import TRAINER
        cls = trainer_or_name if isinstance(trainer_or_name, type) else type(trainer_or_name)
        name = next((k for k, t in TRAINER.items() if issubclass(cls, t)), None)
    if name not in OBJECTIVES:
        raise ValueError(f"score_fn: no differentiable score for {trainer_or_name!r}; known objectives: {OBJECTIVES}")
    return name


def score_fn(trainer_or_name, center=None, nominal_label: int = 0):
    """The differentiable restatement of an objective's `compute_anomaly_score`: a callable features [n, d] -> scores [n] made of torch
    elementwise operations and row sums (host plumbing on an n x d matrix; the score kernels themselves keep no tape).  `trainer_or_name`
    is a trainer (its `center` is taken when none is given), a trainer class or one of 'hsc', 'bce', 'focal', 'dsad', 'dsvdd', 'clip';
    dsvdd needs its centre [1, d], clip the text features [T, d]."""
    name = _objective_name(trainer_or_name)
    if center is None and not isinstance(trainer_or_name, (str, type)):
        center = getattr(trainer_or_name, "center", None)
    if name in ("dsvdd", "clip") and center is None:
        raise ValueError(f"score_fn: the {name} score needs its center ({'the text features' if name == 'clip' else 'prepare_metric'})")
    if name in ("hsc", "dsad"):               # hsc.py:12-15 (dsad.py:12-15 is the same score): 1 - exp(-(sqrt(|f|^2 + 1) - 1))
        return lambda f: 1 - torch.exp(-(torch.sqrt((f * f).sum(dim=1) + 1) - 1))
    if name in ("bce", "focal"):              # bce.py:15-17, focal.py:30-32
        def bce(f):
            s = torch.sigmoid(f).reshape(f.shape[0])
            return s if nominal_label == 0 else 1 - s
        return bce
    if name == "dsvdd":                       # dsvdd.py:24-25
        return lambda f: ((f - center.detach().to(f)) ** 2).sum(dim=-1)

    def clip(f):                              # clip.py:66-79: the softmax probability of the last prompt
        t = center.detach().to(f)
        t = t / t.norm(dim=-1, keepdim=True)
        return (100.0 * (f / f.norm(dim=-1, keepdim=True)) @ t.T).softmax(dim=-1)[:, -1]
    return clip


# ------------------------------------------------------------------------------------------------ the gradient
def _batchnorm_cnn(model: torch.nn.Module, who: str) -> bool:
    """whether the model is one of the BatchNorm encoders `who` serves: False without any `_BatchNorm` module, True where every one is a
    direct child of a CNN32 or CNN28; anything else is refused"""
    from .models.cnn import CNN28, CNN32
    served = {id(c) for m in model.modules() if isinstance(m, (CNN32, CNN28)) for c in m.children()}
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    for m in bns:
        if id(m) not in served:
            raise NotImplementedError(f"{who}: {type(model).__name__} contains a {type(m).__name__} outside a CNN32 or CNN28; an explanation "
                                      "differentiates the eval-mode BatchNorm (running statistics), and the residual junctions and CBAM "
                                      "gates (WideResNet) have no eval-mode backward -- only the ViT towers, CNN32 and CNN28 can be explained")
    return bool(bns)


def conv_image_dgrad_np(dy: np.ndarray, w: np.ndarray, n: int, Hi: int, Wi: int, stride: int, pad: int, std=None,
                        scale_inv: float = 1.0) -> np.ndarray:
    """numpy statement of `eoe_conv_image_dgrad` in float64: dy [n Ho Wo, cout] and w [cout, cin, kh, kw] -> dx [n, cin, Hi, Wi],
    dx[i, c, hi, wi] = (scale_inv / std[c]) sum over (co, ky, kx) of dy[(i, ho, wo), co] w[co, c, ky, kx] with ho stride - pad + ky == hi
    and wo stride - pad + kx == wi; Ho = (Hi + 2 pad - kh) / stride + 1, likewise Wo; std None = 1."""
    w = np.asarray(w, dtype=np.float64)
    cout, cin, kh, kw = w.shape
    Ho, Wo = (Hi + 2 * pad - kh) // stride + 1, (Wi + 2 * pad - kw) // stride + 1
    d = np.asarray(dy, dtype=np.float64).reshape(n, Ho, Wo, cout)
    # the gradient of the padded image, tap by tap; rows / columns past what the last output position reads receive nothing
    full = np.zeros((n, cin, max(Hi + 2 * pad, (Ho - 1) * stride + kh), max(Wi + 2 * pad, (Wo - 1) * stride + kw)))
    for ky in range(kh):
        for kx in range(kw):
            full[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] += np.einsum("nhwo,oc->nchw", d, w[:, :, ky, kx])
    dx = full[:, :, pad:pad + Hi, pad:pad + Wi]
    m = np.full(cin, float(scale_inv)) if std is None else float(scale_inv) / np.asarray(std, dtype=np.float64).reshape(cin)
    return dx * m.reshape(1, cin, 1, 1)


def input_gradient(model: torch.nn.Module, images: torch.Tensor, score_fn) -> torch.Tensor:
    """d score_i / d images_i, fp32 of the images' shape [n, C, H, W] (C = 3; 1 for CNN28), with respect to the tensor handed in (in front
    of a Normalize the encoder fuses).  `score_fn` maps the model's output [n, d] to [n] scores (`explain.score_fn`).

    One forward with the tape on and one `torch.autograd.grad(seed * score.sum(), images)`: no parameter's `.grad` is touched, and the ViT
    blocks' backward takes its in-line form (no late write, `ops._late_write_ok`).  The samples of a LayerNorm tower are independent of
    each other, so the gradient of the sum of the scores IS the per-sample gradient.  Under BatchNorm that holds in eval mode only (the
    running statistics are constants), which is how the model runs here: a CNN32's or CNN28's BatchNorm units take the eval form of their
    backward (dy = gamma rstd g), and their parameters do not require a gradient while the tape is recorded, so the backward launches no
    weight-gradient, column-sum or unpack kernel and writes into no gradient arena; the first convolution hands its gradient back to
    the image (`eoe_conv_image_dgrad`).  A model with a `_BatchNorm` module that is not a direct child of a CNN32 or CNN28 -- WideResNet,
    or anything that wraps one -- is refused: the residual junctions and the CBAM gates have no eval-mode backward.  The running buffers
    are not touched; the model gets every module's train / eval flag (and every parameter its `requires_grad`) back afterwards.
    `seed` is the package's gradient scale
    (`eoe_amd.set_grad_scale`: a power of two, 256 for fp16 compute in the trainers, 1 for bf16) times a power of two per image that
    brings d score_i / d out_i to order one, which keeps the 16-bit dY chain from underflowing even where a score is saturated;
    `eoe_unpatchify_grad` / `eoe_conv_image_dgrad` divides the scale out again and one multiplication of the finished gradient the
    per-image factors, both exactly."""
    cnn = _batchnorm_cnn(model, "input_gradient")
    flags = [(m, m.training) for m in model.modules()]
    frozen = [p for p in model.parameters() if p.requires_grad] if cnn else []
    model.eval()
    try:
        for p in frozen:
            p.requires_grad_(False)
        x = images.detach().requires_grad_()
        with torch.enable_grad():
            out = model(x)
            # d score / d out on the n x d matrix, in fp32 on its own small tape
            o = out.detach().requires_grad_()
            (df,) = torch.autograd.grad(score_fn(o).reshape(-1).sum(), o)
            # A saturated score (1 - exp(-d) at a large d) has a gradient of 1e-9 and less: behind any fixed seed fp16's dY chain
            # flushes it.  Each image is therefore seeded with its own power of two, which brings the largest entry of its row into
            # [1, 2); the factors are exact to apply and to divide out of the finished gradient (eoe_unpatchify_grad undoes the scale).
            amax = df.abs().amax(dim=1)
            live = torch.isfinite(amax) & (amax > 0)
            expo = torch.where(live, torch.floor(torch.log2(torch.where(live, amax, torch.ones_like(amax)))), torch.zeros_like(amax))
            expo = expo.clamp(-100.0, 100.0)
            seed = df * (torch.exp2(-expo) * ops.grad_scale())[:, None]
            (grad,) = torch.autograd.grad(out, x, grad_outputs=seed)
            grad = grad.mul_(torch.exp2(expo)[:, None, None, None])          # the per-image seeds undone: powers of two, exact
    finally:
        for p in frozen:
            p.requires_grad_(True)
        for m, was in flags:
            m.training = was
    return grad


# ------------------------------------------------------------------------------------------------ maps
def _pool_arg(pool) -> int:
    pool = 0 if pool is None else int(pool)
    if pool < 0:
        raise ValueError(f"saliency: pool must be a positive block size or None, not {pool}")
    return pool


def saliency_np(grad: np.ndarray, x: np.ndarray = None, mode: str = "max", pool=None) -> np.ndarray:
    """numpy statement of `eoe_saliency_map`: fp32 [n, H, W] from grad [n, C, H, W].  'max' and the products of 'gradxinput' are the
    kernel's own fp32 operations (exact); sums over channels, the square root and the block means are taken in float64 and rounded once."""
    g = np.asarray(grad, dtype=np.float32)
    if mode not in MODES:
        raise ValueError(f"saliency: mode {mode!r} is none of {tuple(MODES)}")
    if mode == "max":
        s = np.fmax.reduce(np.abs(g), axis=1)
    elif mode == "l2":
        s = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))
    else:
        if x is None:
            raise ValueError("saliency: gradxinput needs x")
        s = np.abs(g * np.asarray(x, dtype=np.float32)).astype(np.float64).sum(axis=1)
    pool = _pool_arg(pool)
    if pool > 1:
        n, H, W = s.shape
        if H % pool or W % pool:
            raise ValueError(f"saliency: pool = {pool} does not divide H = {H} and W = {W}")
        m = s.astype(np.float64).reshape(n, H // pool, pool, W // pool, pool).mean(axis=(2, 4))
        s = np.repeat(np.repeat(m, pool, axis=1), pool, axis=2)
    return s.astype(np.float32)


def saliency(grad: torch.Tensor, x: torch.Tensor = None, mode: str = "max", pool=None, smooth: float = 0) -> torch.Tensor:
    """One map per image, fp32 [n, H, W], from a gradient fp32 [n, C, H, W] (C 1 or 3): mode 'max' max_c |g_c|, 'l2' sqrt(sum_c g_c^2),
    'gradxinput' sum_c |g_c x_c| (needs `x`, the images the gradient belongs to).  `pool=p` gives every aligned p x p block its mean: with
    p = the patch size, the patch-level map of a ViT.  `smooth=sigma` > 0 blurs the map with the Gaussian of the blur multi-scale mode
    (`eoe_msm_filter`; taps as `msm.blur_taps_k` / `msm.blur_np`).  One launch on the device (two with smooth); CPU tensors go through
    `saliency_np` / `msm.blur_np`."""
    if mode not in MODES:
        raise ValueError(f"saliency: mode {mode!r} is none of {tuple(MODES)}")
    if grad.dim() != 4 or grad.shape[1] not in (1, 3):
        raise ValueError(f"saliency: grad must be [n, C, H, W] with C 1 or 3, not {tuple(grad.shape)}")
    if mode == "gradxinput" and (x is None or x.shape != grad.shape):
        raise ValueError("saliency: gradxinput needs x of grad's shape")
    pool = _pool_arg(pool)
    n, ch, H, W = grad.shape
    if pool > 1 and (H % pool or W % pool):
        raise ValueError(f"saliency: pool = {pool} does not divide H = {H} and W = {W}")
    if not grad.is_cuda:
        from .msm import blur_np
        s = saliency_np(grad.detach().numpy(), None if x is None else x.detach().numpy(), mode, pool)
        if smooth and smooth > 0:
            s = blur_np(s[:, None], float(smooth))[:, 0].astype(np.float32)
        return torch.from_numpy(s)
    g = grad.detach().contiguous().float()
    xx = x.detach().to(g.device).contiguous().float() if mode == "gradxinput" else None
    s = torch.empty((n, H, W), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        check(lib.eoe_saliency_map(g.data_ptr(), ops._p(xx), s.data_ptr(), n, ch, H, W, MODES[mode], pool, ops._stream()), "eoe_saliency_map")
        if smooth and smooth > 0 and n:
            from .msm import msm_filter
            s = msm_filter(s[:, None], "blur", smooth)[:, 0]
    return s


def _pictures_u8(pictures) -> bool:
    dt = pictures.dtype
    if dt in (torch.uint8, np.dtype(np.uint8)):
        return True
    if dt in (torch.float32, np.dtype(np.float32)):
        return False
    raise ValueError(f"overlay: pictures must be fp32 NCHW (ToTensor's scale) or uint8 NHWC, not {dt}")


def _overlay_shapes(maps, pictures, alpha):
    u8 = _pictures_u8(pictures)
    if maps.ndim != 3 or pictures.ndim != 4:
        raise ValueError(f"overlay: maps [n, H, W] and pictures of four dimensions, not {tuple(maps.shape)} and {tuple(pictures.shape)}")
    n, H, W = maps.shape
    ch = pictures.shape[3] if u8 else pictures.shape[1]
    want = (n, H, W, ch) if u8 else (n, ch, H, W)
    if ch not in (1, 3) or tuple(pictures.shape) != want:
        raise ValueError(f"overlay: {'uint8 NHWC' if u8 else 'fp32 NCHW'} pictures of shape {tuple(pictures.shape)} do not fit maps "
                         f"{tuple(maps.shape)} (C 1 or 3)")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"overlay: alpha must be in [0, 1], not {alpha}")
    return u8, n, H, W, ch


def overlay_np(maps: np.ndarray, pictures: np.ndarray, alpha: float = 0.6, dtype=np.float32) -> np.ndarray:
    """numpy statement of `eoe_heat_overlay_u8`, uint8 [n, H, W, 3].  With dtype=np.float32 (the default) every operation is the kernel's,
    in its order; dtype=np.float64 is the same formula in double precision, which can differ from it only where
    img (1 - alpha t) + col alpha t + 0.5 lies within rounding of an integer."""
    maps, pictures = np.asarray(maps, dtype=np.float32), np.asarray(pictures)
    u8, n, H, W, ch = _overlay_shapes(maps, pictures, alpha)
    ft = np.dtype(dtype).type
    img = pictures.astype(dtype) if u8 else (pictures.astype(dtype) * ft(255.0)).transpose(0, 2, 3, 1)
    img = np.repeat(img, 3, axis=3) if ch == 1 else img
    out = np.empty((n, H, W, 3), dtype=np.uint8)
    col = np.array(HEAT_COLOUR, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(n):
            s = maps[i].astype(dtype)
            fin = np.isfinite(maps[i])
            t = np.zeros((H, W), dtype=dtype)
            if fin.any():
                lo, hi = s[fin].min(), s[fin].max()
                d = ft(hi - lo)
                if d > 0 and np.isfinite(d):
                    t[fin] = ((s[fin] - lo) / d).astype(dtype)
            a = (ft(alpha) * t).astype(dtype)[..., None]
            ia = (ft(1.0) - a).astype(dtype)
            v = np.floor(((img[i] * ia).astype(dtype) + (col * a).astype(dtype)).astype(dtype) + ft(0.5))
            out[i] = np.clip(np.nan_to_num(v, nan=0.0), 0.0, 255.0).astype(np.uint8)
    return out


def overlay(maps: torch.Tensor, pictures: torch.Tensor, alpha: float = 0.6) -> torch.Tensor:
    """The maps fp32 [n, H, W] laid over the pictures -- fp32 NCHW in ToTensor's scale, or uint8 NHWC; one channel fills the three --
    as uint8 [n, H, W, 3], which `imgrid.image_grid` and `JsonLogger.logimg` take.  Per image t = (s - min) / (max - min) over the map's
    finite entries (0 for a constant map and at a non-finite entry); byte = floor(img (1 - alpha t) + (255, 0, 0) alpha t + 0.5) with img
    on the 0...255 scale.  One launch (`eoe_heat_overlay_u8`); CPU tensors go through `overlay_np`."""
    u8, n, H, W, ch = _overlay_shapes(maps, pictures, alpha)
    if not maps.is_cuda:
        return torch.from_numpy(overlay_np(maps.detach().float().numpy(), pictures.detach().cpu().numpy(), alpha))
    s = maps.detach().contiguous().float()
    pics = pictures.detach().to(s.device).contiguous()
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=s.device)
    with torch.cuda.device(s.device):
        check(lib.eoe_heat_overlay_u8(s.data_ptr(), pics.data_ptr(), 1 if u8 else 0, out.data_ptr(), n, ch, H, W, float(alpha), ops._stream()),
              "eoe_heat_overlay_u8")
    return out


# ------------------------------------------------------------------------------------------------ attention rollout
def _fuse_arg(fuse: str) -> int:
    if fuse not in FUSE:
        raise ValueError(f"attention: fuse {fuse!r} is none of {tuple(FUSE)}")
    return FUSE[fuse]


def attention_probs_np(qkv: np.ndarray, n: int, L: int, heads: int, fuse: str = "mean") -> np.ndarray:
    """numpy statement of `eoe_attn_probs` in float64: qkv [n L, 3 D] (the 16-bit values, q | k | v, D = 64 heads) -> [n, L, L].  Per head
    softmax_rows(q_h k_h^T / 8) with the row maximum subtracted; 'mean' sums the heads in order and multiplies by 1 / heads, 'max' / 'min'
    take the element-wise extreme."""
    _fuse_arg(fuse)
    D = 64 * heads
    x = np.asarray(qkv, dtype=np.float64).reshape(n, L, 3 * D)
    out = None
    for h in range(heads):
        q, k = x[:, :, 64 * h:64 * h + 64], x[:, :, D + 64 * h:D + 64 * h + 64]
        s = np.einsum("nqd,nkd->nqk", q, k) / 8.0
        e = np.exp(s - s.max(axis=2, keepdims=True))
        p = e / e.sum(axis=2, keepdims=True)
        out = p if out is None else out + p if fuse == "mean" else np.maximum(out, p) if fuse == "max" else np.minimum(out, p)
    return out * (1.0 / heads) if fuse == "mean" else out


def rollout_matrix_np(probs: np.ndarray, residual: float) -> np.ndarray:
    """A^ of `eoe_rollout_step` in float64: (1 - residual) probs + residual I, every row divided by its sum; a row whose sum is 0 or not
    finite is the identity row"""
    p = np.asarray(probs, dtype=np.float64)
    eye = np.eye(p.shape[-1])
    a = (1.0 - residual) * p + residual * eye
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = a.sum(axis=-1, keepdims=True)
        ok = np.isfinite(s) & (s != 0)
        return np.where(ok, a / np.where(ok, s, 1.0), eye)


def attention_rollout_np(probs_per_layer, residual: float, grid: int, patch: int) -> np.ndarray:
    """numpy statement of the rollout in float64: R = A^_last ... A^_first over the layers' fused probabilities [n, L, L] (forward order),
    then the class token's row without its class column as [n, grid patch, grid patch], every patch block constant."""
    if not 0.0 <= residual < 1.0:
        raise ValueError(f"attention_rollout: residual must be in [0, 1), not {residual}")
    r = None
    for p in probs_per_layer:
        a = rollout_matrix_np(p, residual)
        r = a if r is None else a @ r
    n, L, _ = r.shape
    if L != grid * grid + 1:
        raise ValueError(f"attention_rollout: L = {L} is not grid^2 + 1 (grid = {grid})")
    m = r[:, 0, 1:].reshape(n, grid, grid)
    return np.repeat(np.repeat(m, patch, axis=1), patch, axis=2)


def attention_probs(qkv: torch.Tensor, n: int, L: int, heads: int, fuse: str = "mean") -> torch.Tensor:
    """One block's softmax probabilities fused over its heads, fp32 [n, L, L], from the packed 16-bit qkv [n L, 3 D] the attention kernels
    read (q | k | v, D = 64 heads; the V third is not read); 1 <= L <= ops.ATTN_LONG_MAX_L.  `fuse`: 'mean' (the heads summed in order,
    times 1 / heads), 'max', 'min'.  One launch (`eoe_attn_probs`); device tensors only."""
    code = _fuse_arg(fuse)
    ops._chk(qkv)
    if qkv.dim() != 2 or tuple(qkv.shape) != (n * L, 3 * 64 * heads) or not qkv.is_contiguous():
        raise ValueError(f"attention_probs: qkv must be contiguous [n L, 192 heads] = [{n * L}, {192 * heads}], not {tuple(qkv.shape)}")
    probs = torch.empty((n, L, L), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(lib.eoe_attn_probs(qkv.data_ptr(), probs.data_ptr(), n, L, heads, ops.dtype_code(qkv.dtype), code, ops._stream()), "eoe_attn_probs")
    return probs


def _visual_transformer(model: torch.nn.Module, who: str):
    from .models.clip_vit import VisualTransformer
    vit = next((m for m in model.modules() if isinstance(m, VisualTransformer)), None)
    if vit is None:
        raise NotImplementedError(f"{who}: {type(model).__name__} has no VisualTransformer whose attention could be rolled out")
    return vit


def block_qkv(blk, tok: torch.Tensor) -> torch.Tensor:
    """the packed 16-bit qkv [n L, 3 D] of a ResidualAttentionBlock from its input tokens fp32 [n L, D], by the stand-alone operations the
    block's own kernel chain is made of: LayerNorm-1 into the compute type, the in-projection as an NT GEMM with its bias"""
    M, D = tok.shape
    dt = ops.compute_dtype()
    xn = torch.empty((M, D), dtype=dt, device=tok.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=tok.device)
    ops.layernorm_fwd(tok, blk.ln_1.weight, blk.ln_1.bias, M, D, D, xn, stats)
    w16, _ = ops.shadow.get(blk.attn.in_proj_weight, True, True)
    qkv = torch.empty((M, 3 * D), dtype=dt, device=tok.device)
    return ops.gemm_nt(xn, w16, qkv, bias=blk.attn.in_proj_bias)


def attention_rollout(model: torch.nn.Module, images: torch.Tensor, fuse: str = "mean", residual: float = 0.5,
                      start_layer: int = 0) -> torch.Tensor:
    """Attention rollout of the model's ViT tower, fp32 [n, H, W] (H = W = the tower's input resolution): how much of each patch reaches
    the class token through the attention of the blocks `start_layer` ... last, every patch block of a map constant -- a form `overlay`
    and `imgrid.image_grid` take.

    Forward pass only, under `torch.no_grad()`: the images are embedded as `VisualTransformer.forward` embeds them (the fused Normalize
    included); per block the packed qkv is computed from the block's input (`block_qkv`), `eoe_attn_probs` fuses the heads' softmax
    probabilities ('mean', 'max' or 'min'), and `eoe_rollout_step` takes R <- A^ R with A^ = (1 - residual) P + residual I, rows
    normalised -- the matrix form in forward order, which holds one [n, L, L] probability buffer and two R buffers whatever the depth.
    `eoe_rollout_map` cuts the class token's row into the map.  `residual` in [0, 1) is the weight of the skip connection (0.5 in the
    paper); a negative `start_layer` counts from the end.  `start_layer = -1` with `residual = 0` is the raw class-token attention of
    the last block, bit for bit row 0 of its `attention_probs` (a row whose fp32 sum is one within the sum's own rounding, 2^-20,
    is not divided again).  Neither the score nor the objective enters: the map does not fade where
    a score saturates.  A model without a VisualTransformer is refused (NotImplementedError), CPU tensors as the tower refuses them."""
    code = _fuse_arg(fuse)
    vit = _visual_transformer(model, "attention_rollout")
    if not 0.0 <= float(residual) < 1.0:
        raise ValueError(f"attention_rollout: residual must be in [0, 1), not {residual}")
    blocks = list(vit.transformer.resblocks)
    first = int(start_layer) + len(blocks) if start_layer < 0 else int(start_layer)
    if not 0 <= first < len(blocks):
        raise ValueError(f"attention_rollout: start_layer {start_layer} outside a tower of {len(blocks)} blocks")
    if not images.is_cuda:
        raise RuntimeError("eoe_amd.VisualTransformer runs on the GPU only (no CPU fallback)")
    n, grid, patch = images.shape[0], vit.input_resolution // vit.patch_size, vit.patch_size
    L = grid * grid + 1
    with torch.no_grad(), torch.cuda.device(images.device):
        tok = vit.embed(images)
        dev = tok.device
        probs = torch.empty((n, L, L), dtype=torch.float32, device=dev)
        r = [torch.empty_like(probs), torch.empty_like(probs)]
        cur = None                                                 # index of the buffer that holds R; None: the identity
        for i, blk in enumerate(blocks):
            if i >= first:
                qkv = block_qkv(blk, tok)
                check(lib.eoe_attn_probs(qkv.data_ptr(), probs.data_ptr(), n, L, blk.n_head, ops.dtype_code(qkv.dtype), code, ops._stream()),
                      "eoe_attn_probs")
                nxt = 0 if cur is None else 1 - cur
                check(lib.eoe_rollout_step(probs.data_ptr(), None if cur is None else r[cur].data_ptr(), r[nxt].data_ptr(), n, L,
                                           float(residual), ops._stream()), "eoe_rollout_step")
                cur = nxt
            if i + 1 < len(blocks):
                tok = blk.forward_tokens(tok, n)
        maps = torch.empty((n, grid * patch, grid * patch), dtype=torch.float32, device=dev)
        check(lib.eoe_rollout_map(r[cur].data_ptr(), maps.data_ptr(), n, L, grid, patch, ops._stream()), "eoe_rollout_map")
    return maps


# ------------------------------------------------------------------------------------------------ Grad-CAM
def cam_np(A: np.ndarray, dA: np.ndarray, mode: str = "gradcam") -> np.ndarray:
    """numpy statement of `eoe_cam_weights` + `eoe_cam_map`: fp32 [n, h, w] from A and dA fp32 NHWC [n, h, w, C]; 'gradcam'
    relu(sum_c alpha_c A_c) with alpha = the mean of dA over the pixels, 'hirescam' relu(sum_c dA_c A_c); every sum in float64, rounded
    once (alpha is rounded to fp32 as the kernel stores it).  relu keeps a NaN."""
    if mode not in CAM_MODES:
        raise ValueError(f"grad_cam: mode {mode!r} is none of {tuple(CAM_MODES)}")
    a, d = np.asarray(A, dtype=np.float32).astype(np.float64), np.asarray(dA, dtype=np.float32).astype(np.float64)
    if a.ndim != 4 or a.shape != d.shape:
        raise ValueError(f"grad_cam: A and dA must be NHWC of one shape, not {a.shape} and {d.shape}")
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "gradcam":
            alpha = d.mean(axis=(1, 2)).astype(np.float32).astype(np.float64)
            m = np.einsum("nhwc,nc->nhw", a, alpha)
        else:
            m = (a * d).sum(axis=3)
        m = np.where((m > 0) | np.isnan(m), m, 0.0)
        return m.astype(np.float32)


def _bilinear_axis(n_in: int, n_out: int):
    """source indices i0, i1 and the weight of i1 per destination index, as `eoe_cam_upsample` takes them: ((2 d + 1) n_in - n_out) /
    (2 n_out) clamped at 0, split in integers"""
    d = np.arange(n_out, dtype=np.int64)
    num, den = np.maximum((2 * d + 1) * n_in - n_out, 0), 2 * n_out
    i0 = num // den
    return i0, np.minimum(i0 + 1, n_in - 1), (num - i0 * den) / float(den)


def bilinear_np(m: np.ndarray, H: int, W: int) -> np.ndarray:
    """numpy statement of `eoe_cam_upsample` in float64, rounded once: [n, h, w] -> fp32 [n, H, W], the positions of
    torch.nn.functional.interpolate(mode='bilinear', align_corners=False)"""
    m = np.asarray(m, dtype=np.float64)
    n, h, w = m.shape
    if H < h or W < w:
        raise ValueError(f"grad_cam: the target {H} x {W} is smaller than the map {h} x {w}")
    y0, y1, ly = _bilinear_axis(h, H)
    x0, x1, lx = _bilinear_axis(w, W)
    ly, lx = ly[None, :, None], lx[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        top = (1 - lx) * m[:, y0][:, :, x0] + lx * m[:, y0][:, :, x1]
        bot = (1 - lx) * m[:, y1][:, :, x0] + lx * m[:, y1][:, :, x1]
        return ((1 - ly) * top + ly * bot).astype(np.float32)


def grad_cam_np(A: np.ndarray, dA: np.ndarray, mode: str, H: int, W: int) -> np.ndarray:
    """`cam_np` then `bilinear_np`, the map kept in float64 between the two"""
    if mode not in CAM_MODES:
        raise ValueError(f"grad_cam: mode {mode!r} is none of {tuple(CAM_MODES)}")
    a, d = np.asarray(A, dtype=np.float64), np.asarray(dA, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.einsum("nhwc,nc->nhw", a, d.mean(axis=(1, 2))) if mode == "gradcam" else (a * d).sum(axis=3)
        m = np.where((m > 0) | np.isnan(m), m, 0.0)
    return bilinear_np(m, H, W)


def cam_weights(dA: torch.Tensor) -> torch.Tensor:
    """alpha fp32 [n, C], the mean of dA fp32 NHWC [n, h, w, C] over the pixels (`eoe_cam_weights`); device tensors only"""
    ops._chk(dA)
    n, h, w, C = dA.shape
    alpha = torch.empty((n, C), dtype=torch.float32, device=dA.device)
    with torch.cuda.device(dA.device):
        check(lib.eoe_cam_weights(dA.data_ptr(), alpha.data_ptr(), n, h, w, C, ops._stream()), "eoe_cam_weights")
    return alpha


def cam_map(A: torch.Tensor, dA: torch.Tensor, mode: str = "gradcam") -> torch.Tensor:
    """the map at the layer's resolution, fp32 [n, h, w], from A and dA fp32 NHWC [n, h, w, C] (C % 4 == 0): one launch for 'hirescam', two
    for 'gradcam' (`eoe_cam_weights`, `eoe_cam_map`); CPU tensors go through `cam_np`"""
    if mode not in CAM_MODES:
        raise ValueError(f"grad_cam: mode {mode!r} is none of {tuple(CAM_MODES)}")
    if A.dim() != 4 or A.shape != dA.shape:
        raise ValueError(f"grad_cam: A and dA must be NHWC of one shape, not {tuple(A.shape)} and {tuple(dA.shape)}")
    if not A.is_cuda:
        return torch.from_numpy(cam_np(A.detach().numpy(), dA.detach().numpy(), mode))
    a, d = A.detach().contiguous().float(), dA.detach().to(A.device).contiguous().float()
    n, h, w, C = a.shape
    m = torch.empty((n, h, w), dtype=torch.float32, device=a.device)
    alpha = cam_weights(d) if mode == "gradcam" else None
    with torch.cuda.device(a.device):
        check(lib.eoe_cam_map(a.data_ptr(), d.data_ptr(), ops._p(alpha), m.data_ptr(), n, h, w, C, CAM_MODES[mode], ops._stream()), "eoe_cam_map")
    return m


def cam_upsample(m: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """bilinear [n, h, w] -> fp32 [n, H, W] (`eoe_cam_upsample`: interpolate's align_corners=False positions; h <= H, w <= W); CPU tensors go
    through `bilinear_np`"""
    if m.dim() != 3:
        raise ValueError(f"grad_cam: a map must be [n, h, w], not {tuple(m.shape)}")
    n, h, w = m.shape
    if H < h or W < w:
        raise ValueError(f"grad_cam: the target {H} x {W} is smaller than the map {h} x {w}")
    if not m.is_cuda:
        return torch.from_numpy(bilinear_np(m.detach().numpy(), H, W))
    mm = m.detach().contiguous().float()
    out = torch.empty((n, H, W), dtype=torch.float32, device=mm.device)
    with torch.cuda.device(mm.device):
        check(lib.eoe_cam_upsample(mm.data_ptr(), out.data_ptr(), n, h, w, int(H), int(W), ops._stream()), "eoe_cam_upsample")
    return out


def _wide_resnet(model: torch.nn.Module, who: str):
    from .models.resnet import WideResNet
    wrn = next((m for m in model.modules() if isinstance(m, WideResNet)), None)
    if wrn is None:
        raise NotImplementedError(f"{who}: {type(model).__name__} has no WideResNet whose layers could be mapped (Grad-CAM serves the "
                                  "WideResNet + CBAM encoder; the ViT towers, CNN32 and CNN28 have input_gradient)")
    return wrn


def grad_cam(model: torch.nn.Module, images: torch.Tensor, score_fn, layer: str = "layer4", mode: str = "gradcam", size=None) -> torch.Tensor:
    """Grad-CAM of the model's WideResNet, fp32 [n, H, W] (`size` = (H, W), default the images'): a form `overlay` takes.

    `WideResNet.features(images, layer)` gives the activation A of `layerK` without a tape; a detached leaf of it (with its 16-bit copy) goes
    through `WideResNet.head` -- and whatever the model wraps around the tower (`build_model`) -- with the tape on, and one
    `torch.autograd.grad(out, leaf, seed)` gives dA.  The model runs in eval mode and no parameter requires a gradient meanwhile: the
    conv units differentiate the running statistics and skip every parameter gradient, a CBAM junction takes its data-only backward
    (`eoe_cbam_junction_bwd_data`), so no running buffer, no `.grad` and no byte of a registered gradient arena is touched; every
    module's flag and every `requires_grad` is restored afterwards, also after an exception.  For 'layer4' the backward is pool and fc
    only.  The backward is seeded as `input_gradient` seeds it: the package's gradient scale times a per-image power of two that brings
    d score_i / d out_i to order one.  Both modes are positively homogeneous of degree 1 in dA, so the finished map is divided by that
    factor exactly (powers of two).  mode 'gradcam': relu(sum_c alpha_c A_c), alpha the pixel mean of dA; 'hirescam': relu(sum_c dA_c A_c).
    Refused before any launch: a model without a WideResNet (NotImplementedError), an unknown layer or mode (ValueError), a layer below
    'layer4' of a model in one of the unfused CBAM forms (`ops_resnet.FUSE_CBAM = False`, `no_spatial`: they have no data-only backward),
    CPU images as the model refuses them."""
    from . import ops_resnet
    wrn = _wide_resnet(model, "grad_cam")
    if layer not in CAM_LAYERS:
        raise ValueError(f"grad_cam: layer {layer!r} is none of {CAM_LAYERS}")
    if mode not in CAM_MODES:
        raise ValueError(f"grad_cam: mode {mode!r} is none of {tuple(CAM_MODES)}")
    if layer != "layer4":
        k = CAM_LAYERS.index(layer) + 1
        later = [b for name in CAM_LAYERS[k:] for b in getattr(wrn, name)]
        if not ops_resnet.FUSE_CBAM or any(b.cbam is None or b.cbam.no_spatial for b in later):
            raise NotImplementedError("grad_cam: below layer4 the backward crosses CBAM junctions, and only the fused unit has a data-only "
                                      "backward (ops_resnet.FUSE_CBAM = False and no_spatial are not served)")
    if images.dim() != 4:
        raise ValueError(f"grad_cam: images must be [n, 3, H, W], not {tuple(images.shape)}")
    H, W = (int(images.shape[2]), int(images.shape[3])) if size is None else (int(size[0]), int(size[1]))
    side = wrn.res >> (2 + CAM_LAYERS.index(layer))              # the stem divides by 4, every later layer by 2
    if H < side or W < side:
        raise ValueError(f"grad_cam: size {H} x {W} is smaller than {layer}'s map {side} x {side}")
    flags = [(m, m.training) for m in model.modules()]
    frozen = [p for p in model.parameters() if p.requires_grad]
    model.eval()
    try:
        for p in frozen:
            p.requires_grad_(False)
        # the model runs once, whatever it wraps around the tower; the tower's own forward is cut at the layer: the first half without a
        # tape, the second from a detached leaf
        cut = {}

        def halves(x):
            with torch.no_grad():
                cut["a"] = wrn.features(x, layer)
            cut["leaf"] = wrn.leaf_of(cut["a"])
            return wrn.head(cut["leaf"], layer)

        with torch.enable_grad():
            wrn.forward = halves
            try:
                out = model(images.detach())
            finally:
                del wrn.forward                                   # the instance attribute: the class's forward shows again
            a, leaf = cut["a"], cut["leaf"]
            o = out.detach().requires_grad_()
            (df,) = torch.autograd.grad(score_fn(o).reshape(-1).sum(), o)
            amax = df.abs().amax(dim=1)
            live = torch.isfinite(amax) & (amax > 0)
            expo = torch.where(live, torch.floor(torch.log2(torch.where(live, amax, torch.ones_like(amax)))), torch.zeros_like(amax))
            expo = expo.clamp(-100.0, 100.0)
            seed = df * (torch.exp2(-expo) * ops.grad_scale())[:, None]
            (dA,) = torch.autograd.grad(out, leaf, grad_outputs=seed)
        maps = cam_upsample(cam_map(a, dA, mode), H, W)
        maps.mul_((torch.exp2(expo) / ops.grad_scale())[:, None, None])      # the seeds undone: powers of two, exact
    finally:
        for p in frozen:
            p.requires_grad_(True)
        for mod, was in flags:
            mod.training = was
    return maps
