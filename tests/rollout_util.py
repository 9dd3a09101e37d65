"""Case tables, inputs, restatements and bars of the attention-rollout tests (tests/test_cpu_rollout.py, tests/test_gpu_rollout.py).

The bars are not tuned to the kernels.  Each is the largest error of a restatement that makes the kernel's KIND of rounding on the CPU,
against the float64 statement on the very inputs the GPU tests use, times a margin of 4:

  PROBS_BAR   `probs_np32` (fp32 dot products, fp32 exp, the kernel's fuse order) against `explain.attention_probs_np` over every case of
              PROBS_CASES x DTYPES x KINDS x fuse.  Measured 5.75e-6 ('peaked' at L = 640, 12 heads, fp16, max: logits of magnitude 40
              carry an fp32 ulp of 4e-6 into the exponent; 'gauss' 3.4e-7, 'equal' 3.9e-9); bar 2.3e-5.  The margin covers the MFMA
              accumulation order and the device exp.
  STEP_BAR    `rollout_chain_np(..., np.float32)` (A^ and the matrix products in fp32) against float64 over STEP_CASES x RESIDUALS x
              STEP_KINDS, after 1 and after 4 steps.  Measured 3.1e-6 (L = 640, residual 0.9, 'unnormalised', 4 steps); bar 1.24e-5.
  E2E bar     not a constant: the float64 restatement of the tower (`tower_rollout_f64`) with each layer's qkv rounded to the compute
              type against the pure float64 run, per (tower, dtype), times 4 -- the 4 for the rounding points that emulation leaves
              out (LayerNorm output, GEMM accumulation, the residual stream).  The GPU test measures it on the CPU before it compares;
              the values it found are in its docstring.
`test_the_bars_follow_from_a_fresh_measurement` repeats the first two measurements on the cases that set them."""
import numpy as np
import torch

GUARD = 4096
DTYPES = (torch.float16, torch.bfloat16)
KINDS = ("equal", "gauss", "peaked")
FUSES = ("mean", "max", "min")
# 63, 64, 65: the edges of the short and long attention kernels' own blocking; 129: a partial last key block; 17: a partial second tile
PROBS_LS = (1, 2, 17, 50, 63, 64, 65, 128, 129, 197, 640)
PROBS_CASES = [(L, heads, n) for L in PROBS_LS for heads in (1, 3, 12) for n in (1, 3) if not (L == 640 and n == 3)]
PROBS_MEASURED, PROBS_BAR = 5.75e-6, 2.3e-5
STEP_CASES = [(L, n) for L in (1, 2, 50, 65, 197, 640) for n in (1, 3)]
RESIDUALS = (0.0, 0.5, 0.9)
STEP_KINDS = ("stochastic", "unnormalised")
STEP_MEASURED, STEP_BAR = 3.1e-6, 1.24e-5
MAP_CASES = ((7, 32), (8, 4), (14, 16))


def _gen(*key):
    """a generator seeded by the case's name (the same on every machine and run)"""
    import zlib
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def qkv_case(L: int, heads: int, n: int, dtype, kind: str) -> torch.Tensor:
    """16-bit [n L, 3 D] on the CPU.  'equal': every q and k element 0.5 (uniform rows); 'gauss': unit Gaussian; 'peaked': q and k times
    sqrt(10), logits of standard deviation 10 whose row maxima reach about 30 (near one-hot rows).  V is filled with NaN: it is never read."""
    D = 64 * heads
    g = _gen("qkv", L, heads, n, kind)
    x = torch.randn((n * L, 3 * D), generator=g)
    if kind == "equal":
        x[:] = 0.5
    elif kind == "peaked":
        x *= 10.0 ** 0.5
    x[:, 2 * D:] = float("nan")
    return x.to(dtype)


def probs_np32(qkv: np.ndarray, n: int, L: int, heads: int, fuse: str) -> np.ndarray:
    """`explain.attention_probs_np` in fp32 arithmetic with the kernel's fuse order"""
    D = 64 * heads
    x = np.asarray(qkv, dtype=np.float32).reshape(n, L, 3 * D)
    out = None
    for h in range(heads):
        q, k = x[:, :, 64 * h:64 * h + 64], x[:, :, D + 64 * h:D + 64 * h + 64]
        s = np.matmul(q, k.transpose(0, 2, 1)).astype(np.float32) * np.float32(0.125)
        e = np.exp(s - s.max(axis=2, keepdims=True), dtype=np.float32)
        p = e / e.sum(axis=2, keepdims=True, dtype=np.float32)
        out = p if out is None else out + p if fuse == "mean" else np.maximum(out, p) if fuse == "max" else np.minimum(out, p)
    return (out * np.float32(1.0 / heads) if fuse == "mean" else out).astype(np.float32)


def step_probs_case(L: int, n: int, kind: str) -> np.ndarray:
    """fp32 [n, L, L]: 'stochastic' rows sum to one (within fp32), 'unnormalised' rows sum to something in [0.5, 1.5) as a max / min fuse
    leaves them"""
    g = _gen("step", L, n, kind)
    p = torch.softmax(2.0 * torch.randn((n, L, L), generator=g, dtype=torch.float64), dim=2)
    if kind == "unnormalised":
        p = p * (0.5 + torch.rand((n, L, 1), generator=g, dtype=torch.float64))
    return p.to(torch.float32).numpy()


def rollout_chain_np(probs_list, residual: float, dtype):
    """[R after step 1, R after step 2, ...] with A^ and the products in `dtype` (np.float64: the statement; np.float32: the bar)"""
    from eoe_amd.explain import rollout_matrix_np
    out, r = [], None
    for p in probs_list:
        a = rollout_matrix_np(p, residual).astype(dtype) if dtype == np.float64 else _matrix32(p, residual)
        r = a if r is None else np.matmul(a, r).astype(dtype)
        out.append(r)
    return out


def _matrix32(p, residual):
    p = np.asarray(p, dtype=np.float32)
    eye = np.eye(p.shape[-1], dtype=np.float32)
    a = np.float32(1.0 - np.float32(residual)) * p + np.float32(residual) * eye
    s = a.sum(axis=-1, keepdims=True, dtype=np.float32)
    ok = np.isfinite(s) & (s != 0)
    return np.where(ok, a / np.where(ok, s, np.float32(1.0)), eye).astype(np.float32)


def step_chain_case(L: int, n: int, kind: str, steps: int = 4):
    return [step_probs_case(L, n, f"{kind}/{i}") if i else step_probs_case(L, n, kind) for i in range(steps)]


# ------------------------------------------------------------------------------------------------ the tower in float64
def round16(x: torch.Tensor, dtype) -> torch.Tensor:
    return x.to(dtype).to(torch.float64)


def tower_rollout_f64(state: dict, images: torch.Tensor, patch: int, heads: int, layers: int, normalize=None, residual: float = 0.5,
                      start_layer: int = 0, fuse: str = "mean", round_qkv=None):
    """Attention rollout of a VisualTransformer restated in float64 torch / numpy from its state_dict (keys under 'feature_model.'):
    returns (maps float64 [n, H, W], [fused probabilities per rolled-out layer]).  `round_qkv`: a 16-bit dtype every layer's qkv is
    rounded to (the emulation behind e2e_bar), or None."""
    from eoe_amd.explain import attention_probs_np, attention_rollout_np
    sd = {k[len("feature_model."):]: v.detach().cpu().double() for k, v in state.items() if k.startswith("feature_model.")}
    x = images.detach().cpu().double()
    if normalize is not None:
        mean, std = (torch.as_tensor(t, dtype=torch.float64).view(1, 3, 1, 1) for t in normalize)
        x = (x - mean) / std
    n, _, res, _ = x.shape
    grid = res // patch
    L = grid * grid + 1
    w = sd["conv1.weight"]
    D = w.shape[0]
    patches = torch.nn.functional.unfold(x, patch, stride=patch).transpose(1, 2)                  # [n, grid^2, 3 p^2], column = c p^2 + ky p + kx
    tok = patches @ w.reshape(D, -1).T
    tok = torch.cat([sd["class_embedding"].expand(n, 1, D), tok], dim=1) + sd["positional_embedding"]

    def ln(t, name):
        return torch.nn.functional.layer_norm(t, (D,), sd[name + ".weight"], sd[name + ".bias"], 1e-5)
    tok = ln(tok, "ln_pre")
    first = start_layer + layers if start_layer < 0 else start_layer
    probs = []
    for i in range(layers):
        pre = f"transformer.resblocks.{i}."
        qkv = ln(tok, pre + "ln_1") @ sd[pre + "attn.in_proj_weight"].T + sd[pre + "attn.in_proj_bias"]
        if round_qkv is not None:
            qkv = round16(qkv, round_qkv)
        if i >= first:
            probs.append(attention_probs_np(qkv.reshape(n * L, 3 * D).numpy(), n, L, heads, fuse))
        if i + 1 < layers:
            q, k, v = (t.reshape(n, L, heads, 64).transpose(1, 2) for t in qkv.split(D, dim=2))
            att = torch.softmax(q @ k.transpose(2, 3) / 8.0, dim=3) @ v
            att = att.transpose(1, 2).reshape(n, L, D)
            tok = tok + att @ sd[pre + "attn.out_proj.weight"].T + sd[pre + "attn.out_proj.bias"]
            h = ln(tok, pre + "ln_2") @ sd[pre + "mlp.c_fc.weight"].T + sd[pre + "mlp.c_fc.bias"]
            h = h * torch.sigmoid(1.702 * h)                                                    # QuickGELU
            tok = tok + h @ sd[pre + "mlp.c_proj.weight"].T + sd[pre + "mlp.c_proj.bias"]
    return attention_rollout_np(probs, residual, grid, patch), probs


TOWERS = {
    # name: (constructor keywords, resolution, patch, heads)
    "b32": (dict(layers=2), 224, 32, 12),                                                          # 50 tokens: the short kernels
    "narrow65": (dict(patch_size=4, width=64, input_resolution=32, layers=2, output_dim=32), 32, 4, 1),   # 65 tokens, 1 head: the long path
}


def tower_images(name: str, n: int = 4) -> torch.Tensor:
    res = TOWERS[name][1]
    return torch.rand((n, 3, res, res), generator=_gen("images", name, n))
