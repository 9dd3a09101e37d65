"""Times CLIP's text tower (CLIP.encode_text: one eoe_clip_text_fwd call) against a stock-torch fp16 composition of the same tower
(nn.MultiheadAttention with the causal mask, nn.LayerNorm in fp32 as model.py:153-159, QuickGELU, fp16 linear layers) in the ViT-B/32
text configuration (width 512, 8 heads, 12 layers, 77 tokens, vocab 49408) at T in {2, 10, 30} prompts -- one_vs_rest, CIFAR-10 and
ImageNet-30 leave_one_out.  The tower runs once per (class, seed), so the question is only whether it is slower than torch.

Median of --repeats windows of >= --window seconds of back-to-back calls timed with device events (ms per call), the two sides
alternated; also the rel RMS of the two results against each other.  One JSON line per T.

  python tools/clip_text_bench.py [--repeats 5] [--window 0.5] [--dtype fp16]"""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402
from torch import nn  # noqa: E402

import eoe_amd       # noqa: E402
from eoe_amd.models import CLIP   # noqa: E402


def window_ms(fn, window_s):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        total = start.elapsed_time(end)
        if total >= window_s * 1e3:
            return total / n
        n = max(n * 2, int(n * 1.2 * window_s * 1e3 / max(total, 1e-3)))


class TorchTower(nn.Module):
    """the reference's text tower (model.py:167-199,343-356) in stock torch, fp16 weights, from a CLIP's parameters"""

    def __init__(self, m: CLIP):
        super().__init__()
        D, heads = m.transformer.width, m.transformer.width // 64
        self.blocks = nn.ModuleList()
        for b in m.transformer.resblocks:
            mha = nn.MultiheadAttention(D, heads)
            mha.in_proj_weight.data.copy_(b.attn.in_proj_weight.data)
            mha.in_proj_bias.data.copy_(b.attn.in_proj_bias.data)
            mha.out_proj.load_state_dict(b.attn.out_proj.state_dict())
            blk = nn.ModuleDict({"attn": mha, "ln_1": copy.deepcopy(b.ln_1), "ln_2": copy.deepcopy(b.ln_2),
                                 "c_fc": copy.deepcopy(b.mlp.c_fc), "c_proj": copy.deepcopy(b.mlp.c_proj)})
            self.blocks.append(blk)
        self.tok = copy.deepcopy(m.token_embedding)
        self.pos = nn.Parameter(m.positional_embedding.data.clone())
        self.ln_final = copy.deepcopy(m.ln_final)
        self.proj = nn.Parameter(m.text_projection.data.clone())
        self.mask = m.build_attention_mask()

    def half_weights(self):
        for blk in self.blocks:
            for k in ("attn", "c_fc", "c_proj"):
                blk[k].half()
        self.proj.data = self.proj.data.half()
        self.mask = self.mask.half().to(self.proj.device)
        return self

    @staticmethod
    def ln(mod, x):
        return mod(x.float()).half()

    def forward(self, text):
        x = self.tok(text).half() + self.pos.half()
        x = x.permute(1, 0, 2)
        for b in self.blocks:
            x = x + b["attn"](*([self.ln(b["ln_1"], x)] * 3), need_weights=False, attn_mask=self.mask)[0]
            h = b["c_fc"](self.ln(b["ln_2"], x))
            x = x + b["c_proj"](h * torch.sigmoid(1.702 * h))
        x = self.ln(self.ln_final, x.permute(1, 0, 2))
        return x[torch.arange(x.shape[0]), text.argmax(dim=-1)] @ self.proj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--dtype", default="fp16")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    eoe_amd.set_compute_dtype(a.dtype)
    torch.manual_seed(0)
    m = CLIP(512, 32, 1, 256, 8, 77, 49408, 512, 8, 12).cuda().eval()      # (a small image tower: only the text side is timed)
    ref = TorchTower(m).cuda().eval().half_weights()
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for T in (2, 10, 30):
            toks = torch.zeros(T, 77, dtype=torch.int64)
            for i in range(T):
                n = int(rng.integers(4, 12))
                toks[i, : n + 2] = torch.tensor([49406] + list(rng.integers(1, 49406, n)) + [49407])
            toks = toks.cuda()
            hip = lambda: m.encode_text(toks)          # noqa: E731
            stock = lambda: ref(toks)                  # noqa: E731
            y, r = hip().double(), stock().double()
            rel = float(((y - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item())
            for _ in range(3):
                hip(), stock()
            th, ts = [], []
            for _ in range(a.repeats):
                th.append(window_ms(hip, a.window))
                ts.append(window_ms(stock, a.window))
            print(json.dumps({"prompts": T, "tokens": 77, "config": "ViT-B/32 text", "dtype": a.dtype,
                              "hip_ms": float(np.median(th)), "torch_fp16_ms": float(np.median(ts)),
                              "speedup": float(np.median(ts) / np.median(th)), "rel_rms_vs_torch": rel,
                              "hip_ms_all": [round(v, 4) for v in th], "torch_ms_all": [round(v, 4) for v in ts]}), flush=True)


if __name__ == "__main__":
    main()
