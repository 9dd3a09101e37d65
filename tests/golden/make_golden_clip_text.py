"""Generates tests/golden/g19_clip_text.npz by running the REFERENCE's own `CLIP.encode_text` (`clip_official/clip/model.py:343-356`)
in fp64 on the CPU.  Run by hand where the reference is available (`python make_golden_clip_text.py <reference checkout>`); the tests
only read the .npz.  `model.py` needs torch alone; the
reference tokenizer (`simple_tokenizer.py`) imports ftfy, which is absent, so `ftfy.fix_text` is stubbed as the identity (exact for
the ASCII prompts below), and its LayerNorm runs in the input's dtype instead of casting to fp32.

Weights: `weights(cfg, names_shapes)` below, oracle.fill values keyed by parameter name with oracle.models.init_std at the TEXT
tower's width and depth -- a pure function of its arguments that tests/test_gpu_clip_text.py restates, so the fixture stores no
weights.  Stored per config ("small", "b32"): the token ids, the fp64 text features and their l2-normalised rows, and the
(name, shape) list of the reference's `CLIP.state_dict()`."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.fill import fill, fill_int   # noqa: E402
from oracle.models import init_std   # noqa: E402

REF_SUBDIR = os.path.join("src", "eoe", "models", "clip_official", "clip")
# embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size, width, heads, layers
CONFIGS = {"small": (64, 32, 2, 256, 8, 77, 1000, 128, 2, 2),
           "b32": (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12)}
PROMPTS = ["a photo of a airplane", "a photo of something", "a photo of a automobile", "a photo of a bird",
           "a photo of something that is not a ship"]


def weights(cfg: str, names_shapes):
    """{name: fp32 array} for the text-tower parameters (everything but visual.*)"""
    width, layers = CONFIGS[cfg][7], CONFIGS[cfg][9]
    out = {}
    for name, shape in names_shapes:
        if name.startswith("visual."):
            continue
        std = init_std(name, tuple(shape), width, layers)
        out[name] = fill(f"g19/{cfg}/{name}", tuple(shape), std=std, mean=1.0 if "ln_" in name and name.endswith("weight") else 0.0)
    return out


def synthetic_tokens(cfg: str) -> np.ndarray:
    """[SOT, ids..., EOT, 0...] rows: the shortest sequence, a full one (EOT at 76), a repeated maximum id before the EOT position
    (pins the first-occurrence argmax), and three of random lengths"""
    ctx, vocab = CONFIGS[cfg][5], CONFIGS[cfg][6]
    sot, eot = vocab - 2, vocab - 1
    rows = []

    def row(body):
        r = np.zeros(ctx, dtype=np.int64)
        seq = [sot] + list(body) + [eot]
        r[:len(seq)] = seq
        return r

    rows.append(row([]))
    rows.append(row(fill_int(f"g19/{cfg}/full", (ctx - 2,), 1, vocab - 2)))
    r = row(fill_int(f"g19/{cfg}/rep", (20,), 1, vocab - 2))
    r[7] = eot                                   # two EOT ids: the first (position 7) is the one read
    rows.append(r)
    for i, n in enumerate((3, 17, 40)):
        rows.append(row(fill_int(f"g19/{cfg}/len{i}", (n,), 1, vocab - 2)))
    return np.stack(rows)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_root: str):
    REF = os.path.join(ref_root, REF_SUBDIR)
    m = types.ModuleType("ftfy")
    m.fix_text = lambda s: s
    sys.modules["ftfy"] = m
    model = _load("ref_clip_model", os.path.join(REF, "model.py"))
    # the reference's LayerNorm casts its input to fp32 (for fp16 towers, model.py:153-159); in fp64 it is torch's LayerNorm as is
    model.LayerNorm.forward = lambda self, x: torch.nn.LayerNorm.forward(self, x)
    tok_mod = _load("ref_simple_tokenizer", os.path.join(REF, "simple_tokenizer.py"))
    tokenizer = tok_mod.SimpleTokenizer(os.path.join(REF, "bpe_simple_vocab_16e6.txt.gz"))
    out = {}
    for cfg, dims in CONFIGS.items():
        torch.manual_seed(0)
        ref = model.CLIP(*dims)
        names_shapes = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        w = weights(cfg, names_shapes)
        with torch.no_grad():
            for name, p in ref.named_parameters():
                if name in w:
                    p.copy_(torch.from_numpy(w[name]))
        ref = ref.double().eval()
        toks = synthetic_tokens(cfg)
        if cfg == "b32":
            sot, eot = tokenizer.encoder["<|startoftext|>"], tokenizer.encoder["<|endoftext|>"]
            assert (sot, eot) == (dims[6] - 2, dims[6] - 1)
            real = np.zeros((len(PROMPTS), dims[5]), dtype=np.int64)
            for i, p in enumerate(PROMPTS):                     # clip.py:187-197 (tokenize)
                ids = [sot] + tokenizer.encode(p) + [eot]
                real[i, :len(ids)] = ids
            toks = np.concatenate([toks, real])
            out["b32/prompts"] = np.array(PROMPTS)
        with torch.no_grad():
            f = ref.encode_text(torch.from_numpy(toks)).numpy()
        out[f"{cfg}/tokens"] = toks
        out[f"{cfg}/features"] = f
        out[f"{cfg}/features_normed"] = f / np.linalg.norm(f, axis=-1, keepdims=True)
        out[f"{cfg}/names"] = np.array([n for n, _ in names_shapes])
        out[f"{cfg}/shapes"] = np.array([",".join(str(d) for d in s) for _, s in names_shapes])
        out[f"{cfg}/dims"] = np.array(dims, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "g19_clip_text.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
