"""GPU tier: CLIP's text tower (csrc/clip_text.hip, csrc/clip_text_driver.cpp).  The causal attention kernel against an fp64 torch
restatement (incl. causality to the bit and no stores behind the last row), CLIP.encode_text against the g19 fixture (the reference's
own encode_text in fp64, tests/golden/make_golden_clip_text.py), and ADClipTrainer encoding its own prompts end to end."""
import importlib.util
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gpu_util import DTYPES, EPS16, rel_rms   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(HERE, "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_clip_text", os.path.join(GOLDEN_DIR, "make_golden_clip_text.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _g19():
    return np.load(os.path.join(GOLDEN_DIR, "g19_clip_text.npz"))


@pytest.fixture
def compute_dtype():
    import eoe_amd
    prev = eoe_amd.ops.compute_dtype()
    yield lambda dt: eoe_amd.set_compute_dtype(dt)
    eoe_amd.set_compute_dtype(prev)


def _attn_ref(qkv, n, L, heads):
    """fp64 restatement: softmax(q k^T / 8 + causal mask) v per (sequence, head)"""
    D = heads * 64
    x = qkv.double().cpu().reshape(n, L, 3, heads, 64).permute(2, 0, 3, 1, 4)      # [3, n, heads, L, 64]
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) / 8.0
    s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    o = torch.softmax(s, dim=-1) @ v                                                # [n, heads, L, 64]
    return o.permute(0, 2, 1, 3).reshape(n * L, D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 77, 128])
def test_attn_causal_matches_fp64_and_is_causal(dtype, heads, L):
    from eoe_amd import ops
    n, D, extra = 3, heads * 64, 5
    g = torch.Generator().manual_seed(1000 * L + heads)
    qkv = (torch.randn(n * L, 3 * D, generator=g) * 1.5).to(dtype).cuda()
    # the output lives in a larger buffer: rows behind n * L must keep their sentinel
    buf = torch.full(((n * L + extra), D), 7.0, dtype=dtype, device="cuda")
    out = buf[: n * L]
    ops.attn_causal_fwd(qkv, out, n, L, heads)
    torch.cuda.synchronize()
    assert torch.equal(buf[n * L:].float().cpu(), torch.full((extra, D), 7.0)), "stores behind the last row"
    ref = _attn_ref(qkv, n, L, heads)
    err = (out.double().cpu() - ref).abs().max().item()
    vmax = qkv[:, 2 * D:].float().abs().max().item()
    assert err <= 6 * EPS16[dtype] * vmax, (err, vmax)
    # keys / values j > i do not reach query i: changing them leaves rows <= i bit-identical
    for i in sorted({0, L // 2, L - 2}):
        if not 0 <= i < L - 1:
            continue
        qkv2 = qkv.clone().reshape(n, L, 3 * D)
        qkv2[:, i + 1:, D:] = (torch.randn(n, L - i - 1, 2 * D, generator=g) * 3).to(dtype).cuda()
        out2 = torch.empty_like(out)
        ops.attn_causal_fwd(qkv2.reshape(n * L, 3 * D), out2, n, L, heads)
        a, b = out.reshape(n, L, D)[:, : i + 1], out2.reshape(n, L, D)[:, : i + 1]
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (L, heads, i)


def _clip_with_g19_weights(cfg):
    from eoe_amd.models import CLIP
    gen, g = _gen(), _g19()
    torch.manual_seed(0)
    m = CLIP(*[int(d) for d in g[f"{cfg}/dims"]])
    names_shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    w = gen.weights(cfg, names_shapes)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name in w:
                p.copy_(torch.from_numpy(w[name]))
    return m.cuda().eval()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", ["small", "b32"])
def test_encode_text_matches_reference(cfg, dtype, compute_dtype):
    from eoe_amd import ops
    compute_dtype(dtype)
    g = _g19()
    m = _clip_with_g19_weights(cfg)
    toks = torch.from_numpy(g[f"{cfg}/tokens"])
    want = torch.from_numpy(g[f"{cfg}/features"])
    with torch.no_grad():
        got = m.encode_text(toks)
        got32 = m.encode_text(toks.to(torch.int32).cuda())          # int32 ids on the device: the same features
    torch.cuda.synchronize()
    assert torch.equal(got, got32)
    assert torch.isfinite(got).all()
    r = rel_rms(got, want)
    # the one_vs_rest score of fixed image features against [normal prompt, anomalous prompt]
    pair = [int(len(toks)) - 5, int(len(toks)) - 4] if cfg == "b32" else [0, 1]
    E = want.shape[1]
    img = torch.randn(256, E, generator=torch.Generator().manual_seed(5))
    img = img + 4.0 * torch.from_numpy(g[f"{cfg}/features_normed"][pair[0]]).float() * torch.linspace(-1, 1, 256)[:, None] * E ** 0.5 / 8
    s_dev = ops.clip_score(img.cuda(), got[pair]).cpu()
    s_ref = ops.clip_score(img.cuda(), torch.from_numpy(g[f"{cfg}/features_normed"][pair]).float().cuda()).cpu()
    ds = (s_dev - s_ref).abs().max().item()
    print(f"\n[clip_text parity] cfg={cfg} dtype={dtype}: rel RMS {r:.3e} (= {r / EPS16[dtype]:.2f} EPS16), "
          f"max |d clip_score| {ds:.3e} (score spread {s_ref.min().item():.3f}..{s_ref.max().item():.3f})")
    # measured on one MI355X: rel RMS 1.5 / 1.8 EPS16 (small / b32, both dtypes); |d clip_score| 3.9e-3 / 2.0e-3 (fp16) and 4.3e-2 /
    # 1.9e-2 (bf16) -- the score is a softmax of 100 x cosine and these image features put samples on its steep part (slope up to 25 per
    # unit of cosine), so a 1e-3 cosine error moves a score by up to 2.5e-2.  Bars: about twice the measured values.
    assert r <= 5 * EPS16[dtype], r
    assert ds <= (8e-3 if dtype == torch.float16 else 8e-2), ds


def test_encode_text_refuses_grad_mode():
    g = _g19()
    m = _clip_with_g19_weights("small")
    toks = torch.from_numpy(g["small/tokens"])
    with pytest.raises(RuntimeError, match="no_grad"):
        m.encode_text(toks)
    for p in m.text_parameters():
        p.requires_grad_(False)
    assert m.encode_text(toks).shape == (len(toks), 64)             # nothing to differentiate: runs


def _fake_tokenizer(vocab=1000, ctx=77):
    """clip.tokenize's contract (str -> int64 [1, ctx], [SOT, ids..., EOT, 0...]) with a deterministic word hash"""
    def tok(text):
        ids = [vocab - 2] + [1 + zlib.crc32(w.encode()) % (vocab - 3) for w in text.split()] + [vocab - 1]
        out = torch.zeros(1, ctx, dtype=torch.int64)
        out[0, :len(ids)] = torch.tensor(ids)
        return out
    return tok


@pytest.mark.parametrize("ad_mode", ["one_vs_rest", "leave_one_out"])
def test_clip_trainer_encodes_its_prompts(ad_mode, monkeypatch):
    from eoe_amd.data import SyntheticAD
    from eoe_amd.models import CLIP
    from eoe_amd.training import TRAINER, ADTrainer
    monkeypatch.setattr(ADTrainer, "KEEP_SNAPSHOT_IN_RAM", True)
    torch.manual_seed(0)
    # visual: 32^2 input, patch 8, width 256, 2 layers; text: the g19 "small" configuration
    model = CLIP(64, 32, 2, 256, 8, 77, 1000, 128, 2, 2)
    master = {k: v.clone() for k, v in model.state_dict().items()}
    ds = SyntheticAD(n_train_normal=64, n_oe=64, n_test=64, res=32, shift=1.0, seed=1)
    tok = _fake_tokenizer()
    classes = ["0", "1", "2"] if ad_mode == "leave_one_out" else None
    tr = TRAINER["clip"](model, dataset=ds, epochs=2, lr=1e-3, batch_size=32, tokenizer=tok, ad_mode=ad_mode,
                         **({"classes": classes} if classes else {}))
    models, res = tr.run(run_classes=[0])
    trained = models[0][0]
    assert trained is not None and np.isfinite(tr.last_losses).all() and np.isfinite(res["mean_auc"])
    assert tr.raw_texts == tr.prompts(tr.classes[0])
    # the center is the normalised text features of those prompts, encoded by the model itself
    trained = trained.cuda()
    with torch.no_grad():
        t = trained.encode_text(torch.cat([tok(s) for s in tr.raw_texts]))
    t = t / t.norm(dim=-1, keepdim=True)
    assert torch.equal(tr.center, t)
    # the text tower is left alone by training; the image tower moved
    sd = trained.state_dict()
    moved = []
    for k, v in sd.items():
        if k.startswith("visual."):
            moved.append(not torch.equal(v.cpu(), master[k]))
        else:
            assert torch.equal(v.cpu(), master[k]), k
    assert any(moved)
