"""CPU checks of the CLIP drop-in (eoe_amd.models.CLIP / build_model) and of ADClipTrainer's prompts: parameter names and shapes
against the reference's own list (fixture g19, tests/golden/make_golden_clip_text.py), strict state-dict loads, the dimensions
build_model infers, the prompts of clip.py:51-57, and the errors of what is not built."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G19 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_clip_text.npz")


def _g19():
    return np.load(G19)


def _names_shapes(g, cfg):
    return [(str(n), tuple(int(d) for d in s.split(",") if d)) for n, s in zip(g[f"{cfg}/names"], g[f"{cfg}/shapes"])]


def _model(cfg):
    from eoe_amd.models import CLIP
    torch.manual_seed(0)
    return CLIP(*[int(d) for d in _g19()[f"{cfg}/dims"]])


def _ref_state_dict(cfg):
    """a state dict in the reference's format: its names and shapes, deterministic values, the build_model-dropped extra keys"""
    g = _g19()
    sd = {n: torch.from_numpy(np.full(s, 0.01 * (i % 7 + 1), dtype=np.float32)) for i, (n, s) in enumerate(_names_shapes(g, cfg))}
    dims = [int(d) for d in g[f"{cfg}/dims"]]
    sd["input_resolution"], sd["context_length"], sd["vocab_size"] = torch.tensor(dims[1]), torch.tensor(dims[5]), torch.tensor(dims[6])
    return sd


@pytest.mark.parametrize("cfg", ["small", "b32"])
def test_parameter_names_and_shapes_match_reference(cfg):
    m = _model(cfg)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _names_shapes(_g19(), cfg)


def test_reference_state_dict_loads_strictly():
    sd = _ref_state_dict("small")
    for k in ("input_resolution", "context_length", "vocab_size"):
        del sd[k]
    m = _model("small")
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.token_embedding.weight, sd["token_embedding.weight"])
    assert torch.equal(m.transformer.resblocks[1].attn.in_proj_weight, sd["transformer.resblocks.1.attn.in_proj_weight"])


@pytest.mark.parametrize("cfg", ["small", "b32"])
def test_build_model_infers_dimensions(cfg):
    from eoe_amd.models import build_model
    g = _g19()
    sd = _ref_state_dict(cfg)
    m = build_model(sd)
    assert "input_resolution" not in sd and "context_length" not in sd and "vocab_size" not in sd      # dropped, as model.py:426-428
    embed, res, vl, vw, vp, ctx, vocab, width, heads, layers = [int(d) for d in g[f"{cfg}/dims"]]
    assert m.context_length == ctx and m.vocab_size == vocab and m.transformer.width == width and m.transformer.layers == layers
    assert m.visual.input_resolution == res and m.visual.patch_size == vp and m.visual.output_dim == embed
    assert len(m.visual.transformer.resblocks) == vl and m.visual.conv1.weight.shape[0] == vw
    assert m.transformer.resblocks[0].n_head == heads and not m.training
    assert all(p.dtype == torch.float32 for p in m.parameters())                 # fp32 masters
    assert torch.equal(m.ln_final.weight, sd["ln_final.weight"])


def test_initialize_parameters_matches_reference_scales():
    m = _model("small")
    w = m.transformer.width
    assert abs(m.token_embedding.weight.std().item() - 0.02) < 2e-3
    assert abs(m.transformer.resblocks[0].attn.in_proj_weight.std().item() - w ** -0.5) < 0.1 * w ** -0.5
    assert abs(m.logit_scale.item() - np.log(1 / 0.07)) < 1e-6
    mask = m.build_attention_mask()
    assert mask.shape == (77, 77) and mask[0, 1] == float("-inf") and mask[1, 0] == 0 and mask[5, 5] == 0


def test_not_built_paths_raise():
    from eoe_amd.models import CLIP, ResidualAttentionBlock, build_model
    with pytest.raises(NotImplementedError):
        CLIP(1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12)
    with pytest.raises(NotImplementedError):
        build_model({"visual.layer1.0.conv1.weight": torch.zeros(64, 64, 1, 1)})
    bad = torch.full((77, 77), float("-inf")).triu_(2)           # not the causal mask
    with pytest.raises(NotImplementedError):
        ResidualAttentionBlock(128, 2, bad)
    with pytest.raises(NotImplementedError):
        ResidualAttentionBlock(128, 2, torch.zeros(77, 77))
    blk = ResidualAttentionBlock(128, 2, torch.full((77, 77), float("-inf")).triu_(1))
    assert blk.causal


def test_token_ids_checked_before_any_device_work():
    m = _model("small")
    ok = torch.zeros(2, 77, dtype=torch.int64)
    with torch.no_grad():
        for bad in (torch.full((2, 77), 1000, dtype=torch.int64), torch.full((2, 77), -1, dtype=torch.int32)):
            with pytest.raises(ValueError):
                m.encode_text(bad)
        with pytest.raises(ValueError):
            m.encode_text(ok.float())
        with pytest.raises(RuntimeError):                # a CPU model: no CPU path
            m.encode_text(ok)


@pytest.mark.parametrize("ad_mode", ["one_vs_rest", "leave_one_out"])
def test_prompts_match_reference(ad_mode):
    from eoe_amd.training import TRAINER
    classes = ["airplane", "automobile", "bird", "cat"]
    for anom in ("a photo of something", "a photo of something that is not a {}"):
        tr = TRAINER["clip"](_model("small"), dataset=None, classes=classes, ad_mode=ad_mode, anom_tkn_ptn=anom, device="cpu")
        for cstr in classes:
            # clip.py:51-55
            if ad_mode == "one_vs_rest":
                want = [f"a photo of a {cstr}", anom.format(cstr)]
            else:
                want = [*[f"a photo of a {cs}" for cs in classes if cs != cstr], anom.format(cstr)]
            assert tr.prompts(cstr) == want


def test_prepare_metric_without_features_or_tokenizer_raises():
    from eoe_amd.training import TRAINER
    tr = TRAINER["clip"](_model("small"), dataset=None, classes=["a", "b"], device="cpu")
    with pytest.raises(RuntimeError, match="tokenizer="):
        tr.prepare_metric("a", None, tr.model, 0)


def test_fresh_model_keeps_clip_weights():
    from eoe_amd.training import TRAINER
    m = _model("small")
    tr = TRAINER["clip"](m, dataset=None, classes=["a", "b"], device="cpu")
    fresh = tr._fresh_model(None)
    assert fresh is not tr.model
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), fresh.state_dict().items()):
        assert torch.equal(a, b), k
    assert all(p.requires_grad and p.is_leaf for p in fresh.parameters())
