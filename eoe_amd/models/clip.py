"""Drop-in for the reference's vendored CLIP model (`src/eoe/models/clip_official/clip/model.py`): `CLIP` (:239-368) and `build_model`
(:395-432), ViT image tower only.

Same constructor signature, same parameter names and shapes (a reference `CLIP.state_dict()` loads with strict=True) and the same
`initialize_parameters`.  `visual` is the fused `VisualTransformer`; the text tower (`transformer` with the causal mask,
`token_embedding`, `positional_embedding`, `ln_final`, `text_projection`) runs forward-only as one C call (`eoe_clip_text_fwd`): the
reference encodes its prompts once per run under no_grad (training/clip.py:59-61).
"""
import numpy as np
import torch
from torch import nn

from .. import ops
from .clip_vit import Transformer, VisualTransformer


class CLIP(nn.Module):
    def __init__(self, embed_dim: int,
                 # vision
                 image_resolution: int, vision_layers, vision_width: int, vision_patch_size: int,
                 # text
                 context_length: int, vocab_size: int, transformer_width: int, transformer_heads: int, transformer_layers: int):
        super().__init__()
        self.context_length = context_length
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("the ModifiedResNet image tower (RN50-style CLIP, tuple vision_layers) is not built; ViT only")
        self.visual = VisualTransformer(input_resolution=image_resolution, patch_size=vision_patch_size, width=vision_width,
                                        layers=vision_layers, heads=vision_width // 64, output_dim=embed_dim)
        self.transformer = Transformer(width=transformer_width, layers=transformer_layers, heads=transformer_heads,
                                       attn_mask=self.build_attention_mask())
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(self.context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.initialize_parameters()

    def initialize_parameters(self):
        # model.py:296-319 (the ModifiedResNet branch does not apply)
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std = (self.transformer.width ** -0.5) * ((2 * self.transformer.layers) ** -0.5)
        attn_std = self.transformer.width ** -0.5
        fc_std = (2 * self.transformer.width) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        if self.text_projection is not None:
            nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    def build_attention_mask(self):
        # model.py:321-327: additive causal mask, -inf strictly above the diagonal
        mask = torch.empty(self.context_length, self.context_length)
        mask.fill_(float("-inf"))
        mask.triu_(1)
        return mask

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def set_normalize(self, mean, std):
        """the trainer's per-channel Normalize, fused into the image tower's first kernel (VisualTransformer.set_normalize)"""
        self.visual.set_normalize(mean, std)

    def text_parameters(self):
        """the parameters encode_text reads (everything but `visual` and `logit_scale`)"""
        return [p for name, p in self.named_parameters() if not name.startswith("visual.") and name != "logit_scale"]

    def encode_image(self, image):
        return self.visual(image)

    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        """model.py:343-356: tokens [n, context_length] (int64 as clip.tokenize returns them, or int32) -> fp32 features [n, embed_dim].
        Forward only: with grad mode on and a text-tower parameter that requires grad this raises instead of returning a tensor that
        silently carries no gradient."""
        ops.check_token_ids(text, self.vocab_size)
        if not self.token_embedding.weight.is_cuda:
            raise RuntimeError("eoe_amd.CLIP.encode_text runs on the GPU only (no CPU fallback)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.text_parameters()):
            raise RuntimeError("eoe_amd.CLIP.encode_text is forward only (the text tower has no backward kernels): "
                               "call it under torch.no_grad()")
        return ops.clip_text_fwd(text, list(self.transformer.resblocks), self.transformer.width // 64, self.token_embedding.weight,
                                 self.positional_embedding, self.ln_final, self.text_projection)

    def forward(self, image, text=None):
        """model.py:358-368 with a text; image features alone without one -- what the reference's CLIP-AD trainer makes of the model
        (`model.forward = model.encode_image`, training/clip.py:33)"""
        image_features = self.encode_image(image)
        if text is None:
            return image_features
        text_features = self.encode_text(text)
        image_features = image_features / image_features.norm(dim=-1, keepdim=True)
        text_features = text_features / text_features.norm(dim=-1, keepdim=True)
        logit_scale = self.logit_scale.exp()
        logits_per_image = logit_scale * image_features @ text_features.t()
        logits_per_text = logits_per_image.t()
        return logits_per_image, logits_per_text


def build_model(state_dict: dict) -> CLIP:
    """model.py:395-432: the dimensions from the state dict, then a strict load.  The masters stay fp32 (the reference's
    `convert_weights` fp16 storage is `eoe_amd.models.convert_weights` / ADClipTrainer(fp16_weights=True)).  Like the reference, the
    `input_resolution` / `context_length` / `vocab_size` entries are removed from `state_dict`."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("the ModifiedResNet image tower (RN50-style CLIP) is not built; ViT only")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict.keys() if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    image_resolution = vision_patch_size * grid_size
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_heads = transformer_width // 64
    transformer_layers = len(set(k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")))
    model = CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_heads, transformer_layers)
    for key in ["input_resolution", "context_length", "vocab_size"]:
        if key in state_dict:
            del state_dict[key]
    model.load_state_dict({k: v.float() if torch.is_tensor(v) and v.is_floating_point() else v for k, v in state_dict.items()})
    return model.eval()
