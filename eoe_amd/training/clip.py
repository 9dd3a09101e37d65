"""CLIP text-prompt objective, `src/eoe/training/clip.py:13-103` on fused HIP kernels.

The reference's `prepare_metric` (clip.py:50-64) builds two (one_vs_rest) or C (leave_one_out) prompts, tokenises them and runs them
through CLIP's *text* tower once per (class, seed).  Here the frozen text features come either from the caller -- `text_features` is
a tensor [T, d] or a callable `(cstr, ad_mode) -> tensor` -- or, for an `eoe_amd.models.CLIP` model and a `tokenizer` (OpenAI's
`clip.tokenize`: str -> int tensor [1, context_length]; the package ships no BPE vocabulary), from the prompts themselves through the
model's HIP text tower (`CLIP.encode_text`).  Either way they are l2-normalised exactly as clip.py:62.  Everything the training loop
does with them -- the loss, the anomaly score, SGD with Nesterov momentum for the image tower (ad_trainer.py:380-381) -- runs on the
GPU kernels (`eoe_clip_fwd/bwd/score`, `eoe_sgd_multi`); the text tower gets no gradients, so the optimiser leaves it untouched."""
from copy import deepcopy

import torch

from .. import ops
from ..optim import FusedSGD
from .ad_trainer import ADTrainer


class ADClipTrainer(ADTrainer):
    def __init__(self, model, *args, text_features=None, fp16_weights=False, anom_tkn_ptn="a photo of something", tokenizer=None, **kwargs):
        """fp16_weights: the reference's CLIP towers carry fp16 convolution / linear / attention / projection parameters on a GPU
        (`convert_weights`, clip/model.py:371-392, applied by build_model :430; `clip.load` undoes it on the CPU only) and SGD updates those
        fp16 tensors; True reproduces that arithmetic (`eoe_amd.models.convert_weights` on the image tower + `eoe_sgd_multi`'s fp16 path).
        The default keeps fp32 masters, which is what the reference gets on a CPU and is strictly more accurate.
        anom_tkn_ptn: the anomalous class's prompt, `{}` is replaced by the normal class's name (clip.py:16,51-55).
        tokenizer: str -> int tensor [1, context_length] (clip.tokenize); with a CLIP model and no text_features, prepare_metric encodes
        the prompts with the model's own text tower."""
        super().__init__(model, *args, **kwargs)
        self.text_features = text_features
        self.fp16_weights = bool(fp16_weights)
        self.anom_tkn_ptn = anom_tkn_ptn
        self.tokenizer = tokenizer
        self.raw_texts = None

    def make_optimizer(self, model):
        # ad_trainer.py:380-381: CLIP models are trained with SGD(momentum 0.9, nesterov)
        if self.fp16_weights:
            from ..models import convert_weights
            convert_weights(getattr(model, "feature_model", model))          # the CLIP tower; a CustomNet head is created in fp32
        return FusedSGD(model.parameters(), lr=self.lr, weight_decay=self.wdk, momentum=0.9, nesterov=True)

    def _fresh_model(self, preset):
        # ad_trainer.py:237-239: a CLIP model starts every (class, seed) run from its (pretrained) weights, not re-initialised ones
        from ..models import CLIP
        if not isinstance(preset, torch.nn.Module) and isinstance(self.model, CLIP):
            model = deepcopy(self.model)
            for p in model.parameters():
                p.detach_().requires_grad_()
            return model
        return super()._fresh_model(preset)

    def prompts(self, cstr):
        """the prompts of clip.py:51-57: the normal class(es) as "a photo of a {name}", then the anomalous prompt"""
        if self.ad_mode == "one_vs_rest":
            return [f"a photo of a {cstr}", self.anom_tkn_ptn.format(cstr)]
        if self.ad_mode == "leave_one_out":
            return [*[f"a photo of a {cs}" for cs in self.classes if cs != cstr], self.anom_tkn_ptn.format(cstr)]
        raise NotImplementedError()

    def prepare_metric(self, cstr, loader, model, seed, **kwargs):
        t = self.text_features(cstr, self.ad_mode) if callable(self.text_features) else self.text_features
        if t is None and self.tokenizer is not None and hasattr(model, "encode_text"):
            self.raw_texts = self.prompts(cstr)
            tokens = torch.cat([self.tokenizer(tk) for tk in self.raw_texts])                      # clip.py:59
            with torch.no_grad():
                t = model.encode_text(tokens)                                                      # clip.py:60-61
        if t is None:
            raise RuntimeError("ADClipTrainer needs the frozen text features of the prompts (clip.py:50-64): pass text_features=, "
                               "or train an eoe_amd.models.CLIP model and pass tokenizer= (e.g. clip.tokenize) to encode them")
        t = torch.as_tensor(t, dtype=torch.float32).to(self.device)
        expect = 2 if self.ad_mode == "one_vs_rest" else None
        if t.dim() != 2 or (expect is not None and t.shape[0] != expect):
            raise ValueError(f"text_features must be [T, d] (T = 2 for one_vs_rest), got {tuple(t.shape)}")
        return t / t.norm(dim=-1, keepdim=True)                              # clip.py:62

    def compute_anomaly_score(self, features, center, train=False, **kwargs):
        return ops.clip_score(features, center)                               # clip.py:66-79

    def loss(self, features, labels, center, **kwargs):
        return ops.clip_loss(features, labels, center, kwargs.get("nominal_label", 0), self.ad_mode == "leave_one_out",
                             kwargs.get("inv_count", None))                   # clip.py:81-103
