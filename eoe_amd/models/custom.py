"""CustomNet subclasses, discoverable the way `src/eoe/main/train_only_custom.py:23-26` discovers them
(`inspect.getmembers` on a `models.custom` module; ctor `(prediction_head, clf, freeze)` as `custom.py:6-8`).

The reference ships no CLIP CustomNet; "CLIP ViT-B/32 frozen encoder + HSC head" and "full fine-tune, BCE"
(BASELINE.json configs 4/5) are only expressible through this API."""
from .custom_base import CustomNet
from .clip_vit import VisualTransformer
from .resnet import WideResNet


class ClipViTB32Custom(CustomNet):
    """feature_model = CLIP ViT-B/32 image tower (224, patch 32, width 768, 12 layers, 12 heads, 512-d) by default; `patch_size`, `width`
    and `output_dim` give the other ViT towers of CLIP (ViT-B/16: patch_size=16; heads = width / 64) and the narrow towers trained from
    scratch on small images (ViT-Ti: width=192, ViT-S: width=384; any multiple of 64 up to 1024), within clip_vit.check_vit_geometry"""

    def __init__(self, prediction_head: bool = True, clf: bool = False, freeze: bool = False, layers: int = 12,
                 input_resolution: int = 224, patch_size: int = 32, width: int = 768, output_dim: int = 512):
        super().__init__(output_dim, prediction_head, clf, freeze)
        self.feature_model = VisualTransformer(input_resolution, patch_size, width, layers, width // 64, output_dim)


class WideResNetCustom(CustomNet):
    """the reference's own example CustomNet (`custom.py:5-8`): feature_model = WideResNet(256, False)"""

    def __init__(self, prediction_head: bool = True, clf: bool = False, freeze: bool = False):
        super().__init__(256, prediction_head, clf, freeze)
        self.feature_model = WideResNet(256, False)
