"""objective name -> trainer class, as `src/eoe/training/__init__.py:8-11`.  'clip' takes the frozen text features from the
caller, or encodes its prompts with an `eoe_amd.models.CLIP` model's text tower given a tokenizer; the autoencoder trainer is not
built."""
from .ad_trainer import ADTrainer, NanGradientsError      # noqa: F401
from .hsc import HSCTrainer
from .bce import BCETrainer
from .dsvdd import DSVDDTrainer
from .dsad import DSADTrainer
from .focal import FocalTrainer
from .clip import ADClipTrainer
from .multiscale import multiscale_experiment      # noqa: F401

TRAINER = {"hsc": HSCTrainer, "bce": BCETrainer, "dsvdd": DSVDDTrainer, "dsad": DSADTrainer, "focal": FocalTrainer,
           "clip": ADClipTrainer}
