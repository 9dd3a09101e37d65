"""Counterpart of the reference trainer base class, `src/eoe/training/ad_trainer.py:93-662`, for the hot path:
`train_cls` (:356-471) and `eval_cls` (:473-550) inner loops, the class x seed `run` loop (:177-354) with
`weight_reset` copies (:31-34,232-243), NaN retry (:257-280), snapshot loading (:552-615), and the three
abstract objective hooks (:624-662) with unchanged signatures.

What differs, deliberately (SURVEY.md sections 3.1 and 8):
  * the optimiser is eoe_amd.FusedAdam (one kernel per step) -- constructed here exactly where the reference
    constructs torch.optim.Adam (:383), same hyper-parameters, driven by the stock MultiStepLR (:384);
  * anomaly scores and the loss stay on the device during an epoch; they are copied to the host once per epoch
    for the NaN check and the AUC (:447-455) instead of forcing two host syncs per step (:436,442);
  * the per-half masked Normalize (:413-425) is one affine with the normal class's statistics, fused into the
    encoder's first kernel when the encoder supports it (SURVEY.md section 8a note 1);
  * optional data parallelism (one process per GPU): each rank trains on its rows of every step batch,
    loss = sum(local) / global batch, gradients summed over RCCL, scores/labels all-gathered for the AUC;
  * multi-scale modes (`msms`, eoe_amd.msm): lpf / hpf / blur run as HIP kernels on the device batch after `.to(device)`
    and before the encoder's fused Normalize (:413-425 train, :501-505 test); so does `sharpen` (Pillow's UnsharpMask, a HIP
    kernel on the [0, 1] batch quantised to uint8; GPU devices only), unless the source applies it to its uint8 images before
    ToTensor and the noise as the reference does (ResidentImageSource.pre_tensor_msms);
  * a source in 'gcn-normalize' mode reports a `GcnNormalize` as `.normalize`: global contrast normalisation is per sample, not a
    per-channel affine, so the encoder's fused normalise is switched off and one HIP launch (eoe_amd.normalize.gcn_normalize)
    runs on the step batch after the multi-scale modes and before the encoder (:415-425), in training and in scoring;
  * `run(load=[[path]], train=False)` loads the snapshot's weights into the model before scoring it, together with the
    `ds_statistics` stored in the file.  The reference only takes the statistics from the file there and scores a freshly reset
    model (:257-264), which makes "score this snapshot again" impossible without training; a module handed in through `load` is
    scored as is, as in the reference.
  * `curves=True` makes the trainer keep what the reference always keeps: the whole ROC of a training epoch (the last one is returned) and the ROC and
    precision-recall curve of the evaluation (:452-455, 516-522), counted on the device (`eoe_rank_curves`), and the per-class
    "mean" curves (`logger.py:94-122`) in `trainer.curves`.  The default keeps the scores alone and does nothing else.
  * `histograms=True` logs what the reference always logs to TensorBoard: after every training epoch the histograms of the epoch's
    anomaly scores, normal half and outlier-exposure half (:458-465), after an evaluation those of the nominal and the anomalous test
    scores (:541-546), bucketed on the device (`eoe_score_hist`), kept in `trainer.histograms` and handed to
    `logger.add_histogram` under the reference's tags.  Off by default.
  * `extremes=k` ranks an evaluation's scores on the device (`eoe_score_extremes`): per label group the k highest and the k lowest
    test scores with their dataset indices -- false alarms and misses; the reference ranks only OE individuals this way
    (`Tree.scores_best` / `imsave_best`) and leaves the test scores to a per-sample JSON -- kept in `trainer.extremes`, logged as
    JSON and, where the source can hand out test images, as one picture.  Off (0) by default.
  * `explain=True` (with `extremes`) says where in those images the score comes from: the ViT tower's input gradient through the
    training backward, reduced to patch-level heat maps and laid over the pictures on the device (`eoe_amd.explain`,
    csrc/explain.hip), kept in `trainer.explanations` and logged as a second picture.  CNN32 and CNN28 are explained the same way,
    through their eval-mode BatchNorm backward and `eoe_conv_image_dgrad`, with pixel-level maps.  Off by default; not for WideResNet.
  * `attention=True` (with `extremes`) answers the same question from the forward pass alone: the attention rollout of the ViT tower
    over those images (`eoe_amd.explain.attention_rollout`, csrc/rollout.hip) -- no backward, no dependence on the objective or on a
    saturated score -- kept in `trainer.attention_maps` and logged as a picture of its own.  Off by default; ViT encoders only;
    independent of `explain`.
  * `cam=True` (with `extremes`) is the explanation of a WideResNet encoder: Grad-CAM maps of those images at `cam_layer`
    (`eoe_amd.explain.grad_cam`, csrc/gradcam.hip), kept in `trainer.cams` and logged as a picture of its own.  Off by default.
  * `breakdown=True` says which class causes the misses: per class of the test split the AUC, the FPR at `breakdown_tpr` and the AP
    of that class against the pool of all samples of the other side, counted on the device (`eoe_class_breakdown`,
    csrc/breakdown.hip), kept in `trainer.breakdowns`, logged as JSON, and after `run` as the task x class AUC matrix
    (`breakdown_matrix()`).  The reference has nothing of the kind.  Off by default; needs a source that kept its test classes.
  * `auc_ci=level` says how much of a test AUC is test-set sampling noise: DeLong's confidence interval per evaluation and, after a
    class's last seed, the paired test of the seeds' AUCs over the shared test split, from exact integer pair counts taken on the
    device (`eoe_delong_counts`, csrc/delong.hip; `metrics.delong`), kept in `trainer.auc_tests` and logged as JSON.  The reference
    has nothing of the kind.  Off by default.
  * `bootstrap=B` gives the same for the numbers DeLong does not cover: percentile intervals of the AUC, the average precision and the
    FPR at 95 % TPR from B stratified bootstrap replicates per evaluation and, after a class's last seed, the paired comparison of
    the seeds, every replicate resampled and counted on the device (`eoe_bootstrap_counts`, csrc/bootstrap.hip; `metrics.bootstrap`),
    kept in `trainer.bootstraps` and logged as JSON.  The reference has nothing of the kind.  Off by default.
Datasets, loggers with tensorboard/PDF output and the CLIP text objective are out of scope.
"""
import json
import math
import os
from abc import ABC, abstractmethod
from copy import deepcopy
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .. import ops, parallel
from ..metrics import (ROC, PRC, roc_auc, average_precision, auc_ap_device, curves_device, mean_plot, roc_curve, precision_recall_curve,
                       score_extremes, score_histograms, class_breakdown, delong, DELONG_MAX_COLUMNS, bootstrap as bootstrap_stats,
                       BOOTSTRAP_MAX_COLUMNS, BOOTSTRAP_MAX_REPLICATES)
from ..msm import apply_msms, check_supported
from ..normalize import GcnNormalize
from ..optim import FusedAdam


class NanGradientsError(RuntimeError):
    pass


def weight_reset(m: torch.nn.Module):
    # ad_trainer.py:31-34
    reset_parameters = getattr(m, "reset_parameters", None)
    if callable(reset_parameters):
        m.reset_parameters()


class JsonLogger:
    """minimal stand-in for `src/eoe/utils/logger.py` (out of scope): JSON lines + snapshots with the reference's
    snapshot dict layout {net, opt, sched, epoch, ds_statistics} (`logger.py:318-340`)"""

    def __init__(self, logdir: Optional[str] = None, active: bool = True):
        # under data parallelism every rank runs the trainer; only rank 0 writes files (the ranks' weights are identical, and
        # for BatchNorm encoders rank 0's running statistics are the ones kept)
        rank0 = int(os.environ.get("RANK", "0")) == 0
        self.dir, self.active = logdir, active and logdir is not None and rank0
        self.histograms = {}                                # tag -> {step: eoe_amd.metrics.Histogram} (add_histogram)
        if self.active:
            os.makedirs(os.path.join(logdir, "snapshots"), exist_ok=True)

    def print(self, msg: str):
        print(msg, flush=True)

    warning = logtxt = print

    def logjson(self, name: str, obj):
        if self.active:
            with open(os.path.join(self.dir, name + ".json"), "w") as f:
                json.dump(obj, f, default=lambda o: None if (isinstance(o, float) and o != o) else o)

    def add_scalar(self, *a, **k):
        pass

    def add_histogram(self, tag: str, hist, step: int = 0):
        """`SummaryWriter.add_histogram(tag, values, step)` for a histogram that is already made (`eoe_amd.metrics.score_histogram`):
        kept in `self.histograms[tag][step]`, and an active logger rewrites `<dir>/histograms.json`, {tag: {step: the seven
        fields}} of everything added so far (JSON turns the step into a string).  No TensorBoard file is written."""
        self.histograms.setdefault(tag, {})[int(step)] = hist
        if self.active:
            self.logjson("histograms", {t: {str(s): h.as_dict() for s, h in steps.items()} for t, steps in self.histograms.items()})

    def logimg(self, name: str, src, rows=None, nrow: int = 8, pad: int = 2, rowheaders=None, row_sep_at=(None, None),
               maxres: int = 128, step: int = None, mark=None, crop=None) -> np.ndarray:
        """`Logger.logimg` (`logger.py:202-295`) on images that lie where they are: `eoe_amd.imgrid.image_grid(src, rows, ...)`
        composes the uint8 [Hg, Wg, 3] picture (on the device for a device source), one copy brings it back, and when the logger is
        active Pillow writes it as `<dir>/<name>.png` (`<name>_v<step>.png` with `step`), sub-directories created.  Text is not
        drawn: `rowheaders` go to `<name>.headers.json` next to the picture (a list of strings, one per grid row) and no black
        header column is added.  Without Pillow the picture is still returned (one warning).  Always returns the array."""
        from ..imgrid import image_grid, save_png
        img = image_grid(src, rows, crop=crop, nrow=nrow, pad=pad, maxres=maxres, mark=mark, row_sep_at=row_sep_at).cpu().numpy()
        if self.active:
            stem = os.path.join(self.dir, f"{name}_v{step}" if step is not None else name)
            os.makedirs(os.path.dirname(stem), exist_ok=True)
            if img.size:
                save_png(stem + ".png", img)
            if rowheaders is not None:
                with open(stem + ".headers.json", "w") as f:
                    json.dump([str(h) for h in rowheaders], f)
        return img

    def snapshot(self, name: str, net: torch.nn.Module, opt=None, sched=None, epoch: int = None, **kwargs):
        if not self.active:
            return None
        path = os.path.join(self.dir, "snapshots", name + ".pt")
        data = {"net": net.state_dict(), "opt": opt.state_dict() if opt is not None else None,
                "sched": sched.state_dict() if sched is not None else None, "epoch": epoch}
        data.update(kwargs)
        torch.save(data, path)
        return path


class ADTrainer(ABC):
    AD_MODES = ("one_vs_rest", "leave_one_out", "fifty_fifty")
    KEEP_SNAPSHOT_IN_RAM = False

    def __init__(self, model: torch.nn.Module, train_transform=None, test_transform=None, dataset=None,
                 oe_dataset=None, datapath: str = None, logger: JsonLogger = None, epochs: int = 1, lr: float = 1e-3,
                 wdk: float = 0.0, milestones: List[int] = (), batch_size: int = 128, ad_mode: str = "one_vs_rest",
                 device: Union[str, torch.device] = "cuda", oe_limit_samples=np.inf, oe_limit_classes=np.inf,
                 msms=(), workers: int = 2, classes: List[str] = None, data_parallel: bool = False,
                 graph_steps: bool = False, sync_bn: bool = True, exact_bn="auto", curves: bool = False,
                 previews: bool = False, histograms: bool = False, extremes: int = 0, explain: bool = False,
                 attention: bool = False, breakdown: bool = False, breakdown_tpr: float = 0.95, auc_ci: Optional[float] = None,
                 cam: bool = False, cam_layer: str = "layer4", cam_mode: str = "gradcam", neighbors: int = 0,
                 knn_baseline: bool = False, mahalanobis_baseline: bool = False, mahalanobis_shrinkage="ledoit_wolf",
                 bootstrap: Optional[int] = None, bootstrap_level: float = 0.95, bootstrap_seed: int = 0, knn_coreset=0):
        """same parameters as the reference (`ad_trainer.py:98-164`).  `dataset` is either a step-batch source
        (eoe_amd.data: an object with `.loaders(batch_size)`, `.nominal_label`, `.normalize`) or a callable
        `(cls, seed) -> source`; `classes` names the classes to iterate (default: one class "0").

        `curves=True`: the ROC / PRC containers that `train_cls` and `eval_cls` return carry their curves (`tpr` / `fpr` / `ths`,
        `prec` / `rec` / `ths`), and `run` leaves `self.curves` = {'train_rocs', 'eval_rocs', 'eval_prcs': [class][seed] containers,
        'mean_train_rocs', 'mean_eval_rocs', 'mean_eval_prcs': [class] `mean_plot` of the seeds that produced one, else None} and
        logs each evaluation's curves as `eval_cls{c}_it{seed}_roc` / `_prc`.  `mean_plot` thins the curves with `np.random.choice`:
        after each class `run` makes the reference's draws in the reference's order (training ROC, evaluation ROC, evaluation
        PRC; `ad_trainer.py:308-313`).  The reference's intermediate plots after every seed (`:283, 295-296`) draw from `np.random`
        as well whenever a class has more than one curve; those draws are NOT replayed, so from the second seed of a class on the
        generator is not where the reference's is.  With `curves=False` (the default) nothing of this runs: no extra launch, no
        draw, the same return values and files as before.

        `previews=True`: with an active logger, the first seed of a class logs `training_cls{c}-{cstr}_preview` (40 images per label of
        the train loader's output) and `eval_cls{c}-{cstr}_preview` (20 per label of the test loader's) as the reference does
        (`ad_trainer.py:386-393, 486-493`), through `ds.preview` and `logger.logimg`: one row per label, the labels' sample counts as
        `rowheaders`.  The source draws the preview from a private generator, so the training that follows is unchanged.  Default
        off: nothing runs, nothing is drawn, the same files as before.

        `histograms=True`: after each training epoch's NaN check `train_cls` makes the two histograms of the epoch's scores (under
        data parallelism: the gathered ones), label 0 and label 1, and `eval_cls` the two of the test scores
        (`eoe_amd.metrics.score_histograms`: one launch sequence per pair for device scores, only counts and five scalars come back).
        They are kept in `self.histograms` = {tag: {step: `metrics.Histogram`}} and handed to `logger.add_histogram(tag, hist, step)`
        under the reference's tags and steps (`ad_trainer.py:458-465, 541-546`): `Training: CLS{cls} SEED{seed} anomaly_scores normal`
        / `... anomalous` at step `ep`, `Eval: (SD{seed}) anomaly_scores cls{cls} nominal` / `... anomalous` at step 0.  A label without
        scores is skipped (the reference's `make_histogram` would raise).  `run` starts with an empty `self.histograms`.  Default off:
        no launch, no file, the same return values and files as before.

        `extremes=k` (k in [1, 1024]): after its metrics `eval_cls` ranks the test scores it holds (`eoe_amd.metrics.score_extremes`:
        one call for device scores, only 4 k pairs and three counts come back) -- per label group, nominal (label 0) and anomalous
        (label 1), the k highest and the k lowest scores, equal scores in ascending position, positions mapped to the loader's dataset
        indices.  The `metrics.Extremes` is kept in `self.extremes[f"eval_cls{cls}_it{seed}"]` and its `as_dict()` logged as
        `eval_cls{cls}_it{seed}_extremes` through `logger.logjson`.  With an active logger and a source that offers
        `test_images(rows)` (ResidentImageSource) the picture `eval_cls{cls}-{clsstr}_it{seed}_extremes` follows through
        `logger.logimg`: one grid row per non-empty list in the order nominal most, nominal least, anomalous most, anomalous least,
        every row cut to the shortest of them (k, or a smaller group's size), `rowheaders` naming each row with its group's size;
        other sources get the JSON alone.  `run` starts with an empty `self.extremes`.  Default 0: no launch, no file, the same
        return values and files as before.

        `explain=True` (needs `extremes` > 0, a ViT, CNN32 or CNN28 encoder and a source with `test_inputs(rows)`; anything else raises -- the first
        here, the other two at the start of `eval_cls`, before any scoring): the rows of the extremes picture are explained
        (`eoe_amd.explain`).  Their test inputs go through the eval loop's own test-time steps, `input_gradient` differentiates the
        trainer's score under the gradient scale of the compute type, `saliency(mode="max", pool=patch)` makes the patch-level maps
        (a CNN32 or CNN28: `pool=None`, pixel-level maps; on a grayscale source the gradient has one channel)
        -- kept in `self.explanations[f"eval_cls{cls}_it{seed}"]`, fp32 [rows, H, W] on the device, rows in the picture's order --
        and `overlay` lays them over `ds.test_pictures(rows)` (those images in the [0, 1] scale, without the source's Normalize); an active logger gets `eval_cls{cls}-{clsstr}_it{seed}_extremes_heat`
        with the layout and row headers of the extremes picture.  One forward and one backward of the tower over 4 k images at most.
        WideResNet is refused (`explain.input_gradient`).  `run` starts with an empty `self.explanations`.  Default
        off: no launch, no file, the same return values and files as before.

        `attention=True` (the same three conditions, but a ViT encoder only; refused the same way): the rows of the extremes picture get their attention
        rollout (`eoe_amd.explain.attention_rollout`, defaults: the heads' mean, residual 0.5, every block): their test inputs go
        through the eval loop's own test-time steps and one forward pass of the tower, nothing is differentiated and neither the
        objective nor the centre enters.  The maps are kept in `self.attention_maps[f"eval_cls{cls}_it{seed}"]`, fp32 [rows, H, W] on
        the device, rows in the picture's order; an active logger with a source that offers `test_pictures` gets
        `eval_cls{cls}-{clsstr}_it{seed}_extremes_attn`, laid over the pictures like the heat maps.  `run` starts with an empty
        `self.attention_maps`.  Independent of `explain`; default off: no launch, no file, the same return values and files as
        before.

        `cam=True` (needs `extremes` > 0, a WideResNet encoder and a source with `test_inputs(rows)`; refused the same way): the rows
        of the extremes picture get their Grad-CAM maps (`eoe_amd.explain.grad_cam` at `cam_layer` -- 'layer1' ... 'layer4' -- in
        `cam_mode` -- 'gradcam' or 'hirescam'; csrc/gradcam.hip): the activation of that layer weighted by the gradient of the score,
        rectified and upsampled onto the image, the explanation a WideResNet gets in place of `explain`.  The maps are kept in
        `self.cams[f"eval_cls{cls}_it{seed}"]`, fp32 [rows, H, W] on the device; an active logger with a source that offers
        `test_pictures` gets `eval_cls{cls}-{clsstr}_it{seed}_extremes_cam`.  `run` starts with an empty `self.cams`.  (`neighbors=k`,
        k in [1, 64], needs `extremes` > 0, a source with `test_inputs` and `normal_inputs` and a model with a feature output: the
        rows of the extremes picture and ALL normal training images under the test transform are embedded in the arithmetic `eval_cls`
        scored in, and one `eoe_amd.neighbors.feature_knn` (csrc/knn.hip) finds each row's k nearest normal training images:
        `self.neighbors[f"eval_cls{cls}_it{seed}"]`, `eval_cls{cls}_it{seed}_extremes_neighbors` as JSON with dataset indices, and with
        `normal_pictures` the picture `eval_cls{cls}-{clsstr}_it{seed}_extremes_neighbors`, each row an image and its k neighbours.
        `knn_baseline=True` (needs `neighbors`) scores the whole test split by the mean distance to its k nearest normal features,
        the standard non-parametric baseline: AUC and AP in `self.knn_results[cls]`, `eval_cls{cls}_it{seed}_knn` and a text line.
        `knn_coreset=m` (needs `neighbors`; an int >= 1 or a float in (0, 1), the share of the normal rows; 0: off) replaces the
        normal features in both searches by their greedy k-center coreset (`eoe_amd.coreset.kcenter`, csrc/coreset.hip; start at
        normal row 0, m clamped to [neighbors, n_normal]): the memory bank a feature-bank detector ships.  The `Coreset` is kept in
        `self.coresets[f"eval_cls{cls}_it{seed}"]` (`run` starts with it empty), its `as_dict` with dataset indices goes to
        `eval_cls{cls}_it{seed}_coreset`, `self.knn_results[cls]` gains "coreset": {m, n, cover}, and with `normal_pictures` the
        first 32 centres, the most mutually distant normal images, are logged as `eval_cls{cls}-{clsstr}_it{seed}_coreset`.
        All default off: no launch, no file, the same lines and return values.)  Default off:
        no launch, no file, the same return values and files as before.

        `mahalanobis_baseline=True` (independent of `extremes` and `neighbors`; needs a source with `normal_inputs` and a model with a
        feature output, refused at the start of `eval_cls` otherwise): the Gaussian baseline in feature space.  All normal training
        images under the test transform are embedded as for `neighbors` (once, when both are on), `eoe_amd.mahalanobis.fit_gaussian`
        fits their mean and covariance (csrc/mahalanobis.hip; `mahalanobis_shrinkage`: "ledoit_wolf" or a number in [0, 1]) and the
        Mahalanobis distance scores the test features `eval_cls` kept: `self.mahalanobis_results[cls]` = {shrinkage, auc, avg_prec,
        n_normal, D, nonfinite}, `eval_cls{cls}_it{seed}_mahalanobis` and a text line.  Default off: no launch, no file, the same
        lines and return values.

        `breakdown=True` (needs a source with `test_classes`, the test rows' original class ids -- a `LabelledImageSet`'s sources have
        them; anything else raises at the start of `eval_cls`, before any scoring): after its metrics `eval_cls` breaks the test
        scores down by class (`eoe_amd.metrics.class_breakdown`: one call for device scores) -- per class the AUC, the FPR at the
        first ROC point whose TPR reaches `breakdown_tpr` and, for anomalous classes, the AP of that class against the pool of all
        samples of the other side, plus the pooled FPR at that TPR.  Under `one_vs_rest` that splits the anomalies ("cat against
        dog", "cat against truck"), under `leave_one_out` the nominal side (which class raises the false alarms).  The
        `metrics.Breakdown` is appended to `self.breakdowns[cls]` (one per seed), its `to_json()` logged as
        `eval_cls{cls}_it{seed}_breakdown`, and one text line names the hardest class (lowest AUC).  After `run`,
        `breakdown_matrix()` is the [task, class] matrix of the seeds' mean AUCs, logged with the tasks' mean pooled FPRs as
        `breakdown_auc`.  `run` starts with an empty `self.breakdowns`.  Default off: no launch, no file, the same return values
        and files as before.

        `auc_ci=level` (a confidence level in (0, 1), such as 0.95; anything else raises here): where `eval_cls` computes the AUC it
        also calls `eoe_amd.metrics.delong` on the labels and scores it holds (device scores: one `eoe_delong_counts` call, a
        handful of integers come back).  The returned `ROC` gains the attributes `ci` = (lo, hi) at that level, `se` and `var`; the
        `AucTest`'s `to_json(level)` is logged as `eval_cls{cls}_it{seed}_auc_ci` and the `Eval:` text line ends with the interval.
        The evaluation's scores stay on the device, and after the last seed of a class `run` tests the seeds against each other
        in one call with one column per seed (the first 8 when there are more, with a logged note) -- the test split and its order
        are the same for every seed -- keeps the `AucTest` in `self.auc_tests[cls]` and logs its AUCs, covariance matrix and
        pairwise p-values as `eval_cls{cls}_auc_compare`: whether the seed-to-seed spread exceeds what the size of the test set
        explains.  Seeds whose label vectors differ are not compared (one logged line).  The scores are kept only inside `run`, from
        a class's first seed to its comparison; `eval_cls` called on its own keeps nothing.  A NaN test score costs that evaluation
        its interval (one logged line, no attribute, no file) and its place in the comparison, not the run.  `run` starts with an
        empty `self.auc_tests`.  Default None: no launch, no file, no attribute, the same text line.

        `bootstrap=B` (an integer in [1, 65 536]; anything else raises here), with `bootstrap_level` (a confidence level in (0, 1)) and
        `bootstrap_seed`: where `eval_cls` computes the AUC it also resamples the test scores B times (`eoe_amd.metrics.bootstrap`: one
        call for device scores, 9 (B + 1) numbers back) -- the stratified bootstrap of the AUC, the average precision and the FPR at
        95 % TPR.  The `Bootstrap` is kept in `self.bootstraps[cls][seed]`, the percentile intervals are attached to the returned
        containers (`roc.boot_ci`, `prc.ci`, `prc.se`), `to_json(bootstrap_level)` is logged as `eval_cls{cls}_it{seed}_bootstrap` and
        the `Eval:` text line ends with the AP's interval.  In `run`, after a class's last seed, the seeds' scores (the first 8) share
        one set of replicates, provided their test labels agree: the intervals and p-values of every pair's difference in AUC, AP and
        FPR are logged as `eval_cls{cls}_bootstrap_compare`.  Independent of `auc_ci`.  A NaN score costs the interval and one logged
        line, not the run.  `run` starts with an empty `self.bootstraps`.  Default None: no launch, no file, no attribute, the same
        text line."""
        self.previews = bool(previews)
        self.model = model.cpu() if model is not None else model
        # replay forward + loss + backward + scores of the full-size step batch from a HIP graph (eoe_amd.GraphedStep): for the
        # launch-bound small encoders (CNN32 at 32x32); single GPU only, ragged batches run eagerly
        self.graph_steps = graph_steps
        self.train_transform, self.test_transform = train_transform, test_transform
        self.dsstr, self.oe_dsstr, self.datapath = dataset, oe_dataset, datapath
        self.logger = logger if logger is not None else JsonLogger(None)
        self.device = torch.device(device)
        self.epochs, self.lr, self.wdk, self.milestones, self.batch_size = epochs, lr, wdk, list(milestones), batch_size
        self.ad_mode = ad_mode
        self.center = None
        self.workers = workers
        self.ds = dataset if hasattr(dataset, "loaders") else None
        if classes is None:
            # a labelled multi-class set (eoe_amd.data.LabelledImageSet) names its own classes, as `str_labels(dsstr)` does
            # in the reference (ad_trainer.py:226); a single pre-built task is one class "0"
            classes = list(dataset.classes) if hasattr(dataset, "source") and hasattr(dataset, "classes") else ["0"]
        self.classes = classes
        self.data_parallel = data_parallel
        self.sync_bn = sync_bn      # data parallel only: BatchNorm statistics of the GLOBAL step batch (eoe_amd.parallel.enable_sync_bn)
        # BatchNorm encoders (CNN32 / CNN28 / WideResNet): the convolutions and linear layers as exact-fp32 implicit GEMMs on the fp32
        # matrix cores (eoe_amd.set_parity_mode, csrc/parity.hip).  The reference runs these nets in fp32 (models/cnn.py:73-86,
        # models/resnet.py:85-149); with 16-bit MFMA operands Adam at lr >= 1e-3 amplifies the operand rounding to 3-10 x the
        # reference's own fp32-vs-fp64 noise within ten steps (tests/test_gpu_parity_big.py), the fp32 mode stays inside it.
        # "auto" = on for a BatchNorm encoder trained with lr >= 1e-3 (every BatchNorm runner of the reference: train_cifar.py:17,
        # train_imagenet.py:16), True / False = forced.  The ViT has no BatchNorm and meets the bar in its 16-bit mode.
        self.exact_bn = exact_bn
        # int k < inf: k random OE samples per task; a list: exactly those rows of the OE set (bases.py:196-201); inf: all (_limit_oe)
        self.oe_limit_samples = oe_limit_samples
        self.msms = list(msms or ())
        check_supported(self.msms, self.device)          # sharpen on a CPU device raises NotImplementedError
        self._step_msms = self.msms                         # the train MSMs left to the step batch (_msm_source)
        self._gcn = None                                    # the task's GcnNormalize, if its source is in that mode (_normalize_hook)
        self.with_curves = bool(curves)
        self.curves = None                                  # filled by run() when with_curves
        self.with_histograms = bool(histograms)
        self.histograms = {}                                # tag -> {step: Histogram}, filled by train_cls / eval_cls when with_histograms
        if isinstance(extremes, bool) or not isinstance(extremes, (int, np.integer)) or not 0 <= extremes <= 1024:
            raise ValueError(f"extremes must be an integer in [0, 1024] (0: off), not {extremes!r}")
        self.n_extremes = int(extremes)
        self.extremes = {}                                  # f"eval_cls{c}_it{seed}" -> Extremes, filled by eval_cls when n_extremes > 0
        self.with_explain = bool(explain)
        if self.with_explain and self.n_extremes == 0:
            raise ValueError("explain=True explains the rows that extremes=k ranks: extremes must be at least 1")
        self.explanations = {}                              # f"eval_cls{c}_it{seed}" -> fp32 [rows, H, W] maps, filled by eval_cls when with_explain
        self.with_attention = bool(attention)
        if self.with_attention and self.n_extremes == 0:
            raise ValueError("attention=True rolls out the rows that extremes=k ranks: extremes must be at least 1")
        self.attention_maps = {}                            # the same keys -> fp32 [rows, H, W] rollout maps, filled by eval_cls when with_attention
        self.with_cam = bool(cam)
        if self.with_cam and self.n_extremes == 0:
            raise ValueError("cam=True maps the rows that extremes=k ranks: extremes must be at least 1")
        if self.with_cam:
            from ..explain import CAM_LAYERS, CAM_MODES
            if cam_layer not in CAM_LAYERS:
                raise ValueError(f"cam_layer {cam_layer!r} is none of {CAM_LAYERS}")
            if cam_mode not in CAM_MODES:
                raise ValueError(f"cam_mode {cam_mode!r} is none of {tuple(CAM_MODES)}")
        self.cam_layer, self.cam_mode = cam_layer, cam_mode
        self.cams = {}                                      # the same keys -> fp32 [rows, H, W] Grad-CAM maps, filled by eval_cls when with_cam
        if isinstance(neighbors, bool) or not isinstance(neighbors, (int, np.integer)) or not 0 <= neighbors <= 64:
            raise ValueError(f"neighbors must be an integer in [0, 64] (0: off), not {neighbors!r}")
        self.n_neighbors = int(neighbors)
        if self.n_neighbors > 0 and self.n_extremes == 0:
            raise ValueError("neighbors=k finds the nearest normal training images of the rows that extremes=k ranks: extremes must "
                             "be at least 1")
        self.with_knn_baseline = bool(knn_baseline)
        if self.with_knn_baseline and self.n_neighbors == 0:
            raise ValueError("knn_baseline=True scores the test split by its neighbors=k nearest normal features: neighbors must be "
                             "at least 1")
        self.neighbors = {}                                 # f"eval_cls{c}_it{seed}" -> eoe_amd.neighbors.Neighbors, filled by eval_cls when n_neighbors > 0
        self.knn_results = {}                               # cls -> {k, auc, avg_prec, n_normal, D} of the last seed, filled by eval_cls when with_knn_baseline
        is_share = isinstance(knn_coreset, (float, np.floating))
        if isinstance(knn_coreset, bool) or not (is_share or isinstance(knn_coreset, (int, np.integer))) \
                or (is_share and not 0.0 < knn_coreset < 1.0) or (not is_share and knn_coreset < 0):
            raise ValueError(f"knn_coreset must be a number of centres >= 1, a share of the normal rows in (0, 1) or 0 (off), "
                             f"not {knn_coreset!r}")
        self.knn_coreset = float(knn_coreset) if is_share else int(knn_coreset)
        if self.knn_coreset and self.n_neighbors == 0:
            raise ValueError("knn_coreset=m searches the neighbors=k nearest rows among m representatives of the normal features: "
                             "neighbors must be at least 1")
        self.coresets = {}                                  # f"eval_cls{c}_it{seed}" -> eoe_amd.coreset.Coreset, filled by eval_cls when knn_coreset
        self.with_mahalanobis = bool(mahalanobis_baseline)
        if self.with_mahalanobis:
            from ..mahalanobis import check_shrinkage
            check_shrinkage(mahalanobis_shrinkage)
        self.mahalanobis_shrinkage = mahalanobis_shrinkage
        self.mahalanobis_results = {}                       # cls -> {shrinkage, auc, avg_prec, n_normal, D, nonfinite} of the last seed, filled by eval_cls when with_mahalanobis
        self.with_breakdown = bool(breakdown)
        if isinstance(breakdown_tpr, bool) or not isinstance(breakdown_tpr, (int, float)) or not 0.0 < breakdown_tpr <= 1.0:
            raise ValueError(f"breakdown_tpr must be in (0, 1], not {breakdown_tpr!r}")
        self.breakdown_tpr = float(breakdown_tpr)
        self.breakdowns = {}                                # cls -> [Breakdown per seed], filled by eval_cls when with_breakdown
        if auc_ci is not None and (isinstance(auc_ci, bool) or not isinstance(auc_ci, (int, float)) or not 0.0 < auc_ci < 1.0):
            raise ValueError(f"auc_ci must be None or a confidence level in (0, 1), not {auc_ci!r}")
        self.auc_ci = None if auc_ci is None else float(auc_ci)
        self.auc_tests = {}                                 # cls -> AucTest over the seeds' scores, filled by run when auc_ci and seeds > 1
        if bootstrap is not None and (isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer))
                                      or not 1 <= bootstrap <= BOOTSTRAP_MAX_REPLICATES):
            raise ValueError(f"bootstrap must be None or a number of replicates in [1, {BOOTSTRAP_MAX_REPLICATES}], not {bootstrap!r}")
        if isinstance(bootstrap_level, bool) or not isinstance(bootstrap_level, (int, float)) or not 0.0 < bootstrap_level < 1.0:
            raise ValueError(f"bootstrap_level must be a confidence level in (0, 1), not {bootstrap_level!r}")
        if isinstance(bootstrap_seed, bool) or not isinstance(bootstrap_seed, (int, np.integer)) or not 0 <= bootstrap_seed < 1 << 64:
            raise ValueError(f"bootstrap_seed must be an integer in [0, 2^64), not {bootstrap_seed!r}")
        self.bootstrap = None if bootstrap is None else int(bootstrap)
        self.bootstrap_level, self.bootstrap_seed = float(bootstrap_level), int(bootstrap_seed)
        self.bootstraps = {}                                # cls -> {seed: Bootstrap}, filled by eval_cls when bootstrap
        self._boot_scores = None
        self._seed_scores = None                            # [(seed, labels, scores)] of the class `run` is at, while it has seeds to compare

    # ------------------------------------------------------------------------------------------- run
    def get_nominal_classes(self, cur_class: int):
        """the normal classes of the task "class `cur_class`" under the AD mode (ad_trainer.py:166-175)"""
        n = len(self.classes)
        if self.ad_mode == "one_vs_rest":
            return [cur_class]
        elif self.ad_mode == "leave_one_out":
            return [c for c in range(n) if c != cur_class]
        elif self.ad_mode == "fifty_fifty":
            return [c % n for c in range(cur_class, n // 2 + cur_class)]
        raise NotImplementedError(f"AD mode {self.ad_mode} unknown. Known modes are {ADTrainer.AD_MODES}.")

    def _limit_oe(self, ds):
        """`oe_limit_samples` as the reference's `create_subset` applies it to the OE data when a task's dataset is made
        (`bases.py:196-201`): an int k < inf keeps `sorted(np.random.choice(n, min(k, n), False))`, a list exactly its rows.  The
        default (inf) does not touch the source.  A pre-built `trainer.ds` is restricted the same way each time a run asks for it
        (the evolve experiment sets the list per individual, `evolve/__init__.py:70-73`)."""
        limit = self.oe_limit_samples
        if isinstance(limit, (int, float)):
            if not limit < np.inf:
                return ds
            if limit < 1:
                raise ValueError(f"oe_limit_samples must be at least 1, not {limit}")
        if not hasattr(ds, "set_oe_subset"):
            raise NotImplementedError(f"oe_limit_samples needs a source whose OE set can be restricted (set_oe_subset); "
                                      f"{type(ds).__name__} has none")
        if isinstance(limit, (int, float)):
            n = len(ds.oe)                          # a tensor or a RaggedImageSet: rows of the resident OE set
            rows = sorted(np.random.choice(n, min(int(limit), n), False))
        else:
            rows = list(limit)
        ds.set_oe_subset([int(r) for r in rows])
        return ds

    def _dataset(self, c: int, seed: int, ds_statistics: Optional[dict] = None):
        """the task of one (class, seed) run (`_task_source`), its outlier exposure limited to `oe_limit_samples`"""
        return self._limit_oe(self._task_source(c, seed, ds_statistics))

    def _task_source(self, c: int, seed: int, ds_statistics: Optional[dict] = None):
        """The reference builds the task with `load_dataset(dsstr, datapath,
        self.get_nominal_classes(c), 0, ...)` unless `trainer.ds` was pre-set (ad_trainer.py:248-253): here a pre-built
        step-batch source is used as is, a labelled image set (`.source(normal_classes, seed)`) is asked for the task of the
        current AD mode, and a callable (cls, seed) -> source decides for itself."""
        if self.ds is not None:
            return self.ds
        if hasattr(self.dsstr, "source"):
            if ds_statistics is not None:            # a snapshot's statistics win over fitting them again (bases.py:326-329)
                return self.dsstr.source(self.get_nominal_classes(c), seed, ds_statistics=ds_statistics)
            return self.dsstr.source(self.get_nominal_classes(c), seed)
        if callable(self.dsstr):
            return self.dsstr(c, seed)
        raise ValueError("dataset must be a step-batch source, a labelled image set or a callable (cls, seed) -> source")

    NAN_ATTEMPTS, NAN_GIVE_UP_AT = 5, 3      # ad_trainer.py:257-280: up to five tries; the third failure clears the result

    def _fresh_model(self, preset) -> torch.nn.Module:
        """the model one (class, seed) run starts from (ad_trainer.py:232-243): a module handed in through `load` as is,
        otherwise a copy of the CPU master with every layer re-initialised through its own `reset_parameters`"""
        if isinstance(preset, torch.nn.Module):
            model = deepcopy(preset)
        else:
            model = deepcopy(self.model)
            model.apply(weight_reset)
        for p in model.parameters():
            p.detach_().requires_grad_()
        return model

    def _train_with_retries(self, c: int, cstr: str, seed: int, preset, train: bool):
        """NaN scores abort a run (`NanGradientsError`); the reference then starts over on a freshly built dataset with fresh
        weights.  Returns (model, training ROC, dataset); the model is None only if the reference would return None"""
        # a snapshot to load brings the statistics its model was trained with (ad_trainer.py:248-252)
        # (the file is read once here and kept for this run: `load` below takes the weights from the same read)
        stats = None
        if isinstance(preset, str):
            self._snapshot_read = (preset, self.unify_snapshot_style(torch.load(preset, map_location="cpu")))
            stats = self.load_ds_statistics(preset)
        try:
            return self._train_attempts(c, cstr, seed, preset, train, stats)
        finally:
            self._snapshot_read = None

    def _train_attempts(self, c: int, cstr: str, seed: int, preset, train: bool, stats):
        ds = self._dataset(c, seed, stats)
        model = roc = None
        for attempt in range(self.NAN_ATTEMPTS):
            model = self._fresh_model(preset)
            try:
                if train:
                    model, roc = self.train_cls(model, ds, c, cstr, seed, preset)
                elif isinstance(preset, str):
                    self.load(preset, model)             # score a snapshot file: its weights with its statistics
                return model, roc, ds
            except NanGradientsError:
                self.logger.warning(f'NaN scores while training class {c} "{cstr}", seed {seed} (failure {attempt + 1} of '
                                    f'{self.NAN_ATTEMPTS}); retrying with fresh weights and data.')
                ds = self._dataset(c, seed, stats)
                if attempt + 1 == self.NAN_GIVE_UP_AT:
                    model = roc = None
        return model, roc, ds

    def run(self, run_classes: List[int] = None, run_seeds: int = 1, load: List[List] = None, test: bool = True,
            train: bool = True) -> Tuple[List[List[torch.nn.Module]], dict]:
        """every requested class x `run_seeds` repetitions (`ad_trainer.py:177-354`): train, evaluate, snapshot.
        Returns (models[class][seed], {'mean_auc', 'mean_avg_prec', 'std_auc', 'cls_aucs'})"""
        n_cls = len(self.classes)
        wanted = set(range(n_cls)) if run_classes is None else set(run_classes)
        # ad_trainer.py:231-232: a pre-loaded dataset is ONE task; iterating classes over it would train the same task again
        assert self.ds is None or len(wanted) == 1, "pre-loading DS (setting trainer.ds to something) only allowed for one class"
        models, train_rocs = [[] for _ in range(n_cls)], [[] for _ in range(n_cls)]
        eval_rocs, eval_prcs = [[] for _ in range(n_cls)], [[] for _ in range(n_cls)]
        means = {k: [None] * n_cls for k in ("mean_train_rocs", "mean_eval_rocs", "mean_eval_prcs")}
        self.histograms = {}
        self.extremes = {}
        self.explanations = {}
        self.attention_maps = {}
        self.cams = {}
        self.neighbors = {}
        self.knn_results = {}
        self.coresets = {}
        self.mahalanobis_results = {}
        self.breakdowns = {}
        self.auc_tests = {}
        self._seed_scores = None
        self.bootstraps = {}
        self._boot_scores = None
        for c, cstr in enumerate(self.classes):
            if c not in wanted:
                continue
            # auc_ci: the seeds' scores are kept, where they are, only from here to the comparison below
            self._seed_scores = [] if self.auc_ci is not None and test and run_seeds > 1 else None
            self._boot_scores = [] if self.bootstrap is not None and test and run_seeds > 1 else None
            for seed in range(run_seeds):
                self.logger.print(f'------ start training cls {c} "{cstr}" ------')
                preset = None
                if load is not None and c < len(load) and seed < len(load[c]):
                    preset = load[c][seed]
                model, roc, ds = self._train_with_retries(c, cstr, seed, preset, train)
                train_rocs[c].append(roc)
                roc = prc = None
                if test and model is not None:
                    roc, prc = self.eval_cls(model, ds, c, cstr, seed)
                eval_rocs[c].append(roc)
                eval_prcs[c].append(prc)
                if self.with_curves and roc is not None:
                    self.logger.logjson(f"eval_cls{c}_it{seed}_roc", {"fpr": roc.fpr.tolist(), "tpr": roc.tpr.tolist(),
                                                                      "ths": roc.ths.tolist(), "auc": roc.auc})
                    self.logger.logjson(f"eval_cls{c}_it{seed}_prc", {"prec": prc.prec.tolist(), "rec": prc.rec.tolist(),
                                                                      "ths": prc.ths.tolist(), "avg_prec": prc.avg_prec})
                if model is not None:
                    self.logger.snapshot(f"snapshot_cls{c}_it{seed}", model, epoch=self.epochs,
                                         ds_statistics=getattr(ds, "ds_statistics", None))
                models[c].append(model if (model is None or ADTrainer.KEEP_SNAPSHOT_IN_RAM) else None)
            if self._seed_scores is not None:
                self._compare_seeds(c)
            if self._boot_scores is not None:
                self._compare_seeds_bootstrap(c)
            if self.with_curves:
                # the seeds' "mean" curves of this class, in the reference's order (:308-313; plot_many skips the seeds without a curve)
                for k, lst in (("mean_train_rocs", train_rocs[c]), ("mean_eval_rocs", eval_rocs[c]), ("mean_eval_prcs", eval_prcs[c])):
                    means[k][c] = mean_plot([r for r in lst if r is not None])

        def per_class(curves, attr):
            """mean over the seeds of each class that produced a curve"""
            return [float(np.mean([getattr(r, attr) for r in lst if r is not None]))
                    for lst in curves if any(r is not None for r in lst)]

        mean_auc = std_auc = mean_avg_prec = float("nan")
        if test:
            aucs, aps = per_class(eval_rocs, "auc"), per_class(eval_prcs, "avg_prec")
            if aucs:
                mean_auc, std_auc = float(np.mean(aucs)), float(np.std(aucs))
            if aps:
                mean_avg_prec = float(np.mean(aps))
            self.logger.logtxt(f"Eval: Overall {mean_auc * 100:04.2f}% +- {std_auc * 100:04.2f}% AUC.")
        if self.with_curves:
            self.curves = {"train_rocs": train_rocs, "eval_rocs": eval_rocs, "eval_prcs": eval_prcs, **means}
        cls_aucs = [[None if r is None else r.get_score() for r in lst] for lst in eval_rocs]
        self.logger.logjson("results", {"eval_mean_auc": mean_auc, "eval_std_auc": std_auc,
                                        "eval_mean_avg_prec": mean_avg_prec, "eval_cls_rocs": cls_aucs,
                                        "classes": self.classes})
        if self.with_breakdown and self.breakdowns:
            nan_none = lambda x: None if x != x else float(x)                                       # noqa: E731
            self.logger.logjson("breakdown_auc", {
                "auc": [[nan_none(x) for x in row] for row in self.breakdown_matrix()], "tpr_level": self.breakdown_tpr,
                "fpr_at_tpr": [nan_none(self._nanmean([b.fpr_at_tpr for b in self.breakdowns.get(c, [])])) for c in range(n_cls)],
                "classes": self.classes})
        return models, {"mean_auc": mean_auc, "mean_avg_prec": mean_avg_prec, "std_auc": std_auc, "cls_aucs": cls_aucs}

    # ------------------------------------------------------------------------------------------- hot loop
    def _msm_source(self, ds):
        """MSMs filter in the [0, 1] pixel scale, before Normalize: a source that fuses Normalize into its batches
        (ResidentImageSource) hands (mean, std) to the encoder's fused normalise instead"""
        if self.msms and hasattr(ds, "defer_normalize"):
            ds.defer_normalize(True)
        # a source that applies some train MSMs itself, before ToTensor (ResidentImageSource: sharpen), claims them; told every
        # time, so that a source shared between trainers never keeps an earlier trainer's claim
        claimed = ds.pre_tensor_msms(self.msms) if hasattr(ds, "pre_tensor_msms") else []
        self._step_msms = [m for m in self.msms if not any(m is c for c in claimed)]

    def _normalize_hook(self, model, ds):
        """install the (mean, std) of the normal class on an encoder that fuses it; returns a fallback callable for
        encoders that do not"""
        norm = getattr(ds, "normalize", None)
        enc = getattr(model, "feature_model", model)
        self._gcn = norm if isinstance(norm, GcnNormalize) else None
        if self._gcn is not None:
            # per-sample statistics: not expressible as the encoder's per-channel (mean, std); the step loop runs the operator
            if hasattr(enc, "set_normalize"):
                enc.set_normalize(None, None)
            return None
        if hasattr(enc, "set_normalize"):
            enc.set_normalize(*(norm if norm is not None else (None, None)))
            return None
        if norm is not None:
            raise NotImplementedError("this encoder has no fused normalise; add one to its first kernel")
        return None

    # the fp16 gradient scale (ops.set_grad_scale) follows the usual dynamic rule: halved when a step was dropped for non-finite
    # gradients, doubled again after SCALE_GROWTH_INTERVAL clean steps (never above SCALE_MAX or below 1).  The optimiser's device
    # counter is read every SCALE_POLL_EVERY steps and at the end of an epoch -- between an overflow and the next poll the steps
    # keep being dropped on the device, nothing non-finite reaches the weights or the moments.
    SCALE_POLL_EVERY, SCALE_GROWTH_INTERVAL, SCALE_MAX = 16, 2000, 65536.0

    def _move_grad_scale(self, opt, clean_steps: int, gstep: int, graphed):
        skipped = opt.skipped_steps() if hasattr(opt, "skipped_steps") else 0
        scale = ops.grad_scale()
        if skipped > 0:
            new = max(1.0, scale / 2.0)
            clean_steps = 0
        elif clean_steps >= self.SCALE_GROWTH_INTERVAL and 1.0 < scale < self.SCALE_MAX:
            new, clean_steps = scale * 2.0, 0
        else:
            return clean_steps, graphed
        if new != scale:
            ops.set_grad_scale(new)
            self.scale_events.append((gstep, new))
            self.logger.print(f"fp16 gradient scale {scale:g} -> {new:g} at step {gstep}" + (f" ({skipped} step(s) dropped)" if skipped else ""))
            graphed = None                   # a captured step has the old scale baked into its loss kernel: capture again
        return clean_steps, graphed

    def _exact_bn_for(self, model: torch.nn.Module) -> bool:
        if self.exact_bn is True or self.exact_bn is False:
            return bool(self.exact_bn)
        has_bn = any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model.modules())
        return has_bn and self.lr >= 1e-3

    def _log_preview(self, ds, name: str, percls: int, train: bool, seed: int):
        """the preview figure of a task's first seed (`ad_trainer.py:386-393, 486-493`); only with `previews=True` and an active logger"""
        if not (self.previews and seed == 0 and self.logger.active):
            return
        if not hasattr(ds, "preview"):
            raise NotImplementedError(f"previews=True needs a source with preview(); {type(ds).__name__} has none")
        prev, stats = ds.preview(percls, train)
        heads = [str(stats[k]) for k in sorted(stats)] if train else [f"{k}: {v}" for k, v in sorted(stats.items())]
        self.logger.logimg(name, prev, nrow=max(prev.shape[0] // len(stats), 1), rowheaders=heads)

    def _log_histograms(self, la: torch.Tensor, sc: torch.Tensor, tag0: str, tag1: str, step: int):
        """the histograms of the scores with label 0 and with label 1 (`histograms=True` only): kept and handed to the logger; a
        label without scores, or no scores at all, is skipped"""
        if sc.numel() == 0:
            return
        for tag, hist in zip((tag0, tag1), score_histograms(la, sc)):
            if hist is not None:
                self.histograms.setdefault(tag, {})[step] = hist
                self.logger.add_histogram(tag, hist, step)

    EXTREME_ROWS = ("nominal most", "nominal least", "anomalous most", "anomalous least")

    def _log_extremes(self, ds, la: torch.Tensor, sc: torch.Tensor, idc: np.ndarray, cls: int, clsstr: str, seed: int):
        """the k most and least anomalous test samples per label group (`extremes=k` only): kept, logged as JSON and, for a source
        with `test_images` under an active logger, as a picture of one row per non-empty list"""
        if sc.numel() == 0:
            return None
        ex = score_extremes(la, sc, self.n_extremes, indices=idc)
        self.extremes[f"eval_cls{cls}_it{seed}"] = ex
        self.logger.logjson(f"eval_cls{cls}_it{seed}_extremes", ex.as_dict())
        if not (self.logger.active and hasattr(ds, "test_images")):
            return ex
        rows, per, heads = self._extreme_rows(ex)
        if per:
            self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_extremes", ds.test_images(rows), nrow=per, rowheaders=heads)
        return ex

    def _extreme_rows(self, ex):
        """the extremes picture's cells: (dataset indices row by row, cells per row, row headers); per = 0 when every list is empty"""
        lists = [(name, pair[0], ex.num[g]) for name, g, pair in zip(self.EXTREME_ROWS, (0, 0, 1, 1),
                                                                    (ex.most[0], ex.least[0], ex.most[1], ex.least[1])) if len(pair[0])]
        if not lists:
            return np.zeros(0, np.int64), 0, []
        per = min(len(rows) for _, rows, _ in lists)
        return np.concatenate([rows[:per] for _, rows, _ in lists]), per, [f"{name}: {num}" for name, _, num in lists]

    def _check_breakdown_source(self, ds):
        """`breakdown=True` only: refuse at the start of an evaluation a source that has forgotten its test rows' classes"""
        if getattr(ds, "test_classes", None) is None:
            raise NotImplementedError(f"breakdown=True needs a source with test_classes (the test rows' original class ids, as the "
                                      f"sources of a LabelledImageSet carry them); {type(ds).__name__} has none")

    def _log_breakdown(self, ds, la: np.ndarray, sc: torch.Tensor, idc: np.ndarray, nominal: int, cls: int, seed: int):
        """the per-class breakdown of the test scores (`breakdown=True` only): kept, logged as JSON and as one text line"""
        if sc.numel() == 0:
            return None
        ids = np.asarray(ds.test_classes)[idc]
        names = getattr(ds, "classes", None) or getattr(self.dsstr, "classes", None) or self.classes
        bd = class_breakdown(sc, ids, np.unique(ids[la == nominal]), tpr=self.breakdown_tpr, names=names)
        self.breakdowns.setdefault(cls, []).append(bd)
        self.logger.logjson(f"eval_cls{cls}_it{seed}_breakdown", bd.to_json())
        hard = bd.hardest()
        if hard is not None:
            self.logger.logtxt(f'Eval: hardest class is {hard[0]} "{hard[1]}" with {hard[2] * 100:04.2f}% AUC against its pool; '
                               f'{bd.fpr_at_tpr * 100:04.2f}% FPR at {bd.tpr_level * 100:g}% TPR pooled (seed {seed}).')
        return bd

    @staticmethod
    def _nanmean(values) -> float:
        kept = [float(v) for v in values if v == v]
        return float(np.mean(kept)) if kept else float("nan")

    def _log_auc_ci(self, roc: ROC, la: np.ndarray, la_t: torch.Tensor, sc_t: torch.Tensor, cls: int, seed: int) -> str:
        """DeLong's interval of one evaluation's AUC (`auc_ci=level` only): attached to `roc`, logged as JSON, and returned as the
        tail of the `Eval:` text line.  While `run` has seeds to compare, the scores are kept where they are.  A NaN score costs the
        interval, not the run: one logged line, no attribute, no file."""
        try:
            test = delong(la_t, sc_t)                  # both classes are present: the caller has an AUC
        except ValueError as e:
            self.logger.logtxt(f"Eval: class {cls}, seed {seed}: no confidence interval of the AUC ({e}).")
            return ""
        (lo,), (hi,) = test.ci(self.auc_ci)
        roc.ci, roc.se, roc.var = (float(lo), float(hi)), float(test.se[0]), float(test.var[0])
        self.logger.logjson(f"eval_cls{cls}_it{seed}_auc_ci", test.to_json(self.auc_ci))
        if self._seed_scores is not None:
            self._seed_scores.append((seed, la, sc_t.detach().reshape(-1).float()))
        return f" {self.auc_ci * 100:g}% CI of the AUC [{lo * 100:04.2f}%, {hi * 100:04.2f}%]."

    def _compare_seeds(self, cls: int):
        """after a class's last seed (`auc_ci=level` only): the paired test of the seeds' AUCs over the shared test split"""
        kept, self._seed_scores = self._seed_scores or [], None
        if len(kept) < 2:
            return
        if len(kept) > DELONG_MAX_COLUMNS:
            self.logger.logtxt(f"Eval: class {cls}: comparing the first {DELONG_MAX_COLUMNS} of {len(kept)} seeds' AUCs.")
            kept = kept[:DELONG_MAX_COLUMNS]
        labels = kept[0][1]
        if any(not np.array_equal(la, labels) for _, la, _ in kept[1:]):
            self.logger.logtxt(f"Eval: class {cls}: the seeds' test labels differ; their AUCs are not compared.")
            return
        scores = [sc for _, _, sc in kept]
        test = delong(labels, scores if scores[0].is_cuda else torch.stack(scores).numpy())
        if test is None:
            return
        self.auc_tests[cls] = test
        self.logger.logjson(f"eval_cls{cls}_auc_compare", {"seeds": [s for s, _, _ in kept], **test.to_json(self.auc_ci)})

    def _log_bootstrap(self, roc: ROC, prc: PRC, la: np.ndarray, la_t: torch.Tensor, sc_t: torch.Tensor, cls: int, seed: int) -> str:
        """the bootstrap of one evaluation's AUC, AP and FPR at 95 % TPR (`bootstrap=B` only): kept, attached to `roc` and `prc`, logged
        as JSON, and returned as the tail of the `Eval:` text line.  While `run` has seeds to compare, the scores are kept where they
        are.  A NaN score costs the intervals, not the run: one logged line, no attribute, no file."""
        try:
            boot = bootstrap_stats(la_t, sc_t, self.bootstrap, self.bootstrap_seed)       # both classes are present: the caller has an AUC
        except ValueError as e:
            self.logger.logtxt(f"Eval: class {cls}, seed {seed}: no bootstrap intervals ({e}).")
            return ""
        level = self.bootstrap_level
        (alo,), (ahi,) = boot.ci(level, "auc")
        (lo,), (hi,) = boot.ci(level, "ap")
        roc.boot_ci = (float(alo), float(ahi))
        prc.ci, prc.se = (float(lo), float(hi)), float(boot.se("ap")[0])
        self.bootstraps.setdefault(cls, {})[seed] = boot
        self.logger.logjson(f"eval_cls{cls}_it{seed}_bootstrap", boot.to_json(level))
        if self._boot_scores is not None:
            self._boot_scores.append((seed, la, sc_t.detach().reshape(-1).float()))
        return f" {level * 100:g}% bootstrap CI of the AP [{lo * 100:04.2f}%, {hi * 100:04.2f}%]."

    def _compare_seeds_bootstrap(self, cls: int):
        """after a class's last seed (`bootstrap=B` only): the seeds' scores under one set of replicates over the shared test split"""
        kept, self._boot_scores = self._boot_scores or [], None
        if len(kept) < 2:
            return
        if len(kept) > BOOTSTRAP_MAX_COLUMNS:
            self.logger.logtxt(f"Eval: class {cls}: comparing the first {BOOTSTRAP_MAX_COLUMNS} of {len(kept)} seeds by bootstrap.")
            kept = kept[:BOOTSTRAP_MAX_COLUMNS]
        labels = kept[0][1]
        if any(not np.array_equal(la, labels) for _, la, _ in kept[1:]):
            self.logger.logtxt(f"Eval: class {cls}: the seeds' test labels differ; they are not compared by bootstrap.")
            return
        scores = [sc for _, _, sc in kept]
        boot = bootstrap_stats(labels, scores if scores[0].is_cuda else torch.stack(scores).numpy(), self.bootstrap, self.bootstrap_seed)
        if boot is None:
            return
        self.logger.logjson(f"eval_cls{cls}_bootstrap_compare", {"seeds": [s for s, _, _ in kept], **boot.to_json(self.bootstrap_level)})

    def breakdown_matrix(self) -> np.ndarray:
        """float64 [no_classes, no_classes]: entry [c, k] is the mean over the seeds of the AUC of task c against class k
        (`breakdown=True`; `self.breakdowns`), NaN where no seed has one: a task that did not run, a class that is not among the
        trainer's classes' indices or not in the test split, a class whose pool was empty."""
        n_cls = len(self.classes)
        cells = [[[] for _ in range(n_cls)] for _ in range(n_cls)]
        for c, per_seed in self.breakdowns.items():
            for bd in per_seed:
                for k, auc in zip(bd.classes, bd.auc):
                    if 0 <= c < n_cls and 0 <= k < n_cls:
                        cells[c][int(k)].append(auc)
        return np.array([[self._nanmean(cell) for cell in row] for row in cells], dtype=np.float64).reshape(n_cls, n_cls)

    def _test_time_inputs(self, imgs: torch.Tensor, lbls: torch.Tensor, nominal: int) -> torch.Tensor:
        """the test-time steps between the loader and the encoder (`ad_trainer.py:501-505`): the test MSMs, then GCN"""
        if self.msms:
            imgs = apply_msms(imgs, lbls, self.msms, "test", nominal)
        if self._gcn is not None:
            imgs = self._gcn(imgs)
        return imgs

    EXPLAIN_ALPHA = 0.6

    def _check_explainable(self, model, ds, option: str = "explain",
                           why: str = "whose patch embedding could hand a gradient back to the pixels"):
        """`explain=True` / `attention=True` only: refuse at the start of an evaluation what its end could not explain"""
        from .. import explain
        from ..models.clip_vit import VisualTransformer
        if not hasattr(ds, "test_inputs"):
            raise NotImplementedError(f"{option}=True needs a source with test_inputs(rows); {type(ds).__name__} has none")
        if option == "cam":
            explain._wide_resnet(model, "cam=True")          # NotImplementedError without one
            return
        if any(isinstance(m, VisualTransformer) for m in model.modules()):
            return
        # the BatchNorm CNNs (CNN32, CNN28) hand an input gradient back through their first convolution; they have no attention
        if option == "explain" and explain._batchnorm_cnn(model, "explain=True"):
            return
        raise NotImplementedError(f"{option}=True needs a ViT encoder{' or a CNN32 / CNN28' if option == 'explain' else ''}: "
                                  f"{type(model).__name__} has no VisualTransformer {why}")

    def _log_attention(self, model, ds, ex, nominal: int, cls: int, clsstr: str, seed: int):
        """attention-rollout maps of the extremes picture's rows (`attention=True` only): kept, and logged as a picture under an active logger"""
        from .. import explain
        rows, per, heads = self._extreme_rows(ex)
        if not per:
            return
        imgs, lbls, _ = ds.test_inputs(rows)
        imgs = self._test_time_inputs(imgs.to(self.device), lbls, nominal)
        maps = explain.attention_rollout(model, imgs)
        self.attention_maps[f"eval_cls{cls}_it{seed}"] = maps
        if self.logger.active and hasattr(ds, "test_pictures"):
            attn = explain.overlay(maps, ds.test_pictures(rows), self.EXPLAIN_ALPHA)
            self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_extremes_attn", attn, nrow=per, rowheaders=heads)

    def _log_cams(self, model, ds, ex, center, nominal: int, cls: int, clsstr: str, seed: int):
        """Grad-CAM maps of the extremes picture's rows (`cam=True` only): kept, and logged as a picture under an active logger"""
        from .. import explain
        rows, per, heads = self._extreme_rows(ex)
        if not per:
            return
        imgs, lbls, _ = ds.test_inputs(rows)
        imgs = self._test_time_inputs(imgs.to(self.device), lbls, nominal)
        prev_scale = ops.grad_scale()
        try:
            ops.set_grad_scale(ops.default_grad_scale())          # as in training: the 16-bit dY chain of fp16 compute must not underflow
            maps = explain.grad_cam(model, imgs, explain.score_fn(self, center, nominal), layer=self.cam_layer, mode=self.cam_mode)
        finally:
            ops.set_grad_scale(prev_scale)
        self.cams[f"eval_cls{cls}_it{seed}"] = maps
        if self.logger.active and hasattr(ds, "test_pictures"):
            cam = explain.overlay(maps, ds.test_pictures(rows), self.EXPLAIN_ALPHA)
            self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_extremes_cam", cam, nrow=per, rowheaders=heads)

    def _log_explanations(self, model, ds, ex, center, nominal: int, cls: int, clsstr: str, seed: int):
        """heat maps of the extremes picture's rows (`explain=True` only): kept, and logged as a second picture under an active logger"""
        from .. import explain
        from ..models.clip_vit import VisualTransformer
        rows, per, heads = self._extreme_rows(ex)
        if not per:
            return
        imgs, lbls, _ = ds.test_inputs(rows)
        imgs = self._test_time_inputs(imgs.to(self.device), lbls, nominal)
        vit = next((m for m in model.modules() if isinstance(m, VisualTransformer)), None)
        patch = vit.patch_size if vit is not None else None          # a ViT's maps are patch-level, a CNN's pixel-level
        prev_scale = ops.grad_scale()
        try:
            ops.set_grad_scale(ops.default_grad_scale())          # as in training: the 16-bit dY chain of fp16 compute must not underflow
            grad = explain.input_gradient(model, imgs, explain.score_fn(self, center, nominal))
        finally:
            ops.set_grad_scale(prev_scale)
        maps = explain.saliency(grad, mode="max", pool=patch)
        self.explanations[f"eval_cls{cls}_it{seed}"] = maps
        if self.logger.active and hasattr(ds, "test_pictures"):
            # the pictures in ToTensor's scale, which overlay reads as 255 x: test_images(rows) carries the source's Normalize
            heat = explain.overlay(maps, ds.test_pictures(rows), self.EXPLAIN_ALPHA)
            self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_extremes_heat", heat, nrow=per, rowheaders=heads)

    def _check_embedding(self, model, ds, nominal: int, what: str = None):
        """`neighbors=k` and `mahalanobis_baseline=True` only: refuse at the start of an evaluation a model without a feature output
        (one test image is embedded; a source without `test_inputs` gives the first normal training image)"""
        if hasattr(ds, "test_inputs"):
            imgs, lbls, _ = ds.test_inputs([0])
        else:
            imgs = ds.normal_inputs([0])[0]
            lbls = torch.full((imgs.shape[0],), nominal, dtype=torch.int64)
        with torch.no_grad():
            out = model(self._test_time_inputs(imgs.to(self.device), lbls, nominal))
        width = out.reshape(out.shape[0], -1).shape[1]
        if width < 2:
            what = what or f"neighbors={self.n_neighbors} searches the encoder's feature space"
            raise NotImplementedError(f"{what}: a classifier head has no embedding; use an objective with a feature output")
        return width

    def _normal_features(self, model, ds, nominal: int, kept: dict):
        """(features fp32 [n_normal, D], dataset indices) of ALL normal training images under the test transform, embedded in batches
        of the trainer's size; `kept` holds them for the evaluation that asked, so that `neighbors` and `mahalanobis_baseline` embed
        them once"""
        if "feats" not in kept:
            from .. import neighbors as knn
            n_normal = ds.n_normal
            normal_ids = []

            def normal_batches():
                for lo in range(0, n_normal, self.batch_size):
                    imgs, ids = ds.normal_inputs(torch.arange(lo, min(lo + self.batch_size, n_normal)))
                    normal_ids.append(ids)
                    yield imgs, torch.full((imgs.shape[0],), nominal, dtype=torch.int64)

            kept["feats"] = knn.embed(model, normal_batches(), trainer=self, nominal=nominal)
            kept["ids"] = torch.cat(normal_ids).cpu().numpy()
        return kept["feats"], kept["ids"]

    def _log_mahalanobis(self, model, ds, la_t, test_feats, nominal: int, cls: int, seed: int, clsstr: str, kept: dict):
        """the Gaussian baseline (`mahalanobis_baseline=True` only): mean and shrunk covariance of the normal training features, the
        Mahalanobis distance of the test features, its AUC and AP"""
        from .. import mahalanobis as mh
        if not (int((la_t == 0).sum()) > 0 and int((la_t == 1).sum()) > 0):          # nothing to rank: embed and fit nothing
            return
        refs, _ = self._normal_features(model, ds, nominal, kept)
        gauss = mh.fit_gaussian(refs, shrinkage=self.mahalanobis_shrinkage)
        score = mh.mahalanobis_score(mh.mahalanobis(test_feats, gauss))
        la = la_t.to(score.device)
        if score.is_cuda:
            auc, ap = auc_ap_device(la, score)
        else:
            auc, ap = roc_auc(la.numpy(), score.numpy()), average_precision(la.numpy(), score.numpy())
        res = {"shrinkage": float(gauss.shrinkage), "auc": float(auc), "avg_prec": float(ap), "n_normal": int(gauss.n),
               "D": int(refs.shape[1]), "nonfinite": int(gauss.nonfinite)}
        self.mahalanobis_results[cls] = res
        self.logger.logjson(f"eval_cls{cls}_it{seed}_mahalanobis", res)
        self.logger.logtxt(f'Eval: class "{clsstr}" (seed {seed}) (Mahalanobis baseline: {auc * 100:04.2f}% AUC)')

    def _log_coreset(self, ds, refs, normal_ids, cls: int, clsstr: str, seed: int):
        """the greedy k-center coreset of the normal features (`knn_coreset=m` only), kept and logged: (the `Coreset`, its centres as
        rows of `refs`, on the device of `refs`)"""
        from .. import coreset
        n = int(refs.shape[0])
        m = self.knn_coreset if isinstance(self.knn_coreset, int) else int(math.ceil(self.knn_coreset * n))
        cs = coreset.kcenter(refs, max(1, min(n, max(m, self.n_neighbors))), 0)
        self.coresets[f"eval_cls{cls}_it{seed}"] = cs
        self.logger.logjson(f"eval_cls{cls}_it{seed}_coreset", cs.as_dict(ref_ids=normal_ids))
        centres = cs.idx[cs.idx >= 0]
        if self.logger.active and hasattr(ds, "normal_pictures"):
            self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_coreset", ds.normal_pictures(centres[:32].cpu()).float())
        return cs, centres

    def _log_neighbors(self, model, ds, ex, la_t, test_feats, nominal: int, cls: int, clsstr: str, seed: int, kept: dict):
        """the k nearest normal training images of the extremes picture's rows in feature space (`neighbors=k` only): kept, logged
        as JSON and, under an active logger with `normal_pictures`, as a picture of each row's image followed by its neighbours;
        with `knn_baseline=True` also the k-NN score of the whole test split against the same normal features"""
        from .. import neighbors as knn
        k = self.n_neighbors
        rows, per, _ = self._extreme_rows(ex)
        if not per:
            return
        n_normal = ds.n_normal
        refs, normal_ids = self._normal_features(model, ds, nominal, kept)
        queries = knn.embed(model, [ds.test_inputs(rows)[:2]], trainer=self, nominal=nominal)
        cs = centres = None
        if self.knn_coreset:
            cs, centres = self._log_coreset(ds, refs, normal_ids, cls, clsstr, seed)
            refs = refs[centres]
        neigh = knn.feature_knn(queries, refs, k)
        if centres is not None:                             # rows of the coreset -> normal rows, as without it
            neigh.idx = torch.where(neigh.idx >= 0, centres[neigh.idx.clamp(min=0)], neigh.idx)
        self.neighbors[f"eval_cls{cls}_it{seed}"] = neigh
        self.logger.logjson(f"eval_cls{cls}_it{seed}_extremes_neighbors", neigh.as_dict(row_ids=rows, ref_ids=normal_ids))
        if self.logger.active and hasattr(ds, "test_pictures") and hasattr(ds, "normal_pictures"):
            own = ds.test_pictures(rows)
            idx = neigh.idx.cpu()
            near = ds.normal_pictures(idx.clamp(min=0).reshape(-1))
            if near.shape[1:] == own.shape[1:]:
                near = near.reshape(len(rows), k, *own.shape[1:]) * (idx >= 0).to(near.device, near.dtype).reshape(len(rows), k, 1, 1, 1)
                cells = torch.cat([own.unsqueeze(1), near], dim=1).reshape(-1, *own.shape[1:]).float()
                self.logger.logimg(f"eval_cls{cls}-{clsstr}_it{seed}_extremes_neighbors", cells, nrow=k + 1)
        if not self.with_knn_baseline or test_feats is None:
            return
        score = knn.knn_score(knn.feature_knn(test_feats, refs, k), "mean")
        la = la_t.to(score.device)
        if not (int((la == 0).sum()) > 0 and int((la == 1).sum()) > 0):
            return
        if score.is_cuda:
            auc, ap = auc_ap_device(la, score)
        else:
            auc, ap = roc_auc(la.numpy(), score.numpy()), average_precision(la.numpy(), score.numpy())
        res = {"k": k, "auc": float(auc), "avg_prec": float(ap), "n_normal": int(n_normal), "D": int(refs.shape[1])}
        if cs is not None:
            res["coreset"] = {"m": int(centres.numel()), "n": cs.n, "cover": cs.cover()}
        self.knn_results[cls] = res
        self.logger.logjson(f"eval_cls{cls}_it{seed}_knn", res)
        self.logger.logtxt(f'Eval: class "{clsstr}" (seed {seed}) (k-NN baseline: {auc * 100:04.2f}% AUC)')

    def make_optimizer(self, model: torch.nn.Module):
        """Adam for every encoder (ad_trainer.py:383); the CLIP objective overrides this with SGD-Nesterov (:380-381)"""
        return FusedAdam(model.parameters(), lr=self.lr, weight_decay=self.wdk, amsgrad=False)

    def train_cls(self, model: torch.nn.Module, ds, cls: int, clsstr: str, seed: int,
                  load: Union[torch.nn.Module, str] = None):
        """the inner loop, `ad_trainer.py:356-471`; returns (model on the CPU in eval mode, training ROC)"""
        model = model.to(self.device).train()
        epochs = self.epochs
        cls_roc = None
        opt = self.make_optimizer(model)                                                              # :380-383
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, self.milestones, 0.1)                       # :384
        self._msm_source(ds)
        loader, _ = ds.loaders(self.batch_size, num_workers=self.workers, persistent=True)              # :385
        self._log_preview(ds, f"training_cls{cls}-{clsstr}_preview", 40, True, seed)                      # :386-393
        ep = self.load(load if isinstance(load, str) else None, model, opt, sched)                      # :396
        center = self.center = self.prepare_metric(clsstr, loader, model, seed)                         # :397
        self._normalize_hook(model, ds)
        rank, world = 0, 1
        arena = comm = None
        nominal = getattr(ds, "nominal_label", 0)
        self.last_losses = []
        self.last_scores = []                               # per epoch: (labels, scores) of every step batch, in order, on the device
        self.scale_events = []                              # (global step, new scale) whenever the fp16 gradient scale moved
        graphed = None                                      # (batch shape, GraphedStep) of the full-size step batch
        # process-wide state this loop changes (gradient scale, wgrad launch form, BatchNorm hook) is restored on every way out
        prev_scale = ops.grad_scale()
        prev_parity = ops.parity_mode()
        try:
            ops.set_parity_mode(self._exact_bn_for(model) or prev_parity)
            # fp16 compute: scale the loss gradient so that the 16-bit backward chain does not underflow (ops.set_grad_scale); the
            # optimiser un-scales, drops a step whose gradients overflowed (optim._NonFiniteGuard) and this loop moves the scale
            ops.set_grad_scale(ops.default_grad_scale())
            clean_steps, gstep = 0, 0
            if self.data_parallel and torch.distributed.is_initialized():
                rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
                # on RCCL: the library's own communicator (side HIP stream, reduce-scatter + all-gather, BatchNorm sums inside the
                # library); gloo rehearsals: torch.distributed collectives (parallel.make_comm)
                comm, _ = parallel.make_comm()
                arena = parallel.GradArena(model, comm=comm)
                arena.install_hooks()
                if any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model.modules()):
                    # the reference's BatchNorm layers see the whole step batch: keep that meaning across the ranks
                    if self.sync_bn:
                        parallel.enable_sync_bn(comm=comm)
                    elif rank == 0:
                        self.logger.warning("data parallel training of a BatchNorm encoder with sync_bn=False: batch statistics are per "
                                            "rank, not those of the single-device full batch (eoe_amd/parallel.py)")
            for ep in range(ep, epochs):
                ep_labels, ep_scores, ep_losses = [], [], []
                for batch in loader:                                                                    # :410
                    imgs, lbls = batch[0], batch[1]
                    n_norm = int((lbls == nominal).sum())
                    n_glob = lbls.shape[0]
                    inv_count, keep_scores = 1.0 / n_glob, True
                    if world > 1:
                        halves = [h for h in (n_norm, n_glob - n_norm) if h > 0]
                        if min(halves) >= world:
                            rows = parallel.shard_rows(n_norm, n_glob - n_norm, rank, world)
                            imgs, lbls = imgs[rows], lbls[rows]
                        else:
                            # a ragged last batch with fewer rows than ranks in one half (no drop_last, bases.py:231-235): every
                            # rank computes the whole batch, weighted 1 / world, so that the summed gradient is the full-batch
                            # one and all ranks issue the same collectives; rank 0 alone reports its scores
                            inv_count, keep_scores = 1.0 / (n_glob * world), rank == 0
                    imgs = imgs.to(self.device, non_blocking=True)                                      # :411
                    lbls = lbls.to(self.device, non_blocking=True)                                      # :412
                    if self.msms:                                                                       # :413-425
                        imgs = apply_msms(imgs, lbls, self._step_msms, "train", nominal)
                    if self._gcn is not None:                                                           # :415-425, after the MSMs
                        imgs = self._gcn(imgs)                # a graphed step below gets the normalised batch
                    opt.zero_grad()                                                                     # :428
                    if self.graph_steps and world == 1 and graphed is None:
                        from ..graph import GraphedStep
                        graphed = (tuple(imgs.shape), GraphedStep(
                            model, lambda f, y: self.loss(f, y, center, inputs=None, nominal_label=nominal, inv_count=inv_count),
                            lambda f: self.compute_anomaly_score(f, center, inputs=None, nominal_label=nominal), imgs, lbls))
                    if graphed is not None and graphed[0] == tuple(imgs.shape):
                        loss, scores = graphed[1](imgs, lbls)                                           # :429-431,434 replayed
                        opt.step()                                                                      # :432
                        loss, scores = loss.detach().clone(), scores.detach().clone()                   # static graph outputs
                    else:
                        feats = model(imgs)                                                             # :429
                        loss = self.loss(feats, lbls, center, inputs=imgs, nominal_label=nominal,
                                         inv_count=inv_count)                                           # :430
                        loss.backward()                                                                 # :431
                        if arena is not None:
                            arena.finish()
                        opt.step()                                                                      # :432
                        opt.zero_grad()                                                                 # :433
                        scores = self.compute_anomaly_score(feats, center, inputs=imgs, nominal_label=nominal)   # :434
                    if keep_scores:
                        ep_labels.append(lbls)
                        ep_scores.append(scores.detach().reshape(-1))
                    ep_losses.append(loss.detach())
                    gstep += 1
                    clean_steps += 1
                    if gstep % self.SCALE_POLL_EVERY == 0:
                        clean_steps, graphed = self._move_grad_scale(opt, clean_steps, gstep, graphed)
                clean_steps, graphed = self._move_grad_scale(opt, clean_steps, gstep, graphed)
                # ---- epoch tail (:447-469): one host copy per epoch
                la = torch.cat(ep_labels) if ep_labels else torch.zeros(0, dtype=torch.int64, device=self.device)
                sc = torch.cat(ep_scores) if ep_scores else torch.zeros(0, dtype=torch.float32, device=self.device)
                ls = torch.stack(ep_losses)
                if world > 1:
                    la, sc = parallel.all_gather_1d(la), parallel.all_gather_1d(sc)
                    torch.distributed.all_reduce(ls)          # local losses are already divided by the global batch
                self.last_losses.extend(ls.cpu().tolist())
                self.last_scores.append((la, sc))
                if bool(torch.isnan(sc).any()):
                    raise NanGradientsError()                                                           # :448-449
                if self.with_histograms:                                                                # :458-465
                    self._log_histograms(la, sc, f"Training: CLS{cls} SEED{seed} anomaly_scores normal",
                                         f"Training: CLS{cls} SEED{seed} anomaly_scores anomalous", ep)
                if bool((la == 1).any()):
                    # the epoch's AUC from the GPU-resident scores (eoe_auc_ap: exact pair counts), no host copy of the scores
                    cls_roc = ROC(auc_ap_device(la, sc)[0] if sc.is_cuda else roc_auc(la.cpu().numpy(), sc.cpu().numpy()))   # :452-455
                    if self.with_curves:                          # every epoch, as the reference: the last one with anomalies is returned
                        cls_roc.fpr, cls_roc.tpr, cls_roc.ths = roc_curve(la if sc.is_cuda else la.cpu().numpy(),
                                                                          sc if sc.is_cuda else sc.cpu().numpy())
                sched.step()                                                                            # :468
        finally:
            ops.set_grad_scale(prev_scale)
            ops.set_parity_mode(prev_parity)
            if arena is not None:
                parallel.disable_sync_bn()
                arena.remove_hooks()
                for p in model.parameters():
                    if hasattr(p, "_eoe_grad_buf"):
                        del p._eoe_grad_buf
            if comm is not None:
                comm.close()
        return model.cpu().eval(), cls_roc                                                              # :471

    def eval_cls(self, model: torch.nn.Module, ds, cls: int, clsstr: str, seed: int):
        """forward-only scoring of the test split, `ad_trainer.py:473-550`"""
        model = model.to(self.device).eval()
        if self.with_explain:
            self._check_explainable(model, ds)
        if self.with_attention:
            self._check_explainable(model, ds, "attention", "whose attention could be rolled out")
        if self.with_cam:
            self._check_explainable(model, ds, "cam", "")
        if self.with_breakdown:
            self._check_breakdown_source(ds)
        if self.n_neighbors > 0:
            for need in ("test_inputs", "normal_inputs"):
                if not hasattr(ds, need):
                    raise NotImplementedError(f"neighbors={self.n_neighbors} needs a source with {need}(rows); {type(ds).__name__} has none")
        if self.with_mahalanobis and not hasattr(ds, "normal_inputs"):
            raise NotImplementedError(f"mahalanobis_baseline=True needs a source with normal_inputs(rows); {type(ds).__name__} has none")
        self._msm_source(ds)
        _, loader = ds.loaders(self.batch_size, num_workers=self.workers, shuffle_test=False)
        self._log_preview(ds, f"eval_cls{cls}-{clsstr}_preview", 20, False, seed)                         # :486-493
        self._normalize_hook(model, ds)
        center = self.center
        nominal = getattr(ds, "nominal_label", 0)
        if self.n_neighbors > 0:
            self._check_embedding(model, ds, nominal)
        if self.with_mahalanobis:
            from ..mahalanobis import MAHALANOBIS_MAX_D
            width = self._check_embedding(model, ds, nominal, "mahalanobis_baseline=True fits a Gaussian in the encoder's feature space")
            if width > MAHALANOBIS_MAX_D:
                raise NotImplementedError(f"mahalanobis_baseline=True fits a Gaussian in at most {MAHALANOBIS_MAX_D} dimensions; the "
                                          f"model's features have {width}")
        ep_labels, ep_scores, ep_idcs, ep_feats = [], [], [], []
        normal_kept = {}                               # the normal training features, embedded at most once (_normal_features)
        prev_parity = ops.parity_mode()
        ops.set_parity_mode(self._exact_bn_for(model) or prev_parity)      # scored in the arithmetic it was trained in
        try:
            for batch in loader:
                imgs, lbls = batch[0].to(self.device), batch[1]
                imgs = self._test_time_inputs(imgs, lbls, nominal)                                      # :501-505
                with torch.no_grad():
                    feats = model(imgs)
                ep_scores.append(self.compute_anomaly_score(feats, center, inputs=imgs, nominal_label=nominal))
                if self.with_knn_baseline or self.with_mahalanobis:
                    ep_feats.append(feats.detach().reshape(feats.shape[0], -1).float())
                ep_labels.append(lbls)
                ep_idcs.append(batch[2] if len(batch) > 2 else torch.arange(len(lbls)))
        finally:
            ops.set_parity_mode(prev_parity)
        la_t, sc_t = torch.cat(ep_labels), torch.cat(ep_scores).reshape(-1)
        la = la_t.cpu().numpy()
        sc = sc_t.cpu().numpy()                        # host copy only for the per-sample score log below
        idc = torch.cat(ep_idcs).cpu().numpy()
        if (la == 0).sum() > 0 and (la == 1).sum() > 0:
            if sc_t.is_cuda:                           # AUC / AP on the device (ad_trainer.py:517-521)
                auc, ap = auc_ap_device(la_t, sc_t)
            else:
                auc, ap = roc_auc(la, sc), average_precision(la, sc)
            cls_roc, cls_prc = ROC(auc), PRC(ap)
            if self.with_curves:                       # one eoe_rank_curves call serves both (ad_trainer.py:517, 520)
                if sc_t.is_cuda:
                    (cls_roc.fpr, cls_roc.tpr, cls_roc.ths), (cls_prc.prec, cls_prc.rec, cls_prc.ths) = curves_device(la_t, sc_t)
                else:
                    cls_roc.fpr, cls_roc.tpr, cls_roc.ths = roc_curve(la, sc)
                    cls_prc.prec, cls_prc.rec, cls_prc.ths = precision_recall_curve(la, sc)
            interval = self._log_auc_ci(cls_roc, la, la_t, sc_t, cls, seed) if self.auc_ci is not None else ""
            if self.bootstrap is not None:
                interval += self._log_bootstrap(cls_roc, cls_prc, la, la_t, sc_t, cls, seed)
            self.logger.logtxt(f'Eval: class "{clsstr}" yields {cls_roc.auc * 100:04.2f}% AUC and '
                               f'{cls_prc.avg_prec * 100:04.2f}% average precision (seed {seed}).' + interval)
        else:
            cls_roc = cls_prc = None
        if self.with_breakdown:
            self._log_breakdown(ds, la, sc_t, idc, nominal, cls, seed)
        if self.with_histograms:                                                                        # :541-546
            self._log_histograms(la_t, sc_t, f"Eval: (SD{seed}) anomaly_scores cls{cls} nominal",
                                 f"Eval: (SD{seed}) anomaly_scores cls{cls} anomalous", 0)
        self.logger.logjson(f"eval_cls{cls}_it{seed}_anomaly_scores", {int(k): float(v) for k, v in zip(idc, sc)})
        if self.n_extremes > 0:
            ex = self._log_extremes(ds, la_t, sc_t, idc, cls, clsstr, seed)
            if self.with_explain and ex is not None:
                self._log_explanations(model, ds, ex, center, nominal, cls, clsstr, seed)
            if self.with_attention and ex is not None:
                self._log_attention(model, ds, ex, nominal, cls, clsstr, seed)
            if self.with_cam and ex is not None:
                self._log_cams(model, ds, ex, center, nominal, cls, clsstr, seed)
            if self.n_neighbors > 0 and ex is not None:
                self._log_neighbors(model, ds, ex, la_t, torch.cat(ep_feats) if ep_feats else None, nominal, cls, clsstr, seed, normal_kept)
        if self.with_mahalanobis and ep_feats:
            self._log_mahalanobis(model, ds, la_t, torch.cat(ep_feats), nominal, cls, seed, clsstr, normal_kept)
        model.cpu()
        return cls_roc, cls_prc

    # ------------------------------------------------------------------------------------------- snapshots
    def load(self, path: str, model: torch.nn.Module, opt=None, sched=None) -> int:
        """restore a snapshot file into (model, opt, sched) and return the epoch to resume from (`ad_trainer.py:552-598`).
        Two layouts are understood (`unify_snapshot_style`): the trainer's own {net, opt, sched, epoch, ...} and a bare
        state_dict, which is taken as pre-trained encoder weights of a `CustomNet`.  With or without a file, a model that can
        freeze its encoder does so here -- this is where the reference applies `freeze_parts` (:593-596)."""
        epoch = 0
        if path is not None:
            snap = self._read_snapshot(path)
            encoder_weights = snap.get("feature_model")
            if encoder_weights is not None:
                if not hasattr(model, "load_feature_model_weights"):
                    raise ValueError(f"{path} holds encoder weights for a CustomNet, but the model to train is a "
                                     f"{type(model).__name__}, which has no feature model to load them into.")
                model.load_feature_model_weights(encoder_weights)
            for key, target in (("net", model), ("opt", opt), ("sched", sched)):
                state = snap.get(key)
                if state is not None and target is not None:
                    target.load_state_dict(state)
            epoch = snap.get("epoch") or 0
        if hasattr(model, "freeze_parts"):
            model.freeze_parts()
        return epoch

    def load_ds_statistics(self, path: str) -> Optional[dict]:
        """the normalisation statistics a snapshot was trained with (`ad_trainer.py:600-603`); None for a file without any"""
        if path is None:
            return None
        return self._read_snapshot(path).get("ds_statistics")

    def _read_snapshot(self, path: str) -> dict:
        """the unified snapshot dict of a file: the read `run` keeps for the (class, seed) pair it is working on, else a fresh one"""
        kept = getattr(self, "_snapshot_read", None)
        if kept is not None and kept[0] == path:
            return kept[1]
        return self.unify_snapshot_style(torch.load(path, map_location="cpu"))

    def unify_snapshot_style(self, snapshot: dict) -> dict:
        """map both accepted file layouts onto one dict (`ad_trainer.py:608-615`)"""
        if isinstance(snapshot.get("net"), dict):
            return snapshot
        if snapshot and all(torch.is_tensor(v) for v in snapshot.values()):
            return {"feature_model": snapshot}
        raise ValueError("unrecognised snapshot layout: neither a trainer snapshot with a 'net' state_dict nor a bare state_dict")

    # ------------------------------------------------------------------------------------------- objective hooks
    @abstractmethod
    def prepare_metric(self, cstr: str, loader, model: torch.nn.Module, seed: int, **kwargs) -> torch.Tensor:
        pass

    @abstractmethod
    def compute_anomaly_score(self, features: torch.Tensor, center: torch.Tensor, **kwargs) -> torch.Tensor:
        pass

    @abstractmethod
    def loss(self, features: torch.Tensor, labels: torch.Tensor, center: torch.Tensor, **kwargs) -> torch.Tensor:
        pass
