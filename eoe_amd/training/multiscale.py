"""`multiscale_experiment` of the reference (`src/eoe/main/__init__.py:485-550`, the paper's Appendix C): the full class x seed
training once per MSM magnitude, one trainer per magnitude.  When every MSM filters a test part only, the magnitudes other than 0
do not train: they evaluate the magnitude-0 models (0 epochs)."""
from typing import Callable, List, Sequence

from ..msm import DS_PARTS, MSM
from .ad_trainer import ADTrainer


def multiscale_experiment(make_trainer: Callable[[List[MSM], int], ADTrainer], msms: Sequence[MSM],
                          magnitudes: Sequence[int] = (0, 1, 2, 4, 8, 16, 32), classes: List[int] = None,
                          iterations: int = 1, logger=None) -> dict:
    """`make_trainer(msms, magnitude)` builds the trainer of one magnitude (the reference's `create_trainer` with
    `msm=[msm.set_magnitude(magnitude) ...]`); returns {magnitudes, aucs, stds, ms_mode}"""
    test_only = all(m.ds_part not in (DS_PARTS["train_nominal"], DS_PARTS["train_oe"]) for m in msms)
    aucs, magn0_models = [], None
    for magnitude in magnitudes:
        cur = [m.set_magnitude(magnitude) for m in msms]
        trainer = make_trainer(cur, magnitude)
        if magnitude != 0 and test_only:
            trainer.epochs = 0
            _, results = trainer.run(classes, iterations, magn0_models)
        else:
            # the test-only case evaluates these models again at every other magnitude: keep them in RAM for this run only
            keep = ADTrainer.KEEP_SNAPSHOT_IN_RAM
            ADTrainer.KEEP_SNAPSHOT_IN_RAM = keep or (test_only and magnitude == 0)
            try:
                models, results = trainer.run(classes, iterations)
            finally:
                ADTrainer.KEEP_SNAPSHOT_IN_RAM = keep
            if magnitude == 0:
                magn0_models = models
        aucs.append((results["mean_auc"], results["std_auc"]))
    for s, (a, std) in zip(magnitudes, aucs):
        msg = f"{list(msms)} with magnitude={s:02d} yielded {a * 100:04.2f} +- {std * 100:04.2f}."
        if logger is not None:
            logger.print(msg)
    results = {"magnitudes": list(magnitudes), "aucs": [a for a, _ in aucs], "stds": [s for _, s in aucs],
               "ms_mode": [repr(m) for m in msms]}
    if logger is not None:
        logger.logjson("results", results)
    return results
