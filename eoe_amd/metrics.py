"""Epoch-tail metrics of the trainer (`src/eoe/training/ad_trainer.py:452-455,516-522`): the reference calls
sklearn's `roc_curve` + `auc` (trapezoid) and `average_precision_score` on host copies of the epoch's labels and
scores.  Same place (host, once per epoch), written as the tie-aware rank statistic, which equals the trapezoidal
ROC area, and the step-wise precision-recall sum.

The curves themselves (`roc_curve`, `precision_recall_curve` below) come from one table of exact integer counts per distinct
score -- `eoe_rank_curves` for GPU tensors, a sort for host arrays -- and sklearn's finishing steps in float64 on the host."""
import numpy as np

CURVES_MAX_N = 1 << 20            # eoe_rank_curves


class ROC:
    """container mirroring `src/eoe/utils/logger.py:36-62`.  `ROC(auc, std, n)` keeps the score alone, as the trainer does unless
    it is asked for curves; the keyword-only `tpr`, `fpr`, `ths` hold the curve (the reference's first three arguments)."""

    def __init__(self, auc: float, std: float = None, n: int = -1, *, tpr=None, fpr=None, ths=None):
        self.auc, self.std, self.n = auc, std, n
        self.tpr, self.fpr, self.ths = tpr, fpr, ths

    def get_x(self):
        return self.fpr

    def get_y(self):
        return self.tpr

    def get_score(self):
        return self.auc


class PRC:
    """container mirroring `src/eoe/utils/logger.py:65-91`; `prec`, `rec`, `ths` hold the curve"""

    def __init__(self, avg_prec: float, std: float = None, n: int = -1, *, prec=None, rec=None, ths=None):
        self.avg_prec, self.std, self.n = avg_prec, std, n
        self.prec, self.rec, self.ths = prec, rec, ths

    def get_x(self):
        return self.rec

    def get_y(self):
        return self.prec

    def get_score(self):
        return self.avg_prec


def mean_plot(results):
    """the "mean" of several ROCs or PRCs (`logger.py:94-122`): every curve is thinned to the shortest one's length by
    `sorted(np.random.choice(len, shortest, replace=False))` -- one draw per curve, in list order, from the global `np.random`
    state, exactly the reference's -- and the thinned arrays are averaged point by point; the score is the mean of the scores, `std`
    their standard deviation, `n` their number.  None for an empty list or one that holds a None."""
    if results is None or len(results) == 0 or any(r is None for r in results):
        return None
    ys = [np.asarray(r.get_y()) for r in results]
    xs = [np.asarray(r.get_x()) for r in results]
    ths = [np.asarray(r.ths) for r in results]
    scores = [r.get_score() for r in results]
    shortest = min(len(t) for t in ths)
    for i in range(len(ths)):
        pick = sorted(np.random.choice(len(ths[i]), size=shortest, replace=False))
        ys[i], xs[i], ths[i] = ys[i][pick], xs[i][pick], ths[i][pick]
    y, x, th = (np.mean(np.asarray(a), axis=0) for a in (ys, xs, ths))
    score, std, n = np.mean(scores), np.std(scores), len(scores)
    if isinstance(results[0], ROC):
        return ROC(score, std, n, tpr=y, fpr=x, ths=th)
    return PRC(score, std, n, prec=y, rec=x, ths=th)


def _avg_ranks(sorted_scores: np.ndarray) -> np.ndarray:
    n = sorted_scores.size
    bounds = np.flatnonzero(np.diff(sorted_scores) != 0) + 1
    starts = np.concatenate([[0], bounds])
    ends = np.concatenate([bounds, [n]])
    mid = 0.5 * (starts + ends - 1) + 1.0
    return np.repeat(mid, ends - starts)


def roc_auc(labels, scores) -> float:
    labels = np.asarray(labels).astype(np.int64).ravel()
    scores = np.asarray(scores, dtype=np.float64).ravel()
    pos = labels == 1
    n_pos = int(pos.sum())
    n_neg = labels.size - n_pos
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    order = np.argsort(scores, kind="stable")
    ranks = np.empty(labels.size, dtype=np.float64)
    ranks[order] = _avg_ranks(scores[order])
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def average_precision(labels, scores) -> float:
    labels = np.asarray(labels).astype(np.int64).ravel()
    scores = np.asarray(scores, dtype=np.float64).ravel()
    n_pos = int((labels == 1).sum())
    if n_pos == 0:
        return float("nan")
    order = np.argsort(-scores, kind="stable")
    s, y = scores[order], labels[order] == 1
    tp, fp = np.cumsum(y), np.cumsum(~y)
    last = np.concatenate([np.flatnonzero(np.diff(s) != 0), [s.size - 1]])
    tp, fp = tp[last], fp[last]
    recall = tp / n_pos
    return float(np.sum(np.diff(np.concatenate([[0.0], recall])) * (tp / (tp + fp))))


def auc_ap_device(labels, scores):
    """(ROC AUC, average precision) of GPU-resident scores without the host round trip: `eoe_auc_ap` (exact integer pair counts,
    tie-aware; equals `roc_auc` / `average_precision` above up to fp64 rounding).  labels: int tensor [n] (1 = anomalous)."""
    import torch
    from ._lib import check, lib
    if not scores.is_cuda:
        raise RuntimeError("auc_ap_device needs GPU tensors (use roc_auc / average_precision on the host)")
    sc = scores.detach().reshape(-1).contiguous().float()
    la = labels.to(sc.device).reshape(-1).contiguous().to(torch.int64)
    n = sc.numel()
    out = torch.empty(2, dtype=torch.float64, device=sc.device)
    scratch = torch.empty(((n + 255) // 256) * 24, dtype=torch.uint8, device=sc.device)
    check(lib.eoe_auc_ap(sc.data_ptr(), la.data_ptr(), 1, out.data_ptr(), scratch.data_ptr(), n, torch.cuda.current_stream().cuda_stream),
          "eoe_auc_ap")
    auc, ap = out.cpu().tolist()
    return auc, ap


# ------------------------------------------------------------------------------------------------------ curves
def _check_counts(fps, tps):
    """both classes must be present: the rates divide by the class sizes (the last entries of the cumulative counts)"""
    if tps[-1] == 0 or fps[-1] == 0:
        raise ValueError(f"curves need both classes: {int(tps[-1])} positive (label 1) and {int(fps[-1])} other samples")


def _host_inputs(labels, scores):
    labels = np.asarray(labels).ravel()
    scores = np.asarray(scores).ravel()
    if scores.dtype != np.float32:
        scores = scores.astype(np.float64)
    if labels.size != scores.size or scores.size == 0:
        raise ValueError(f"curves need as many labels as scores and at least one, not {labels.size} and {scores.size}")
    if not np.isfinite(scores).all():
        raise ValueError("scores contain NaN or infinity")
    return labels == 1, scores


def _counts_host(pos: np.ndarray, scores: np.ndarray):
    """(fps, tps, thresholds) per distinct score, descending: the table `eoe_rank_curves` makes from pair counts, here from a stable
    sort.  Reversing a stable ascending sort leaves the smallest index last in a group of equal scores; the group's threshold is
    that element (its bits: -0.0 and 0.0 are one group)."""
    order = np.argsort(scores, kind="stable")[::-1]
    s, y = scores[order], pos[order]
    last = np.concatenate([np.flatnonzero(s[1:] != s[:-1]), [s.size - 1]])
    tps = np.cumsum(y, dtype=np.int64)[last]
    return last + 1 - tps, tps, s[last]


def _roc_keep(fps: np.ndarray, tps: np.ndarray) -> np.ndarray:
    """the slots `drop_intermediate` keeps: the ends and every point that is not on the line between its neighbours"""
    if fps.size <= 2:
        return np.arange(fps.size)
    bend = (np.diff(fps, 2) != 0) | (np.diff(tps, 2) != 0)
    return np.flatnonzero(np.concatenate([[True], bend, [True]]))


def _finish_roc(fps, tps, thr):
    _check_counts(fps, tps)
    fps, tps = np.concatenate([[0], fps]), np.concatenate([[0], tps])
    thr = np.concatenate([np.array([np.inf], thr.dtype), thr])
    return fps / fps[-1], tps / tps[-1], thr


def _finish_prc(fps, tps, thr):
    _check_counts(fps, tps)
    total = tps + fps
    precision = np.zeros(tps.size, np.float64)
    np.divide(tps, total, out=precision, where=total != 0)
    recall = tps / tps[-1]
    return np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]]), thr[::-1].copy()


def rank_curves_device(labels, scores, drop_intermediate: bool = True):
    """`eoe_rank_curves` on GPU-resident scores: ((fps, tps, thr), (roc_fps, roc_tps, roc_thr)) as host arrays (int64, int64,
    float32) of lengths K and K_roc -- the count table per distinct score and what `drop_intermediate` leaves of it.  One launch
    sequence serves both curves; only the K used entries are copied to the host."""
    import torch
    from ._lib import check, lib
    if not scores.is_cuda:
        raise RuntimeError("rank_curves_device needs GPU tensors (roc_curve / precision_recall_curve take host arrays as they are)")
    sc = scores.detach().reshape(-1).contiguous().float()
    la = torch.as_tensor(labels).to(sc.device).reshape(-1).contiguous().to(torch.int64)
    n = sc.numel()
    if la.numel() != n or n == 0:
        raise ValueError(f"curves need as many labels as scores and at least one, not {la.numel()} and {n}")
    if n > CURVES_MAX_N:
        raise ValueError(f"eoe_rank_curves takes at most {CURVES_MAX_N} scores, not {n}")
    if not bool(torch.isfinite(sc).all()):
        raise ValueError("scores contain NaN or infinity")
    counts_i = torch.empty((4, n), dtype=torch.int64, device=sc.device)
    thr = torch.empty((2, n), dtype=torch.float32, device=sc.device)
    counts = torch.empty(2, dtype=torch.int32, device=sc.device)
    scratch = torch.empty(lib.eoe_rank_curves_scratch_bytes(n), dtype=torch.uint8, device=sc.device)
    check(lib.eoe_rank_curves(sc.data_ptr(), la.data_ptr(), 1, n, 1 if drop_intermediate else 0, counts_i[0].data_ptr(),
                              counts_i[1].data_ptr(), thr[0].data_ptr(), counts_i[2].data_ptr(), counts_i[3].data_ptr(), thr[1].data_ptr(),
                              counts.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream), "eoe_rank_curves")
    K, K_roc = counts.cpu().tolist()
    full = (counts_i[0, :K].cpu().numpy(), counts_i[1, :K].cpu().numpy(), thr[0, :K].cpu().numpy())
    roc = (counts_i[2, :K_roc].cpu().numpy(), counts_i[3, :K_roc].cpu().numpy(), thr[1, :K_roc].cpu().numpy())
    return full, roc


def _is_gpu_tensor(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def _to_host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def roc_curve(labels, scores, drop_intermediate: bool = True):
    """(fpr, tpr, thresholds) of sklearn's `roc_curve(labels, scores)` (`ad_trainer.py:453, 517`; positive label 1): float64 rates,
    thresholds in the scores' precision (float32 stays float32) with `inf` in front.  GPU scores are counted on the device
    (`eoe_rank_curves`), host arrays through a sort; both give the same integers, and the one division is done here.
    ValueError for non-finite scores and when a class is missing."""
    if _is_gpu_tensor(scores):
        _, (fps, tps, thr) = rank_curves_device(labels, scores, drop_intermediate)
        return _finish_roc(fps, tps, thr)
    pos, s = _host_inputs(_to_host(labels), _to_host(scores))
    fps, tps, thr = _counts_host(pos, s)
    if drop_intermediate:
        keep = _roc_keep(fps, tps)
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    return _finish_roc(fps, tps, thr)


def precision_recall_curve(labels, scores):
    """(precision, recall, thresholds) of sklearn's `precision_recall_curve(labels, scores)` (`ad_trainer.py:520`): thresholds
    ascending, the point (precision 1, recall 0) appended.  Same routing and errors as `roc_curve`."""
    if _is_gpu_tensor(scores):
        (fps, tps, thr), _ = rank_curves_device(labels, scores, False)
        return _finish_prc(fps, tps, thr)
    pos, s = _host_inputs(_to_host(labels), _to_host(scores))
    return _finish_prc(*_counts_host(pos, s))


def curves_device(labels, scores):
    """both curves of GPU-resident scores from one `eoe_rank_curves` call: ((fpr, tpr, thresholds), (precision, recall, thresholds))"""
    full, roc = rank_curves_device(labels, scores, True)
    return _finish_roc(*roc), _finish_prc(*full)
