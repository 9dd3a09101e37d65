"""Epoch-tail metrics of the trainer (`src/eoe/training/ad_trainer.py:452-455,516-522`): the reference calls
sklearn's `roc_curve` + `auc` (trapezoid) and `average_precision_score` on host copies of the epoch's labels and
scores.  Same place (host, once per epoch), written as the tie-aware rank statistic, which equals the trapezoidal
ROC area, and the step-wise precision-recall sum.

The curves themselves (`roc_curve`, `precision_recall_curve` below) come from one table of exact integer counts per distinct
score -- `eoe_rank_curves` for GPU tensors, a sort for host arrays -- and sklearn's finishing steps in float64 on the host.

The score histograms the reference logs next to them (`:458-465, 541-546`, TensorBoard's `add_histogram`) are `score_histogram` /
`score_histograms`: integer counts over TensorBoard's fixed edges -- `eoe_score_hist` for GPU tensors, `np.histogram` for host
arrays -- and the same trimming of the integer arrays on the host.

Which test images those numbers rest on -- per label group the highest and the lowest scores with their positions, as the reference
ranks OE individuals in `Tree.scores_best` -- is `score_extremes`: `eoe_score_extremes` (an exact radix select) for GPU tensors, two
stable argsorts for host arrays.

Which class causes the misses -- per class of the test split the AUC, the FPR at a TPR level and the AP of that class against the
pool of all samples of the other side, which the reference does not have -- is `class_breakdown`: `eoe_class_breakdown` (exact
integer pair counts, one workgroup per class) for GPU tensors, sorts for host arrays.

How much of a difference between two AUCs is test-set sampling noise -- DeLong's confidence interval of an AUC and the paired test of
K models scored on the same samples, which neither the reference nor sklearn has -- is `delong` / `AucTest`: `eoe_delong_counts`
(per sample the doubled count of opposite-label samples it beats or ties, then their sums and cross sums: exact integers) for GPU
tensors, `searchsorted` for host arrays; the numerators in Python integers and one division per entry on the host.

What the other two numbers next to every AUC are worth -- the average precision and the FPR at a TPR level, for which there is no
DeLong -- is `bootstrap` / `Bootstrap`: a stratified, paired bootstrap whose draws are stated exactly (Philox4x32-10 counters), every
replicate resampled and counted by `eoe_bootstrap_counts` for GPU tensors and by `bootstrap_np` (the same integers) for host arrays."""
from typing import Optional

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


# ------------------------------------------------------------------------------------------------------ histograms
HIST_MAX_EDGES = 4001             # eoe_score_hist: the edge table and both groups' counters share a workgroup's LDS
_HIST_STATS = 5                   # count, min, max, sum, sum of squares


class Histogram:
    """what `SummaryWriter.add_histogram(tag, values, step)` stores of `values` under its defaults (`ad_trainer.py:458-465, 541-546`;
    the seven fields of TensorBoard's HistogramProto): `min`, `max`, `num`, `sum`, `sum_squares` over all values, and the occupied
    range of `np.histogram(values, bins=edges)` as `bucket_limit` (right edges, floats) and `bucket` (counts, ints) with one empty
    bucket in front.  Both lists are empty when no value lies inside the edges."""
    FIELDS = ("min", "max", "num", "sum", "sum_squares", "bucket_limit", "bucket")

    def __init__(self, min: float, max: float, num: int, sum: float, sum_squares: float, bucket_limit, bucket):
        self.min, self.max, self.num, self.sum, self.sum_squares = float(min), float(max), int(num), float(sum), float(sum_squares)
        self.bucket_limit, self.bucket = [float(x) for x in bucket_limit], [int(c) for c in bucket]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, Histogram) and self.as_dict() == other.as_dict()

    def __repr__(self):
        return f"Histogram(num={self.num}, min={self.min}, max={self.max}, sum={self.sum}, {len(self.bucket)} buckets)"


_DEFAULT_EDGES = None


def default_edges() -> np.ndarray:
    """TensorBoard's `bins='tensorflow'` table, by its own float64 loop (a closed form would move edges by an ulp): 1e-12 * 1.1^k below
    1e20, mirrored, 0 in the middle; 1 549 edges"""
    global _DEFAULT_EDGES
    if _DEFAULT_EDGES is None:
        pos, v = [], 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        _DEFAULT_EDGES = np.array([-p for p in reversed(pos)] + [0] + pos, dtype=np.float64)
        _DEFAULT_EDGES.setflags(write=False)
    return _DEFAULT_EDGES


def _hist_edges(bins) -> np.ndarray:
    if isinstance(bins, str):
        if bins != "tensorflow":
            raise ValueError(f"bins must be 'tensorflow' or an array of edges, not {bins!r}")
        return default_edges()
    edges = np.array(_to_host(bins), dtype=np.float64).ravel()
    if edges.size < 2 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
        raise ValueError("bins must be at least two finite, strictly ascending edges")
    if edges.size > HIST_MAX_EDGES:
        raise ValueError(f"bins may hold at most {HIST_MAX_EDGES} edges, not {edges.size}")
    return edges


def _trim_histogram(counts: np.ndarray, edges: np.ndarray, num, vmin, vmax, vsum, vsq) -> Histogram:
    """the occupied range of the integer counts: first to last non-empty bin, one empty bin in front (the real bin to the left when
    there is one), the right edges of what is kept"""
    filled = np.flatnonzero(counts)
    if filled.size == 0:
        return Histogram(vmin, vmax, num, vsum, vsq, [], [])
    first, last = int(filled[0]), int(filled[-1])
    kept = counts[first - 1:last + 1] if first > 0 else np.concatenate([[0], counts[:last + 1]])
    return Histogram(vmin, vmax, num, vsum, vsq, edges[first:last + 2].tolist(), kept.tolist())


def _hist_host(values: np.ndarray, edges: np.ndarray) -> Optional[Histogram]:
    if values.size == 0:
        return None
    v = values.astype(np.float64)
    counts, _ = np.histogram(v, bins=edges)
    return _trim_histogram(counts, edges, v.size, v.min(), v.max(), v.sum(), np.dot(v, v))


_EDGES_ON_DEVICE = {}             # (device, the table's bytes) -> (host array, device tensor): uploaded once per device


def _device_edges(edges: np.ndarray, device):
    import torch
    key = (str(device), edges.tobytes())
    hit = _EDGES_ON_DEVICE.get(key)
    if hit is None:
        if len(_EDGES_ON_DEVICE) >= 16:                      # explicit tables come and go; the default one is uploaded again at worst
            _EDGES_ON_DEVICE.clear()
        host = np.ascontiguousarray(edges, dtype=np.float64)
        hit = _EDGES_ON_DEVICE[key] = (host, torch.from_numpy(host.copy()).to(device))
    return hit


def score_hist_device(scores, labels=None, bins="tensorflow", scratch=None):
    """`eoe_score_hist` on GPU-resident scores: (counts int64 [2, E-1], stats float64 [2, 5], edges float64 [E]) as host arrays -- per
    label group (row 0: label 0, row 1: label 1; other labels in neither; `labels=None`: everything in row 0) the untrimmed
    `np.histogram` counts and (count, min, max, sum, sum of squares).  One memset, two launches and one copy back for both groups.
    `scratch`: a uint8 GPU tensor of at least `eoe_score_hist_scratch_bytes(n)` bytes to reuse (its content does not matter)."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(scores):
        raise RuntimeError("score_hist_device needs GPU tensors (score_histogram takes host arrays as they are)")
    edges = _hist_edges(bins)
    sc = scores.detach().reshape(-1).contiguous().float()
    n = sc.numel()
    la = None
    if labels is not None:
        la = torch.as_tensor(labels).to(sc.device).reshape(-1).contiguous().to(torch.int64)
    if n == 0 or (la is not None and la.numel() != n):
        raise ValueError(f"histograms need at least one score and as many labels as scores, not {n} and {None if la is None else la.numel()}")
    if n >= 1 << 31:
        raise ValueError(f"eoe_score_hist takes fewer than 2^31 scores, not {n}")
    if not bool(torch.isfinite(sc).all()):
        raise ValueError("scores contain NaN or infinity")
    host_edges, dev_edges = _device_edges(edges, sc.device)
    nb = edges.size - 1
    need = lib.eoe_score_hist_scratch_bytes(n)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=sc.device)
    elif scratch.dtype != torch.uint8 or scratch.device != sc.device or scratch.numel() < need or not scratch.is_contiguous():
        raise ValueError(f"scratch must be a contiguous uint8 tensor of at least {need} bytes on {sc.device}")
    # one buffer, one copy back: the 10 doubles first (8-byte aligned), then the 2 x (E - 1) counts
    out = torch.empty(2 * _HIST_STATS * 8 + 2 * nb * 4, dtype=torch.uint8, device=sc.device)
    check(lib.eoe_score_hist(sc.data_ptr(), la.data_ptr() if la is not None else None, n, host_edges.ctypes.data, dev_edges.data_ptr(),
                             edges.size, out.data_ptr() + 2 * _HIST_STATS * 8, out.data_ptr(), scratch.data_ptr(),
                             torch.cuda.current_stream().cuda_stream), "eoe_score_hist")
    raw = out.cpu().numpy()
    stats = raw[:2 * _HIST_STATS * 8].view(np.float64).reshape(2, _HIST_STATS).copy()
    counts = raw[2 * _HIST_STATS * 8:].view(np.int32).reshape(2, nb).astype(np.int64)
    return counts, stats, edges


def _hist_from_device(counts, stats, edges, g: int) -> Optional[Histogram]:
    num = int(stats[g, 0])
    if num == 0:
        return None
    return _trim_histogram(counts[g], edges, num, stats[g, 1], stats[g, 2], stats[g, 3], stats[g, 4])


def _hist_host_inputs(scores, labels):
    s = np.asarray(_to_host(scores)).ravel()
    if s.dtype != np.float32:
        s = s.astype(np.float64)
    y = None if labels is None else np.asarray(_to_host(labels)).ravel()
    if s.size == 0 or (y is not None and y.size != s.size):
        raise ValueError(f"histograms need at least one score and as many labels as scores, not {s.size} and {None if y is None else y.size}")
    if not np.isfinite(s).all():
        raise ValueError("scores contain NaN or infinity")
    return s, y


def score_histograms(labels, scores, bins="tensorflow"):
    """(histogram of the scores with label 0, histogram of those with label 1): the two pictures the reference logs per epoch and per
    evaluation.  Scores with any other label (-1 for unlabelled images) are in neither; a group without members gives None (the
    reference's `make_histogram` would raise on it).  GPU scores cost one `eoe_score_hist` launch sequence for both; host arrays and
    CPU tensors go through `np.histogram`.  `bins` as in `score_histogram`."""
    if labels is None:
        raise ValueError("score_histograms needs labels (score_histogram(scores) bins everything)")
    if _is_gpu_tensor(scores):
        counts, stats, edges = score_hist_device(scores, labels, bins)
        return _hist_from_device(counts, stats, edges, 0), _hist_from_device(counts, stats, edges, 1)
    edges = _hist_edges(bins)
    s, y = _hist_host_inputs(scores, labels)
    return _hist_host(s[y == 0], edges), _hist_host(s[y == 1], edges)


def score_histogram(scores, labels=None, label=None, bins="tensorflow"):
    """The `Histogram` TensorBoard's `add_histogram(tag, scores, step)` would store (`make_histogram(scores, default_bins)`): counts of
    `np.histogram` over the 1 549 'tensorflow' edges -- bins half-open, the last one closed, float32 scores compared as float64 --
    trimmed to the occupied range, and min / max / num / sum / sum_squares over all scores (the sums in float64).  With `labels` and
    `label` (0 or 1) only the scores carrying that label count; None when there are none.  GPU tensors are bucketed on the device
    (`eoe_score_hist`; only the counts and five scalars per group come back), host arrays and CPU tensors by `np.histogram`; both
    give the same `bucket`, `bucket_limit`, `num`, `min` and `max`.

    `bins` may be an explicit array of finite, strictly ascending edges instead, at most `HIST_MAX_EDGES` = 4001 of them (4 000 bins:
    what one workgroup's LDS holds next to the counters); longer arrays are a ValueError on both paths.  `max_bins` sub-sampling is
    not offered.  ValueError for non-finite scores, no scores, and labels of another length."""
    if (labels is None) != (label is None):
        raise ValueError("labels and label go together: both or neither")
    if label is not None and label not in (0, 1):
        raise ValueError(f"label must be 0 or 1, not {label!r}")
    if labels is not None:
        return score_histograms(labels, scores, bins)[int(label)]
    if _is_gpu_tensor(scores):
        return _hist_from_device(*score_hist_device(scores, None, bins), 0)
    s, _ = _hist_host_inputs(scores, None)
    return _hist_host(s, _hist_edges(bins))


# ------------------------------------------------------------------------------------------------------ extremes
EXTREMES_MAX_N = 1 << 20          # eoe_score_extremes: a position fits the low 20 bits of its key
EXTREMES_MAX_K = 1024             # what one workgroup sorts in LDS
_GROUP_NAMES = ("nominal", "anomalous")


class Extremes:
    """the extremes of an evaluation's scores per label group g (0: label 0, nominal; 1: label 1, anomalous): `most[g]` and `least[g]`
    are (indices int64 ndarray, scores float32 ndarray) pairs of min(k, num[g]) entries -- the highest scores first resp. the lowest
    first, equal scores by ascending position -- and `num[g]` the size of the group.  `most[0]` are the false alarms, `least[1]` the
    misses."""

    def __init__(self, most, least, num):
        pair = lambda p: (np.asarray(p[0], dtype=np.int64), np.asarray(p[1], dtype=np.float32))    # noqa: E731
        self.most, self.least = (pair(most[0]), pair(most[1])), (pair(least[0]), pair(least[1]))
        self.num = (int(num[0]), int(num[1]))

    def as_dict(self) -> dict:
        """{"nominal": {"most": [[index, score], ...], "least": [...], "num": m}, "anomalous": {...}}: ints and floats, for JSON"""
        rows = lambda p: [[int(i), float(v)] for i, v in zip(*p)]                                    # noqa: E731
        return {name: {"most": rows(self.most[g]), "least": rows(self.least[g]), "num": self.num[g]} for g, name in enumerate(_GROUP_NAMES)}

    def __eq__(self, other):
        return isinstance(other, Extremes) and self.num == other.num and all(
            np.array_equal(a[j], b[j]) and a[j].dtype == b[j].dtype
            for a, b in zip(self.most + self.least, other.most + other.least) for j in (0, 1))

    def __repr__(self):
        return f"Extremes(num={self.num}, k={[len(p[0]) for p in self.most]})"


def _check_extremes_k(k):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1 or k > EXTREMES_MAX_K:
        raise ValueError(f"k must be an integer in [1, {EXTREMES_MAX_K}], not {k!r}")
    return int(k)


def _extremes_host(s: np.ndarray, y: Optional[np.ndarray], k: int):
    """the two stable argsorts per group: ((most pairs), (least pairs), (num)) over positions"""
    most, least, num = [], [], []
    for g in (0, 1):
        members = np.flatnonzero(y == g) if y is not None else (np.arange(s.size) if g == 0 else np.zeros(0, np.int64))
        sg = s[members]
        if not np.isfinite(sg).all():
            raise ValueError("scores contain NaN or infinity")
        hi, lo = members[np.argsort(-sg, kind="stable")[:k]], members[np.argsort(sg, kind="stable")[:k]]
        most.append((hi, s[hi]))
        least.append((lo, s[lo]))
        num.append(members.size)
    return most, least, num


def score_extremes_device(labels, scores, k: int = 20, scratch=None):
    """`eoe_score_extremes` on GPU-resident scores: (idx int32 [2, 2, k], val float32 [2, 2, k], counts [m_0, m_1, non-finite]) as host
    arrays -- [group][end] with end 0 = most, end 1 = least; the slots past min(k, m_g) hold -1 and 0.  One call (a memset and seven
    launches) and ONE copy back of the 4 k pairs and the three counts.  `labels` None: every score in group 0.  `scratch`: a uint8 GPU
    tensor of at least `eoe_score_extremes_scratch_bytes(n, k)` bytes to reuse (its content does not matter)."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(scores):
        raise RuntimeError("score_extremes_device needs GPU tensors (score_extremes takes host arrays as they are)")
    k = _check_extremes_k(k)
    sc = scores.detach().reshape(-1).contiguous().float()
    n = sc.numel()
    la = None
    if labels is not None:
        la = torch.as_tensor(labels).to(sc.device).reshape(-1).contiguous().to(torch.int64)
    if n == 0 or (la is not None and la.numel() != n):
        raise ValueError(f"extremes need at least one score and as many labels as scores, not {n} and {None if la is None else la.numel()}")
    if n > EXTREMES_MAX_N:
        raise ValueError(f"eoe_score_extremes takes at most {EXTREMES_MAX_N} scores, not {n}")
    need = lib.eoe_score_extremes_scratch_bytes(n, k)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=sc.device)
    elif scratch.dtype != torch.uint8 or scratch.device != sc.device or scratch.numel() < need or not scratch.is_contiguous() \
            or scratch.data_ptr() % 16:
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {sc.device}")
    # one buffer, one copy back: 4 k positions (-1 where a list is shorter), 4 k scores, 3 counts
    out = torch.empty(8 * k + 3, dtype=torch.int32, device=sc.device)
    out[:4 * k] = -1
    out[4 * k:] = 0
    with torch.cuda.device(sc.device):
        check(lib.eoe_score_extremes(sc.data_ptr(), la.data_ptr() if la is not None else None, n, k, out.data_ptr(),
                                     out.data_ptr() + 16 * k, out.data_ptr() + 32 * k, scratch.data_ptr(),
                                     torch.cuda.current_stream(sc.device).cuda_stream), "eoe_score_extremes")
    raw = out.cpu().numpy()
    return raw[:4 * k].reshape(2, 2, k).copy(), raw[4 * k:8 * k].view(np.float32).reshape(2, 2, k).copy(), raw[8 * k:].tolist()


def score_extremes(labels, scores, k: int = 20, indices=None) -> Extremes:
    """The most and the least anomalous samples per label group: for the scores with label 0 (nominal) and those with label 1
    (anomalous) the `k` highest -- `np.argsort(-s, kind="stable")[:k]` over the group's members -- and the `k` lowest --
    `np.argsort(s, kind="stable")[:k]` -- with equal scores (-0.0 == 0.0) in ascending position.  Scores with any other label (-1 for
    unlabelled images) are in neither group; `labels=None` puts every score in group 0.  A `k` larger than a group returns the whole
    group, ranked.  Scores are ranked as float32.

    GPU tensors go through `eoe_score_extremes` in one call, and only the 4 k pairs and three counts come back; NumPy arrays and CPU
    tensors take the two stable argsorts on the host.  Both give the same positions and the same score bits.

    `indices` (optional, one per score) maps positions to dataset indices in the returned `indices`; the ranking itself is by position.
    ValueError for a non-finite score among the members of a group, for k outside [1, 1024], for no scores, and for labels or
    `indices` of another length; the device path takes at most 2^20 scores."""
    k = _check_extremes_k(k)
    remap = None if indices is None else np.asarray(_to_host(indices)).ravel().astype(np.int64)
    if _is_gpu_tensor(scores):
        if remap is not None and remap.size != scores.numel():
            raise ValueError(f"indices must name every score: {remap.size} for {scores.numel()} scores")
        idx, val, (m0, m1, bad) = score_extremes_device(labels, scores, k)
        if bad:
            raise ValueError("scores contain NaN or infinity")
        num = (m0, m1)
        most = [(idx[g, 0, :min(k, num[g])].astype(np.int64), val[g, 0, :min(k, num[g])]) for g in (0, 1)]
        least = [(idx[g, 1, :min(k, num[g])].astype(np.int64), val[g, 1, :min(k, num[g])]) for g in (0, 1)]
    else:
        s = np.asarray(_to_host(scores)).ravel().astype(np.float32)
        y = None if labels is None else np.asarray(_to_host(labels)).ravel()
        if s.size == 0 or (y is not None and y.size != s.size):
            raise ValueError(f"extremes need at least one score and as many labels as scores, not {s.size} and {None if y is None else y.size}")
        if remap is not None and remap.size != s.size:
            raise ValueError(f"indices must name every score: {remap.size} for {s.size} scores")
        most, least, num = _extremes_host(s, y, k)
    if remap is not None:
        most, least = [(remap[i], v) for i, v in most], [(remap[i], v) for i, v in least]
    return Extremes(most, least, num)


# ------------------------------------------------------------------------------------------------------ per-class breakdown
BREAKDOWN_MAX_N = 1 << 20         # eoe_class_breakdown: the cap of eoe_rank_curves
BREAKDOWN_MAX_CLASSES = 1024      # a dense class id shares one word with the side
_BD_COLS = 4                      # a row of the integer table: 2U, fps, tps, n_k


class Breakdown:
    """An evaluation's scores broken down by class.  A sample's side is 0 (nominal) when its class is a normal class and 1
    (anomalous) otherwise; the sub-problem of class k is class k against the pool of ALL samples of the other side, label 1 on the
    anomalous side.  Arrays have one entry per class present, in ascending order of the class id:

      classes   the class ids (int64);  names  their names (str);  side  0 / 1;  n  the class sizes
      auc       `roc_auc_score` of the sub-problem: 2U / (2 n_pos n_neg), 2U = sum over (positive, negative) of 2 [s_p > s_n] + [s_p == s_n]
      fpr       the sub-problem's false-positive rate at the first ROC point whose TPR reaches `tpr_level`
      ap        `average_precision_score` of the sub-problem for an ANOMALOUS class, a list of floats; None for a nominal class: its
                positives are the pool, so it would take a count per (pool sample, class), which is not built
      fpr_at_tpr, threshold   the same rate on the pooled problem (every anomalous sample against every nominal one) and the score
                at which it is taken: a sample is flagged when its score is >= threshold
    A class whose pool is empty has NaN in `auc`, `fpr` and `ap`; the pooled numbers are NaN when a side is missing.

    What the rates are divided from is kept as well: `counts` int64 [K + 1, 4] with rows {2U, fps, tps, n} (fps / tps: negatives /
    positives at or above the threshold; row K: the pooled problem's fps and tps) and `thresholds` [K + 1] in the scores' precision
    (a nominal class's threshold is the pooled one, its positives being the whole anomalous side); rows of an empty problem are 0 / NaN."""

    def __init__(self, classes, names, side, n, auc, ap, fpr, tpr_level, fpr_at_tpr, threshold, counts=None, thresholds=None):
        self.classes, self.side, self.n = (np.asarray(a, dtype=np.int64) for a in (classes, side, n))
        self.names = [str(x) for x in names]
        self.auc, self.fpr = np.asarray(auc, dtype=np.float64), np.asarray(fpr, dtype=np.float64)
        self.ap = [None if a is None else float(a) for a in ap]
        self.tpr_level, self.fpr_at_tpr, self.threshold = float(tpr_level), float(fpr_at_tpr), float(threshold)
        self.counts = None if counts is None else np.asarray(counts, dtype=np.int64)
        self.thresholds = None if thresholds is None else np.asarray(thresholds)

    def hardest(self):
        """(class id, name, auc) of the class with the lowest AUC; None when no class has one"""
        if not np.isfinite(self.auc).any():
            return None
        k = int(np.nanargmin(self.auc))
        return int(self.classes[k]), self.names[k], float(self.auc[k])

    def to_json(self) -> dict:
        """ints, floats, strings and None (for NaN and for the AP of a nominal class): strict JSON"""
        num = lambda x: None if (x is None or x != x) else float(x)                                 # noqa: E731
        return {"classes": [int(c) for c in self.classes], "names": list(self.names), "side": [int(x) for x in self.side],
                "n": [int(x) for x in self.n], "auc": [num(x) for x in self.auc], "ap": [num(x) for x in self.ap],
                "fpr": [num(x) for x in self.fpr], "tpr_level": self.tpr_level, "fpr_at_tpr": num(self.fpr_at_tpr),
                "threshold": num(self.threshold)}

    def __repr__(self):
        return f"Breakdown({len(self.classes)} classes, tpr_level={self.tpr_level}, fpr_at_tpr={self.fpr_at_tpr})"


def place_for_tpr(tpr: float, n_pos: int) -> int:
    """the smallest integer m with m / n_pos >= tpr in float64 -- the number of positives the first ROC point with TPR >= tpr holds
    (sklearn's `tps / tps[-1]` is this division); 0 when there are no positives"""
    if n_pos < 1:
        return 0
    m = min(max(int(np.ceil(tpr * n_pos)), 1), n_pos)
    while m > 1 and (m - 1) / n_pos >= tpr:
        m -= 1
    while m < n_pos and m / n_pos < tpr:
        m += 1
    return m


def _ge(sorted_x: np.ndarray, q) -> np.ndarray:
    return sorted_x.size - np.searchsorted(sorted_x, q, side="left")


def _gt(sorted_x: np.ndarray, q) -> np.ndarray:
    return sorted_x.size - np.searchsorted(sorted_x, q, side="right")


def _threshold_host(pos: np.ndarray, m: int):
    """the score at place m (1-based) of `pos` in descending order, with the bits of the smallest index among its equal scores: what
    a reversed stable sort leaves last in the group (-0.0 and 0.0 are one group)"""
    v = pos[np.argsort(pos, kind="stable")[::-1][m - 1]]
    return pos[np.flatnonzero(pos == v)[0]]


def _breakdown_host(s: np.ndarray, dense: np.ndarray, side: np.ndarray, m_cls: np.ndarray, m_pooled: int):
    """the tables of `eoe_class_breakdown` from sorts: (counts int64 [K + 1, 4], ap float64 [K], thresholds [K + 1])"""
    K = side.size
    counts, ap, thr = np.zeros((K + 1, _BD_COLS), np.int64), np.zeros(K, np.float64), np.zeros(K + 1, s.dtype)
    on_side = side[dense]
    pooled = [s[on_side == 0], s[on_side == 1]]                                  # in index order
    pool = [np.sort(p) for p in pooled]
    if m_pooled >= 1:
        thr[K] = _threshold_host(pooled[1], m_pooled)
        counts[K, 1], counts[K, 2] = _ge(pool[0], thr[K]), _ge(pool[1], thr[K])
    by_class = np.argsort(dense, kind="stable")                                  # members of a class in index order
    starts = np.searchsorted(dense[by_class], np.arange(K + 1))
    for k in range(K):
        sk = s[by_class[starts[k]:starts[k + 1]]]
        counts[k, 3] = sk.size
        if sk.size == 0:
            continue
        if side[k]:
            ge_pool, ge_own = _ge(pool[0], sk), _ge(np.sort(sk), sk)
            counts[k, 0] = 2 * sk.size * pool[0].size - int((ge_pool + _gt(pool[0], sk)).sum())
            ap[k] = float(np.sum(ge_own / (ge_own + ge_pool).astype(np.float64))) / sk.size
            if m_cls[k] >= 1:
                thr[k] = _threshold_host(sk, int(m_cls[k]))
                counts[k, 1], counts[k, 2] = _ge(pool[0], thr[k]), _ge(np.sort(sk), thr[k])
        else:
            counts[k, 0] = int((_ge(pool[1], sk) + _gt(pool[1], sk)).sum())
            counts[k, 1], counts[k, 2], thr[k] = int((sk >= thr[K]).sum()), counts[K, 2], thr[K]
    return counts, ap, thr


def class_breakdown_device(scores, dense, side, m_cls, m_pooled: int):
    """`eoe_class_breakdown` on GPU-resident scores: (counts int64 [K + 1, 4], ap float64 [K], thresholds float32 [K + 1]) as host
    arrays.  `dense` int32 [n] (class ids in [0, K)), `side` uint8 [K] and `m_cls` int32 [K] are host arrays: one upload, one call (two
    memsets and two launches) and ONE copy back."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(scores):
        raise RuntimeError("class_breakdown_device needs GPU scores (class_breakdown takes host arrays as they are)")
    sc = scores.detach().reshape(-1).contiguous().float()
    n, K = sc.numel(), int(side.size)
    if n < 1 or n > BREAKDOWN_MAX_N:
        raise ValueError(f"eoe_class_breakdown takes between 1 and {BREAKDOWN_MAX_N} scores, not {n}")
    if dense.size != n or m_cls.size != K:
        raise ValueError(f"one class id per score and one place per class: {dense.size} ids for {n} scores, {m_cls.size} places for {K} classes")
    # one upload: the class ids, the places and the sides (a byte each, behind the 4-byte words)
    host = np.concatenate([np.ascontiguousarray(dense, np.int32).view(np.uint8), np.ascontiguousarray(m_cls, np.int32).view(np.uint8),
                           np.ascontiguousarray(side, np.uint8)])
    dev = torch.from_numpy(host).to(sc.device)
    # one buffer, one copy back: the integer table and the APs (8-byte words) first, then the thresholds
    o_ap, o_thr = (K + 1) * _BD_COLS * 8, (K + 1) * _BD_COLS * 8 + K * 8
    out = torch.empty(o_thr + (K + 1) * 4, dtype=torch.uint8, device=sc.device)
    scratch = torch.empty(lib.eoe_class_breakdown_scratch_bytes(n, K), dtype=torch.uint8, device=sc.device)
    with torch.cuda.device(sc.device):
        check(lib.eoe_class_breakdown(sc.data_ptr(), dev.data_ptr(), dev.data_ptr() + 4 * n + 4 * K, dev.data_ptr() + 4 * n, int(m_pooled),
                                      n, K, out.data_ptr(), out.data_ptr() + o_ap, out.data_ptr() + o_thr, scratch.data_ptr(),
                                      torch.cuda.current_stream(sc.device).cuda_stream), "eoe_class_breakdown")
    raw = out.cpu().numpy()
    return (raw[:o_ap].view(np.int64).reshape(K + 1, _BD_COLS).copy(), raw[o_ap:o_thr].view(np.float64).copy(),
            raw[o_thr:].view(np.float32).copy())


def class_breakdown(scores, classes, normal_classes, tpr: float = 0.95, names=None) -> Breakdown:
    """Which class causes the misses: per class present in `classes` the AUC, the FPR at the first ROC point whose TPR reaches `tpr`
    and (anomalous classes) the AP of that class against the pool of all samples of the other side, plus the pooled FPR at that TPR
    and its threshold -- see `Breakdown`.  `classes` holds one class id per score (any integers, a host array or a tensor on either
    device); a class is nominal iff it is in `normal_classes` (`data.ad_targets`).  `names`: a sequence indexed by class id or a
    mapping id -> name; ids it does not cover are named by their number.

    FPR at a TPR level: with m the smallest integer with m / n_pos >= tpr (float64, as sklearn's `tps / tps[-1]`), the threshold is
    the score of the positive whose group of equal scores holds place m among the positives in descending order, and the rate is the
    share of negatives at or above it: `fpr[np.argmax(tpr_arr >= tpr)]` of `roc_curve(y, s, drop_intermediate=False)`.  For a nominal
    class the positives are the whole anomalous side, so every nominal class shares the pooled threshold.

    AP is reported for anomalous classes only (None for a nominal class): with the pool as positives it would need a count per (pool
    sample, class), which is not built.

    GPU scores go through `eoe_class_breakdown` (exact integer pair counts; the class ids are mapped to 0..K-1 on the host, which
    costs one copy of `classes` when they live on the device, and only the (K + 1) x 4 integers, K APs and K + 1 thresholds come
    back); host arrays and CPU tensors through sorts.  Both give the same integers and the same threshold bits; the APs agree to the
    rounding of a float64 sum of n_k terms.  Scores are taken as float32 on the device; host float32 stays float32, anything else is
    compared as float64.

    ValueError for non-finite scores, no scores, another number of class ids than scores, `tpr` outside (0, 1] and more than 1024
    classes; the device path takes at most 2^20 scores."""
    if isinstance(tpr, bool) or not isinstance(tpr, (int, float, np.integer, np.floating)) or not 0.0 < float(tpr) <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], not {tpr!r}")
    tpr = float(tpr)
    ids = np.asarray(_to_host(classes)).ravel()
    n = int(scores.numel()) if hasattr(scores, "numel") else int(np.asarray(scores).size)
    if ids.size != n or n == 0:
        raise ValueError(f"a breakdown needs as many class ids as scores and at least one, not {ids.size} and {n}")
    if ids.dtype.kind not in "iu":
        raise ValueError(f"class ids must be integers, not {ids.dtype}")
    present, dense = np.unique(ids.astype(np.int64), return_inverse=True)
    K = int(present.size)
    if K > BREAKDOWN_MAX_CLASSES:
        raise ValueError(f"a breakdown takes at most {BREAKDOWN_MAX_CLASSES} classes, not {K}")
    normal = {int(c) for c in np.asarray(_to_host(normal_classes)).ravel()}
    side = np.array([0 if int(c) in normal else 1 for c in present], dtype=np.uint8)
    sizes = np.bincount(dense, minlength=K).astype(np.int64)
    n_side = [int(sizes[side == 0].sum()), int(sizes[side == 1].sum())]
    m_pooled = place_for_tpr(tpr, n_side[1])
    m_cls = np.array([place_for_tpr(tpr, int(sizes[k])) if side[k] else m_pooled for k in range(K)], dtype=np.int32)
    if _is_gpu_tensor(scores):
        import torch
        if not bool(torch.isfinite(scores).all()):
            raise ValueError("scores contain NaN or infinity")
        counts, ap, thr = class_breakdown_device(scores, dense.astype(np.int32), side, m_cls, m_pooled)
    else:
        s = np.asarray(_to_host(scores)).ravel()
        if s.dtype != np.float32:
            s = s.astype(np.float64)
        if not np.isfinite(s).all():
            raise ValueError("scores contain NaN or infinity")
        counts, ap, thr = _breakdown_host(s, dense, side, m_cls, m_pooled)
    # the divisions, once, in float64; a problem with an empty side is cleared to 0 / NaN on both paths
    auc, fpr, aps = np.full(K, np.nan), np.full(K, np.nan), []
    for k in range(K):
        n_pos, n_neg = (int(sizes[k]), n_side[0]) if side[k] else (n_side[1], int(sizes[k]))
        if n_pos == 0 or n_neg == 0:
            counts[k, :3], thr[k] = 0, np.nan
            aps.append(float("nan") if side[k] else None)
            continue
        auc[k] = int(counts[k, 0]) / (2 * n_pos * n_neg)
        fpr[k] = int(counts[k, 1]) / n_neg
        aps.append(float(ap[k]) if side[k] else None)
    fpr_at_tpr = float("nan")
    if n_side[0] and n_side[1]:
        fpr_at_tpr = int(counts[K, 1]) / n_side[0]
    else:
        counts[K, :3], thr[K] = 0, np.nan
    if names is None:
        names = {}
    label = (lambda c: names.get(c, c)) if hasattr(names, "get") else (lambda c: names[c] if 0 <= c < len(names) else c)
    return Breakdown(present, [label(int(c)) for c in present], side, sizes, auc, aps, fpr, tpr, fpr_at_tpr, float(thr[K]), counts, thr)


# ------------------------------------------------------------------------------------------------------ DeLong
DELONG_MAX_N = BREAKDOWN_MAX_N    # eoe_delong_counts: the cap of eoe_class_breakdown
DELONG_MAX_COLUMNS = 8            # score columns (models) per call
DELONG_TILE = 256                 # the count pass: rows per workgroup and opposite-side scores per LDS tile


def delong_slices(n: int, K: int) -> int:
    """into how many slices `eoe_delong_counts` cuts the opposite side at n samples and K columns (`eoe_delong_slices`; 0 for an n or
    K it refuses): a slice is ceil(tiles / slices) tiles of `DELONG_TILE` scores, so with more tiles than slices a workgroup walks
    several tiles, and with more than one slice the partial counts of a row meet in one integer counter"""
    from ._lib import lib
    return int(lib.eoe_delong_slices(int(n), int(K)))


def _pairs(K: int):
    return [(k, l) for k in range(K) for l in range(k, K)]


class AucTest:
    """DeLong's estimate (DeLong, DeLong & Clarke-Pearson 1988) of the K ROC AUCs of K score columns over the same test samples and of
    their covariance matrix: what a difference between two AUCs is worth on a test set of this size.

      auc [K]   `roc_auc` of every column;  cov [K, K]  the AUCs' covariance;  var  its diagonal;  se  sqrt(var)
      n_pos, n_neg   the numbers of label-1 and label-0 samples (any other label is in neither)
      counts    the integer table everything is divided from: {"T_pos", "T_neg": int64 [K], "A", "B": int64 [K (K + 1) / 2] (upper
                triangles, row by row), "n_pos", "n_neg"}

    Stated over doubled counts -- a[k,i] = 2 #{negatives below positive i} + #{negatives equal to it} in column k, b[k,j] the same for
    negative j over the positives above and equal to it -- T[k] = sum a[k,:] = sum b[k,:], A[k,l] = sum_i a[k,i] a[l,i], B[k,l] =
    sum_j b[k,j] b[l,j], m = n_pos, n0 = n_neg:
        auc[k]   = T[k] / (2 m n0)
        S10[k,l] = (m A[k,l] - T[k] T[l]) / (m (m - 1) 4 n0^2)        S01[k,l] = (n0 B[k,l] - T[k] T[l]) / (n0 (n0 - 1) 4 m^2)
        cov[k,l] = S10[k,l] / m + S01[k,l] / n0
    The numerators are formed in Python integers (T^2 passes 2^63) and every entry is one exactly rounded division, so nothing depends
    on a summation order and an exact zero stays an exact zero.  With one positive or one negative the variance is undefined: `cov`,
    `var` and `se` are NaN.

    Positives {0.8, 0.6} against negatives {0.7, 0.5, 0.6}: a = {6, 3}, b = {2, 4, 3}, T = 9, auc = 9 / 12 = 0.75, S10 = (2 * 45 - 81) /
    (2 * 1 * 4 * 9) = 0.125, S01 = (3 * 29 - 81) / (3 * 2 * 4 * 4) = 0.0625, var = 0.125 / 2 + 0.0625 / 3 = 1 / 12."""

    def __init__(self, t_pos, t_neg, A, B, n_pos: int, n_neg: int):
        from fractions import Fraction
        self.n_pos, self.n_neg = int(n_pos), int(n_neg)
        m, n0 = self.n_pos, self.n_neg
        t_pos, t_neg, A, B = ([int(x) for x in np.asarray(v).ravel()] for v in (t_pos, t_neg, A, B))
        K = len(t_pos)
        if m < 1 or n0 < 1 or K < 1 or len(t_neg) != K or len(A) != len(B) or len(A) != K * (K + 1) // 2:
            raise ValueError("an AUC test needs both classes and a table of K, K, K (K + 1) / 2 and K (K + 1) / 2 integers")
        if t_pos != t_neg:
            raise RuntimeError(f"the positives' pair counts {t_pos} and the negatives' {t_neg} differ: the count table is broken")
        self.counts = {"T_pos": np.array(t_pos, np.int64), "T_neg": np.array(t_neg, np.int64), "A": np.array(A, np.int64),
                       "B": np.array(B, np.int64), "n_pos": m, "n_neg": n0}
        self.auc = np.array([t / (2 * m * n0) for t in t_pos], dtype=np.float64)       # int / int: one exactly rounded division
        self.cov = np.full((K, K), np.nan)
        self._cov = None                                                                # the exact entries, when they are defined
        self._pair = {}
        for p, (k, l) in enumerate(_pairs(K)):
            self._pair[k, l] = self._pair[l, k] = p
        if m > 1 and n0 > 1:
            self._cov = {}
            for p, (k, l) in enumerate(_pairs(K)):
                tt = t_pos[k] * t_pos[l]
                c = Fraction(m * A[p] - tt, m * (m - 1) * 4 * n0 * n0 * m) + Fraction(n0 * B[p] - tt, n0 * (n0 - 1) * 4 * m * m * n0)
                self._cov[k, l] = self._cov[l, k] = c
                self.cov[k, l] = self.cov[l, k] = float(c)
        self.var = np.diagonal(self.cov).copy()
        self.se = np.sqrt(self.var)

    def cov_fraction(self, k: int, l: int):
        """cov[k, l] as the exact rational number (`fractions.Fraction`); None where it is undefined"""
        return None if self._cov is None else self._cov[k, l]

    def ci(self, level: float = 0.95):
        """(lo [K], hi [K]): auc -+ z se with z = NormalDist().inv_cdf((1 + level) / 2), clipped to [0, 1]; NaN where se is"""
        from statistics import NormalDist
        level = _check_level(level)
        z = NormalDist().inv_cdf((1.0 + level) / 2.0)
        return np.clip(self.auc - z * self.se, 0.0, 1.0), np.clip(self.auc + z * self.se, 0.0, 1.0)

    def compare(self, k: int, l: int):
        """the paired test of columns k and l: (diff = auc[k] - auc[l], z = diff / sqrt(var_diff), two-sided p = erfc(|z| / sqrt 2)) with
        var_diff = cov[k,k] + cov[l,l] - 2 cov[k,l] (formed exactly before it is rounded: it cannot come out negative).  var_diff == 0:
        z is 0 and p 1.0 where diff == 0, else z is +-inf and p 0.0.  Where the covariance is undefined (one positive or one negative):
        (0.0, 0.0, 1.0) for two columns whose doubled counts agree sample by sample -- the difference is identically zero whatever
        the variance -- and (diff, NaN, NaN) otherwise."""
        import math
        diff = float(self.auc[k] - self.auc[l])
        if self._cov is None:
            if all(int(self.counts[t][self._pair[k, k]]) == int(self.counts[t][self._pair[k, l]]) == int(self.counts[t][self._pair[l, l]])
                   for t in ("A", "B")):                               # sum (a_k - a_l)^2 == 0 and sum (b_k - b_l)^2 == 0
                return 0.0, 0.0, 1.0
            return diff, float("nan"), float("nan")
        var_diff = float(self._cov[k, k] + self._cov[l, l] - 2 * self._cov[k, l])
        if var_diff == 0.0:
            return (diff, 0.0, 1.0) if diff == 0.0 else (diff, math.copysign(math.inf, diff), 0.0)
        z = diff / math.sqrt(var_diff)
        return diff, z, math.erfc(abs(z) / math.sqrt(2.0))

    def pvalues(self) -> np.ndarray:
        """[K, K]: `compare(k, l)[2]` for every pair (1.0 on the diagonal)"""
        K = self.auc.size
        return np.array([[self.compare(k, l)[2] for l in range(K)] for k in range(K)], dtype=np.float64).reshape(K, K)

    def to_json(self, level: float = 0.95) -> dict:
        """ints, floats, lists and None (for NaN): strict JSON"""
        num = lambda x: None if x != x else float(x)                                                 # noqa: E731
        lo, hi = self.ci(level)
        return {"auc": [num(x) for x in self.auc], "cov": [[num(x) for x in row] for row in self.cov], "var": [num(x) for x in self.var],
                "se": [num(x) for x in self.se], "n_pos": self.n_pos, "n_neg": self.n_neg, "level": float(level),
                "ci_lo": [num(x) for x in lo], "ci_hi": [num(x) for x in hi], "pvalues": [[num(x) for x in row] for row in self.pvalues()]}

    def __repr__(self):
        return f"AucTest(auc={self.auc.tolist()}, se={self.se.tolist()}, n_pos={self.n_pos}, n_neg={self.n_neg})"


def _check_level(level) -> float:
    if isinstance(level, bool) or not isinstance(level, (int, float, np.integer, np.floating)) or not 0.0 < float(level) < 1.0:
        raise ValueError(f"a confidence level must be in (0, 1), not {level!r}")
    return float(level)


def _delong_host(y: np.ndarray, s: np.ndarray):
    """the table of `eoe_delong_counts` from sorts: (T_pos [K], T_neg [K], A [P], B [P], m, n0) for labels y [n] and scores s [K, n].
    With `lt` and `le` the numbers of opposite-side scores below and at-or-below a score (two `searchsorted`), a positive's doubled
    count is lt + le and a negative's 2 m - lt - le."""
    pos, neg = y == 1, y == 0
    m, n0 = int(pos.sum()), int(neg.sum())
    a, b = np.empty((s.shape[0], m), np.int64), np.empty((s.shape[0], n0), np.int64)
    for k, col in enumerate(s):
        sp, sn = col[pos], col[neg]
        if np.isnan(sp).any() or np.isnan(sn).any():
            raise ValueError("scores contain NaN")
        sorted_p, sorted_n = np.sort(sp), np.sort(sn)
        a[k] = np.searchsorted(sorted_n, sp, side="left") + np.searchsorted(sorted_n, sp, side="right")
        b[k] = 2 * m - np.searchsorted(sorted_p, sn, side="left") - np.searchsorted(sorted_p, sn, side="right")
    pairs = _pairs(s.shape[0])
    # int64 holds every sum: at most 16 n^3 / 27 < 2^63 for n <= 2^20
    return (a.sum(axis=1), b.sum(axis=1), np.array([np.dot(a[k], a[l]) for k, l in pairs], np.int64),
            np.array([np.dot(b[k], b[l]) for k, l in pairs], np.int64), m, n0)


def _check_delong_shape(n: int, K: int, n_labels: int):
    if K < 1 or K > DELONG_MAX_COLUMNS:
        raise ValueError(f"an AUC test takes between 1 and {DELONG_MAX_COLUMNS} score columns, not {K}")
    if n_labels != n:
        raise ValueError(f"an AUC test needs as many labels as scores per column, not {n_labels} and {n}")
    if n < 2 or n > DELONG_MAX_N:
        raise ValueError(f"an AUC test takes between 2 and {DELONG_MAX_N} samples, not {n}")


def delong_device(labels, scores):
    """`eoe_delong_counts` on GPU-resident scores [n] or [K, n]: (T_pos int64 [K], T_neg int64 [K], A int64 [K (K + 1) / 2], B the same,
    m, n0, the number of NaN scores) as host arrays and ints -- the raw table, unchecked.  16-bit scores are compared as float32.
    `labels` may live on either device: at most one upload, one call (a memset and three launches) and ONE copy back."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(scores):
        raise RuntimeError("delong_device needs GPU scores (delong takes host arrays as they are)")
    sc = scores.detach()
    sc = (sc.reshape(1, -1) if sc.dim() <= 1 else sc.reshape(sc.shape[0], -1)).contiguous().float()
    K, n = int(sc.shape[0]), int(sc.shape[1])
    la = torch.as_tensor(labels).reshape(-1).to(torch.int64).to(sc.device).contiguous()
    _check_delong_shape(n, K, la.numel())
    P = K * (K + 1) // 2
    out = torch.empty(2 * K + 2 * P + 3, dtype=torch.int64, device=sc.device)
    scratch = torch.empty(lib.eoe_delong_scratch_bytes(n, K), dtype=torch.uint8, device=sc.device)
    with torch.cuda.device(sc.device):
        check(lib.eoe_delong_counts(sc.data_ptr(), la.data_ptr(), n, K, out.data_ptr(), scratch.data_ptr(),
                                    torch.cuda.current_stream(sc.device).cuda_stream), "eoe_delong_counts")
    raw = out.cpu().numpy()
    return (raw[:K].copy(), raw[K:2 * K].copy(), raw[2 * K:2 * K + P].copy(), raw[2 * K + P:2 * K + 2 * P].copy(),
            int(raw[-3]), int(raw[-2]), int(raw[-1]))


def delong(labels, scores) -> Optional[AucTest]:
    """DeLong's confidence intervals and paired tests for the ROC AUCs of `scores` [n] or [K, n] -- K <= 8 models scored on the same n
    samples in the same order -- against `labels` [n] (1: positive, 0: negative, anything else is ignored): see `AucTest`.  None when
    there is no positive or no negative, as the trainer skips the AUC there.

    GPU tensors, or a list of K GPU tensors of one length (stacked on the device), go through `eoe_delong_counts` (exact integer pair
    counts; only 2 K + K (K + 1) + 3 integers come back); host arrays and CPU tensors through sorts.  Both give the same integers,
    and everything after them is the same host code.  Scores are compared as float32 on the device; host float32 stays float32,
    anything else is compared as float64.  -0.0 equals 0.0 and the infinities are ordinary values.

    ValueError for a NaN score among the positives and negatives, for K outside [1, 8], for n outside [2, 2^20] and for another number
    of labels than scores."""
    if isinstance(scores, (list, tuple)) and len(scores) > 0 and all(_is_gpu_tensor(x) for x in scores):
        import torch
        if len({int(x.numel()) for x in scores}) != 1:
            raise ValueError(f"the score columns must have one length, not {[int(x.numel()) for x in scores]}")
        if len(scores) > DELONG_MAX_COLUMNS:
            raise ValueError(f"an AUC test takes between 1 and {DELONG_MAX_COLUMNS} score columns, not {len(scores)}")
        scores = torch.stack([x.detach().reshape(-1).float() for x in scores])
    if _is_gpu_tensor(scores):
        t_pos, t_neg, A, B, m, n0, bad = delong_device(labels, scores)
        if bad:
            raise ValueError("scores contain NaN")
    else:
        s = np.asarray(_to_host(scores)) if not isinstance(scores, (list, tuple)) else np.stack([np.asarray(_to_host(x)).ravel() for x in scores])
        if s.ndim > 1 and s.shape[0] == 0:
            _check_delong_shape(2, 0, 2)
        s = s.reshape(1, -1) if s.ndim <= 1 else s.reshape(s.shape[0], -1)
        if s.dtype != np.float32:
            s = s.astype(np.float64)
        y = np.asarray(_to_host(labels)).ravel()
        _check_delong_shape(s.shape[1], s.shape[0], y.size)
        t_pos, t_neg, A, B, m, n0 = _delong_host(y, s)
    if m == 0 or n0 == 0:
        return None
    return AucTest(t_pos, t_neg, A, B, m, n0)


# ------------------------------------------------------------------------------------------------------ bootstrap
BOOTSTRAP_MAX_N = DELONG_MAX_N            # eoe_bootstrap_counts
BOOTSTRAP_MAX_COLUMNS = DELONG_MAX_COLUMNS
BOOTSTRAP_MAX_REPLICATES = 1 << 16
BOOTSTRAP_CHUNK = 16384                   # sorted positions a workgroup of the replicate pass counts in LDS at a time (EOE_BOOTSTRAP_CHUNK)
BOOTSTRAP_STATS = ("auc", "ap", "fpr")
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011): `counter` [..., 4] and `key` [..., 2] as unsigned 32-bit words (the shapes
    broadcast over the leading axes) -> uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64) & 0xFFFFFFFF
    k = np.asarray(key, dtype=np.uint64) & 0xFFFFFFFF
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead).copy() for i in range(2))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2           # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & mask, (k1 + np.uint64(_PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _bootstrap_positions(size: int, reps: np.ndarray, stratum: int, seed: int) -> np.ndarray:
    """int64 [len(reps), size]: the positions within a stratum of `size` samples that the replicates `reps` draw"""
    calls = (size + 3) // 4
    counter = np.zeros((reps.size, calls, 4), np.uint64)
    counter[..., 0] = np.arange(calls, dtype=np.uint64)[None, :]
    counter[..., 1] = reps.astype(np.uint64)[:, None]
    counter[..., 2] = stratum
    words = philox4x32(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    words = words.reshape(reps.size, calls * 4)[:, :size].astype(np.uint64)       # the unused words of the last call are dropped
    return ((words * np.uint64(size)) >> np.uint64(32)).astype(np.int64)


def _check_seed(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"a bootstrap seed must be an integer in [0, 2^64), not {seed!r}")
    return int(seed)


def _bootstrap_used_counts(m: int, n0: int, reps: np.ndarray, seed: int) -> np.ndarray:
    """int64 [len(reps), m + n0]: per replicate the multiplicity of every used sample, positives first, each stratum in index order"""
    N, R = m + n0, reps.size
    rows = np.arange(R, dtype=np.int64)[:, None] * N
    hit = np.concatenate([(rows + _bootstrap_positions(m, reps, 1, seed)).ravel(), (rows + m + _bootstrap_positions(n0, reps, 0, seed)).ravel()])
    return np.bincount(hit, minlength=R * N).reshape(R, N)


def bootstrap_multiplicities_np(labels, b: int, seed: int = 0) -> np.ndarray:
    """int32 [n]: how often replicate `b` of the stratified bootstrap holds each sample -- m draws with replacement among the m samples
    with label 1 and n0 among the n0 with label 0, each stratum numbered in ascending sample index; 0 for every other label.  Draws
    4j .. 4j+3 of a (replicate, stratum) are the words of `philox4x32((j, b, stratum, 0), (seed & 0xffffffff, seed >> 32))`, stratum 0
    for the negatives and 1 for the positives; a word w selects position (w * size) >> 32."""
    y = np.asarray(_to_host(labels)).ravel()
    seed = _check_seed(seed)
    pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
    out = np.zeros(y.size, np.int32)
    if pos.size == 0 and neg.size == 0:
        return out
    c = _bootstrap_used_counts(pos.size, neg.size, np.array([int(b)], np.int64), seed)[0]
    out[pos], out[neg] = c[:pos.size], c[pos.size:]
    return out


def _check_bootstrap_shape(n: int, K: int, n_labels: int, B):
    if K < 1 or K > BOOTSTRAP_MAX_COLUMNS:
        raise ValueError(f"a bootstrap takes between 1 and {BOOTSTRAP_MAX_COLUMNS} score columns, not {K}")
    if n_labels != n:
        raise ValueError(f"a bootstrap needs as many labels as scores per column, not {n_labels} and {n}")
    if n < 2 or n > BOOTSTRAP_MAX_N:
        raise ValueError(f"a bootstrap takes between 2 and {BOOTSTRAP_MAX_N} samples, not {n}")
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 1 or B > BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"a bootstrap takes between 1 and {BOOTSTRAP_MAX_REPLICATES} replicates, not {B!r}")


def _check_tpr(tpr) -> float:
    if isinstance(tpr, bool) or not isinstance(tpr, (int, float, np.integer, np.floating)) or not 0.0 < float(tpr) <= 1.0:
        raise ValueError(f"tpr must be in (0, 1], not {tpr!r}")
    return float(tpr)


def bootstrap_np(labels, scores, replicates: int = 2000, seed: int = 0, tpr: float = 0.95):
    """The NumPy statement of the stratified, paired bootstrap (`bootstrap`): (u2 int64 [K, B + 1], fps int64 [K, B + 1], ap float64
    [K, B + 1], m, n0) for labels [n] and scores [n] or [K, n].  Column b < B belongs to replicate b, column B to the full sample
    (every multiplicity 1).  With c the multiplicities of `bootstrap_multiplicities_np` (shared by the K columns):

      u2    sum over (positive i, negative j) of c[i] c[j] (2 [s_i > s_j] + [s_i == s_j]); the replicate's AUC is u2 / (2 m n0)
      fps   the weighted negatives at or above the score at place `place_for_tpr(tpr, m)` of the resampled positives in descending
            order; the FPR at that TPR is fps / n0
      ap    sklearn's `average_precision_score` of the resample: over the distinct scores in descending order
            sum (tps_g - tps_{g-1}) / m * (tps_g / (tps_g + fps_g)) with the weighted cumulative counts

    from one stable sort per column, a `bincount` per replicate and `cumsum`s over the groups of equal scores.  float32 scores are
    compared as float32, anything else as float64; -0.0 equals 0.0 and the infinities are ordinary values.  ValueError for a NaN
    among the used scores.  Without a positive or a negative the tables are zeros."""
    y = np.asarray(_to_host(labels)).ravel()
    s = np.asarray(_to_host(scores))
    s = s.reshape(1, -1) if s.ndim <= 1 else s.reshape(s.shape[0], -1)
    if s.dtype != np.float32:
        s = s.astype(np.float64)
    K, n = s.shape
    B, seed, tpr = replicates, _check_seed(seed), _check_tpr(tpr)
    _check_bootstrap_shape(n, K, y.size, B)
    B = int(B)
    pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
    m, n0 = int(pos.size), int(neg.size)
    N = m + n0
    u2, fps, ap = np.zeros((K, B + 1), np.int64), np.zeros((K, B + 1), np.int64), np.zeros((K, B + 1), np.float64)
    used = np.concatenate([pos, neg])
    if np.isnan(s[:, used]).any():
        raise ValueError("scores contain NaN")
    if m == 0 or n0 == 0:
        return u2, fps, ap, m, n0
    place = place_for_tpr(tpr, m)
    cols = []
    for k in range(K):
        su = s[k, used]
        perm = np.argsort(su, kind="stable")
        ss = su[perm]
        starts = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
        cols.append((perm, starts, (perm < m).astype(np.int64)))
    step = max(1, (1 << 21) // N)
    for b0 in range(0, B + 1, step):
        reps = np.arange(b0, min(b0 + step, B + 1), dtype=np.int64)
        full = reps[-1] == B
        c = _bootstrap_used_counts(m, n0, reps[:-1] if full else reps, seed)
        if full:
            c = np.concatenate([c, np.ones((1, N), np.int64)])
        sl = slice(b0, b0 + reps.size)
        for k, (perm, starts, is_pos) in enumerate(cols):
            cs = c[:, perm]
            posw = np.add.reduceat(cs * is_pos, starts, axis=1)                   # [R, groups], ascending score
            negw = np.add.reduceat(cs * (1 - is_pos), starts, axis=1)
            p_lt, n_lt = np.cumsum(posw, axis=1) - posw, np.cumsum(negw, axis=1) - negw
            u2[k, sl] = (posw * (2 * n_lt + negw)).sum(axis=1)
            tps, fpc = m - p_lt, n0 - n_lt                                        # the descending curve's counts at each group
            at = (tps >= place).sum(axis=1) - 1                                   # tps falls along the groups: the last one that holds the place
            fps[k, sl] = fpc[np.arange(reps.size), at]
            with np.errstate(invalid="ignore", divide="ignore"):
                term = np.where(posw > 0, (posw / m) * (tps / (tps + fpc).astype(np.float64)), 0.0)
            ap[k, sl] = term[:, ::-1].sum(axis=1)
    return u2, fps, ap, m, n0


def bootstrap_device(labels, scores, replicates: int = 2000, seed: int = 0, tpr: float = 0.95):
    """`eoe_bootstrap_counts` on GPU-resident scores [n] or [K, n]: (u2 int64 [K, B + 1], fps int64 [K, B + 1], ap float64 [K, B + 1], m,
    n0, the number of NaN scores) as host arrays and ints -- the raw tables of `bootstrap_np`, unchecked.  16-bit scores are compared
    as float32.  `labels` may live on either device: at most one upload, one call (a memset and four launches) and ONE copy back."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(scores):
        raise RuntimeError("bootstrap_device needs GPU scores (bootstrap takes host arrays as they are)")
    sc = scores.detach()
    sc = (sc.reshape(1, -1) if sc.dim() <= 1 else sc.reshape(sc.shape[0], -1)).contiguous().float()
    K, n = int(sc.shape[0]), int(sc.shape[1])
    la = torch.as_tensor(labels).reshape(-1).to(torch.int64).to(sc.device).contiguous()
    seed, tpr = _check_seed(seed), _check_tpr(tpr)
    _check_bootstrap_shape(n, K, la.numel(), replicates)
    B = int(replicates)
    T = K * (B + 1)
    out = torch.empty(3 * T + 2, dtype=torch.int64, device=sc.device)      # u2 | fps | ap (float64 bits) | counts (three int32)
    scratch = torch.empty(lib.eoe_bootstrap_scratch_bytes(n, K, B), dtype=torch.uint8, device=sc.device)
    base = out.data_ptr()
    with torch.cuda.device(sc.device):
        check(lib.eoe_bootstrap_counts(sc.data_ptr(), la.data_ptr(), n, K, B, seed, tpr, base, base + 8 * T, base + 16 * T, base + 24 * T,
                                       scratch.data_ptr(), torch.cuda.current_stream(sc.device).cuda_stream), "eoe_bootstrap_counts")
    raw = out.cpu().numpy()
    m, n0, bad = (int(x) for x in raw[3 * T:].view(np.int32)[:3])
    return (raw[:T].reshape(K, B + 1).copy(), raw[T:2 * T].reshape(K, B + 1).copy(), raw[2 * T:3 * T].view(np.float64).reshape(K, B + 1).copy(),
            m, n0, bad)


def bootstrap_multiplicities_device(labels, b: int, seed: int = 0) -> np.ndarray:
    """`eoe_bootstrap_draws`: `bootstrap_multiplicities_np` drawn on the device, for telling a difference in the draws from one in the
    counting.  `labels`: a tensor on the GPU."""
    import torch
    from ._lib import check, lib
    if not _is_gpu_tensor(labels):
        raise RuntimeError("bootstrap_multiplicities_device needs GPU labels")
    la = labels.detach().reshape(-1).to(torch.int64).contiguous()
    n, seed = int(la.numel()), _check_seed(seed)
    _check_bootstrap_shape(n, 1, n, 1)
    if not 0 <= int(b) < BOOTSTRAP_MAX_REPLICATES:
        raise ValueError(f"a replicate's number must be in [0, {BOOTSTRAP_MAX_REPLICATES}), not {b}")
    out = torch.empty(n, dtype=torch.int32, device=la.device)
    scratch = torch.empty(lib.eoe_bootstrap_scratch_bytes(n, 1, 1), dtype=torch.uint8, device=la.device)
    with torch.cuda.device(la.device):
        check(lib.eoe_bootstrap_draws(la.data_ptr(), n, int(b), seed, out.data_ptr(), scratch.data_ptr(),
                                      torch.cuda.current_stream(la.device).cuda_stream), "eoe_bootstrap_draws")
    return out.cpu().numpy()


class Bootstrap:
    """The stratified, paired bootstrap of K score columns over the same test samples: what an AUC, an average precision or an FPR at a
    TPR level -- or a difference of two of them -- is worth on a test set of this size, without DeLong's normal approximation.

      auc, ap, fpr [K]                    the statistics of the full sample;  tpr  the level of `fpr`
      auc_reps, ap_reps, fpr_reps [K, B]  the replicates' (float64; one division per entry: u2 / (2 m n0), fps / n0)
      n_pos, n_neg, replicates, seed
      counts   the tables everything is divided from: {"u2", "fps": int64 [K, B + 1], "ap": float64 [K, B + 1]}, column B the full sample

    Every replicate draws n_pos positives and n_neg negatives with replacement, and the K columns share the draws, so differences
    between columns are paired.  `stat` is one of "auc", "ap", "fpr"."""

    def __init__(self, u2, fps, ap, n_pos: int, n_neg: int, seed: int = 0, tpr: float = 0.95):
        u2, fps, ap = np.asarray(u2, np.int64), np.asarray(fps, np.int64), np.asarray(ap, np.float64)
        self.n_pos, self.n_neg, self.seed, self.tpr = int(n_pos), int(n_neg), int(seed), float(tpr)
        if self.n_pos < 1 or self.n_neg < 1 or u2.ndim != 2 or u2.shape[1] < 2 or u2.shape != fps.shape or u2.shape != ap.shape:
            raise ValueError("a bootstrap needs both classes and three tables of K x (B + 1) numbers")
        self.counts = {"u2": u2, "fps": fps, "ap": ap}
        self.replicates = u2.shape[1] - 1
        auc, fpr = u2 / float(2 * self.n_pos * self.n_neg), fps / float(self.n_neg)         # int64 -> float64 is exact below 2^53
        self.auc, self.ap, self.fpr = auc[:, -1].copy(), ap[:, -1].copy(), fpr[:, -1].copy()
        self.auc_reps, self.ap_reps, self.fpr_reps = auc[:, :-1].copy(), ap[:, :-1].copy(), fpr[:, :-1].copy()

    def _reps(self, stat: str) -> np.ndarray:
        if stat not in BOOTSTRAP_STATS:
            raise ValueError(f"stat must be one of {BOOTSTRAP_STATS}, not {stat!r}")
        return getattr(self, stat + "_reps")

    def se(self, stat: str = "auc") -> np.ndarray:
        """[K]: the replicates' standard deviation (ddof = 1; 0 with one replicate)"""
        r = self._reps(stat)
        return r.std(axis=1, ddof=1) if r.shape[1] > 1 else np.zeros(r.shape[0])

    def ci(self, level: float = 0.95, stat: str = "auc"):
        """(lo [K], hi [K]): the percentile interval, `np.quantile(reps, (1 -+ level) / 2, method="linear")`"""
        level = _check_level(level)
        r = self._reps(stat)
        return (np.quantile(r, (1.0 - level) / 2.0, axis=1, method="linear"), np.quantile(r, (1.0 + level) / 2.0, axis=1, method="linear"))

    def _diffs(self, stat: str):
        r = self._reps(stat)
        return [r[k] - r[l] for k, l in _pairs(r.shape[0])]

    def diff_ci(self, level: float = 0.95, stat: str = "auc"):
        """(lo [P], hi [P]) over the pairs (k, l), k <= l, row by row (the order of `AucTest`'s upper triangles): the percentile
        interval of stat[k] - stat[l] over the shared replicates; [0, 0] for k == l"""
        level = _check_level(level)
        d = np.stack(self._diffs(stat))
        return (np.quantile(d, (1.0 - level) / 2.0, axis=1, method="linear"), np.quantile(d, (1.0 + level) / 2.0, axis=1, method="linear"))

    def diff_p(self, stat: str = "auc") -> np.ndarray:
        """[P], the same pairs: the two-sided bootstrap p-value of "the difference is 0", 2 min(#(d <= 0) + 1, #(d >= 0) + 1) / (B + 1)
        capped at 1"""
        B = self.replicates
        return np.array([min(1.0, 2.0 * min(int((d <= 0).sum()) + 1, int((d >= 0).sum()) + 1) / (B + 1)) for d in self._diffs(stat)])

    def to_json(self, level: float = 0.95) -> dict:
        """ints, floats and lists: strict JSON"""
        lst = lambda a: [float(x) for x in a]                                                        # noqa: E731
        out = {"n_pos": self.n_pos, "n_neg": self.n_neg, "replicates": self.replicates, "seed": self.seed, "tpr": self.tpr,
               "level": float(_check_level(level)), "pairs": [list(p) for p in _pairs(self.auc.size)]}
        for stat in BOOTSTRAP_STATS:
            (lo, hi), (dlo, dhi) = self.ci(level, stat), self.diff_ci(level, stat)
            out[stat] = {"value": lst(getattr(self, stat)), "se": lst(self.se(stat)), "ci_lo": lst(lo), "ci_hi": lst(hi),
                         "diff_ci_lo": lst(dlo), "diff_ci_hi": lst(dhi), "diff_p": lst(self.diff_p(stat))}
        return out

    def __repr__(self):
        return (f"Bootstrap(auc={self.auc.tolist()}, ap={self.ap.tolist()}, fpr={self.fpr.tolist()}, replicates={self.replicates}, "
                f"n_pos={self.n_pos}, n_neg={self.n_neg})")


def bootstrap(labels, scores, replicates: int = 2000, seed: int = 0, tpr: float = 0.95) -> Optional[Bootstrap]:
    """Bootstrap intervals and paired tests for the ROC AUC, the average precision and the FPR at the TPR level `tpr` of `scores` [n]
    or [K, n] -- K <= 8 models scored on the same n samples in the same order -- against `labels` [n] (1: positive, 0: negative,
    anything else is ignored): see `Bootstrap`.  None when there is no positive or no negative.

    The resampling is stratified and stated exactly (`bootstrap_multiplicities_np`: Philox4x32-10 counters, so a replicate is a
    function of (seed, b) alone and neither of the order of evaluation nor of the device).  A position is selected by multiply-shift
    without rejection, (w * size) >> 32: its probability is off from 1 / size by less than size / 2^32 (2.4e-4 relative at the cap of
    2^20 samples, 2e-6 at 10 000), far below what B <= 65 536 replicates resolve.

    GPU tensors, or a list of K GPU tensors of one length (stacked on the device), go through `eoe_bootstrap_counts` (csrc/bootstrap.hip:
    every replicate is resampled and counted on the device, 3 K (B + 1) numbers come back in one copy); host arrays and CPU tensors
    through `bootstrap_np`.  Both give the same integers, the APs agree within 4 n 2^-53, and everything after the tables is the same
    host code.  Scores are compared as float32 on the device; host float32 stays float32, anything else is compared as float64.

    ValueError for a NaN score among the positives and negatives, for K outside [1, 8], n outside [2, 2^20], `replicates` outside
    [1, 65 536], `tpr` outside (0, 1] and for another number of labels than scores."""
    seed, tpr = _check_seed(seed), _check_tpr(tpr)
    if isinstance(scores, (list, tuple)) and len(scores) > 0 and all(_is_gpu_tensor(x) for x in scores):
        import torch
        if len({int(x.numel()) for x in scores}) != 1:
            raise ValueError(f"the score columns must have one length, not {[int(x.numel()) for x in scores]}")
        if len(scores) > BOOTSTRAP_MAX_COLUMNS:
            raise ValueError(f"a bootstrap takes between 1 and {BOOTSTRAP_MAX_COLUMNS} score columns, not {len(scores)}")
        scores = torch.stack([x.detach().reshape(-1).float() for x in scores])
    if _is_gpu_tensor(scores):
        u2, fps, ap, m, n0, bad = bootstrap_device(labels, scores, replicates, seed, tpr)
        if bad:
            raise ValueError("scores contain NaN")
    else:
        if isinstance(scores, (list, tuple)):
            if len(scores) == 0:
                _check_bootstrap_shape(2, 0, 2, 1)
            if len({int(np.asarray(_to_host(x)).size) for x in scores}) != 1:
                raise ValueError("the score columns must have one length")
            scores = np.stack([np.asarray(_to_host(x)).ravel() for x in scores])
        s = np.asarray(_to_host(scores))
        if s.ndim > 1 and s.shape[0] == 0:
            _check_bootstrap_shape(2, 0, 2, 1)
        u2, fps, ap, m, n0 = bootstrap_np(labels, s, replicates, seed, tpr)
    if m == 0 or n0 == 0:
        return None
    return Bootstrap(u2, fps, ap, m, n0, seed, tpr)
