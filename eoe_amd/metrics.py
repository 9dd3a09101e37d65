"""Epoch-tail metrics of the trainer (`src/eoe/training/ad_trainer.py:452-455,516-522`): the reference calls
sklearn's `roc_curve` + `auc` (trapezoid) and `average_precision_score` on host copies of the epoch's labels and
scores.  Same place (host, once per epoch), written as the tie-aware rank statistic, which equals the trapezoidal
ROC area, and the step-wise precision-recall sum.

The curves themselves (`roc_curve`, `precision_recall_curve` below) come from one table of exact integer counts per distinct
score -- `eoe_rank_curves` for GPU tensors, a sort for host arrays -- and sklearn's finishing steps in float64 on the host.

The score histograms the reference logs next to them (`:458-465, 541-546`, TensorBoard's `add_histogram`) are `score_histogram` /
`score_histograms`: integer counts over TensorBoard's fixed edges -- `eoe_score_hist` for GPU tensors, `np.histogram` for host
arrays -- and the same trimming of the integer arrays on the host."""
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
