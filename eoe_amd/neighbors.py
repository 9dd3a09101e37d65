"""Nearest neighbours in feature space: which normal training images an encoder thinks a test image resembles, and the feature-space
k-NN anomaly score that outlier-exposure results are compared against.

  feature_knn(queries, refs, k)   the k nearest rows of `refs` per row of `queries` by squared Euclidean distance -> `Neighbors`.
                                  GPU tensors go through `eoe_feature_knn` (csrc/knn.hip: distances on the fp32 matrix cores, the
                                  selection fused behind them, no nq x nr matrix in memory); CPU tensors and arrays through `knn_np`.
  knn_np(q, r, k)                 the statement of the result in float64 NumPy: a stable argsort of the distances.
  knn_score(neigh, mode)          the k-NN anomaly score: the mean of the k distances or the k-th one.
  embed(model, batches)           the features of a list of batches, fp32 [n, D].

One contract for both routes: ascending by distance, equal distances by ascending reference index; fewer than k eligible references
leave idx = -1, d2 = +inf in the tail; a reference row with a NaN or an infinity is never returned; a query row with one gets
idx = -1, d2 = NaN throughout; `nonfinite` counts both kinds of rows.
"""
from typing import Optional

import numpy as np

KNN_MAX_K = 64
KNN_MAX_D = 2048
KNN_MAX_REFS = (1 << 24) - 1


class Neighbors:
    """`idx` int64 [nq, k]: rows of the reference set, nearest first (-1: no such neighbour); `d2` fp32 [nq, k]: their squared
    distances; `nonfinite` = (query rows, reference rows) that hold a NaN or an infinity.  Tensors, on the device of the queries."""

    def __init__(self, idx, d2, nonfinite):
        self.idx, self.d2 = idx, d2
        self.nonfinite = (int(nonfinite[0]), int(nonfinite[1]))

    @property
    def k(self) -> int:
        return int(self.idx.shape[1])

    def dist(self):
        """the Euclidean distances, fp32 [nq, k]"""
        return self.d2.sqrt()

    def as_dict(self, row_ids=None, ref_ids=None) -> dict:
        """{"k": k, "nonfinite": [q, r], "rows": [{"row": id, "neighbors": [[ref id, distance], ...]}, ...]}: ints and floats, for
        JSON.  `row_ids` names the query rows (default: their position), `ref_ids` maps reference rows to dataset indices; a missing
        neighbour (idx -1) is left out."""
        idx = self.idx.detach().cpu().numpy()
        dist = self.dist().detach().cpu().numpy()
        rows = np.arange(idx.shape[0]) if row_ids is None else np.asarray(_host(row_ids)).ravel()
        if rows.size != idx.shape[0]:
            raise ValueError(f"row_ids must name every query row: {rows.size} for {idx.shape[0]} rows")
        refs = None if ref_ids is None else np.asarray(_host(ref_ids)).ravel()
        name = (lambda j: int(j)) if refs is None else (lambda j: int(refs[j]))
        return {"k": self.k, "nonfinite": list(self.nonfinite),
                "rows": [{"row": int(rows[i]), "neighbors": [[name(j), float(d)] for j, d in zip(idx[i], dist[i]) if j >= 0]}
                         for i in range(idx.shape[0])]}

    def __repr__(self):
        return f"Neighbors(nq={self.idx.shape[0]}, k={self.k}, nonfinite={self.nonfinite})"


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def _check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be an integer in [1, {KNN_MAX_K}], not {k!r}")
    return int(k)


def knn_np(q, r, k: int):
    """(idx int64 [nq, k], d2 float64 [nq, k], (non-finite query rows, non-finite reference rows)): per query
    `np.argsort(d2_row, kind="stable")[:k]` over the finite reference rows with d2 = sum((q - r)^2) in float64."""
    k = _check_k(k)
    q, r = np.asarray(_host(q), dtype=np.float64), np.asarray(_host(r), dtype=np.float64)
    if q.ndim != 2 or r.ndim != 2 or q.shape[1] != r.shape[1]:
        raise ValueError(f"queries and refs must be [nq, D] and [nr, D], not {q.shape} and {r.shape}")
    nq, D = q.shape
    q_ok, r_ok = np.isfinite(q).all(axis=1), np.isfinite(r).all(axis=1)
    elig = np.flatnonzero(r_ok)
    re = r[elig]
    idx = np.full((nq, k), -1, np.int64)
    d2 = np.full((nq, k), np.inf, np.float64)
    d2[~q_ok] = np.nan
    m = min(k, elig.size)
    step = max(1, (1 << 24) // max(1, elig.size * max(D, 1)))
    good = np.flatnonzero(q_ok)
    for lo in range(0, good.size if m else 0, step):
        rows = good[lo:lo + step]
        diff = q[rows, None, :] - re[None, :, :]
        dd = np.einsum("qrd,qrd->qr", diff, diff)
        order = np.argsort(dd, axis=1, kind="stable")[:, :m]
        idx[rows, :m] = elig[order]
        d2[rows, :m] = np.take_along_axis(dd, order, axis=1)
    return idx, d2, (int((~q_ok).sum()), int((~r_ok).sum()))


def _rows(t, D):
    """(tensor, row stride in elements): `t` as it is where its rows are contiguous and at least D apart, else a contiguous copy"""
    ok = (D == 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= D)
    t = t if ok else t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else D)


def feature_knn_device(queries, refs, k: int, scratch=None):
    """`eoe_feature_knn` on GPU-resident fp32 [nq, D] and [nr, D] tensors (rows may be strided, the last axis is contiguous):
    (idx int32 [nq, k], d2 fp32 [nq, k], counts int32 [2]) on the device; nothing comes back to the host.  `scratch`: a uint8 GPU
    tensor of at least `eoe_feature_knn_scratch_bytes(nq, nr, D, k)` bytes to reuse (its content does not matter)."""
    import torch
    from ._lib import check, lib
    k = _check_k(k)
    for name, t in (("queries", queries), ("refs", refs)):
        if not (hasattr(t, "is_cuda") and t.is_cuda):
            raise RuntimeError(f"feature_knn_device needs GPU tensors ({name} is not one; feature_knn takes host arrays as they are)")
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{name} must be a 2-D float32 tensor, not {tuple(t.shape)} {t.dtype}")
    if queries.shape[1] != refs.shape[1] or refs.device != queries.device:
        raise ValueError(f"queries {tuple(queries.shape)} and refs {tuple(refs.shape)} must share their width and their device")
    nq, D = queries.shape
    nr = refs.shape[0]
    if not 1 <= D <= KNN_MAX_D:
        raise ValueError(f"the feature width must be in [1, {KNN_MAX_D}], not {D}")
    if nr > KNN_MAX_REFS:
        raise ValueError(f"eoe_feature_knn takes fewer than 2^24 reference rows, not {nr}")
    (q, ldq), (r, ldr) = _rows(queries.detach(), D), _rows(refs.detach(), D)
    dev = q.device
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    need = lib.eoe_feature_knn_scratch_bytes(nq, nr, D, k)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.dtype != torch.uint8 or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous() \
            or scratch.data_ptr() % 16:
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {dev}")
    if nq == 0:
        return idx, d2, counts
    rp = r.data_ptr() if nr else q.data_ptr()            # an empty tensor has no storage to point at; nothing of it is read
    with torch.cuda.device(dev):
        check(lib.eoe_feature_knn(q.data_ptr(), ldq, rp, ldr, nq, nr, D, k, idx.data_ptr(), d2.data_ptr(), counts.data_ptr(),
                                  scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "eoe_feature_knn")
    return idx, d2, counts


def feature_knn(queries, refs, k: int) -> Neighbors:
    """The k nearest rows of `refs` [nr, D] for every row of `queries` [nq, D] (fp32): GPU tensors through `eoe_feature_knn`, CPU
    tensors and arrays through `knn_np`; the same contract either way (the module docstring)."""
    import torch
    k = _check_k(k)
    if hasattr(queries, "is_cuda") and queries.is_cuda:
        idx, d2, counts = feature_knn_device(queries, refs, k)
        return Neighbors(idx.to(torch.int64), d2, counts.tolist() if queries.shape[0] else _count_rows(queries, refs))
    for name, t in (("queries", queries), ("refs", refs)):
        if hasattr(t, "dtype") and hasattr(t, "is_cuda") and t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, not {t.dtype}")
    idx, d2, bad = knn_np(queries, refs, k)
    return Neighbors(torch.from_numpy(idx), torch.from_numpy(d2.astype(np.float32)), bad)


def _count_rows(queries, refs):
    import torch
    return (0, int((~torch.isfinite(refs).all(dim=1)).sum()) if refs.shape[0] else 0)


def knn_score(neigh: Neighbors, mode: str = "mean"):
    """the feature-space k-NN anomaly score, fp32 [nq], where the neighbours lie: the mean of the k distances ("mean") or the k-th
    distance ("kth"); distances, not squares.  A query with fewer than k neighbours scores +inf, a non-finite one NaN."""
    if mode not in ("mean", "kth"):
        raise ValueError(f"mode must be 'mean' or 'kth', not {mode!r}")
    dist = neigh.dist()
    return dist.mean(dim=1) if mode == "mean" else dist[:, -1].clone()


def embed(model, batches, trainer=None, nominal: int = 0):
    """fp32 [n, D]: `model(x)` of every batch, concatenated, in eval mode under `no_grad` (the model's mode is put back).  A batch is
    a tensor or a tuple whose first entry is one (and whose second may hold the labels; default: all `nominal`).  With `trainer` the
    images first pass the trainer's test-time steps (`_test_time_inputs`: test MSMs, GCN) and the model runs in the arithmetic
    `eval_cls` scores in."""
    import torch
    from . import ops
    was_training = model.training
    model.eval()
    dev = next((p.device for p in model.parameters()), None)
    prev_parity = ops.parity_mode()
    if trainer is not None:
        ops.set_parity_mode(trainer._exact_bn_for(model) or prev_parity)
    feats = []
    try:
        for batch in batches:
            x, rest = (batch[0], batch[1:]) if isinstance(batch, (tuple, list)) else (batch, ())
            if dev is not None:
                x = x.to(dev)
            if trainer is not None:
                lbls = rest[0] if rest else torch.full((x.shape[0],), nominal, dtype=torch.int64)
                x = trainer._test_time_inputs(x, lbls, nominal)
            with torch.no_grad():
                f = model(x)
            f = f.reshape(f.shape[0], -1).float()
            if f.shape[1] < 2:
                raise ValueError("a classifier head has no embedding; use an objective with a feature output")
            feats.append(f)
    finally:
        ops.set_parity_mode(prev_parity)
        model.train(was_training)
    if not feats:
        raise ValueError("embed needs at least one batch")
    return torch.cat(feats)
