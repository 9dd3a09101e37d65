"""Representatives of a feature set: the greedy k-center (farthest-point) coreset that feature-bank detectors of the PatchCore / SPADE
family keep in place of all normal training features.  m rows are chosen one after the other, each the row that lies farthest from
the centres chosen so far; the covering radius they reach is within a factor 2 of the best any m rows can reach.

  kcenter(x, m, start=0)          -> `Coreset`.  GPU tensors go through `eoe_feature_coreset` (csrc/coreset.hip: one streaming pass over
                                  x per centre, the next centre's index stays on the device); CPU tensors and arrays through `kcenter_np`.
                                  `m` is a number of rows or a float in (0, 1), the share ceil(m n) of them.
  kcenter_np(x, m, start=0)       the statement of the result in float64 NumPy.
  kcenter_device(x, m, start=0)   the raw device outputs of `eoe_feature_coreset`; nothing comes back to the host.

One contract for both routes.  idx[0] = start; idx[t] is the eligible, not yet chosen row with the largest squared distance to its
nearest centre among idx[:t], equal distances to the lowest row; radius[t] is that squared distance, radius[0] = +inf.  assign[i] is the
position of row i's nearest centre, the earliest chosen one on equal distances (updated only on strictly smaller), d2min[i] that squared
distance; a centre has its own position and 0.  A row with a NaN or an infinity is never a centre: assign = -1, d2min = NaN, counted in
`nonfinite`; as `start` it raises ValueError.  With fewer than m eligible rows the tail holds idx = -1, radius = NaN.  The distance is
sum((x - c)^2), the difference form: a row next to a centre keeps its distance, integer-valued features give exact results.
"""
import math

import numpy as np

from .neighbors import _host, _rows

CORESET_MAX_D = 2048
CORESET_MAX_ROWS = (1 << 24) - 1
CORESET_ROWS_PER_WAVE = 8              # csrc/coreset.hip: CS_W, the rows a wave takes ...
CORESET_ROWS_PER_WORKGROUP = 32        # ... and CS_R, the rows of a workgroup (the edge shapes of the tests)


class Coreset:
    """`idx` int64 [m]: the chosen rows in the order chosen (-1: no eligible row was left); `radius` fp32 [m]: the squared distance of
    each to the centres before it (+inf first); `assign` int64 [n]: the position in `idx` of every row's nearest centre (-1: a
    non-finite row); `d2min` fp32 [n]: the squared distance to it; `nonfinite`: the rows that hold a NaN or an infinity.  Tensors, on
    the device of the features."""

    def __init__(self, idx, radius, assign, d2min, nonfinite):
        self.idx, self.radius, self.assign, self.d2min = idx, radius, assign, d2min
        self.nonfinite = int(nonfinite)

    @property
    def m(self) -> int:
        return int(self.idx.shape[0])

    @property
    def n(self) -> int:
        return int(self.assign.shape[0])

    def cover(self) -> float:
        """the covering radius after all m centres, a distance: the square root of the largest finite `d2min` (NaN: no finite row)"""
        d2 = self.d2min[self.assign >= 0]
        return math.sqrt(float(d2.max())) if d2.numel() else float("nan")

    def sizes(self):
        """int64 [m]: the rows every centre is the nearest one of, itself included"""
        import torch
        a = self.assign[self.assign >= 0]
        return torch.bincount(a, minlength=self.m)[:self.m]

    def as_dict(self, ref_ids=None) -> dict:
        """{"m", "n", "nonfinite", "cover", "centres": [id, ...], "radius": [distance, ...], "sizes": [rows, ...]}: ints and floats,
        for JSON.  `ref_ids` maps rows to dataset indices (default: the rows themselves); the radius curve is in distances, not
        squares, and starts at its second entry (the first centre has none); positions without a centre (idx -1) are left out."""
        idx = self.idx.detach().cpu().numpy()
        refs = None if ref_ids is None else np.asarray(_host(ref_ids)).ravel()
        if refs is not None and refs.size != self.n:
            raise ValueError(f"ref_ids must name every row: {refs.size} for {self.n} rows")
        have = idx >= 0
        radius = self.radius.detach().cpu().numpy().astype(np.float64)
        return {"m": self.m, "n": self.n, "nonfinite": self.nonfinite, "cover": self.cover(),
                "centres": [int(j if refs is None else refs[j]) for j in idx[have]],
                "radius": [float(math.sqrt(r)) for r in radius[have][1:]],
                "sizes": [int(s) for s in self.sizes().cpu().numpy()[have]]}

    def __repr__(self):
        return f"Coreset(m={self.m}, n={self.n}, nonfinite={self.nonfinite})"


def _check_m(m, n: int) -> int:
    """the number of centres: an integer in [1, n], or a float in (0, 1) for ceil(m n) (at least 1)"""
    if isinstance(m, (float, np.floating)):
        if not 0.0 < m < 1.0:
            raise ValueError(f"m as a share of the rows must be a float in (0, 1), not {m!r}")
        return max(1, min(n, int(math.ceil(float(m) * n))))
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= n:
        raise ValueError(f"m must be an integer in [1, n = {n}] or a float in (0, 1), not {m!r}")
    return int(m)


def _check_start(start, n: int) -> int:
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= start < n:
        raise ValueError(f"start must be an integer in [0, n = {n}), not {start!r}")
    return int(start)


def _check_shape(shape):
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError(f"x must be [n, D] with at least one row, not {tuple(shape)}")
    if not 1 <= shape[1] <= CORESET_MAX_D:
        raise ValueError(f"the feature width must be in [1, {CORESET_MAX_D}], not {shape[1]}")
    if shape[0] > CORESET_MAX_ROWS:
        raise ValueError(f"eoe_feature_coreset takes fewer than 2^24 rows, not {shape[0]}")


def kcenter_np(x, m, start: int = 0):
    """(idx int64 [m], radius float64 [m], assign int64 [n], d2min float64 [n], non-finite rows): greedy k-center with
    d2 = sum((x - c)^2) in float64, the running minimum updated on strictly smaller, then `np.argmax` over the eligible rows (the
    first of equal maxima: the lowest row)."""
    x = np.asarray(_host(x), dtype=np.float64)
    _check_shape(x.shape)
    n = x.shape[0]
    m, start = _check_m(m, n), _check_start(start, n)
    ok = np.isfinite(x).all(axis=1)
    if not ok[start]:
        raise ValueError(f"the start row {start} holds a NaN or an infinity")
    idx = np.full(m, -1, np.int64)
    radius = np.full(m, np.nan, np.float64)
    assign = np.where(ok, 0, -1).astype(np.int64)
    d2min = np.full(n, np.nan, np.float64)
    elig = ok.copy()                                     # finite and not yet chosen
    xs = np.where(ok[:, None], x, 0.0)
    c, r = start, np.inf
    for t in range(m):
        idx[t], radius[t] = c, r
        diff = xs - xs[c]
        d2 = np.einsum("nd,nd->n", diff, diff)
        with np.errstate(invalid="ignore"):              # NaN marks a row without a distance yet, and a non-finite one for good
            upd = (ok & (d2 < d2min)) if t else ok
        d2min[upd], assign[upd] = d2[upd], t
        d2min[c], assign[c], elig[c] = 0.0, t, False
        if not elig.any():
            break
        cand = np.where(elig, d2min, -1.0)
        c = int(np.argmax(cand))
        r = cand[c]
    return idx, radius, assign, d2min, int((~ok).sum())


def kcenter_device(x, m: int, start: int = 0, scratch=None):
    """`eoe_feature_coreset` on a GPU-resident fp32 [n, D] tensor (rows may be strided, the last axis is contiguous): (idx int32 [m],
    radius fp32 [m], assign int32 [n], d2min fp32 [n], counts int32 [2] = {non-finite rows, 1 if `start` is one}) on the device;
    nothing comes back to the host.  `scratch`: a uint8 GPU tensor of at least `eoe_feature_coreset_scratch_bytes(n, D, m)` bytes to
    reuse (its content does not matter)."""
    import torch
    from ._lib import check, lib
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise RuntimeError("kcenter_device needs a GPU tensor (kcenter takes host arrays as they are)")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"x must be a 2-D float32 tensor, not {tuple(x.shape)} {x.dtype}")
    _check_shape(x.shape)
    n, D = x.shape
    if isinstance(m, (float, np.floating)):
        raise ValueError(f"kcenter_device takes the number of centres, not a share ({m!r}); kcenter resolves one")
    m, start = _check_m(m, n), _check_start(start, n)
    xr, ldx = _rows(x.detach(), D)
    dev = xr.device
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    radius = torch.empty(m, dtype=torch.float32, device=dev)
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    d2min = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    need = lib.eoe_feature_coreset_scratch_bytes(n, D, m)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.dtype != torch.uint8 or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous() \
            or scratch.data_ptr() % 16:
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {dev}")
    with torch.cuda.device(dev):
        check(lib.eoe_feature_coreset(xr.data_ptr(), ldx, n, D, m, start, idx.data_ptr(), radius.data_ptr(), assign.data_ptr(),
                                      d2min.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), "eoe_feature_coreset")
    return idx, radius, assign, d2min, counts


def kcenter(x, m, start: int = 0) -> Coreset:
    """The greedy k-center coreset of the rows of `x` [n, D] (fp32): GPU tensors through `eoe_feature_coreset`, CPU tensors and
    arrays through `kcenter_np`; the same contract either way (the module docstring).  `m`: the number of centres, or a float in
    (0, 1) for ceil(m n) of the rows."""
    import torch
    if hasattr(x, "is_cuda") and x.is_cuda:
        if x.dim() != 2:
            raise ValueError(f"x must be [n, D], not {tuple(x.shape)}")
        m = _check_m(m, int(x.shape[0]))
        idx, radius, assign, d2min, counts = kcenter_device(x, m, start)
        bad, bad_start = counts.tolist()
        if bad_start:
            raise ValueError(f"the start row {start} holds a NaN or an infinity")
        return Coreset(idx.to(torch.int64), radius, assign.to(torch.int64), d2min, bad)
    if hasattr(x, "dtype") and hasattr(x, "is_cuda") and x.dtype != torch.float32:
        raise ValueError(f"x must be float32, not {x.dtype}")
    idx, radius, assign, d2min, bad = kcenter_np(x, m, start)
    return Coreset(torch.from_numpy(idx), torch.from_numpy(radius.astype(np.float32)), torch.from_numpy(assign),
                   torch.from_numpy(d2min.astype(np.float32)), bad)
