"""What the bootstrap tests share: the plain-Python statement of a replicate's three numbers -- a double loop over the pairs of the
resample written out with its repeats, the threshold read off the sorted positives, the AP by its hand formula -- and the score
cases.  Nothing here sorts with NumPy or uses a cumulative sum: it is the independent side of `metrics.bootstrap_np`."""
import math

import numpy as np

from eoe_amd import metrics


def brute(labels, scores, replicates, seed, tpr):
    """(u2, fps, ap) as lists [K][B + 1] (column B: the full sample), m, n0 -- floats compared as Python floats of the float32 values"""
    y = np.asarray(labels).ravel()
    s = np.asarray(scores, np.float32)
    s = s.reshape(1, -1) if s.ndim == 1 else s
    m, n0 = int((y == 1).sum()), int((y == 0).sum())
    place = metrics.place_for_tpr(tpr, m)
    mults = [metrics.bootstrap_multiplicities_np(y, b, seed) for b in range(replicates)] + [((y == 1) | (y == 0)).astype(np.int32)]
    u2, fps, ap = [], [], []
    for col in s:
        u2.append([]), fps.append([]), ap.append([])
        for c in mults:
            pos = [float(col[i]) for i in range(y.size) if y[i] == 1 for _ in range(int(c[i]))]
            neg = [float(col[i]) for i in range(y.size) if y[i] == 0 for _ in range(int(c[i]))]
            assert len(pos) == m and len(neg) == n0
            u2[-1].append(sum(2 * (p > q) + (p == q) for p in pos for q in neg))
            thr = sorted(pos, reverse=True)[place - 1]
            fps[-1].append(sum(q >= thr for q in neg))
            total, before = 0.0, 0
            for t in sorted(set(pos + neg), reverse=True):           # -0.0 and 0.0 are one member of the set: they are equal
                tp, fp = sum(p >= t for p in pos), sum(q >= t for q in neg)
                total += (tp - before) / m * (tp / (tp + fp))
                before = tp
            ap[-1].append(total)
    return u2, fps, ap, m, n0


def case(n, split, kind, seed, K=1):
    """labels int64 [n] and scores float32 [K, n].  split: "half", "one_pos", "one_neg", "mixed" (labels -1 and 2 among them);
    kind: "continuous", "four" (4 distinct values), "tied" (one value), "special" (+-inf, -0.0 and 0.0 among few values)"""
    rng = np.random.default_rng(seed)
    y = np.zeros(n, np.int64)
    if split == "half":
        y[rng.permutation(n)[:max(1, n // 2)]] = 1
    elif split == "one_pos":
        y[rng.integers(n)] = 1
    elif split == "one_neg":
        y[:] = 1
        y[rng.integers(n)] = 0
    elif split == "mixed":
        y = rng.choice(np.array([-1, 0, 1, 2]), size=n, p=[0.15, 0.4, 0.3, 0.15]).astype(np.int64)
        y[0], y[n - 1] = 1, 0
    else:
        raise ValueError(split)
    if kind == "continuous":
        s = rng.standard_normal((K, n)) + 0.8 * (y == 1)
    elif kind == "four":
        s = rng.integers(0, 4, (K, n)) * 0.25 + 0.25 * (rng.random((K, n)) < 0.3) * (y == 1)
    elif kind == "tied":
        s = np.full((K, n), 0.5)
    elif kind == "special":
        s = rng.choice(np.array([-math.inf, -1.0, -0.0, 0.0, 2.5, math.inf]), size=(K, n))
    else:
        raise ValueError(kind)
    return y, np.ascontiguousarray(s, dtype=np.float32)


def ap_bound(n):
    """|ap - ap'| for two float64 evaluations of the same AP: a sum of at most n non-negative terms that total at most 1, so either
    summation order is off by at most n 2^-53 plus a few roundings per term"""
    return 4 * n * 2.0 ** -53
