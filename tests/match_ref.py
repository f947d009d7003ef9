"""The canonical matcher of include/saccot.h (sc_match), restated in numpy float32: the reference of tests/test_gpu_match.py.
No fused multiply-add anywhere, so plain float32 array arithmetic IS the definition, exact without compiling anything."""
import numpy as np


def distances(a, b):
    """acc = 0; for c ascending: d = a[c] - b[c]; acc = acc + d * d — every operation rounded to fp32.  (ns, nt) float32."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    with np.errstate(over="ignore", under="ignore"):
        for c in range(a.shape[1]):
            d = a[:, c][:, None] - b[:, c][None, :]
            acc = acc + d * d
    assert acc.dtype == np.float32
    return acc


def ranked(acc):
    """-> (order, back): row i's target indices by ascending key (bits(acc) << 32) | j, and every target row's minimum source
    row under the reverse key (bits(acc) << 32) | i.  Keys are distinct, so the sort's stability is not even needed."""
    ns, nt = acc.shape
    hi = acc.view(np.uint32).astype(np.uint64) << np.uint64(32)
    order = np.argsort(hi | np.arange(nt, dtype=np.uint64)[None, :], axis=1, kind="stable")
    back = np.argmin(hi | np.arange(ns, dtype=np.uint64)[:, None], axis=0)
    return order, back


def select(acc, order, back, knn=1, mutual=False, ratio=0.0):
    """-> (corr (n, 2) int32, d2 (n,) float32) in ascending (source row, rank) order."""
    ns, nt = acc.shape
    keep = np.ones((ns, min(knn, nt)), bool)
    if mutual or ratio > 0:
        assert knn == 1
        rows, j = np.arange(ns), order[:, 0]
        if mutual:
            keep[:, 0] &= back[j] == rows
        if ratio > 0 and nt > 1:
            r = np.float32(ratio)
            r2 = np.float32(np.float64(r) * np.float64(r))
            with np.errstate(over="ignore", under="ignore", invalid="ignore"):
                keep[:, 0] &= acc[rows, j] < r2 * acc[rows, order[:, 1]]
    i_idx, rank = np.nonzero(keep)
    j_idx = order[i_idx, rank]
    return np.stack([i_idx, j_idx], axis=1).astype(np.int32).reshape(-1, 2), acc[i_idx, j_idx].astype(np.float32)


def match(a, b, knn=1, mutual=False, ratio=0.0):
    acc = distances(a, b)
    return select(acc, *ranked(acc), knn=knn, mutual=mutual, ratio=ratio)
