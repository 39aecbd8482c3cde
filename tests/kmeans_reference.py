"""The fp64 yardstick of the k-means tests: Lloyd's iterations as include/eagcn_hip.h states them, restated in numpy, and the common
data generator.  test_kmeans_cpu.py pins it against scikit-learn; test_gpu_kmeans.py holds the HIP kernels to it."""
import numpy as np


def make_data(seed, n, F, k):
    """(X [n, F] float32, init [k, F] float32 = k distinct rows of X, the true means, the true labels)"""
    rs = np.random.RandomState(seed)
    cen = rs.randn(k, F) * 3
    lab = rs.randint(0, k, n)
    lab[:k] = np.arange(k)
    X = (cen[lab] + rs.randn(n, F)).astype(np.float32)
    init = X[rs.choice(n, k, replace=False)]
    return X, init, cen, lab


def sqdist(X, C):
    """[n, k] float64: direct sums of squared differences"""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    return np.stack([((X - C[c]) ** 2).sum(axis=1) for c in range(C.shape[0])], axis=1)


def margins(d):
    """relative margin (d2 - d1) / (d2 + d1) of every row between its two nearest centres (inf for k = 1 or d1 = d2 = 0)"""
    if d.shape[1] < 2:
        return np.full(d.shape[0], np.inf)
    s = np.sort(d, axis=1)
    den = s[:, 1] + s[:, 0]
    return np.where(den > 0, (s[:, 1] - s[:, 0]) / np.where(den > 0, den, 1.0), np.inf)


def update(X, labels, C):
    """(new centres, counts): the mean of every cluster's rows; an empty cluster keeps its centre"""
    X = np.asarray(X, dtype=np.float64)
    Cn = np.array(C, dtype=np.float64)
    counts = np.bincount(labels, minlength=C.shape[0])
    for c in range(C.shape[0]):
        if counts[c]:
            Cn[c] = X[labels == c].mean(axis=0)
    return Cn, counts


def lloyd(X, C0, max_iter=300, tol=1e-4):
    """dict: centers, labels, inertia, n_iter, n_empty (of the final labels), counts, ever_empty, min_margin (over every iteration's
    assignment and the final one)"""
    X64 = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    tol_abs = tol * X64.var(axis=0).mean()
    prev, n_iter, ever_empty, min_margin = None, 0, False, np.inf
    for it in range(1, max_iter + 1):
        d = sqdist(X64, C)
        lab = d.argmin(axis=1)
        min_margin = min(min_margin, margins(d).min())
        Cn, counts = update(X64, lab, C)
        ever_empty = ever_empty or bool((counts == 0).any())
        shift = ((Cn - C) ** 2).sum()
        C, n_iter = Cn, it
        if prev is not None and np.array_equal(lab, prev):
            break
        prev = lab
        if shift <= tol_abs:
            break
    d = sqdist(X64, C)
    lab = d.argmin(axis=1)
    min_margin = min(min_margin, margins(d).min())
    counts = np.bincount(lab, minlength=C.shape[0])
    return dict(centers=C, labels=lab, inertia=d.min(axis=1).sum(), n_iter=n_iter, n_empty=int((counts == 0).sum()), counts=counts,
                ever_empty=ever_empty or bool((counts == 0).any()), min_margin=min_margin)


def find_seed(n, F, k, seeds=range(64), min_iter=3, margin=2e-4):
    """The first seed whose fit never empties a cluster, takes at least `min_iter` iterations and keeps every point's relative margin
    at or above `margin` in every iteration: (seed, X, init, fit), or None."""
    for seed in seeds:
        X, init, _, _ = make_data(seed, n, F, k)
        fit = lloyd(X, init)
        if not fit['ever_empty'] and fit['n_iter'] >= min_iter and fit['min_margin'] >= margin:
            return seed, X, init, fit
    return None
