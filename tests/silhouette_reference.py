"""The fp64 yardstick of the clustering-score tests, in numpy: silhouette samples from a distance matrix by the formulae of
include/eagcn_hip.h, the cluster moments, the Davies-Bouldin and Calinski-Harabasz indices from them, and the adjusted Rand index,
normalised mutual information and purity of a contingency matrix.  test_silhouette_cpu.py pins it against scikit-learn;
test_gpu_silhouette.py holds the HIP kernels (csrc/silhouette.hip) and eagcn_amd.analysis to it.  Data generators, fp64 distances and the
error margin of the fp32 distances are those of knn_reference."""
import numpy as np

from knn_reference import clusters, gaussian, margin, sqdist64  # noqa: F401


def silhouette_from_distances(D, labels, k):
    """(samples [n] (NaN for a row whose label is outside 0 .. k - 1), counts [k]) from the distance matrix D [n, n] (distances, not
    squares): S[i, c] = the sum of D[i, j] over the rows j of cluster c; a = S[i, own] / (cnt[own] - 1), b = the least S[i, c] / cnt[c]
    over the other non-empty clusters, s = (b - a) / max(a, b); 0 for a row alone in its cluster and where the quotient is no number."""
    D = np.asarray(D, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    n = D.shape[0]
    inside = (labels >= 0) & (labels < k)
    onehot = np.zeros((n, k))
    onehot[np.nonzero(inside)[0], labels[inside]] = 1.0
    counts = onehot.sum(axis=0).astype(np.int64)
    S = D @ onehot
    out = np.full(n, np.nan)
    rows = np.nonzero(inside)[0]
    own = labels[rows]
    cnt_own = counts[own]
    with np.errstate(divide='ignore', invalid='ignore'):
        a = S[rows, own] / (cnt_own - 1)
        mean = S[rows] / counts[None, :]
        mean[:, counts == 0] = np.inf
        mean[np.arange(rows.size), own] = np.inf
        b = mean.min(axis=1)
        s = (b - a) / np.maximum(a, b)
    s[cnt_own == 1] = 0.0
    out[rows] = np.nan_to_num(s, nan=0.0)
    return out, counts


def silhouette_samples(X, labels, k):
    """the same from the rows: D = the square root of knn_reference.sqdist64 (direct differences, column by column)"""
    return silhouette_from_distances(np.sqrt(sqdist64(X, X)), labels, k)


def summary(samples, labels, k):
    """(score, cluster_means [k], n_ignored) of given samples: the mean over the scored rows (NaN with fewer than two non-empty
    clusters), the mean of every cluster (NaN for an empty one), the number of rows outside 0 .. k - 1"""
    samples = np.asarray(samples, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    inside = (labels >= 0) & (labels < k)
    means = np.array([samples[labels == c].mean() if np.any(labels == c) else np.nan for c in range(k)])
    score = samples[inside].mean() if np.sum(~np.isnan(means)) >= 2 else np.nan
    return score, means, int((~inside).sum())


def moments(X, labels, k):
    """(centers [k, F], scatter [k], wss [k], counts [k]) in fp64: the centroid of every cluster, the mean distance of its rows to it,
    the sum of their squared distances; NaN centres and scatter for an empty cluster"""
    X = np.asarray(X, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    centers, scatter, wss = np.full((k, X.shape[1]), np.nan), np.full(k, np.nan), np.zeros(k)
    counts = np.zeros(k, dtype=np.int64)
    for c in range(k):
        rows = X[labels == c]
        counts[c] = len(rows)
        if len(rows):
            centers[c] = rows.mean(axis=0)
            d2 = ((rows - centers[c]) ** 2).sum(axis=1)
            scatter[c], wss[c] = np.sqrt(d2).mean(), d2.sum()
    return centers, scatter, wss, counts


def davies_bouldin(centers, scatter, counts):
    """sklearn.metrics.davies_bouldin_score over the non-empty clusters"""
    there = counts > 0
    cen, s = centers[there], scatter[there]
    d = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(s, 0) or np.allclose(d, 0):
        return 0.0
    d[d == 0] = np.inf
    return float(np.mean(np.max((s[:, None] + s[None, :]) / d, axis=1)))


def calinski_harabasz(centers, wss, counts):
    """sklearn.metrics.calinski_harabasz_score over the non-empty clusters"""
    there = counts > 0
    cen, cnt = centers[there], counts[there].astype(np.float64)
    n, k = cnt.sum(), float(there.sum())
    mean = (cen * cnt[:, None]).sum(axis=0) / n
    extra, intra = (cnt * ((cen - mean) ** 2).sum(axis=1)).sum(), wss[there].sum()
    return 1.0 if intra == 0.0 else float(extra * (n - k) / (intra * (k - 1.0)))


def contingency(y_true, labels, n_true, k):
    """[n_true, k] int64: entry (t, c) counts the rows of class t in cluster c"""
    cm = np.zeros((n_true, k), dtype=np.int64)
    np.add.at(cm, (np.asarray(y_true, dtype=np.int64), np.asarray(labels, dtype=np.int64)), 1)
    return cm


def adjusted_rand(cm):
    """sklearn.metrics.adjusted_rand_score from the contingency matrix: the pair counts as Python integers"""
    cm = [[int(v) for v in row] for row in np.asarray(cm)]
    n = sum(map(sum, cm))
    sq = sum(v * v for row in cm for v in row)
    rows, cols = [sum(r) for r in cm], [sum(c) for c in zip(*cm)]
    tp = sq - n
    fp = sum(v * cols[j] for row in cm for j, v in enumerate(row)) - sq
    fn = sum(v * rows[i] for i, row in enumerate(cm) for v in row) - sq
    tn = n * n - fp - fn - sq
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def normalized_mutual_info(cm):
    """sklearn.metrics.normalized_mutual_info_score(average_method='arithmetic') from the contingency matrix; empty rows and columns
    do not count"""
    c = np.asarray(cm, dtype=np.float64)
    c = c[c.sum(axis=1) > 0][:, c.sum(axis=0) > 0]
    if c.shape[0] == c.shape[1] and c.shape[0] <= 1:
        return 1.0
    if c.shape[0] == 1 or c.shape[1] == 1:
        return 0.0
    n, pi, pj = c.sum(), c.sum(axis=1), c.sum(axis=0)
    i, j = np.nonzero(c)
    v = c[i, j]
    mi = (v / n) * (np.log(v) - np.log(n)) + (v / n) * (-np.log(pi[i] * pj[j]) + 2.0 * np.log(n))
    mi = max(np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi).sum(), 0.0)
    if mi == 0:
        return 0.0
    h = [-np.sum((p / n) * (np.log(p) - np.log(n))) for p in (pi, pj)]
    return float(mi / (0.5 * (h[0] + h[1])))


def purity(cm):
    """the share of the rows that carry the most frequent class of their cluster"""
    cm = np.asarray(cm)
    return float(cm.max(axis=0).sum() / cm.sum())


def remap9(lab, n):
    """The six clusters of knn_reference.clusters as a labelling with k = 9: cluster 6 stays empty, row n - 1 is alone in cluster 7 and
    rows of cluster 0 with an odd index move to cluster 8."""
    lab = np.asarray(lab, dtype=np.int64).copy()
    lab[(lab == 0) & (np.arange(n) % 2 == 1)] = 8
    lab[n - 1] = 7
    return lab


def tile_edge_labels(n):
    """k = 9 labels for n >= 600 rows with clusters of exactly 1 (7), 64 (1), 65 (2) and 128 (3) rows, cluster 6 empty, the rest spread
    over 0, 4, 5 and 8 in turn -- rows interleaved, so that the cluster order is a real permutation"""
    assert n >= 600
    lab = np.empty(n, dtype=np.int64)
    rest = np.array([0, 4, 5, 8])
    lab[:] = rest[np.arange(n) % 4]
    pick = np.random.RandomState(n).permutation(n)
    lab[pick[:64]] = 1
    lab[pick[64:129]] = 2
    lab[pick[129:257]] = 3
    lab[pick[257]] = 7
    return lab
