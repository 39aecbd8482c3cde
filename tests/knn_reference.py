"""The fp64 yardstick of the nearest-neighbour tests, in numpy: brute-force neighbours and ranks under the order of
include/eagcn_hip.h -- (distance, row index) ascending --, the trustworthiness of an embedding, the data generators and the error
margin of the fp32 distances.  test_knn_cpu.py pins it against scikit-learn; test_gpu_knn.py holds the HIP kernels (csrc/knn.hip) to it.
"""
import numpy as np


def margin(F):
    """Relative error bound of an fp32 F-term sum of squared fp32 differences, one fmaf accumulator in column order: the difference is
    rounded once (2^-24), its square and every one of the F additions once more -- (F + 2) 2^-24 to first order; (F + 4) 2^-23 is
    twice that and more."""
    return (F + 4) * 2.0 ** -23


def gaussian(seed, n, F):
    """[n, F] float32, standard normal"""
    return np.random.RandomState(seed).randn(n, F).astype(np.float32)


def clusters(seed, n, F, n_dup=5):
    """(X [n, F] float32, labels [n]): six Gaussian clusters; `n_dup` rows are exact copies of other rows (rows 0 .. n_dup - 1 are
    copied to random places beyond them, so that a row and its duplicate are far apart by index)"""
    rs = np.random.RandomState(seed)
    cen = rs.randn(6, F) * 3
    lab = rs.randint(0, 6, n)
    X = (cen[lab] + rs.randn(n, F)).astype(np.float32)
    n_dup = min(n_dup, n // 3)
    if n_dup:
        dst = n_dup + rs.choice(n - n_dup, n_dup, replace=False)
        X[dst] = X[:n_dup]
        lab[dst] = lab[:n_dup]
    return X, lab


def sqdist64(Q, X, gram=False):
    """[m, n] float64 squared distances between the rows of Q and of X.  Direct sums of squared differences, column by column; with
    gram=True  |q|^2 + |x|^2 - 2 q.x  in fp64 (clamped at 0), whose cancellation error is a few 2^-53 (|q|^2 + |x|^2): for data WITHOUT
    near-duplicate rows, where it is eleven orders below margin(F) d and a large block takes a matrix product instead of F passes."""
    Q = np.asarray(Q, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    if gram:
        D = (Q * Q).sum(axis=1)[:, None] + (X * X).sum(axis=1)[None, :] - 2.0 * (Q @ X.T)
        return np.maximum(D, 0.0)
    D = np.zeros((Q.shape[0], X.shape[0]))
    Xt = np.ascontiguousarray(X.T)
    for c in range(Q.shape[1]):
        t = Q[:, c, None] - Xt[c][None, :]
        t *= t
        D += t
    return D


def order(D, exclude_self=False):
    """[m, n (- 1)] int64: every row's candidates sorted by (D, index); exclude_self drops candidate j == i by index"""
    o = np.argsort(D, axis=1, kind='stable')                  # (stable: equal distances keep their index order; NaN sorts last)
    if exclude_self:
        m = D.shape[0]
        o = o[o != np.arange(m)[:, None]].reshape(m, D.shape[1] - 1)
    return o


def neighbours(D, k, exclude_self=False):
    """(indices [m, k], distances [m, k]) of the k first candidates of every row of the distance block D"""
    idx = order(D, exclude_self)[:, :k]
    return idx, np.take_along_axis(D, idx, axis=1)


def ranks(D, cand):
    """int64 [n, k]: rank[i, c] = 1 + #{l != i : (D[i, l], l) < (D[i, j], j)}, j = cand[i, c]; -1 where j == i or j is no row"""
    n = D.shape[0]
    o = order(D, exclude_self=True)
    pos = np.zeros((n, n), dtype=np.int64)
    np.put_along_axis(pos, o, np.arange(1, n)[None, :].repeat(n, axis=0), axis=1)
    cand = np.asarray(cand, dtype=np.int64)
    bad = (cand < 0) | (cand >= n) | (cand == np.arange(n)[:, None])
    r = np.take_along_axis(pos, np.where(bad, 0, cand), axis=1)
    return np.where(bad, -1, r)


def near_counts(D, cand, rel):
    """int64 [n, k]: e[i, c] = #{l != i, l != j : |D[i, l] - D[i, j]| <= rel D[i, j]}, j = cand[i, c] (a valid candidate): the rows whose
    order against j an error of `rel` in the distances can change -- the most a rank computed from such distances can be off"""
    n = D.shape[0]
    cand = np.asarray(cand, dtype=np.int64)
    out = np.zeros(cand.shape, dtype=np.int64)
    rows = np.arange(n)
    for c in range(cand.shape[1]):
        dj = D[rows, cand[:, c]]
        near = np.abs(D - dj[:, None]) <= rel * dj[:, None]
        near[rows, rows] = False
        near[rows, cand[:, c]] = False
        out[:, c] = near.sum(axis=1)
    return out


def trustworthiness(DX, DY, k):
    """sklearn.manifold.trustworthiness from the two squared-distance matrices: the k neighbours of every row in Y, their ranks in X,
    T = 1 - 2 / (n k (2 n - 3 k - 1)) sum max(0, rank - k).  (T, neighbours in Y [n, k], their ranks in X [n, k])"""
    n = DX.shape[0]
    nb, _ = neighbours(DY, k, exclude_self=True)
    r = ranks(DX, nb)
    t = np.maximum(r - k, 0).sum()
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))), nb, r


def pca2(X):
    """[n, 2] float32: the fp64 projection of the centred rows on their two leading principal axes"""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    Y = np.zeros((X.shape[0], 2))
    Y[:, :min(2, vt.shape[0])] = Xc @ vt[:2].T
    return Y.astype(np.float32)


def least_gap(D, upto, exclude_self=True):
    """The least relative gap (d[p + 1] - d[p]) / d[p + 1] between consecutive ones of every row's first `upto` sorted distances"""
    o = order(D, exclude_self)[:, :upto]
    s = np.take_along_axis(D, o, axis=1)
    hi = s[:, 1:]
    return float(np.min(np.where(hi > 0, (hi - s[:, :-1]) / np.where(hi > 0, hi, 1.0), 0.0)))


def find_seed(n, F, k, seeds=range(64)):
    """The first seed whose cluster data (no duplicates) has, in its fp32 two-column PCA, no relative gap of 2 margin(2) or less among
    the first k + 1 neighbours of any row -- the fp32 distances then order those neighbours as fp64 does:
    (seed, X, Y, DX, DY) with the fp64 distance matrices, or None."""
    for seed in seeds:
        X, _ = clusters(seed, n, F, n_dup=0)
        Y = pca2(X)
        DY = sqdist64(Y, Y)
        if least_gap(DY, k + 1) > 2 * margin(2):
            return seed, X, Y, sqdist64(X, X), DY
    return None
