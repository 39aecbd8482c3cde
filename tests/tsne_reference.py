"""The fp64 yardstick of the t-SNE and PCA tests: the semantics of include/eagcn_hip.h restated in plain numpy, the common data
generator and the seed searches.  test_tsne_cpu.py pins it against scikit-learn; test_gpu_tsne.py and test_gpu_pca.py hold the HIP
kernels of csrc/embed.hip to it."""
import numpy as np

EPS = np.finfo(np.float64).eps           # scikit-learn's MACHINE_EPSILON
PERP_TOL = 1e-5
EXPLORE = 250                            # iterations of the early-exaggeration stage
CHECK = 50                               # the stop rule is evaluated every CHECK-th iteration
STOP_MAX_ITER, STOP_NO_PROGRESS, STOP_GRAD_NORM = 1, 2, 3


def make_data(seed, n, F, blobs=5, outlier=False, duplicates=0):
    """X [n, F] float32: `blobs` Gaussian clusters; `outlier`: row 0 is moved far away from every other row (its row sum of
    exp(-D) underflows to zero at beta = 1); `duplicates`: the last rows repeat the first ones"""
    rs = np.random.RandomState(seed)
    cen = rs.randn(blobs, F) * 2.0
    lab = rs.randint(0, blobs, n)
    X = (cen[lab] + rs.randn(n, F)).astype(np.float32)
    if outlier:
        X[0] = X[0] + np.float32(40.0)
    for d in range(duplicates):
        X[n - 1 - d] = X[1 + d]
    return X


def sqdist(X):
    """[n, n] float64: direct sums of squared differences, accumulated column by column"""
    X = np.asarray(X, dtype=np.float64)
    D = np.zeros((X.shape[0], X.shape[0]))
    for f in range(X.shape[1]):
        d = X[:, f:f + 1] - X[None, :, f]
        d *= d
        D += d
    return D


def sqdist32(X):
    """the same rounded to float32: what the affinities are computed from"""
    return sqdist(X).astype(np.float32)


def conditional(D32, perplexity):
    """scikit-learn's _binary_search_perplexity in fp64 on fp32 distances.  dict: P (conditional, [n, n]), betas (of the last
    evaluation), steps (evaluations made), margin (per row the least distance of |H - log perplexity| from the tolerance over the
    last evaluation and the one before: the stopping step cannot move while fp64 noise stays below it), zero_rows (rows whose
    sum was zero at some evaluation: the 1e-8 branch)"""
    D = np.asarray(D32, dtype=np.float32).astype(np.float64)
    n = D.shape[0]
    off = ~np.eye(n, dtype=bool)
    target = np.log(perplexity)
    P = np.zeros((n, n))
    betas, steps, margin, zero = np.ones(n), np.zeros(n, dtype=np.int32), np.full(n, np.inf), np.zeros(n, dtype=bool)
    for i in range(n):
        d = D[i][off[i]]
        beta, bmin, bmax, prev = 1.0, -np.inf, np.inf, np.inf
        for step in range(100):
            p = np.exp(-d * beta)
            s = p.sum()
            if s == 0.0:
                s = 1e-8
                zero[i] = True
            p = p / s
            H = np.log(s) + beta * (d * p).sum()
            diff = H - target
            gap = abs(abs(diff) - PERP_TOL)
            used = beta
            if abs(diff) <= PERP_TOL:
                break
            prev = gap
            if diff > 0.0:
                bmin = beta
                beta = beta * 2.0 if bmax == np.inf else (beta + bmax) / 2.0
            else:
                bmax = beta
                beta = beta / 2.0 if bmin == -np.inf else (beta + bmin) / 2.0
        P[i][off[i]] = p
        betas[i], steps[i], margin[i] = used, step + 1, min(gap, prev)
    return dict(P=P, betas=betas, steps=steps, margin=margin, zero_rows=zero)


def joint(Pc):
    """scikit-learn's _joint_probabilities as a full matrix: max((C + C^T) / sum, eps) off the diagonal, 0 on it"""
    P = Pc + Pc.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def objective(P, Y, alpha=1.0, dtype=np.float64):
    """dict: grad [n, 2], kl (scikit-learn's, Q clamped at eps), kl_free (the header's form, Q not clamped), Z, bound [n, 2] =
    4 sum_j (|alpha P| + |Q|) w |y_i - y_j| per component, all computed in `dtype`"""
    Y = np.asarray(Y, dtype=dtype)
    aP = (np.asarray(P, dtype=dtype) * dtype(alpha)).astype(dtype)
    n = Y.shape[0]
    off = ~np.eye(n, dtype=bool)
    dx, dy = Y[:, 0:1] - Y[None, :, 0], Y[:, 1:2] - Y[None, :, 1]
    w = (1.0 / (1.0 + (dx * dx + dy * dy))).astype(dtype)
    np.fill_diagonal(w, 0.0)
    Z = w.sum(dtype=np.float64)
    Q = np.maximum(w / dtype(Z), dtype(EPS))
    np.fill_diagonal(Q, 0.0)
    t, tb = (aP - Q) * w, (np.abs(aP) + np.abs(Q)) * w
    grad = 4.0 * np.stack([(t * dx).sum(1), (t * dy).sum(1)], axis=1)
    bound = 4.0 * np.stack([(tb * np.abs(dx)).sum(1), (tb * np.abs(dy)).sum(1)], axis=1)
    del t, tb, dx, dy
    p64, q64, w64 = aP[off].astype(np.float64), Q[off].astype(np.float64), w[off].astype(np.float64)
    kl = float((p64 * np.log(np.maximum(p64, EPS) / q64)).sum())
    kl_free = float((p64 * np.log(np.maximum(p64, EPS))).sum() - (p64 * np.log(w64)).sum() + np.log(Z) * p64.sum())
    return dict(grad=grad.astype(dtype), kl=kl, kl_free=kl_free, Z=float(Z), bound=bound.astype(np.float64))


def update(Y, U, G, grad, momentum, lr, dtype=np.float64):
    """scikit-learn's _gradient_descent step, element-wise in `dtype`: (Y, update, gains, gained gradient)"""
    grad, U, G, Y = (np.asarray(a, dtype=dtype) for a in (grad, U, G, Y))
    inc = U * grad < 0.0
    G = np.where(inc, G + dtype(0.2), G * dtype(0.8)).astype(dtype)
    G = np.maximum(G, dtype(0.01))
    gg = (grad * G).astype(dtype)
    U = (dtype(momentum) * U - dtype(lr) * gg).astype(dtype)
    return (Y + U).astype(dtype), U, G, gg


def descend(P, Y0, lr, early_exaggeration=12.0, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64,
            record=()):
    """The driver of include/eagcn_hip.h.  dict: Y, n_iter (iterations made), reason, kl (of the final embedding against P), checks
    [(iteration, kl, |gained grad|)], trajectory {it: (Y, update, gains) BEFORE iteration it, it in record}"""
    Y = np.array(Y0, dtype=dtype)
    U, G = np.zeros_like(Y), np.ones_like(Y)
    best, best_it, reason, checks, traj = np.finfo(np.float64).max, 0, 0, [], {}
    it = 0
    while it < max_iter:
        early = it < EXPLORE
        if it == EXPLORE:
            U, G, best, best_it = np.zeros_like(Y), np.ones_like(Y), np.finfo(np.float64).max, it
        if it in record:
            traj[it] = (Y.copy(), U.copy(), G.copy())
        ob = objective(P, Y, early_exaggeration if early else 1.0, dtype)
        Y, U, G, gg = update(Y, U, G, ob['grad'], 0.5 if early else 0.8, lr, dtype)
        if (it + 1) % CHECK == 0:
            gn = float(np.sqrt((gg.astype(np.float64) ** 2).sum()))
            checks.append((it, ob['kl'], gn))
            if ob['kl'] < best:
                best, best_it = ob['kl'], it
            elif it - best_it > (EXPLORE if early else n_iter_without_progress):
                reason = STOP_NO_PROGRESS
            if not reason and gn <= min_grad_norm:
                reason = STOP_GRAD_NORM
        it += 1
        if reason:
            break
    if not reason:
        reason = STOP_MAX_ITER
    for r in record:
        if r == it:
            traj[it] = (Y.copy(), U.copy(), G.copy())
    return dict(Y=Y, n_iter=it, reason=reason, kl=objective(P, Y, 1.0, np.float64)['kl'], checks=checks, trajectory=traj)


def affinities(X, perplexity):
    """(D32, conditional dict, joint P) of the rows X"""
    D = sqdist32(X)
    c = conditional(D, perplexity)
    return D, c, joint(c['P'])


def find_seed(n, F, perplexity, seeds=range(16), margin=1e-10, **kw):
    """The first seed whose every row keeps |H - log perplexity| at least `margin` away from the tolerance at the stopping step and
    at the step before it: (seed, X, D32, conditional dict, joint P), or None."""
    for seed in seeds:
        X = make_data(seed, n, F, **kw)
        D, c, P = affinities(X, perplexity)
        if c['margin'].min() >= margin:
            return seed, X, D, c, P
    return None


# ---- PCA ---------------------------------------------------------------------------------------------------------------------------

def make_pca_data(seed, n, F, k=8):
    """X [n, F] float32 = U diag(s) V^T + a mean, U orthonormal and orthogonal to the constant vector: the covariance has the
    eigenvalues s^2 / (n - 1) BY CONSTRUCTION -- 25 (1 - 0.11 m) for the first eight, 0.1 after: relative gaps of 0.11 and more"""
    rs = np.random.RandomState(seed)
    r = min(F, n - 1)
    U = np.linalg.qr(np.concatenate([np.ones((n, 1)), rs.randn(n, r)], axis=1))[0][:, 1:]
    V = np.linalg.qr(rs.randn(F, F))[0][:, :r]
    var = np.array([25.0 * (1.0 - 0.11 * m) if m < 8 else 0.1 for m in range(r)])
    return ((U * np.sqrt(var * (n - 1))) @ V.T + rs.randn(F) * 3.0).astype(np.float32)


def pca(X, k):
    """dict: mean, cov, components [k, F] (entry of largest magnitude positive), variance [k], embedding [n, k], gaps =
    (lambda_m - lambda_{m+1}) / lambda_1 for m <= k -- all fp64"""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    cov = Xc.T @ Xc / (X.shape[0] - 1)
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1]
    comp = vec[:, :k].T.copy()
    big = np.abs(comp).argmax(axis=1)
    comp *= np.sign(comp[np.arange(comp.shape[0]), big])[:, None]
    nxt = np.append(lam, 0.0)
    gaps = (lam[:k] - nxt[1:k + 1]) / lam[0]
    return dict(mean=mean, cov=cov, components=comp, variance=lam[:k].copy(), embedding=Xc @ comp.T, gaps=gaps)


def find_pca_seed(n, F, k, seeds=range(16), gap=0.1):
    """The first seed whose relative eigengaps are all at least `gap`: (seed, X, pca dict), or None."""
    for seed in seeds:
        X = make_pca_data(seed, n, F, k)
        fit = pca(X, k)
        if fit['gaps'].min() >= gap:
            return seed, X, fit
    return None
