"""CPU-only checks of the clustering scores (csrc/silhouette.hip, eagcn_amd.analysis): the symbols are exported and bound, the workspace
sizes are the header's formulae, every argument outside the envelope comes back as a message before any HIP call, host tensors are
refused, and the numpy yardstick of the GPU tests (silhouette_reference) is scikit-learn's."""
import numpy as np
import pytest

import silhouette_reference as R

NEW = ('eagcn_silhouette_workspace_bytes', 'eagcn_silhouette', 'eagcn_cluster_moments_workspace_bytes', 'eagcn_cluster_moments')
SHAPES = [(17, 1), (65, 3), (129, 33), (257, 7), (515, 32), (300, 700), (1027, 24)]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from eagcn_amd import _lib
    return _lib.load()


def _msg(lib):
    return lib.eagcn_last_error().decode()


def test_symbols_exported_bound_and_abi_unchanged(lib):
    from eagcn_amd import _lib, analysis
    import eagcn_amd
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.eagcn_abi_version() == _lib.ABI_VERSION == 8
    for name in ('silhouette_samples', 'silhouette_score', 'SilhouetteResult', 'cluster_moments', 'ClusterMoments', 'davies_bouldin_score',
                 'calinski_harabasz_score', 'adjusted_rand_score', 'normalized_mutual_info_score', 'purity'):
        assert getattr(eagcn_amd, name) is getattr(analysis, name) and name in eagcn_amd.__all__
    assert analysis.SIL_MAX_K == 256
    assert analysis.SilhouetteResult._fields == ('samples', 'score', 'cluster_means', 'counts', 'n_ignored')
    assert analysis.ClusterMoments._fields == ('centers', 'scatter', 'wss', 'counts')


def test_workspace_bytes_are_the_header_formulae(lib):
    from eagcn_amd import analysis
    for n in (1, 17, 63, 64, 65, 1023, 1024, 1025, 8209, 100000, 1048577, 2 ** 31 - 1):
        for F, k in ((1, 2), (700, 18), (1024, 256), (24, 9)):
            assert lib.eagcn_cluster_moments_workspace_bytes(n, F, k) == analysis.cluster_moments_workspace_bytes(n, F, k) > 0, (n, F, k)
            for slabs in (0, 1, 2, 3, 7, 64, 5000):
                got = lib.eagcn_silhouette_workspace_bytes(n, F, k, slabs)
                assert got == analysis.silhouette_workspace_bytes(n, F, k, slabs) > 0, (n, F, k, slabs)
    # the slab rule of knn on the tile bound ceil(n / 64) + k
    assert [analysis.silhouette_slabs(8209, 18, s) for s in (1, 2, 3, 7, 0)] == [1, 2, 3, 7, 30]
    assert analysis.silhouette_slabs(100000, 18) == 3 and analysis.silhouette_slabs(17, 2, 5000) == 3 and analysis.silhouette_slabs(17, 2) == 3
    n, k = 100000, 18
    part = 8 * 3 * n * k
    assert analysis.silhouette_workspace_bytes(n, 700, k) - (part + 255) // 256 * 256 < 1 << 20          # (the rest is small)
    for n, F, k, slabs in ((0, 4, 2, 0), (2 ** 31, 4, 2, 0), (10, 0, 2, 0), (10, 1025, 2, 0), (10, 4, 1, 0), (10, 4, 257, 0), (10, 4, 2, -1)):
        assert lib.eagcn_silhouette_workspace_bytes(n, F, k, slabs) == 0, (n, F, k, slabs)
        if slabs >= 0:
            assert lib.eagcn_cluster_moments_workspace_bytes(n, F, k) == 0, (n, F, k)


def test_arguments_outside_the_envelope_are_refused_without_a_gpu(lib):
    P, WS, BIG = 4096, 8192, 1 << 50                        # non-null addresses that are never dereferenced: every check comes first
    ok = dict(X=P, n=100, F=8, ld=8, labels=P, k=3, slabs=0, samples=P, means=P, counts=P, stats=P, ws=WS, nbytes=BIG)

    def sil(**kw):
        a = dict(ok, **kw)
        return lib.eagcn_silhouette(a['X'], a['n'], a['F'], a['ld'], a['labels'], a['k'], a['slabs'], a['samples'], a['means'], a['counts'],
                                    a['stats'], a['ws'], a['nbytes'], None)

    need = lib.eagcn_silhouette_workspace_bytes(100, 8, 3, 0)
    assert need > 0
    cases = [(dict(k=1), 'k = 1 is not in 2 .. 256'), (dict(k=257), 'k = 257 is not in 2 .. 256'), (dict(k=0), 'k = 0 is not in 2 .. 256'),
             (dict(F=1025, ld=1025), 'F = 1025 is not in 1 .. 1024'), (dict(F=0), 'F = 0 is not in 1 .. 1024'),
             (dict(ld=7), 'row stride 7 of X is smaller than F = 8'), (dict(X=None), 'X is null'), (dict(X=4098), 'X must be 4-byte aligned'),
             (dict(n=0), 'rows of X are not in'), (dict(n=2 ** 31), 'rows of X are not in'), (dict(labels=None), 'labels is null'),
             (dict(slabs=-1), 'slabs = -1 is negative'), (dict(samples=None), 'samples is null'), (dict(means=None), 'cluster_mean is null'),
             (dict(counts=None), 'counts is null'), (dict(stats=None), 'stats is null'), (dict(ws=None), 'workspace is null'),
             (dict(ws=WS + 16), 'workspace must be 256-byte aligned'),
             (dict(nbytes=need - 1), 'workspace too small (%d < %d bytes)' % (need - 1, need))]
    for kw, text in cases:
        assert sil(**kw) == -1, kw
        assert 'eagcn_silhouette: ' in _msg(lib) and text in _msg(lib), (kw, _msg(lib))

    okm = dict(X=P, n=100, F=8, ld=8, labels=P, k=3, centers=P, scatter=P, wss=P, counts=P, ws=WS, nbytes=BIG)

    def mom(**kw):
        a = dict(okm, **kw)
        return lib.eagcn_cluster_moments(a['X'], a['n'], a['F'], a['ld'], a['labels'], a['k'], a['centers'], a['scatter'], a['wss'], a['counts'],
                                         a['ws'], a['nbytes'], None)

    need = lib.eagcn_cluster_moments_workspace_bytes(100, 8, 3)
    assert need > 0
    cases = [(dict(k=1), 'k = 1 is not in 2 .. 256'), (dict(k=257), 'k = 257 is not in 2 .. 256'), (dict(F=1025, ld=1025), 'F = 1025 is not in'),
             (dict(F=0), 'F = 0 is not in'), (dict(ld=7), 'row stride 7 of X is smaller than F = 8'), (dict(X=None), 'X is null'),
             (dict(X=4098), 'X must be 4-byte aligned'), (dict(n=0), 'rows of X are not in'), (dict(n=2 ** 31), 'rows of X are not in'),
             (dict(labels=None), 'labels is null'), (dict(centers=None), 'centers is null'), (dict(scatter=None), 'scatter is null'),
             (dict(wss=None), 'wss is null'), (dict(counts=None), 'counts is null'), (dict(ws=None), 'workspace is null'),
             (dict(ws=WS + 16), 'workspace must be 256-byte aligned'),
             (dict(nbytes=need - 1), 'workspace too small (%d < %d bytes)' % (need - 1, need))]
    for kw, text in cases:
        assert mom(**kw) == -1, kw
        assert 'eagcn_cluster_moments: ' in _msg(lib) and text in _msg(lib), (kw, _msg(lib))


def test_python_refuses_host_tensors():
    import torch
    from eagcn_amd import analysis
    from eagcn_amd._lib import EagcnHipError
    X, lab = torch.zeros(20, 4), torch.zeros(20, dtype=torch.int64)
    for fn in (analysis.silhouette_samples, analysis.silhouette_score, analysis.cluster_moments, analysis.davies_bouldin_score,
               analysis.calinski_harabasz_score):
        with pytest.raises(EagcnHipError, match='no CPU path'):
            fn(X, lab, 3)
    for fn in (analysis.adjusted_rand_score, analysis.normalized_mutual_info_score, analysis.purity):
        with pytest.raises(ValueError, match='confusion_matrix'):
            fn(torch.zeros(3, 3))
        with pytest.raises(ValueError, match='confusion_matrix'):
            fn(torch.zeros(9, dtype=torch.int64))


def _case(n, F):
    """cluster data with duplicates under k = 9 labels: cluster 6 empty, cluster 7 a single row"""
    X, lab = R.clusters(n * 1000 + F, n, F, n_dup=5)
    return X, R.remap9(lab, n)


@pytest.mark.parametrize('n,F', SHAPES)
def test_yardstick_is_sklearn(n, F):
    from sklearn import metrics
    X, lab = _case(n, F)
    k = 9
    counts = np.bincount(lab, minlength=k)
    assert counts[6] == 0 and counts[7] == 1 and (counts > 1).sum() >= 4
    X64 = X.astype(np.float64)
    s, cnt = R.silhouette_samples(X, lab, k)
    want = metrics.silhouette_samples(X64, lab, metric='euclidean')
    print('n=%d F=%d: worst |sample - sklearn| = %.3e' % (n, F, np.abs(s - want).max()))
    assert np.array_equal(cnt, counts) and s[n - 1] == 0.0 == want[n - 1]          # the single row of cluster 7
    assert np.abs(s - want).max() <= 1e-8
    score, means, ignored = R.summary(s, lab, k)
    assert ignored == 0 and np.isnan(means[6]) and means[7] == 0.0
    assert abs(score - metrics.silhouette_score(X64, lab, metric='euclidean')) <= 1e-8
    cen, sc, wss, cnt = R.moments(X, lab, k)
    assert np.array_equal(cnt, counts) and np.isnan(cen[6]).all() and np.isnan(sc[6]) and sc[7] == 0.0 == wss[7]
    db, ch = R.davies_bouldin(cen, sc, cnt), R.calinski_harabasz(cen, wss, cnt)
    assert abs(db - metrics.davies_bouldin_score(X64, lab)) <= 1e-10 * max(1.0, db)
    assert abs(ch - metrics.calinski_harabasz_score(X64, lab)) <= 1e-10 * max(1.0, ch)
    _, true = R.clusters(n * 1000 + F, n, F, n_dup=5)
    cm = R.contingency(true, lab, 6, k)
    assert cm.sum() == n and np.array_equal(cm.sum(axis=0), counts)
    assert abs(R.adjusted_rand(cm) - metrics.adjusted_rand_score(true, lab)) <= 1e-10
    assert abs(R.normalized_mutual_info(cm) - metrics.normalized_mutual_info_score(true, lab)) <= 1e-10
    assert abs(R.purity(cm) - sum(np.bincount(true[lab == c]).max() for c in range(k) if counts[c]) / n) <= 1e-15


def test_yardstick_leaves_rows_outside_the_labelling_out():
    n, F, k = 129, 5, 9
    X, lab = _case(n, F)
    out = lab.copy()
    out[3::7] = -1
    out[5::11] = k
    keep = (out >= 0) & (out < k)
    s, cnt = R.silhouette_samples(X, out, k)
    s_kept, cnt_kept = R.silhouette_samples(X[keep], out[keep], k)
    assert np.isnan(s[~keep]).all() and np.array_equal(cnt, cnt_kept)
    assert np.abs(s[keep] - s_kept).max() <= 1e-13             # (the matrix product sums in another order over the shorter rows)
    assert R.summary(s, out, k)[2] == int((~keep).sum())
    for got, want in zip(R.moments(X, out, k), R.moments(X[keep], out[keep], k)):
        assert np.array_equal(got, want, equal_nan=True)
    one = np.where(lab == 1, 1, -1)                          # a single cluster: no score
    s, _ = R.silhouette_samples(X, one, k)
    assert np.isnan(R.summary(s, one, k)[0])


MATRICES = [[[5, 0, 2], [1, 7, 0], [0, 3, 9]], [[4, 0, 0, 3], [0, 0, 0, 0], [2, 0, 6, 1]], [[3, 0], [0, 4]], [[2, 5]], [[7]], [[3], [4]],
            [[1, 1], [1, 1]], [[100000, 3], [7, 250000]]]


@pytest.mark.parametrize('cm', MATRICES)
def test_agreement_scores_on_cpu_tensors_are_sklearn(cm):
    """adjusted_rand_score, normalized_mutual_info_score and purity are plain torch: on host matrices, against scikit-learn on labels
    that have this contingency matrix -- among them one with an empty row and an empty column"""
    import torch
    from sklearn import metrics
    from eagcn_amd import analysis
    cm = np.array(cm, dtype=np.int64)
    t, c = np.nonzero(cm)
    true, lab = np.repeat(t, cm[t, c]), np.repeat(c, cm[t, c])
    assert np.array_equal(R.contingency(true, lab, *cm.shape), cm)
    got = analysis.confusion_matrix(torch.from_numpy(true), torch.from_numpy(lab), *cm.shape)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), cm)
    want = (metrics.adjusted_rand_score(true, lab), metrics.normalized_mutual_info_score(true, lab), cm.max(axis=0).sum() / cm.sum())
    for fn, ref, w in zip((analysis.adjusted_rand_score, analysis.normalized_mutual_info_score, analysis.purity),
                          (R.adjusted_rand, R.normalized_mutual_info, R.purity), want):
        for m in (got, got.to(torch.int32)):
            v = fn(m)
            assert isinstance(v, float) and abs(v - w) <= 1e-10, (fn.__name__, v, w)
        assert abs(ref(cm) - w) <= 1e-10, (ref.__name__, ref(cm), w)


def test_moment_scores_on_host_moments_are_the_yardstick():
    """the k x k part of the two indices is plain torch on the moments: on host tensors made from the yardstick's moments"""
    import torch
    from eagcn_amd import analysis
    for n, F in ((65, 3), (257, 7)):
        X, lab = _case(n, F)
        cen, sc, wss, cnt = R.moments(X, lab, 9)
        m = analysis.ClusterMoments(*(torch.from_numpy(a) for a in (cen, sc, wss, cnt)))
        db, k1, n1 = analysis.davies_bouldin_from_moments(m)
        ch, k2, n2 = analysis.calinski_harabasz_from_moments(m)
        assert int(k1) == int(k2) == 8 and int(n1) == int(n2) == n
        assert abs(float(db) - R.davies_bouldin(cen, sc, cnt)) <= 1e-12 and abs(float(ch) - R.calinski_harabasz(cen, wss, cnt)) <= 1e-10 * float(ch)
    # coincident centres: the pair counts as infinitely far apart, as in scikit-learn; all-zero scatter: 0
    cen = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0]])
    sc, wss, cnt = np.array([1.0, 2.0, 0.5]), np.array([2.0, 8.0, 0.5]), np.array([2, 2, 2])
    m = analysis.ClusterMoments(*(torch.from_numpy(a) for a in (cen, sc, wss, cnt)))
    assert abs(float(analysis.davies_bouldin_from_moments(m)[0]) - R.davies_bouldin(cen, sc, cnt)) <= 1e-15
    assert R.davies_bouldin(cen, sc, cnt) == pytest.approx((1.5 / 5 + 2.5 / 5 + 2.5 / 5) / 3, abs=1e-15)
    m0 = analysis.ClusterMoments(m.centers, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), m.counts)
    assert float(analysis.davies_bouldin_from_moments(m0)[0]) == 0.0 and float(analysis.calinski_harabasz_from_moments(m0)[0]) == 1.0
