"""CPU-only checks of the nearest-neighbour entry points (csrc/knn.hip): the symbols are exported and bound, the workspace size is the
header's formula, every argument outside the envelope comes back as a message before any HIP call, and the numpy yardstick of the GPU
tests (knn_reference) is scikit-learn's brute-force search and its trustworthiness."""
import numpy as np
import pytest

import knn_reference as R

NEW = ('eagcn_knn_workspace_bytes', 'eagcn_knn', 'eagcn_knn_rank')


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
    for name in ('knn', 'KNNResult', 'neighbor_ranks', 'trustworthiness', 'continuity', 'neighbor_agreement'):
        assert getattr(eagcn_amd, name) is getattr(analysis, name) and name in eagcn_amd.__all__
    assert analysis.KNN_MAX_K == 128


def test_workspace_bytes_is_the_header_formula(lib):
    from eagcn_amd import analysis
    for n in (1, 17, 63, 64, 65, 1027, 8209, 20011, 100000, 2 ** 31 - 1):
        for m in (1, 64, 65, 256, 4096, 100000, 2 ** 31 - 1):
            for F, k in ((1, 1), (700, 16), (1024, 128), (2, 90)):
                if k > n:
                    continue
                for slabs in (0, 1, 2, 3, 7, 64, 5000):
                    got = lib.eagcn_knn_workspace_bytes(n, m, F, k, slabs)
                    assert got == analysis.knn_workspace_bytes(n, m, F, k, slabs) > 0, (n, m, F, k, slabs)
    assert analysis.knn_slabs(100000, 100000) == 3 and analysis.knn_slabs(100000, 4096) == 63 and analysis.knn_slabs(20011, 256) == 63
    assert analysis.knn_slabs(65, 1, 7) == 2 and analysis.knn_slabs(8209, 8209, 3) == 3 and analysis.knn_slabs(17, 17, 5000) == 1
    assert analysis.knn_workspace_bytes(100000, 4096, 700, 16, 0) == 64 * 8 * 4096 * 16
    for n, m, F, k, slabs in ((0, 4, 4, 1, 0), (2 ** 31, 4, 4, 1, 0), (4, 0, 4, 1, 0), (4, 2 ** 31, 4, 1, 0), (10, 10, 0, 2, 0),
                              (10, 10, 1025, 1, 0), (10, 10, 4, 0, 0), (1000, 10, 4, 129, 0), (10, 10, 4, 2, -1)):
        assert lib.eagcn_knn_workspace_bytes(n, m, F, k, slabs) == 0, (n, m, F, k, slabs)


def test_arguments_outside_the_envelope_are_refused_without_a_gpu(lib):
    P, WS, BIG = 4096, 8192, 1 << 50                        # non-null addresses that are never dereferenced: every check comes first
    ok = dict(X=P, n=100, F=8, ldx=8, Q=P, m=100, ldq=8, k=3, excl=1, slabs=0, idx=P, dist=P, ws=WS, nbytes=BIG)

    def knn(**kw):
        a = dict(ok, **kw)
        return lib.eagcn_knn(a['X'], a['n'], a['F'], a['ldx'], a['Q'], a['m'], a['ldq'], a['k'], a['excl'], a['slabs'], a['idx'], a['dist'],
                             a['ws'], a['nbytes'], None)

    need = lib.eagcn_knn_workspace_bytes(100, 100, 8, 3, 0)
    assert need > 0
    cases = [(dict(k=0), 'k = 0 is not in 1 .. 128'), (dict(k=129, n=1000, m=1000), 'k = 129 is not in 1 .. 128'),
             (dict(k=100), 'k = 100 is more than the 99 candidates'), (dict(k=101, excl=0), 'k = 101 is more than the 100 candidates'),
             (dict(m=99), 'exclude_self needs m = n'), (dict(excl=2), 'exclude_self = 2'),
             (dict(F=1025, ldx=1025, ldq=1025), 'F = 1025 is not in 1 .. 1024'), (dict(F=0), 'F = 0 is not in 1 .. 1024'),
             (dict(ldx=7), 'row stride 7 of X is smaller than F = 8'), (dict(ldq=7), 'row stride 7 of Q is smaller than F = 8'),
             (dict(X=None), 'X is null'), (dict(Q=None), 'Q is null'), (dict(idx=None), 'idx is null'), (dict(dist=None), 'dist is null'),
             (dict(X=4098), 'X must be 4-byte aligned'), (dict(n=0, m=0), 'rows of X are not in'), (dict(n=2 ** 31, m=2 ** 31), 'rows of X are not in'),
             (dict(m=2 ** 31, excl=0), 'rows of Q are not in'), (dict(slabs=-1), 'slabs = -1 is negative'),
             (dict(ws=None), 'workspace is null'), (dict(ws=WS + 16), 'workspace must be 256-byte aligned'),
             (dict(nbytes=need - 1), 'workspace too small (%d < %d bytes)' % (need - 1, need))]
    for kw, text in cases:
        assert knn(**kw) == -1, kw
        assert 'eagcn_knn: ' in _msg(lib) and text in _msg(lib), (kw, _msg(lib))

    okr = dict(X=P, n=100, F=8, ld=8, cand=P, k=3, slabs=0, rank=P, ws=WS, nbytes=BIG)

    def rank(**kw):
        a = dict(okr, **kw)
        return lib.eagcn_knn_rank(a['X'], a['n'], a['F'], a['ld'], a['cand'], a['k'], a['slabs'], a['rank'], a['ws'], a['nbytes'], None)

    cases = [(dict(k=0), 'k = 0 is not in 1 .. 128'), (dict(k=129), 'k = 129 is not in 1 .. 128'), (dict(F=1025, ld=1025), 'F = 1025 is not in'),
             (dict(ld=7), 'row stride 7 of X is smaller than F = 8'), (dict(X=None), 'X is null'), (dict(cand=None), 'cand is null'),
             (dict(rank=None), 'rank is null'), (dict(n=0), 'rows of X are not in'), (dict(slabs=-2), 'slabs = -2 is negative'),
             (dict(ws=None), 'workspace is null'), (dict(ws=WS + 16), 'workspace must be 256-byte aligned'),
             (dict(nbytes=need - 1), 'workspace too small (%d < %d bytes)' % (need - 1, need))]
    for kw, text in cases:
        assert rank(**kw) == -1, kw
        assert 'eagcn_knn_rank: ' in _msg(lib) and text in _msg(lib), (kw, _msg(lib))


def test_python_refuses_host_tensors_and_bad_arguments():
    import torch
    from eagcn_amd import analysis
    from eagcn_amd._lib import EagcnHipError
    with pytest.raises(EagcnHipError, match='no CPU path'):
        analysis.knn(torch.zeros(20, 4), 3)
    with pytest.raises(EagcnHipError, match='no CPU path'):
        analysis.neighbor_ranks(torch.zeros(20, 4), torch.zeros(20, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match='metric'):
        analysis.knn(torch.zeros(20, 4), 3, metric='manhattan')
    with pytest.raises(ValueError, match='should be less than n_samples / 2'):
        analysis.trustworthiness(torch.zeros(20, 4), torch.zeros(20, 2), 10)
    idx = torch.tensor([[1, 2], [0, 2], [0, 1], [4, 0], [3, 0]])
    got = analysis.neighbor_agreement(idx, torch.tensor([0, 0, 1, 1, 1]))
    assert got.dtype == torch.float64 and got.tolist() == [0.5, 0.5, 0.0, 0.5, 0.5]


@pytest.mark.parametrize('n,F,k', [(17, 1, 16), (65, 3, 5), (257, 7, 17), (515, 32, 128), (300, 700, 16)])
def test_yardstick_neighbours_are_sklearn_brute_force(n, F, k):
    """Gaussian data has no ties: the yardstick's indices equal sklearn's, for a self-join and for separate queries."""
    from sklearn.neighbors import NearestNeighbors
    X = R.gaussian(n + F, n, F).astype(np.float64)
    Q = R.gaussian(n + F + 1, 40, F).astype(np.float64)
    nn = NearestNeighbors(n_neighbors=k, algorithm='brute', metric='sqeuclidean').fit(X)
    idx, d = R.neighbours(R.sqdist64(X, X), k, exclude_self=True)
    sd, si = nn.kneighbors()                                   # (no argument: a row is not its own neighbour)
    assert np.array_equal(idx, si) and np.allclose(d, sd, rtol=1e-10, atol=0)
    idx, d = R.neighbours(R.sqdist64(Q, X), k)
    sd, si = nn.kneighbors(Q)
    assert np.array_equal(idx, si) and np.allclose(d, sd, rtol=1e-10, atol=0)
    assert np.abs(R.sqdist64(Q, X, gram=True) - R.sqdist64(Q, X)).max() <= 1e-12 * R.sqdist64(Q, X).max()
    idx0, d0 = R.neighbours(R.sqdist64(X, X), 1)
    assert np.array_equal(idx0[:, 0], np.arange(n)) and not d0.any()


def test_yardstick_order_breaks_ties_by_index_and_ranks_agree():
    X, _ = R.clusters(3, 129, 5, n_dup=7)
    D = R.sqdist64(X, X)
    assert (np.sort(D + np.diag(np.full(129, np.inf)), axis=1)[:, 0] == 0).sum() >= 14      # the duplicated rows see each other at 0
    o = R.order(D, exclude_self=True)
    s = np.take_along_axis(D, o, axis=1)
    assert np.all((s[:, 1:] > s[:, :-1]) | ((s[:, 1:] == s[:, :-1]) & (o[:, 1:] > o[:, :-1])))
    assert np.array_equal(R.ranks(D, o), np.arange(1, 129)[None, :].repeat(129, axis=0))
    cand = np.stack([np.arange(129), np.full(129, -1), np.full(129, 129)], axis=1)
    assert np.array_equal(R.ranks(D, cand), np.full((129, 3), -1))
    Dn = D.copy()
    Dn[:, 5] = np.nan                                           # a NaN distance ranks behind every number
    assert np.all(R.order(Dn, exclude_self=False)[:, -1] == 5)


@pytest.mark.parametrize('n,F,k', [(65, 3, 5), (257, 7, 12), (257, 700, 5), (515, 24, 12)])
def test_yardstick_trustworthiness_is_sklearn(n, F, k):
    from sklearn.manifold import trustworthiness
    found = R.find_seed(n, F, k)
    assert found is not None
    _, X, Y, DX, DY = found
    t, nb, r = R.trustworthiness(DX, DY, k)
    want = trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=k, metric='euclidean')
    assert abs(t - want) <= 1e-12, (t, want)
    assert 0.5 < t < 1.0 and nb.shape == r.shape == (n, k) and r.min() >= 1 and r.max() <= n - 1
    assert R.margin(700) == 704 * 2.0 ** -23
