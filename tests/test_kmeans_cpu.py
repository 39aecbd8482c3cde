"""CPU-only checks of the atom-representation dump and k-means entry points (csrc/reps.hip): the symbols are exported and bound, the
workspace size is the header's formula, every argument outside the envelope comes back as a message before any HIP call, and the
numpy yardstick of the GPU tests (kmeans_reference.lloyd) is scikit-learn's Lloyd wherever no cluster runs empty."""
import ctypes as C
import warnings

import numpy as np
import pytest

from kmeans_reference import lloyd, make_data

NEW = ('eagcn_rep_gather', 'eagcn_rep_gather_dense', 'eagcn_kmeans_workspace_bytes', 'eagcn_kmeans_begin', 'eagcn_kmeans_iterate',
       'eagcn_kmeans_finish', 'eagcn_kmeans_assign')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from eagcn_amd import _lib
    return _lib.load()


def test_symbols_exported_bound_and_abi_unchanged(lib):
    from eagcn_amd import _lib, analysis
    import eagcn_amd
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.eagcn_abi_version() == _lib.ABI_VERSION == 8
    for name in ('RepBuffers', 'dump_atom_rep', 'kmeans', 'KMeansResult', 'confusion_matrix'):
        assert getattr(eagcn_amd, name) is getattr(analysis, name)


def test_workspace_bytes_is_the_header_formula(lib):
    from eagcn_amd import analysis
    for n, F, k in ((7, 1, 7), (1, 1, 1), (63, 3, 7), (64, 5, 3), (65, 24, 7), (257, 257, 16), (1027, 255, 7), (20011, 700, 7),
                    (20011, 24, 16), (100000, 700, 6), (32768, 1024, 8), (32769, 512, 16), (2 ** 31 - 1, 4, 2)):
        assert lib.eagcn_kmeans_workspace_bytes(n, F, k) == analysis.workspace_bytes(n, F, k) > 0, (n, F, k)
    lay = analysis.workspace_layout(100000, 700, 6)
    assert lay['centers'] == 256 and lay['counts'] == 256 + 16896 and lay['labels'] == lay['counts'] + 256
    for n, F, k in ((0, 4, 2), (2 ** 31, 4, 2), (10, 0, 2), (10, 1025, 1), (10, 4, 0), (10, 4, 17)):
        assert lib.eagcn_kmeans_workspace_bytes(n, F, k) == 0, (n, F, k)


def _msg(lib):
    return lib.eagcn_last_error().decode()


def test_kmeans_arguments_outside_the_envelope_are_refused_without_a_gpu(lib):
    X, WS, BIG = 4096, 8192, 1 << 40                       # non-null addresses that are never dereferenced: every check comes first
    ok = dict(X=X, n=100, F=8, ld=8, k=3, ws=WS, nbytes=BIG)

    def call(fn, **kw):
        a = dict(ok, **kw)
        if fn == 'begin':
            return lib.eagcn_kmeans_begin(a['X'], a['n'], a['F'], a['ld'], a['k'], a.get('init', X), a.get('tol', 1e-4), a['ws'], a['nbytes'],
                                          None)
        if fn == 'assign':
            return lib.eagcn_kmeans_assign(a['X'], a['n'], a['F'], a['ld'], a.get('centers', X), a['k'], a.get('labels', X),
                                           a.get('mind', X), a['ws'], a['nbytes'], None)
        return getattr(lib, 'eagcn_kmeans_' + fn)(a['X'], a['n'], a['F'], a['ld'], a['k'], a['ws'], a['nbytes'], None)

    need = lib.eagcn_kmeans_workspace_bytes(100, 8, 3)
    cases = [(dict(X=None), 'X is null'), (dict(k=0), 'k = 0 is not in 1 .. 16'), (dict(k=17), 'k = 17 is not in 1 .. 16'),
             (dict(F=0), 'F = 0 is not in 1 .. 1024'), (dict(F=1025, ld=1025), 'F = 1025 is not in 1 .. 1024'),
             (dict(F=1024, ld=1024, k=9), 'k x pad4(F) = 9 x 1024 is more than 8192'), (dict(F=1021, ld=1021, k=9), 'more than 8192'),
             (dict(n=2), 'n = 2 rows are fewer than k = 3'), (dict(n=2 ** 31), 'does not fit the 32-bit row index'),
             (dict(ld=7), 'row stride ld = 7 is smaller than F = 8'), (dict(X=4098), 'X must be 4-byte aligned'),
             (dict(ws=None), 'workspace is null'), (dict(ws=WS + 16), 'workspace must be 256-byte aligned'),
             (dict(nbytes=need - 1), 'workspace too small (%d < %d bytes)' % (need - 1, need))]
    for fn in ('begin', 'iterate', 'finish', 'assign'):
        for kw, text in cases:
            assert call(fn, **kw) == -1, (fn, kw)
            assert ('eagcn_kmeans_%s: ' % fn) in _msg(lib) and text in _msg(lib), (fn, kw, _msg(lib))
    assert call('begin', init=None) == -1 and 'init is null' in _msg(lib)
    assert call('begin', tol=-1.0) == -1 and 'is negative' in _msg(lib)
    for kw, text in ((dict(centers=None), 'centers is null'), (dict(labels=None), 'labels is null'), (dict(mind=None), 'mind is null')):
        assert call('assign', **kw) == -1 and text in _msg(lib), kw


def test_rep_gather_null_and_size_arguments_are_refused_without_a_gpu(lib):
    from eagcn_amd import _lib
    P = 4096
    lay = _lib.make_layout([5, 3], [16, 16])
    b = _lib.new_batch(4, 10, [9, 4])
    b.nat = b.row0 = P
    good = [C.byref(b), P, C.byref(lay), None, P, 1, 18, P, P, P, P, P, P, 40, None]
    names = {0: 'batch is null', 2: 'layout is null', 4: 'subtype is null', 7: 'mol_index is null', 8: 'count is null',
             9: 'scratch is null', 10: 'output buffer is null', 11: 'output buffer is null', 12: 'output buffer is null'}
    for pos, text in names.items():
        a = list(good)
        a[pos] = None
        assert lib.eagcn_rep_gather(*a) == -1 and text in _msg(lib), (pos, _msg(lib))
    a = list(good)
    a[13] = 39
    assert lib.eagcn_rep_gather(*a) == -1 and 'cap = 39 is not in B x N = 40' in _msg(lib), _msg(lib)
    b.T = 7
    a = list(good)
    a[1] = None
    assert lib.eagcn_rep_gather(*a) == -1 and 'null packed matrix' in _msg(lib)
    dgood = [P, 4, 10, 8, P, 10, 1, 18, P, P, P, P, P, P, 40, None]
    for pos, text in ((0, 'dense is null'), (4, 'subtype is null'), (9, 'count is null')):
        a = list(dgood)
        a[pos] = None
        assert lib.eagcn_rep_gather_dense(*a) == -1 and text in _msg(lib), (pos, _msg(lib))
    a = list(dgood)
    a[2] = 9
    assert lib.eagcn_rep_gather_dense(*a) == -1 and 'N = 9 is smaller' in _msg(lib), _msg(lib)


@pytest.mark.parametrize('n,F,k', [(7, 1, 7), (63, 3, 7), (255, 5, 3), (515, 24, 7), (1027, 24, 7), (257, 255, 7)])
def test_numpy_yardstick_is_sklearn_lloyd(n, F, k):
    """Same labels, same n_iter, inertia to 2e-7 against sklearn KMeans(init=C0, n_init=1, algorithm='lloyd', tol=1e-4) on the first
    seed whose fit empties no cluster (scikit-learn relocates empty clusters, the yardstick keeps them: the one deviation)."""
    from sklearn.cluster import KMeans
    for seed in range(8):
        X, init, _, _ = make_data(seed, n, F, k)
        fit = lloyd(X, init)
        if not fit['ever_empty']:
            break
    else:
        pytest.fail('no seed in 0..7 keeps every cluster populated')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        km = KMeans(n_clusters=k, init=init.astype(np.float64), n_init=1, algorithm='lloyd', tol=1e-4, max_iter=300).fit(X.astype(np.float64))
    assert np.array_equal(km.labels_, fit['labels'])
    assert km.n_iter_ == fit['n_iter']
    # (the floor: an inertia of exactly 0, n == k, against scikit-learn's fp64 arithmetic on the mean-centred rows)
    assert abs(km.inertia_ - fit['inertia']) <= 2e-7 * fit['inertia'] + 1e-13 * float((X.astype(np.float64) ** 2).sum())
    assert np.abs(km.cluster_centers_ - fit['centers']).max() <= 1e-9 * max(np.abs(fit['centers']).max(), 1.0)
