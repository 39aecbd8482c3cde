"""The t-SNE / PCA yardstick of tsne_reference.py against scikit-learn on the CPU (no GPU needed): conditional and joint
probabilities, gradient and divergence, the update rule, PCA, and the distances the affinities start from."""
import numpy as np
import pytest
from scipy.spatial.distance import squareform

import tsne_reference as R

SHAPES = [(65, 7, 5.0), (200, 24, 15.0), (300, 700, 30.0)]


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: 'n%d_F%d_p%g' % s)
def case(request):
    n, F, perp = request.param
    X = R.make_data(0, n, F)
    D, c, P = R.affinities(X, perp)
    return dict(n=n, F=F, perp=perp, X=X, D=D, c=c, P=P)


def test_distances_equal_pairwise_distances_bit_for_bit(case):
    from sklearn.metrics import pairwise_distances
    want = pairwise_distances(case['X'], metric='euclidean', squared=True)
    assert want.dtype == np.float32
    assert np.array_equal(case['D'], want)


def test_conditional_probabilities(case):
    from sklearn.manifold._utils import _binary_search_perplexity
    want = _binary_search_perplexity(case['D'], case['perp'], 0)
    err = np.abs(case['c']['P'] - want).max()
    print('conditional P: max abs err %.2e, closest approach to the tolerance %.2e' % (err, case['c']['margin'].min()))
    assert err <= 1e-12


def test_joint_probabilities(case):
    from sklearn.manifold._t_sne import _joint_probabilities
    want = squareform(_joint_probabilities(case['D'], case['perp'], 0))
    err = np.abs(case['P'] - want).max()
    print('joint P: max abs err %.2e' % err)
    assert err <= 1e-12
    assert np.array_equal(case['P'], case['P'].T) and not case['P'].diagonal().any()


@pytest.mark.parametrize('alpha,spread', [(1.0, 1e-4), (12.0, 1e-4), (1.0, 5.0), (12.0, 0.3)])
def test_gradient_and_divergence(case, alpha, spread):
    from sklearn.manifold._t_sne import _kl_divergence
    n = case['n']
    Y = np.random.RandomState(1).randn(n, 2) * spread
    kl, grad = _kl_divergence(Y.ravel().copy(), squareform(case['P']) * alpha, 1, n, 2)
    got = R.objective(case['P'], Y, alpha)
    gerr = np.abs(got['grad'] - grad.reshape(n, 2)).max() / np.abs(grad).max()
    print('grad rel err %.2e, kl %.12g / %.12g, unclamped %.12g' % (gerr, got['kl'], kl, got['kl_free']))
    assert gerr <= 1e-12
    assert abs(got['kl'] - kl) <= 1e-12 * max(abs(kl), 1.0)
    assert abs(got['kl_free'] - kl) <= 1e-9 * max(abs(kl), 1.0)      # no Q reaches the clamp at these embeddings


def test_update_rule_against_gradient_descent(case):
    """60 iterations at the first stage's settings, in fp64: scikit-learn's _gradient_descent driven with the SAME objective (the
    yardstick's, which the test above pins to _kl_divergence) against the yardstick's driver -- with one objective only the update
    rule, the schedule and the bookkeeping are compared; two objectives 1e-16 apart drift to O(1) within some 50 iterations"""
    from sklearn.manifold._t_sne import _gradient_descent
    n = case['n']
    Y0 = np.random.RandomState(2).randn(n, 2) * 1e-4
    lr = max(n / 12.0 / 4.0, 50.0)

    def same(p, P, alpha, compute_error=True):
        ob = R.objective(P, p.reshape(n, 2), alpha)
        return ob['kl'], ob['grad'].ravel().copy()
    want, _, it = _gradient_descent(same, Y0.ravel().copy(), 0, 60, n_iter_check=50, n_iter_without_progress=250, momentum=0.5,
                                    learning_rate=lr, min_grad_norm=1e-7, args=[case['P'], 12.0])
    got = R.descend(case['P'], Y0, lr, early_exaggeration=12.0, max_iter=60)
    err = np.abs(got['Y'] - want.reshape(n, 2)).max() / np.abs(want).max()
    print('60 iterations: err / max|Y| %.2e' % err)
    assert it == 59 and got['n_iter'] == 60 and got['reason'] == R.STOP_MAX_ITER
    assert err <= 1e-9


@pytest.mark.parametrize('n,F,k', [(65, 7, 2), (200, 24, 8), (300, 700, 2)])
def test_pca_against_sklearn(n, F, k):
    from sklearn.decomposition import PCA
    X = R.make_pca_data(0, n, F, k)
    fit = R.pca(X, k)
    sk = PCA(n_components=k, svd_solver='full')
    emb = sk.fit_transform(X)
    cerr = np.abs(fit['components'] - sk.components_).max()
    verr = np.abs(fit['variance'] - sk.explained_variance_).max() / fit['variance'].max()
    eerr = np.abs(fit['embedding'] - emb).max() / np.abs(emb).max()
    print('PCA n=%d F=%d k=%d: components %.2e, variance %.2e, projection %.2e, least gap %.3f' % (n, F, k, cerr, verr, eerr,
                                                                                                 fit['gaps'].min()))
    assert fit['gaps'].min() >= 0.1
    assert cerr <= 1e-5 and verr <= 1e-5 and eerr <= 1e-5


def test_seed_searches_certify():
    found = R.find_seed(65, 7, 5.0)
    assert found is not None and found[3]['margin'].min() >= 1e-10
    out = R.find_seed(65, 7, 5.0, outlier=True)
    assert out is not None and out[3]['zero_rows'][0] and not out[3]['zero_rows'][1:].any()
    assert R.find_pca_seed(65, 24, 8) is not None


def test_exports_and_argument_errors_need_no_gpu():
    """null or out-of-envelope arguments return -1 with a message before any HIP call; CPU tensors raise"""
    import torch
    import __graft_entry__ as g
    g.build()
    import eagcn_amd
    from eagcn_amd import _lib, analysis
    for name in ('pca', 'PCAResult', 'tsne', 'TSNEResult', 'subsample'):
        assert hasattr(eagcn_amd, name) and hasattr(analysis, name), name
    lib = _lib.load()
    assert lib.eagcn_tsne_workspace_bytes(16) == 0 and lib.eagcn_tsne_workspace_bytes(32769) == 0
    assert lib.eagcn_tsne_workspace_bytes(17) > 0 and lib.eagcn_tsne_workspace_bytes(32768) > 0
    assert lib.eagcn_pca_workspace_bytes(100, 1025) == 0 and lib.eagcn_pca_workspace_bytes(100000, 700) > 0
    fake = 4096                                               # an aligned non-null address that is never dereferenced
    calls = [
        (lambda: lib.eagcn_sqdist(None, 100, 8, 8, fake, None), b'X is null'),
        (lambda: lib.eagcn_sqdist(fake, 16, 8, 8, fake, None), b'n = 16'),
        (lambda: lib.eagcn_sqdist(fake, 100, 1025, 1025, fake, None), b'F = 1025'),
        (lambda: lib.eagcn_sqdist(fake, 100, 8, 7, fake, None), b'ld = 7'),
        (lambda: lib.eagcn_tsne_affinities(fake, 100, 30.0, None, 100, fake, None, fake, 1 << 30, None), b'P is null'),
        (lambda: lib.eagcn_tsne_affinities(fake, 100, 100.0, fake, 100, fake, None, fake, 1 << 30, None), b'perplexity'),
        (lambda: lib.eagcn_tsne_gradient(fake, 102, fake, 100, 1.0, 1, fake, fake, fake, 1 << 30, None), b'ldp = 102'),
        (lambda: lib.eagcn_tsne_begin(fake, 100, 100, fake, 12.0, 50.0, 10, 300, 1e-7, fake, 64, None), b'workspace too small'),
        (lambda: lib.eagcn_tsne_iterate(fake, 32772, 32769, fake, 1 << 30, None), b'n = 32769'),
        (lambda: lib.eagcn_tsne_finish(fake, 100, 100, None, 0, None), b'workspace is null'),
        (lambda: lib.eagcn_pca_cov(fake, 100, 8, 8, None, fake, fake, 1 << 30, None), b'mean is null'),
        (lambda: lib.eagcn_pca_project(fake, 100, 8, 8, fake, fake, 9, fake, None), b'k = 9'),
    ]
    for call, msg in calls:
        assert call() == -1 and msg in lib.eagcn_last_error(), msg
    with pytest.raises(_lib.EagcnHipError, match='no CPU'):
        analysis.tsne(torch.zeros(100, 4))
    with pytest.raises(_lib.EagcnHipError, match='no CPU'):
        analysis.subsample(torch.zeros(10, dtype=torch.int64), [0], 3)
