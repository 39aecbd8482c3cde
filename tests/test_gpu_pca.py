"""The device PCA (csrc/embed.hip: eagcn_pca_cov / eagcn_pca_project, eagcn_amd.analysis.pca) against the fp64 yardstick of
tsne_reference.py, which test_tsne_cpu.py pins to sklearn.decomposition.PCA(svd_solver='full').

The inputs have their covariance spectrum by construction (make_pca_data): relative eigengaps (lambda_m - lambda_{m+1}) / lambda_1 of
0.11 and more for m <= 8, which find_pca_seed certifies.  Bounds: the mean, an fp64 sum, to 1e-6 of max|mean|; the covariance, fp32
products summed in fp32 over 256 rows and in fp64 beyond, to 1e-5 of max|cov|; an eigenvector moves by the covariance error over the
gap, about 1e-5, so components and embedding are held to 1e-4 of their maxima -- a tenfold margin."""
import numpy as np
import pytest
import torch

import tsne_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(17, 3), (65, 24), (257, 700), (1027, 1024)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('k', [1, 2, 8])
@pytest.mark.parametrize('n,F', SHAPES)
def test_pca_equals_the_yardstick(n, F, k):
    from eagcn_amd._lib import EagcnHipError
    from eagcn_amd.analysis import pca, pca_cov
    if k > F:                                                 # more components than columns: refused, as scikit-learn refuses it
        with pytest.raises(EagcnHipError, match='k = 8'):
            pca(_dev(R.make_pca_data(0, n, F)), k)
        return
    found = R.find_pca_seed(n, F, k)
    assert found is not None, 'no certified seed for n=%d F=%d k=%d' % (n, F, k)
    seed, X, fit = found
    Xd = _dev(X)
    mean, cov = pca_cov(Xd)
    res = pca(Xd, k)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    comp, emb, var = res.components.cpu().numpy().astype(np.float64), res.embedding.cpu().numpy().astype(np.float64), res.explained_variance.cpu().numpy()
    merr = np.abs(mean - fit['mean']).max() / np.abs(fit['mean']).max()
    cerr = np.abs(cov - fit['cov']).max() / np.abs(fit['cov']).max()
    verr = np.abs(var - fit['variance']).max() / fit['variance'].max()
    perr = np.abs(comp - fit['components']).max() / np.abs(fit['components']).max()
    eerr = np.abs(emb - fit['embedding']).max() / np.abs(fit['embedding']).max()
    print('n=%d F=%d k=%d seed %d: mean %.2e, cov %.2e, variance %.2e, components %.2e, embedding %.2e, least gap %.3f'
          % (n, F, k, seed, merr, cerr, verr, perr, eerr, fit['gaps'].min()))
    assert merr <= 1e-6 and cerr <= 1e-5 and verr <= 1e-5
    assert perr <= 1e-4 and eerr <= 1e-4
    big = np.abs(fit['components']).argmax(axis=1)
    assert np.all(comp[np.arange(k), big] > 0)                # signs: the entry of largest magnitude of every component is positive
    assert np.array_equal(np.sign(comp[np.arange(k), big]), np.sign(fit['components'][np.arange(k), big]))
    assert np.array_equal(cov, cov.T)
    assert torch.equal(res.mean.cpu(), torch.from_numpy(mean)) and res.embedding.shape == (n, k) and res.components.shape == (k, F)


@pytest.mark.parametrize('n,F', [(65, 24), (300, 701)])
def test_strided_rows_and_repeat_runs(n, F):
    from eagcn_amd.analysis import pca
    X = R.make_pca_data(1, n, F)
    wide = torch.full((n, F + 3), 7.0e5, device='cuda')
    wide[:, :F] = _dev(X)
    a, b, c = pca(wide[:, :F], 2), pca(_dev(X), 2), pca(_dev(X), 2)
    for x, y in ((a, b), (b, c)):
        assert torch.equal(x.embedding, y.embedding) and torch.equal(x.components, y.components) and torch.equal(x.mean, y.mean)


def test_many_rows_over_all_slabs():
    """n = 20011: every row slab of the covariance and 313 chunks of the column sums"""
    from eagcn_amd.analysis import pca_cov
    n, F = 20011, 40
    rs = np.random.RandomState(0)
    X = (rs.randn(n, F) * (1.0 + np.arange(F)) + 100.0 * rs.randn(F)).astype(np.float32)
    mean, cov = pca_cov(_dev(X))
    X64 = X.astype(np.float64)
    wm = X64.mean(axis=0)
    wc = (X64 - wm).T @ (X64 - wm) / (n - 1)
    merr = np.abs(mean.cpu().numpy() - wm).max() / np.abs(wm).max()
    cerr = np.abs(cov.cpu().numpy() - wc).max() / np.abs(wc).max()
    print('n=%d F=%d: mean %.2e, cov %.2e' % (n, F, merr, cerr))
    assert merr <= 1e-6 and cerr <= 1e-5
