"""The device k-means (csrc/reps.hip, eagcn_amd.analysis.kmeans) against the fp64 yardstick of kmeans_reference.py, which
test_kmeans_cpu.py pins to scikit-learn.

Full fits are compared on inputs the yardstick itself certifies (find_seed): no cluster ever empty, at least three iterations, and
every point's relative margin (d2 - d1) / (d2 + d1) between its two nearest centres at least 2e-4 in every iteration -- above the worst
fp32 error of a 700-term sum of non-negative terms, 700 * 2^-24 = 4e-5, so no label can flip for arithmetic reasons and labels,
n_iter and counts must be IDENTICAL.  Centroids are held to 1e-5 of max|C| (the project's parity bound), inertia to 1e-5 relative."""
import os
import re

import numpy as np
import pytest
import torch

from kmeans_reference import find_seed, lloyd, make_data, margins, sqdist

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'eagcn_amd', 'csrc', 'reps.hip')).read()
KM_ROWS = int(re.search(r'constexpr int KM_ROWS = (\d+);', _SRC).group(1))
MARGIN = 2e-4
SHAPES = [(1, 2), (3, 7), (5, 3), (24, 7), (255, 7), (256, 4), (700, 6)]
SHAPES_K16 = [(4, 16), (257, 16)]
SHAPES_EDGE = [(1024, 8), (512, 16), (1021, 8)]             # k * pad4(F) = 8192: 96 KB of LDS, the limit is raised for the launch


def _rows(cap):
    ns = {63, 64, 65, KM_ROWS - 1, KM_ROWS, KM_ROWS + 1, 2 * KM_ROWS + 3, 255, 257, 515, 1027}
    return sorted(n for n in ns if 17 <= n <= cap)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kmeans(*a, **kw):
    from eagcn_amd.analysis import kmeans
    return kmeans(*a, **kw)


def _check_fit(res, fit, tag):
    C = fit['centers']
    cerr = np.abs(res.centers.cpu().numpy().astype(np.float64) - C).max() / np.abs(C).max()
    ierr = abs(res.inertia - fit['inertia']) / fit['inertia']
    print('%s: n_iter %d / %d, centroid err / max|C| %.2e, inertia rel err %.2e' % (tag, res.n_iter, fit['n_iter'], cerr, ierr))
    assert np.array_equal(res.labels.cpu().numpy(), fit['labels']), tag
    assert res.n_iter == fit['n_iter'], tag
    assert np.array_equal(res.counts.cpu().numpy(), fit['counts']), tag
    assert cerr <= 1e-5, (tag, cerr)
    assert ierr <= 1e-5, (tag, ierr)
    assert res.n_empty == 0 and res.converged, tag


@pytest.mark.parametrize('F,k', SHAPES + SHAPES_K16)
def test_full_fit_equals_the_yardstick(F, k):
    for n in _rows(257 if k == 16 else 1100):
        found = find_seed(n, F, k, margin=MARGIN)
        assert found is not None, 'no seed in 0..63 for n=%d F=%d k=%d' % (n, F, k)
        seed, X, init, fit = found
        res = _kmeans(_dev(X), k, init=_dev(init))
        _check_fit(res, fit, 'n=%d F=%d k=%d seed=%d' % (n, F, k, seed))


@pytest.mark.parametrize('F,k', SHAPES_EDGE)
def test_full_fit_at_the_edge_of_the_envelope(F, k):
    for n in (65, 2 * KM_ROWS + 3):
        found = find_seed(n, F, k, margin=MARGIN)
        assert found is not None, 'no seed in 0..63 for n=%d F=%d k=%d' % (n, F, k)
        seed, X, init, fit = found
        _check_fit(_kmeans(_dev(X), k, init=_dev(init)), fit, 'n=%d F=%d k=%d seed=%d' % (n, F, k, seed))


@pytest.mark.parametrize('F,k', [(700, 7), (24, 16)])
def test_single_iteration_over_many_workgroups(F, k):
    """n = 20011 rows (313 chunks): labels of ONE iteration equal the fp64 argmin wherever the margin is at least 2e-4 and are one of
    the two nearest centres elsewhere (at most 2 % of the points); the centroid update from the device's own labels is the fp64 mean."""
    from eagcn_amd.analysis import _Problem
    n = 20011
    X, init, _, _ = make_data(0, n, F, k)
    p = _Problem(_dev(X), k)
    p.begin(_dev(init), 1e-4)
    p.iterate()
    lab = p.labels.cpu().numpy()
    state = p.state_i.tolist()
    d = sqdist(X, init)
    order = np.argsort(d, axis=1, kind='stable')
    safe = margins(d) >= MARGIN
    print('F=%d k=%d: %.2f %% of the points below the margin' % (F, k, 100.0 * (1 - safe.mean())))
    assert (~safe).mean() <= 0.02
    assert np.array_equal(lab[safe], order[safe, 0])
    assert np.all((lab == order[:, 0]) | (lab == order[:, 1]))
    assert state[1] == 1 and state[2] == n                   # n_iter, changed: every label is new in the first iteration
    counts = np.bincount(lab, minlength=k)
    assert np.array_equal(p.counts.cpu().numpy(), counts) and counts.min() > 0
    X64 = X.astype(np.float64)
    want = np.stack([X64[lab == c].mean(axis=0) for c in range(k)])
    cerr = np.abs(p.centers.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
    print('centroid err / max|C| %.2e' % cerr)
    assert cerr <= 1e-5
    mind = p.mind.cpu().numpy().astype(np.float64)
    # (an fp32 sum of F non-negative terms, each rounded three times: (F + 3) * 2^-24 <= 4.2e-5 of the row's own distance)
    assert np.all(np.abs(mind - d.min(axis=1)) <= 5e-5 * d.min(axis=1))
    shift = ((p.centers.cpu().numpy().astype(np.float64) - init.astype(np.float64)) ** 2).sum()
    assert abs(p.state_d[1].item() - shift) <= 1e-9 * shift and abs(p.state_d[0].item() - mind.sum()) <= 1e-6 * mind.sum()


@pytest.fixture(scope='module')
def blob():
    """one certified input shared by the property tests: n = 2 KM_ROWS + 3 rows, F = 24, k = 7"""
    found = find_seed(2 * KM_ROWS + 3, 24, 7, margin=MARGIN)
    assert found is not None
    return found


def _same(a, b):
    assert torch.equal(a.centers, b.centers) and torch.equal(a.labels, b.labels) and torch.equal(a.counts, b.counts)
    assert a.inertia == b.inertia and a.n_iter == b.n_iter and a.n_empty == b.n_empty


def test_two_runs_are_bit_identical(blob):
    _, X, init, fit = blob
    a, b = _kmeans(_dev(X), 7, init=_dev(init)), _kmeans(_dev(X), 7, init=_dev(init))
    _same(a, b)
    X2, init2, _, _ = make_data(5, 5000, 700, 6)              # many workgroups, the reference's width
    _same(_kmeans(_dev(X2), 6, init=_dev(init2), max_iter=5), _kmeans(_dev(X2), 6, init=_dev(init2), max_iter=5))


def test_result_does_not_depend_on_sync_every(blob):
    _, X, init, fit = blob
    runs = [_kmeans(_dev(X), 7, init=_dev(init), sync_every=s, max_iter=300) for s in (1, 7, 300)]
    assert runs[0].n_iter == fit['n_iter']
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    capped = [_kmeans(_dev(X), 7, init=_dev(init), sync_every=s, max_iter=2) for s in (1, 7)]      # stopped by max_iter
    assert capped[0].n_iter == 2 and not capped[0].converged
    _same(capped[0], capped[1])


@pytest.mark.parametrize('F,k,n', [(24, 7, 131), (700, 6, 257), (5, 3, 65)])
def test_strided_rows_equal_contiguous_rows(F, k, n):
    """ld = F + 3: rows that are not 16-byte aligned (scalar loads) give the bits of the contiguous (16-byte load) path"""
    X, init, _, _ = make_data(1, n, F, k)
    wide = torch.full((n, F + 3), 7.0e5, device='cuda')       # what lies between the rows must never be read into a sum
    wide[:, :F] = _dev(X)
    view = wide[:, :F]
    assert view.stride(0) == F + 3 and not view.is_contiguous()
    _same(_kmeans(view, k, init=_dev(init)), _kmeans(_dev(X), k, init=_dev(init)))


def test_empty_cluster_keeps_its_centroid():
    k, F, n = 5, 16, 200
    for seed in range(64):
        X, init, _, _ = make_data(seed, n, F, k)
        init = init.copy()
        init[2] = 1000.0                                      # far from every point: never the nearest centre
        fit = lloyd(X, init)
        if fit['min_margin'] >= MARGIN and fit['n_empty'] == 1 and fit['n_iter'] >= 2:
            break
    else:
        pytest.fail('no seed in 0..63')
    res = _kmeans(_dev(X), k, init=_dev(init))
    got = res.centers.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[2], init[2].astype(np.float64))
    assert res.n_empty == 1 and res.counts[2].item() == 0
    assert np.array_equal(res.labels.cpu().numpy(), fit['labels']) and res.n_iter == fit['n_iter']
    others = [c for c in range(k) if c != 2]
    assert np.abs(got[others] - fit['centers'][others]).max() <= 1e-5 * np.abs(fit['centers'][others]).max()


@pytest.mark.parametrize('n,F', [(63, 5), (131, 700), (1027, 24)])
def test_one_cluster_is_the_column_mean(n, F):
    X, _, _, _ = make_data(3, n, F, 2)
    res = _kmeans(_dev(X), 1, init=_dev(X[:1]))
    mean = X.astype(np.float64).mean(axis=0)
    assert np.abs(res.centers.cpu().numpy()[0] - mean).max() <= 1e-5 * np.abs(mean).max()
    assert res.labels.max().item() == 0 and res.counts.tolist() == [n]
    want = ((X.astype(np.float64) - mean) ** 2).sum()
    assert abs(res.inertia - want) <= 1e-5 * want


@pytest.mark.parametrize('F,k', [(1, 2), (3, 7), (24, 7), (700, 6), (4, 16), (257, 16)])
def test_n_equal_k_every_point_is_its_own_cluster(F, k):
    X, init, _, _ = make_data(0, k, F, k)
    res = _kmeans(_dev(X), k, init=_dev(init))
    assert res.inertia == 0.0 and res.n_empty == 0 and res.counts.tolist() == [1] * k
    lab = res.labels.cpu().numpy()
    assert sorted(lab.tolist()) == list(range(k))
    assert np.array_equal(res.centers.cpu().numpy()[lab], X)


def test_kmeans_plus_plus_seeding_and_n_init():
    """blobs 30 sigma apart: every initial centre is a row of X, the centres are distinct, and the best of eight seeded runs is no
    worse than Lloyd started from the true means"""
    k, F, n = 5, 16, 500
    rs = np.random.RandomState(11)
    means = np.zeros((k, F))
    means[np.arange(k), np.arange(k)] = 30.0 * np.sqrt(2.0)          # pairwise distance 60 sigma
    lab = rs.randint(0, k, n)
    lab[:k] = np.arange(k)
    X = (means[lab] + rs.randn(n, F)).astype(np.float32)
    dist = np.sqrt(((means[:, None] - means[None]) ** 2).sum(-1))
    assert dist[~np.eye(k, dtype=bool)].min() >= 30.0
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1234)
    Xd = _dev(X)
    res = _kmeans(Xd, k, init='k-means++', n_init=8, generator=gen)
    ic = res.init_centers.cpu().numpy()
    for c in range(k):
        assert (X == ic[c]).all(axis=1).any(), c
    assert len({ic[c].tobytes() for c in range(k)}) == k
    true = _kmeans(Xd, k, init=_dev(means.astype(np.float32)))
    assert res.inertia <= (1 + 1e-6) * true.inertia
    assert res.labels.shape == (n,) and int(res.counts.sum()) == n
    gen.manual_seed(1234)
    again = _kmeans(Xd, k, init='k-means++', n_init=8, generator=gen)
    _same(res, again)
    rnd = _kmeans(Xd, k, init='random', generator=gen)
    ir = rnd.init_centers.cpu().numpy()
    assert all((X == ir[c]).all(axis=1).any() for c in range(k)) and len({ir[c].tobytes() for c in range(k)}) == k
