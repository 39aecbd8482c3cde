"""The device silhouette, cluster moments and the scores built on them (csrc/silhouette.hip, eagcn_amd.analysis) against
(a) the fp64 yardstick of silhouette_reference.py, which test_silhouette_cpu.py pins to scikit-learn, within margin(F) + 2^-22 -- a
    distance carries at most half of margin(F) = (F + 4) 2^-23 relative (the bound of its square) plus one rounding of the root, a and b
    are means of such distances, and s = 1 - a / b or b / a - 1 carries at most twice that --, and
(b) analysis.sqdist, existing code with the same distance bits: fp64 sums of the roots of that matrix on the host, to 1e-12 (only the
    order of the fp64 sums differs)."""
import functools

import numpy as np
import pytest
import torch

import silhouette_reference as R

pytestmark = pytest.mark.gpu

NS = (17, 63, 64, 65, 129, 257, 1027)
FS = (1, 3, 32, 33, 700)
K = 9


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wide(X, extra=3):
    """the rows of X inside a wider matrix (ld = F + extra) whose other columns hold large numbers"""
    wide = torch.full((X.shape[0], X.shape[1] + extra), 7.0e5, device='cuda')
    wide[:, :X.shape[1]] = X
    return wide[:, :X.shape[1]]


def _bits(t):
    return t.contiguous().view(torch.int64)


@functools.lru_cache(maxsize=None)
def _case(n, F):
    """(X, labels with k = 9: cluster 6 empty, cluster 7 one row; at n = 1027 clusters of exactly 1, 64, 65 and 128 rows) and the
    yardstick's samples and counts"""
    X, lab = R.clusters(n * 1000 + F, n, F, n_dup=5)
    lab = R.tile_edge_labels(n) if n == 1027 else R.remap9(lab, n)
    s, cnt = R.silhouette_samples(X, lab, K)
    return X, lab, s, cnt


def _check_summary(res, lab, k):
    """cluster_means, score and n_ignored of a device result against its own samples"""
    s = res.samples.cpu().numpy()
    score, means, ignored = R.summary(s, lab, k)
    got = res.cluster_means.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(means)) and np.abs(np.nan_to_num(got - means)).max() <= 1e-12
    assert abs(float(res.score) - score) <= 1e-12 and int(res.n_ignored) == ignored
    assert res.samples.dtype == res.score.dtype == res.cluster_means.dtype == torch.float64
    assert res.counts.dtype == res.n_ignored.dtype == torch.int64 and res.score.is_cuda and res.n_ignored.is_cuda


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('n', NS)
def test_samples_against_the_yardstick_and_sqdist(n, F):
    from eagcn_amd.analysis import silhouette_samples, sqdist
    X, lab, want, cnt = _case(n, F)
    assert cnt[6] == 0 and cnt[7] == 1
    if n == 1027:
        assert cnt[1] == 64 and cnt[2] == 65 and cnt[3] == 128
    Xd = _wide(_dev(X)) if (n + F) % 2 else _dev(X)
    res = silhouette_samples(Xd, _dev(lab), K)
    got = res.samples.cpu().numpy()
    bound = R.margin(F) + 2.0 ** -22
    print('n=%d F=%d: worst |sample - yardstick| = %.3e (bound %.3e)' % (n, F, np.abs(got - want).max(), bound))
    assert got.shape == (n,) and np.abs(got - want).max() <= bound
    assert got[lab == 7][0] == 0.0                             # alone in its cluster
    assert np.array_equal(res.counts.cpu().numpy(), cnt)
    _check_summary(res, lab, K)
    # the same distances, bit for bit: roots of the float32 matrix of sqdist, summed in fp64 on the host
    D = np.sqrt(sqdist(Xd).cpu().numpy()).astype(np.float64)
    pinned, _ = R.silhouette_from_distances(D, lab, K)
    print('    worst |sample - samples from sqdist| = %.3e' % np.abs(got - pinned).max())
    assert np.abs(got - pinned).max() <= 1e-12


@pytest.mark.parametrize('n,F', [(129, 3), (1027, 33)])
def test_rows_outside_the_labelling_take_no_part(n, F):
    from eagcn_amd.analysis import silhouette_samples, cluster_moments
    X, lab, _, _ = _case(n, F)
    out = lab.copy()
    out[3::7] = -1
    out[5::11] = K
    keep = (out >= 0) & (out < K)
    Xd = _dev(X)
    res = silhouette_samples(Xd, _dev(out), K)
    got = res.samples.cpu().numpy()
    assert np.isnan(got[~keep]).all() and not np.isnan(got[keep]).any()
    assert int(res.n_ignored) == int((~keep).sum()) and np.array_equal(res.counts.cpu().numpy(), np.bincount(out[keep], minlength=K))
    _check_summary(res, out, K)
    alone = silhouette_samples(_dev(X[keep]), _dev(out[keep]), K)
    assert int(alone.n_ignored) == 0
    assert np.abs(got[keep] - alone.samples.cpu().numpy()).max() <= 1e-12
    assert abs(float(res.score) - float(alone.score)) <= 1e-12
    for a, b in zip(cluster_moments(Xd, _dev(out), K), cluster_moments(_dev(X[keep]), _dev(out[keep]), K)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.abs(np.nan_to_num(a - b)).max() <= 1e-12 * max(1.0, np.nanmax(np.abs(b)))
    # int64 labels with values beyond int32, and a single cluster: no score
    far = torch.where(_dev(keep), _dev(out), torch.full((n,), 2 ** 40, dtype=torch.int64, device='cuda'))
    assert torch.equal(_bits(silhouette_samples(Xd, far, K).samples), _bits(res.samples))
    one = silhouette_samples(Xd, _dev(np.where(lab == 1, 1, -1)), K)
    assert bool(torch.isnan(one.score)) and int(one.n_ignored) == int((lab != 1).sum())


@pytest.mark.parametrize('n,F', [(8209, 24), (515, 700)])
def test_result_does_not_depend_on_the_split_and_repeats(n, F):
    from eagcn_amd.analysis import silhouette_samples, silhouette_slabs
    k = 18
    X, _ = R.clusters(n, n, F, n_dup=5)
    lab = np.random.RandomState(n).randint(0, k, n)           # 18 classes, interleaved rows
    Xd, ld = _dev(X), _dev(lab)
    assert len({silhouette_slabs(n, k, s) for s in (1, 2, 3, 7, 0)}) == 5
    runs = {s: silhouette_samples(Xd, ld, k, slabs=s) for s in (1, 2, 3, 7, 0)}
    for s, r in runs.items():
        again = silhouette_samples(Xd, ld, k, slabs=s)
        assert torch.equal(_bits(again.samples), _bits(r.samples)) and torch.equal(_bits(again.score), _bits(r.score))
        assert torch.equal(_bits(again.cluster_means), _bits(r.cluster_means))
        assert float((r.samples - runs[1].samples).abs().max()) <= 1e-12
        assert torch.equal(r.counts, runs[1].counts)
    from eagcn_amd.analysis import sqdist
    pinned, cnt = R.silhouette_from_distances(np.sqrt(sqdist(Xd).cpu().numpy()).astype(np.float64), lab, k)
    got = runs[0].samples.cpu().numpy()
    assert np.array_equal(runs[0].counts.cpu().numpy(), cnt) and np.abs(got - pinned).max() <= 1e-12
    if n <= 1027:                                              # (the fp64 distances of the larger case would take this test's time alone)
        assert np.abs(got - R.silhouette_samples(X, lab, k)[0]).max() <= R.margin(F) + 2.0 ** -22
    _check_summary(runs[0], lab, k)


@pytest.mark.parametrize('n,F', [(257, 7), (1027, 700), (8209, 24)])
def test_moments_and_indices_against_the_yardstick(n, F):
    from eagcn_amd.analysis import calinski_harabasz_score, cluster_moments, davies_bouldin_score
    X, lab = R.clusters(n * 1000 + F, n, F, n_dup=5)
    lab = R.remap9(lab, n)
    Xd = _wide(_dev(X)) if n == 257 else _dev(X)
    m = cluster_moments(Xd, _dev(lab), K)
    cen, sc, wss, cnt = R.moments(X, lab, K)
    assert m.centers.dtype == m.scatter.dtype == m.wss.dtype == torch.float64 and m.counts.dtype == torch.int64
    assert np.array_equal(m.counts.cpu().numpy(), cnt) and cnt[6] == 0 and cnt[7] == 1
    got = m.centers.cpu().numpy()
    assert np.isnan(got[6]).all() and not np.isnan(np.delete(got, 6, axis=0)).any()
    assert np.abs(np.nan_to_num(got - cen)).max() <= 1e-12 * np.nanmax(np.abs(cen))
    gs, gw = m.scatter.cpu().numpy(), m.wss.cpu().numpy()
    assert np.isnan(gs[6]) and gw[6] == 0.0 and gs[7] == 0.0 == gw[7]
    assert np.abs(np.nan_to_num(gs - sc)).max() <= 1e-12 * np.nanmax(sc) and np.abs(gw - wss).max() <= 1e-12 * wss.max()
    db, ch = davies_bouldin_score(Xd, _dev(lab), K), calinski_harabasz_score(Xd, _dev(lab), K)
    want_db, want_ch = R.davies_bouldin(cen, sc, cnt), R.calinski_harabasz(cen, wss, cnt)
    print('n=%d F=%d: DB %.12f (yardstick %.12f), CH %.9f (yardstick %.9f)' % (n, F, db, want_db, ch, want_ch))
    assert isinstance(db, float) and abs(db - want_db) <= 1e-10 * max(1.0, want_db)
    assert isinstance(ch, float) and abs(ch - want_ch) <= 1e-10 * max(1.0, want_ch)


def test_kmeans_end_to_end_and_errors():
    from sklearn import metrics
    from eagcn_amd.analysis import adjusted_rand_score, confusion_matrix, kmeans, normalized_mutual_info_score, purity, silhouette_score
    n, F = 1027, 24
    X, true = R.clusters(5, n, F, n_dup=5)
    Xd = _dev(X)
    g = torch.Generator(device='cuda')
    g.manual_seed(3)
    km = kmeans(Xd, 6, generator=g)
    lab = km.labels.cpu().numpy()
    score = silhouette_score(Xd, km.labels, 6)
    want, _ = R.silhouette_samples(X, lab, 6)
    print('silhouette of the k-means labels %.9f (yardstick %.9f)' % (score, want.mean()))
    assert isinstance(score, float) and abs(score - want.mean()) <= R.margin(F) + 2.0 ** -22
    cm = confusion_matrix(_dev(true), km.labels, 6, 6)
    assert abs(adjusted_rand_score(cm) - metrics.adjusted_rand_score(true, lab)) <= 1e-12
    assert abs(normalized_mutual_info_score(cm) - metrics.normalized_mutual_info_score(true, lab)) <= 1e-10
    assert abs(purity(cm) - R.purity(R.contingency(true, lab, 6, 6))) <= 1e-15
    sub = _dev(np.random.RandomState(0).randint(0, 18, n))    # the sub-type labels' 18 classes are inside the envelope (k-means stops at 16)
    assert -1.0 <= silhouette_score(Xd, sub, 18) <= 1.0
    with pytest.raises(ValueError, match='Number of labels is 1'):
        silhouette_score(Xd, torch.zeros(n, dtype=torch.int64, device='cuda'), 6)
    with pytest.raises(ValueError, match='Number of labels is 17'):
        silhouette_score(Xd[:17], torch.arange(17, device='cuda'), 17)
    from eagcn_amd._lib import EagcnHipError
    with pytest.raises(EagcnHipError, match='k = 257 is not in 2 .. 256'):
        silhouette_score(Xd, km.labels, 257)
    with pytest.raises(EagcnHipError, match='labels must be an integer device tensor'):
        silhouette_score(Xd, km.labels[:-1], 6)
