"""The device nearest-neighbour search, the neighbour ranks and the trustworthiness (csrc/knn.hip, eagcn_amd.analysis) against
(a) analysis.sqdist, existing code with the same distance bits, sorted by torch: indices and distance BITS must be identical, and
(b) the fp64 yardstick of knn_reference.py, which test_knn_cpu.py pins to scikit-learn, within margin(F) = (F + 4) 2^-23, the
relative error bound of the fp32 distances (knn_reference.margin)."""
import functools

import numpy as np
import pytest
import torch

import knn_reference as R

pytestmark = pytest.mark.gpu

NS = (17, 63, 64, 65, 129, 257, 1027)
FS = (1, 3, 31, 32, 33, 700)
KS = (1, 5, 16, 17, 64, 128)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ks(n):
    return sorted(set(k for k in KS if k <= n - 1) | ({n - 1} if n - 1 <= 128 else set()))


def _wide(X, extra=3):
    """the rows of X inside a wider matrix (ld = F + extra) whose other columns hold large numbers"""
    wide = torch.full((X.shape[0], X.shape[1] + extra), 7.0e5, device='cuda')
    wide[:, :X.shape[1]] = X
    return wide[:, :X.shape[1]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sorted_rows(D):
    """(values, indices) of every row of the device matrix D without its diagonal entry, by (d, j)"""
    D = D.clone()
    D.fill_diagonal_(float('inf'))                             # removed by index: it sorts last and is cut off
    v, i = torch.sort(D, dim=1, stable=True)
    return v[:, :-1], i[:, :-1]


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('n', NS)
def test_self_join_equals_sorted_sqdist_to_the_bit(n, F):
    from eagcn_amd.analysis import knn, sqdist
    X, _ = R.clusters(n * 1000 + F, n, F, n_dup=5)
    Xd = _wide(_dev(X)) if (n + F) % 2 else _dev(X)
    v, i = _sorted_rows(sqdist(Xd))
    assert int((v[:, 0] == 0).sum()) >= 10                     # the duplicated rows are there
    for k in _ks(n):
        res = knn(Xd, k)
        assert res.indices.dtype == torch.int32 and res.indices.shape == res.distances.shape == (n, k)
        assert torch.equal(res.indices.long(), i[:, :k]), (n, F, k)
        assert torch.equal(_bits(res.distances), _bits(v[:, :k])), (n, F, k)


@pytest.mark.parametrize('n,F,k', [(8209, 24, 17), (515, 700, 128)])
def test_result_does_not_depend_on_the_split(n, F, k):
    from eagcn_amd.analysis import knn, knn_slabs
    X, _ = R.clusters(n, n, F, n_dup=5)
    Xd = _dev(X)
    runs = [knn(Xd, k, slabs=s) for s in (1, 2, 3, 7, 0, 0)]
    assert len({knn_slabs(n, n, s) for s in (1, 2, 3, 7)}) == 4
    for r in runs[1:]:
        assert torch.equal(r.indices, runs[0].indices) and torch.equal(_bits(r.distances), _bits(runs[0].distances))
    Q = _dev(R.gaussian(1, 70, F))                            # few queries: slabs = 0 splits the data rows
    assert knn_slabs(n, 70) > 1
    a, b, c = knn(Xd, k, queries=Q), knn(Xd, k, queries=Q, slabs=1), knn(Xd, k, queries=Q)
    for r in (b, c):
        assert torch.equal(r.indices, a.indices) and torch.equal(_bits(r.distances), _bits(a.distances))


def _check_against_fp64(idx, dist, D64, k, F, scale=1.0):
    """the four conditions on a device result (distances `dist` = scale x the squared distance) against the fp64 block D64"""
    mg = R.margin(F)
    o = R.order(D64)
    S = np.take_along_axis(D64, o, axis=1)[:, :k + 1] * scale  # the k + 1 least true distances of every query, sorted
    true = np.take_along_axis(D64, idx.astype(np.int64), axis=1) * scale
    err = np.abs(dist.astype(np.float64) - S[:, :k])
    print('F=%d k=%d: worst |dist - S64| / S64 = %.3e (margin %.3e)' % (F, k, float((err / np.maximum(S[:, :k], 1e-300)).max()), mg))
    assert np.all(err <= mg * S[:, :k])
    assert np.all(true <= S[:, k - 1:k] * (1 + 2 * mg))
    must = D64 * scale < S[:, k - 1:k] * (1 - 2 * mg)
    have = np.zeros_like(must)
    np.put_along_axis(have, idx.astype(np.int64), True, axis=1)
    assert have.sum() == idx.size                              # k distinct rows per query
    assert not np.any(must & ~have)
    up = (S[:, 1:] - S[:, :-1]) > 2 * mg * S[:, 1:]            # [m, k]: the gap above position p
    clear = up.copy()
    clear[:, 1:] &= up[:, :-1]
    print('    positions with clear gaps on both sides: %.1f %%' % (100.0 * clear.mean()))
    assert np.array_equal(idx[clear], o[:, :k][clear])
    return clear.mean()


@pytest.mark.parametrize('F', [7, 700])
def test_queries_against_fp64(F):
    from eagcn_amd.analysis import knn
    n, m, k = 20011, 256, 16
    X, Q = R.gaussian(F, n, F), R.gaussian(F + 1, m, F)
    res = knn(_dev(X), k, queries=_dev(Q))
    share = _check_against_fp64(res.indices.cpu().numpy(), res.distances.cpu().numpy(), R.sqdist64(Q, X, gram=True), k, F)
    assert share > (0.99 if F == 7 else 0.75)                  # (the last condition is about most positions: a property of the fp64 data)


def test_exclude_self_and_edges():
    from eagcn_amd.analysis import knn
    n, F = 17, 5
    X, _ = R.clusters(0, n, F, n_dup=3)
    Xd = _dev(X)
    D = R.sqdist64(X, X)
    own = knn(Xd, 3, exclude_self=False)
    first = R.order(D)[:, 0]                                   # the row itself, or its duplicate of lower index
    assert torch.equal(own.indices[:, 0].cpu().long(), torch.from_numpy(first)) and not own.distances[:, 0].any()
    assert int((first != np.arange(n)).sum()) == 3             # (the three copies see their original first)
    plain = _dev(R.gaussian(5, n, F))
    own = knn(plain, 1, exclude_self=False)
    assert torch.equal(own.indices[:, 0].cpu().long(), torch.arange(n)) and not own.distances.any()
    rest = knn(Xd, n - 1)                                      # k = n - 1: every other row
    assert torch.equal(torch.sort(rest.indices.long(), dim=1).values.cpu(),
                       torch.tensor([[j for j in range(n) if j != i] for i in range(n)]))
    both = knn(Xd, n, exclude_self=False)
    assert torch.equal(torch.sort(both.indices.long(), dim=1).values.cpu(), torch.arange(n).repeat(n, 1))
    one = knn(Xd, 4, queries=Xd[5:6])                          # m = 1
    assert one.indices.shape == (1, 4)
    assert torch.equal(one.indices, knn(Xd, 4, exclude_self=False).indices[5:6])
    from eagcn_amd._lib import EagcnHipError
    with pytest.raises(EagcnHipError, match='more than the 16 candidates'):
        knn(Xd, n)
    with pytest.raises(EagcnHipError, match='exclude_self needs m = n'):
        knn(Xd, 2, queries=Xd[:5], exclude_self=True)


def _ranks_from_sqdist(D, cand):
    """the ranks under (d, j) from the device matrix D, and -1 for candidates that are the row itself or no row"""
    n = D.shape[0]
    _, i = _sorted_rows(D)
    pos = torch.zeros((n, n), dtype=torch.int64, device=D.device)
    pos.scatter_(1, i, torch.arange(1, n, device=D.device).repeat(n, 1))
    c = cand.long()
    bad = (c < 0) | (c >= n) | (c == torch.arange(n, device=D.device).unsqueeze(1))
    return torch.where(bad, torch.full_like(c, -1), torch.gather(pos, 1, torch.where(bad, torch.zeros_like(c), c)))


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('n', NS)
def test_ranks_equal_sorted_sqdist(n, F):
    from eagcn_amd.analysis import neighbor_ranks, sqdist
    X, _ = R.clusters(n * 1000 + F, n, F, n_dup=5)
    Xd = _dev(X) if (n + F) % 2 else _wide(_dev(X))
    D = sqdist(Xd)
    rs = np.random.RandomState(n + F)
    dup = [int(np.nonzero((X == X[i]).all(axis=1))[0][-1]) for i in range(5)]      # the copies of the rows 0 .. 4
    assert all(j > 4 for j in dup)
    for k in KS:
        cand = rs.randint(0, n, (n, k))
        cand[:5, 0] = dup
        if k >= 5:
            cand[:, 1], cand[:, 2], cand[:, 3] = np.arange(n), -1, n
        cand_d = _dev(cand.astype(np.int32))
        got = neighbor_ranks(Xd, cand_d)
        assert got.dtype == torch.int32 and got.shape == (n, k)
        assert torch.equal(got.long(), _ranks_from_sqdist(D, cand_d)), (n, F, k)
        if k >= 5:
            assert bool((got[:, 1:4] == -1).all())
        for s in (1, 3):
            assert torch.equal(neighbor_ranks(Xd, cand_d, slabs=s), got)


@functools.lru_cache(maxsize=None)
def _dup_case():
    n, F = 1027, 700
    X, _ = R.clusters(11, n, F, n_dup=5)
    return X, R.sqdist64(X, X)


def test_ranks_against_fp64():
    """|rank - rank64| <= e_ij, the yardstick's count of the rows whose distance lies within margin(F) of d(i, j)"""
    from eagcn_amd.analysis import neighbor_ranks
    X, D = _dup_case()
    n, k = X.shape[0], 12
    rs = np.random.RandomState(5)
    cand = rs.randint(0, n, (n, k))
    cand[:, 0] = R.order(D, exclude_self=True)[:, 0]           # the nearest row (the duplicate, where there is one)
    cand = np.where(cand == np.arange(n)[:, None], (cand + 1) % n, cand)
    got = neighbor_ranks(_dev(X), _dev(cand.astype(np.int32))).cpu().numpy().astype(np.int64)
    want = R.ranks(D, cand)
    e = R.near_counts(D, cand, R.margin(X.shape[1]))
    print('ranks off at %d of %d candidates, worst %d; allowed sum %d' % ((got != want).sum(), got.size, np.abs(got - want).max(), e.sum()))
    assert np.all(np.abs(got - want) <= e)


@functools.lru_cache(maxsize=None)
def _embedding_case(n, F):
    found = R.find_seed(n, F, 12)
    assert found is not None, 'no seed with clear gaps in the embedding for n=%d F=%d' % (n, F)
    return found


@pytest.mark.parametrize('k', [5, 12])
@pytest.mark.parametrize('n,F', [(257, 7), (257, 700), (1027, 7), (1027, 700)])
def test_trustworthiness_against_sklearn(n, F, k):
    from sklearn.manifold import trustworthiness as sk_trust
    from eagcn_amd.analysis import continuity, knn, trustworthiness
    _, X, Y, DX, DY = _embedding_case(n, F)
    Xd, Yd = _dev(X), _dev(Y)
    want_t, nb, _ = R.trustworthiness(DX, DY, k)
    got_nb = knn(Yd, k).indices.cpu().numpy()
    assert np.array_equal(np.sort(got_nb, axis=1), np.sort(nb, axis=1))
    t_sk = sk_trust(X.astype(np.float64), Y.astype(np.float64), n_neighbors=k, metric='euclidean')
    t = trustworthiness(Xd, Yd, k)
    unit = 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
    bound = unit * R.near_counts(DX, nb, R.margin(F)).sum() + 1e-12
    print('n=%d F=%d k=%d: T = %.12f, sklearn %.12f, yardstick %.12f, bound %.3e' % (n, F, k, t, t_sk, want_t, bound))
    assert isinstance(t, float) and abs(t - t_sk) <= bound
    c = continuity(Xd, Yd, k)
    assert c == trustworthiness(Yd, Xd, k) and 0.0 < c <= 1.0


def test_trustworthiness_needs_k_below_half_the_rows():
    from eagcn_amd.analysis import continuity, trustworthiness
    X, Y = _dev(R.gaussian(0, 20, 4)), _dev(R.gaussian(1, 20, 2))
    for fn in (trustworthiness, continuity):
        with pytest.raises(ValueError, match='should be less than n_samples / 2'):
            fn(X, Y, 10)
        assert 0.0 < fn(X, Y, 9) <= 1.0


def test_metrics_and_agreement():
    from eagcn_amd.analysis import knn, neighbor_agreement
    n, m, F, k = 4099, 130, 7, 16
    X, lab = R.clusters(2, n, F, n_dup=0)
    Q = R.gaussian(3, m, F) * 3
    Xd, Qd = _dev(X), _dev(Q)
    sq, eu = knn(Xd, k, queries=Qd), knn(Xd, k, queries=Qd, metric='euclidean')
    assert torch.equal(eu.indices, sq.indices) and torch.equal(eu.distances, sq.distances.sqrt())
    # cosine: half the squared distance of the L2-normalised copies the call makes (torch, fp32) -- the yardstick runs on those copies
    Xn, Qn = Xd / Xd.norm(dim=1, keepdim=True), Qd / Qd.norm(dim=1, keepdim=True)
    assert float((Xn.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    co = knn(Xd, k, queries=Qd, metric='cosine')
    D64 = R.sqdist64(Qn.cpu().numpy(), Xn.cpu().numpy())
    _check_against_fp64(co.indices.cpu().numpy(), co.distances.cpu().numpy(), D64, k, F, scale=0.5)
    cos = 1.0 - (Qn.double() @ Xn.double().t()).gather(1, co.indices.long())
    assert float((co.distances.double() - cos).abs().max()) <= 1e-6
    own = knn(Xd, 5, metric='cosine')                          # a self-join on the copies
    assert own.indices.shape == (n, 5) and bool((own.indices.long() != torch.arange(n, device='cuda').unsqueeze(1)).all())
    nb = knn(Xd, 10).indices
    want = (lab[nb.cpu().numpy()] == lab[:, None]).mean(axis=1)
    got = neighbor_agreement(nb, _dev(lab))
    # (a share of ten neighbours: the two means may round count / 10 differently in the last place)
    assert got.dtype == torch.float64 and np.abs(got.cpu().numpy() - want).max() <= 2.0 ** -52
    assert want.mean() > 0.5                                   # rows of one cluster sit together
