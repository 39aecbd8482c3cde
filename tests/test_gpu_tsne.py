"""The device t-SNE (csrc/embed.hip, eagcn_amd.analysis.tsne) against the fp64 yardstick of tsne_reference.py, which test_tsne_cpu.py
pins to scikit-learn: distances, affinities, the gradient pass alone, the update rule, a short trajectory, the schedule and stop
rule, whole fits against scikit-learn's, and the path from a model's dump to an embedding.

Row counts straddle the 64-row tile of the distance / joint-probability kernels (EM_TILE), the 8 rows a workgroup of the gradient pass
owns (TS_ROWS) and the 1024 columns it walks at a time (TS_CHUNK = 4 x 256 threads); every bound below is derived in its test."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import tsne_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'eagcn_amd', 'csrc', 'embed.hip')).read()
T = int(re.search(r'constexpr int EM_TILE = (\d+);', _SRC).group(1))
TS_ROWS = int(re.search(r'constexpr int TS_ROWS = (\d+);', _SRC).group(1))
NS = sorted({17, 63, 64, 65, T - 1, T, T + 1, 255, 257, 513, 1027})
U24 = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _an():
    from eagcn_amd import analysis
    return analysis


# ---- distances ---------------------------------------------------------------------------------------------------------------------

def _d64_torch(X):
    """fp64 direct sums of squared differences with torch ops on the device, 64 rows at a time: the reference where the numpy
    yardstick would take many seconds (it is held to the yardstick on the small shapes)"""
    X64 = _dev(X).double()
    return torch.cat([(X64[i:i + 64, None, :] - X64[None, :, :]).pow(2).sum(-1) for i in range(0, X64.shape[0], 64)]).cpu().numpy()


def _check_dist(D, X, tag):
    n, F = X.shape
    if n <= 65:
        D64 = R.sqdist(X)
        assert np.all(np.abs(_d64_torch(X) - D64) <= 1e-13 * D64), tag
    else:
        D64 = _d64_torch(X)
    got = D.cpu().numpy()
    err = np.abs(got.astype(np.float64) - D64)
    worst = (err / np.where(D64 > 0, D64, 1.0)).max()
    print('%s: worst |D - D64| / D64 = %.2e (bound %.2e)' % (tag, worst, (F + 2) * U24))
    assert np.all(err <= (F + 2) * U24 * D64), tag
    assert not got.diagonal().any(), tag
    assert np.array_equal(got, got.T), tag


@pytest.mark.parametrize('F', [1, 3, 24, 255, 256, 700, 1021, 1024])
def test_distances(F):
    """|D - D64| <= (F + 2) 2^-24 D64: an fp32 sum of F non-negative terms in any order is off by at most (F - 1) roundings of the
    sum and three inside a term (difference, square, the fused add counts with the sum).  D64 is the numpy yardstick up to n = 65
    and the same direct fp64 sum written with torch ops beyond (the yardstick takes 11 s at 1027 x 1024)."""
    for n in NS:
        X = R.make_data(n % 7, n, F)
        _check_dist(_an().sqdist(_dev(X)), X, 'n=%d F=%d' % (n, F))


@pytest.mark.parametrize('n,F', [(65, 24), (257, 700), (131, 5)])
def test_distances_of_strided_rows(n, F):
    X = R.make_data(1, n, F)
    wide = torch.full((n, F + 3), 7.0e5, device='cuda')       # what lies between the rows must never be read into a sum
    wide[:, :F] = _dev(X)
    view = wide[:, :F]
    assert view.stride(0) == F + 3 and not view.is_contiguous()
    D = _an().sqdist(view)
    _check_dist(D, X, 'ld=F+3 n=%d F=%d' % (n, F))
    assert torch.equal(D, _an().sqdist(_dev(X)))


# ---- affinities ------------------------------------------------------------------------------------------------------------------

def _check_affinities(n, found, perp, tag):
    seed, X, D, c, P = found
    p = _an()._TSNEProblem(n, 'cuda')
    p.affinities(_dev(D), perp)
    steps, betas, got = p.steps.cpu().numpy(), p.betas.cpu().numpy(), p.P.cpu().numpy()
    assert np.array_equal(steps, c['steps']), tag             # the certified margin keeps the fp64 search on the same step
    berr = (np.abs(betas - c['betas']) / c['betas']).max()
    perr = np.abs(got[:, :n].astype(np.float64) - P)
    print('%s seed %d: steps %d..%d, beta rel err %.2e, P worst rel err %.2e, margin %.2e'
          % (tag, seed, steps.min(), steps.max(), berr, (perr / np.maximum(P, R.EPS)).max(), c['margin'].min()))
    assert berr <= 1e-12, tag
    assert np.all(perr <= np.maximum(2.0 ** -23 * P, R.EPS)), tag          # fp32 storage of an fp64 result
    assert not got[:, n:].any() and not got[:, :n].diagonal().any() and np.array_equal(got[:, :n], got[:, :n].T), tag
    return c


@pytest.mark.parametrize('perp', [5.0, 30.0])
def test_affinities(perp):
    for n in NS:
        pp = n / 4.0 if (n == 17 and perp == 30.0) else perp
        found = R.find_seed(n, 24, pp)
        assert found is not None, 'no certified seed for n=%d perplexity=%g' % (n, pp)
        _check_affinities(n, found, pp, 'n=%d perplexity=%g' % (n, pp))


def test_affinities_with_an_outlier_row():
    """row 0 lies 40 units away in every coordinate: its row sum underflows to zero at beta = 1 (the 1e-8 branch)"""
    found = R.find_seed(257, 24, 30.0, outlier=True)
    assert found is not None
    c = _check_affinities(257, found, 30.0, 'outlier')
    assert c['zero_rows'][0]


def test_affinities_with_duplicate_rows():
    found = R.find_seed(129, 24, 5.0, duplicates=3)
    assert found is not None and (found[2] == 0).sum() == 129 + 6
    _check_affinities(129, found, 5.0, 'duplicates')


# ---- the gradient pass alone -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trajectory(n):
    """certified input, its joint P rounded to fp32 (the matrix the device holds) and the yardstick's fp64 trajectory on it"""
    seed, X, D, c, P = R.find_seed(n, 24, 30.0)
    P32 = P.astype(np.float32)
    Y0 = (np.random.RandomState(7).randn(n, 2) * 1e-4).astype(np.float32)
    lr = max(n / 12.0 / 4.0, 50.0)
    run = R.descend(P32, Y0, lr, max_iter=301, record=(0, 20, 300))
    return X, P32, Y0, lr, run


def _check_gradient(P32, Y, alpha, tag):
    n = P32.shape[0]
    Y32 = np.asarray(Y, dtype=np.float32)
    want = R.objective(P32, Y32, alpha)
    p = _an()._TSNEProblem(n, 'cuda')
    p.set_P(_dev(P32))
    grad, out = p.gradient(_dev(Y32), alpha)
    grad, (Z, kl, gnorm) = grad.cpu().numpy().astype(np.float64), out.tolist()
    err = np.abs(grad - want['grad'])
    bound = (n + 16) * U24 * want['bound']
    print('%s: worst err / bound %.3f, Z rel %.2e, KL %.9g / %.9g rel %.2e' % (tag, (err / bound).max(), abs(Z - want['Z']) / want['Z'],
                                                                              kl, want['kl'], abs(kl - want['kl']) / abs(want['kl'])))
    assert np.all(err <= bound), tag
    assert abs(Z - want['Z']) <= 1e-5 * want['Z'], tag
    assert abs(kl - want['kl']) <= 1e-5 * abs(want['kl']), tag
    assert abs(gnorm - np.sqrt((grad ** 2).sum())) <= 1e-12 * gnorm, tag
    return p


@pytest.mark.parametrize('alpha', [1.0, 12.0])
@pytest.mark.parametrize('n', [200, 513])
def test_gradient_pass(n, alpha):
    """|grad - grad64| <= (n + 16) 2^-24 A_i per component, A_i = 4 sum_j (|alpha P_ij| + |Q_ij|) w_ij |y_i - y_j|: the worst case of an
    fp32 sum of n signed terms plus the roundings inside a term; Z and KL to 1e-5 relative.  Y from the yardstick's trajectory at
    iterations 0 (tiny), 20 (expanding) and 300 (spread)."""
    X, P32, Y0, lr, run = _trajectory(n)
    for it in (0, 20, 300):
        _check_gradient(P32, run['trajectory'][it][0], alpha, 'n=%d alpha=%g it=%d' % (n, alpha, it))


def test_gradient_pass_over_many_workgroups():
    """n = 4099: 513 workgroups, five column chunks, the last of three columns; P any symmetric non-negative matrix of sum 1"""
    n = 4099
    assert n % TS_ROWS and n % 4                              # a short last workgroup, rows that are not 16-byte multiples
    rs = np.random.RandomState(3)
    P = rs.rand(n, n) ** 8
    P = P + P.T
    np.fill_diagonal(P, 0.0)
    P32 = (P / P.sum()).astype(np.float32)
    Y = rs.randn(n, 2) * 3.0
    for alpha in (1.0, 12.0):
        _check_gradient(P32, Y, alpha, 'n=%d alpha=%g' % (n, alpha))


# ---- update, trajectory, schedule --------------------------------------------------------------------------------------------------

def test_update_rule():
    """Four driver iterations; before each, the device's own gradient at the current state (the stand-alone pass: the same kernels) goes
    through the yardstick's fp32 update.  Y, update and gains agree to 4 x 2^-24 of the largest magnitude; gains exactly wherever
    |update grad| is not subnormal.  From the second iteration on both branches of the gains are taken."""
    n = 200
    X, P32, Y0, lr, run = _trajectory(n)
    Y20, U20, G20 = run['trajectory'][20]
    an = _an()
    p = an._TSNEProblem(n, 'cuda')
    p.set_P(_dev(P32))
    p.begin(_dev(Y20.astype(np.float32)), 12.0, lr, 1000, 300, 1e-7)
    g = an._TSNEProblem(n, 'cuda')
    g.set_P(_dev(P32))
    seen = set()
    for step in range(4):
        Y, U, G = (t.cpu().numpy().copy() for t in (p.Y, p.U, p.gains))
        grad = g.gradient(p.Y.clone(), 12.0, compute_kl=False)[0].cpu().numpy()
        wy, wu, wg, _ = R.update(Y, U, G, grad, 0.5, lr, np.float32)
        p.iterate()
        gy, gu, gg = (t.cpu().numpy() for t in (p.Y, p.U, p.gains))
        for name, got, want in (('Y', gy, wy), ('update', gu, wu), ('gains', gg, wg)):
            err = np.abs(got.astype(np.float64) - want).max()
            print('step %d %s: max err %.2e of max %.2e' % (step, name, err, np.abs(want).max()))
            assert err <= 4 * U24 * np.abs(want).max(), (step, name)
        normal = np.abs(U.astype(np.float64) * grad) >= np.finfo(np.float32).tiny
        assert np.array_equal(gg[normal], wg[normal]), step
        seen |= set(np.unique((U * grad < 0)[normal]).tolist())
    assert seen == {True, False}
    assert p.state_i.tolist()[:2] == [0, 4]


@pytest.mark.parametrize('n', [200, 513])
def test_short_trajectory(n):
    """Five iterations from a fixed init against the fp64 yardstick.  The tolerance is 10 x the deviation of the yardstick's own fp32 run
    from its fp64 run on the same input at iteration 5 (trajectories are chaotic: nothing is asserted later)."""
    X, P32, Y0, lr, run = _trajectory(n)
    y64 = R.descend(P32, Y0, lr, max_iter=5)['Y']
    y32 = R.descend(P32, Y0, lr, max_iter=5, dtype=np.float32)['Y']
    tol = 10.0 * np.abs(y32.astype(np.float64) - y64).max()
    p = _an()._TSNEProblem(n, 'cuda')
    p.set_P(_dev(P32))
    p.begin(_dev(Y0), 12.0, lr, 5, 300, 1e-7)
    for _ in range(5):
        p.iterate()
    err = np.abs(p.Y.cpu().numpy().astype(np.float64) - y64).max()
    print('n=%d: device - fp64 %.3e, yardstick fp32 - fp64 %.3e (tolerance %.3e), max|Y| %.3e' % (n, err, tol / 10, tol, np.abs(y64).max()))
    assert err <= tol
    assert p.state_i.tolist()[:3] == [1, 5, R.STOP_MAX_ITER]


@pytest.fixture(scope='module')
def blob():
    X = R.make_data(2, 300, 24)
    Y0 = (np.random.RandomState(5).randn(300, 2) * 1e-4).astype(np.float32)
    return _dev(X), _dev(Y0)


def _same(a, b):
    assert torch.equal(a.embedding, b.embedding) and a.kl_divergence == b.kl_divergence
    assert a.n_iter == b.n_iter and a.stop_reason == b.stop_reason


def test_result_does_not_depend_on_sync_every(blob):
    X, Y0 = blob
    runs = [_an().tsne(X, max_iter=120, init=Y0, sync_every=s) for s in (1, 7, 50, 120)]
    assert runs[0].n_iter == 120 and runs[0].stop_reason == 'max_iter'
    for r in runs[1:]:
        _same(runs[0], r)


def test_stop_at_the_first_check(blob):
    """a huge min_grad_norm stops the fit at the first check, iteration 50; the 70 iterations enqueued behind it change nothing"""
    X, Y0 = blob
    a = _an().tsne(X, max_iter=120, init=Y0, sync_every=50, min_grad_norm=1e30)
    b = _an().tsne(X, max_iter=120, init=Y0, sync_every=120, min_grad_norm=1e30)
    c = _an().tsne(X, max_iter=50, init=Y0, sync_every=50)
    assert a.n_iter == 50 and a.stop_reason == 'min_grad_norm'
    _same(a, b)
    assert torch.equal(a.embedding, c.embedding) and c.stop_reason == 'max_iter'


def test_two_runs_are_bit_identical(blob):
    X, Y0 = blob
    _same(_an().tsne(X, max_iter=300, init=Y0), _an().tsne(X, max_iter=300, init=Y0))
    gen = torch.Generator(device='cuda')
    runs = []
    for _ in range(2):
        gen.manual_seed(11)
        runs.append(_an().tsne(X, max_iter=60, init='random', generator=gen))
    _same(*runs)
    assert torch.equal(runs[0].P, runs[1].P) and torch.equal(runs[0].betas, runs[1].betas)
    pc = _an().tsne(X, max_iter=60, init='pca')
    assert pc.embedding.shape == (300, 2) and bool(torch.isfinite(pc.embedding).all())


def test_cpu_tensors_and_bad_arguments_raise():
    an = _an()
    from eagcn_amd._lib import EagcnHipError
    with pytest.raises(EagcnHipError, match='no CPU'):
        an.tsne(torch.zeros(100, 4))
    with pytest.raises(EagcnHipError, match='no CPU'):
        an.pca(torch.zeros(100, 4))
    with pytest.raises(EagcnHipError):
        an.tsne(torch.zeros(16, 4, device='cuda'))            # n below the envelope
    with pytest.raises(EagcnHipError):
        an.sqdist(torch.zeros(20, 1025, device='cuda'))       # F above it


# ---- whole fits ----------------------------------------------------------------------------------------------------------------------

def test_whole_fit_against_sklearn():
    """n = 300, F = 24, perplexity 30, random init, 500 iterations, five seeds each.  Every KL is recomputed by the yardstick against
    the same P; the device fits must have KL <= max_sk + 2 spread_sk and trustworthiness >= min_sk - 2 spread_sk, spread = max - min
    over scikit-learn's five fits."""
    from sklearn.manifold import TSNE, trustworthiness
    n = 300
    X = R.make_data(4, n, 24)
    _, _, P = R.affinities(X, 30.0)
    sk_kl, sk_tw = [], []
    for s in range(5):
        emb = TSNE(method='exact', max_iter=500, init='random', perplexity=30.0, random_state=s).fit_transform(X)
        sk_kl.append(R.objective(P, emb)['kl'])
        sk_tw.append(trustworthiness(X, emb, n_neighbors=10))
    kl_max, kl_spread, tw_min, tw_spread = max(sk_kl), max(sk_kl) - min(sk_kl), min(sk_tw), max(sk_tw) - min(sk_tw)
    print('scikit-learn: KL %.4f .. %.4f, trustworthiness %.4f .. %.4f' % (min(sk_kl), kl_max, tw_min, max(sk_tw)))
    gen = torch.Generator(device='cuda')
    Xd = _dev(X)
    for s in range(5):
        gen.manual_seed(100 + s)
        res = _an().tsne(Xd, perplexity=30.0, max_iter=500, init='random', generator=gen)
        emb = res.embedding.cpu().numpy().astype(np.float64)
        kl, tw = R.objective(P, emb)['kl'], trustworthiness(X, emb, n_neighbors=10)
        print('device seed %d: KL %.4f (reported %.4f), trustworthiness %.4f, n_iter %d' % (s, kl, res.kl_divergence, tw, res.n_iter))
        assert res.n_iter == 500 and res.stop_reason == 'max_iter'
        # the device's P comes from its own fp32 distances: (F + 2) 2^-24 = 1.5e-6 of D apart from the yardstick's, so exp(-beta D) moves
        # by up to beta D x 1.5e-6 <= 6e-5 where it matters (beta D <= 40) and the divergence, a sum of P log(P / Q) with |log| ~ 10,
        # by up to 6e-4 of a KL of 0.4 in the worst case
        assert abs(res.kl_divergence - kl) <= 1e-3 * kl
        assert kl <= kl_max + 2 * kl_spread
        assert tw >= tw_min - 2 * tw_spread


# ---- from the model ----------------------------------------------------------------------------------------------------------------

def test_from_a_models_dump_to_embeddings():
    from eagcn_amd import EAGCN
    from eagcn_amd.analysis import dump_atom_rep, subsample, tsne
    from eagcn_amd.synthetic import make_batch
    torch.manual_seed(4)
    model = EAGCN(28, 24, n_den1=16, n_den2=8, nclass=2, dropout=0.0, structure='Concate', n_layers=2, widths1=[8, 6, 10, 7, 5],
                  widths2=[12, 10, 7, 9, 5]).cuda().eval()
    batches = []
    for j in range(4):
        mb = make_batch(B=8, n_max=20, n_med=7, rel_channels=(28, 4, 2, 2, 2), seed=41 + j, isolated_frac=0.25, n_tasks=2)
        subtype = torch.from_numpy(np.random.RandomState(j).randint(0, 7, size=(8, mb.N)))
        batches.append((tuple(t.cuda() for t in mb.dense()), torch.from_numpy(mb.labels), subtype, torch.arange(8) + 8 * j))
    d = dump_atom_rep(model, batches, subtype_range=(1, 6)).finish()
    assert d.X.is_cuda and d.X.shape[0] > 200
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    classes, cap = [1, 2, 3, 5], 30
    idx = subsample(d.subtype, classes, cap, generator=gen)
    assert idx.is_cuda and idx.dtype == torch.int64
    picked = d.subtype[idx].cpu().numpy()
    counts = np.bincount(d.subtype.cpu().numpy(), minlength=8)
    assert (counts[classes] > cap).any() and len(set(idx.tolist())) == idx.numel()
    for c in range(8):
        assert (picked == c).sum() == (min(counts[c], cap) if c in classes else 0), c
    atoms = tsne(d.X[idx], perplexity=10.0, max_iter=100, generator=gen)
    assert atoms.embedding.is_cuda and atoms.embedding.shape == (idx.numel(), 2) and bool(torch.isfinite(atoms.embedding).all())
    assert atoms.n_iter == 100 and np.isfinite(atoms.kl_divergence)
    mols = tsne(d.graph_rep, perplexity=8.0, max_iter=100, init='random', generator=gen)
    assert mols.embedding.shape == (32, 2) and bool(torch.isfinite(mols.embedding).all()) and np.isfinite(mols.kl_divergence)
