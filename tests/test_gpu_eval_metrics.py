"""Evaluation metrics on the device (csrc/metrics.hip behind EvalBuffers.metrics()): per-task ROC-AUC, average precision, RMSE and
MAE over the device-resident evaluation buffers against sklearn / numpy fp64 on the same fp32 inputs.

Row counts sit around the tile of entries a workgroup owns (R) and the chunk of rows it stages at a time (J), as built.  Bounds:
sklearn's auc / average_precision_score accumulate at most `rows` fp64 terms of magnitude <= 1 (2307 * 2^-52 = 5e-13) and the
device AUC numerator is an exact integer, so both metrics are held to 1e-10 absolute; the regression sums have non-negative terms
(error <= rows * 2^-53) and are held to 1e-12 relative."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'eagcn_amd', 'csrc', 'metrics.hip')).read()
R = int(re.search(r'constexpr int EVAL_R = (\d+);', _SRC).group(1))
J = int(re.search(r'constexpr int EVAL_J = (\d+);', _SRC).group(1))
ROWS = [1, 2, R - 1, R, R + 1, J + 1, 2 * J + R + 3]
VARIANTS = ['plain', 'ties', 'equal', 'nopos', 'nolabel']


def make_class_case(rows, T, variant):
    """fp32 scores in [0, 1), labels in {1, 0, -1}: about 20 % positives, 15 % missing; (scores, labels, deliberate task or None)"""
    rng = np.random.RandomState(7919 * rows + 31 * T + VARIANTS.index(variant))
    s = rng.rand(rows, T).astype(np.float32)
    u = rng.rand(rows, T)
    y = np.where(u < 0.15, -1.0, np.where(u < 0.35, 1.0, 0.0)).astype(np.float32)
    k = None
    if variant == 'ties':
        s = (np.round(s * 5) / 5).astype(np.float32)
    elif variant == 'equal':
        s[:] = 0.5
    elif variant == 'nopos':
        k = T // 2
        y[:, k][y[:, k] == 1] = 0.0
    elif variant == 'nolabel':
        k = T // 2
        y[:, k] = -1.0
    return s, y, k


def sklearn_class(s, y):
    """per task over the labelled entries: (roc_curve + auc, average_precision_score, P, N); nan where a class is missing"""
    from sklearn import metrics
    T = s.shape[1]
    auc, ap, P, N = np.full(T, np.nan), np.full(T, np.nan), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    for t in range(T):
        m = y[:, t] != -1
        yt, st = y[m, t].astype(int), s[m, t]
        P[t], N[t] = int((yt == 1).sum()), int((yt == 0).sum())
        if P[t] and N[t]:
            fpr, tpr, _ = metrics.roc_curve(yt, st, pos_label=1)
            auc[t] = metrics.auc(fpr, tpr)
            ap[t] = metrics.average_precision_score(yt, st)
    return auc, ap, P, N


def nanmean(v):
    return float(np.mean(v[~np.isnan(v)])) if (~np.isnan(v)).any() else float('nan')


def fill(s, y, classification, cap=None):
    """EvalBuffers holding exactly these scores / targets (valid as eagcn_eval_append sets it), no model involved"""
    from eagcn_amd.training import EvalBuffers
    rows, T = s.shape
    buf = EvalBuffers(T, classification, torch.device('cuda'), cap=cap or max(rows, 1))
    buf.scores[:rows] = torch.from_numpy(s).cuda()
    buf.targets[:rows] = torch.from_numpy(y).cuda()
    buf.valid[:rows] = torch.from_numpy(((y == 0) | (y == 1)) if classification else np.ones_like(y, dtype=bool)).cuda().to(torch.uint8)
    buf.rows = rows
    return buf


def words(t):
    return t.view(torch.int64).cpu()


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('T', [1, 3, 12])
@pytest.mark.parametrize('rows', ROWS)
def test_classification_metrics_match_sklearn(rows, T, variant):
    s, y, k = make_class_case(rows, T, variant)
    auc_w, ap_w, P_w, N_w = sklearn_class(s, y)
    if rows > 2:                                            # no case passes by nan == nan
        for t in range(T):
            assert t == k or (P_w[t] > 0 and N_w[t] > 0), (t, P_w[t], N_w[t])
    if k is not None:
        assert math.isnan(auc_w[k])
    res = fill(s, y, True).metrics()
    assert res.kind == 'class' and res.T == T and res.values.dtype == torch.float64 and res.values.shape == (5 * T + 2,)
    v = res.values.cpu().numpy()
    auc, ap = v[:T], v[T:2 * T]
    ok = ~np.isnan(auc_w)
    print('rows %d T %d %s: max |auc - sklearn| %.2e, max |ap - sklearn| %.2e' % (
        rows, T, variant, np.abs(auc[ok] - auc_w[ok]).max(initial=0.0), np.abs(ap[ok] - ap_w[ok]).max(initial=0.0)))
    assert (v[2 * T:3 * T] == P_w).all() and (v[3 * T:4 * T] == N_w).all() and (v[4 * T:5 * T] == 0).all()
    assert (np.isnan(auc) == np.isnan(auc_w)).all() and (np.isnan(ap) == np.isnan(ap_w)).all()
    assert (np.abs(auc[ok] - auc_w[ok]) <= 1e-10).all(), (auc, auc_w)
    assert (np.abs(ap[ok] - ap_w[ok]) <= 1e-10).all(), (ap, ap_w)
    for got, want in ((v[5 * T], nanmean(auc_w)), (v[5 * T + 1], nanmean(ap_w))):
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-10, (got, want)
    # the accessors read the same vector
    assert res.n_pos == list(P_w) and res.n_neg == list(N_w)
    np.testing.assert_array_equal(np.array(res.auc), auc)
    np.testing.assert_array_equal(np.array(res.ap), ap)
    aucs, mean = res.as_reference()
    np.testing.assert_array_equal(np.array(aucs), auc)
    np.testing.assert_array_equal(np.array([mean, res.mean_auc, res.mean_ap]), v[[5 * T, 5 * T, 5 * T + 1]])
    if variant == 'equal' and rows > 2:
        assert (auc == 0.5).all()


@pytest.mark.parametrize('rows, T', [(2 * J + R + 3, 60), (R + 1, 300)])
def test_many_tasks_take_the_unsplit_paths(rows, T):
    """Beyond the task counts above: 60 tasks of three chunks each, walked by one workgroup per tile (more tiles than CUs: nothing is
    split); more tasks than a workgroup has lanes (a lane's staging step never leaves its row)."""
    s, y, _ = make_class_case(rows, T, 'ties')
    auc_w, ap_w, P_w, N_w = sklearn_class(s, y)
    assert (P_w > 0).all() and (N_w > 0).all()
    v = fill(s, y, True).metrics().values.cpu().numpy()
    print('rows %d T %d: max |auc - sklearn| %.2e, max |ap - sklearn| %.2e' % (rows, T, np.abs(v[:T] - auc_w).max(), np.abs(v[T:2 * T] - ap_w).max()))
    assert (v[2 * T:3 * T] == P_w).all() and (v[3 * T:4 * T] == N_w).all() and (v[4 * T:5 * T] == 0).all()
    assert np.abs(v[:T] - auc_w).max() <= 1e-10 and np.abs(v[T:2 * T] - ap_w).max() <= 1e-10
    assert abs(v[5 * T] - auc_w.mean()) <= 1e-10 and abs(v[5 * T + 1] - ap_w.mean()) <= 1e-10


def test_signed_zeros_and_subnormal_gaps():
    """Whatever arithmetic the pair loop counts with (compares today; a form on the sign bits of differences was tried): scores one
    subnormal step apart are different scores, -0 and +0 are the same one (as for sklearn), neighbouring large scores stay apart."""
    rows, T = R + 1, 3
    rng = np.random.RandomState(17)
    tiny, big = np.float32(1e-45), np.float32(1e30)            # (larger ones overflow the sums of sklearn's input checks)
    pool = np.array([0.0, -0.0, tiny, -tiny, 2 * tiny, np.finfo(np.float32).tiny, np.finfo(np.float32).tiny - tiny, big, -big,
                     np.nextafter(big, np.float32(0))], dtype=np.float32)
    s = pool[rng.randint(0, len(pool), size=(rows, T))]
    u = rng.rand(rows, T)
    y = np.where(u < 0.15, -1.0, np.where(u < 0.5, 1.0, 0.0)).astype(np.float32)
    auc_w, ap_w, P_w, N_w = sklearn_class(s, y)
    assert (P_w > 0).all() and (N_w > 0).all()
    v = fill(s, y, True).metrics().values.cpu().numpy()
    print('max |auc - sklearn| %.2e, max |ap - sklearn| %.2e' % (np.abs(v[:T] - auc_w).max(), np.abs(v[T:2 * T] - ap_w).max()))
    assert (v[2 * T:3 * T] == P_w).all() and (v[3 * T:4 * T] == N_w).all() and (v[4 * T:5 * T] == 0).all()
    assert np.abs(v[:T] - auc_w).max() <= 1e-10 and np.abs(v[T:2 * T] - ap_w).max() <= 1e-10


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('rows', ROWS)
def test_regression_metrics_match_numpy(rows, T):
    from sklearn import metrics
    rng = np.random.RandomState(104729 * T + rows)
    s, y = rng.randn(rows, T).astype(np.float32), rng.randn(rows, T).astype(np.float32)
    res = fill(s, y, False).metrics()
    assert res.kind == 'reg' and res.values.shape == (3 * T + 2,)
    v = res.values.cpu().numpy()
    d = s.astype(np.float64) - y.astype(np.float64)
    want = np.concatenate([np.sqrt((d * d).mean(0)), np.abs(d).mean(0), np.full(T, float(rows)),
                           [math.sqrt(metrics.mean_squared_error(y.astype(np.float64).ravel(), s.astype(np.float64).ravel())), np.abs(d).mean()]])
    rel = np.abs(v - want) / np.abs(want)
    print('rows %d T %d: max relative error %.2e' % (rows, T, rel.max()))
    assert (v[2 * T:3 * T] == rows).all()
    assert (rel <= 1e-12).all(), (v, want)
    assert res.per_task_rmse == list(v[:T]) and res.per_task_mae == list(v[T:2 * T]) and res.count == [rows] * T
    assert res.rmse == v[3 * T] == res.as_reference() and res.mae == v[3 * T + 1]
    from eagcn_amd import _lib
    with pytest.raises(_lib.EagcnHipError):
        res.auc


@pytest.fixture(scope='module', params=[1, 3])
def big_case(request):
    """the largest shape with heavy ties, ten tiles with a partial last tile and chunk.  One task: three workgroups share a tile's rows
    and the finalize forms the ratios from their per-entry counts; three tasks: a workgroup walks all three chunks itself."""
    s, y, _ = make_class_case(2 * J + R + 3, request.param, 'ties')
    return s, y


def test_row_order_does_not_move_the_auc(big_case):
    s, y = big_case
    v0 = fill(s, y, True).metrics().values
    perm = np.random.RandomState(5).permutation(s.shape[0])
    v1 = fill(s[perm], y[perm], True).metrics().values
    T = s.shape[1]
    assert torch.equal(words(v0[:T]), words(v1[:T])) and torch.equal(words(v0[2 * T:5 * T + 1]), words(v1[2 * T:5 * T + 1]))
    assert (v0[T:2 * T] - v1[T:2 * T]).abs().max().item() <= 1e-12 and abs((v0[-1] - v1[-1]).item()) <= 1e-12


def test_two_calls_are_bit_identical(big_case):
    s, y = big_case
    buf = fill(s, y, True)
    assert torch.equal(words(buf.metrics().values), words(buf.metrics().values))
    rng = np.random.RandomState(11)
    reg = fill(rng.randn(2 * J + R + 3, 3).astype(np.float32), rng.randn(2 * J + R + 3, 3).astype(np.float32), False)
    assert torch.equal(words(reg.metrics().values), words(reg.metrics().values))


@pytest.mark.parametrize('classification', [True, False])
def test_poisoned_workspace_gives_the_same_words(big_case, classification):
    """through the C ABI: the kernels write every workspace word the finalize reads, so the workspace needs no clear"""
    from eagcn_amd import _lib
    lib = _lib.load()
    s, y = big_case
    buf = fill(s, y, classification)
    rows, T = s.shape
    nbytes = lib.eagcn_eval_metrics_workspace_bytes(rows, T)
    fn = lib.eagcn_eval_class_metrics if classification else lib.eagcn_eval_reg_metrics
    outs = []
    for byte in (0x00, 0xFF):
        ws = torch.full((nbytes,), byte, dtype=torch.uint8, device='cuda')
        out = torch.full(((5 if classification else 3) * T + 2,), -7.0, dtype=torch.float64, device='cuda')
        _lib.check(fn(buf.scores.data_ptr(), buf.targets.data_ptr(), buf.valid.data_ptr(), rows, T, ws.data_ptr(), nbytes, out.data_ptr(),
                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'metrics')
        outs.append(words(out))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], words(buf.metrics().values))


def test_device_auc_equals_auc_per_task(big_case):
    from eagcn_amd import training
    for s, y in (big_case, make_class_case(R + 1, 12, 'nopos')[:2]):
        buf = fill(s, y, True)
        aucs, mean = training.auc_per_task(*buf.views())
        got, got_mean = buf.metrics().as_reference()
        for a, b in zip(aucs + [mean], got + [got_mean]):
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (aucs, got)


def test_nan_score_is_counted_and_raises():
    from eagcn_amd import _lib
    s, y, _ = make_class_case(R + 1, 3, 'plain')
    y[R, 1] = 1.0                                            # a labelled entry, in the second tile
    s[R, 1] = np.nan
    s[3, 2] = np.nan                                         # ... and an unlabelled one, which does not count
    y[3, 2] = -1.0
    res = fill(s, y, True).metrics()
    v = res.values.cpu().numpy()
    assert list(v[4 * 3:5 * 3]) == [0.0, 1.0, 0.0]
    assert math.isnan(v[1]) and math.isnan(v[3 + 1])
    assert np.isfinite(v[[0, 2, 3, 5]]).all() and np.isfinite(v[15:]).all()
    auc_w, ap_w, _, _ = sklearn_class(s[:, [0, 2]], y[:, [0, 2]])
    assert np.abs(v[[0, 2]] - auc_w).max() <= 1e-10 and np.abs(v[[3, 5]] - ap_w).max() <= 1e-10
    assert abs(v[15] - auc_w.mean()) <= 1e-10 and abs(v[16] - ap_w.mean()) <= 1e-10
    for name in ('auc', 'ap', 'mean_auc', 'mean_ap', 'as_reference'):
        with pytest.raises(_lib.EagcnHipError, match=r'task 1 has 1 labelled'):
            getattr(res, name)() if name == 'as_reference' else getattr(res, name)


def test_workspace_regrows_with_the_buffers():
    """appended batches (eagcn_eval_append: sigmoid of the logits) that outgrow cap = 64 once; metrics before and after"""
    from eagcn_amd.training import EvalBuffers
    rng = np.random.RandomState(3)
    logits = rng.randn(96, 3).astype(np.float32)
    y = rng.choice(np.array([0.0, 1.0, -1.0], dtype=np.float32), size=(96, 3), p=[0.6, 0.25, 0.15])
    buf = EvalBuffers(3, True, torch.device('cuda'), cap=64)
    for i in range(2):
        buf.append(torch.from_numpy(logits[32 * i:32 * i + 32]).cuda(), torch.from_numpy(y[32 * i:32 * i + 32]).cuda())
    first = buf.metrics()
    ws = buf._workspace
    buf.append(torch.from_numpy(logits[64:]).cuda(), torch.from_numpy(y[64:]).cuda())
    assert buf.cap == 128 and buf.rows == 96 and buf._workspace is None
    second = buf.metrics()
    assert buf._workspace is not None and buf._workspace is not ws
    for res, n in ((first, 64), (second, 96)):
        want = sklearn_class(buf.scores[:n].cpu().numpy(), y[:n])
        assert np.abs(np.array(res.auc) - want[0]).max() <= 1e-10 and np.abs(np.array(res.ap) - want[1]).max() <= 1e-10


@pytest.mark.parametrize('task', ['class', 'reg'])
def test_evaluate_with_device_metrics_equals_the_default_path(task, monkeypatch):
    import functools
    from eagcn_amd import Concate_GCN, training
    from eagcn_amd.synthetic import make_batch
    torch.manual_seed(4)
    model = Concate_GCN(7, 24, *[8, 6, 4, 4, 5], *[10, 7, 5, 6, 4], 16, 8, 3, 0.3, n_layers=2, graph=True).cuda().train()
    mbs = [make_batch(B=32, n_max=20, n_med=8, rel_channels=(7, 4, 2, 2, 2), seed=200 + i, n_tasks=3, task=task) for i in range(3)]
    batches = [(tuple(t.cuda() for t in mb.dense()), torch.from_numpy(mb.labels).cuda()) for mb in mbs]
    grown = []
    real_alloc = training.EvalBuffers._alloc
    monkeypatch.setattr(training.EvalBuffers, '_alloc', lambda self, cap: (grown.append(cap), real_alloc(self, cap))[1])
    monkeypatch.setattr(training, 'EvalBuffers', functools.partial(training.EvalBuffers, cap=64))
    want = training.evaluate(model, batches, task, 3)
    assert model.training and grown == [64, 128]
    res = training.evaluate(model, batches, task, 3, device_metrics=True)
    assert model.training and grown == [64, 128, 64, 128]
    assert isinstance(res, training.EvalResult) and res.values.is_cuda
    got = res.as_reference()
    if task == 'class':
        assert len(got[0]) == 3 and not any(math.isnan(a) for a in want[0])
        assert max(abs(a - b) for a, b in zip(got[0] + [got[1]], want[0] + [want[1]])) <= 1e-12, (got, want)
        assert all(0.0 < a <= 1.0 for a in res.ap) and 0.0 < res.mean_ap <= 1.0
    else:
        assert abs(got - want) <= 1e-12, (got, want)
        assert res.mae > 0.0
