"""Agreement of a regression and thresholded metrics of a classification on the device (csrc/agree.hip behind
EvalBuffers.agreement() / threshold_metrics()) against scipy and sklearn in fp64 on the same fp32 inputs.

Row counts sit around the tile of entries a workgroup owns (R) and the chunk of rows it stages at a time (J), as built.  Bounds:
Kendall and Spearman are integer counts, one root and one division on either side (1e-12 absolute); the thresholded metrics are
exact counts and one division, log-loss and Brier sums of at most 2307 fp64 terms below 14 (1e-12); Pearson and R^2 are quotients
of centred fp64 sums whose terms, with both columns offset by 1e4, carry a relative error of a few 2^-53 * 1e4 (1e-10 absolute)."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'eagcn_amd', 'csrc', 'agree.hip')).read()
R = int(re.search(r'constexpr int AGR_R = (\d+);', _SRC).group(1))
J = int(re.search(r'constexpr int AGR_J = (\d+);', _SRC).group(1))
ROWS = [1, 2, 3, R - 1, R, R + 1, J + 1, 2 * J + R + 3]
REG_VARIANTS = ['plain', 'ties', 'offset', 'const_scores', 'const_targets', 'invalid', 'nonfinite']
CLS_VARIANTS = ['plain', 'tied', 'nopos', 'nolabel']
RANK_TOL, MOMENT_TOL = 1e-12, 1e-10


def fill(s, y, classification, valid=None, cap=None):
    """EvalBuffers holding exactly these scores / targets / validity (default: as eagcn_eval_append sets it), no model involved"""
    from eagcn_amd.training import EvalBuffers
    rows, T = s.shape
    if valid is None:
        valid = ((y == 0) | (y == 1)) if classification else np.ones_like(y, dtype=bool)
    buf = EvalBuffers(T, classification, torch.device('cuda'), cap=cap or max(rows, 1))
    buf.scores[:rows] = torch.from_numpy(s).cuda()
    buf.targets[:rows] = torch.from_numpy(y).cuda()
    buf.valid[:rows] = torch.from_numpy(valid).cuda().to(torch.uint8)
    buf.rows = rows
    return buf


def words(t):
    return t.view(torch.int64).cpu()


def nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.mean(v[~np.isnan(v)])) if (~np.isnan(v)).any() else float('nan')


def close(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.isnan(got) == np.isnan(want)).all() and (np.abs(got - want)[~np.isnan(want)] <= tol).all())


# ---- regression -------------------------------------------------------------------------------------------------------

def make_reg_case(rows, T, variant):
    """(scores, targets, valid, deliberate task or None): correlated fp32 columns"""
    rng = np.random.RandomState(6151 * rows + 17 * T + REG_VARIANTS.index(variant))
    y = rng.randn(rows, T).astype(np.float32)
    s = (0.7 * y + 0.7 * rng.randn(rows, T)).astype(np.float32)
    valid = np.ones((rows, T), dtype=bool)
    k = None
    if variant == 'ties':
        s, y = (np.round(s * 2) / 2).astype(np.float32), (np.round(y * 3) / 3).astype(np.float32)
    elif variant == 'offset':
        s, y = (s + np.float32(1e4)).astype(np.float32), (y + np.float32(1e4)).astype(np.float32)
    elif variant == 'const_scores':
        k = T // 2
        s[:, k] = np.float32(0.25)
    elif variant == 'const_targets':
        k = T // 2
        y[:, k] = np.float32(-1.5)
    elif variant == 'invalid':
        valid = rng.rand(rows, T) >= 0.15
        s[~valid] = np.float32(777.0)                      # what an invalid entry holds must not matter
        y[~valid] = np.float32(np.nan)
    elif variant == 'nonfinite':
        k = T // 2
        s[rows // 2, k] = np.float32(np.inf if rows % 2 else np.nan)
    return s, y, valid, k


def reg_reference(s, y, valid):
    """per task over the valid entries, on fp64 copies: [r2_score, pearsonr, spearmanr, kendalltau], count, bad; nan for n < 2, for a
    non-finite entry, where scipy says nan (a constant column) and for r2 of a constant targets column (the documented deviation)"""
    from scipy import stats
    from sklearn.metrics import r2_score
    T = s.shape[1]
    m, cnt, bad = np.full((4, T), np.nan), np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int64)
    for t in range(T):
        sd, yd = s[valid[:, t], t].astype(np.float64), y[valid[:, t], t].astype(np.float64)
        cnt[t], bad[t] = len(sd), int((~(np.isfinite(sd) & np.isfinite(yd))).sum())
        if cnt[t] < 2 or bad[t]:
            continue
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if (yd != yd[0]).any():
                m[0, t] = r2_score(yd, sd)
            m[1, t] = stats.pearsonr(sd, yd)[0]
            m[2, t] = stats.spearmanr(sd, yd)[0]
            m[3, t] = stats.kendalltau(sd, yd)[0]
    return m, cnt, bad


def check_reg(res, s, y, valid, k=None, variant='plain'):
    rows, T = s.shape
    want, cnt_w, bad_w = reg_reference(s, y, valid)
    if rows > 2:                                            # no case passes by nan == nan
        assert np.isfinite(want).all(0).any(), want
    assert res.T == T and res.values.dtype == torch.float64 and res.values.shape == (6 * T + 4,) and res.values.is_cuda
    v = res.values.cpu().numpy()
    got = v[:4 * T].reshape(4, T)
    err = np.abs(got - want)
    print('rows %d T %d %s: max |r2| %.2e |pearson| %.2e |spearman| %.2e |kendall| %.2e' % (
        (rows, T, variant) + tuple(np.nanmax(err[q]) if (~np.isnan(err[q])).any() else 0.0 for q in range(4))))
    assert (v[4 * T:5 * T] == cnt_w).all() and (v[5 * T:6 * T] == bad_w).all(), (v[4 * T:6 * T], cnt_w, bad_w)
    assert (np.isnan(got) == np.isnan(want)).all(), (got, want)
    assert close(got[0], want[0], MOMENT_TOL) and close(got[1], want[1], MOMENT_TOL), (got[:2], want[:2])
    assert close(got[2], want[2], RANK_TOL) and close(got[3], want[3], RANK_TOL), (got[2:], want[2:])
    for q, tol in enumerate((MOMENT_TOL, MOMENT_TOL, RANK_TOL, RANK_TOL)):
        assert close(v[6 * T + q], nanmean(want[q]), tol), (q, v[6 * T + q], nanmean(want[q]))
    if k is not None and rows > 2:
        if variant == 'const_scores':
            assert np.isnan(got[1:, k]).all() and np.isfinite(got[0, k])
        elif variant in ('const_targets', 'nonfinite'):
            assert np.isnan(got[:, k]).all()
    # the accessors read the same vector
    np.testing.assert_array_equal(np.array(res.r2), got[0])
    np.testing.assert_array_equal(np.array(res.pearson), got[1])
    np.testing.assert_array_equal(np.array(res.rsquared), got[1] * got[1])
    np.testing.assert_array_equal(np.array(res.spearman), got[2])
    np.testing.assert_array_equal(np.array(res.kendall), got[3])
    assert res.count == list(cnt_w) and res.n_bad == list(bad_w)
    np.testing.assert_array_equal(np.array([res.mean_r2, res.mean_pearson, res.mean_spearman, res.mean_kendall]), v[6 * T:])


@pytest.mark.parametrize('variant', REG_VARIANTS)
@pytest.mark.parametrize('T', [1, 3, 12])
@pytest.mark.parametrize('rows', ROWS)
def test_regression_agreement_matches_scipy(rows, T, variant):
    from eagcn_amd import _lib
    s, y, valid, k = make_reg_case(rows, T, variant)
    if T == 1 and rows > 2 and variant in ('const_scores', 'const_targets', 'nonfinite'):
        k = None                                            # the only task stays a plain one: it must carry four finite values
        s, y, valid, _ = make_reg_case(rows, T, 'plain')
    # of these shapes, those with one task and more than one chunk of rows are the ones whose rows several workgroups share
    assert (_lib.load().eagcn_eval_agreement_splits(rows, T) > 1) == (rows > J and T == 1)
    check_reg(fill(s, y, False, valid).agreement(), s, y, valid, k, variant)


def test_split_threshold():
    """the smallest one-task row count whose j range is shared by several workgroups (the finalize forms a, b from the summed counts),
    and the one just below it (each lane forms them): both with heavy ties and invalid entries"""
    from eagcn_amd import _lib
    sp = _lib.load().eagcn_eval_agreement_splits
    first = next(rows for rows in range(1, 1 << 16) if sp(rows, 1) > 1)
    assert sp(first, 1) != sp(first - 1, 1) == 1
    for rows in (first - 1, first):
        s, y, _, _ = make_reg_case(rows, 1, 'ties')
        valid = np.random.RandomState(rows).rand(rows, 1) >= 0.15
        check_reg(fill(s, y, False, valid).agreement(), s, y, valid, None, 'ties at the split threshold')


def test_signed_zeros_are_one_value():
    s = np.array([[0.0], [-0.0], [1.0], [-1.0], [0.0]], dtype=np.float32)
    y = np.array([[-0.0], [0.0], [2.0], [-3.0], [1.0]], dtype=np.float32)
    valid = np.ones_like(s, dtype=bool)
    check_reg(fill(s, y, False, valid).agreement(), s, y, valid)


# ---- classification ---------------------------------------------------------------------------------------------------

def make_cls_case(rows, T, variant, thr):
    """fp32 scores in [1e-6, 1 - 1e-6] (no clip is active), labels in {1, 0, -1}: about 20 % positives, 15 % missing"""
    rng = np.random.RandomState(7919 * rows + 31 * T + CLS_VARIANTS.index(variant))
    s = (1e-6 + (1 - 2e-6) * rng.rand(rows, T)).astype(np.float32)
    u = rng.rand(rows, T)
    y = np.where(u < 0.15, -1.0, np.where(u < 0.35, 1.0, 0.0)).astype(np.float32)
    y[0], y[rows - 1] = 1.0, 0.0                            # labelled entries in every task, whatever the draw
    k = None
    if variant == 'tied':
        s[rng.rand(rows, T) < 0.3] = np.float32(thr)       # exactly at the threshold: not predicted positive
    elif variant == 'nopos':
        k = T // 2
        y[:, k][y[:, k] == 1] = 0.0
    elif variant == 'nolabel':
        k = T // 2
        y[:, k] = -1.0
    return s, y, k


def cls_reference(s, y, thr):
    """[log_loss, brier, tp, fp, tn, fn, accuracy, precision, recall, f1, mcc] per task from sklearn over the labelled entries, on fp64
    copies of the scores; nan throughout for a task without labels"""
    from sklearn import metrics
    T = s.shape[1]
    m = np.full((11, T), np.nan)
    for t in range(T):
        lab = y[:, t] != -1
        if not lab.any():
            continue
        yt, sd = y[lab, t].astype(np.int64), s[lab, t].astype(np.float64)
        pred = (s[lab, t] > np.float32(thr)).astype(np.int64)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            cm = metrics.confusion_matrix(yt, pred, labels=[0, 1])
            m[:, t] = [metrics.log_loss(yt, sd, labels=[0, 1]), metrics.brier_score_loss(yt, sd), cm[1, 1], cm[0, 1], cm[0, 0], cm[1, 0],
                       metrics.accuracy_score(yt, pred), metrics.precision_score(yt, pred), metrics.recall_score(yt, pred),
                       metrics.f1_score(yt, pred), metrics.matthews_corrcoef(yt, pred)]
    return m


def check_cls(res, want, rows, T, label=''):
    assert res.T == T and res.values.dtype == torch.float64 and res.values.shape == (12 * T + 4,) and res.values.is_cuda
    v = res.values.cpu().numpy()
    got = v[:11 * T].reshape(11, T)
    err = np.abs(got - want)
    print('rows %d T %d %s: max |log_loss| %.2e |brier| %.2e |f1| %.2e |mcc| %.2e' % (
        (rows, T, label) + tuple(np.nanmax(err[q]) if (~np.isnan(err[q])).any() else 0.0 for q in (0, 1, 9, 10))))
    assert (np.isnan(got) == np.isnan(want)).all(), (got, want)
    lab = ~np.isnan(want[0])
    assert (got[2:6, lab] == want[2:6, lab]).all(), (got[2:6], want[2:6])
    assert (v[11 * T:12 * T] == 0).all()
    assert close(got, want, RANK_TOL), (got, want)
    for q, row in enumerate((0, 1, 9, 10)):
        assert close(v[12 * T + q], nanmean(want[row]), RANK_TOL), (q, v[12 * T + q], nanmean(want[row]))
    for name, row in (('log_loss', 0), ('brier', 1), ('accuracy', 6), ('precision', 7), ('recall', 8), ('f1', 9), ('mcc', 10)):
        np.testing.assert_array_equal(np.array(getattr(res, name)), got[row])
    for name, row in (('tp', 2), ('fp', 3), ('tn', 4), ('fn', 5)):
        assert getattr(res, name) == [int(c) if ok else None for c, ok in zip(got[row], lab)]
    np.testing.assert_array_equal(np.array([res.mean_log_loss, res.mean_brier, res.mean_f1, res.mean_mcc]), v[12 * T:])


@pytest.mark.parametrize('thr', [0.5, 0.3])
@pytest.mark.parametrize('variant', CLS_VARIANTS)
@pytest.mark.parametrize('T', [1, 3, 12])
@pytest.mark.parametrize('rows', ROWS)
def test_threshold_metrics_match_sklearn(rows, T, variant, thr):
    s, y, k = make_cls_case(rows, T, variant, thr)
    want = cls_reference(s, y, thr)
    if k is not None and variant == 'nolabel':
        assert np.isnan(want[:, k]).all()
    if rows > 2 and not (T == 1 and variant == 'nolabel'):  # no case passes by nan == nan
        assert np.isfinite(want).all(0).any()
    res = fill(s, y, True).threshold_metrics(thr)
    assert res.threshold == thr
    check_cls(res, want, rows, T, '%s at %.1f' % (variant, thr))


def test_scores_of_exactly_zero_and_one_are_clipped():
    rows, T = R + 1, 3
    rng = np.random.RandomState(23)
    s = rng.randint(0, 2, size=(rows, T)).astype(np.float32)
    y = rng.randint(0, 2, size=(rows, T)).astype(np.float32)
    eps = 2.0 ** -52
    p, yd = np.clip(s.astype(np.float64), eps, 1.0 - eps), y.astype(np.float64)
    ll = -(yd * np.log(p) + (1 - yd) * np.log(1 - p)).mean(0)
    br = ((p - yd) ** 2).mean(0)
    assert (ll > 10).all()                                  # about half of the entries sit at the clip
    v = fill(s, y, True).threshold_metrics().values.cpu().numpy()
    print('clip: max relative log-loss error %.2e, max brier error %.2e' % ((np.abs(v[:T] - ll) / ll).max(), np.abs(v[T:2 * T] - br).max()))
    assert (np.abs(v[:T] - ll) <= 1e-12 * ll).all() and (np.abs(v[T:2 * T] - br) <= 1e-12).all(), (v[:2 * T], ll, br)
    assert (v[2 * T:3 * T] == ((s == 1) & (y == 1)).sum(0)).all() and (v[4 * T:5 * T] == ((s == 0) & (y == 0)).sum(0)).all()


def test_nonfinite_labelled_score_is_counted_and_raises():
    from eagcn_amd import _lib
    s, y, _ = make_cls_case(R + 1, 3, 'plain', 0.5)
    y[R, 1], s[R, 1] = 1.0, np.nan                          # a labelled entry, in the second tile
    y[3, 2], s[3, 2] = -1.0, np.inf                         # ... and an unlabelled one, which does not count
    res = fill(s, y, True).threshold_metrics()
    v = res.values.cpu().numpy()
    assert list(v[11 * 3:12 * 3]) == [0.0, 1.0, 0.0]
    assert np.isnan(v[1:11 * 3:3]).all() and np.isfinite(v[0:11 * 3:3]).all() and np.isfinite(v[2:11 * 3:3]).all()
    want = cls_reference(s[:, [0, 2]], y[:, [0, 2]], 0.5)
    assert close(v[:11 * 3].reshape(11, 3)[:, [0, 2]], want, RANK_TOL)
    assert close(v[36:], [nanmean(want[q]) for q in (0, 1, 9, 10)], RANK_TOL)
    for name in ('log_loss', 'tp', 'f1', 'mean_mcc'):
        with pytest.raises(_lib.EagcnHipError, match=r'task 1 has 1 labelled'):
            getattr(res, name)


# ---- both kinds -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module', params=[1, 3])
def big_reg(request):
    """the largest shape with heavy ties and invalid entries.  One task: three workgroups share a tile's rows; three tasks: one walks them"""
    s, y, _, _ = make_reg_case(2 * J + R + 3, request.param, 'ties')
    valid = np.random.RandomState(99).rand(*s.shape) >= 0.15
    return s, y, valid


@pytest.fixture(scope='module')
def big_cls():
    return make_cls_case(2 * J + R + 3, 3, 'tied', 0.5)[:2]


def test_two_calls_are_bit_identical_and_leave_metrics_alone(big_reg, big_cls):
    s, y, valid = big_reg
    buf = fill(s, y, False, valid)
    before = words(buf.metrics().values)
    assert torch.equal(words(buf.agreement().values), words(buf.agreement().values))
    assert torch.equal(words(buf.metrics().values), before)
    buf = fill(*big_cls, True)
    before = words(buf.metrics().values)
    assert torch.equal(words(buf.threshold_metrics().values), words(buf.threshold_metrics().values))
    assert torch.equal(words(buf.metrics().values), before)


@pytest.mark.parametrize('classification', [True, False])
def test_poisoned_workspace_gives_the_same_words(big_reg, big_cls, classification):
    """through the C ABI: the kernels write every workspace word the finalize reads, so the workspace needs no clear"""
    from eagcn_amd import _lib
    lib = _lib.load()
    buf = fill(*big_cls, True) if classification else fill(big_reg[0], big_reg[1], False, big_reg[2])
    rows, T = buf.rows, buf.T
    nbytes = lib.eagcn_eval_agreement_workspace_bytes(rows, T)
    outs = []
    for byte in (0x00, 0xFF):
        ws = torch.full((nbytes,), byte, dtype=torch.uint8, device='cuda')
        out = torch.full(((12 if classification else 6) * T + 4,), -7.0, dtype=torch.float64, device='cuda')
        head = (buf.scores.data_ptr(), buf.targets.data_ptr(), buf.valid.data_ptr(), rows, T)
        tail = (ws.data_ptr(), nbytes, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        rc = lib.eagcn_eval_class_threshold(*head, 0.5, *tail) if classification else lib.eagcn_eval_reg_agreement(*head, *tail)
        _lib.check(rc, 'agreement')
        outs.append(words(out))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], words((buf.threshold_metrics() if classification else buf.agreement()).values))


def test_wrong_buffer_kind_raises(big_cls):
    from eagcn_amd import _lib
    s, y = big_cls
    with pytest.raises(_lib.EagcnHipError, match='classification'):
        fill(s[:5], y[:5], True).agreement()
    with pytest.raises(_lib.EagcnHipError, match='regression'):
        fill(s[:5], y[:5], False).threshold_metrics()


def test_workspace_regrows_with_the_buffers():
    from eagcn_amd.training import EvalBuffers
    rng = np.random.RandomState(3)
    x, y = rng.randn(96, 3).astype(np.float32), rng.randn(96, 3).astype(np.float32)
    buf = EvalBuffers(3, False, torch.device('cuda'), cap=64)
    buf.append(torch.from_numpy(x[:64]).cuda(), torch.from_numpy(y[:64]).cuda())
    first = buf.agreement()
    ws = buf._agree_workspace
    buf.append(torch.from_numpy(x[64:]).cuda(), torch.from_numpy(y[64:]).cuda())
    assert buf.cap == 128 and buf._agree_workspace is None
    second = buf.agreement()
    assert buf._agree_workspace is not None and buf._agree_workspace is not ws
    for res, n in ((first, 64), (second, 96)):
        check_reg(res, x[:n], y[:n], np.ones((n, 3), dtype=bool))


# ---- end to end -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('task', ['class', 'reg'])
def test_evaluate_extended(task, monkeypatch):
    from eagcn_amd import Concate_GCN, training
    from eagcn_amd.synthetic import make_batch
    torch.manual_seed(4)
    model = Concate_GCN(7, 24, *[8, 6, 4, 4, 5], *[10, 7, 5, 6, 4], 16, 8, 3, 0.3, n_layers=2, graph=True).cuda().train()
    mbs = [make_batch(B=32, n_max=20, n_med=8, rel_channels=(7, 4, 2, 2, 2), seed=200 + i, n_tasks=3, task=task) for i in range(2)]
    batches = [(tuple(t.cuda() for t in mb.dense()), torch.from_numpy(mb.labels).cuda()) for mb in mbs]
    with pytest.raises(ValueError, match='device_metrics'):
        training.evaluate(model, batches, task, 3, extended=True)
    plain = training.evaluate(model, batches, task, 3, device_metrics=True)
    made = []

    class Recorded(training.EvalBuffers):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(training, 'EvalBuffers', Recorded)
    res, more = training.evaluate(model, batches, task, 3, device_metrics=True, extended=True, threshold=0.3)
    assert model.training and isinstance(res, training.EvalResult)
    assert torch.equal(words(res.values), words(plain.values))
    scores, targets, valid = (t.cpu().numpy() for t in made[-1].views())       # the buffers the extended result was computed over
    assert scores.shape == (64, 3)
    if task == 'reg':
        assert isinstance(more, training.AgreementResult)
        check_reg(more, scores, targets, valid)
    else:
        assert isinstance(more, training.ThresholdResult) and more.threshold == 0.3
        check_cls(more, cls_reference(scores, np.where(valid, targets, -1.0).astype(np.float32), 0.3), 64, 3, 'end to end')
