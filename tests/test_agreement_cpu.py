"""Host side of the agreement / thresholded metrics (csrc/agree.hip, include/eagcn_hip.h eagcn_eval_reg_agreement and
eagcn_eval_class_threshold), no GPU needed: the symbols exist and are bound, argument errors come back as messages before any HIP
call, the workspace size is the header's formula, the integer identities the kernels implement equal scipy's kendalltau, spearmanr
and pearsonr and sklearn's r2_score, and the kernels carry no scratch."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('eagcn_eval_agreement_workspace_bytes', 'eagcn_eval_agreement_splits', 'eagcn_eval_reg_agreement', 'eagcn_eval_class_threshold')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()                                       # hipcc cross-compiles gfx950 without a GPU
    from eagcn_amd import _lib
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from eagcn_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r'\b%s\s*\(' % name, re.sub(r'/\*.*?\*/', '', header, flags=re.S)), name
    assert lib.eagcn_abi_version() == _lib.ABI_VERSION == 8
    import eagcn_amd
    from eagcn_amd import training
    assert eagcn_amd.AgreementResult is training.AgreementResult and eagcn_amd.ThresholdResult is training.ThresholdResult


def _call(lib, fn, scores=16, targets=16, valid=16, rows=4, T=1, workspace=16, workspace_bytes=1 << 20, out=16, threshold=0.5):
    # the pointers are never dereferenced: every case fails its argument check, which comes before any HIP call
    if fn == 'eagcn_eval_class_threshold':
        return getattr(lib, fn)(scores, targets, valid, rows, T, threshold, workspace, workspace_bytes, out, None)
    return getattr(lib, fn)(scores, targets, valid, rows, T, workspace, workspace_bytes, out, None)


BAD = [(dict(scores=None), 'scores'), (dict(targets=None), 'targets'), (dict(valid=None), 'valid'), (dict(workspace=None), 'workspace'),
       (dict(out=None), 'out'), (dict(rows=0), 'rows'), (dict(rows=-3), 'rows'), (dict(T=0), 'T'),
       (dict(rows=2 ** 31, workspace_bytes=2 ** 62), 'rows'), (dict(rows=300, T=12, workspace_bytes=1000), 'workspace')]


@pytest.mark.parametrize('fn, bad, word', [(fn, bad, word) for fn in NAMES[2:] for bad, word in BAD] +
                         [('eagcn_eval_class_threshold', dict(threshold=float('nan')), 'threshold')])
def test_argument_errors_name_the_argument(lib, fn, bad, word):
    from eagcn_amd import _lib
    rc = _call(lib, fn, **bad)
    assert rc == -1
    msg = lib.eagcn_last_error().decode()
    assert fn in msg and re.search(r'\b%s\b' % word, msg), msg
    with pytest.raises(_lib.EagcnHipError):
        _lib.check(rc, fn)


def _formula(rows, T):
    tiles, chunks = -(-rows // 256), -(-rows // 1024)
    return T * tiles * (min(chunks, 8) * 256 * 20 + 128)


def test_workspace_bytes_is_the_headers_formula(lib):
    header = open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read()
    assert 'T * tiles * (min(chunks, 8) * 256 * 20 + 128)' in header
    ws = lib.eagcn_eval_agreement_workspace_bytes
    for rows, T in ((1, 1), (257, 12), (40000, 1)):
        assert ws(rows, T) == _formula(rows, T) > 0, (rows, T)
    assert ws(1, 1) == 5248 and ws(257, 12) == 12 * 2 * 5248 and ws(40000, 1) == 157 * (8 * 5120 + 128)
    assert ws(0, 3) == 0 and ws(5, 0) == 0 and ws(-1, 1) == 0
    rows = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2307, 8191, 8192, 8193, 40000, 2 ** 31 - 1]
    for T in (1, 3, 12):
        sizes = [ws(r, T) for r in rows]
        assert sizes == sorted(sizes), (T, sizes)
    for r in rows:
        sizes = [ws(r, T) for T in range(1, 14)]
        assert sizes == sorted(sizes), (r, sizes)


def test_splits(lib):
    sp = lib.eagcn_eval_agreement_splits
    for rows, T in ((1, 1), (2, 1), (255, 3), (1024, 1), (257, 12), (300, 300)):
        assert sp(rows, T) == 1, (rows, T)
    split = [rows for rows in range(1, 5000) if sp(rows, 1) > 1]
    assert split, 'no one-task shape below 5000 rows is split'
    assert 1 < sp(40000, 1) <= 8 and sp(100000, 1) == 1      # 157 tiles leave CUs idle, 391 do not
    for rows, T in ((1025, 1), (4200, 1), (100000, 1), (100000, 12), (2 ** 31 - 1, 1)):
        assert 1 <= sp(rows, T) <= min(8, -(-rows // 1024)), (rows, T)


def mirror(s, y):
    """numpy mirror of the integer identities of csrc/agree.hip over one task's valid entries (s, y fp32): the pair counts, a, b, S, n1,
    n2, and the quotients of its finalize; the moments in plain centred fp64.  O(n^2) memory: test sizes only.
    Returns (r2, pearson, spearman, kendall), nan as the header defines it."""
    s, y = np.asarray(s, dtype=np.float32), np.asarray(y, dtype=np.float32)
    n = len(s)
    lt_s, eq_s = (s[None, :] < s[:, None]).sum(1).astype(np.int64), (s[None, :] == s[:, None]).sum(1).astype(np.int64)
    lt_y, eq_y = (y[None, :] < y[:, None]).sum(1).astype(np.int64), (y[None, :] == y[:, None]).sum(1).astype(np.int64)
    S = (np.sign(s[:, None] - s[None, :]).astype(np.int64) * np.sign(y[:, None] - y[None, :]).astype(np.int64)).sum(1)
    a, b = 2 * lt_s + eq_s - n, 2 * lt_y + eq_y - n
    n0, n1, n2 = n * (n - 1) // 2, int((eq_s - 1).sum()) // 2, int((eq_y - 1).sum()) // 2
    nan = float('nan')
    if n < 2:
        return nan, nan, nan, nan
    sd, yd = s.astype(np.float64), y.astype(np.float64)
    cs, cy = sd - sd.mean(), yd - yd.mean()
    r2 = 1.0 - ((yd - sd) ** 2).sum() / (cy * cy).sum() if n0 > n2 else nan
    if n0 == n1 or n0 == n2:
        return r2, nan, nan, nan
    pearson = (cs * cy).sum() / np.sqrt((cs * cs).sum() * (cy * cy).sum())
    spearman = int((a * b).sum()) / np.sqrt(float(int((a * a).sum())) * float(int((b * b).sum())))
    kendall = (int(S.sum()) // 2) / (np.sqrt(float(n0 - n1)) * np.sqrt(float(n0 - n2)))
    return r2, pearson, spearman, kendall


def make_pair(n, variant, seed=0):
    rng = np.random.RandomState(2000 + n + seed)
    y = rng.randn(n).astype(np.float32)
    s = (0.7 * y + 0.7 * rng.randn(n)).astype(np.float32)
    if variant == 'ties':
        s, y = (np.round(s * 2) / 2).astype(np.float32), (np.round(y * 3) / 3).astype(np.float32)
    elif variant == 'offset':
        s, y = (s + np.float32(1e4)).astype(np.float32), (y + np.float32(1e4)).astype(np.float32)
    elif variant == 'const':
        s[:] = np.float32(0.25)
    return s, y


def scipy_reference(s, y):
    """(r2_score, pearsonr, spearmanr, kendalltau) on fp64 copies; nan where scipy says nan (constant input), and r2 = nan for constant
    targets (the documented deviation) or fewer than two entries"""
    import warnings
    from scipy import stats
    from sklearn.metrics import r2_score
    sd, yd = np.asarray(s, dtype=np.float64), np.asarray(y, dtype=np.float64)
    nan = float('nan')
    if len(sd) < 2:
        return nan, nan, nan, nan
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        r2 = r2_score(yd, sd) if (yd != yd[0]).any() else nan
        return (r2, float(stats.pearsonr(sd, yd)[0]), float(stats.spearmanr(sd, yd)[0]), float(stats.kendalltau(sd, yd)[0]))


@pytest.mark.parametrize('n', [2, 3, 17, 256, 1025, 2307])
@pytest.mark.parametrize('variant', ['plain', 'ties', 'offset', 'const'])
def test_identities_match_scipy(n, variant):
    s, y = make_pair(n, variant)
    if variant == 'ties' and n == 2:
        y[1] = y[0] + 1.0                                   # two entries rounded onto one value would be a constant column
        s[1] = s[0] - 0.5
    got, want = mirror(s, y), scipy_reference(s, y)
    for name, g, w in zip(('r2', 'pearson', 'spearman', 'kendall'), got, want):
        assert np.isnan(g) == np.isnan(w), (name, g, w)
        assert np.isnan(w) or abs(g - w) <= 1e-12, (name, g, w, g - w)
    if variant == 'const':
        assert np.isnan(got[1]) and np.isnan(got[2]) and np.isnan(got[3]) and not np.isnan(got[0])
    else:
        assert not np.isnan(got).any()


def class_mirror(s, y, thr):
    """numpy form of the thresholded metrics over one task's labelled entries (s fp32 scores, y in {0, 1}), as the header defines them"""
    s = np.asarray(s, dtype=np.float32)
    y = np.asarray(y).astype(np.float64)
    eps = 2.0 ** -52
    p = np.clip(s.astype(np.float64), eps, 1.0 - eps)
    pred = s > np.float32(thr)
    tp, fp = int((pred & (y == 1)).sum()), int((pred & (y == 0)).sum())
    tn, fn = int((~pred & (y == 0)).sum()), int((~pred & (y == 1)).sum())
    den = np.sqrt(float((tp + fp) * (tp + fn)) * float((tn + fp) * (tn + fn)))
    return dict(log_loss=float(-(y * np.log(p) + (1 - y) * np.log(1 - p)).mean()), brier=float(((p - y) ** 2).mean()),
                tp=tp, fp=fp, tn=tn, fn=fn, accuracy=(tp + tn) / len(y),
                precision=tp / (tp + fp) if tp + fp else 0.0, recall=tp / (tp + fn) if tp + fn else 0.0,
                f1=2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0, mcc=(tp * tn - fp * fn) / den if den > 0 else 0.0)


@pytest.mark.parametrize('n', [3, 17, 1025])
@pytest.mark.parametrize('thr', [0.5, 0.3])
def test_threshold_formulas_match_sklearn(n, thr):
    import warnings
    from sklearn import metrics
    rng = np.random.RandomState(n)
    s = (1e-6 + (1 - 2e-6) * rng.rand(n)).astype(np.float32)
    s[::5] = np.float32(thr)                                # tied at the threshold: not predicted positive
    y = (rng.rand(n) < 0.3).astype(np.int64)
    y[0], y[1] = 1, 0
    got = class_mirror(s, y, thr)
    sd, pred = s.astype(np.float64), (s > np.float32(thr)).astype(np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        cm = metrics.confusion_matrix(y, pred, labels=[0, 1])
        want = dict(log_loss=metrics.log_loss(y, sd, labels=[0, 1]), brier=metrics.brier_score_loss(y, sd), tn=cm[0, 0], fp=cm[0, 1],
                    fn=cm[1, 0], tp=cm[1, 1], accuracy=metrics.accuracy_score(y, pred), precision=metrics.precision_score(y, pred),
                    recall=metrics.recall_score(y, pred), f1=metrics.f1_score(y, pred), mcc=metrics.matthews_corrcoef(y, pred))
    for k, w in want.items():
        assert abs(got[k] - w) <= 1e-12, (k, got[k], w)


def test_agreement_kernels_have_no_scratch(tmp_path):
    """compiled with the flags of tests/test_isa_cpu.py: no scratch and at most 128 VGPRs for every kernel of csrc/agree.hip"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'hipcc not found'
    from test_isa_cpu import FLAGS, _kernels
    out = str(tmp_path / 'agree.s')
    r = subprocess.run([hipcc] + FLAGS + ['-o', out, os.path.join(ROOT, 'eagcn_amd', 'csrc', 'agree.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = _kernels(open(out).read())
    want = ('agree_pair_kernel', 'agree_reg_finalize_kernel', 'agree_class_kernel', 'agree_class_finalize_kernel')
    assert len(ks) == 4 and all(any(k in name for name in ks) for k in want), sorted(ks)
    for name, (scratch, vgpr) in ks.items():
        assert scratch == 0, '%s: %d bytes of scratch per lane (%d VGPRs)' % (name, scratch, vgpr)
        assert vgpr <= 128, (name, vgpr)
