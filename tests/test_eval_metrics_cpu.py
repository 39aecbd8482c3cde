"""Host side of the device evaluation metrics (csrc/metrics.hip, include/eagcn_hip.h eagcn_eval_*_metrics), no GPU needed: the
symbols exist and are bound, argument errors come back as messages before any HIP call, the workspace size is the header's formula,
the two sort-free identities the kernels implement equal sklearn's roc_curve + auc and average_precision_score, and the kernels
carry no scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('eagcn_eval_metrics_workspace_bytes', 'eagcn_eval_class_metrics', 'eagcn_eval_reg_metrics')


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


def _call(lib, fn, scores=16, targets=16, valid=16, rows=4, T=1, workspace=16, workspace_bytes=1 << 20, out=16):
    # the pointers are never dereferenced: every case fails its argument check, which comes before any HIP call
    return getattr(lib, fn)(scores, targets, valid, rows, T, workspace, workspace_bytes, out, None)


@pytest.mark.parametrize('fn', NAMES[1:])
@pytest.mark.parametrize('bad, word', [
    (dict(scores=None), 'scores'), (dict(targets=None), 'targets'), (dict(valid=None), 'valid'), (dict(workspace=None), 'workspace'),
    (dict(out=None), 'out'), (dict(rows=0), 'rows'), (dict(rows=-3), 'rows'), (dict(T=0), 'T'), (dict(rows=2 ** 31, workspace_bytes=2 ** 62), 'rows'),
    (dict(rows=300, T=12, workspace_bytes=1000), 'workspace')])
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
    return T * tiles * min(chunks, 8) * (256 * 8 + 32)


def test_workspace_bytes_is_the_headers_formula(lib):
    header = open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read()
    assert 'T * tiles * min(chunks, 8) * (256 * 8 + 32)' in header
    ws = lib.eagcn_eval_metrics_workspace_bytes
    for rows, T in ((1, 1), (257, 12), (40000, 1)):
        assert ws(rows, T) == _formula(rows, T) > 0, (rows, T)
    assert ws(1, 1) == 2080 and ws(257, 12) == 12 * 2 * 2080 and ws(40000, 1) == 157 * 8 * 2080
    assert ws(0, 3) == 0 and ws(5, 0) == 0
    rows = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2307, 8191, 8192, 8193, 40000, 2 ** 31 - 1]
    for T in (1, 3, 12):
        sizes = [ws(r, T) for r in rows]
        assert sizes == sorted(sizes), (T, sizes)
    for r in rows:
        sizes = [ws(r, T) for T in range(1, 14)]
        assert sizes == sorted(sizes), (r, sizes)


def mirror(s, y):
    """numpy mirror of the two identities over the labelled entries (s fp32 scores, y in {0, 1}): the integer counts of
    csrc/metrics.hip and the two quotients of its finalize.  O(P n) memory: test sizes only."""
    s, y = np.asarray(s, dtype=np.float32), np.asarray(y)
    pos, neg = s[y == 1], s[y == 0]
    P, N = len(pos), len(neg)
    neg_lt = (neg[None, :] < pos[:, None]).sum(1)
    neg_eq = (neg[None, :] == pos[:, None]).sum(1)
    pos_ge = (pos[None, :] >= pos[:, None]).sum(1)
    auc = int((2 * neg_lt + neg_eq).sum()) / (2.0 * P * N)
    ap = float((pos_ge / (pos_ge + (N - neg_lt)).astype(np.float64)).sum()) / P
    return auc, ap


@pytest.mark.parametrize('n', [2, 3, 17, 256, 1000, 5000])
@pytest.mark.parametrize('ties', ['none', 'fifths', 'all'])
def test_identities_match_sklearn(n, ties):
    from sklearn import metrics
    rng = np.random.RandomState(1000 + n)
    y = (rng.rand(n) < 0.2).astype(np.int64)
    y[0], y[1] = 1, 0                                   # both classes, always
    s = rng.rand(n).astype(np.float32)
    if ties == 'fifths':
        s = (np.round(s * 5) / 5).astype(np.float32)
    elif ties == 'all':
        s[:] = 0.5
    auc, ap = mirror(s, y)
    fpr, tpr, _ = metrics.roc_curve(y, s)
    assert abs(auc - metrics.auc(fpr, tpr)) <= 1e-12
    assert abs(ap - metrics.average_precision_score(y, s)) <= 1e-12
    if ties == 'all':
        assert auc == 0.5 and abs(ap - y.mean()) <= 1e-15


def test_metrics_kernels_have_no_scratch(tmp_path):
    """compiled with the flags of tests/test_isa_cpu.py: private_segment_fixed_size == 0 for every kernel of csrc/metrics.hip"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'hipcc not found'
    from test_isa_cpu import FLAGS, _kernels
    out = str(tmp_path / 'metrics.s')
    r = subprocess.run([hipcc] + FLAGS + ['-o', out, os.path.join(ROOT, 'eagcn_amd', 'csrc', 'metrics.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = _kernels(open(out).read())
    seen = {k for k in ('eval_rank_kernel', 'eval_sums_kernel', 'eval_finalize_kernel') if any(k in name for name in ks)}
    assert len(seen) == 3 and len(ks) == 4, sorted(ks)          # the finalize has a classification and a regression form
    for name, (scratch, vgpr) in ks.items():
        assert scratch == 0, '%s: %d bytes of scratch per lane (%d VGPRs)' % (name, scratch, vgpr)
        assert vgpr <= 128, (name, vgpr)                          # the rank kernel keeps 8 waves per SIMD, the finalize runs 1024 threads
