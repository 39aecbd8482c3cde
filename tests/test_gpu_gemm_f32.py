"""The fp32 matrix-core GEMM (csrc/gemm.hip, balanced form csrc/gemm3.hip; reference layers.py:382-387 `x @ W` and layers.py:40
`torch.mm` with its two autograd products) through its C-ABI entry points eagcn_gemm_f32, eagcn_gemm_f32_dev and eagcn_gemm_f32_sk,
held to the float64 product of the logical operands.

Harness: every operand lives in an allocation with a leading dimension larger than its extent and spare rows, everything outside
the logical matrix holds +-7e30 (an over-read shows up as a wrong result, never as an access outside the allocation); C has
ldc > N and spare rows and is pre-filled with NaN: after the call the logical block matches float64 and everything else is still
NaN.  Error measure e = max |got - ref| / sum_k |a||b| in units of 2^-24, against two bounds:
  hard    e <= K: the kernel is a k-ordered fmaf chain (exact products, one rounding per accumulate), so K 2^-24 sum|a||b| is
          rigorous, and for K < 4096 still smaller than one dropped or duplicated term;
  tighter e <= max(8, 4 e_torch): e_torch is the same measure for torch.matmul in fp32 on the same operands (an independent
          implementation); 8 is the project's own figure for the plane kernel (test_gpu_bx3.py), 4 covers the different
          summation order (tools/gemm_accuracy.py measured 4-6 eps for both).
Each case prints its e and e_torch."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
POISON = 7.0e30
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _lib():
    from eagcn_amd import _lib as L
    return L.load(), L


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _up4(n):
    return (n + 3) // 4 * 4


@pytest.fixture
def gemm_mode(request):
    """gemm mode of the case (0: fp32 MFMA; 1: bf16 x 6 for K >= 64, csrc/gemm_x6.h), restored afterwards"""
    lib, _ = _lib()
    old = lib.eagcn_set_gemm_mode(getattr(request, 'param', 0))
    try:
        yield getattr(request, 'param', 0)
    finally:
        lib.eagcn_set_gemm_mode(old)


@functools.lru_cache(maxsize=3)
def _case(M, N, K):
    """Logical operands a [M, K], b [K, N] (fp32, b with a wide dynamic range), their float64 product, sum |a||b| and e_torch:
    computed once per shape on the device, shared by every form / mode / layout of that shape and never written to."""
    g = torch.Generator(device='cuda').manual_seed(1000003 * M + 1009 * N + K)
    a = torch.randn(M, K, device='cuda', generator=g)
    b = torch.randn(K, N, device='cuda', generator=g)
    b = b * torch.exp(3.0 * torch.randn(K, N, device='cuda', generator=g))
    return (a, b) + _reference(a, b)


def _reference(a, b):
    ref = a.double() @ b.double()
    den = a.double().abs() @ b.double().abs()
    e_torch = _measure(torch.matmul(a, b), ref, den) if a.shape[1] else 0.0
    return ref, den, e_torch


def _measure(got, ref, den):
    return ((got.double() - ref).abs() / den.clamp_min(1e-300)).max().item() / EPS


def _store(x, trans, poison, ld=None, offset=0, spare=3):
    """The logical matrix x [R, Cc] as a kernel operand: stored as it is or transposed, inside a poisoned allocation with `spare`
    rows after the last one, a leading dimension `ld` (default: 4 to 7 floats more than the extent, a multiple of 4) and
    `offset` floats in front of the base (a view into the larger tensor: offset 1 breaks the 16-byte alignment and nothing
    else).  Returns (view [rows + spare, ld] whose data_ptr() is the operand's base, ld)."""
    xs = x.t() if trans else x
    R, Cc = xs.shape
    ld = ld if ld is not None else _up4(Cc) + 4
    assert ld > Cc
    buf = torch.full((offset + (R + spare) * ld + 64,), poison, device='cuda')
    view = buf[offset:offset + (R + spare) * ld].view(R + spare, ld)
    view[:R, :Cc] = xs
    return view, ld


def _output(M, N, ldc=None, spare=3):
    ldc = ldc if ldc is not None else N + 5
    return torch.full((M + spare, ldc), float('nan'), device='cuda'), ldc


def _held(Cm, rows, N, ref, den, e_torch, K, tag):
    """The logical block Cm[:rows, :N] against float64 under both bounds; everything else of Cm still NaN.  Returns e."""
    got = Cm[:rows, :N]
    assert not torch.isnan(got).any(), '%s: the logical block is not completely written' % tag
    e = _measure(got, ref[:rows], den[:rows]) if rows and N else 0.0
    print('%s: e = %.3f, e_torch = %.3f (units of 2^-24 of sum |a||b|)' % (tag, e, e_torch))
    rest = Cm.clone()
    rest[:rows, :N] = float('nan')
    assert torch.isnan(rest).all(), '%s: a store landed outside the logical block' % tag
    assert e <= K, '%s: e = %.3f beyond the k-ordered fmaf chain bound K = %d' % (tag, e, K)
    assert e <= max(8.0, 4.0 * e_torch), '%s: e = %.3f, e_torch = %.3f' % (tag, e, e_torch)
    return e


# ---- eagcn_gemm_f32 -------------------------------------------------------------------------------------------------------------
def _gemm_f32(ta, tb, a, b, lda=None, ldb=None, offset=0):
    lib, L = _lib()
    (M, K), N = a.shape, b.shape[1]
    As, lda = _store(a, ta, POISON, lda, offset)
    Bs, ldb = _store(b, tb, -POISON, ldb, offset)
    Cm, ldc = _output(M, N)
    L.check(lib.eagcn_gemm_f32(ta, tb, M, N, K, _ptr(As), lda, _ptr(Bs), ldb, _ptr(Cm), ldc, _stream()), 'eagcn_gemm_f32')
    return Cm


# (1,1,1) smallest extents | one tile, one k-tile, fewer k-tiles than register stages | scalar loads on both operands, tile edge
# +-1 | vector loads, 6 k-tiles + a 4-wide tail, more k-tiles than stages | the same, scalar | the shape of test_gemm_bf16x6_mode |
# 65 k-tiles: many rounds of the register stages
SHAPES = [(1, 1, 1), (64, 64, 16), (63, 65, 17), (68, 132, 100), (65, 129, 99), (133, 72, 100), (300, 200, 1030)]
# 24 x 23 = 552 tiles of 128 and K >= 1024: the 128x128 tile with three register stages (cfg 3 of launch_gemm), ragged in M, N and K
BIG = (2945, 2817, 1028)
F32_CASES = [(s, f, m) for s in SHAPES for f in FORMS for m in (0, 1)] + [(BIG, f, 0) for f in ((0, 1), (1, 0))]


@pytest.mark.parametrize('shape,form,gemm_mode', F32_CASES, indirect=['gemm_mode'],
                         ids=['%dx%dx%d-%d%d-mode%d' % (s + f + (m,)) for s, f, m in F32_CASES])
def test_gemm_f32_vs_float64(shape, form, gemm_mode):
    a, b, ref, den, e_torch = _case(*shape)
    Cm = _gemm_f32(form[0], form[1], a, b)
    _held(Cm, shape[0], shape[1], ref, den, e_torch, shape[2], 'gemm_f32 %s form %s mode %d' % (shape, form, gemm_mode))


@pytest.mark.parametrize('layout', ['ld_not_multiple_of_4', 'base_off_by_one_float'])
@pytest.mark.parametrize('gemm_mode', [0, 1], indirect=True, ids=['mode0', 'mode1'])
@pytest.mark.parametrize('form', FORMS, ids=['%d%d' % f for f in FORMS])
def test_gemm_f32_scalar_branch_by_layout_alone(form, gemm_mode, layout):
    """(68, 132, 100) takes float4 loads; a leading dimension that is not a multiple of 4, or a base one float off 16-byte
    alignment, alone switch both operands to the scalar branch: still held to float64, and no further from the aligned run."""
    shape = (68, 132, 100)
    a, b, ref, den, e_torch = _case(*shape)
    ta, tb = form
    aligned = _gemm_f32(ta, tb, a, b)
    if layout == 'ld_not_multiple_of_4':
        ca, cb = (shape[0] if ta else shape[2]), (shape[2] if tb else shape[1])      # contiguous extents of the two storages
        lda, ldb = (c + 5 + ((c + 5) % 4 == 0) for c in (ca, cb))
        assert lda % 4 and ldb % 4
        Cm = _gemm_f32(ta, tb, a, b, lda=lda, ldb=ldb)
    else:
        Cm = _gemm_f32(ta, tb, a, b, offset=1)
    tag = 'gemm_f32 %s form %s mode %d %s' % (shape, form, gemm_mode, layout)
    _held(Cm, shape[0], shape[1], ref, den, e_torch, shape[2], tag)
    drift = _measure(Cm[:shape[0], :shape[1]], aligned[:shape[0], :shape[1]].double(), den)
    print('%s: drift from the aligned run %.3f' % (tag, drift))
    assert drift <= max(8.0, 4.0 * e_torch), (drift, e_torch)


# ---- eagcn_gemm_f32_dev ---------------------------------------------------------------------------------------------------------
def _gemm_dev(ta, tb, M, N, K, As, lda, Bs, ldb, Cm, ldc, ext, which):
    lib, L = _lib()
    L.check(lib.eagcn_gemm_f32_dev(ta, tb, M, N, K, _ptr(As), lda, _ptr(Bs), ldb, _ptr(Cm), ldc, _ptr(ext), which, _stream()),
            'eagcn_gemm_f32_dev')


@pytest.mark.parametrize('form', FORMS, ids=['%d%d' % f for f in FORMS])
def test_gemm_f32_dev_row_extent(form, gemm_mode):
    """which = 0: the row count of A and C comes from device memory, rewritten between launches without a host synchronisation
    (250 is clamped to the capacity).  The rows of A at and beyond the extent are poisoned (columns of its storage when ta = 1);
    the rows of C below it match float64, the rows at and beyond it are not written."""
    M, N, K = 200, 72, 40
    ta, tb = form
    a, b, ref, den, _ = _case(M, N, K)
    As, lda = _store(a, ta, POISON)
    Bs, ldb = _store(b, tb, -POISON)
    ext = torch.zeros(1, dtype=torch.int32, device='cuda')
    launches = []
    for x in (0, 1, 64, 65, 137, 200, 250):
        rows = min(x, M)
        Ax = As.clone()
        if ta:
            Ax[:, rows:M] = POISON
        else:
            Ax[rows:M] = POISON
        Cm, ldc = _output(M, N)
        ext.fill_(x)
        _gemm_dev(ta, tb, M, N, K, Ax, lda, Bs, ldb, Cm, ldc, ext, 0)
        launches.append((x, rows, Ax, Cm))
    for x, rows, _, Cm in launches:
        e_torch = _measure(torch.matmul(a[:rows], b), ref[:rows], den[:rows]) if rows else 0.0
        _held(Cm, rows, N, ref, den, e_torch, K, 'gemm_f32_dev rows %d of %d form %s' % (x, M, form))


@pytest.mark.parametrize('form', FORMS, ids=['%d%d' % f for f in FORMS])
def test_gemm_f32_dev_reduction_extent(form, gemm_mode):
    """which = 2: the reduction length comes from device memory (400 is clamped to the capacity 300).  The entries of both
    operands at k >= extent are poisoned; C is completely written and equals the float64 product over the first `extent` k's --
    element by element also where a K-contiguous operand (ta = 0, tb = 1) is read as float4 and the extent ends inside one;
    extent 0 gives exact zeros."""
    M, N, K = 68, 72, 300
    ta, tb = form
    a, b, _, _, _ = _case(M, N, K)
    As, lda = _store(a, ta, POISON)
    Bs, ldb = _store(b, tb, -POISON)
    ext = torch.zeros(1, dtype=torch.int32, device='cuda')
    launches = []
    for x in (0, 1, 3, 16, 17, 127, 128, 130, 300, 400):
        kx = min(x, K)
        Ax, Bx = As.clone(), Bs.clone()
        if ta:
            Ax[kx:K] = POISON
        else:
            Ax[:, kx:K] = POISON
        if tb:
            Bx[:, kx:K] = -POISON
        else:
            Bx[kx:K] = -POISON
        Cm, ldc = _output(M, N)
        ext.fill_(x)
        _gemm_dev(ta, tb, M, N, K, Ax, lda, Bx, ldb, Cm, ldc, ext, 2)
        launches.append((x, kx, Ax, Bx, Cm))
    failed = []
    for x, kx, _, _, Cm in launches:
        tag = 'gemm_f32_dev k %d of %d form %s' % (x, K, form)
        if kx == 0:
            assert torch.equal(Cm[:M, :N], torch.zeros(M, N, device='cuda')), '%s: an empty reduction must give exact zeros' % tag
            assert torch.isnan(Cm[M:]).all() and torch.isnan(Cm[:, N:]).all(), tag
            continue
        ref, den, e_torch = _reference(a[:, :kx].contiguous(), b[:kx].contiguous())
        try:
            _held(Cm, M, N, ref, den, e_torch, kx, tag)
        except AssertionError as err:                    # (every extent is reported, not only the first that fails)
            failed.append(str(err))
    assert not failed, '\n'.join(failed)


# ---- eagcn_gemm_f32_sk ----------------------------------------------------------------------------------------------------------
SK_FORMS = [(0, 0), (0, 1), (1, 0)]
SK_SHAPES = [(4, 4, 4), (64, 64, 16), (68, 132, 100), (1000, 256, 80), (36, 128, 144), (128, 16, 4000)]


@functools.lru_cache(maxsize=1)
def _workspace():
    """eagcn_gemm_sk_workspace_bytes() of scratch that need not be initialised: filled once with a byte pattern that is neither
    a clean flag nor a plausible partial tile"""
    lib, _ = _lib()
    return torch.full((int(lib.eagcn_gemm_sk_workspace_bytes()),), 0xA5, dtype=torch.uint8, device='cuda')


def _gemm_sk(ta, tb, M, N, K, As, lda, Bs, ldb, Cm, ldc):
    lib, _ = _lib()
    ws = _workspace()
    return lib.eagcn_gemm_f32_sk(ta, tb, M, N, K, _ptr(As), lda, _ptr(Bs), ldb, _ptr(Cm), ldc, _ptr(ws), ws.numel(), _stream())


@pytest.mark.parametrize('form', SK_FORMS, ids=['%d%d' % f for f in SK_FORMS])
@pytest.mark.parametrize('shape', SK_SHAPES, ids=['%dx%dx%d' % s for s in SK_SHAPES])
def test_gemm_f32_sk_vs_float64(shape, form):
    """The single balanced product: extents and leading dimensions are multiples of 4 and the bases 16-byte aligned (the entry
    needs that), so only the slack is poisoned.  Three launches on one workspace that was never cleared: every launch leaves the
    hand-off flags clean for the next, each result is held to float64, and no hand-off times out."""
    lib, L = _lib()
    M, N, K = shape
    ta, tb = form
    a, b, ref, den, e_torch = _case(M, N, K)
    As, lda = _store(a, ta, POISON)
    Bs, ldb = _store(b, tb, -POISON)
    for rep in range(3):
        Cm, ldc = _output(M, N, ldc=_up4(N) + 4)
        L.check(_gemm_sk(ta, tb, M, N, K, As, lda, Bs, ldb, Cm, ldc), 'eagcn_gemm_f32_sk')
        _held(Cm, M, N, ref, den, e_torch, K, 'gemm_f32_sk %s form %s launch %d' % (shape, form, rep))
    assert lib.eagcn_gemm_sk_timeouts() == 0 and lib.eagcn_gemm_sk_failed() == 0


@pytest.mark.parametrize('ta,tb,M,N,K,offset', [(1, 1, 64, 64, 16, 0), (0, 1, 64, 64, 18, 0), (1, 0, 66, 64, 16, 0), (1, 0, 64, 66, 16, 0),
                                                (0, 1, 64, 64, 16, 1), (1, 0, 64, 64, 16, 1), (0, 0, 64, 64, 18, 0), (0, 0, 64, 66, 16, 0),
                                                (0, 0, 64, 64, 16, 1)],
                         ids=['TT', 'NT_K18', 'TN_M66', 'TN_N66', 'NT_misaligned', 'TN_misaligned', 'NN_K18', 'NN_N66', 'NN_misaligned'])
def test_gemm_f32_sk_refuses_what_it_cannot_load(ta, tb, M, N, K, offset):
    """The balanced kernel loads float4 without predication: the (1,1) form, a contiguous extent that is not a multiple of 4 and a
    misaligned base are refused with an error (never run on another path), and C is left untouched."""
    lib, L = _lib()
    a, b, _, _, _ = _case(M, N, K)
    As, lda = _store(a, ta, POISON, offset=offset)
    Bs, ldb = _store(b, tb, -POISON, offset=offset)
    assert lda % 4 == 0 and ldb % 4 == 0
    Cm, ldc = _output(M, N, ldc=_up4(N) + 4)
    with pytest.raises(L.EagcnHipError):
        L.check(_gemm_sk(ta, tb, M, N, K, As, lda, Bs, ldb, Cm, ldc), 'eagcn_gemm_f32_sk')
    torch.cuda.synchronize()
    assert torch.isnan(Cm).all(), 'a refused product wrote to C'
    assert lib.eagcn_gemm_sk_timeouts() == 0 and lib.eagcn_gemm_sk_failed() == 0
