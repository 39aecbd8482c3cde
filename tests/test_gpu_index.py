"""The batch index (eagcn_amd/csrc/index.hip) against its numpy reference (tests/index_reference.py), buffer by buffer.

Every array of the index is an integer function of the 0/1 adjacency and the one-hot relation tensors, so every comparison here
is equality: no tolerance, no skipped case.  The batches are built to reach what molecule-shaped inputs never reach: a clique
whose rows fill three gather passes of one wavefront, adjacency tensors at every load width (by N and by a misaligned base),
both bond-list kernels and the LDS opt-in boundary, the 64-molecule chunks, the solo runs and the 16-molecule cap of the row-block
builder, static buffers that still hold a larger batch, capacities that do not fit, and inputs that must be rejected."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                   # (run as a script by the legacy-scan case)
    sys.path.insert(0, ROOT)

from eagcn_amd import _lib as L
from index_reference import compare_index, densify, read_index, reference_index, reference_index_from_bonds

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _rpw(N):
    """Rows one wavefront of the streaming scan takes."""
    return 8 if N <= 256 else (4 if N <= 512 else 2)


def _clique_size(N):
    return 20 if N <= 256 else (40 if N <= 512 else 70)


def _chain(atoms):
    s = set()
    for a, b in zip(atoms[:-1], atoms[1:]):
        s |= {(a, b), (b, a)}
    return s


def _bond_arrays(mols, channels, rng):
    bm, bi, bj = [], [], []
    for b, m in enumerate(mols):
        for i, j in sorted(m):
            bm.append(b), bi.append(i), bj.append(j)
    bm, bi, bj = (np.asarray(a, dtype=np.int64) for a in (bm, bi, bj))
    bc = np.stack([rng.integers(0, c, size=len(bm)) for c in channels], axis=1).astype(np.int64)
    if len(bm):
        bc[0] = [c - 1 for c in channels]                    # the largest code of every view occurs
    return bm, bi, bj, bc


def adversarial(N, channels, seed=0, n_rand=2):
    """One batch (B <= 20) that holds, at any N that has room for it: a clique block sized to the scan's rows per wave (more than
    128 bonds in one wave's rows: three gather passes) that starts at an atom index no multiple of the rows per wave; a molecule
    without a bond first, in the middle and last; bond-less atoms below nat and trailing; a self loop; a one-directional bond
    into an atom beyond nat; a molecule with nat = N and a bond in the last column."""
    rng = np.random.default_rng(seed)
    start = 3 if N >= 6 else 0
    S = min(_clique_size(N), N - start)
    a = {(i, j) for i in range(start, start + S) for j in range(start, start + S) if i != j}
    a.add((start, start))                                    # a self loop
    if start:
        a |= {(0, 1), (1, 0)}                                # atom 2: no bond, below nat
    if N - 1 >= start + S:
        a.add((0 if start else start, N - 1))                # one-directional, its target beyond nat (and trailing bond-less atoms)
    f = _chain(list(range(min(N, 6)))) | {(0, N - 1), (N - 1, 0)} if N > 1 else {(0, 0)}
    mols = [set(), a]
    if N <= 512:
        s = {(0, 1), (1, 0), (1, 1)} if N >= 2 else {(0, 0)}
        if N >= 4:
            s.add((0, N - 1))                                # nat = 2, target N - 1
        mols.append(s)
    mols += [set(), f]
    for _ in range(n_rand if N <= 512 else 0):
        n = int(rng.integers(1, N + 1))
        atoms = sorted(set(rng.choice(n, size=min(n, 12), replace=False).tolist()) | {n - 1})
        mols.append(_chain(atoms) if len(atoms) > 1 else {(n - 1, n - 1)})
    mols.append(set())
    assert len(mols) <= 20
    bm, bi, bj, bc = _bond_arrays(mols, channels, rng)
    return dict(B=len(mols), N=N, channels=list(channels), bm=bm, bi=bi, bj=bj, bc=bc)


def sized(sizes, N, channels, seed=0):
    """Chain molecules of the given atom counts (0: no bond, 1: a self loop): the input of the row-block builder."""
    rng = np.random.default_rng(seed)
    mols = [set() if n == 0 else ({(0, 0)} if n == 1 else _chain(list(range(n)))) for n in sizes]
    bm, bi, bj, bc = _bond_arrays(mols, channels, rng)
    return dict(B=len(mols), N=N, channels=list(channels), bm=bm, bi=bi, bj=bj, bc=bc)


def _views_for(N):
    return (5, 3, 2) if N <= 256 else ((3, 2) if N <= 600 else (2, 1))


def _dense(fx):
    return densify(fx['B'], fx['N'], fx['channels'], fx['bm'], fx['bi'], fx['bj'], fx['bc'])


def _wave_totals(adj):
    B, N, _ = adj.shape
    per_row = (adj.reshape(B * N, N) != 0).sum(axis=1)
    rpw = _rpw(N)
    pad = (-len(per_row)) % rpw
    return np.concatenate([per_row, np.zeros(pad, dtype=per_row.dtype)]).reshape(-1, rpw).sum(axis=1)


def _wave_position(adj, b, i, j):
    """Position of bond (b, i, j) in the bond list of the wavefront that scans its row."""
    B, N, _ = adj.shape
    flat = adj.reshape(B * N, N) != 0
    g = b * N + i
    w0 = g // _rpw(N) * _rpw(N)
    return int(flat[w0:g].sum() + flat[g, :j].sum())


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device='cuda', dtype=dtype) if dtype is not None else t.cuda()


def _bond_tensors(fx, perm=None):
    perm = np.arange(len(fx['bm'])) if perm is None else perm
    return (_cuda(fx['bm'][perm], torch.int32), _cuda(fx['bi'][perm], torch.int32), _cuda(fx['bj'][perm], torch.int32),
            _cuda(fx['bc'][perm], torch.uint8))


def check_batch(fx, adj_dev=None, dense=None):
    """Eager index from the dense tensors, then from the same molecules as a shuffled bond list: both equal to the reference."""
    from eagcn_amd import ops
    adj, rels = dense if dense is not None else _dense(fx)
    want = reference_index(adj, rels)
    ta = adj_dev if adj_dev is not None else _cuda(adj)
    idx = ops.BatchIndex(ta, [_cuda(r) for r in rels], bond_lists=True)
    torch.cuda.synchronize()
    compare_index(read_index(idx), want)
    del idx
    perm = np.random.default_rng(5).permutation(len(fx['bm']))
    idc = ops.BatchIndex.from_bonds(fx['B'], fx['N'], fx['channels'], *_bond_tensors(fx, perm), bond_lists=True)
    torch.cuda.synchronize()
    wantc = reference_index_from_bonds(fx['B'], fx['N'], fx['channels'], fx['bm'][perm], fx['bi'][perm], fx['bj'][perm], fx['bc'][perm])
    compare_index(read_index(idc), wantc)
    return want


SWEEP = (1, 5, 16, 33, 34, 36, 132, 222, 256, 257, 258, 300, 512, 513, 600, 1024)


@pytest.mark.parametrize('N', SWEEP)
def test_index_equals_reference_over_n(N):
    """NIT 1 / 2 / 4, adjacency loads of 16 / 8 / 4 bytes by N, ldc = N and ldc > N, both bond-list kernels, the dynamic-LDS
    opt-in (N = 512).  Above N = 512 the batch has five molecules and two narrow views, so the input stays below 100 MB."""
    fx = adversarial(N, _views_for(N), seed=N)
    dense = _dense(fx)
    if N >= 33:                                              # the fixture does what it is for: a wave with three gather passes
        assert _wave_totals(dense[0]).max() > 128
    want = check_batch(fx, dense=dense)
    assert want['nat'][0] == 0 and want['nat'][-1] == 0 and (want['nat'][2:-2] == 0).any() and want['nat'].max() == N


@pytest.mark.parametrize('N,offset', [(36, 1), (36, 2), (132, 1), (132, 2), (260, 1), (260, 2), (34, 1)])
def test_index_with_a_misaligned_adjacency(N, offset):
    """N % 4 == 0 with the adjacency at a storage offset of 1 or 2 floats: 4- and 8-byte loads chosen from the base pointer."""
    fx = adversarial(N, _views_for(N), seed=100 + N)
    dense = _dense(fx)
    n = fx['B'] * N * N
    flat = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
    view = flat[offset:offset + n].view(fx['B'], N, N)
    view.copy_(_cuda(dense[0]))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    check_batch(fx, adj_dev=view, dense=dense)


@pytest.mark.parametrize('channels', [(3,), (3, 2, 2, 2, 2, 2, 2, 1), (255, 4, 2, 2, 2), (64, 1)],
                         ids=['K1', 'K8', 'c255', 'c64_1'])
def test_index_over_views(channels):
    """One view, EAGCN_MAX_VIEWS views, a channel list longer than one wave with codes up to 255, a view boundary at lane 64."""
    want = check_batch(adversarial(33, channels, seed=len(channels)))
    assert want['code'][0].max() == channels[0]


BLOCK_BATCHES = {
    'tiny1': ([2], 4), 'tiny16': ([1, 2, 3, 4] * 4, 4), 'tiny17': ([1, 2, 3, 4] * 4 + [2], 4),
    'tiny64': ([2, 1, 4, 3] * 16, 4), 'tiny65': ([2, 1, 4, 3] * 16 + [1], 4), 'tiny130': ([3, 1, 2, 4, 2] * 26, 4),
    'zeros': ([0] * 20 + [1] + [0] * 17 + [2, 0], 4),
    # {200, 56} and {1, 255}: exactly 256 rows; {200} + 57 would be 257; {57, 199}; a full molecule; a block closed by the cap
    'rows256_257': ([200, 56, 1, 255, 200, 57, 199, 128, 128, 256, 255, 1, 1] + [1] * 18, 256),
    # molecules 61 .. 67 cannot pair with their successors: a solo run across the 64-molecule chunk boundary
    'solo_run': ([3] * 61 + [130] * 7 + [3] * 4, 132),
    'solo_run_only': ([130] * 66, 132),
    'over256': ([5, 300, 5, 0, 290, 10], 300),
}


@pytest.mark.parametrize('name', list(BLOCK_BATCHES))
def test_row_blocks_and_lists_over_batch_shapes(name):
    sizes, N = BLOCK_BATCHES[name]
    want = check_batch(sized(sizes, N, (2, 1), seed=len(sizes)))
    assert want['nat'].tolist() == sizes


# ---- static buffers (graph.StaticIndex) through ops.index_build ---------------------------------------------------------------
def _static(B, N_cap, channels):
    from eagcn_amd.graph import StaticIndex
    idx = StaticIndex(B, N_cap, list(channels), torch.device('cuda', 0), B * N_cap, edge_cap=8 * B * N_cap + 4096)
    idx.c.build_lists = 1
    assert idx.c.blk
    return idx


def _build(idx, adj, rels, n_logical, bonds=None, rows=True):
    from eagcn_amd import ops
    host = torch.zeros(L.META_WORDS, dtype=torch.int32).pin_memory()
    idx.c.n_logical = int(n_logical)                         # as GraphRunner._prepare sets it: 0 when the batch has the capacity's size
    ops.index_build(idx.c, adj, rels, bonds, host, ops._stream(), rows=rows)
    torch.cuda.synchronize()
    return host.tolist()


@pytest.mark.parametrize('Nin,N_cap', [(36, 48), (34, 48), (33, 48), (222, 300)])
def test_static_buffers_hold_no_stale_batch(Nin, N_cap):
    """A large batch, then a smaller one with n_logical = Nin < N_cap (Nin % 4 = 0, 2, 1, and a scan with fewer column trips than
    the capacity has) into the SAME buffers, dense and compact: the second equals its reference on every defined field."""
    ch = (5, 3, 2)
    big = adversarial(N_cap, ch, seed=7, n_rand=3)
    small = adversarial(Nin, ch, seed=8, n_rand=3)
    assert small['B'] == big['B']
    idx = _static(big['B'], N_cap, ch)
    for compact in (False, True):
        adj, rels = _dense(big)
        meta = _build(idx, _cuda(adj), [_cuda(r) for r in rels], 0)
        want = reference_index(adj, rels)
        assert meta[:10] == want['meta'][:10].tolist()[:9] + [0]          # (the host copy leaves before the row blocks are counted)
        compare_index(read_index(idx), want)
        if compact:
            meta = _build(idx, None, None, Nin, bonds=_bond_tensors(small))
            want = reference_index_from_bonds(small['B'], Nin, ch, small['bm'], small['bi'], small['bj'], small['bc'], N_cap=N_cap)
        else:
            adj, rels = _dense(small)
            meta = _build(idx, _cuda(adj), [_cuda(r) for r in rels], Nin)
            want = reference_index(adj, rels, N_cap=N_cap)
        assert want['meta'][L.META_NLOG] == Nin and meta[L.META_NLOG] == Nin
        compare_index(read_index(idx), want)


def _fill(idx):
    for t in (idx._blob, idx._rows, idx._ptrs, idx._edges):
        t.fill_(SENTINEL)
    idx.code.fill_(0x5A)


def _region(idx, t, field):
    """Host words of tensor t from the Batch struct's pointer `field` to the end of t."""
    off = getattr(idx.c, field) - t.data_ptr()
    assert off >= 0 and off % 4 == 0
    return t.cpu().numpy()[off // 4:]


@pytest.mark.parametrize('which', ['rows', 'edges'])
def test_capacity_overflow_is_indexed_as_empty(which):
    """The struct's capacity (T or E) one below what the batch needs, the allocations large enough for all of it, every buffer
    pre-filled with a sentinel: the batch is indexed as empty, the count and the message are the documented ones, and nothing
    at or beyond the stated capacity -- and nothing of the lists and blocks -- is written."""
    ch = (5, 3, 2)
    fx = adversarial(33, ch, seed=21, n_rand=3)
    adj, rels = _dense(fx)
    want = reference_index(adj, rels)
    T, NE, B = int(want['meta'][L.META_T]), int(want['meta'][L.META_NEDGE]), fx['B']
    idx = _static(B, 33, ch)
    T_alloc, E_alloc = int(idx.c.T), int(idx.c.E)
    assert T_alloc > T and E_alloc > NE
    _fill(idx)
    if which == 'rows':
        idx.c.T = T - 1
    else:
        idx.c.E = NE - 1
    meta = _build(idx, _cuda(adj), [_cuda(r) for r in rels], 0)
    assert meta[L.META_T] == 0 and meta[L.META_NTILES] == 0
    assert meta[L.META_NEDGE] == NE and meta[L.META_NMAX] == 33
    msg = L.index_error(meta, row_cap=int(idx.c.T), edge_cap=int(idx.c.E))
    if which == 'rows':
        assert meta[L.META_OVERFLOW] == T and meta[L.META_EDGE_OVERFLOW] == 0
        assert msg == '%d packed rows, more than row_cap=%d (the batch is indexed as an empty batch; no memory is overwritten)' % (T, T - 1)
    else:
        assert meta[L.META_OVERFLOW] == 0 and meta[L.META_EDGE_OVERFLOW] == NE
        assert msg == '%d directed bonds, more than edge_cap=%d (the batch is indexed as an empty batch; no memory is overwritten)' % (NE, NE - 1)
    # the small arrays are those of the batch itself
    blob_lay, rows_lay = L.index_layout(B, 33, T_alloc, int(idx.c.n_tiles))
    blob = idx._blob.cpu().numpy()
    for name in ('nat', 'row0', 'edge0', 'ecnt'):
        assert np.array_equal(blob[blob_lay[name]], want[name]), name
    assert blob[blob_lay['meta']][L.META_NBLK] == 0
    # per-row arrays: nothing at or beyond the stated row capacity (and nothing beyond the batch's own rows)
    cap = min(int(idx.c.T), T)
    rows = idx._rows.cpu().numpy()
    for name in ('row_mol', 'row_loc', 'row_deg', 'row_m'):
        r = rows[rows_lay[name]]
        assert (r[cap:] == SENTINEL).all(), name
        assert (r[:cap] != SENTINEL).all(), name
    assert np.array_equal(rows[rows_lay['row_mol']][:cap], want['row_mol'][:cap])
    assert (rows[rows_lay['row_info']][4 * cap:] == SENTINEL).all()
    NT = int(want['meta'][L.META_NTILES])
    assert (rows[rows_lay['tile_mol']][NT:] == SENTINEL).all() and (rows[rows_lay['tile_info']][4 * NT:] == SENTINEL).all()
    # molecules whose rows do not fit are empty to every consumer of mol_info
    mol = _region(idx, idx._ptrs, 'mol_info')[:4 * B].reshape(B, 4)
    fit = want['row0'][:B] + want['nat'] <= int(idx.c.T)
    assert np.array_equal(mol[:, 0], np.where(fit, want['nat'], 0)) and np.array_equal(mol[:, 1:], want['mol_info'][:, 1:])
    # lists and blocks: untouched
    ptrs = idx._ptrs.cpu().numpy()
    mol_off = (idx.c.mol_info - idx._ptrs.data_ptr()) // 4
    assert (ptrs[:mol_off] == SENTINEL).all(), 'row_ptr / col_ptr'
    assert (_region(idx, idx._ptrs, 'blk') == SENTINEL).all(), 'blk'
    assert (idx._edges.cpu().numpy() == SENTINEL).all(), 'nbr / tnbr / ecode / tcode'
    # ... and the same buffers take the batch once the capacity is back
    idx.c.T, idx.c.E = T_alloc, E_alloc
    _build(idx, _cuda(adj), [_cuda(r) for r in rels], 0)
    compare_index(read_index(idx), want)


def _third_pass_bond(adj, b):
    N = adj.shape[1]
    for i in range(N):
        for j in np.nonzero(adj[b, i])[0]:
            if _wave_position(adj, b, i, int(j)) >= 128:
                return i, int(j)
    raise AssertionError('no bond in a third gather pass')


def _counters(fx, adj, rels):
    from eagcn_amd import ops
    idx = _static(fx['B'], fx['N'], fx['channels'])
    ta, tr = _cuda(adj), [_cuda(r) for r in rels]
    meta = _build(idx, ta, tr, 0, rows=False)
    want = reference_index(adj, rels)['meta']
    assert (meta[L.META_BAD_ADJ], meta[L.META_BAD_REL]) == (int(want[L.META_BAD_ADJ]), int(want[L.META_BAD_REL]))
    with pytest.raises(L.EagcnHipError):
        ops.BatchIndex(ta, tr, bond_lists=True)
    return meta


def test_rejected_adjacency_entries_are_counted_exactly():
    """A 0.5 in the last column of an odd N and a NaN inside the clique block."""
    fx = adversarial(33, (70, 3), seed=31)
    adj, rels = _dense(fx)
    adj[4, 5, 32] = 0.5                                      # a new "bond": also zero-hot in both views
    meta = _counters(fx, adj, rels)
    assert meta[L.META_BAD_ADJ] == 1 and meta[L.META_BAD_REL] == 2
    i, j = _third_pass_bond(adj, 1)
    adj[1, i, j] = np.nan                                    # on a bond of the clique: its relation channels stay one-hot
    meta = _counters(fx, adj, rels)
    assert meta[L.META_BAD_ADJ] == 2 and meta[L.META_BAD_REL] == 2


def test_rejected_relation_entries_are_counted_exactly():
    """Two-hot with the second 1 in a channel >= 64, zero-hot, and a 0.5 on a bond that falls into the third gather pass."""
    fx = adversarial(33, (70, 3), seed=32)
    adj, rels = _dense(fx)
    i, j = _third_pass_bond(adj, 1)
    hot = int(rels[0][1, :, i, j].argmax())
    rels[0][1, hot, i, j] = 0.5
    assert _counters(fx, adj, rels)[L.META_BAD_REL] == 1
    b2, i2, j2 = (int(v) for v in np.argwhere(adj != 0)[0])
    hot = int(rels[0][b2, :, i2, j2].argmax())
    rels[0][b2, 69 if hot != 69 else 68, i2, j2] = 1.0       # two-hot
    b3, i3, j3 = (int(v) for v in np.argwhere(adj != 0)[-1])
    rels[1][b3, :, i3, j3] = 0.0                             # zero-hot
    meta = _counters(fx, adj, rels)
    assert meta[L.META_BAD_ADJ] == 0 and meta[L.META_BAD_REL] == 3


def test_legacy_scan_equals_reference():
    """EAGCN_SCAN4=0 (read once per process: a subprocess) at N = 33, 132, 300."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '33', '132', '300'], env=dict(os.environ, EAGCN_SCAN4='0'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'LEGACY_SCAN_OK 33 132 300' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- layout conversions on the same arrays ------------------------------------------------------------------------------------
@pytest.mark.parametrize('widths,pads', [((5, 16, 3), (16, 16, 16)), ((24,), (24,))], ids=['three_segments', 'single24'])
def test_layout_conversions_equal_numpy_indexing(widths, pads):
    """ops.pack_rows, ops.unpack_rows with and without pad_row and eagcn_pad_rows, on a batch with molecules of no atoms."""
    from eagcn_amd import ops
    from eagcn_amd.collate import pad_rows
    fx = adversarial(33, (5, 3, 2), seed=41)
    adj, rels = _dense(fx)
    want = reference_index(adj, rels)
    assert (want['nat'] == 0).any()
    B, N, T = fx['B'], 33, int(want['meta'][L.META_T])
    idx = ops.BatchIndex(_cuda(adj), [_cuda(r) for r in rels])
    lay = ops.ColLayout(widths, pads)
    F, ld = sum(widths), sum(pads)
    rng = np.random.default_rng(3)
    dense = rng.standard_normal((B, N, F)).astype(np.float32)
    exact = np.concatenate([np.arange(w) + sum(pads[:s]) for s, w in enumerate(widths)])      # packed column of every exact column
    expect = np.zeros((T, ld), dtype=np.float32)
    expect[:, exact] = dense[want['row_mol'], want['row_loc']]
    assert np.array_equal(ops.pack_rows(idx, lay, _cuda(dense)).cpu().numpy(), expect)
    packed = rng.standard_normal((T, ld)).astype(np.float32)
    pad_row = rng.standard_normal(ld).astype(np.float32)
    for pr in (None, pad_row):
        expect = np.zeros((B, N, F), dtype=np.float32)
        if pr is not None:
            expect[:] = pr[exact]
        for b in range(B):
            n, r0 = int(want['nat'][b]), int(want['row0'][b])
            expect[b, :n] = packed[r0:r0 + n][:, exact]
        got = ops.unpack_rows(idx, lay, _cuda(packed), None if pr is None else _cuda(pr))
        assert np.array_equal(got.cpu().numpy(), expect)
    rows = rng.standard_normal((T, F)).astype(np.float32)
    expect = np.zeros((B, N, F), dtype=np.float32)
    for b in range(B):
        n, r0 = int(want['nat'][b]), int(want['row0'][b])
        expect[b, :n] = rows[r0:r0 + n]
    got = pad_rows(_cuda(rows), _cuda(want['row0']), B, N)
    assert np.array_equal(got.cpu().numpy(), expect)


if __name__ == '__main__':                                   # the legacy-scan case: EAGCN_SCAN4 is read once per process
    assert os.environ.get('EAGCN_SCAN4') == '0'
    for n in (int(a) for a in sys.argv[1:]):
        check_batch(adversarial(n, _views_for(n), seed=n))
    print('LEGACY_SCAN_OK ' + ' '.join(sys.argv[1:]))
