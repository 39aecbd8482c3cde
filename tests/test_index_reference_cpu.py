"""tests/index_reference.py must not be the thing that is wrong: the numpy reference of the batch index against brute force
(plain loops over the adjacency), against the invariants of the row blocks, against hand-written block answers, and its dense
and compact entry points against each other."""
import numpy as np
import pytest

from eagcn_amd import _lib as L
from eagcn_amd.collate import compact_host
from eagcn_amd.synthetic import make_batch
from index_reference import (compare_index, densify, pack_blocks, reference_index, reference_index_from_bonds)
from test_collate_cpu import _load


def _random_dense(seed, B=5, N=11, channels=(5, 3), density=0.3):
    """Directed 0/1 adjacency with self loops, bond-less atoms below nat, trailing bond-less atoms and an empty molecule."""
    rng = np.random.default_rng(seed)
    adj = (rng.random((B, N, N)) < density).astype(np.float32)
    adj[:, rng.integers(0, N // 2)] = 0                     # a bond-less row below nat (columns may still point at it)
    for b in range(B):
        n = int(rng.integers(1, N + 1))
        adj[b, n:] = 0                                      # rows beyond n: no bonds; columns beyond n stay (one-directional bonds out of nat)
    adj[B // 2] = 0                                         # a molecule without a bond
    adj[0, 1, 1] = 1
    rels = []
    for c in channels:
        t = rng.integers(0, c, size=(B, N, N))
        r = np.zeros((B, c, N, N), dtype=np.float32)
        for ch in range(c):
            r[:, ch] = (t == ch) * adj
        rels.append(r)
    return adj, rels


@pytest.mark.parametrize('seed', range(6))
def test_reference_against_brute_force(seed):
    adj, rels = _random_dense(seed)
    B, N, _ = adj.shape
    K = len(rels)
    ref = reference_index(adj, rels)
    assert ref['meta'][L.META_BAD_ADJ] == 0 and ref['meta'][L.META_BAD_REL] == 0
    e0 = 0
    r0 = 0
    for b in range(B):
        deg = [sum(1 for j in range(N) if adj[b, i, j] != 0) for i in range(N)]
        assert ref['deg_bn'][b].tolist() == deg
        nat = max([i + 1 for i in range(N) if deg[i] > 0], default=0)
        assert ref['nat'][b] == nat and ref['ecnt'][b] == sum(deg)
        assert ref['row0'][b] == r0 and ref['edge0'][b] == e0
        assert ref['mol_info'][b].tolist() == [nat, r0, e0, sum(deg)]
        bi, bj = np.nonzero(adj[b, :nat, :nat])
        listed = 0
        run = e0
        for i in range(nat):
            first, cnt = ref['row_ptr'][r0 + i]
            js = bj[bi == i]
            assert first == run and cnt == len(js), (b, i)
            assert ref['nbr'][first:first + cnt].tolist() == js.tolist()
            assert ref['listed'][first:first + cnt].all()
            for e, j in zip(range(first, first + cnt), js):
                want = sum((int(np.argmax(rels[k][b, :, i, j])) + 1) << (8 * k) for k in range(K))
                assert int(ref['ecode'][e]) == want
                assert [int(ref['code'][k, b, i, j]) for k in range(K)] == [(want >> (8 * k)) & 255 for k in range(K)]
            run += cnt
            listed += cnt
            assert ref['row_info'][r0 + i].tolist() == [b, i, nat, r0]
            assert ref['row_deg'][r0 + i] == deg[i] and ref['row_m'][r0 + i] == (1.0 if deg[i] else 0.0)
        assert listed == int(adj[b, :nat, :nat].sum())
        assert listed <= sum(deg)
        # the transpose: rows ascending per column, and the same bond carries the same code word
        ti, tj = np.nonzero(adj[b, :nat, :nat].T)               # (column, row) pairs, column-major
        run = e0
        for j in range(nat):
            first, cnt = ref['col_ptr'][r0 + j]
            is_ = tj[ti == j]
            assert first == run and cnt == len(is_), (b, j)
            assert ref['tnbr'][first:first + cnt].tolist() == is_.tolist()
            for e, i in zip(range(first, first + cnt), is_):
                f2, c2 = ref['row_ptr'][r0 + i]
                at = f2 + ref['nbr'][f2:f2 + c2].tolist().index(j)
                assert ref['tcode'][e] == ref['ecode'][at]
            run += cnt
        assert int(ref['tlisted'].sum()) == int(ref['listed'].sum())
        r0 += nat
        e0 += sum(deg)
    assert ref['meta'][L.META_T] == r0 and ref['meta'][L.META_NEDGE] == e0
    assert ref['meta'][L.META_NMAX] == ref['nat'].max()
    assert ref['meta'][L.META_NTILES] == sum((int(n) + 15) // 16 for n in ref['nat'])
    assert ref['code'].shape == (K, B, N, (N + 15) // 16 * 16) and not ref['code'][..., N:].any()
    assert ((ref['code'][0, :, :N, :N] != 0) == (adj != 0)).all()


def test_reference_counts_rejected_entries():
    adj, rels = _random_dense(9)
    bonds = np.argwhere(adj == 1)
    adj[tuple(bonds[0])] = 0.5                                 # (its relation channels stay one-hot)
    adj[1, 0, 3] = np.nan                                      # a NaN is a bond, and a bad one
    for r in rels:
        r[1, :, 0, 3] = 0
        r[1, 0, 0, 3] = 1
    (b, i, j), (b2, i2, j2), (b3, i3, j3) = bonds[1], bonds[2], bonds[-1]
    rels[0][b, :, i, j] = 0                                    # zero-hot
    rels[1][b2, :, i2, j2] = 1                                 # all-hot
    rels[0][b3, :, i3, j3] *= 0.5                              # the right channel, the wrong value
    rels[1][0, 1, 4, 4] += 7 * (adj[0, 4, 4] == 0)             # off the bonds nothing is looked at
    ref = reference_index(adj, rels)
    assert ref['meta'][L.META_BAD_ADJ] == 2
    assert ref['meta'][L.META_BAD_REL] == 3


def _check_block_invariants(nat, edge0, blk, rb=256, maxm=16):
    B = len(nat)
    nb = len(blk) // 2
    row0 = np.concatenate(([0], np.cumsum(nat)))
    nxt = 0
    for q in range(nb):
        first, cnt, r0, rows = (int(v) for v in blk[2 * q])
        e_first, e_cnt, z0, z1 = (int(v) for v in blk[2 * q + 1])
        assert first == nxt and cnt >= 1                          # whole molecules, contiguous
        nxt = first + cnt
        assert cnt <= maxm
        assert rows <= rb or cnt == 1
        assert r0 == row0[first] and rows == sum(int(n) for n in nat[first:nxt])
        assert e_first == edge0[first] and e_cnt == edge0[nxt] - edge0[first] and z0 == 0 and z1 == 0
        if nxt < B:                                              # maximal: the next molecule would not have fitted
            assert rows + int(nat[nxt]) > rb or cnt + 1 > maxm
    assert nxt == (B if nb else 0)                               # covering 0 .. B exactly once


@pytest.mark.parametrize('seed', range(8))
def test_block_invariants_on_random_sizes(seed):
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 200))
    nat = rng.choice([0, 1, 2, 7, 16, 40, 100, 128, 129, 200, 256, 300], size=B)
    ecnt = 2 * nat
    edge0 = np.concatenate(([0], np.cumsum(ecnt)))
    for rb, maxm in ((256, 16), (64, 16), (256, 3)):
        _check_block_invariants(nat, edge0, pack_blocks(nat, edge0, rb, maxm), rb, maxm)


def _blocks_of(sizes):
    nat = np.asarray(sizes)
    edge0 = np.concatenate(([0], np.cumsum(3 * nat)))
    blk = pack_blocks(nat, edge0)
    _check_block_invariants(nat, edge0, blk)
    return [(int(blk[2 * q][0]), int(blk[2 * q][1])) for q in range(len(blk) // 2)]


def test_block_corner_cases():
    assert _blocks_of([1] * 17) == [(0, 16), (16, 1)]
    assert _blocks_of([200, 56, 1]) == [(0, 2), (2, 1)]
    assert _blocks_of([200, 57]) == [(0, 1), (1, 1)]
    assert _blocks_of([5, 300, 5]) == [(0, 1), (1, 1), (2, 1)]
    assert _blocks_of([0] * 20) == [(0, 16), (16, 4)]                       # molecules without atoms count as molecules
    assert _blocks_of([256, 0, 0, 1]) == [(0, 3), (3, 1)]
    assert _blocks_of([300, 0, 4]) == [(0, 1), (1, 2)]                      # nothing joins a block that is already over
    assert _blocks_of([1] * 65) == [(0, 16), (16, 16), (32, 16), (48, 16), (64, 1)]
    assert _blocks_of([1] * 129) == [(16 * q, 16) for q in range(8)] + [(128, 1)]
    assert _blocks_of([130] * 65) == [(q, 1) for q in range(65)]
    assert _blocks_of([120] * 129) == [(2 * q, 2) for q in range(64)] + [(128, 1)]


def test_reference_of_an_empty_batch():
    adj = np.zeros((3, 5, 5), dtype=np.float32)
    ref = reference_index(adj, [np.zeros((3, 2, 5, 5), dtype=np.float32)])
    assert ref['meta'][L.META_T] == 0 and ref['meta'][L.META_NBLK] == 0 and len(ref['blk']) == 0
    assert ref['nat'].tolist() == [0, 0, 0] and ref['row0'].tolist() == [0, 0, 0, 0]


def _assert_same(a, b):
    compare_index(a, b)
    compare_index(b, a)
    assert np.array_equal(a['listed'], b['listed']) and np.array_equal(a['tlisted'], b['tlisted'])


@pytest.mark.parametrize('name', ['collate_class', 'collate_reg'])
def test_dense_and_compact_agree_on_the_collate_fixtures(name):
    z, mols = _load(name)
    h = compact_host(mols)
    adj = z['out/adj']
    B, N = adj.shape[:2]
    dense = reference_index(adj, [z['out/r%d' % k] for k in range(5)])
    comp = reference_index_from_bonds(B, N, h['channels'], h['bond_mol'], h['bond_i'], h['bond_j'], h['bond_code'])
    _assert_same(dense, comp)
    assert dense['nat'].tolist() == z['out/size'].tolist()
    assert dense['meta'][L.META_BAD_ADJ] == 0 and dense['meta'][L.META_BAD_REL] == 0


@pytest.mark.parametrize('kw', [dict(B=13, n_max=33, n_med=9, rel_channels=(6, 4, 2, 2, 2), seed=70, isolated_frac=0.15),
                                dict(B=7, n_max=40, n_med=20, rel_channels=(28, 4), seed=3)])
def test_dense_and_compact_agree_on_synthetic_batches(kw):
    mb = make_batch(**kw)
    d = mb.dense()
    dense = reference_index(d[0].numpy(), [t.numpy() for t in d[2:-1]], N_cap=48)
    e = mb.edges
    comp = reference_index_from_bonds(mb.B, mb.N, mb.rel_channels, e[:, 0], e[:, 1], e[:, 2], mb.codes, N_cap=48)
    _assert_same(dense, comp)
    assert dense['meta'][L.META_NLOG] == mb.N and dense['code_cols'] == (mb.N + 15) // 16 * 16
    adj2, rels2 = densify(mb.B, mb.N, mb.rel_channels, e[:, 0], e[:, 1], e[:, 2], mb.codes)
    assert np.array_equal(adj2, d[0].numpy()) and all(np.array_equal(a, b.numpy()) for a, b in zip(rels2, d[2:-1]))


def test_compact_reference_counts_rejected_bonds():
    bm, bi, bj = np.array([0, 0, 0, 1, 0]), np.array([0, 1, 0, 2, 7]), np.array([1, 0, 1, 2, 0])
    bc = np.array([[0], [1], [0], [3], [0]])
    ref = reference_index_from_bonds(2, 5, [3], bm, bi, bj, bc)
    assert ref['meta'][L.META_BAD_ADJ] == 2                     # one listed twice, one out of range
    assert ref['meta'][L.META_BAD_REL] == 1


def test_compare_index_names_the_difference():
    adj, rels = _random_dense(2)
    ref = reference_index(adj, rels)
    for field, where in (('nbr', 'nbr differs at entry'), ('row_ptr', 'row_ptr differs at molecule'), ('nat', 'nat differs'),
                         ('blk', 'blk differs at record'), ('code', 'code differs at view')):
        bad = dict(ref)
        bad[field] = ref[field].copy()
        if field == 'code':
            k, b, i, j = (int(v[0]) for v in np.nonzero(ref['code']))
            bad[field][k, b, i, j] += 1
        elif field == 'nbr':
            bad[field][np.nonzero(ref['listed'])[0][0]] += 1
        else:
            bad[field].reshape(-1)[0] += 1
        with pytest.raises(AssertionError, match=where):
            compare_index(bad, ref)
