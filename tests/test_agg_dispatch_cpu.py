"""The case table of tests/test_gpu_agg_dispatch.py (tests/agg_dispatch_cases.py), checked without a GPU: that the restated
dispatch gives the launches the table was written for, that the table reaches every form of the matrix-core aggregation kernels
(so that a later edit of the table cannot silently lose one), that every batch is valid input, and that the oracle's dense
tensors stay small."""
import numpy as np
import pytest

import agg_dispatch_cases as T
import index_reference as IR


def _layers():
    return [(c, d) for c in T.CASES for d in c.layers()]


def test_restated_dispatch_on_written_out_launches():
    """dispatch() against launches worked out by hand from the description of the policy."""
    d = T.dispatch([128] * 3, 12, 200, 20, 47, 5)
    assert (d['tmax'], d['nchunk'], d['CT'], d['masked'], d['form'], d['agg_wg'], d['agg_passes']) == (8, 1, 9, True, 'ksplit', 20, 1)
    assert not d['partial'] and not d['skipped'] and d['nct'] == [8]
    d = T.dispatch([160] * 3, 12, 200, 20, 47, 5, maxb=0)
    assert (d['tmax'], d['nchunk'], d['CT'], d['masked'], d['form'], d['agg_wg']) == (10, 2, 5, False, 'wave', 5)
    d = T.dispatch([256] * 3, 12, 200, 20, 47, 5)
    assert (d['nchunk'], d['CT'], d['masked'], d['nct']) == (2, 9, True, [7, 9])
    d = T.dispatch([304] * 3, 12, 200, 20, 47, 5)
    assert (d['nchunk'], d['CT'], d['nct']) == (3, 7, [5, 7])
    d = T.dispatch([100] * 3, 12, 200, 20, 47, 5)
    assert (d['tmax'], d['CT']) == (7, 7)
    d = T.dispatch([160, 48, 16], 12, 200, 20, 47, 5)             # 10 / 3 / 1 tiles, chunks of 5: views 1 and 2 have no second chunk
    assert (d['nchunk'], d['CT'], d['skipped'], d['nct']) == (2, 5, True, [1, 3, 5])
    d = T.dispatch([112, 40, 16], 12, 200, 20, 47, 5)
    assert (d['nchunk'], d['CT'], d['skipped'], d['partial'], d['nct']) == (1, 7, False, True, [1, 3, 7])
    # 600 x 33 atoms, K-split forced: 1800 tiles over 1024 workgroups; 19800 rows = 1238 blocks over 1024 workgroups; no hand-out
    d = T.dispatch([16, 16], 600, 19800, 1800, 33, 9, maxb=100000)
    assert (d['form'], d['agg_wg'], d['agg_passes'], d['edge_wg'], d['edge_passes'], d['tile_handout'], d['edge_handout']) == \
        ('ksplit', 1024, 2, 1024, 2, False, False)
    # 1100 x 33: 3300 tiles over 512 x 4; 36300 rows = 2269 blocks; 3300 < 4400 and 36300 < 70400: both hand-outs off
    d = T.dispatch([16, 16], 1100, 36300, 3300, 33, 9)
    assert (d['form'], d['agg_wg'], d['agg_passes'], d['edge_passes'], d['tile_handout'], d['edge_handout']) == ('wave', 512, 2, 3, False, False)
    # 300 x 70: 1500 tiles = 375 workgroups (375 = 8 * 46 + 7); 21000 rows = 1313 blocks > 1024, 21000 >= 19200
    d = T.dispatch([16, 16], 300, 21000, 1500, 70, 9)
    assert (d['agg_wg'], d['agg_passes'], d['tile_handout'], d['tile_rem'], d['edge_handout'], d['edge_wg'], d['edge_passes'], d['edge_rem']) == \
        (375, 1, True, [7], True, 1024, 2, 0)
    # 130 x 70: 9100 rows = 569 blocks (569 = 8 * 71 + 1)
    d = T.dispatch([80, 80], 130, 9100, 650, 70, 9, maxb=0)
    assert (d['CT'], d['edge_handout'], d['edge_wg'], d['edge_rem'], d['tile_rem']) == (5, True, 569, 1, [3])
    d = T.dispatch([128] * 3, 5, 616, 41, 300, 62)
    assert d['flush'] and d['segments'] == 2 and d['form'] == 'ksplit'


@pytest.mark.parametrize('n', [1, 7, 8, 9, 375, 569, 1024])
def test_hand_out_is_a_bijection(n):
    """The remap of the description, over n live workgroups: every position once, and the workgroups of one XCD contiguous."""
    pos = [T.remap(n, bx) for bx in range(n)]
    assert sorted(pos) == list(range(n))
    for x in range(8):
        mine = [T.remap(n, bx) for bx in range(x, n, 8)]
        assert mine == list(range(mine[0], mine[0] + len(mine))) if mine else True


def test_table_covers_the_dispatch_space():
    L = _layers()
    for form in ('ksplit', 'wave'):
        assert {d['CT'] for _, d in L if d['form'] == form} >= {1, 2, 3, 4, 5, 6, 7, 9}, form
        assert any(d['masked'] and d['nchunk'] == 1 for _, d in L if d['form'] == form), form
        assert {d['nchunk'] for _, d in L if d['form'] == form} >= {1, 2, 3}, form
        assert any(d['skipped'] for _, d in L if d['form'] == form), form
        assert any(d['partial'] and d['nchunk'] == 1 for _, d in L if d['form'] == form), form
        # the slab form of the edge gradients above CT = 1, in both distributions
        assert {d['CT'] for _, d in L if d['form'] == form and d['edge_out'] == 'slab'} >= {7, 9}, form
        for s in ('Concate', 'Weighted_sum'):
            assert {d['CT'] for c, d in L if d['form'] == form and c.structure == s} >= {1, 2, 3, 4, 5, 6, 7, 9}, (form, s)
    assert {d['edge_out'] for _, d in L} == {'atomic', 'slab'}
    assert any(d['form'] == 'ksplit' and d['agg_passes'] > 1 for _, d in L)               # the cap of 1024 tiles
    assert any(d['form'] == 'wave' and d['agg_passes'] > 1 for _, d in L)                 # the cap of 512 workgroups
    assert any(d['edge_passes'] > 1 and not d['edge_handout'] for _, d in L)              # the cap of 1024 row blocks
    assert any(d['edge_passes'] > 1 and d['edge_handout'] for _, d in L)                  # ... with the hand-out on
    assert any(d['tile_handout'] and any(d['tile_rem']) for _, d in L)
    assert any(d['edge_handout'] and d['edge_rem'] for _, d in L)
    assert any(d['form'] == 'wave' and not d['tile_handout'] and d['agg_passes'] > 1 for _, d in L)
    assert any(d['flush'] for _, d in L) and any(d['segments'] == 2 for _, d in L)
    # the forms the default policy still takes are taken with no switch
    assert any(c.child is None and d['segments'] == 2 for c, d in L)
    assert {d['form'] for c, d in L if c.child is None and c.general} == {'ksplit', 'wave'}


def test_children_share_one_switch_and_stay_small():
    kids = T.children()
    for child, names in kids.items():
        env = T.child_env(child)
        assert env['EAGCN_AGG'] == 'dense' and len(names) <= 6, (child, names)
        want = 'wave' if 'wave' in child else 'ksplit'
        assert {d['form'] for n in names for d in T.BY_NAME[n].layers()} == {want}, child
    assert len([c for c in kids if c.startswith('ct-')]) == 6 and len([c for c in kids if c.startswith('caps-')]) == 4


def _bonds(mb):
    e = mb.edges
    return mb.B, mb.N, list(mb.rel_channels), e[:, 0], e[:, 1], e[:, 2], mb.codes


@pytest.mark.parametrize('key', sorted({c.batch_key for c in T.CASES}, key=str), ids=str)
def test_batches_are_valid_input(key):
    mb = T.batch(*key)
    cases = [c for c in T.CASES if c.batch_key == key]
    idx = IR.reference_index_from_bonds(*_bonds(mb))
    assert idx['meta'][IR.L.META_BAD_ADJ] == 0 and idx['meta'][IR.L.META_BAD_REL] == 0
    s = T.shape(mb)
    assert (idx['nat'] == s['nat']).all() and idx['meta'][IR.L.META_T] == s['T'] and idx['meta'][IR.L.META_NTILES] == s['tiles']
    e = mb.edges
    pairs = set(map(tuple, e.tolist()))
    assert len(pairs) == len(e) and all((b, j, i) in pairs for b, i, j in pairs), 'symmetric, every directed bond once'
    lo, hi = np.minimum(e[:, 1], e[:, 2]), np.maximum(e[:, 1], e[:, 2])
    order = np.lexsort((hi, lo, e[:, 0]))
    k3 = np.stack([e[:, 0], lo, hi], axis=1)[order]
    same = (k3[1:] == k3[:-1]).all(axis=1)
    assert (mb.codes[order][1:][same] == mb.codes[order][:-1][same]).all(), 'a bond has one type in both directions'
    for c in cases:
        assert int(mb.sizes.max()) <= c.n_atoms and mb.N <= max(c.n_atoms, mb.N if c.general else 0), c.name
        assert all(0 <= ch <= 255 for ch in c.channels) and (mb.codes < np.asarray(mb.rel_channels)[None, :]).all()
        if c.typed:
            assert (mb.codes[:, 0] == e[:, 0] % 12).all() and len(set(mb.sizes.tolist())) == 1 and (s['nat'] == c.n_atoms).all()


def test_ragged_batch_has_the_edges_it_is_there_for():
    mb = T.batch('ragged', T.CH3)
    s = T.shape(mb)
    assert set(mb.sizes.tolist()) >= {1, 15, 16, 17, 31, 33, 47} and mb.B == 12
    assert {int(t) for t in (s['nat'] + 15) // 16} >= {1, 2, 3} and (s['nat'] % 4 != 0).any()
    deg = T._degrees(mb)
    inside = [(b, i) for b in range(mb.B) for i in range(int(s['nat'][b])) if deg[b, i] == 0]
    assert inside, 'isolated atoms inside the stored rows'
    assert (mb.edges[:, 1] == mb.edges[:, 2]).sum() == 1, 'one self bond'
    assert int(mb.sizes.max()) < 48                               # (the edge parameters' filler sums stay far below the rule)


def test_big_batch_has_the_hub_and_the_second_segment():
    mb = T.batch('big', T.CH3)
    s = T.shape(mb)
    assert sorted(mb.sizes.tolist(), reverse=True) == [300, 257, 40, 17, 2] and mb.N == 300 and s['nat'].max() > 256
    hub = mb.edges[(mb.edges[:, 0] == 0) & (mb.edges[:, 1] == 5)][:, 2]
    assert len(hub) > 60 and (hub >= 256).sum() >= 20 and (hub < 256).sum() >= 20 and s['hits'] > T.HIT_FLUSH
    assert (mb.edges[:, 1] == mb.edges[:, 2]).sum() == 1


def test_code_book_batches():
    for B in (260, 24):
        dense, mols = T.general_dense(B)
        adj, rels = dense[0], dense[2:-1]
        assert adj.shape == (B, 21, 21) and len(mols) == B and [r.shape[1] for r in rels] == list(T.GENERAL_CHANNELS)
        assert (adj == adj.transpose(0, 2, 1)).all() and all((r == r.transpose(0, 1, 3, 2)).all() for r in rels)
        assert all(((r != 0).any(axis=1) <= (adj != 0)).all() for r in rels)
        assert any(((r != 0) & (r != 1)).any() for r in rels), 'not one-hot: the code book is needed'


def test_no_pre_activation_at_a_relu_boundary():
    """What agg_dispatch_check.run_case asserts before it compares, for every case, here: the float64 oracle keeps every
    pre-activation RELU_MARGIN away from 0 (a later edit of the table or of a seed shows here, not as a miss on the GPU)."""
    import copy
    import agg_dispatch_check as K
    for c in T.CASES:
        dense, _ = K.inputs(c)
        twin = copy.deepcopy(K.oracle(c, dense)).double().train()
        assert K.relu_margin(c, twin, dense, K.to64) >= K.RELU_MARGIN, c.name


def test_oracle_tensors_stay_small():
    """The dense float64 tensors of the largest case (adjacency, atom features, relation tensors and the per-view attention
    matrices of one layer, kept for the backward) stay under 1 GB."""
    worst = (0, '')
    for c in T.CASES:
        mb = c.batch()
        per_view = 6 * mb.B * mb.N * mb.N                        # s, sigmoid, a1, u, u / rs, a_hat
        n = mb.B * mb.N * mb.N * (1 + sum(c.channels)) + mb.B * mb.N * 24 + 2 * len(c.channels) * per_view
        worst = max(worst, (8 * n, c.name))
    assert worst[0] < 1e9, worst
