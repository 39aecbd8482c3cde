"""The matrix-core aggregation (csrc/agg.hip: forward, transposed pass, transposed pass co-launched with the edge gradients) against
the float64 oracle ACROSS ITS DISPATCH SPACE: every count of column tiles per workgroup (1..7, 9 and the masked 8 -> 9) in both work
distributions (K split over a workgroup's waves / one wave per tile), several column chunks, views of unequal width, the three
grid caps with their second pass, both XCD-contiguous hand-outs with a remainder, the slab form of the edge gradients, the early
flush of a row's hit queue and the second 256-column segment of a code row.  Since the bond-list kernels (csrc/lagg.hip) took
over molecules of up to 256 atoms, these kernels run by default only for larger batches' padding, for code-book relations'
backward and under EAGCN_AGG=dense -- and nothing else in the suite reaches most of their instantiations.

The cases and what each of them takes (restated, not asked of the library) are in tests/agg_dispatch_cases.py, the comparison in
tests/agg_dispatch_check.py.  Cases that need a switch share subprocesses (the library reads its switches once)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest

import agg_dispatch_cases as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHECK = os.path.join(HERE, 'agg_dispatch_check.py')


def _child(child, extra=(), **env):
    names = T.children()[child]
    env = dict(os.environ, **(env or T.child_env(child)))
    r = subprocess.run([sys.executable, CHECK, *extra, *names], env=env, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('AGG_DISPATCH')]
    print('\n'.join(lines))                          # (relayed before the verdict: a miss names its case and tensors)
    assert r.returncode == 0 and 'AGG_DISPATCH_OK' in lines, (r.stdout[-3000:], r.stderr[-3000:])
    done = [ln for ln in lines if ln.startswith('AGG_DISPATCH_SAVED ' if '--save-dir' in extra else 'AGG_DISPATCH ')]
    assert len(done) == len(names), lines
    return done


@pytest.mark.timeout(600)
@pytest.mark.parametrize('child', [c for c in T.children() if c.startswith('ct-')])
def test_every_column_tile_count_in_both_distributions(child):
    """(a) B = 12 ragged molecules (1..47 atoms, isolated atoms, a self bond), K = 3: equal widths with 1..10, 16 and 19 column
    tiles, a width that is no multiple of 16, views of unequal width; Concate and Weighted_sum; K-split and wave-per-tile."""
    _child(child)


@pytest.mark.timeout(600)
@pytest.mark.parametrize('child', [c for c in T.children() if c.startswith('caps-')])
def test_grid_caps_and_xcd_hand_outs(child):
    """(b) Batches beyond a grid cap (a second pass of the K-split kernel, of the wave-per-tile kernel and of the edge gradients)
    and batches that switch the XCD-contiguous hand-outs on, with live workgroup counts that are no multiple of 8.  View 0 gives
    every bond of molecule b the type 1 + (b mod 12): an entry of d att.weight comes from a twelfth of the molecules, so a
    dropped or doubled row block is an error of percent size in one entry."""
    case = T.BY_NAME[T.children()[child][0]]
    if case.edge_ref != 'lds':
        _child(child)
        return
    # 70-atom molecules: att.weight / self_r may miss the rule by the dense kernels' fp32 sums of filler products; then they are
    # held to the bond-list path's run of the same batch (see agg_dispatch_check.py)
    with tempfile.TemporaryDirectory() as d:
        _child(child, ('--save-dir', d), EAGCN_AGG='lds')
        _child(child, ('--lds-dir', d))


# ---- (c) the default policy, in this process ---------------------------------------------------------------------------------------
def _routes(case):
    """eagcn_layer_route of the case's two layers (training forward + full backward), asked with made-up addresses as
    tests/route_check.py does: nothing is dereferenced."""
    import route_check as R
    L = R.L
    lib = L.load()
    s = T.shape(case.batch())
    c = L.new_batch(s['B'], s['N'], list(case.channels))
    c.T, c.n_max, c.n_tiles = s['T'], int(s['nat'].max()), s['tiles']
    L.point_batch(c, R.fake(), R.fake())
    c.code = R.fake()
    for f in ('mol_info', 'row_ptr', 'col_ptr', 'nbr', 'tnbr', 'ecode', 'tcode', 'blk'):     # bond lists present: dense by POLICY
        setattr(c, f, R.fake())
    c.build_lists, c.E = 1, int(len(case.batch().edges))
    if case.general:
        for k, ch in enumerate(T.GENERAL_CHANNELS):
            c.rel_vec[k], c.rel_c[k] = R.fake(), ch
    out = []
    segs = [(24, 24)]
    for l, w in enumerate((case.w1, case.w2)):
        vw = T.view_widths(case.structure, w)
        p = L.LayerParams()
        p.K, p.structure, p.training = len(vw), L.STRUCTURES[case.structure], 1
        p.inp.nseg = len(segs)
        for i, (wd, pad) in enumerate(segs):
            p.inp.width[i], p.inp.pad[i] = wd, pad
        p.dropout, p.bn_eps, p.bn_momentum, p.seed = 0.0, 1e-5, 0.1, 7
        for k, wd in enumerate(vw):
            p.width[k] = wd
            for f in ('att_w', 'self_r', 'W', 'bias', 'gamma', 'beta', 'run_mean', 'run_var'):
                getattr(p, f)[k] = R.fake()
        p.ave_w = R.fake() if case.structure == 'Weighted_sum' else None
        bufs = R.make_bufs(True, False, False)
        r = (C.c_int32 * 16)()
        rc = lib.eagcn_layer_route(C.byref(c), C.byref(p), C.byref(bufs), int(l > 0), 0, 0, int(l > 0), C.byref(r))
        assert rc == 0, lib.eagcn_last_error()
        out.append((R, list(r)))
        segs = [(wd, T.pad16(wd)) for wd in vw] if case.structure == 'Concate' else [(vw[0], T.pad16(vw[0]))]
    return out


def _run_in_process(name):
    assert not [k for k in os.environ if k.startswith('EAGCN_AGG')], 'the default policy is what this test is about'
    import agg_dispatch_check as K
    case = T.BY_NAME[name]
    for R, r in _routes(case):
        if case.general:                         # code book: the whole backward is dense, the edge gradients leave as slabs
            assert r[R.BWD_AGG] == 0 and r[R.EDGE_ATOMIC] == 0 and r[R.EDGE] == R.COLAUNCH, r
        else:                                    # padded beyond 256 atoms: dense in both directions
            assert r[R.FWD_AGG] == 0 and r[R.BWD_AGG] == 0 and r[R.EDGE] == R.COLAUNCH, r
    print(K.run_case(case))


@pytest.mark.parametrize('name', [c.name for c in T.CASES if c.child is None and not c.general])
def test_batch_padded_beyond_256_atoms(name):
    """(c) Molecules of 300, 257, 40, 17 and 2 atoms: the only aggregation such a batch has.  A hub atom with more than 60 bonds,
    half of them to atoms at 256 and above: the early flush of the hit queue and the second segment of the code row.  Widths 128
    (the masked 9) and 208 (two chunks)."""
    _run_in_process(name)


@pytest.mark.parametrize('name', [c.name for c in T.CASES if c.child is None and c.general])
def test_code_book_relations_backward(name):
    """(c) Real-valued relation tensors through collate_compact(..., general=True): the backward is the dense co-launch with the
    edge gradients leaving as one slab per workgroup, at 260 molecules (wave per tile) and 24 (K-split), CT = 9 (masked, with
    views of 6, 3 and 1 tiles) and 7."""
    _run_in_process(name)
