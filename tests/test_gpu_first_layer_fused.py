"""The first layer's weight gradient formed in the epilogue of the transposed aggregation (csrc/lagg_kernel.h DWF, csrc/lagg_dw.hip;
csrc/layer.hip plan_layer dw_fused: no stored dP, no split-K launch) against the route it replaces (eagcn_set_first_layer_fused(0):
dP stored, dWcat = X^T.dP as a launch of its own) and against the float64 oracle.

Two-layer Concate models, K = 2 views.  Batches (all through the dense entry point):
  one     one molecule of five atoms (and a bond-less single atom, which has no packed row: the head's BatchNorm wants two molecules):
          T = 5 packed rows, one block, one workgroup row
  r65     five molecules, T = 65 rows: one atom with six bonds (a row with 5..8 bonds), a bond-less atom in the middle of a molecule and
          a trailing one, a self bond; 30 atom features (packed 32 input columns: both 16-row MFMA tiles full)
  r300    24 molecules, T = 300 rows: two blocks (256 + 44 rows by the row limit, 16 + 8 by the molecule limit), one atom with ten bonds
          (more than 8: the general row loop), one with six, self bonds, bond-less atoms
  many    40 molecules of three atoms: T = 120 rows in three blocks of 16 / 16 / 8 molecules; 30 atom features
  pairs   200 molecules of two atoms, 30 atom features (32 packed input columns): T = 400 rows in 13 blocks of 16 molecules.  The launch
          would take 17 workgroup rows; the dWcat area holds 8 slabs and the dP area 400 / 32 = 12, so the slabs live in the dP area,
          the grid is capped at 12 rows and the first of them walks two blocks (adds to its slab) -- asserted through
          eagcn_first_layer_fused_last; every other case keeps its slabs in the dWcat area
  gen     a batch of the project's generator (make_batch: 12 random trees of up to 30 atoms with ring closures, 8 % bond-less atoms)
First-layer view widths 16 (a half chunk), 80 (32 + 32 + 16) and 140.  Eager engine and the captured fused step; r300 once more in a
child process with several chunks per workgroup forced (EAGCN_LAGG_CPW=2: the library reads it once).

Bounds.  The forward is the same code on both routes; outputs are held to 1e-5 relative as the issue sets.  Every gradient is held to
the rule tests/test_gpu_lagg.py::test_lds_staged_aggregation_matches_the_dense_kernels uses for two routes of one operator (1e-5 of
the tensor's largest entry + 2e-6 of the largest gradient; twice that for the edge parameters), and every gradient of the fused route
to helpers.assert_grad_parity at its default tolerances.  eagcn_first_layer_fused_taken shows the route: one layer call per step on
the fused route, none with the switch off, when d(input) is asked for, in the input-only form and with code-book relations -- and
there the results are bit-identical to those with the switch off."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from eagcn_amd.synthetic import MolBatch, bce_weights
from helpers import assert_grad_parity

pytestmark = pytest.mark.gpu

N_DEN1, N_DEN2, NCLASS = 20, 10, 3
CHANS = [6, 4]
TILE_SIZES = [20, 13, 9, 16, 11, 14, 8, 19, 12, 15, 10, 17, 6, 7, 13, 18, 9, 14, 11, 16, 12, 6, 15, 9]


def _chain(a, b):
    return [(i, i + 1) for i in range(a, b)]


def _mol_batch(sizes, bonds, N, seed, n_afeat):
    """bonds: per molecule a list of undirected (i, j), i != j"""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    eb, ei, ej, cd = [], [], [], []
    for b, prs in enumerate(bonds):
        for (i, j) in prs:
            assert i != j and max(i, j) < sizes[b]
            c = [int(rng.integers(0, ch)) for ch in CHANS]
            for (p, q) in ((i, j), (j, i)):
                eb.append(b); ei.append(p); ej.append(q); cd.append(c)
    edges = np.stack([np.array(eb), np.array(ei), np.array(ej)], axis=1).astype(np.int64) if eb else np.zeros((0, 3), dtype=np.int64)
    codes = np.array(cd, dtype=np.int64).reshape(len(eb), len(CHANS))
    afm = np.zeros((B, N, n_afeat), dtype=np.float32)
    for b, n in enumerate(sizes):
        afm[b, :n, :] = rng.random((n, n_afeat), dtype=np.float32)
    labels = rng.integers(-1, 2, size=(B, NCLASS)).astype(np.float32)
    return MolBatch(B=B, N=N, n_afeat=n_afeat, rel_channels=list(CHANS), sizes=np.array(sizes, dtype=np.int64), edges=edges, codes=codes,
                    afm=afm, labels=labels)


def _one():
    return _mol_batch([5, 1], [_chain(0, 4), []], 5, 21, 24), []


def _r65():
    sizes = [20, 13, 9, 16, 7]
    assert sum(sizes) == 65
    bonds = [[(0, j) for j in range(1, 7)] + _chain(6, 18),                    # atom 0: six bonds; atom 19: trailing, bond-less
             _chain(0, 5) + _chain(7, 12),                                     # atom 6: bond-less in the middle
             _chain(0, 8) + [(0, 8)], _chain(0, 15) + [(3, 11)], _chain(0, 6)]
    return _mol_batch(sizes, bonds, 20, 22, 30), [(2, 4)]                      # self bond on atom 4 of molecule 2


def _r300():
    T = sum(TILE_SIZES)
    assert len(TILE_SIZES) == 24 and T == 300
    bonds = [_chain(0, n - 1) + ([(0, n - 1)] if n > 8 else []) for n in TILE_SIZES]
    bonds[0] = [(0, j) for j in range(1, 11)] + _chain(10, 19)                 # ten bonds on atom 0 of a 20-atom molecule
    bonds[7] = [(2, j) for j in (0, 1, 3, 4, 5, 6)] + _chain(6, 17)            # six bonds on atom 2; atom 18: bond-less
    bonds[15] = _chain(0, 8) + _chain(10, 17)                                  # atom 9: bond-less in the middle
    return _mol_batch(TILE_SIZES, bonds, 20, 23, 24), [(0, 0), (3, 5), (20, 1)]


def _pairs():
    return _mol_batch([2] * 200, [[(0, 1)]] * 200, 2, 25, 30), []


def _gen():
    from eagcn_amd.synthetic import make_batch
    return make_batch(B=12, n_max=30, n_med=10, rel_channels=tuple(CHANS), seed=5, isolated_frac=0.08, n_tasks=NCLASS), []


def _many():
    return _mol_batch([3] * 40, [_chain(0, 2)] * 40, 3, 24, 30), []


CASES = {'one': (_one, [16, 80], [12, 20]), 'r65': (_r65, [80, 16], [12, 20]), 'r300': (_r300, [140, 16], [12, 20]),
         'many': (_many, [16, 16], [12, 20]), 'pairs': (_pairs, [16, 80], [12, 20]), 'gen': (_gen, [80, 16], [12, 20])}


def _dense(mb, selfs, device='cpu'):
    """the dense tensors of the batch with self bonds (type 0 in every view) on the listed (molecule, atom) pairs"""
    t = [x.clone() for x in mb.dense()]
    for (b, i) in selfs:
        t[0][b, i, i] = 1.0
        for r in t[2:2 + len(CHANS)]:
            r[b, 0, i, i] = 1.0
    return [x.to(device) for x in t]


_ORACLE = {}


def _oracle(name):
    """fp32 and fp64 oracle of one step (same parameters): once per case, shared and left unchanged"""
    if name in _ORACLE:
        return _ORACLE[name]
    import oracle.eagcn_ref as R
    from eagcn_amd.losses import classification_loss
    build, w1, w2 = CASES[name]
    mb, selfs = build()
    torch.manual_seed(3)
    ref = R.RefEAGCN(CHANS[0], mb.n_afeat, w1, w2, N_DEN1, N_DEN2, NCLASS, 0.0, structure='Concate', molfp_mode='sum', n_layers=2,
                     rel_channels=CHANS)
    R.weights_init_(ref)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    cpu = _dense(mb, selfs)
    labels = torch.from_numpy(mb.labels)
    bw = bce_weights(NCLASS)
    res = []
    for m in (ref, copy.deepcopy(ref).double()):
        dt = next(m.parameters()).dtype
        m.zero_grad(set_to_none=True)
        m.train()
        out, _, _ = m(*[t.to(dt) if t.is_floating_point() else t for t in cpu])
        classification_loss(out, labels, bw).backward()
        res.append({k: q.grad.detach().clone() for k, q in m.named_parameters() if q.grad is not None})
    _ORACLE[name] = dict(mb=mb, selfs=selfs, w1=w1, w2=w2, sd=sd, g32=res[0], g64=res[1])
    return _ORACLE[name]


def _model(orc, graph, **kw):
    from eagcn_amd import EAGCN
    mb = orc['mb']
    hip = EAGCN(CHANS[0], mb.n_afeat, n_den1=N_DEN1, n_den2=N_DEN2, nclass=NCLASS, dropout=0.0, structure='Concate', molfp_mode='sum',
                n_layers=2, widths1=orc['w1'], widths2=orc['w2'], rel_channels=CHANS, graph=graph, validate='deferred', **kw)
    hip = hip.to(torch.device('cuda', 0)).train()
    hip.load_state_dict(orc['sd'], strict=True)
    return hip


def _hip_step(lib, switch, orc, graph):
    """one training step with the switch at `switch`: (loss, out, gradients, eagcn_first_layer_fused_last of the step)"""
    import ctypes
    from eagcn_amd.losses import fused_classification_loss
    dev = torch.device('cuda', 0)
    old = lib.eagcn_set_first_layer_fused(switch)
    try:
        assert lib.eagcn_set_first_layer_fused(switch) == switch          # returns the previous value
        lib.eagcn_first_layer_fused_taken(1)
        hip = _model(orc, graph, grad_mode='direct')
        dense = tuple(_dense(orc['mb'], orc['selfs'], dev))
        labels = torch.from_numpy(orc['mb'].labels).to(dev)
        bw = torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)
        if graph:
            loss, (out, _, _) = hip.fused_step(dense, labels, 'class', bw)
        else:
            out, _, _ = hip(*dense)
            loss = fused_classification_loss(out, labels, bw)
            loss.backward()
        torch.cuda.synchronize()
        grads = {k: q.grad.detach().clone() for k, q in hip.named_parameters() if q.grad is not None}
        taken = lib.eagcn_first_layer_fused_taken(1)
        want = 1 if switch else 0
        # (a captured step may also issue the calls once more while it warms up: a whole multiple)
        assert (taken == want) if not graph else (taken >= want and (taken == 0) == (want == 0)), (taken, want, switch)
        last = (ctypes.c_int32 * 3)()
        lib.eagcn_first_layer_fused_last(last)
        return loss.detach().clone(), out.detach().clone(), grads, tuple(last)
    finally:
        lib.eagcn_set_first_layer_fused(old)


def _two_route_tol(k, v, scale):
    edge = k.endswith('self_r') or k.endswith('att.weight')
    return (2e-5 if edge else 1e-5) * v.abs().max().item() + (4e-6 if edge else 2e-6) * scale


def _check(name, graph):
    from eagcn_amd import _lib
    lib = _lib.load()
    assert lib.eagcn_set_first_layer_fused(1) == 1            # the default
    orc = _oracle(name)
    l1, o1, gr1, (ny, in_dp, ny_free) = _hip_step(lib, 1, orc, graph)
    l0, o0, gr0, _ = _hip_step(lib, 0, orc, graph)
    print('%s/%s: %d slabs, in the dP area: %d, y extent without the cap: %d' % (name, 'graph' if graph else 'eager', ny, in_dp, ny_free))
    if name == 'pairs':      # slabs in the dP area, the grid capped below both its own estimate and the 13 blocks: a workgroup row walks two
        assert in_dp == 1 and 8 < ny < ny_free and ny < 13, (ny, in_dp, ny_free)
    else:
        assert in_dp == 0 and ny == ny_free, (name, ny, in_dp, ny_free)
    assert torch.isfinite(l1).all() and torch.isfinite(o1).all()
    assert ((o1 - o0).abs().max() / o0.abs().max()).item() <= 1e-5
    assert abs(float(l1) - float(l0)) <= 1e-5 * abs(float(l0))
    g32, g64 = orc['g32'], orc['g64']
    assert set(gr1) == set(g32) == set(gr0)
    tag = '%s/%s' % (name, 'graph' if graph else 'eager')
    scale0 = max(v.abs().max().item() for v in gr0.values())
    for k in sorted(gr1):
        assert torch.isfinite(gr1[k]).all(), (k, tag)
        d = (gr1[k].double() - gr0[k].double()).abs().max().item()
        tol = _two_route_tol(k, gr0[k], scale0)
        if 'layer1' in k and k.endswith('graph_conv.weight'):
            print('%s %s: max |grad(fused) - grad(launch)| = %.3e, bound %.3e' % (tag, k, d, tol))
        assert d <= tol, (k, tag, d, tol)
    scale = max(v.abs().max().item() for v in g32.values())
    for k in sorted(gr1):
        assert_grad_parity(gr1[k], g32[k], lambda k=k: g64[k], scale, '%s %s' % (k, tag))


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_route_against_the_separate_launch_and_the_oracle(name, graph):
    _check(name, graph)


def test_several_chunks_per_workgroup():
    """EAGCN_LAGG_CPW=2 (read once by the library: a child process): the instantiation that walks several 32-column chunks of a block
    -- the 140-column view's five chunks in groups of two, the last group a single half-used one -- eager and captured"""
    env = dict(os.environ, EAGCN_LAGG_CPW='2')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', os.path.abspath(__file__), '-k',
                        'test_fused_route_against_the_separate_launch_and_the_oracle and r300'], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and '2 passed' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_the_environment_switch_presets_the_separate_launch():
    """EAGCN_FIRST_LAYER_FUSED=0 (read once by the library: a child process): the setter reports 0 as the previous value and a step
    does not advance the counter"""
    code = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import test_gpu_first_layer_fused as t
from eagcn_amd import _lib
from eagcn_amd.losses import fused_classification_loss
lib = _lib.load()
lib.eagcn_first_layer_fused_taken(1)
orc = t._oracle('one')
dev = torch.device('cuda', 0)
hip = t._model(orc, False, grad_mode='direct')
out, _, _ = hip(*t._dense(orc['mb'], [], dev))
fused_classification_loss(out, torch.from_numpy(orc['mb'].labels).to(dev), torch.tensor(t.bce_weights(t.NCLASS), dtype=torch.float32, device=dev)).backward()
torch.cuda.synchronize()
assert lib.eagcn_first_layer_fused_taken(1) == 0
assert lib.eagcn_set_first_layer_fused(1) == 0
print('child ok')
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, EAGCN_FIRST_LAYER_FUSED='0'), capture_output=True, text=True)
    assert r.returncode == 0 and 'child ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _few_blocks_batch():
    """the shape of `many` (B = 40, N = 3) with two molecules that have bonds: T = 5 rows"""
    sizes = [1] * 40
    sizes[5], sizes[33] = 3, 2
    bonds = [[] for _ in range(40)]
    bonds[5], bonds[33] = _chain(0, 2), [(0, 1)]
    return _mol_batch(sizes, bonds, 3, 31, 30)


def test_graph_replay_across_block_counts():
    """ONE captured step, replayed with a batch of three blocks, with one of five rows and with one WITHOUT a bond (no packed row and no
    block on the device: every workgroup of the captured launch writes zeros, the weight gradient is exactly zero): every slab of the
    weight gradient is written whatever the block count.  The runner's buffers come out of memory that held
    NaN bit patterns (a poisoned allocation freed just before: asserted by address), so a slab left undefined shows."""
    from eagcn_amd import _lib
    from eagcn_amd.losses import fused_classification_loss
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    orc = _oracle('many')
    nobond = _mol_batch([1] * 40, [[] for _ in range(40)], 3, 32, 30)
    batches = [orc['mb'], _few_blocks_batch(), nobond, orc['mb']]
    bw = torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)
    eager = _model(orc, False, grad_mode='direct')
    want = []
    for mb in batches[:3]:
        for p in eager.parameters():
            p.grad = None
        out, _, _ = eager(*_dense(mb, [], dev))
        fused_classification_loss(out, torch.from_numpy(mb.labels).to(dev), bw).backward()
        want.append({k: q.grad.detach().clone() for k, q in eager.named_parameters() if q.grad is not None})
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=dev)
    lo, hi = poison.data_ptr(), poison.data_ptr() + poison.numel()
    torch.cuda.synchronize()
    del poison
    lib.eagcn_first_layer_fused_taken(1)
    g = _model(orc, True, grad_mode='direct')
    for i, mb in enumerate(batches):
        for p in g.parameters():
            p.grad = None
        g.fused_step(tuple(_dense(mb, [], dev)), torch.from_numpy(mb.labels).to(dev), 'class', bw)
        torch.cuda.synchronize()
        if i == 0:
            runners = [r for r in g._runners.values() if hasattr(r, 'scratch')]
            assert len(runners) == 1 and lo <= runners[0].scratch.data_ptr() < hi, 'the scratch block did not come out of the poisoned memory'
        got = {k: q.grad.detach().clone() for k, q in g.named_parameters() if q.grad is not None}
        ref = want[i % 3]
        if mb is nobond:
            for k in got:
                if 'layer1' in k and k.endswith('graph_conv.weight'):
                    assert torch.equal(got[k], torch.zeros_like(got[k])), k
        scale = max(v.abs().max().item() for v in ref.values())
        for k in sorted(ref):
            assert torch.isfinite(got[k]).all(), (i, k)
            d = (got[k].double() - ref[k].double()).abs().max().item()
            assert d <= _two_route_tol(k, ref[k], scale), (i, k, d)
    assert lib.eagcn_first_layer_fused_taken(1) >= 1
    assert len(g._runners) == 1                       # one shape, one captured step


def _autograd_step(lib, switch, orc, want_dx, params, relations='onehot'):
    from eagcn_amd.losses import fused_classification_loss
    dev = torch.device('cuda', 0)
    old = lib.eagcn_set_first_layer_fused(switch)
    try:
        lib.eagcn_first_layer_fused_taken(1)
        hip = _model(orc, False, relations=relations)
        for p in hip.parameters():
            p.requires_grad_(params)
        dense = _dense(orc['mb'], orc['selfs'], dev)
        dense[1].requires_grad_(want_dx)
        out, _, _ = hip(*dense)
        fused_classification_loss(out, torch.from_numpy(orc['mb'].labels).to(dev), torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)).backward()
        torch.cuda.synchronize()
        grads = {k: q.grad.detach().clone() for k, q in hip.named_parameters() if q.grad is not None}
        if want_dx:
            grads['afm'] = dense[1].grad.detach().clone()
        return grads, lib.eagcn_first_layer_fused_taken(1)
    finally:
        lib.eagcn_set_first_layer_fused(old)


@pytest.mark.parametrize('form', ['dx', 'input_only', 'code_books'])
def test_other_forms_keep_their_path_bit_for_bit(form):
    """d(input) asked for, the input-only backward and code-book relations: the counter does not advance and the switch changes no bit.
    (The plain autograd step of the same model does take the route: the counter's own check.)"""
    from eagcn_amd import _lib
    lib = _lib.load()
    orc = _oracle('r65')
    kw = dict(want_dx=form != 'code_books', params=form != 'input_only', relations='general' if form == 'code_books' else 'onehot')
    g1, t1 = _autograd_step(lib, 1, orc, **kw)
    g0, t0 = _autograd_step(lib, 0, orc, **kw)
    assert t1 == 0 and t0 == 0, (form, t1, t0)
    assert set(g1) == set(g0) and len(g1) >= 1
    for k in g1:
        assert torch.equal(g1[k], g0[k]), (form, k)
    _, t = _autograd_step(lib, 1, orc, want_dx=False, params=True)
    assert t == 1, t


def test_a_batch_without_a_bond_has_an_exactly_zero_weight_gradient():
    from eagcn_amd import _lib
    from eagcn_amd.losses import fused_classification_loss
    lib = _lib.load()
    dev = torch.device('cuda', 0)
    orc = _oracle('many')
    mb = _mol_batch([3, 2, 1], [[], [], []], 3, 41, 30)
    hip = _model(orc, False, grad_mode='direct')
    out, _, _ = hip(*_dense(mb, [], dev))
    fused_classification_loss(out, torch.from_numpy(mb.labels).to(dev), torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)).backward()
    torch.cuda.synchronize()
    n = 0
    for k, q in hip.named_parameters():
        if 'layer1' in k and k.endswith('graph_conv.weight'):
            n += 1
            assert q.grad is not None and torch.equal(q.grad, torch.zeros_like(q.grad)), k
    assert n == len(CHANS)
