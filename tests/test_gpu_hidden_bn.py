"""A hidden Concate layer's BatchNorm backward from the dX product of the layer above it (csrc/bx3.h BxBnEpi, csrc/bx3_epi.h: the units of
the plane GEMMs form the layer below's dH and the column sums of dH and dH xhat on their way out; csrc/layer.hip plan_layer dh_given,
csrc/head.hip model_backward_impl) against the reduction pass over the rows it replaces (eagcn_set_hidden_bn_sums(0)) and against the
oracle.

Batches:
  corner / tiny   the batches of test_gpu_top_bn.py (B = 6, N_pad = 20, sizes 1/2/5/20/20/3, a six-bond atom, a trailing bond-less atom;
                  B = 3 with T = 5 rows), K = 2, widths 9/7 -> 12/20, two and three layers.  Their layers are narrower than the 128 input
                  columns the plane GEMMs start at (csrc/layer.hip layer_dims), so no layer of them has a plane-pair layer above it: they
                  hold the switch to changing NOTHING where the route does not apply (every gradient bit-identical).
  corner5 / tiny5 the same two batches with K = 5 views of exact width 28 (packed 32: padded columns; Fp = 160 >= 128, so layer 2 and up
                  run the plane pair and the layers below them are fused): T = 49 and T = 5 rows, fewer than one 64-row block -- a single
                  partial slab.  (A fused layer narrower than 128 columns does not exist: the layer above it would not run the plane
                  GEMMs.  The 64-column block of 32 columns at the right edge of the 160 is the narrowest block there is.)
  tile edges      24 chain molecules of 6..20 atoms, T = 300 packed rows (three 128-row tiles, the last one partial; five 64-row blocks,
                  the last one of 44 rows -- asserted on the CPU), K = 5 views of exact width 28 (packed 160 columns: two 128-column
                  tiles, the second one partial, and a 64-column block of 32 columns).  Two layers (layer 1 fused) and three layers (layers
                  2 and 1 fused: both ping-pong buffers in both roles), dropout 0 and 0.3, eager engine and the captured fused step; and
                  once more in a child process with EAGCN_BX3_WIDE=1 (the 256 x 128 kernel does not carry the code: the pass stays).

Every step asserts through eagcn_hidden_bn_sums_taken that the route was taken exactly where it applies (n_layers - 1 layer calls per
step with the five-view widths and the switch at 1, none otherwise -- nor where the layer above runs on the 256 x 128 kernel).  With the switch at 1 and at 0 the forward is the same code: outputs, graph representation, running statistics and loss must be
bit-identical.  Every gradient of the switch-1 run is held to helpers.assert_grad_parity at its default tolerances.  dH is formed from
the same factors in the same order on both routes, so every gradient but the fused layers' d gamma / d beta is bit-identical too; those
two are fp64 sums of the same fp32 terms in another order, rounded once to fp32: at most one fp32 ulp of the tensor's largest magnitude
apart."""
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
SMALL = dict(chans=[6, 4], w1=[9, 7], w2=[12, 20])
WIDE = dict(chans=[6, 4, 3, 5, 2], w1=[28] * 5, w2=[28] * 5)
TILE_SIZES = [20, 13, 9, 16, 11, 14, 8, 19, 12, 15, 10, 17, 6, 7, 13, 18, 9, 14, 11, 16, 12, 6, 15, 9]


def _mol_batch(sizes, bonds, N, seed, chans):
    """bonds: per molecule a list of undirected (i, j)"""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    eb, ei, ej, cd = [], [], [], []
    for b, prs in enumerate(bonds):
        for (i, j) in prs:
            c = [int(rng.integers(0, ch)) for ch in chans]
            for (p, q) in ((i, j), (j, i)):
                eb.append(b); ei.append(p); ej.append(q); cd.append(c)
    edges = np.stack([np.array(eb), np.array(ei), np.array(ej)], axis=1).astype(np.int64)
    codes = np.array(cd, dtype=np.int64).reshape(len(eb), len(chans))
    afm = np.zeros((B, N, 24), dtype=np.float32)
    for b, n in enumerate(sizes):
        afm[b, :n, :] = rng.random((n, 24), dtype=np.float32)
    labels = rng.integers(-1, 2, size=(B, NCLASS)).astype(np.float32)
    return MolBatch(B=B, N=N, n_afeat=24, rel_channels=list(chans), sizes=np.array(sizes, dtype=np.int64), edges=edges, codes=codes,
                    afm=afm, labels=labels)


def _chain(a, b):
    return [(i, i + 1) for i in range(a, b)]


def _tile_batch():
    """chains (the longer ones closed to rings): every atom has a bond, so T = sum of the sizes"""
    T = sum(TILE_SIZES)
    assert len(TILE_SIZES) == 24 and max(TILE_SIZES) <= 20
    assert 257 <= T <= 383 and T % 64 != 0 and ((T + 63) // 64) % 2 == 1 and (T + 127) // 128 == 3, T
    return _mol_batch(TILE_SIZES, [_chain(0, n - 1) + ([(0, n - 1)] if n > 8 else []) for n in TILE_SIZES], 20, 11, WIDE['chans'])


def _corner_wide_batch():
    """the corner batch of test_gpu_top_bn.py with five views: B = 6, N_pad = 20, sizes 1/2/5/20/20/3 (the one-atom molecule has no packed
    row), one atom with six bonds, one trailing bond-less atom; T = 49 packed rows: ONE partial 64-row block, one partial slab"""
    bonds = [[], [(0, 1)], _chain(0, 4), [(0, j) for j in range(1, 7)] + _chain(6, 19) + [(3, 11)], _chain(0, 18) + [(2, 9)], _chain(0, 2)]
    return _mol_batch([1, 2, 5, 20, 20, 3], bonds, 20, 5, WIDE['chans'])


def _tiny_wide_batch():
    """B = 3 and T = 5 packed rows, five views: fewer rows than one 64-row block (and than the seven rows of one slab of the row pass)"""
    return _mol_batch([2, 3, 1], [[(0, 1)], [(0, 1), (1, 2)], []], 3, 6, WIDE['chans'])


def _widths(cfg, n_layers):
    return [cfg['w1'], cfg['w2'], [2 * w for w in cfg['w2']]][:n_layers]


_ORACLE = {}


def _oracle(name, mb, cfg, n_layers, p, hseed):
    """fp32 and fp64 oracle of one step (same parameters, the kernels' dropout masks injected): once per (batch, layers, p)"""
    key = (name, n_layers, p)
    if key in _ORACLE:
        assert _ORACLE[key]['hseed'] == hseed
        return _ORACLE[key]
    import oracle.eagcn_ref as R
    from eagcn_amd.losses import classification_loss
    from test_gpu_parity import _hip_dropout_masks
    chans = cfg['chans']
    torch.manual_seed(3)
    ref = R.RefEAGCN(chans[0], 24, cfg['w1'], cfg['w2'], N_DEN1, N_DEN2, NCLASS, p, structure='Concate', molfp_mode='sum', n_layers=n_layers,
                     rel_channels=chans)
    R.weights_init_(ref)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    ref64 = copy.deepcopy(ref).double()
    cpu = mb.dense()
    labels = torch.from_numpy(mb.labels)
    bw = bce_weights(NCLASS)
    masks = _hip_dropout_masks(mb, _widths(cfg, n_layers), 'Concate', N_DEN1, p, hseed) if p > 0 else []
    res = []
    for m in (ref, ref64):
        dt = next(m.parameters()).dtype
        queue = [t.to(dt) for t in masks]
        orig = R.F.dropout
        if p > 0:
            R.F.dropout = lambda x, p=0.5, training=True, inplace=False: x * queue.pop(0) if training else x
        try:
            m.zero_grad(set_to_none=True)
            m.train()
            out, _, gr = m(*[t.to(dt) if t.is_floating_point() else t for t in cpu])
            classification_loss(out, labels, bw).backward()
            assert not queue
        finally:
            R.F.dropout = orig
        res.append({k: q.grad.detach().clone() for k, q in m.named_parameters() if q.grad is not None})
    _ORACLE[key] = dict(sd=sd, g32=res[0], g64=res[1], hseed=hseed)
    return _ORACLE[key]


def _hip_step(lib, switch, mb, cfg, n_layers, p, graph, sd):
    """one training step with the switch at `switch`: (loss, out, graph_rep, gradients, state_dict after the step, dropout seed)"""
    from eagcn_amd import EAGCN
    from eagcn_amd.losses import fused_classification_loss
    dev = torch.device('cuda', 0)
    old = lib.eagcn_set_hidden_bn_sums(switch)
    try:
        assert lib.eagcn_set_hidden_bn_sums(switch) == switch          # returns the previous value
        lib.eagcn_hidden_bn_sums_taken(1)
        chans = cfg['chans']
        hip = EAGCN(chans[0], 24, n_den1=N_DEN1, n_den2=N_DEN2, nclass=NCLASS, dropout=p, structure='Concate', molfp_mode='sum',
                    n_layers=n_layers, widths1=cfg['w1'], widths2=cfg['w2'], rel_channels=chans, grad_mode='direct', graph=graph,
                    validate='deferred').to(dev).train()
        hip.load_state_dict(sd, strict=True)
        dense = tuple(t.to(dev) for t in mb.dense())
        labels = torch.from_numpy(mb.labels).to(dev)
        bw = torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)
        torch.manual_seed(77)
        hseed = int(torch.randint(0, 2 ** 62, (1,)).item())       # what the step is about to draw for its dropout seeds
        torch.manual_seed(77)
        if graph:
            loss, (out, _, gr) = hip.fused_step(dense, labels, 'class', bw)
        else:
            out, _, gr = hip(*dense)
            loss = fused_classification_loss(out, labels, bw)
            loss.backward()
        torch.cuda.synchronize()
        grads = {k: q.grad.detach().clone() for k, q in hip.named_parameters() if q.grad is not None}
        state = {k: v.detach().clone() for k, v in hip.state_dict().items()}
        # THE ROUTE WAS TAKEN (or not): layer backward calls that found dH and its sums where the layer above left them -- every layer
        # below the top one of a model whose layers are wide enough for the plane GEMMs, once per step (a captured step: at its capture)
        taken = lib.eagcn_hidden_bn_sums_taken(1)
        want = (n_layers - 1) if (switch and cfg is WIDE and os.environ.get('EAGCN_BX3_WIDE') != '1') else 0
        # (a captured step may also issue the calls once more while it warms up: a whole multiple)
        assert (taken == want) if not graph else (taken >= want and (taken == 0) == (want == 0) and taken % max(want, 1) == 0), \
            (taken, want, switch, n_layers)
        return loss.detach().clone(), out.detach().clone(), gr.detach().clone(), grads, state, hseed
    finally:
        lib.eagcn_set_hidden_bn_sums(old)


def _is_fused_bn(k, n_layers):
    """d gamma / d beta of a layer below the top one"""
    return any(k.startswith('layer%d.' % l) for l in range(1, n_layers)) and 'batch_norm' in k and (k.endswith('weight') or k.endswith('bias'))


def _check(name, mb, cfg, n_layers, p, graph):
    from eagcn_amd import _lib
    lib = _lib.load()
    assert lib.eagcn_set_hidden_bn_sums(1) == 1          # the default
    if os.environ.get('EAGCN_BX3_WIDE') == '1':          # (the child process of the wide-kernel test: every plane GEMM runs on the 256 x 128 kernel)
        assert lib.eagcn_set_bx3_wide(1) == 1
    torch.manual_seed(77)
    hseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    orc = _oracle(name, mb, cfg, n_layers, p, hseed)
    l1, o1, g1, gr1, st1, hs1 = _hip_step(lib, 1, mb, cfg, n_layers, p, graph, orc['sd'])
    l0, o0, g0, gr0, st0, hs0 = _hip_step(lib, 0, mb, cfg, n_layers, p, graph, orc['sd'])
    assert hs1 == hs0 == hseed
    assert torch.isfinite(l1).all() and torch.isfinite(o1).all()
    assert torch.equal(l1, l0), (float(l1), float(l0))
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    assert set(st1) == set(st0)
    for k in st1:                                     # parameters (untouched) and every BatchNorm running buffer
        assert torch.equal(st1[k], st0[k]), k
    g32, g64 = orc['g32'], orc['g64']
    assert set(gr1) == set(g32) == set(gr0)
    scale = max(v.abs().max().item() for v in g32.values())
    tag = '%s/L%d/p%s/%s' % (name, n_layers, p, 'graph' if graph else 'eager')
    nfused = 0
    for k in sorted(gr1):
        a, b = gr1[k].float().cpu(), gr0[k].float().cpu()
        d = (a.double() - b.double()).abs().max().item()
        if _is_fused_bn(k, n_layers):
            nfused += 1
            ulp = float(np.spacing(np.float32(max(a.abs().max().item(), b.abs().max().item()))))
            print('%s %s: max |grad(1) - grad(0)| = %.3e, one ulp of the largest magnitude = %.3e' % (tag, k, d, ulp))
            assert d <= ulp, (k, tag, d, ulp)
        else:
            assert torch.equal(gr1[k], gr0[k]), (k, tag, d)
    assert nfused == 2 * len(cfg['chans']) * (n_layers - 1), nfused
    for k in sorted(gr1):
        assert_grad_parity(gr1[k], g32[k], lambda k=k: g64[k], scale, '%s %s' % (k, tag))


def _corner():
    from test_gpu_top_bn import _corner_batch
    return _corner_batch()


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('n_layers', [2, 3])
def test_corner_batch(n_layers, p, graph):
    _check('corner', _corner(), SMALL, n_layers, p, graph)


def test_fewer_rows_than_one_block():
    from test_gpu_top_bn import _tiny_batch
    _check('tiny', _tiny_batch(), SMALL, 2, 0.0, False)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('n_layers', [2, 3])
def test_tile_edges(n_layers, p, graph):
    _check('tile', _tile_batch(), WIDE, n_layers, p, graph)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('n_layers', [2, 3])
def test_corner_batch_five_views(n_layers, p, graph):
    _check('corner5', _corner_wide_batch(), WIDE, n_layers, p, graph)


@pytest.mark.parametrize('n_layers', [2, 3])
def test_fewer_rows_than_one_block_five_views(n_layers):
    # dropout 0, as the tiny case of test_gpu_top_bn.py: with dropout 0.3 a BatchNorm over these five rows is too ill-conditioned for
    # the oracle bound on EITHER route (layer1.block2.graph_conv.weight: 1.25e-4 of its own maximum against the fp32 oracle's 1.6e-5,
    # the same bits with the switch at 0 and at 1); dropout on a single partial block is covered by the T = 49 batch above
    _check('tiny5', _tiny_wide_batch(), WIDE, n_layers, 0.0, False)


NARROW = dict(chans=[6, 4], w1=[64, 64], w2=[64, 64])       # Fp = 128: the narrowest layer whose output leaves as plane images


@pytest.mark.parametrize('wide', [False, True], ids=['by_size', 'wide_kernel'])
def test_engine_runs_the_plan_it_reports(wide, monkeypatch):
    """The hand-offs a backward call takes are the ones its plan reports (eagcn_model_route, asked with the very blocks the call runs
    on): three Concate layers of two 64-column views, six chain molecules of 3..20 atoms, one eager training step.  The layer calls
    that found dH and its sums in their upstream buffer (eagcn_hidden_bn_sums_taken) and those whose weight gradient left the
    aggregation's epilogue (eagcn_first_layer_fused_taken) are as many as the plan has layers with bit 32 and bit 128 -- by default
    both hidden links and the first layer, none of the links once every plane GEMM is forced onto the 256 x 128 kernel, which does
    not carry the tail pass.  The gradients hold the file's bounds against the oracle either way."""
    import ctypes as C
    from eagcn_amd import EAGCN, _lib
    from eagcn_amd.losses import fused_classification_loss
    lib = _lib.load()
    sizes = [3, 20, 7, 12, 5, 16]
    mb = _mol_batch(sizes, [_chain(0, n - 1) for n in sizes], 20, 13, NARROW['chans'])
    p, n_layers = 0.3, 3
    torch.manual_seed(77)
    hseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    orc = _oracle('narrow', mb, NARROW, n_layers, p, hseed)
    plans = []
    backward = lib.eagcn_model_backward

    def planned_backward(b, m, size, saved, saved_bytes, scratch, scratch_bytes, *rest):
        out = (C.c_int32 * 16 * 4)()
        _lib.check(lib.eagcn_model_route(b, m, saved, saved_bytes, scratch, scratch_bytes, 1, n_layers - 1, 0, 0, 0, C.byref(out)), 'eagcn_model_route')
        plans.append([list(row) for row in out])
        return backward(b, m, size, saved, saved_bytes, scratch, scratch_bytes, *rest)
    monkeypatch.setattr(lib, 'eagcn_model_backward', planned_backward)
    old = lib.eagcn_set_bx3_wide(1) if wide else None
    try:
        dev = torch.device('cuda', 0)
        hip = EAGCN(NARROW['chans'][0], 24, n_den1=N_DEN1, n_den2=N_DEN2, nclass=NCLASS, dropout=p, structure='Concate', molfp_mode='sum',
                    n_layers=n_layers, widths1=NARROW['w1'], widths2=NARROW['w2'], rel_channels=NARROW['chans'], grad_mode='direct',
                    graph=False, validate='deferred').to(dev).train()
        hip.load_state_dict(orc['sd'], strict=True)
        dense = tuple(t.to(dev) for t in mb.dense())
        labels = torch.from_numpy(mb.labels).to(dev)
        bw = torch.tensor(bce_weights(NCLASS), dtype=torch.float32, device=dev)
        lib.eagcn_hidden_bn_sums_taken(1)
        lib.eagcn_first_layer_fused_taken(1)
        torch.manual_seed(77)
        out, _, gr = hip(*dense)
        fused_classification_loss(out, labels, bw).backward()
        torch.cuda.synchronize()
        taken = (lib.eagcn_hidden_bn_sums_taken(1), lib.eagcn_first_layer_fused_taken(1))
    finally:
        if wide:
            lib.eagcn_set_bx3_wide(old)
    assert len(plans) == 1, len(plans)
    bits = [row[14] for row in plans[0][:n_layers]]
    print('plan bits per layer: %s, taken (hidden sums, first-layer dW): %s' % (bits, taken))
    assert taken == (sum(bool(v & 32) for v in bits), sum(bool(v & 128) for v in bits)), (taken, bits)
    assert [bool(v & 32) for v in bits] == ([False] * 3 if wide else [True, True, False]), bits
    assert [bool(v & 256) for v in bits] == [False, wide, wide] and [bool(v & 64) for v in bits] == [False, not wide, not wide], bits
    grads = {k: q.grad.detach().clone() for k, q in hip.named_parameters() if q.grad is not None}
    g32, g64 = orc['g32'], orc['g64']
    assert set(grads) == set(g32)
    scale = max(v.abs().max().item() for v in g32.values())
    for k in sorted(grads):
        assert_grad_parity(grads[k], g32[k], lambda k=k: g64[k], scale, '%s narrow/%s' % (k, 'wide' if wide else 'by_size'))


def test_tile_edges_on_the_wide_kernel():
    """The 256 x 128 kernel does not carry the tail pass: its launches leave the layer below on the reduction pass.  The library reads
    EAGCN_BX3_WIDE once: a child process runs the three-layer dropout case of test_tile_edges with it set -- _check asserts there that
    the library's setting is `always the 256 x 128 kernel`, the step that the route was NOT taken with either switch setting, and
    everything else as ever (the step must not fail, the gradients hold their bounds)"""
    env = dict(os.environ, EAGCN_BX3_WIDE='1')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider',
                        os.path.abspath(__file__) + '::test_tile_edges[3-0.3-eager]'], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and '1 passed' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
