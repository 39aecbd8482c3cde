"""The top layer's BatchNorm backward from the read-out's per-molecule sums (csrc/readout.hip A1 / A2, csrc/head2.hip HeadTopSums,
csrc/layer.hip BN2_STAGED_FROM_READOUT, csrc/lagg_top.hip) against the reduction pass over the rows it replaces
(eagcn_set_top_bn_sums(0)) and against the oracle.

One batch small enough to sit on the corners: B = 6, N_pad = 20, molecules of 1, 2, 5, 20, 20 and 3 atoms (the one-atom molecule has no
packed row), one atom with six bonds (overflow record of the LDS-staged kernel), one trailing bond-less atom (counted by `size`, not
stored), K = 2 views of exact widths 12 and 20 (packed 16 and 32: padded columns), two layers; dropout 0 and 0.3, read-out sum and
ave, eager engine and the captured fused step (the eager cases also with the switch at 2: rows of the read-out gradient instead of
the per-molecule gather).  With the switch at 1 and at 0 the forward is the same code but for two extra stores:
outputs, graph_representation, running statistics and loss must be bit-identical.  The gradients of the switch-1 run are held to
helpers.assert_grad_parity at its default tolerances (fp32 oracle, else no farther from the fp64 oracle than the fp32 oracle is)."""
import copy

import numpy as np
import pytest
import torch

from eagcn_amd.synthetic import MolBatch, bce_weights
from helpers import assert_grad_parity

pytestmark = pytest.mark.gpu

CHANS = [6, 4]
W1, W2 = [9, 7], [12, 20]
N_DEN1, N_DEN2, NCLASS = 20, 10, 3


def _mol_batch(sizes, bonds, N, seed):
    """bonds: per molecule a list of undirected (i, j)"""
    rng = np.random.default_rng(seed)
    B = len(sizes)
    eb, ei, ej, cd = [], [], [], []
    for b, prs in enumerate(bonds):
        for (i, j) in prs:
            c = [int(rng.integers(0, ch)) for ch in CHANS]
            for (p, q) in ((i, j), (j, i)):
                eb.append(b); ei.append(p); ej.append(q); cd.append(c)
    edges = np.stack([np.array(eb), np.array(ei), np.array(ej)], axis=1).astype(np.int64)
    codes = np.array(cd, dtype=np.int64).reshape(len(eb), len(CHANS))
    afm = np.zeros((B, N, 24), dtype=np.float32)
    for b, n in enumerate(sizes):
        afm[b, :n, :] = rng.random((n, 24), dtype=np.float32)
    labels = np.array([[1, 0, -1], [0, 0, 1], [-1, 1, 0], [0, 1, 1], [1, -1, 0], [0, 0, 0]], dtype=np.float32)[:B]
    return MolBatch(B=B, N=N, n_afeat=24, rel_channels=list(CHANS), sizes=np.array(sizes, dtype=np.int64), edges=edges, codes=codes,
                    afm=afm, labels=labels)


def _corner_batch():
    chain = lambda a, b: [(i, i + 1) for i in range(a, b)]
    bonds = [[],                                                  # one atom: no bond, no packed row
             [(0, 1)],
             chain(0, 4),
             [(0, j) for j in range(1, 7)] + chain(6, 19) + [(3, 11)],        # atom 0: six bonds; one ring closure
             chain(0, 18) + [(2, 9)],                                         # atom 19 has no bond: trailing, not stored
             chain(0, 2)]
    return _mol_batch([1, 2, 5, 20, 20, 3], bonds, 20, 5)


def _tiny_batch():
    """B = 3 and T = 5 packed rows: fewer than the seven rows one slab of the reduction pass covers -- the finalize must still add
    up every slab of the read-out's sums"""
    return _mol_batch([2, 3, 1], [[(0, 1)], [(0, 1), (1, 2)], []], 3, 6)


_ORACLE = {}


def _oracle(name, mb, mode, p, hseed):
    """fp32 and fp64 oracle of one step (same parameters, the kernels' dropout masks injected): computed once per (batch, mode, p)"""
    key = (name, mode, p)
    if key in _ORACLE:
        assert _ORACLE[key]['hseed'] == hseed
        return _ORACLE[key]
    import oracle.eagcn_ref as R
    from eagcn_amd.losses import classification_loss
    from test_gpu_parity import _hip_dropout_masks
    torch.manual_seed(3)
    ref = R.RefEAGCN(CHANS[0], 24, W1, W2, N_DEN1, N_DEN2, NCLASS, p, structure='Concate', molfp_mode=mode, n_layers=2, rel_channels=CHANS)
    R.weights_init_(ref)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    ref64 = copy.deepcopy(ref).double()
    cpu = mb.dense()
    labels = torch.from_numpy(mb.labels)
    bw = bce_weights(NCLASS)
    masks = _hip_dropout_masks(mb, [W1, W2], 'Concate', N_DEN1, p, hseed) if p > 0 else []
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


def _hip_step(lib, switch, mb, mode, p, graph, sd):
    """one training step with the switch at `switch`: (loss, out, graph_rep, gradients, state_dict after the step, dropout seed)"""
    from eagcn_amd import EAGCN
    from eagcn_amd.losses import fused_classification_loss
    dev = torch.device('cuda', 0)
    old = lib.eagcn_set_top_bn_sums(switch)
    try:
        hip = EAGCN(CHANS[0], 24, n_den1=N_DEN1, n_den2=N_DEN2, nclass=NCLASS, dropout=p, structure='Concate', molfp_mode=mode, n_layers=2,
                    widths1=W1, widths2=W2, rel_channels=CHANS, grad_mode='direct', graph=graph, validate='deferred').to(dev).train()
        if sd is not None:
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
        return loss.detach().clone(), out.detach().clone(), gr.detach().clone(), grads, state, hseed
    finally:
        lib.eagcn_set_top_bn_sums(old)


def _check(name, mb, mode, p, graph):
    from eagcn_amd import _lib
    lib = _lib.load()
    assert lib.eagcn_set_top_bn_sums(1) == 1          # the default
    # (the oracle draws the parameters; the dropout seed is a function of torch's generator state alone)
    torch.manual_seed(77)
    hseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    orc = _oracle(name, mb, mode, p, hseed)
    l1, o1, g1, gr1, st1, hs1 = _hip_step(lib, 1, mb, mode, p, graph, orc['sd'])
    l0, o0, g0, gr0, st0, hs0 = _hip_step(lib, 0, mb, mode, p, graph, orc['sd'])
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
    worst = 0.0
    for k in sorted(gr1):
        d = (gr1[k].double().cpu() - gr0[k].double().cpu()).abs().max().item()
        worst = max(worst, d / scale)
    print('%s mode=%s p=%s graph=%s: max |grad(1) - grad(0)| / scale = %.3e' % (name, mode, p, graph, worst))
    tag = '%s/%s/p%s/%s' % (name, mode, p, 'graph' if graph else 'eager')
    for k in sorted(gr1):
        assert_grad_parity(gr1[k], g32[k], lambda k=k: g64[k], scale, '%s %s' % (k, tag))
    if graph:
        return
    # switch at 2: the same sums, the read-out gradient written out as rows instead of gathered per molecule (the form that view
    # widths which are no multiples of four take): same forward, same bounds
    l2, o2, g2, gr2, st2, _ = _hip_step(lib, 2, mb, mode, p, graph, orc['sd'])
    assert torch.equal(l2, l0) and torch.equal(o2, o0) and torch.equal(g2, g0)
    for k in st2:
        assert torch.equal(st2[k], st0[k]), k
    assert set(gr2) == set(g32)
    for k in sorted(gr2):
        assert_grad_parity(gr2[k], g32[k], lambda k=k: g64[k], scale, '%s %s rows' % (k, tag))


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('mode', ['sum', 'ave'])
@pytest.mark.parametrize('p', [0.0, 0.3])
def test_top_bn_sums_equal_reduction_pass(p, mode, graph):
    _check('corner', _corner_batch(), mode, p, graph)


def test_fewer_rows_than_one_slab_of_the_row_pass():
    _check('tiny', _tiny_batch(), 'sum', 0.0, False)
