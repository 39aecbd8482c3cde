"""Per-bond attributions (csrc/battr.hip, EAGCN.bond_attributions) against the CPU oracle's autograd (tests/bond_attr_reference.py):
gradient x attention and gradient x relation input per view, judged with the project's three-way rule (1e-5 of the tensor's own
largest entry, or no farther from float64 than the fp32 oracle is) per view with the largest entry over the views as scale; the
structure of the result, run-to-run identity, agreement of the dense / compact / graph-model calls, and what a call must leave
untouched."""
import copy

import numpy as np
import pytest
import torch

from bond_attr_reference import autograd_scores, target_weights
from helpers import Golden, assert_grad_parity, build_oracle_model

pytestmark = pytest.mark.gpu

GOLDEN = ['model_concate_eval', 'model_weighted_eval', 'model_gcn_eval', 'model_concate_isolated', 'model_concate_single_atom',
          'model_concate_bigN']
GOLDEN_CASES = [(n, m) for n in GOLDEN for m in ('attention', 'relation') if not (n == 'model_gcn_eval' and m == 'relation')]


def _dev(ts):
    return [t.cuda() for t in ts]


def _targets(B, nclass):
    return [nclass - 1, torch.randn(B, nclass, generator=torch.Generator().manual_seed(11))]


def _judge(res, ref, cpu, target, mode, name):
    """res: BondAttributions of the HIP model; ref: the fp32 oracle (eval); every view against the oracle's autograd"""
    B, nclass = cpu[0].shape[0], ref.den3.weight.shape[1]
    dout = target_weights(B, nclass, target)
    s32 = autograd_scores(ref, cpu, dout, mode)
    cache = {}

    def s64():
        if 'v' not in cache:
            cache['v'] = autograd_scores(copy.deepcopy(ref).double().eval(), cpu, dout.double(), mode)
        return cache['v']
    got = res.dense('all').cpu()
    assert got.shape == s32.shape, (got.shape, s32.shape)
    scale = s32.abs().max().item()
    assert scale > 0
    for k in range(s32.shape[0]):
        print('%s view %d: max |got - ref32| = %.3e, own max %.3e, scale %.3e'
              % (name, k, (got[k].double() - s32[k].double()).abs().max().item(), s32[k].abs().max().item(), scale))
        assert_grad_parity(got[k], s32[k], lambda k=k: s64()[k], scale, '%s view %d' % (name, k))
    assert (res.per_view.sum(0) - res.score).abs().max().item() <= 1e-6 * scale
    return scale


def _structure_checks(res, adj):
    """entries = exactly the non-zeros of adj, in row-major order; nothing but exact zeros off the bonds"""
    nz = (adj != 0).nonzero().cpu()
    got = torch.stack([res.mol, res.i, res.j], 1).long().cpu()
    assert got.shape == nz.shape and (got == nz).all()
    off = adj == 0
    assert (res.dense()[off] == 0).all() and (res.dense('all')[:, off] == 0).all()
    bondless = (adj.sum((1, 2)) == 0).nonzero().flatten().tolist()
    assert not set(bondless) & set(res.mol.tolist())
    und = res.undirected()
    d = res.dense()
    assert torch.equal(und, torch.triu(0.5 * (d + d.transpose(1, 2)), diagonal=1))


def _golden_models(name):
    from eagcn_amd import EAGCN
    g = Golden(name)
    meta = g.meta
    ref = build_oracle_model(meta)
    ref.load_state_dict(g.state_dict(), strict=True)
    hip = EAGCN(meta['n_bfeat'], meta['n_afeat'], *meta['widths1'], *meta['widths2'], meta['dens'][0], meta['dens'][1],
                meta['nclass'], 0.0, structure=meta['structure'], molfp_mode=meta['molfp'])
    hip.load_state_dict(g.state_dict(), strict=True)
    return g, hip.cuda().eval(), ref.eval()


@pytest.mark.parametrize('name,mode', GOLDEN_CASES)
def test_golden_models_vs_oracle(name, mode):
    g, hip, ref = _golden_models(name)
    cpu = g.batch.dense()
    dev = _dev(cpu)
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    for target in _targets(g.batch.B, g.meta['nclass']):
        res = hip.bond_attributions(adj, afm, *rels, size=size, target=target.cuda() if torch.is_tensor(target) else target,
                                    mode=mode)
        _judge(res, ref, cpu, target, mode, '%s %s' % (name, mode))
        _structure_checks(res, adj)
    if name == 'model_concate_single_atom':
        assert (adj.sum((1, 2)) == 0).any()              # the case holds a molecule without bonds


W1, W2 = [30, 10, 10, 10, 20], [60, 20, 20, 20, 20]      # Tox21 widths: 80 / 140 in all (Weighted_sum: 140 -> 144 padded columns)


def _pair(structure, w1=W1, w2=W2, channels=(28, 4, 2, 2, 2), nclass=12, seed=3, **kw):
    """(HIP model, fp32 oracle), eval mode, non-trivial running statistics and attention logits of O(1)"""
    from eagcn_amd import EAGCN
    from oracle.eagcn_ref import RefEAGCN, weights_init_
    torch.manual_seed(seed)
    ref = RefEAGCN(channels[0], 24, w1, w2, 64, 32, nclass, 0.0, structure=structure, n_layers=2, rel_channels=list(channels))
    weights_init_(ref)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    if structure != 'GCN':
        for l in (ref.layer1, ref.layer2):
            for k in range(len(w1)):
                getattr(l, 'block%d' % (k + 1)).att.weight.data.normal_(0.0, 0.8)
    hip = EAGCN(channels[0], 24, widths1=w1, widths2=w2, n_den1=64, n_den2=32, nclass=nclass, dropout=0.0, structure=structure,
                n_layers=2, rel_channels=list(channels), **kw)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.cuda().eval(), ref.eval()


def _call(hip, dev, target, mode, **kw):
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    return hip.bond_attributions(adj, afm, *rels, size=size, target=target.cuda() if torch.is_tensor(target) else target, mode=mode, **kw)


@pytest.mark.parametrize('mode', ['attention', 'relation'])
@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_tox21_widths_vs_oracle(structure, mode):
    from eagcn_amd.synthetic import make_batch
    hip, ref = _pair(structure)
    mb = make_batch(B=8, n_max=40, n_med=16, seed=5)
    cpu = mb.dense()
    dev = _dev(cpu)
    for target in _targets(8, 12):
        res = _call(hip, dev, target, mode, dense=True)
        _judge(res, ref, cpu, target, mode, 'tox21 %s %s' % (structure, mode))
        _structure_checks(res, dev[0])


@pytest.mark.parametrize('mode', ['attention', 'relation'])
def test_wide_layers_vs_oracle(mode):
    """the launch shapes the Tox21 widths do not reach: 5 x 176 = 880 packed columns (four 256-column chunks per lane) and
    5 x 416 = 2080 (a launch of eight chunks and a second launch for the 32 columns beyond 2048)"""
    from eagcn_amd import ops
    from eagcn_amd.synthetic import make_batch
    hip, ref = _pair('Weighted_sum', [36, 35, 35, 35, 35], [84, 83, 83, 83, 83], nclass=2)
    assert hip.layer1.spec_for(ops.ColLayout.single(24)).fp == 880 and hip.layer2.spec_for(ops.ColLayout.single(176, 16)).fp == 2080
    mb = make_batch(B=4, n_max=12, n_med=8, seed=12)
    cpu = mb.dense()
    dev = _dev(cpu)
    res = _call(hip, dev, 1, mode)
    _judge(res, ref, cpu, 1, mode, 'wide %s' % mode)
    _structure_checks(res, dev[0])


@pytest.mark.parametrize('mode', ['attention', 'relation'])
def test_molecule_above_256_atoms_vs_oracle(mode):
    """a 272-atom molecule: the forward runs on the matrix-core aggregation, the bond kernel gathers from global memory all the same"""
    from eagcn_amd.synthetic import make_batch
    hip, ref = _pair('Concate', [4, 3, 2, 2, 3], [5, 3, 2, 2, 4], nclass=2)
    mb = make_batch(B=2, n_max=272, n_med=60, seed=9)
    assert mb.sizes.max() == 272
    cpu = mb.dense()
    dev = _dev(cpu)
    res = _call(hip, dev, 1, mode)
    _judge(res, ref, cpu, 1, mode, 'n272 %s' % mode)
    _structure_checks(res, dev[0])


def test_run_to_run_identity_and_call_paths_agree():
    from eagcn_amd.synthetic import make_batch
    hip, ref = _pair('Concate')
    mb = make_batch(B=8, n_max=40, n_med=16, seed=6)
    dev = _dev(mb.dense())
    target = torch.randn(8, 12, generator=torch.Generator().manual_seed(2))
    a = _call(hip, dev, target, 'attention')
    b = _call(hip, dev, target, 'attention', dense=True)
    for x, y in ((a.mol, b.mol), (a.i, b.i), (a.j, b.j), (a.per_view, b.per_view), (a.score, b.score), (a.dense('all'), b.dense('all'))):
        assert torch.equal(x, y)
    scale = a.per_view.abs().max().item()
    # the compact batch
    bonds, afm_c, size_c = mb.compact(torch.device('cuda', 0))
    c = hip.bond_attributions(None, afm_c, size=size_c, target=target.cuda(), bonds=bonds)
    assert (c.dense('all') - a.dense('all')).abs().max().item() <= 1e-6 * scale
    # a graph-mode model takes the same eager path
    hg, _ = _pair('Concate', graph=True)
    hg.load_state_dict(hip.state_dict(), strict=True)
    d = _call(hg.eval(), dev, target, 'attention')
    assert (d.dense('all') - a.dense('all')).abs().max().item() <= 1e-6 * scale


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_call_leaves_model_state_untouched(structure):
    from eagcn_amd.synthetic import make_batch
    hip, _ = _pair(structure)
    mb = make_batch(B=8, n_max=40, n_med=16, seed=7)
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    out, _, _ = hip(adj, afm, *rels, size)               # some parameter gradients to find unchanged
    out.sum().backward()
    grads = {k: p.grad.clone() for k, p in hip.named_parameters() if p.grad is not None}
    assert grads
    state = {k: v.clone() for k, v in hip.state_dict().items()}
    score0, attr0 = hip.atom_attributions(adj, afm, *rels, size=size, target=0)
    _call(hip, dev, 0, 'attention')
    _call(hip, dev, 3, 'relation')
    for k, p in hip.named_parameters():
        if k in grads:
            assert torch.equal(p.grad, grads[k]), k
        else:
            assert p.grad is None, k
    for k, v in hip.state_dict().items():
        assert torch.equal(v, state[k]), k
    assert afm.grad is None and not afm.requires_grad
    score1, attr1 = hip.atom_attributions(adj, afm, *rels, size=size, target=0)
    assert torch.equal(score0, score1) and torch.equal(attr0, attr1)


def _general_dense(seed, B, channels):
    """a batch whose relation tensors hold, at every bond, one of a handful of REAL-valued multi-hot channel vectors (symmetric
    per bond), as tests/test_gpu_general_relations.py builds them"""
    from eagcn_amd.synthetic import make_batch
    rng = np.random.default_rng(seed)
    mb = make_batch(B=B, n_max=21, n_med=9, rel_channels=channels, seed=seed, isolated_frac=0.1)
    dense = [t.numpy() for t in mb.dense()]
    adj = dense[0]
    palettes = [np.round(rng.normal(0.0, 1.0, size=(5 + k, c)), 2).astype(np.float32) * (rng.random((5 + k, c)) < 0.6)
                for k, c in enumerate(channels)]
    rels = [np.zeros((B, c, mb.N, mb.N), dtype=np.float32) for c in channels]
    for b in range(B):
        i, j = np.nonzero(np.triu(adj[b]))
        for k, pal in enumerate(palettes):
            pick = pal[rng.integers(0, len(pal), size=len(i))]
            rels[k][b][:, i, j] = pick.T
            rels[k][b][:, j, i] = pick.T
    return [torch.from_numpy(t) for t in [adj, dense[1]] + rels] + [torch.from_numpy(mb.sizes)]


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_general_relation_tensors_vs_oracle(structure):
    channels = (6, 4, 3, 2, 2)
    cpu = _general_dense(17, 9, channels)
    hip, ref = _pair(structure, [8, 6, 4, 4, 6], [10, 8, 6, 6, 6], channels=channels, nclass=2, relations='general')
    dev = _dev(cpu)
    for mode in ('relation', 'attention'):
        res = _call(hip, dev, 1, mode)
        _judge(res, ref, cpu, 1, mode, 'general %s %s' % (structure, mode))
        _structure_checks(res, dev[0])


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_diagonal_and_one_directional_bonds_vs_oracle(structure):
    from eagcn_amd.synthetic import make_batch
    channels = (28, 4, 2, 2, 2)
    mb = make_batch(B=4, n_max=12, n_med=8, seed=21)
    cpu = [t.clone() for t in mb.dense()]
    adj, rels = cpu[0], cpu[2:-1]

    def add(b, i, j):
        assert adj[b, i, j] == 0
        adj[b, i, j] = 1.0
        for k, r in enumerate(rels):
            r[b, (3 * i + j + k) % channels[k], i, j] = 1.0
    deg = adj.sum(2)
    add(0, 1, 1)                                          # a bond on the diagonal
    b = 1
    n = int((deg[b] > 0).nonzero().max()) + 1             # atoms with a bond of their own: 0 .. n-1 are stored rows
    i, j = next((i, j) for i in range(n) for j in range(n) if i != j and adj[b, i, j] == 0 and deg[b, i] > 0 and deg[b, j] > 0)
    add(b, i, j)                                          # a one-directional bond between two stored atoms
    assert adj[b, j, i] == 0
    hip, ref = _pair(structure, [8, 6, 4, 4, 5], [10, 7, 5, 6, 4], nclass=2)
    dev = _dev(cpu)
    for mode in ('attention', 'relation'):
        res = _call(hip, dev, 0, mode)
        _judge(res, ref, cpu, 0, mode, 'directed %s %s' % (structure, mode))
        _structure_checks(res, dev[0])


def test_unsupported_calls_raise():
    from eagcn_amd import EAGCN
    from eagcn_amd._lib import EagcnHipError
    from eagcn_amd.synthetic import make_batch
    mb = make_batch(B=4, n_max=12, n_med=8, seed=4)
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    w1, w2 = [8, 6, 4, 4, 5], [10, 7, 5, 6, 4]

    def model(structure, molfp='sum', n_layers=2):
        return EAGCN(28, 24, widths1=w1, widths2=w2, n_den1=16, n_den2=8, nclass=2, dropout=0.0, structure=structure,
                     molfp_mode=molfp, n_layers=n_layers).cuda().eval()
    with pytest.raises(EagcnHipError, match='GAT'):
        model('GAT').bond_attributions(adj, afm, *rels, size=size, target=0)
    with pytest.raises(EagcnHipError, match='pool'):
        model('Concate', 'pool', 4).bond_attributions(adj, afm, *rels, size=size, target=0)
    with pytest.raises(EagcnHipError, match='eval'):
        model('Concate').train().bond_attributions(adj, afm, *rels, size=size, target=0)
    with pytest.raises(EagcnHipError, match='relation'):
        model('GCN').bond_attributions(adj, afm, *rels, size=size, target=0, mode='relation')
    with pytest.raises(ValueError):
        model('Concate').bond_attributions(adj, afm, *rels, size=size, target=0, mode='saliency')
    res = model('GCN').bond_attributions(adj, afm, *rels, size=size, target=0)       # (attention mode is served)
    assert res.per_view.shape[0] == 1 and res.score.numel() == int(adj.sum().item())
