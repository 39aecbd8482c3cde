"""Atom-feature gradients and per-atom attributions on the model engine (eagcn_model_backward_input, csrc/attr.hip,
EAGCN.atom_attributions): d/d afms through autograd against the float64 oracle and the reference's attribution vectors
(tests/golden/attr_*), the input-only backward against the full one, integrated-gradients completeness, per-molecule
independence in eval mode, and agreement of the eager / graph / compact / direct paths and of the composed fallback."""
import copy

import pytest
import torch

from helpers import Golden, assert_grad_parity, build_oracle_model, golden_cases, rel_err

pytestmark = pytest.mark.gpu

ENGINE_CASES = [n for n in golden_cases('model')
                if Golden(n).meta['structure'] in ('Concate', 'Weighted_sum', 'GCN') and Golden(n).meta['molfp'] in ('sum', 'ave')]
ATTR_CASES = golden_cases('attr')


def _dev(ts):
    return [t.cuda() for t in ts]


def _hip(meta, **kw):
    from eagcn_amd import EAGCN
    return EAGCN(meta['n_bfeat'], meta['n_afeat'], *meta['widths1'], *meta['widths2'], meta['dens'][0], meta['dens'][1],
                 meta['nclass'], 0.0, structure=meta['structure'], molfp_mode=meta['molfp'], **kw)


def _oracle(g):
    ref = build_oracle_model(g.meta)
    ref.load_state_dict(g.state_dict(), strict=True)
    ref.train(g.meta['training'])
    return ref


def _cotangents(g, out_shape, gr_shape):
    gen = torch.Generator().manual_seed(77)
    G = torch.from_numpy(g.z['gout']) if 'gout' in g.z.files else torch.randn(out_shape, generator=gen)
    G2 = torch.from_numpy(g.z['gout_graph_rep']) if 'gout_graph_rep' in g.z.files else torch.randn(gr_shape, generator=gen) * 0.1
    return G, G2


def _oracle_afm_grad(ref, cpu, G, G2, cast=lambda t: t):
    adj, afm, rels, size = cpu[0], cpu[1], cpu[2:-1], cpu[-1]
    x = cast(afm).clone().requires_grad_(True)
    out, _, gr = ref(cast(adj), x, *[cast(r) for r in rels], size)
    ((out * cast(G)).sum() + (gr * cast(G2)).sum()).backward()
    return x.grad


@pytest.mark.parametrize('name', ENGINE_CASES)
def test_afm_grad_through_autograd_vs_oracle(name):
    """model(adj, afm.requires_grad_(), ...) + backward gives afm.grad (the forward used to raise); parameter gradients are the
    ones of the same backward without d/d afm."""
    g = Golden(name)
    cpu = g.batch.dense()
    ref = _oracle(g)
    ref32 = copy.deepcopy(ref)
    hip = _hip(g.meta)
    hip.load_state_dict(g.state_dict(), strict=True)
    hip.cuda().train(g.meta['training'])
    plain = copy.deepcopy(hip)
    dev = _dev(cpu)
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    x = afm.clone().requires_grad_(True)
    out, _, gr = hip(adj, x, *rels, size)
    G, G2 = _cotangents(g, out.shape, gr.shape)
    ((out * G.cuda()).sum() + (gr * G2.cuda()).sum()).backward()
    assert x.grad is not None
    g32 = _oracle_afm_grad(ref32, cpu, G, G2)
    scale = g32.abs().max().item()

    def g64():
        twin = copy.deepcopy(ref).double()
        return _oracle_afm_grad(twin, cpu, G, G2, lambda t: t.double() if t.is_floating_point() else t)
    assert_grad_parity(x.grad.cpu(), g32, g64, scale, name + ' afm', rtol=1e-5)
    # parameter gradients: the same as the backward that forms no d/d afm
    out2, _, gr2 = plain(adj, afm, *rels, size)
    ((out2 * G.cuda()).sum() + (gr2 * G2.cuda()).sum()).backward()
    pscale = max(p.grad.abs().max().item() for p in plain.parameters() if p.grad is not None)
    for (k, p), q in zip(hip.named_parameters(), plain.parameters()):
        if q.grad is None:
            assert p.grad is None, k
            continue
        err = (p.grad - q.grad).abs().max().item()
        assert err <= 1e-6 * q.grad.abs().max().item() + 1e-7 * pscale, (k, err)


@pytest.mark.parametrize('name', ATTR_CASES)
def test_attr_golden(name):
    g = Golden(name)
    hip = _hip(g.meta)
    hip.load_state_dict(g.state_dict(), strict=True)
    hip.cuda().train(g.meta['training'])
    dev = _dev(g.batch.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    gout = torch.from_numpy(g.z['gout']).cuda()
    x = afm.clone().requires_grad_(True)
    out, _, _ = hip(adj, x, *rels, size)
    (out * gout).sum().backward()
    assert rel_err(x.grad.cpu(), g.z['grad/afm'], 'grad/afm') < 1e-5
    if 'ig8/attr' in g.z.files:
        score, attr = hip.atom_attributions(adj, afm, *rels, size=size, target=gout, steps=g.meta['ig_steps'])
        assert rel_err(attr.cpu(), g.z['ig8/attr'], 'ig8/attr') < 1e-5
        assert rel_err(score.cpu(), g.z['ig8/score'], 'ig8/score') < 1e-5


def _tox_model(structure, graph=False, n_bfeat=28, **kw):
    from eagcn_amd import EAGCN
    from oracle.eagcn_ref import RefEAGCN, weights_init_
    torch.manual_seed(3)
    w1, w2 = ([80] * 5, [140] * 5) if structure == 'Concate' else ([40] * 5, [60] * 5)
    ref = RefEAGCN(n_bfeat, 24, w1, w2, 256, 64, 12, 0.0, structure=structure, n_layers=2)
    weights_init_(ref)
    for mod in ref.modules():                       # non-trivial running statistics for the eval BatchNorms
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
    hip = EAGCN(n_bfeat, 24, *w1, *w2, 256, 64, 12, 0.0, structure=structure, n_layers=2, graph=graph, **kw).cuda()
    hip.load_state_dict(ref.state_dict(), strict=True)
    return hip.eval(), ref.eval()


def _tox_batch(B=64, n_max=40, seed=5):
    from eagcn_amd.synthetic import make_batch
    return make_batch(B=B, n_max=n_max, n_med=16, rel_channels=(28, 4, 2, 2, 2), seed=seed)


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
@pytest.mark.parametrize('training', [False, True])
def test_input_only_equals_full(structure, training):
    hip, _ = _tox_model(structure)
    hip.train(training)
    mb = _tox_batch()
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    G = torch.randn(64, 12, generator=torch.Generator().manual_seed(1)).cuda()
    frozen = copy.deepcopy(hip)
    state = copy.deepcopy(hip.state_dict())
    x = afm.clone().requires_grad_(True)
    (hip(adj, x, *rels, size)[0] * G).sum().backward()                     # full: parameter gradients + d/d afm
    for p in frozen.parameters():
        p.requires_grad_(False)
    frozen.load_state_dict(state)
    y = afm.clone().requires_grad_(True)
    (frozen(adj, y, *rels, size)[0] * G).sum().backward()                  # input-only
    assert rel_err(y.grad, x.grad, 'input-only vs full') < 1e-6


def test_attributions_touch_no_grad_and_no_running_stat():
    hip, _ = _tox_model('Concate')
    mb = _tox_batch()
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    before = {k: v.clone() for k, v in hip.state_dict().items()}
    hip.atom_attributions(adj, afm, *rels, size=size, target=0, steps=4)
    hip.atom_attributions(adj, afm, *rels, size=size, target=0)
    assert all(p.grad is None for p in hip.parameters())
    for k, v in hip.state_dict().items():
        assert torch.equal(v, before[k]), k
    hip.train()
    with pytest.raises(Exception, match='eval'):
        hip.atom_attributions(adj, afm, *rels, size=size, target=0)


def test_ig_completeness():
    """|sum score - (f(x) - f(x'))| / |f(x) - f(x')| falls from m = 8 to m = 64 and is below 1e-3 there (zero baseline; the batch of
    attr_concate_eval under the 2-layer Tox21-width model -- the 4-layer fixture models are so kinked that the reference's own
    midpoint rule does not converge monotonically at these m)."""
    g = Golden('attr_concate_eval')
    hipg, _ = _tox_model('Concate', n_bfeat=g.meta['n_bfeat'])
    dev = _dev(g.batch.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    gout = torch.randn(afm.shape[0], 12, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        fx = (hipg(adj, afm, *rels, size)[0].double() * gout.double()).sum().item()
        f0 = (hipg(adj, torch.zeros_like(afm), *rels, size)[0].double() * gout.double()).sum().item()
    errs = {}
    for m in (8, 64):
        score, _ = hipg.atom_attributions(adj, afm, *rels, size=size, target=gout, steps=m)
        errs[m] = abs(score.double().sum().item() - (fx - f0)) / abs(fx - f0)
    assert errs[64] < errs[8], errs
    assert errs[64] < 1e-3, errs


def test_eval_independence():
    hip, _ = _tox_model('Weighted_sum')
    mb = _tox_batch(B=16)
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    score, _ = hip.atom_attributions(adj, afm, *rels, size=size, target=3)
    scale = score.abs().max().item()
    for b in (0, 7):
        s1, _ = hip.atom_attributions(adj[b:b + 1], afm[b:b + 1], *[r[b:b + 1] for r in rels], size=size[b:b + 1], target=3)
        assert (s1[0] - score[b]).abs().max().item() <= 1e-6 * scale, b
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(2)).cuda()
    sp, _ = hip.atom_attributions(adj[perm], afm[perm], *[r[perm] for r in rels], size=size[perm], target=3)
    assert (sp - score[perm]).abs().max().item() <= 1e-6 * scale


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
def test_paths_agree(structure):
    eager, _ = _tox_model(structure)
    graph, _ = _tox_model(structure, graph=True)
    mb = _tox_batch(B=32)
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    G = torch.randn(32, 12, generator=torch.Generator().manual_seed(4)).cuda()
    base = 0.1 * torch.ones_like(afm)
    s_e, a_e = eager.atom_attributions(adj, afm, *rels, size=size, target=G, steps=6, baseline=base)
    for _ in range(3):                                   # eager warm-up + capture, then replays
        s_g, a_g = graph.atom_attributions(adj, afm, *rels, size=size, target=G, steps=6, baseline=base)
        assert rel_err(a_g, a_e, 'graph vs eager') < 1e-6
        assert rel_err(s_g, s_e, 'graph vs eager score') < 1e-6
    graph.release_graphs()
    bonds, afm_c, size_c = mb.compact('cuda')
    s_c, a_c = eager.atom_attributions(None, afm_c, size=size_c, target=G, steps=6, baseline=base, bonds=bonds)
    assert rel_err(a_c, a_e, 'compact vs dense') < 1e-6
    # grad_mode='direct': parameters into .grad as today, afm through the returned tuple
    direct, _ = _tox_model(structure, grad_mode='direct')
    auto, _ = _tox_model(structure)
    xs = []
    for mdl in (direct, auto):
        x = afm.clone().requires_grad_(True)
        (mdl(adj, x, *rels, size)[0] * G).sum().backward()
        xs.append(x.grad)
    assert rel_err(xs[0], xs[1], 'direct vs autograd') < 1e-6
    both = [(p.grad, q.grad) for p, q in zip(direct.parameters(), auto.parameters()) if p.grad is not None and q.grad is not None]
    assert len(both) > 10
    for gp, gq in both:
        assert rel_err(gp, gq, 'direct param') < 1e-6


@pytest.mark.parametrize('structure', ['Concate', 'Weighted_sum'])
@pytest.mark.parametrize('training', [False, True])
def test_large_molecules_dense_aggregation(structure, training):
    """Molecules of more than 256 atoms: the transposed aggregation of agg.hip (no edge kernel) in the input-only backward -- eval mode
    through atom_attributions (dY' from the reduction kernel's APPLY pass with zero means), training mode through autograd with every
    parameter frozen (the BatchNorm reductions kept; Weighted_sum: with the gradient of the non-stored rows)."""
    hip, ref = _tox_model(structure)
    mb = _tox_batch(B=3, n_max=300, seed=9)
    cpu = mb.dense()
    dev = _dev(cpu)
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    G = torch.randn(3, 12, generator=torch.Generator().manual_seed(5))
    x = cpu[1].clone().requires_grad_(True)
    ref.train(training)
    out, _, _ = ref(cpu[0], x, *cpu[2:-1], cpu[-1])
    (out * G).sum().backward()
    if not training:
        score, attr = hip.atom_attributions(adj, afm, *rels, size=size, target=G.cuda())
        assert rel_err(attr.cpu(), cpu[1] * x.grad, 'N>256 attr') < 1e-5
        assert rel_err(score.cpu(), (cpu[1] * x.grad).sum(-1), 'N>256 score') < 1e-5
    else:
        hip.train()
        full = copy.deepcopy(hip)
        for p in hip.parameters():
            p.requires_grad_(False)
        y = afm.clone().requires_grad_(True)
        (hip(adj, y, *rels, size)[0] * G.cuda()).sum().backward()              # input-only
        z = afm.clone().requires_grad_(True)
        (full(adj, z, *rels, size)[0] * G.cuda()).sum().backward()             # full (today's dense-aggregation backward)
        assert rel_err(y.grad, z.grad, 'N>256 training input-only vs full') < 1e-6

        def g64():                                                              # float64 twin of the oracle, same training forward
            twin = copy.deepcopy(ref).double().train()
            xd = cpu[1].double().clone().requires_grad_(True)
            o, _, _ = twin(cpu[0].double(), xd, *[r.double() for r in cpu[2:-1]], cpu[-1])
            (o * G.double()).sum().backward()
            return xd.grad
        assert_grad_parity(y.grad.cpu(), x.grad, g64, x.grad.abs().max().item(), 'N>256 training d/d afm', rtol=1e-5)


@pytest.mark.parametrize('direct', [False, True])
def test_single_trainable_parameter_keeps_its_gradient(direct):
    """afm requires a gradient and only the FIRST hot parameter (layer 1, view 1 attention weight: plan.params[0]) does: the backward
    must take the full form and deliver that parameter's gradient, equal to the one of a fully trainable model."""
    hip, _ = _tox_model('Concate', grad_mode='direct' if direct else 'autograd')
    hip.train()
    full = copy.deepcopy(hip)
    mb = _tox_batch()
    dev = _dev(mb.dense())
    adj, afm, rels, size = dev[0], dev[1], dev[2:-1], dev[-1]
    G = torch.randn(64, 12, generator=torch.Generator().manual_seed(8)).cuda()
    first = hip.plan().params[0]
    for p in hip.parameters():
        p.requires_grad_(p is first)
    x = afm.clone().requires_grad_(True)
    (hip(adj, x, *rels, size)[0] * G).sum().backward()
    assert first.grad is not None, 'plan.params[0] lost its gradient'
    y = afm.clone().requires_grad_(True)
    (full(adj, y, *rels, size)[0] * G).sum().backward()
    ref_first = full.plan().params[0]
    assert rel_err(first.grad, ref_first.grad, 'params[0]') < 1e-6
    assert rel_err(x.grad, y.grad, 'afm') < 1e-6


@pytest.mark.parametrize('name', ['model_gat_eval', 'model_gat_pool_eval', 'model_weighted_pool_eval'])
def test_composed_fallback(name):
    g = Golden(name)
    hip = _hip(g.meta)
    hip.load_state_dict(g.state_dict(), strict=True)
    hip.cuda().eval()
    cpu = g.batch.dense()
    dev = _dev(cpu)
    ref = _oracle(g)
    G = torch.randn(cpu[0].shape[0], g.meta['nclass'], generator=torch.Generator().manual_seed(6))
    score, attr = hip.atom_attributions(dev[0], dev[1], *dev[2:-1], size=dev[-1], target=G.cuda())
    x = cpu[1].clone().requires_grad_(True)
    out, _, _ = ref(cpu[0], x, *cpu[2:-1], cpu[-1])
    (out * G).sum().backward()
    want = cpu[1] * x.grad
    assert rel_err(attr.cpu(), want, name + ' attr') < 1e-5
    assert rel_err(score.cpu(), want.sum(-1), name + ' score') < 1e-5
