"""Pin the CPU oracle (oracle/eagcn_ref.py) against every golden vector produced by the
unmodified reference (tools/make_golden.py).  fp32 CPU vs fp32 CPU, same ATen op sequence:
tolerance 2e-6 relative (max|d|/max|ref|).

The golden vectors hold the fp32 rounding of the BLAS kernels of the CPU they were made on.  The model
cases named in ILL_CONDITIONED amplify that rounding (BatchNorms over a few rows; a projection loss
whose terms cancel) beyond the tolerance on a CPU whose BLAS takes another code path.  There, and only
there, a value that misses its bound is arbitrated against the oracle evaluated in float64:
  * the golden value itself must lie within GOLDEN_F64 of that float64 result (a bound independent of
    the fp32 oracle: a bug in the oracle moves its float64 run away from the golden vector), and
  * the fp32 oracle must be at most ARB_SLACK times as far from it as the golden value is.
tools/oracle_arbitration.py prints both quantities for every value of these cases."""
import numpy as np
import pytest
import torch

from helpers import Golden, assert_grad_close, build_oracle_layer, build_oracle_model, golden_cases, rel_err

TOL = 2e-6
# case -> keys that may be arbitrated (None: every key).  The isolated-atom and single-atom cases miss their direct bounds on
# CPUs whose MKL takes its AVX2, SSE4.2 or vendor-generic code path (AMD EPYC); the pooled GAT case only in its cancelling
# projection loss; the pooled concate case in its output, whose golden value is itself 1.3e-6 from the exact one
ILL_CONDITIONED = {'model_concate_isolated': None, 'model_concate_single_atom': None, 'model_gat_pool_eval': ('out/loss',),
                   'model_concate_pool_train': ('out/out',)}
# largest ratio measured with tools/oracle_arbitration.py: 1.34 under MKL_ENABLE_INSTRUCTIONS=AVX2 / SSE4_2 and
# MKL_CBWR=COMPATIBLE on an AVX-512 Xeon, 2.02 on an AMD EPYC 9575F (MKL's generic path, no setting)
ARB_SLACK = 3.0
# |golden - f64| bounds, relative to the value's largest entry (outputs, layer outputs, state after the step; the loss:
# relative to max(1, |loss|), a projection loss to the sum of |terms|), for gradients relative to max(own largest entry,
# 1e-3 x the case's largest gradient).  Largest measured over all 22 model cases: 2.1e-6 and 4.6e-4
GOLDEN_F64 = {'value': 1e-5, 'grad': 2e-3}


def _scalar_loss(g, out, graph_rep):
    from oracle.eagcn_ref import classification_loss, regression_loss
    kind = g.meta['loss']
    if kind == 'proj':
        return (out * torch.from_numpy(g.z['gout'])).sum() + \
               (graph_rep * torch.from_numpy(g.z['gout_graph_rep'])).sum()
    labels = torch.from_numpy(g.z['labels'])
    if kind == 'bce':
        return classification_loss(out, labels, g.z['bce_weight'].tolist())
    return regression_loss(out, labels)


def _f64_case(g):
    """The golden model case evaluated by the oracle in float64: layer outputs, outputs, loss, gradients, state after."""
    import copy
    with torch.enable_grad():                      # (the caller may be inside a no_grad block)
        model = build_oracle_model(g.meta).double()
        model.load_state_dict({k: v.double() for k, v in g.state_dict().items()}, strict=True)
        model.train(g.meta['training'])
        dense = g.batch.dense()
        adj, afm, rels, size = dense[0].double(), dense[1].double(), [r.double() for r in dense[2:-1]], dense[-1]
        with torch.no_grad():
            layers = [x.detach() for x in copy.deepcopy(model).layer_outputs(adj, afm, *rels)]
        out, atom_rep, graph_rep = model(adj, afm, *rels, size)
        kind = g.meta['loss']
        if kind == 'proj':
            loss = (out * torch.from_numpy(g.z['gout']).double()).sum() + \
                   (graph_rep * torch.from_numpy(g.z['gout_graph_rep']).double()).sum()
        elif kind == 'bce':
            labels = torch.from_numpy(g.z['labels'])
            w = torch.tensor(g.z['bce_weight']).double()
            weights = ((labels == 1).double() * w[:, 0].view(1, -1) + (labels == 0).double() * w[:, 1].view(1, -1)).view(-1)
            non_nan = ((labels == 1).sum() + (labels == 0).sum()).double()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(
                out.view(-1), labels.double().view(-1), weight=weights, reduction='sum') / non_nan
        else:
            loss = torch.nn.functional.mse_loss(out.view(-1), torch.from_numpy(g.z['labels']).double().view(-1))
        loss.backward()
    res = {'out/layer%d' % (i + 1): x for i, x in enumerate(layers)}
    res.update({'out/out': out.detach(), 'out/atom_rep': atom_rep.detach(), 'out/graph_rep': graph_rep.detach(),
                'out/loss': loss.detach()})
    res.update({'grad/' + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    res.update({'sd_after/' + k: v for k, v in model.state_dict().items()})
    return res


def _loss_terms(g):
    """What a loss value's fp32 rounding scales with: the sum of |terms| of a projection loss (they cancel), else max(1, |loss|)."""
    if g.meta['loss'] == 'proj':
        return float(np.abs(g.z['out/out'] * g.z['gout']).sum() + np.abs(g.z['out/graph_rep'] * g.z['gout_graph_rep']).sum())
    return max(1.0, abs(float(g.z['out/loss'])))


def _golden_f64_bound(g, key, scale):
    """GOLDEN_F64 of the key's magnitude (see the constant)."""
    ref = np.abs(g.z[key])
    if key.startswith('grad/'):
        return GOLDEN_F64['grad'] * max(float(ref.max()), 1e-3 * float(scale))
    return GOLDEN_F64['value'] * (_loss_terms(g) if key == 'out/loss' else float(ref.max()))


class _Arbiter:
    """Decides a value of an ILL_CONDITIONED case that missed its direct bound (module docstring); a miss anywhere else
    fails with the direct comparison's message `miss`."""

    def __init__(self, name, g):
        self.name, self.g, self.f64 = name, g, None
        self.scale = max(np.abs(v).max() for v in g.group('grad/').values())

    def __call__(self, key, got, floor, miss):
        keys = ILL_CONDITIONED.get(self.name, ())
        assert keys is None or key in keys, miss
        if self.f64 is None:
            self.f64 = _f64_case(self.g)
        got = torch.as_tensor(got.detach() if torch.is_tensor(got) else got, dtype=torch.float64).reshape(-1)
        ref = torch.as_tensor(self.g.z[key], dtype=torch.float64).reshape(-1)
        exact = self.f64[key].detach().double().reshape(-1)
        e_orc = (got - exact).abs().max().item()
        e_ref = (ref - exact).abs().max().item()
        bound = _golden_f64_bound(self.g, key, self.scale)
        assert e_ref <= bound, (miss, key, 'golden vs f64', e_ref, 'allowed', bound)
        assert e_orc <= ARB_SLACK * e_ref + floor, (miss, key, 'oracle vs f64', e_orc, 'golden vs f64', e_ref, 'slack', ARB_SLACK)


def _check_rel(arb, key, got, tol=TOL):
    e = rel_err(got, arb.g.z[key])
    if e < tol:
        return
    arb(key, got, 1e-7 * float(np.abs(arb.g.z[key]).max()), (key, 'rel err', e, 'tol', tol))


@pytest.mark.parametrize('name', golden_cases('model'))
def test_model_matches_reference(name):
    g = Golden(name)
    arb = _Arbiter(name, g)
    model = build_oracle_model(g.meta)
    model.load_state_dict(g.state_dict(), strict=True)        # identical key set to the reference
    model.train(g.meta['training'])
    dense = g.batch.dense()
    adj, afm, rels, size = dense[0], dense[1], dense[2:-1], dense[-1]
    import copy
    probe = copy.deepcopy(model)
    with torch.no_grad():
        for i, x in enumerate(probe.layer_outputs(adj, afm, *rels)):
            _check_rel(arb, 'out/layer%d' % (i + 1), x)
    out, atom_rep, graph_rep = model(adj, afm, *rels, size)
    _check_rel(arb, 'out/out', out)
    _check_rel(arb, 'out/atom_rep', atom_rep)
    _check_rel(arb, 'out/graph_rep', graph_rep)
    loss = _scalar_loss(g, out, graph_rep)
    ref_loss = float(g.z['out/loss'])
    d_loss = abs(float(loss.detach()) - ref_loss)
    if d_loss > 5e-6 * max(1.0, abs(ref_loss)):
        # a projection loss cancels (its terms are up to 45x larger than the sum): its floor is 2 fp32 ulps of the terms
        arb('out/loss', loss, (2e-7 if g.meta['loss'] == 'proj' else 1e-7) * _loss_terms(g), ('out/loss', d_loss))
    loss.backward()
    grads = g.group('grad/')
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(grads), 'set of parameters that receive a gradient differs'
    scale = max(np.abs(v).max() for v in grads.values())
    for k, ref in grads.items():
        # per-tensor relative error, with an absolute floor for gradients that are analytically
        # zero (biases in front of a training-mode BatchNorm)
        try:
            assert_grad_close(got[k], ref, scale, k)
        except AssertionError as e:
            arb('grad/' + k, got[k], 1e-6 * float(scale), e.args)
    for k, ref in g.group('sd_after/').items():
        _check_rel(arb, 'sd_after/' + k, model.state_dict()[k].double())


@pytest.mark.parametrize('name', sorted(ILL_CONDITIONED))
def test_golden_vectors_of_ill_conditioned_cases_are_near_exact(name):
    """The independent half of the arbitration, checked whether or not a value needs it: every golden value of an
    ILL_CONDITIONED case lies within GOLDEN_F64 of the float64 oracle."""
    g = Golden(name)
    f64 = _f64_case(g)
    scale = max(np.abs(v).max() for v in g.group('grad/').values())
    for key, exact in f64.items():
        if key not in g.z.files or 'num_batches_tracked' in key:
            continue
        e = np.abs(g.z[key].astype(np.float64) - exact.detach().double().numpy()).max()
        assert e <= _golden_f64_bound(g, key, scale), (key, e, _golden_f64_bound(g, key, scale))


def test_arbiter_decides_a_layer_output_inside_no_grad():
    """Layer outputs are compared inside torch.no_grad(): arbitration there still builds the float64 run (with its
    backward), accepts a value as close to the exact answer as fp32 can be, and rejects one 1e-3 away."""
    name = 'model_concate_single_atom'
    g = Golden(name)
    exact = _f64_case(g)['out/layer1']
    den = float(np.abs(g.z['out/layer1']).max())
    with torch.no_grad():
        _Arbiter(name, g)('out/layer1', exact.float(), 1e-7 * den, 'miss')
        with pytest.raises(AssertionError):
            _Arbiter(name, g)('out/layer1', exact.float() * 1.001, 1e-7 * den, 'miss')


@pytest.mark.parametrize('where', ['head', 'layers'])
@pytest.mark.parametrize('name', sorted(ILL_CONDITIONED) + ['model_concate_train'])
def test_oracle_bug_is_not_arbitrated_away(monkeypatch, name, where):
    """A bug in the oracle shows in its fp32 and its float64 run alike; the golden vectors still catch it (the model output
    x 1.05, or every layer output x 1.01)."""
    from oracle.eagcn_ref import RefEAGCN
    if where == 'head':
        fwd = RefEAGCN.forward

        def forward(self, *a):
            out, atom_rep, graph_rep = fwd(self, *a)
            return out * 1.05, atom_rep, graph_rep
        monkeypatch.setattr(RefEAGCN, 'forward', forward)
    else:
        lo = RefEAGCN.layer_outputs

        def layer_outputs(self, *a, with_a=False):
            outs, att = lo(self, *a, with_a=True)
            outs = [x * 1.01 for x in outs]
            return (outs, att) if with_a else outs
        monkeypatch.setattr(RefEAGCN, 'layer_outputs', layer_outputs)
    with pytest.raises(AssertionError):
        test_model_matches_reference(name)


@pytest.mark.parametrize('name', golden_cases('layer'))
def test_layer_matches_reference(name):
    g = Golden(name)
    layer = build_oracle_layer(g.meta, g.batch.rel_channels)
    layer.load_state_dict(g.state_dict(), strict=True)
    layer.train(g.meta['training'])
    dense = g.batch.dense()
    adj, rels = dense[0], dense[2:-1]
    x_in = torch.from_numpy(g.z['x_in'].copy()).requires_grad_(True)
    y, a_w = layer(adj, x_in, *rels)
    assert rel_err(y, g.z['out/x']) < TOL
    assert rel_err(a_w, g.z['out/A_weight']) < TOL
    (y * torch.from_numpy(g.z['gout'])).sum().backward()
    grads = g.group('grad/')
    scale = max(np.abs(v).max() for v in grads.values())
    assert rel_err(x_in.grad, grads.pop('x_in')) < 2e-5
    for k, ref in grads.items():
        p = dict(layer.named_parameters())[k]
        assert_grad_close(p.grad, ref, scale, k)
    for k, ref in g.group('sd_after/').items():
        assert rel_err(layer.state_dict()[k].double(), ref) < TOL, k


def test_fewer_layers_equal_prefix_of_reference_stack():
    """n_layers extension: the first two layers of a 2-layer oracle are the reference's layer1/2."""
    g = Golden('model_concate_train')
    model = build_oracle_model(g.meta, n_layers=2)
    sd = {k: v for k, v in g.state_dict().items()
          if k.startswith('layer1.') or k.startswith('layer2.')}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected
    assert all(not m.startswith('layer') for m in missing)
    dense = g.batch.dense()
    with torch.no_grad():
        outs = model.layer_outputs(dense[0], dense[1], *dense[2:-1])
    assert rel_err(outs[0], g.z['out/layer1']) < TOL
    assert rel_err(outs[1], g.z['out/layer2']) < TOL
