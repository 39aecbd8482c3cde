"""Body of tests/test_gpu_agg_dispatch.py: cases of tests/agg_dispatch_cases.py through the HIP model and through the CPU oracle
(oracle/eagcn_ref.py, float32 and its float64 twin), one forward and one backward each.  Run as a script it is the subprocess
of the cases that need a switch (the library reads EAGCN_AGG and EAGCN_AGG_KSPLIT_MAXB once per process: the parent sets them):

    agg_dispatch_check.py [--save-dir D | --lds-dir D] CASE [CASE ...]

prints one line per case (what the case's two layers take, as restated by agg_dispatch_cases.dispatch; the achieved output error;
the worst gradient distance over its bound) and AGG_DISPATCH_OK at the end.  --save-dir: no comparison, the gradients of every
case are saved to D/CASE.pt (the parent runs this with EAGCN_AGG=lds);  --lds-dir: the saved gradients of such a run, the yardstick
of att.weight / self_r for the cases with edge_ref == 'lds'.

Tolerances (the project's rule): outputs and BatchNorm running statistics rel_err < 1e-5 against the float64 oracle; every
gradient helpers.assert_grad_parity against the oracle's fp32 gradient, arbitrated by the float64 twin (slack 1, rtol 1e-5,
floor 2e-6).  The one exception, for cases with molecules of 70 atoms and more and for att.weight / self_r only (the dense kernels
sum the 1e-9 filler products one by one in fp32): a tensor that misses the rule there is held
  * edge_ref 'lds': to the run of the bond-list path on the same batch, within the margin tests/test_gpu_lagg.py grants the pair of
    kernels (2e-5 of the tensor's own largest entry + 4e-6 of the case's scale);
  * edge_ref 'sentinel' (more than 256 atoms: no bond-list path): entry by entry to 1 % of the float64 value (plus the rule's floor,
    2e-6 of the case's scale, which is what the rule grants an entry that is zero).
"""
import copy
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import agg_dispatch_cases as T                                   # noqa: E402
from helpers import assert_grad_parity, rel_err                  # noqa: E402

N_AFEAT, DEN1, DEN2, NCLASS = 24, 32, 16, 3
# A relu is a step in the gradient: an fp32 pre-activation that lands on the other side of 0 than the oracle's changes a whole row's
# contribution, and with 10^5 .. 10^6 pre-activations per case some lie within fp32 rounding of 0 whatever the seed.  The relus are
# not what these cases are about (the aggregation runs in front of the BatchNorm), so oracle() SETTLES them: layer by layer, from
# the float64 oracle alone, every column's BatchNorm bias is moved by at most RELU_WINDOW to the middle of the widest gap between
# that column's pre-activations (a training-mode BatchNorm's bias shifts its column and nothing else).  The relus still gate about
# half of the entries; run_case asserts that none lies within RELU_MARGIN (32 ulp of fp32) of the boundary, relative to the layer
# view's largest pre-activation.  The head relus never gate (biases at 6).
RELU_WINDOW, RELU_MARGIN = 0.1, 4e-6


def is_edge(name):
    return name.endswith('self_r') or name.endswith('att.weight')


def inputs(case):
    """(dense CPU tensors of the batch as the oracle takes them, per-molecule tuples of a code-book batch or None)."""
    if case.general:
        dense, mols = T.general_dense(case.batch_key[1])
        return [torch.from_numpy(t) for t in dense], mols
    return list(case.batch().dense()), None


def _settle_relus(case, ref, dense):
    """Move the layers' BatchNorm biases of `ref` (see RELU_WINDOW above), layer 1 first: layer 2's input depends on it."""
    live = dense[0].max(dim=2)[0] > 0
    args = [to64(t) for t in dense[:-1]]
    for l in (1, 2):
        twin = copy.deepcopy(ref).double().train()
        layer = getattr(twin, 'layer%d' % l)
        zs = {}
        hooks = [getattr(layer, 'block%d' % (k + 1)).batch_norm.register_forward_hook(lambda m, i, o, k=k: zs.__setitem__(k, o.detach()))
                 for k in range(layer.K)]
        with torch.no_grad():
            twin.layer_outputs(*args)
        for h in hooks:
            h.remove()
        for k, z in zs.items():
            v = z[live] if case.structure == 'Concate' else z.reshape(-1, z.shape[-1])      # the entries whose relu matters
            edge = torch.full((1, v.shape[1]), 1.5 * RELU_WINDOW, dtype=v.dtype)
            v = torch.cat([v, edge, -edge]).sort(dim=0)[0]
            gap, mid = v[1:] - v[:-1], 0.5 * (v[1:] + v[:-1])
            best = torch.where(mid.abs() <= RELU_WINDOW, gap, torch.full_like(gap, -1.0)).argmax(dim=0, keepdim=True)
            shift = -mid.gather(0, best)[0]
            with torch.no_grad():
                getattr(getattr(ref, 'layer%d' % l), 'block%d' % (k + 1)).batch_norm.bn.bias.add_(shift.to(torch.float32))


def oracle(case, dense):
    """The float32 oracle in training mode with the case's parameters: attention weights of O(1) (the logits must matter),
    BatchNorm weights off 1, head biases at 6 (the head relus never gate), the layers' relus settled on the batch `dense`."""
    from oracle.eagcn_ref import RefEAGCN
    torch.manual_seed(zlib.crc32(case.name.encode()) & 0xFFFF)
    ref = RefEAGCN(case.channels[0], N_AFEAT, case.w1, case.w2, DEN1, DEN2, NCLASS, 0.0, structure=case.structure, n_layers=2,
                   rel_channels=list(case.channels))
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if name.endswith('att.weight'):
                p.normal_(0.0, 0.8)
            elif name.endswith('self_r'):
                p.normal_(0.0, 0.5)
            elif name.endswith('batch_norm.bn.weight') or name.endswith('batch_norm.bn.bias') or name.startswith('Graph_BN.'):
                # (Graph_BN.bias of O(1): the batch mean in front of bn_den1 is W . bias -- with a bias of 0 an analytic zero, with a
                #  small one a cancelled sum that carries the rounding of addends ten times its size)
                p.add_(torch.randn_like(p) * (1.0 if name == 'Graph_BN.bias' else 0.1))
        ref.bn_den1.bias.fill_(6.0)
        ref.bn_den2.bias.fill_(6.0)
    ref.train()
    _settle_relus(case, ref, dense)
    return ref


def relu_margin(case, model, dense, cast):
    """Smallest |pre-activation| / largest |pre-activation| of a layer view, over the entries whose relu matters (Concate masks
    the rows of atoms without bonds after the relu; Weighted_sum keeps every row), in a forward of `model`."""
    from oracle.eagcn_ref import _AtomBN
    zs = []
    hooks = [m.register_forward_hook(lambda mod, i, o: zs.append(o.detach())) for m in model.modules() if isinstance(m, _AtomBN)]
    with torch.no_grad():
        model(*[cast(t) for t in dense])
    for h in hooks:
        h.remove()
    live = dense[0].max(dim=2)[0] > 0
    worst = float('inf')
    for z in zs:
        a = z.abs() / z.abs().max()
        worst = min(worst, (a[live] if case.structure == 'Concate' else a).min().item())
    return worst


def to64(t):
    return t.double() if t.is_floating_point() else t


def run_oracle(model, dense, cot, cast):
    out, _, gr = model(*[cast(t) for t in dense])
    ((out * cast(cot)).sum() + 0.1 * gr.sum()).backward()
    return out.detach(), gr.detach()


def run_hip(case, sd, dense, mols, cot):
    from eagcn_amd import EAGCN
    dev = torch.device('cuda', 0)
    m = EAGCN(case.channels[0], N_AFEAT, widths1=case.w1, widths2=case.w2, n_den1=DEN1, n_den2=DEN2, nclass=NCLASS, dropout=0.0,
              structure=case.structure, n_layers=2, rel_channels=list(case.channels), grad_mode='direct')
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    if mols is not None:
        from eagcn_amd.collate import collate_compact
        bonds, afms, size, _ = collate_compact(mols, dev, general=True)
        assert bonds.rel_vectors is not None
        out, _, gr = m.forward_compact(bonds, afms, size)
    else:
        out, _, gr = m(*[t.to(dev) for t in dense])
    ((out * cot.to(dev)).sum() + 0.1 * gr.sum()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    stats = {k: v.detach().cpu() for k, v in m.state_dict().items() if 'running_' in k}
    return out.detach().cpu(), gr.detach().cpu(), grads, stats


def run_case(case, lds=None, save=None):
    """One case: returns its result line (printed by the caller); raises on a miss.  save: path the HIP gradients are written to
    INSTEAD of comparing;  lds: gradients of such a run."""
    dense, mols = inputs(case)
    ref = oracle(case, dense)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    torch.manual_seed(4)
    cot = torch.randn(case.batch().B, NCLASS)
    out_h, gr_h, g_h, st_h = run_hip(case, sd, dense, mols, cot)
    if save is not None:
        torch.save(g_h, save)
        return 'AGG_DISPATCH_SAVED %s' % case.name
    twin = copy.deepcopy(ref).double().train()
    margin64 = relu_margin(case, copy.deepcopy(twin), dense, to64)
    assert margin64 >= RELU_MARGIN, (case.name, 'a pre-activation of the float64 oracle lies at a relu boundary', margin64)
    run_oracle(ref, dense, cot, lambda t: t)
    out64, gr64 = run_oracle(twin, dense, cot, to64)
    e_out = max(rel_err(out_h, out64, 'out'), rel_err(gr_h, gr64, 'graph_rep'))
    assert e_out < 1e-5, (case.name, 'out / graph_rep', e_out)
    st64 = twin.state_dict()
    e_st, k_st = max((rel_err(v, st64[k], k), k) for k, v in st_h.items())
    assert e_st < 1e-5, (case.name, 'running statistics', k_st, e_st)
    g32 = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}
    g64 = {k: p.grad.detach() for k, p in twin.named_parameters() if p.grad is not None}
    assert not set(g32) - set(g_h), (case.name, set(g32) - set(g_h))
    scale = max(v.abs().max().item() for v in g32.values())
    worst, notes, misses = (0.0, ''), [], []
    for k, r32 in g32.items():
        got, r64 = g_h[k].double(), g64[k]
        plain = (got - r32.double()).abs().max().item() / (1e-5 * r32.abs().max().item() + 2e-6 * scale)
        arb = (got - r64).abs().max().item() / ((r32.double() - r64).abs().max().item() + 1e-6 * scale)
        ratio = min(plain, arb)
        own = max(r64.abs().max().item(), 1e-300)
        d64 = (got - r64).abs().max().item()
        if case.edge_ref == 'lds' and is_edge(k):
            d_lds = (got - lds[k].double()).abs().max().item()
            margin = 2e-5 * lds[k].abs().max().item() + 4e-6 * scale
            notes.append((d64 / own, ratio, d_lds / margin, k))
        elif case.edge_ref == 'sentinel' and is_edge(k):
            notes.append((d64 / own, ratio, ((got - r64).abs() / (0.01 * r64.abs() + 2e-6 * scale)).max().item(), k))
        try:
            assert_grad_parity(g_h[k], r32, lambda k=k: g64[k], scale, '%s %s' % (case.name, k), rtol=1e-5, floor=2e-6, slack=1.0)
        except AssertionError as e:                  # (every tensor of the case is looked at before the case fails)
            if not (case.edge_ref and is_edge(k)):
                misses.append(str(e))
            elif case.edge_ref == 'lds':
                if d_lds > margin:
                    misses.append('%s misses the rule (distance / bound %.2f) and the bond-list run: %.3g > %.3g' % (k, ratio, d_lds, margin))
            else:
                bad = (got - r64).abs() > 0.01 * r64.abs() + 2e-6 * scale
                if bad.any():
                    misses.append('%s misses the rule (distance / bound %.2f) and the 1 %% sentinel: %s vs %s'
                                  % (k, ratio, got[bad][:4].tolist(), r64[bad][:4].tolist()))
            continue
        worst = max(worst, (ratio, k))
    assert not misses, (case.name, case.line(), misses)
    line = 'AGG_DISPATCH %s: %s | out %.1e stats %.1e | worst gradient distance / bound %.2f (%s)' % (
        case.name, case.line(), e_out, e_st, worst[0], worst[1])
    if notes:
        n = max(notes)
        what = 'to the bond-list run / margin' if case.edge_ref == 'lds' else 'largest entry error / 1 % sentinel'
        line += ' | edge parameters: to float64 / own max %.1e, / rule %.2f, %s %.2g (%s)' % (n[0], n[1], what, n[2], n[3])
    return line


def main(argv):
    save_dir = lds_dir = None
    if argv and argv[0] in ('--save-dir', '--lds-dir'):
        save_dir, lds_dir = (argv[1], None) if argv[0] == '--save-dir' else (None, argv[1])
        argv = argv[2:]
    assert os.environ.get('EAGCN_AGG') == ('lds' if save_dir else 'dense'), 'the parent sets EAGCN_AGG'
    failed = 0
    for name in argv:
        case = T.BY_NAME[name]
        lds = None
        if lds_dir is not None and case.edge_ref == 'lds':
            lds = torch.load(os.path.join(lds_dir, name + '.pt'))
        try:
            print(run_case(case, lds=lds, save=None if save_dir is None else os.path.join(save_dir, name + '.pt')), flush=True)
        except AssertionError as e:                  # the other cases of the child still run: one run shows every miss
            failed += 1
            print('AGG_DISPATCH_MISS %s: %s' % (name, e), flush=True)
    if failed:
        sys.exit('%d of %d cases failed' % (failed, len(argv)))
    print('AGG_DISPATCH_OK')


if __name__ == '__main__':
    main(sys.argv[1:])
