"""Gradient-norm clipping and non-finite step skipping of FlatAdam (csrc/clip.hip: eagcn_grad_norm + eagcn_adam_step_clipped) against
float64 sums and against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.

Bounds.  The norm: squares of fp32 values are exact in fp64, a sum of n <= 4 M non-negative fp64 terms in any order is within
n 2^-53 < 1e-10 relative of the exact one (and torch's own float64 sum, the reference, likewise).  The update: the bound of
test_flat_adam_kernel_matches_torch_adam (worst |dp| / max|p| < 2e-6 after 20 steps): clipping adds one fp32 multiply per gradient
and a coefficient that torch forms from an fp32 norm (1e-7 relative).  Should the update exceed that bound, the same gradients go
through a float64 torch chain and FlatAdam may be at most 1.5 x as far from it as the fp32 torch chain is."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

W1, W2 = [16, 12, 8, 8, 8], [24, 12, 12, 12, 12]
BOUND = 2e-6
NORM_REL = 1e-10


def _small(**kw):
    from eagcn_amd import EAGCN
    return EAGCN(9, 24, *W1, *W2, 32, 16, 3, 0.0, n_layers=2, **kw).cuda()


def _live_mask(plan):
    """True for the elements of parameters that take gradients; False for pad words and the slots of frozen parameters."""
    mask = torch.zeros(plan.offsets[-1], dtype=torch.bool)
    for p, o, k in zip(plan.params, plan.offsets, plan.sizes):
        if p.requires_grad:
            mask[o:o + k] = True
    return mask.cuda()


def _lanes(mask):
    return mask.view(-1, 4).sum(1).to(torch.uint8)        # (pads sit BEHIND a parameter: the live floats of a group lead it)


def _workspace():
    from eagcn_amd import _lib as L
    return torch.zeros(int(L.load().eagcn_grad_norm_workspace_bytes()) // 8, dtype=torch.int64, device='cuda')


def _norm_launch(g, lanes, ws, off=0, n=None, accumulate=False):
    """-> the workspace's first two words as int64 bits: [sumsq (a double's bits), n_bad]"""
    from eagcn_amd import _lib as L
    n = g.numel() - off if n is None else n
    L.check(L.load().eagcn_grad_norm(C.c_void_p(g.data_ptr() + 4 * off), C.c_void_p(lanes.data_ptr() + off // 4) if lanes is not None else None,
                                     n, C.c_void_p(ws.data_ptr()), 1 if accumulate else 0,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'eagcn_grad_norm')
    return ws[:2].cpu()


def _sumsq(h):
    return float(h[:1].view(torch.float64)[0])


def _ref_sumsq(g, mask):
    return float((g.double()[mask] ** 2).sum())


@pytest.mark.parametrize('layout', [4, 1020, 1048580, 'model'])
def test_norm_launch_against_float64(layout):
    """4 floats (one thread), 1020 (one workgroup, a partial last wave), 1 048 580 (one group of four past 1024 x 256: the grid cap
    and a second trip of the grid-stride loop), the small model's layout (pads behind 1-element parameters, a lane table)."""
    gen = torch.Generator(device='cuda').manual_seed(3)
    if layout == 'model':
        mask = _live_mask(_small().plan())
        lanes = _lanes(mask)
        assert int((~mask).sum()) > 0
    else:
        mask, lanes = torch.ones(layout, dtype=torch.bool, device='cuda'), None
    n = mask.numel()
    g = torch.randn(n, device='cuda', generator=gen) * 10.0 ** torch.randint(-6, 1, (n,), device='cuda', generator=gen).float()
    g[~mask] = float('nan')                                # dead words hold anything
    ws = _workspace()
    h1 = _norm_launch(g, lanes, ws)
    ref = _ref_sumsq(g, mask)
    print('norm launch [%s]: sumsq %.17g, float64 reference %.17g, relative error %.2e' % (layout, _sumsq(h1), ref, abs(_sumsq(h1) - ref) / ref))
    assert abs(_sumsq(h1) - ref) <= NORM_REL * ref and int(h1[1]) == 0
    assert int(ws[2]) == 0                                 # the ticket is back at 0
    # bit-reproducible: the same workspace again, and a fresh one
    assert torch.equal(_norm_launch(g, lanes, ws), h1)
    assert torch.equal(_norm_launch(g, lanes, _workspace()), h1)
    # two accumulating launches over two halves (n = 4: an empty first half, which must still replace the stored totals)
    half = (n // 8) * 4
    _norm_launch(g, lanes, ws, 0, half, accumulate=False)
    h2 = _norm_launch(g, lanes, ws, half, n - half, accumulate=True)
    assert abs(_sumsq(h2) - ref) <= NORM_REL * ref and int(h2[1]) == 0
    # 1e25: the squares overflow fp32, not fp64
    big = torch.where(mask, torch.full_like(g, 1e25), g)
    hb = _norm_launch(big, lanes, ws)
    refb = _ref_sumsq(big, mask)
    assert math.isfinite(_sumsq(hb)) and abs(_sumsq(hb) - refb) <= NORM_REL * refb and int(hb[1]) == 0
    assert abs(math.sqrt(_sumsq(hb)) - 1e25 * math.sqrt(int(mask.sum()))) <= 1e-6 * 1e25 * math.sqrt(int(mask.sum()))
    # one NaN and one Inf among the live elements
    idx = mask.nonzero().view(-1)
    bad = g.clone()
    bad[idx[0]] = float('nan')
    if idx.numel() > 1:
        bad[idx[-1]] = float('-inf')
    hn = _norm_launch(bad, lanes, ws)
    assert int(hn[1]) == min(2, idx.numel()) and not math.isfinite(_sumsq(hn))


@pytest.mark.parametrize('structure', ['Concate', 'GCN'])
def test_pad_words_and_frozen_slots_stay_out_of_the_norm(structure):
    """Widths that leave pad words; a frozen parameter (Concate: frozen by hand, GCN: the constant attention weights).  Pads and frozen
    slots of the gradient hold NaN and 1e30: the step must not be skipped and last_norm is the float64 norm over parameter elements."""
    from eagcn_amd import EAGCN
    from eagcn_amd.optim import FlatAdam
    torch.manual_seed(4)
    m = EAGCN(9, 24, 8, 6, 4, 4, 5, 10, 7, 5, 6, 4, 32, 16, 3, 0.0, structure=structure, n_layers=2).cuda()
    plan = m.plan()
    if structure == 'Concate':
        plan.params[2].requires_grad_(False)
    assert plan.offsets[-1] > sum(plan.sizes) and any(not p.requires_grad for p in plan.params)
    opt = FlatAdam(m, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    mask = _live_mask(plan)
    assert torch.equal(opt.lanes, _lanes(mask))
    gen = torch.Generator(device='cuda').manual_seed(9)
    flat = torch.randn(mask.numel(), device='cuda', generator=gen)
    dead = (~mask).nonzero().view(-1)
    flat[dead[0::2]] = float('nan')
    flat[dead[1::2]] = 1e30
    before = opt.flat.clone()
    opt.launch(flat)
    st = opt.clip_stats()
    ref = math.sqrt(_ref_sumsq(flat, mask))
    assert st['skipped'] == 0 and st['applied'] == 1 and st['clipped'] == 1, st
    assert abs(st['last_norm'] - ref) <= NORM_REL * ref, (st['last_norm'], ref)
    assert int(opt.step_count) == 1 and int(opt.ticket) == 0
    assert bool(torch.isfinite(opt.flat[mask]).all()) and not torch.equal(opt.flat[mask], before[mask])


def _grads(plan, steps, keep=lambda step, i: True):
    """The gradients of test_flat_adam_kernel_matches_torch_adam: normal, a random decade 1e-6 .. 1 per tensor; None for frozen
    parameters and where `keep` says so."""
    torch.manual_seed(11)
    gen = torch.Generator(device='cuda').manual_seed(1)
    return [[torch.randn(p.shape, device='cuda', generator=gen) * (10.0 ** float(torch.randint(-6, 1, (1,))))
             if p.requires_grad and keep(step, i) else None for i, p in enumerate(plan.params)] for step in range(steps)]


def _norm64(gs):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs if g is not None))


def _twin(params0, grads, c, wd, dtype, lr, lr_at_10=None):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam over copies of the parameters, in `dtype`."""
    ps = [p.detach().clone().to(dtype).requires_grad_(True) for p in params0]
    opt = torch.optim.Adam(ps, lr=lr, weight_decay=wd)
    clipped = 0
    for step, gs in enumerate(grads):
        if step == 10 and lr_at_10 is not None:
            opt.param_groups[0]['lr'] = lr_at_10
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(dtype).clone()
        if c is not None:
            total = torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], c)
            clipped += int(float(total) > c)
        opt.step()
    return [p.detach() for p in ps], clipped


def _distance(ps, qs):
    return max((p.double() - q.double()).abs().max().item() / max(q.abs().max().item(), 1e-3) for p, q in zip(ps, qs))


def _flat_run(model, opt, grads, lr_at_10=None):
    plan = model.plan()
    for step, gs in enumerate(grads):
        if step == 10 and lr_at_10 is not None:
            opt.set_lr(lr_at_10)
        for p, g in zip(plan.params, gs):
            p.grad = None if g is None else g.clone()
        opt.step()


def _assert_parity(what, mine, t32, params0, grads, c, wd, lr, lr_at_10=None):
    d = _distance(mine, t32)
    t64, _ = _twin(params0, grads, c, wd, torch.float64, lr, lr_at_10)
    d_mine, d_t32 = _distance(mine, t64), _distance(t32, t64)
    print('%s: worst |dp| / max|p| FlatAdam vs fp32 torch %.2e; to the float64 chain: FlatAdam %.2e, fp32 torch %.2e' % (what, d, d_mine, d_t32))
    assert d < BOUND or d_mine <= 1.5 * d_t32, (d, d_mine, d_t32)


@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_clipped_steps_match_clip_grad_norm_and_torch_adam(wd):
    """The 20-step protocol of test_flat_adam_kernel_matches_torch_adam (lr change at step 10) with max_grad_norm = half the float64
    norm of the first step's gradients."""
    from eagcn_amd.optim import FlatAdam
    torch.manual_seed(5)
    a = _small()
    plan = a.plan()
    live = [i for i, p in enumerate(plan.params) if p.requires_grad]
    params0 = [plan.params[i].detach().clone() for i in live]
    grads = _grads(plan, 20)
    glive = [[gs[i] for i in live] for gs in grads]
    c = 0.5 * _norm64(glive[0])
    opt = FlatAdam(a, lr=1e-3, weight_decay=wd, max_grad_norm=c)
    _flat_run(a, opt, grads, 3e-4)
    st = opt.clip_stats()
    t32, n_clipped = _twin(params0, glive, c, wd, torch.float32, 1e-3, 3e-4)
    assert st['applied'] == 20 and st['skipped'] == 0 and st['clipped'] >= 1 and st['clipped'] == n_clipped, (st, n_clipped)
    assert int(opt.step_count) == 20 and int(opt.ticket) == 0
    ref = _norm64(glive[-1])
    assert abs(st['last_norm'] - ref) <= NORM_REL * ref
    for p, g in zip(plan.params, grads[-1]):              # the gradients themselves are only read
        assert g is None or torch.equal(p.grad, g)
    _assert_parity('clipped, wd=%g' % wd, [plan.params[i].detach() for i in live], t32, params0, glive, c, wd, 1e-3, 3e-4)


@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_infinite_bound_is_bit_identical_to_the_plain_step(wd):
    """max_grad_norm = inf measures and never clips: parameters, both moments and the step count equal a plain FlatAdam's bit for bit,
    over the 20 range-by-range steps of the protocol and three whole-buffer launches."""
    from eagcn_amd.optim import FlatAdam
    torch.manual_seed(5)
    a, b = _small(), _small()
    b.load_state_dict(a.state_dict())
    opt_a = FlatAdam(a, lr=1e-3, weight_decay=wd, max_grad_norm=float('inf'))
    opt_b = FlatAdam(b, lr=1e-3, weight_decay=wd)
    assert not opt_b.clipping and not hasattr(opt_b, 'norm_ws')
    grads = _grads(a.plan(), 20)
    _flat_run(a, opt_a, grads, 3e-4)
    _flat_run(b, opt_b, grads, 3e-4)
    gen = torch.Generator(device='cuda').manual_seed(2)
    for _ in range(3):
        flat = torch.randn(opt_a.flat.numel(), device='cuda', generator=gen) * 1e-2
        opt_a.launch(flat)
        opt_b.launch(flat)
    for name in ('flat', 'exp_avg', 'exp_avg_sq', 'step_count'):
        assert torch.equal(getattr(opt_a, name), getattr(opt_b, name)), name
    st = opt_a.clip_stats()
    assert int(opt_a.step_count) == 23 and st['applied'] == 23 and st['clipped'] == 0 and st['skipped'] == 0, st


def test_nonfinite_gradient_skips_the_step_or_propagates():
    from eagcn_amd import _lib as L
    from eagcn_amd.optim import FlatAdam
    torch.manual_seed(5)
    a, b, c = _small(), _small(), _small()
    b.load_state_dict(a.state_dict())
    c.load_state_dict(a.state_dict())
    opt_a = FlatAdam(a, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    opt_b = FlatAdam(b, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0, skip_nonfinite=True)      # never sees the bad gradient
    mask = _live_mask(a.plan())
    gen = torch.Generator(device='cuda').manual_seed(6)
    g1, g2 = (torch.randn(mask.numel(), device='cuda', generator=gen) for _ in range(2))
    bad = g2.clone()
    bad[mask.nonzero().view(-1)[5]] = float('nan')
    opt_a.launch(g1)
    snap = {k: getattr(opt_a, k).clone() for k in ('flat', 'exp_avg', 'exp_avg_sq', 'step_count')}
    opt_a.launch(bad)
    for k, v in snap.items():
        assert torch.equal(getattr(opt_a, k), v), k
    st = opt_a.clip_stats()
    assert st['skipped'] == 1 and st['applied'] == 1 and math.isnan(st['last_norm']) and int(opt_a.ticket) == 0, st
    opt_a.launch(g2)                                       # a clean gradient: the step the skipped one would have been
    opt_b.launch(g1)
    opt_b.launch(g2)
    assert int(opt_a.step_count) == 2 and not torch.equal(opt_a.flat, snap['flat'])
    for k in snap:
        assert torch.equal(getattr(opt_a, k), getattr(opt_b, k)), k
    assert opt_a.clip_stats()['applied'] == 2
    # skipping off: the NaN propagates, as with clip_grad_norm_(error_if_nonfinite=False) (a NaN coefficient scales every gradient)
    opt_c = FlatAdam(c, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    opt_c.launch(bad)
    assert bool(torch.isnan(opt_c.flat[mask]).all()) and int(opt_c.step_count) == 1
    assert opt_c.clip_stats()['skipped'] == 0
    # the settings of a live optimizer: the bound is a device write, switching the feature on or off is refused
    opt_a.set_max_grad_norm(2.5)
    assert float(opt_a.clip[0]) == 2.5
    sd = opt_a.state_dict()
    assert sd['max_grad_norm'] == 2.5 and sd['skip_nonfinite'] is True and (sd['applied'], sd['skipped'], sd['clipped']) == (2, 1, 2)
    assert {'exp_avg', 'exp_avg_sq', 'step', 'hyper', 'param_group'} <= set(sd)
    plain = FlatAdam(_small(), lr=1e-3)
    for call in (lambda: plain.set_max_grad_norm(1.0), lambda: opt_a.set_max_grad_norm(None), lambda: plain.clip_stats(),
                 lambda: plain.load_state_dict(sd)):
        with pytest.raises(L.EagcnHipError):
            call()
    old = {k: v for k, v in sd.items() if k not in ('max_grad_norm', 'skip_nonfinite', 'applied', 'skipped', 'clipped')}
    opt_b.load_state_dict(old)                             # a state without the new keys leaves the constructor's settings
    assert opt_b.max_grad_norm == 1.0 and opt_b.skip_nonfinite and float(opt_b.clip[0]) == 1.0
    opt_b.load_state_dict(sd)
    assert opt_b.max_grad_norm == 2.5 and float(opt_b.clip[0]) == 2.5 and opt_b.clip_stats()['skipped'] == 1


def test_autograd_mode_takes_one_norm_over_the_live_ranges():
    """Step 0 gives every parameter a gradient, steps 1 .. 3 leave out every third one (their staging slots then hold step 0's values):
    the norm covers the parameters that have a gradient, the others do not move, the rest matches the torch twin."""
    from eagcn_amd.optim import FlatAdam
    torch.manual_seed(5)
    a = _small()
    plan = a.plan()
    live = [i for i, p in enumerate(plan.params) if p.requires_grad]
    params0 = [plan.params[i].detach().clone() for i in live]
    grads = _grads(plan, 4, keep=lambda step, i: step == 0 or i % 3 != 1)
    glive = [[gs[i] for i in live] for gs in grads]
    c = 0.5 * _norm64(glive[0])
    opt = FlatAdam(a, lr=1e-2, weight_decay=1e-2, max_grad_norm=c)
    _flat_run(a, opt, grads[:1])
    after0 = [p.detach().clone() for p in plan.params]
    _flat_run(a, opt, grads[1:])
    st = opt.clip_stats()
    ref = _norm64(glive[-1])
    assert st['applied'] == 4 and st['clipped'] >= 1 and int(opt.step_count) == 4, st
    assert abs(st['last_norm'] - ref) <= NORM_REL * ref, (st['last_norm'], ref, _norm64(glive[0]))
    for i in live:
        if i % 3 == 1:
            assert torch.equal(plan.params[i].detach(), after0[i]), 'parameter %d has no gradient and must not move' % i
    t32, n_clipped = _twin(params0, glive, c, 1e-2, torch.float32, 1e-2)
    assert st['clipped'] == n_clipped
    _assert_parity('autograd mode', [plan.params[i].detach() for i in live], t32, params0, glive, c, 1e-2, 1e-2)


def test_clipping_and_skipping_inside_the_step_graph():
    """training.train_step on a graph=True model: the two launches are captured behind the backward.  The twin is a graph-mode copy
    stepped with fused_step (no optimizer), clip_grad_norm_ and torch.optim.Adam.

    lr = 1e-5.  Here the gradients come from the model, so the two runs feed back into their own inputs, and Graph_BN.bias (in front of
    a training-mode BatchNorm: an analytically zero gradient, rounding noise that Adam normalises to +-lr steps) walks differently in
    any two fp32 runs: at lr = 1e-3 two TORCH twins started one unit in the last place apart end 4.7e-1 of that bias's scale apart after
    these 6 steps (FlatAdam and the twin: 2.2e-1), at 1e-4 8.0e-2 (8.7e-2), and the gradient norm drops below half its first value
    within two steps at 1e-3, so that only 2 of 6 steps clip.  At 1e-5 the norm stays within 6 % of its first value, every step clips,
    and FlatAdam ends 1.0e-7 from the twin.  At this lr the parameters alone say little about the coefficient (Adam's step hardly
    depends on the gradient's scale), so the first moments, which are linear in the clipped gradient, are compared as well."""
    from eagcn_amd import training
    from eagcn_amd.optim import FlatAdam
    from eagcn_amd.synthetic import make_batch
    torch.manual_seed(7)
    hip, twin = _small(graph=True).train(), _small(graph=True).train()
    twin.load_state_dict(hip.state_dict())
    mb = make_batch(B=8, n_max=12, rel_channels=(9, 4, 2, 2, 2), seed=70, n_tasks=3, task='reg')
    batch = tuple(t.cuda() for t in mb.dense())
    labels = torch.from_numpy(mb.labels).cuda()
    live_t = [p for p in twin.plan().params if p.requires_grad]
    live_h = [p for p in hip.plan().params if p.requires_grad]
    opt_t = torch.optim.Adam(live_t, lr=1e-5, weight_decay=1e-4)
    opt_h, c, n_clipped = None, None, 0
    for step in range(6):
        opt_t.zero_grad(set_to_none=True)
        twin.fused_step(batch, labels, 'reg')
        with_grad = [p for p in live_t if p.grad is not None]
        if step == 0:
            c = 0.5 * _norm64([p.grad for p in with_grad])
            opt_h = FlatAdam(hip, lr=1e-5, weight_decay=1e-4, max_grad_norm=c, skip_nonfinite=True)
        n_clipped += int(float(torch.nn.utils.clip_grad_norm_(with_grad, c)) > c)
        opt_t.step()
        training.train_step(hip, opt_h, batch, labels, 'reg')
    st = opt_h.clip_stats()
    d = _distance([p.detach() for p in live_h], [p.detach() for p in live_t])
    print('step graph, 6 clipped steps: worst |dp| / max|p| vs the torch twin %.2e; stats %r, twin clipped %d' % (d, st, n_clipped))
    assert st['applied'] == 6 and st['clipped'] == 6 and st['skipped'] == 0 and n_clipped == 6, (st, n_clipped)
    assert int(opt_h.step_count) == 6
    assert d < BOUND, d
    m_h = [v for v, p in zip(hip.plan().grad_views(opt_h.exp_avg), hip.plan().params) if p.requires_grad]
    m_t = [opt_t.state[p]['exp_avg'] if p in opt_t.state else torch.zeros_like(p) for p in live_t]
    scale = max(m.abs().max().item() for m in m_t)
    dm = max((a - b).abs().max().item() for a, b in zip(m_h, m_t)) / scale
    print('step graph: worst |d exp_avg| / max|exp_avg| vs the twin %.2e' % dm)
    assert dm < 1e-5, dm                                  # (the existing test's rtol for a moment; an unclipped step would be 5e-1 off)
    # a NaN label: the MSE gradient is NaN everywhere; parameters and moments keep their bits
    snap = {k: getattr(opt_h, k).clone() for k in ('flat', 'exp_avg', 'exp_avg_sq', 'step_count')}
    poisoned = labels.clone()
    poisoned[0, 0] = float('nan')
    training.train_step(hip, opt_h, batch, poisoned, 'reg')
    for k, v in snap.items():
        assert torch.equal(getattr(opt_h, k), v), k
    assert opt_h.clip_stats()['skipped'] == 1
    training.train_step(hip, opt_h, batch, labels, 'reg')   # a clean replay moves them again
    st = opt_h.clip_stats()
    assert not torch.equal(opt_h.flat, snap['flat']) and int(opt_h.step_count) == 7 and st['applied'] == 7 and st['clipped'] == 7, st
    # the bound is read at every replay: no re-capture
    opt_h.set_max_grad_norm(1e30)
    training.train_step(hip, opt_h, batch, labels, 'reg')
    assert opt_h.clip_stats()['clipped'] == 7
    opt_h.set_max_grad_norm(c)
    training.train_step(hip, opt_h, batch, labels, 'reg')
    st = opt_h.clip_stats()
    assert st['clipped'] == 8 and st['applied'] == 9 and st['skipped'] == 1 and math.isfinite(st['last_norm']), st
