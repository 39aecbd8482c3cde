"""a-11 / f-3: the reference's training loop (train.py:289-334: Adam with weight decay on the weighted masked BCE / MSE) and
its evaluation (train.py:130-211) on the HIP engine in graph mode, tracked against the CPU oracle over 50 optimizer steps:
loss curve, parameters, BatchNorm running statistics, num_batches_tracked, validation AUC / RMSE.

Training is a chaotic map: the fp32 CPU oracle itself leaves the fp64 trajectory by 1e-4 .. 2e-2 within 50 Adam steps
(tests/probe_train_drift.py), so the yardstick is the fp64 oracle and the bar is the reference's own fp32 drift, STEP BY
STEP and TENSOR BY TENSOR: while the fp32 oracle's copy is within 1e-4 of the fp64 trajectory, the HIP copy may be at most
as far from it as the oracle is -- compared as distributions over the tensors (median x3, worst x10); after that Adam has amplified rounding noise and nothing is compared.
"The fp32 oracle" is four runs -- the oracle and three copies started one unit in the last place away -- and its drift the largest
of theirs: where the trajectory passes a relu kink a single run's side of it, and with it the bar, depended on the host CPU."""
import numpy as np
import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('optim', ['torch', 'flat'])
@pytest.mark.parametrize('task', ['class', 'reg'])
def test_fifty_adam_steps_track_the_oracle(task, optim):
    """optim='flat': the update is eagcn_amd.optim.FlatAdam -- one kernel over the flat parameter buffer, captured into the step
    graph -- against torch.optim.Adam on the oracle; same bars."""
    from sklearn import metrics
    from eagcn_amd import EAGCN, training
    from eagcn_amd.synthetic import make_batch
    from oracle.eagcn_ref import RefEAGCN, weights_init_
    T = 4 if task == 'class' else 1
    w1, w2 = [16, 12, 8, 8, 8], [24, 12, 12, 12, 12]
    torch.manual_seed(2)
    ref = RefEAGCN(9, 24, w1, w2, 32, 16, T, 0.0, n_layers=2)
    weights_init_(ref)
    hip = EAGCN(9, 24, *w1, *w2, 32, 16, T, 0.0, n_layers=2, graph=True).cuda().train()
    hip.load_state_dict(ref.state_dict(), strict=True)
    mbs = [make_batch(B=32, n_max=40, n_med=12, rel_channels=(9, 4, 2, 2, 2), seed=60 + i, n_tasks=T, task=task) for i in range(4)]
    cpu = [(mb.dense(), torch.from_numpy(mb.labels)) for mb in mbs]
    dev = [(tuple(t.cuda() for t in d), l.cuda()) for d, l in cpu]
    bw = training.set_weight(torch.cat([l for _, l in cpu]), T) if task == 'class' else None
    bw_dev = torch.tensor(bw, device='cuda') if bw else None
    ref64 = RefEAGCN(9, 24, w1, w2, 32, 16, T, 0.0, n_layers=2).double()
    ref64.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
    cpu64 = [([t.double() if t.is_floating_point() else t for t in d], l) for d, l in cpu]
    # The fp32 yardstick is an ENSEMBLE of oracle runs: the oracle as initialised, and copies whose initial parameters are moved
    # by at most one unit in the last place (seeded).  One fp32 run is one sample of where fp32 arithmetic leaves the fp64
    # trajectory: in the `class` case an activation sits on its relu kink around step 9, and which side a run takes is decided by
    # the last bit -- of four one-ulp copies, three leave the fp64 trajectory there (as the HIP run does) and one follows it until
    # step 26; the unperturbed oracle does the one or the other depending on the host CPU's kernels.  A bar taken from a
    # single run therefore depended on the machine the test ran on.
    def ulp_copy(seed):
        m = RefEAGCN(9, 24, w1, w2, 32, 16, T, 0.0, n_layers=2)
        g = torch.Generator().manual_seed(seed)
        m.load_state_dict({k: v * (1 + 2.0 ** -23 * torch.randint(-1, 2, v.shape, generator=g).float()) if v.is_floating_point() else v
                           for k, v in ref.state_dict().items()})
        return m
    refs = [ref] + [ulp_copy(seed) for seed in (1, 2, 3)]
    opt_rs = [torch.optim.Adam(m.parameters(), lr=5e-4, weight_decay=1e-4) for m in refs]
    opt_x = torch.optim.Adam(ref64.parameters(), lr=5e-4, weight_decay=1e-4)
    if optim == 'flat':
        from eagcn_amd.optim import FlatAdam
        opt_h = FlatAdam(hip, lr=5e-4, weight_decay=1e-4)
    else:
        opt_h = torch.optim.Adam(hip.parameters(), lr=5e-4, weight_decay=1e-4)

    def loss_of(out, l):
        if task == 'reg':
            return torch.nn.functional.mse_loss(out.view(-1), l.to(out.dtype).view(-1))
        w = torch.tensor(bw, dtype=out.dtype)
        wt = ((l == 1).to(out.dtype) * w[:, 0].view(1, -1) + (l == 0).to(out.dtype) * w[:, 1].view(1, -1)).view(-1)
        return torch.nn.functional.binary_cross_entropy_with_logits(out.view(-1), l.to(out.dtype).view(-1), weight=wt,
                                                                  reduction='sum') / ((l == 1).sum() + (l == 0).sum()).to(out.dtype)
    def noise_key(k):
        if k.endswith('num_batches_tracked') or k.endswith('batch_norm.weight') or k.endswith('batch_norm.bias'):
            return True                                # counters / the reference's unused parameters
        # a bias in front of a training-mode BatchNorm has an analytically ZERO gradient: what reaches Adam is rounding
        # noise, which Adam normalises to +-lr steps -- a random walk that no two arithmetics share (the bias itself is
        # cancelled by the BatchNorm; the per-view running_mean tracks mean + bias and walks with it, and bn_den1's running
        # mean is Graph_BN.bias . den1: the column means of a product of a zero-mean matrix)
        return k.endswith('graph_conv.bias') or k == 'Graph_BN.bias' or (k.endswith('running_mean') and 'block' in k) or \
            k == 'bn_den1.running_mean'

    def drifts(sd, sd_x):
        """distance of every compared tensor to the fp64 trajectory, relative to the tensor's own scale"""
        return {k: (sd[k].double().cpu() - v).abs().max().item() / max(v.abs().max().item(), 1e-3)
                for k, v in sd_x.items() if not noise_key(k)}

    # Trajectory parity, step by step and tensor by tensor: as long as EVERY fp32 oracle run's copy of a tensor stays within 1e-4
    # of the fp64 trajectory the comparison means something, and there the HIP run's copy must be as close to fp64 as the fp32
    # oracle's is (its drift = the largest of the runs'; three times it + 1e-5 of the tensor's scale: two fp32 arithmetics round
    # differently, and a one-element tensor such as self_r moves by whole multiples of Adam's step).  A tensor an oracle run has
    # lost (Adam turns rounding noise in a near-zero gradient into +-lr steps) is not compared any more from that step on
    # (the old bound admitted 22 % of a parameter's scale after 50 steps).
    loss_rs, loss_x, loss_h = [[] for _ in refs], [], []
    alive, window = None, {}
    pworst, worst_ratio, n_cmp = 0.0, 0.0, 0
    for step in range(50):
        for m, o, data, acc in [(m, o, cpu, acc) for m, o, acc in zip(refs, opt_rs, loss_rs)] + [(ref64, opt_x, cpu64, loss_x)]:
            d, l = data[step % 4]
            o.zero_grad()
            out, _, _ = m(*d)
            lo = loss_of(out, l)
            lo.backward()
            o.step()
            acc.append(float(lo.detach()))
        dd, ll = dev[step % 4]
        loss_h.append(float(training.train_step(hip, opt_h, dd, ll, task, bw_dev).detach()))
        if alive is None or alive:
            sd_x = ref64.state_dict()
            d_rs = [drifts(m.state_dict(), sd_x) for m in refs]
            d_r = {k: max(d[k] for d in d_rs) for k in d_rs[0]}
            if alive is None:
                alive = set(d_r)
            alive = {k for k in alive if d_r[k] < 1e-4}
            if alive:
                d_h = drifts(hip.state_dict(), sd_x)
                # two fp32 arithmetics leave the exact trajectory with different random constants: what is compared is the
                # DISTRIBUTION over the tensors the oracle still tracks -- the median HIP drift against the median oracle drift
                # (x3), the worst HIP drift against the worst oracle drift (x10) -- not tensor against tensor (a one-element
                # self_r or a two-channel att.weight moves by whole Adam steps on rounding noise)
                hs, rs = sorted(d_h[k] for k in alive), sorted(d_r[k] for k in alive)
                assert hs[len(hs) // 2] <= 3.0 * rs[len(rs) // 2] + 1e-6, (step, 'median', hs[len(hs) // 2], rs[len(rs) // 2])
                worst_k = max(alive, key=lambda k: d_h[k])
                assert hs[-1] <= 10.0 * rs[-1] + 1e-5, (step, worst_k, hs[-1], rs[-1])
                for k in alive:
                    window[k] = step + 1
                    n_cmp += 1
                pworst = max(pworst, hs[-1])
                worst_ratio = max(worst_ratio, hs[-1] / max(rs[-1], 1e-6))
                if len(alive) == len(d_r):             # the loss is compared while the oracle tracks EVERY tensor
                    dl_r, dl_h = max(abs(acc[-1] - loss_x[-1]) for acc in loss_rs), abs(loss_h[-1] - loss_x[-1])
                    assert dl_h <= 3.0 * dl_r + 1e-5 * max(abs(loss_x[-1]), 1.0), (step, loss_h[-1], loss_x[-1], dl_r)
    wl = sorted(window.values())
    print('trajectory parity [%s]: %d tensor-steps compared; per-tensor windows min %d / median %d / max %d of 50 steps; worst HIP '
          'drift %.1e, worst HIP/oracle drift ratio %.2f' % (task, n_cmp, wl[0], wl[len(wl) // 2], wl[-1], pworst, worst_ratio))
    assert len(wl) >= 70 and wl[len(wl) // 2] >= 5, wl        # the comparison is not vacuous
    rel_err(torch.tensor([pworst]), torch.tensor([0.0]), 'worst HIP distance to the fp64 trajectory over %d compared tensor-steps '
            '(median window %d steps)' % (n_cmp, wl[len(wl) // 2]))
    assert loss_x[-1] < loss_x[0] and loss_h[-1] < loss_h[0]                      # it trains
    if optim == 'flat':
        assert int(opt_h.step_count) == 50 and int(opt_h.ticket) == 0
        for n, p in hip.named_parameters():                                       # the parameters ARE the flat buffer
            if p.grad is not None:
                assert opt_h.flat.data_ptr() <= p.data_ptr() < opt_h.flat.data_ptr() + 4 * opt_h.flat.numel(), n
    for k, v in hip.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 50, k
    # evaluation (train.py:130-211): the oracle takes the HIP-trained weights, so that what is compared is the
    # evaluation path and not 50 steps of training drift (an AUC moves by 1/(pos*neg) per swapped pair)
    ref = ref64.float()
    ref.load_state_dict({k: v.detach().cpu() for k, v in hip.state_dict().items()})
    val = [make_batch(B=32, n_max=40, n_med=12, rel_channels=(9, 4, 2, 2, 2), seed=90 + i, n_tasks=T, task=task) for i in range(2)]
    got = training.evaluate(hip, [(tuple(t.cuda() for t in mb.dense()), torch.from_numpy(mb.labels).cuda()) for mb in val], task, T)
    ref.eval()
    with torch.no_grad():
        outs = torch.cat([ref(*mb.dense())[0] for mb in val])
    labels = torch.cat([torch.from_numpy(mb.labels) for mb in val])
    if task == 'class':
        probs = torch.sigmoid(outs).numpy()
        for j in range(T):
            m = (labels[:, j] != -1).numpy()
            fpr, tpr, _ = metrics.roc_curve(labels[:, j].numpy()[m].astype(int), probs[:, j][m], pos_label=1)
            assert abs(got[0][j] - metrics.auc(fpr, tpr)) < 2e-3, (j, got[0][j])
    else:
        want = float(np.sqrt(metrics.mean_squared_error(outs.numpy().ravel(), labels.numpy().ravel())))
        assert abs(got - want) < 1e-3 * max(want, 1.0), (got, want)
    assert hip.training


@pytest.mark.parametrize('wd', [0.0, 1e-4])
def test_flat_adam_kernel_matches_torch_adam(wd):
    """eagcn_adam_step on its own: the same gradients fed to FlatAdam and to torch.optim.Adam (train.py:303), 20 steps; the two are
    the same fp32 arithmetic up to the order of two multiplications (a few ulp per step)."""
    from eagcn_amd import EAGCN
    from eagcn_amd.optim import FlatAdam
    w1, w2 = [16, 12, 8, 8, 8], [24, 12, 12, 12, 12]
    torch.manual_seed(5)
    a = EAGCN(9, 24, *w1, *w2, 32, 16, 3, 0.0, n_layers=2).cuda()
    b = EAGCN(9, 24, *w1, *w2, 32, 16, 3, 0.0, n_layers=2).cuda()
    b.load_state_dict(a.state_dict())
    plan_a, plan_b = a.plan(), b.plan()
    opt_a = FlatAdam(a, lr=1e-3, weight_decay=wd)
    live_b = [p for p in plan_b.params if p.requires_grad]
    opt_b = torch.optim.Adam(live_b, lr=1e-3, weight_decay=wd)
    g = torch.Generator(device='cuda').manual_seed(1)
    for step in range(20):
        if step == 10:
            opt_a.set_lr(3e-4)
            opt_b.param_groups[0]['lr'] = 3e-4
        for pa, pb in zip(plan_a.params, plan_b.params):
            if not pa.requires_grad:
                continue
            gr = torch.randn(pa.shape, device='cuda', generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,))))
            pa.grad, pb.grad = gr.clone(), gr.clone()
        opt_a.step()
        opt_b.step()
    worst = 0.0
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        worst = max(worst, (pa - pb).abs().max().item() / max(pb.abs().max().item(), 1e-3))
    print('FlatAdam vs torch.optim.Adam after 20 steps (wd=%g): worst |dp| / max|p| = %.2e' % (wd, worst))
    assert worst < 2e-6, worst
    st = opt_b.state[live_b[0]]
    i0 = next(i for i, p in enumerate(plan_a.params) if p.requires_grad)
    m0 = plan_a.grad_views(opt_a.exp_avg)[i0]
    assert torch.allclose(m0, st['exp_avg'], rtol=1e-5, atol=1e-12)
    assert int(opt_a.step_count) == 20


def test_flat_adam_skips_parameters_without_gradient_and_notices_rehomed_parameters():
    """torch.optim.Adam skips a parameter whose .grad is None -- no weight decay, no moment update (FlatAdam zero-filled
    such slots and decayed them); and a parameter whose .data was re-assigned after the optimizer was built no longer lives in the
    flat buffer: the step must refuse instead of updating memory nobody reads."""
    from eagcn_amd import EAGCN, _lib as L
    from eagcn_amd.optim import FlatAdam
    w1, w2 = [16, 12, 8, 8, 8], [24, 12, 12, 12, 12]
    torch.manual_seed(5)
    a = EAGCN(9, 24, *w1, *w2, 32, 16, 3, 0.0, n_layers=2).cuda()
    b = EAGCN(9, 24, *w1, *w2, 32, 16, 3, 0.0, n_layers=2).cuda()
    b.load_state_dict(a.state_dict())
    plan_a, plan_b = a.plan(), b.plan()
    opt_a = FlatAdam(a, lr=1e-2, weight_decay=1e-2)
    live_b = [p for p in plan_b.params if p.requires_grad]
    opt_b = torch.optim.Adam(live_b, lr=1e-2, weight_decay=1e-2)
    g = torch.Generator(device='cuda').manual_seed(1)
    before = [p.detach().clone() for p in plan_a.params]
    for step in range(3):
        for i, (pa, pb) in enumerate(zip(plan_a.params, plan_b.params)):
            pa.grad = pb.grad = None
            if pa.requires_grad and i % 3 != 1:               # every third parameter never receives a gradient
                gr = torch.randn(pa.shape, device='cuda', generator=g)
                pa.grad, pb.grad = gr.clone(), gr.clone()
        opt_a.step()
        opt_b.step()
    assert int(opt_a.step_count) == 3
    for i, (pa, pb, p0) in enumerate(zip(plan_a.params, plan_b.params, before)):
        if not pa.requires_grad:
            continue
        if i % 3 == 1:
            assert torch.equal(pa.detach(), p0), 'parameter %d has no gradient and must not move (weight decay 1e-2)' % i
        else:
            assert (pa - pb).abs().max().item() <= 2e-6 * max(pb.abs().max().item(), 1e-3), i
    victim = next(p for p in plan_a.params if p.requires_grad)
    victim.data = victim.data.clone()
    with pytest.raises(L.EagcnHipError):
        opt_a.step()
