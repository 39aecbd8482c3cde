"""Time of the bond-gradient launch (csrc/battr.hip, eagcn_layer_bond_grad) per layer and of a whole EAGCN.bond_attributions call at the
Tox21 shape (B = 256, N = 132, 2 layers, widths 80 / 140), Concate and Weighted_sum.

    python tools/bond_attr_bench.py [--B 256] [--N 132] [--iters 200] [--warmup 20] [--group 10] [--out profiles/bond_attr_timing.txt]

A sample of the launch is a group of `group` launches between two HIP events on the stream (one launch is a few microseconds: the
events' own cost would dominate a single one), reported per launch as median with p10 .. p90 over `iters` samples; a sample of
the whole call is one call (index build, layer-by-layer forward, autograd to every layer output, the launches, finalize) ending in
a synchronise.  The yardstick is the transposed aggregation with edge gradients of the same layer in a training backward
(`lagg_kernel<true, ...>`: 25 - 31 us per launch at this shape in profiles/r05_sq_counters.txt / r06_sq_counters.txt), which gathers
the same P rows once.  Needs the GPU; inputs come from a seed."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAGG_US = 25.0            # lagg_kernel<true, ...> per launch at this shape (profiles/)
W1, W2 = [30, 10, 10, 10, 20], [60, 20, 20, 20, 20]


def stats(ts):
    a = np.sort(np.array(ts))
    return float(np.median(a)), float(a[len(a) // 10]), float(a[(9 * len(a)) // 10])


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if reps > 1:
        # the host needs longer to enqueue a launch than the GPU to run it: a spin kernel in front lets the group queue up, so that
        # the events bracket back-to-back launches and not the host's enqueue rate
        torch.cuda._sleep(4000000)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps       # us per repetition


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=256)
    ap.add_argument('--N', type=int, default=132)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--group', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bond_attr_bench needs the GPU (no timing without one)')
    from eagcn_amd import EAGCN, ops
    from eagcn_amd._lib import structure_code
    from eagcn_amd.synthetic import make_batch
    mb = make_batch(B=args.B, n_max=args.N, n_med=16, seed=1234)
    adj, afm, *rels, size = [t.cuda() for t in mb.dense()]
    lines = ['bond attribution timing, B = %d, N = %d, %d directed bonds, 2 layers, widths %d / %d'
             % (args.B, args.N, len(mb.edges), sum(W1), sum(W2)),
             'yardstick: lagg_kernel<true, ...> (transposed aggregation with edge gradients) ~ %.0f us per launch (profiles/)' % LAGG_US]
    for structure in ('Concate', 'Weighted_sum'):
        torch.manual_seed(1)
        model = EAGCN(28, 24, widths1=W1, widths2=W2, n_den1=256, n_den2=64, nclass=12, dropout=0.0, structure=structure,
                      n_layers=2).cuda().eval()
        index = ops.BatchIndex(adj, rels, bond_lists=True, structure=structure_code(structure))
        with torch.enable_grad():
            outs = model.forward_layers(index, afm.clone().requires_grad_(True))
            x, pad_row, layout = outs[-1]
            g = ops.readout(index, layout, x, pad_row if structure == 'Weighted_sum' else None, 'sum', size)
            out, _ = model.head_forward(g)
            xouts = [o[0] for o in outs]
            nodes = [(xo.grad_fn.spec, xo.grad_fn.buffers, xo.grad_fn.saved_tensors) for xo in xouts]
            douts = torch.autograd.grad(out[:, 0].sum(), xouts)
        acc = torch.zeros((index.K, index.E), dtype=torch.float32, device='cuda')
        lines.append('%s: %d packed rows' % (structure, index.rows))
        for l, ((spec, buffers, saved), dx) in enumerate(zip(nodes, douts)):
            for mode in ('attention', 'relation'):
                fn = lambda: ops.layer_bond_grad(index, spec, buffers, saved, dx, mode, acc, 1.0, first=True)
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                med, lo, hi = stats([timed(fn, args.group) for _ in range(args.iters)])
                lines.append('  layer %d (%4d packed columns) %-9s  %7.2f us per launch  (p10 %.2f .. p90 %.2f)  = %.2f x lagg_kernel<true>'
                             % (l, spec.fp, mode, med, lo, hi, med / LAGG_US))
        fin = lambda: ops.bond_attr_finalize(index, acc, False)
        for _ in range(args.warmup):
            fin()
        torch.cuda.synchronize()
        med, lo, hi = stats([timed(fin, args.group) for _ in range(args.iters)])
        lines.append('  finalize (with its four output allocations)  %7.2f us  (p10 %.2f .. p90 %.2f)' % (med, lo, hi))

        def whole():
            model.bond_attributions(adj, afm, *rels, size=size, target=0)
            torch.cuda.synchronize()
        for _ in range(5):
            whole()
        med, lo, hi = stats([timed(whole) for _ in range(max(20, args.iters // 10))])
        lines.append('  whole bond_attributions call              %9.1f us  (p10 %.1f .. p90 %.1f)' % (med, lo, hi))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
