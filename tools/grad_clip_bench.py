"""Cost of gradient clipping / non-finite skipping in the training iteration: the Tox21 C2 step (bench.py's tox21_c2 workload, batch 256,
forward + loss + backward + FlatAdam as ONE captured graph) with the optimizer built plain and built with max_grad_norm / skip_nonfinite
(one more launch, the norm, and the clipped update in place of the plain one).  Needs the GPU: there is nothing to time without one.

    python tools/grad_clip_bench.py [--tree OTHER_CHECKOUT] [--rounds 3] [--blocks 10] [--steps 50] [--warmup 20] [--out profiles/grad_clip_speed.txt]

Every configuration is timed in a fresh child process (its own graph capture), the configurations alternate over `--rounds` rounds so
that drift of a shared machine hits all of them alike; a block of `--steps` replays is bracketed by two device events.  `--tree` adds
the plain optimizer of another checkout of this project (built there already), e.g. the parent commit: "clipping off" must lie within
the run-to-run spread of that."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, args.child_tree)
    os.chdir(args.child_tree)
    import torch
    if not torch.cuda.is_available():
        sys.exit('grad_clip_bench: needs the GPU')
    import bench
    from eagcn_amd.optim import FlatAdam
    from eagcn_amd.synthetic import bce_weights, make_batch
    dev = torch.device('cuda')
    cfg = dict(bench.WORKLOADS['tox21_c2'])
    torch.manual_seed(1234)
    mb = make_batch(B=256, n_max=cfg['n_max'], n_med=cfg['n_med'], rel_channels=bench.rel_channels(cfg), seed=1234,
                    n_tasks=cfg['nclass'], task=cfg['task'], all_full=cfg.get('all_full', False))
    dense, labels = mb.dense(dev), torch.from_numpy(mb.labels).to(dev)
    bce_w = torch.tensor(bce_weights(cfg['nclass']), dtype=torch.float32, device=dev)
    model = bench.build_model(cfg, 0.3, dev, graph=True)
    model.train()
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if args.child_clip == 'on' else {}
    opt = FlatAdam(model, lr=1e-4, weight_decay=1e-4, **kw)
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        return model.fused_step(dense, labels, cfg['task'], bce_w, None, optimizer=opt)[0]

    for _ in range(4 + args.warmup):
        step()
    ms = []
    for _ in range(args.blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            loss = step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / args.steps)
    out = {'ms': ms, 'loss': float(loss), 'steps': int(opt.step_count), 'floats': int(opt.flat.numel())}
    if kw:
        out['clip_stats'] = opt.clip_stats()
    print('RESULT ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=None, help='another checkout of the project (built), timed with its plain FlatAdam')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--blocks', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child-tree', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-clip', default='off', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_tree:
        return child(args)
    configs = [('this tree, clipping off', HERE, 'off'), ('this tree, clipping on', HERE, 'on')]
    if args.tree:
        configs.insert(0, ('other tree (%s), plain' % os.path.basename(os.path.abspath(args.tree)), os.path.abspath(args.tree), 'off'))
    times = {c[0]: [] for c in configs}
    notes = {}
    for r in range(args.rounds):
        for label, tree, clip in configs:
            cmd = [sys.executable, os.path.abspath(__file__), '--child-tree', tree, '--child-clip', clip, '--blocks', str(args.blocks),
                   '--steps', str(args.steps), '--warmup', str(args.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            res = [l for l in p.stdout.splitlines() if l.startswith('RESULT ')]
            if p.returncode != 0 or not res:
                sys.exit('grad_clip_bench: %r failed (%d):\n%s\n%s' % (label, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            d = json.loads(res[0][7:])
            times[label].append(d['ms'])
            notes[label] = d
            print('round %d  %-40s median %.4f ms/step' % (r, label, sorted(d['ms'])[len(d['ms']) // 2]), flush=True)
    lines = ['# ms per Tox21 C2 training iteration (batch 256, forward + loss + backward + FlatAdam in one captured graph, %d flat floats);'
             % notes[configs[0][0]]['floats'],
             '# %d rounds x %d blocks of %d replays per configuration, a fresh process per round, configurations alternating; device events.'
             % (args.rounds, args.blocks, args.steps),
             '# median over all blocks [min .. max]; per-round medians; spread = largest - smallest per-round median',
             '%-42s %9s %22s   %s' % ('configuration', 'median', '[min .. max]', 'per-round medians')]
    med = {}
    for label, _, _ in configs:
        allb = sorted(x for rnd in times[label] for x in rnd)
        per = [sorted(rnd)[len(rnd) // 2] for rnd in times[label]]
        med[label] = (allb[len(allb) // 2], max(per) - min(per))
        lines.append('%-42s %9.4f [%9.4f .. %9.4f]   %s' % (label, med[label][0], allb[0], allb[-1], ' '.join('%.4f' % x for x in per)))
    base = configs[0][0]
    for label, _, _ in configs[1:]:
        lines.append('%s - %s: %+.4f ms (%+.2f %%); run-to-run spread of the base %.4f ms'
                     % (label, base, med[label][0] - med[base][0], 100.0 * (med[label][0] / med[base][0] - 1.0), med[base][1]))
    on = notes.get('this tree, clipping on', {})
    if 'clip_stats' in on:
        lines.append('clipping on, last round: %r after %d steps' % (on['clip_stats'], on['steps']))
    print('\n'.join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
