#!/usr/bin/env python3
"""How much of a fused step's period is NOT its kernels?  (a) the normal loop (index build of the next batch on the side stream,
cross-stream wait, graph replay); (b) the two captured step graphs replayed back to back with nothing in between (same resident
batch: kernel chain + bare graph-to-graph gap); (c) the same with an event record + wait on an idle stream's event between replays."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from eagcn_amd.synthetic import bce_weights, make_batch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cfg = dict(bench.WORKLOADS['tox21_c2'])
dev = torch.device('cuda', 0)
mb = make_batch(B=B, n_max=cfg['n_max'], n_med=cfg['n_med'], rel_channels=(28, 4, 2, 2, 2), seed=1234, n_tasks=12)
dense = mb.dense(dev)
labels = torch.from_numpy(mb.labels).to(dev)
bw = torch.tensor(bce_weights(12), dtype=torch.float32, device=dev)
model = bench.build_model(cfg, 0.3, dev, graph=True).train()
params = list(model.parameters())


def step():
    for p in params:
        p.grad = None
    return model.fused_step(dense, labels, 'class', bw, None)[0]


for _ in range(20):
    step()
torch.cuda.synchronize()
n = 300
t0 = time.perf_counter()
for _ in range(n):
    step()
torch.cuda.synchronize()
print('(a) normal loop            %.1f us/step' % ((time.perf_counter() - t0) / n * 1e6))
from eagcn_amd.ops import _index_stream  # noqa: E402
runner = next(iter(model._runners.values()))
g = [runner.graphs[(0, 'step')][1], runner.graphs[(1, 'step')][1]]
side = _index_stream(dev)
main = torch.cuda.current_stream(dev)
hand = runner.handoff


def replay(i):
    """One replay with the runner's own hand-off around it and no batch work: the side stream waits until the slot's last user is
    done and raises the slot's batch-ready flag, which the step graph's first launch polls and clears.  (The flag alone, raised
    once per replay by a host that runs many replays ahead, is raised again before the replay two back has cleared it and is
    then missing when its own replay polls: every such replay sits out the 2 s budget of the poll.)"""
    hand.begin(main, side, True)
    hand.ready(i & 1, main, side, True)
    g[i & 1].replay()
    hand.started()


def run(tag, between):
    for i in range(10):
        between(i)
        replay(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        between(i)
        replay(i)
    torch.cuda.synchronize()
    print('%-44s %.1f us/step' % (tag, (time.perf_counter() - t0) / n * 1e6))


def ev_wait(i):
    ev = torch.cuda.Event()
    ev.record(side)
    main.wait_event(ev)


def ev_record_main(i):
    torch.cuda.Event().record(main)


keep = []


def ev_record_main_side_wait(i):
    ev = torch.cuda.Event()
    ev.record(main)
    side.wait_event(ev)


scalar = torch.zeros((), device=dev)
run('(b) bare replays', lambda i: None)
run('(c) + record(side), main.wait_event', ev_wait)
run('(e) + record(main)', ev_record_main)
run('(f) + record(main), side.wait_event', ev_record_main_side_wait)
run('(g) + clone of a scalar on main', lambda i: scalar.clone())
run('(b) bare replays again', lambda i: None)
