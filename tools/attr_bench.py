#!/usr/bin/env python3
"""Attribution timings on the model engine (eval mode), BASELINE.json configs[1] model (Tox21 synthetic, 2-layer 5-view Concate,
80 / 140 per view, 12 tasks) at B = 256 (N = 132) and B = 1024.  Every variant is ONE captured HIP graph over the same batch index
and buffers, replayed `--reps` times after `--warmup` replays (device time per replay, CUDA events):

    fwd          eagcn_model_forward
    fwd+full     eagcn_model_forward + eagcn_model_backward (every parameter gradient)
    fwd+input    eagcn_model_forward + eagcn_attr_step (input-only backward + packed accumulation)
    ig32         32 x (eagcn_attr_pack_input + forward + eagcn_attr_step) + eagcn_attr_finalize (ops.attribution_launches)

plus ig32 through EAGCN.atom_attributions(graph=True) end to end (index build and input copies included) and molecules/s of it.
Prints one JSON line per shape.

    python tools/attr_bench.py [--B 256 1024] [--steps 32] [--reps 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagcn_amd import EAGCN, ops  # noqa: E402
from eagcn_amd import _lib as L  # noqa: E402
from eagcn_amd.synthetic import make_batch  # noqa: E402


def timed(fn, warmup, reps):
    g = torch.cuda.CUDAGraph()
    fn()                                           # eager warm-up (first launches outside a capture)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run_shape(B, steps, warmup, reps):
    lib = L.load()
    torch.manual_seed(0)
    w1, w2 = [80] * 5, [140] * 5
    model = EAGCN(28, 24, *w1, *w2, 256, 64, 12, 0.0, structure='Concate', n_layers=2).cuda().eval()
    mb = make_batch(B=B, n_max=132, n_med=19, rel_channels=(28, 4, 2, 2, 2), seed=1234)
    adj, afm, *rels, size = [t.cuda() for t in mb.dense()]
    index = ops.BatchIndex(adj, rels, structure=0)
    plan = model.plan()
    m = L.Model.from_buffer_copy(plan.cmodel(False, 0, 0.0))
    m.input_packed = 1
    bufs = ops.attribution_buffers(index.ref(), m, B, index.N, 24, afm.device)
    saved, scratch = bufs['saved'], bufs['scratch']
    sb, wb = saved.numel(), scratch.numel()
    dout = torch.randn(B, 12, device='cuda')
    L.check(lib.eagcn_model_pack_input(index.ref(), C.byref(m), ops._ptr(afm), ops._ptr(saved), sb, ops._stream()), 'pack')
    flat = torch.zeros(plan.offsets[-1], dtype=torch.float32, device='cuda')
    lg, hg = plan.grad_structs(flat)
    nul = C.c_void_p(0)

    def fwd():
        L.check(lib.eagcn_model_forward(index.ref(), C.byref(m), nul, nul, ops._ptr(saved), sb, ops._ptr(scratch), wb,
                                        ops._ptr(bufs['out']), ops._ptr(bufs['graph_rep']), ops._stream()), 'forward')

    def fwd_full():
        fwd()
        L.check(lib.eagcn_model_backward(index.ref(), C.byref(m), nul, ops._ptr(saved), sb, ops._ptr(scratch), wb, ops._ptr(dout), nul,
                                         lg, C.byref(hg), ops._stream()), 'backward')

    def fwd_input():
        fwd()
        L.check(lib.eagcn_attr_step(index.ref(), C.byref(m), nul, ops._ptr(saved), sb, ops._ptr(scratch), wb, ops._ptr(dout), nul,
                                    1.0, 1, ops._ptr(bufs['acc']), ops._stream()), 'attr_step')

    def ig():
        ops.attribution_launches(index.ref(), m, m, nul, saved, scratch, bufs['out'], bufs['graph_rep'], afm, None, dout,
                                 bufs['acc'], bufs['attr'], bufs['score'], steps)

    res = {'B': B, 'N': int(index.N), 'steps': steps}
    res['fwd_ms'] = timed(fwd, warmup, reps)
    res['fwd_full_bwd_ms'] = timed(fwd_full, warmup, reps)
    res['fwd_input_bwd_ms'] = timed(fwd_input, warmup, reps)
    res['ig_graph_ms'] = timed(ig, max(1, warmup // 4), max(1, reps // 4))
    res['ig_over_steps_x_fwd_input'] = res['ig_graph_ms'] / (steps * res['fwd_input_bwd_ms'])
    # end to end through the public API (graph mode: index build + copies + one replay per call)
    gm = EAGCN(28, 24, *w1, *w2, 256, 64, 12, 0.0, structure='Concate', n_layers=2, graph=True).cuda().eval()
    gm.load_state_dict(model.state_dict())
    for _ in range(3):
        gm.atom_attributions(adj, afm, *rels, size=size, target=dout, steps=steps)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(1, reps // 4)
    e0.record()
    for _ in range(n):
        gm.atom_attributions(adj, afm, *rels, size=size, target=dout, steps=steps)
    e1.record()
    torch.cuda.synchronize()
    res['ig_api_ms'] = e0.elapsed_time(e1) / n
    res['ig_api_molecules_per_s'] = B / (res['ig_api_ms'] * 1e-3)
    res['ig_graph_molecules_per_s'] = B / (res['ig_graph_ms'] * 1e-3)
    gm.release_graphs()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--steps', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('attr_bench.py needs the MI355X')
    for B in args.B:
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in run_shape(B, args.steps, args.warmup, args.reps).items()}),
              flush=True)


if __name__ == '__main__':
    main()
