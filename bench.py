#!/usr/bin/env python3
"""Headline benchmark: molecules/sec, forward + backward, 2-layer 5-view Concate EAGCN on a
Tox21-shaped synthetic batch (BASELINE.json metric; SURVEY.md 8d measurement plan).

    python bench.py --gpus 1 --steps 50 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch resident in HBM: batch index build from the
reference's dense collate tensors, all graph-conv layers forward, read-out + head, the train.py loss,
full backward (gradients of every parameter), and for N > 1 the gradient all-reduce.  The optimizer
is excluded.  Weak scaling: every rank processes its own batch of `--batch` molecules.

Timing: after W warm-up steps, exactly K steps are timed, in R blocks (`--repeats`; default: up to 5 blocks
of at least 50 steps each, so that K < 100 is one block) that split the K steps as evenly as possible (barrier + synchronize on both sides of every block, MAX over ranks);
`ms_per_step` / `value` are the MEDIAN block's time per step, `value_min` / `value_max` the slowest /
fastest block's.  `--dump-outputs DIR` writes what the last timed step computed (loss, outputs, graph
representation, a seeded sample of the atom representations, every parameter gradient) as DIR/<name>.npy.
Rank 0 prints ONE JSON line.  At N = 1 the line also carries `extra`: the same measurement for the
north-star shape (Tox21, batch 1024) and the other BASELINE.json configs that fit one GPU,
each with its whole-step fraction of the fp32-MFMA roofline.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

WORKLOADS = {
    # BASELINE.json configs[1]: Tox21 12-task, 2-layer 5-view Concate, batch 256 (fp32 here)
    'tox21_c2': dict(structure='Concate', n_layers=2, widths1=[80] * 5, widths2=[140] * 5, dens=(256, 64),
                     nclass=12, n_bfeat=28, batch=256, n_max=132, n_med=16, task='class'),
    # configs[2]: HIV, 2-layer Weighted_sum, batch 1024, N=222
    'hiv_c3': dict(structure='Weighted_sum', n_layers=2, widths1=[100] * 5, widths2=[250] * 5, dens=(512, 128),
                   nclass=1, n_bfeat=28, batch=1024, n_max=222, n_med=23, task='class'),
    # configs[3]: Lipophilicity regression, 3-layer Concate, batch 4096 over 8 GPUs (512 / GPU)
    'lipo_c4': dict(structure='Concate', n_layers=3, widths1=[60] * 5, widths2=[100] * 5, dens=(128, 64),
                    nclass=1, n_bfeat=18, batch=512, n_max=115, n_med=27, task='reg'),
    # configs[4]: synthetic roofline stress, N = 256 atoms in every molecule, K = 8 views (channels
    # [32,4,2,2,2,2,2,2], widths 64 / 128: SURVEY.md section 8 config table), batch 8192 over 8 GPUs (1024 / GPU)
    'c5_synth': dict(structure='Concate', n_layers=2, widths1=[64] * 8, widths2=[128] * 8, dens=(256, 64),
                     nclass=1, n_bfeat=32, rel_channels=[32, 4, 2, 2, 2, 2, 2, 2], batch=1024, n_max=256, n_med=None,
                     all_full=True, task='reg'),
}
PEAK_FP32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 256 CU x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2500.0     # dense bf16 (v_mfma_f32_32x32x16_bf16); an fp32-equivalent product costs SIX of them (gemm_bx3.hip)
GEMM_MODES = {0: 'f32 (fp32 MFMA v_mfma_f32_16x16x4_f32, exact fp32 products)',
              3: 'f32 (bf16x3 split, fp32 accumulate): every fp32 operand leaves its producer as three bf16 planes, six v_mfma_f32_32x32x16_bf16 '
                 'piece products per 16 k rebuild the fp32 product (csrc/gemm_bx3.hip); aggregation, BatchNorm, head, first layer fp32',
              4: 'bf16 operands (ONE plane, round to nearest even), fp32 accumulate: BASELINE configs[1] as written; NOT the parity path'}
PEAK_HBM_GBS = 8000.0
PMC_FILE = next((os.path.join('profiles', f) for f in ('r06_pmc_traffic.json', 'r05_pmc_traffic.json', 'r04_pmc_traffic.json', 'r03_pmc_traffic.json', 'r02_pmc_traffic.json')
                 if os.path.exists(os.path.join(ROOT, 'profiles', f))), os.path.join('profiles', 'r04_pmc_traffic.json'))


def rel_channels(cfg):
    return list(cfg.get('rel_channels') or [cfg['n_bfeat'], 4, 2, 2, 2])


def build_model(cfg, dropout, device, graph=False):
    from eagcn_amd import EAGCN, weights_init
    # graph_outputs='static' / validate='deferred': the step consumes its outputs at once (loss) and the synthetic
    # batches are valid by construction -- both are reported in the JSON `config`
    m = EAGCN(cfg['n_bfeat'], 24, n_den1=cfg['dens'][0], n_den2=cfg['dens'][1], nclass=cfg['nclass'], dropout=dropout,
              widths1=cfg['widths1'], widths2=cfg['widths2'], rel_channels=rel_channels(cfg), structure=cfg['structure'],
              n_layers=cfg['n_layers'], atom_rep='lazy', grad_mode='direct',
              overlap_index=os.environ.get('EAGCN_BENCH_OVERLAP', '1') == '1', graph=graph,
              graph_outputs='static', validate='deferred')
    m.apply(weights_init)
    return m.to(device)


def algorithmic_flops(cfg, sizes):
    """per molecule, true atom count n, cheaper association per layer, bwd = 2x fwd."""
    K = len(cfg['widths1'])
    w1, w2 = list(cfg['widths1']), list(cfg['widths2'])
    if cfg['structure'] == 'Weighted_sum':
        w1, w2 = [sum(w1)] * K, [sum(w2)] * K
        f1, f2 = w1[0], w2[0]
    else:
        f1, f2 = sum(w1), sum(w2)
    w3 = [2 * w for w in w2]
    plan = [(24, w1, f1), (f1, w2, f2), (f2, w3, 2 * f2), (2 * f2, w3, 2 * f2)][:cfg['n_layers']]
    total = 0.0
    for n in sizes:
        n = float(n)
        for fin, ws, _ in plan:
            for fk in ws:
                total += min(2 * n * n * fin + 2 * n * fin * fk, 2 * n * fin * fk + 2 * n * n * fk)
        f_last = plan[-1][2]
        total += 2 * (f_last * cfg['dens'][0] + cfg['dens'][0] * cfg['dens'][1] + cfg['dens'][1] * cfg['nclass'])
    return 3.0 * total


def algorithmic_bytes(cfg, sizes, n_pad):
    """SURVEY.md 8(d) "algorithmic bytes per molecule": the dense inputs as the reference signature delivers them, read once
    (4 (1 + n_bfeat + sum_{k>=2} C_k) N_pad^2), per layer the forward minimum 4 n F_in + 4 n sum F_k + (K+1) n^2 plus the same
    activations again for the BatchNorm second pass, and twice the forward activations for the backward."""
    chans = rel_channels(cfg)
    K = len(cfg['widths1'])
    w1, w2 = list(cfg['widths1']), list(cfg['widths2'])
    if cfg['structure'] == 'Weighted_sum':
        w1, w2 = [sum(w1)] * K, [sum(w2)] * K
        f1, f2 = w1[0], w2[0]
    else:
        f1, f2 = sum(w1), sum(w2)
    w3 = [2 * w for w in w2]
    plan = [(24, w1), (f1, w2), (f2, w3), (2 * f2, w3)][:cfg['n_layers']]
    dense = 4.0 * (1 + sum(chans)) * n_pad * n_pad * len(sizes)
    act = 0.0
    for n in sizes:
        n = float(n)
        for fin, ws in plan:
            fwd = 4 * n * fin + 4 * n * sum(ws) + (K + 1) * n * n
            act += fwd + 4 * n * sum(ws) * 2 + 2 * (4 * n * fin + 4 * n * sum(ws))     # forward, BatchNorm second pass, backward
    return dense, act


def moved_bytes(cfg, mb):
    """Bytes the DESIGN has to move per step (what `hbm_frac_moved` prices against 8 TB/s): the adjacency read once (4 B N_pad^2),
    one 32-byte sector per (directed bond, relation channel) for the gathered one-hot channels, the uint8 bond codes written once
    and read by the aggregation of every layer and direction, and the per-layer activation minimum of algorithmic_bytes().  The
    84 %% of SURVEY 8(d)'s byte count that are dense one-hot relation planes are NOT in it: the index never streams them."""
    chans = rel_channels(cfg)
    K = len(chans)
    E = int(mb.edges.shape[0])
    rows = float(sum(int(n) for n in mb.sizes))
    ldc = (mb.N + 15) // 16 * 16
    adj = 4.0 * mb.B * mb.N * mb.N
    gathered = 32.0 * E * sum(chans)
    codes = K * rows * ldc * (1 + 3 * cfg['n_layers'])               # written once; read forward, transposed and by the edge gradients
    return adj + gathered + codes + algorithmic_bytes(cfg, mb.sizes, mb.N)[1]


def aggregation_bytes(cfg, rows):
    """Algorithmic bytes per step of the aggregation kernels (what `roofline_aggregation` prices against 8 TB/s): per layer and packed
    row the forward reads P and writes Y' (8 B per column), the backward reads dH, Y' and P and writes dP (16 B per column; the dP
    planes of the plane GEMM are 6 B instead of 4: not counted).  Exact widths; bond lists / codes are < 2 % of it."""
    K = len(cfg['widths1'])
    w1, w2 = list(cfg['widths1']), list(cfg['widths2'])
    if cfg['structure'] == 'Weighted_sum':
        w1, w2 = [sum(w1)] * K, [sum(w2)] * K
    w3 = [2 * w for w in w2]
    cols = sum(sum(ws) for ws in [w1, w2, w3, w3][:cfg['n_layers']])
    return (8.0 + 16.0) * float(rows) * cols


def committed_traffic(kernel_substr):
    """HBM-side bytes per launch of the dominant kernel from the committed PMC passes of this command
    (tools/pmc_traffic.py -> profiles/*_pmc_traffic.json; rocprofv3 cannot run inside bench.py)."""
    try:
        table = json.load(open(os.path.join(ROOT, PMC_FILE)))
    except Exception:
        return None, None
    big = [v for k, v in table.items() if all(part in k for part in kernel_substr.split('|'))]
    n = sum(v['launches'] for v in big)
    if not n:
        return None, None
    return sum(v['hbm_bytes_per_launch'] * v['launches'] for v in big) / n, PMC_FILE


def cpu_baseline(cfg, mb, dropout, bce_w, steps=5, warmup=2, threads=None, sweep_steps=3):
    """The CPU oracle (oracle/eagcn_ref.py, kind 'port') timed on this host, same workload.  `threads`: the thread counts to try
    (default 8 / 16 / 32 / 64 up to the cores available); every count is judged by the median of `sweep_steps` steps after a warm-up
    step, the fastest is timed for `steps` steps and the whole sweep is reported (`thread_sweep`)."""
    from oracle.eagcn_ref import RefEAGCN, classification_loss, regression_loss, weights_init_
    avail = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except Exception:
        pass
    model = RefEAGCN(cfg['n_bfeat'], 24, cfg['widths1'], cfg['widths2'], cfg['dens'][0], cfg['dens'][1],
                     cfg['nclass'], dropout, structure=cfg['structure'], n_layers=cfg['n_layers'],
                     rel_channels=rel_channels(cfg))
    weights_init_(model)
    dense = mb.dense('cpu')
    labels = torch.from_numpy(mb.labels)

    def one_step():
        model.zero_grad(set_to_none=True)
        out, _, _ = model(*dense)
        loss = classification_loss(out, labels, bce_w) if cfg['task'] == 'class' else regression_loss(out, labels)
        loss.backward()

    # the many small ATen ops of this path do not scale to hundreds of threads: pick the fastest of a few thread counts,
    # each judged by the median of three steps after a warm-up step at that count, and report it as `cores`
    best = (None, 1e30)
    cands = sorted({int(c) for c in threads if 1 <= int(c) <= avail}) if threads else [c for c in (8, 16, 32, 64) if c <= avail]
    sweep = {}
    for nt in (cands or [avail]):
        torch.set_num_threads(nt)
        one_step()
        ts = []
        for _ in range(sweep_steps):
            t0 = time.perf_counter()
            one_step()
            ts.append(time.perf_counter() - t0)
        dt = sorted(ts)[len(ts) // 2]
        sweep[nt] = round(mb.B / dt, 1)
        if dt < best[1]:
            best = (nt, dt)
    cores = best[0]
    torch.set_num_threads(cores)
    ts = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        one_step()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    ts.sort()
    med = ts[len(ts) // 2]
    model_name = ''
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    model_name = line.split(':', 1)[1].strip()
                    break
    except Exception:
        pass
    return {'value': mb.B / med, 'unit': 'molecules/s', 'cores': cores, 'kind': 'port', 'thread_sweep': sweep,
            'sample': '%d timed fwd+bwd steps (median, after %d warm-up) of the same %d-molecule batch (%d tasks, N_pad %d), '
                      'oracle/eagcn_ref.py RefEAGCN on torch %s CPU, %d threads (%s), %s'
                      % (steps, warmup, mb.B, cfg['nclass'], mb.N, torch.__version__, cores,
                         'fastest of %s by the median of %d warmed step(s) each' % ('/'.join(str(c) for c in sweep), sweep_steps),
                         model_name or 'unknown CPU')}


DUMP_LIMIT_BYTES = 64 << 20          # --dump-outputs: at most this much in all
DUMP_ARRAY_BYTES = 16 << 20          # a larger array is stored as a fixed, seeded sample of this size


BLOCKS_DEFAULT, BLOCK_MIN_STEPS = 5, 50    # --repeats not given: up to 5 blocks, none shorter than 50 steps


def block_sizes(steps, repeats):
    """The `steps` timed steps split into min(repeats, steps) blocks as evenly as possible (repeats None: the default)."""
    if repeats is None:
        repeats = min(BLOCKS_DEFAULT, steps // BLOCK_MIN_STEPS)
    n = max(1, min(repeats, steps))
    return [steps // n + (1 if i < steps % n else 0) for i in range(n)]


def host_outputs(model, loss, outs):
    """What a caller of the timed step receives, copied to the host at once (the step's buffers are static and reused):
    {name: float32 / float64 numpy array}.  An array above DUMP_ARRAY_BYTES is a fixed, seeded sample of its elements."""
    out, atom_rep, graph_rep = outs
    arrays = [('loss', loss), ('out', out), ('graph_representation', graph_rep)]
    if atom_rep is not None:
        arrays.append(('atom_representations', atom_rep.cpu() if hasattr(atom_rep, 'cpu') else atom_rep))
    arrays += [('grad.' + k, p.grad) for k, p in model.named_parameters() if p.grad is not None]
    res = {}
    for name, t in arrays:
        if not isinstance(t, torch.Tensor):
            continue
        a = t.detach().cpu()
        a = (a if a.dtype == torch.float64 else a.float()).numpy()
        if a.nbytes > DUMP_ARRAY_BYTES:
            keep = DUMP_ARRAY_BYTES // a.itemsize
            idx = np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))
            a, name = a.reshape(-1)[idx], name + '.sample'
        res[name] = np.ascontiguousarray(a)
    return res


def dump_outputs(d, arrays):
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit('--dump-outputs: %d bytes exceed the %d-byte limit' % (total, DUMP_LIMIT_BYTES))
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + '.npy'), a)


def run_workload(name, B, args, lib, dev, rank, world, reducer_cls, detail):
    """Build the model and one resident batch, time K steps in R blocks.  Returns a dict (timings are the MAX over
    ranks); with `detail` also the per-kernel-class HIP-event durations of eager steps of the same workload."""
    from eagcn_amd.losses import fused_classification_loss, fused_regression_loss
    from eagcn_amd.synthetic import bce_weights, make_batch
    cfg = dict(WORKLOADS[name])
    torch.manual_seed(1234 + rank)
    nrot = max(1, int(getattr(args, 'rotate', 1)))
    mbs = [make_batch(B=B, n_max=cfg['n_max'], n_med=cfg['n_med'], rel_channels=rel_channels(cfg),
                      seed=1234 + rank + 1000 * i, n_tasks=cfg['nclass'], task=cfg['task'], all_full=cfg.get('all_full', False))
           for i in range(nrot)]
    mb = mbs[0]
    denses = [m_.dense(dev) if args.input == 'dense' else None for m_ in mbs]
    compacts = [m_.compact(dev) if args.input == 'compact' else None for m_ in mbs]
    labelss = [torch.from_numpy(m_.labels).to(dev) for m_ in mbs]
    dense, compact, labels = denses[0], compacts[0], labelss[0]
    counter = [0]
    last = [None]                   # (out, atom_rep, graph_rep) of the latest step
    bce_w = bce_weights(cfg['nclass'])
    bce_w_dev = torch.tensor(bce_w, dtype=torch.float32, device=dev)
    model = build_model(cfg, args.dropout, dev, graph=not args.eager)
    model.train()
    reducer = reducer_cls(model.parameters(), model=model)
    params = list(model.parameters())

    fused = (not args.eager) and not args.separate_graphs
    # --optimizer: the whole training iteration of train.py:310-334 (zero_grad, forward, loss, backward, Adam(lr, weight_decay)).
    # 'flat' = eagcn_amd.optim.FlatAdam, ONE kernel over the flat parameter buffer, captured into the step graph;
    # 'torch' = torch.optim.Adam (foreach) on the same parameters, launched by the host behind every step graph.
    opt_kind = getattr(args, 'optimizer', 'none')
    optimizer = None
    if opt_kind == 'flat':
        from eagcn_amd.optim import FlatAdam
        optimizer = FlatAdam(model, lr=1e-4, weight_decay=1e-4)
    elif opt_kind == 'torch':
        optimizer = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)

    def step():
        i = counter[0] % nrot       # resident batches taken round-robin (--rotate; 1: the same batch every step)
        counter[0] += 1
        dense, compact, labels = denses[i], compacts[i], labelss[i]
        for p in params:            # optimizer.zero_grad(set_to_none=True) of the reference loop (train.py:317)
            p.grad = None
        if fused and model.graph:
            # forward + loss + backward as ONE captured graph (EAGCN.fused_step, what eagcn_amd.training.train_step runs); with
            # more than one rank the gradient average is captured INTO that graph (upper bucket beside the first layer's
            # backward) and the global BCE normalisation is a 1-element collective issued with the batch preparation
            batch = dense if compact is None else (compact[1], compact[2])
            loss, last[0] = model.fused_step(batch, labels, cfg['task'], bce_w_dev, 'dp' if (world > 1 and cfg['task'] == 'class') else None,
                                       bonds=None if compact is None else compact[0], reducer=reducer if world > 1 else None,
                                       **({'optimizer': optimizer} if opt_kind == 'flat' else {}))
            if opt_kind == 'torch':
                optimizer.step()
            return loss
        last[0] = model(*dense) if compact is None else model.forward_compact(*compact)
        out = last[0][0]
        if cfg['task'] == 'class':
            loss = fused_classification_loss(out, labels, bce_w_dev, dp_global_norm=(world > 1))
        else:
            loss = fused_regression_loss(out, labels)
        loss.backward()
        reducer()
        if optimizer is not None:
            optimizer.step()
        return loss

    # set-up, not warm-up: a graph-mode model issues its first step per buffer slot eagerly and captures it (two slots; with more
    # than one rank each capture is preceded by a 0.35 s drain of the eager collectives, eagcn_amd/graph.py) -- those four steps
    # must not land in the timed region when the caller asks for fewer than four warm-up steps
    for _ in range(max(0, 4 - args.warmup) if not args.eager else 0):
        step()
    for _ in range(args.warmup):
        step()
    profile_in_loop = args.eager and detail   # HIP events cannot bracket kernels inside a replayed graph
    lib.eagcn_prof_reset()
    blocks = []
    loss = None
    sizes = block_sizes(args.steps, args.repeats)
    for nsteps in sizes:
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        lib.eagcn_prof_enable(1 if profile_in_loop else 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            loss = step()
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        lib.eagcn_prof_enable(0)
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if dist.is_initialized():
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        blocks.append(float(t.item()) / nsteps)          # seconds per step of this block
    if not torch.isfinite(loss.detach()).item():
        raise SystemExit('non-finite loss')
    dumped = host_outputs(model, loss, last[0]) if (detail and rank == 0 and args.dump_outputs) else None
    res = {'cfg': cfg, 'mb': mb, 'bce_w': bce_w, 'B': B, 'blocks': sorted(blocks), 'dumped': dumped,
           'gflop': algorithmic_flops(cfg, mb.sizes) / 1e9, 'N': mb.N, 'bytes': algorithmic_bytes(cfg, mb.sizes, mb.N),
           'moved': moved_bytes(cfg, mb),
           'rank_ms': None, 'allreduce': None}
    if dist.is_initialized() and world > 1:
        mine = torch.tensor([sorted(blocks)[len(blocks) // 2] * 1e3], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        res['rank_ms'] = [round(float(t), 4) for t in every]
        runner = next(iter(model._runners.values()), None) if model.graph else None
        res['allreduce'] = ('in-place AVG of the flat fp32 gradient buffer over RCCL, captured inside the step graph: bucket [layers >= 2 '
                            '+ head] started before the first layer\'s backward, bucket [layer 1] after it'
                            if (runner is not None and runner.comm_in_graph) else
                            'in-place AVG of the flat fp32 gradient buffer over RCCL, one host-issued collective after the step graph')
    prof_steps = args.steps
    if detail and not profile_in_loop:
        # per-kernel-class durations: the same step, same batch, eager launches with one HIP-event pair per
        # kernel class on the launch stream (the timed region above replays the identical kernels as graphs)
        model.graph = False
        prof_steps = min(args.steps, 30)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        lib.eagcn_prof_reset()
        lib.eagcn_prof_enable(1)
        for _ in range(prof_steps):
            step()
        torch.cuda.synchronize()
        lib.eagcn_prof_enable(0)
        model.graph = not args.eager
    kern = {}
    if detail:
        for tag in range(lib.eagcn_prof_ntags()):
            ms, work, n = C.c_double(), C.c_double(), C.c_int64()
            lib.eagcn_prof_read(tag, C.byref(ms), C.byref(work), C.byref(n))
            kern[lib.eagcn_prof_tag_name(tag).decode()] = (ms.value, work.value, n.value)
    res.update(kern=kern, prof_steps=prof_steps, profile_in_loop=profile_in_loop)
    if detail and args.eval_throughput and not args.eager:
        model.eval()
        with torch.no_grad():
            for _ in range(10):
                model(*dense) if compact is None else model.forward_compact(*compact)
            torch.cuda.synchronize()
            te = time.perf_counter()
            for _ in range(args.steps):
                model(*dense) if compact is None else model.forward_compact(*compact)
            torch.cuda.synchronize()
            te = time.perf_counter() - te
        model.train()
        res['eval_forward'] = {'molecules_per_s': round(B * args.steps / te, 1), 'ms_per_batch': round(te / args.steps * 1e3, 4),
                               'execution': 'forward-only HIP graph, eval mode, no_grad'}
    return res


def summarize(res, args, world):
    """(value, ms_per_step, min, max, step_frac) of a run_workload result: median block (`blocks`: seconds per step)."""
    b = res['blocks']
    med = b[len(b) // 2]
    ms = med * 1e3
    value = world * res['B'] / med
    dense_b, act_b = res['bytes']
    t_mfma = res['gflop'] / PEAK_FP32_MFMA_TFLOPS                     # ms at the fp32 MFMA peak
    t_hbm = (dense_b + act_b) / (PEAK_HBM_GBS * 1e6)                   # ms at 8 TB/s
    return {'value': round(value, 1), 'ms_per_step': round(ms, 4),
            'value_min': round(world * res['B'] / b[-1], 1), 'value_max': round(world * res['B'] / b[0], 1),
            'algorithmic_gflop_per_step': round(res['gflop'], 3),
            'step_tflops': round(res['gflop'] / ms, 2), 'step_frac': round(res['gflop'] / ms / PEAK_FP32_MFMA_TFLOPS, 4),
            # "report both numbers per config; relevant roofline = max(T_flops, T_bytes)"
            'algorithmic_mbytes_per_step': {'dense_inputs': round(dense_b / 1e6, 1), 'activations': round(act_b / 1e6, 1)},
            'hbm_frac': round(t_hbm / ms, 4), 'relevant_roofline': 'hbm' if t_hbm > t_mfma else 'mfma',
            # the same against the bytes the design must move (moved_bytes(): no dense one-hot planes)
            'moved_mbytes_per_step': round(res['moved'] / 1e6, 1), 'hbm_frac_moved': round(res['moved'] / (PEAK_HBM_GBS * 1e6) / ms, 4),
            'relevant_frac': round(max(t_hbm, t_mfma) / ms, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50, help='timed steps (in all)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=None,
                    help='timed blocks the --steps steps are split into; the median block is reported (default: up to %d blocks of at '
                         'least %d steps)' % (BLOCKS_DEFAULT, BLOCK_MIN_STEPS))
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed (loss, outputs, graph representation, a seeded sample of the atom '
                         'representations, every parameter gradient) as DIR/<name>.npy, float32 / float64, at most 64 MB in all')
    ap.add_argument('--workload', default='tox21_c2', choices=sorted(WORKLOADS))
    ap.add_argument('--batch', type=int, default=None, help='molecules per GPU (default: the config\'s)')
    ap.add_argument('--dropout', type=float, default=0.3)
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--rotate', type=int, default=1, help='distinct HBM-resident batches per rank, taken round-robin (1: the same batch every step)')
    ap.add_argument('--optimizer', choices=('none', 'flat', 'torch'), default='none',
                    help="add the optimizer step to the timed step: 'flat' = eagcn_amd.optim.FlatAdam inside the step graph, 'torch' = torch.optim.Adam "
                         "behind it (the headline metric is fwd+bwd: BASELINE.json; extra.train_step carries the whole iteration)")
    ap.add_argument('--no-extras', action='store_true', help='skip the extra single-GPU shapes (north-star batch 1024, HIV, Lipo, C5)')
    ap.add_argument('--eager', action='store_true', help='eager launches instead of HIP-graph replay')
    ap.add_argument('--separate-graphs', action='store_true', help='graph mode with separate forward / backward graphs and an eager loss kernel '
                    '(the nn.Module call sequence) instead of the single whole-step graph')
    ap.add_argument('--cpu-steps', type=int, default=5)
    ap.add_argument('--eval-throughput', action='store_true',
                    help='also time the eval-mode forward (forward-only graph under no_grad); reported as an extra field')
    ap.add_argument('--gemm-mode', type=int, default=None, help='layer products: 3 (default) bf16x3 planes on the bf16 matrix cores, 0 fp32 MFMA, '
                    '4 one bf16 plane (eagcn_set_gemm_mode)')
    ap.add_argument('--require-in-graph-allreduce', action='store_true',
                    help='N > 1: fail instead of falling back to a host-issued all-reduce when the collective cannot be captured into the step graph')
    ap.add_argument('--input', default='dense', choices=('dense', 'compact'),
                    help="dense: the reference's collate tensors (headline); compact: bond list via forward_compact")
    args = ap.parse_args()
    if args.steps < 1 or (args.repeats is not None and args.repeats < 1):
        raise SystemExit('--steps and --repeats must be >= 1')

    if args.require_in_graph_allreduce:
        os.environ['EAGCN_REQUIRE_IN_GRAPH_ALLREDUCE'] = '1'      # (read by eagcn_amd.graph at import)
    from eagcn_amd import _lib
    from eagcn_amd.parallel import GradientAllReducer, init_distributed
    lib = _lib.load()                                    # fail loudly if the HIP library is missing
    if args.gemm_mode is not None:
        lib.eagcn_set_gemm_mode(args.gemm_mode)
    gemm_mode = lib.eagcn_set_gemm_mode(0)
    lib.eagcn_set_gemm_mode(gemm_mode)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X: there is no CPU path')
    rank, world, local = init_distributed()
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run)' % (args.gpus, world))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    B = args.batch or WORKLOADS[args.workload]['batch']
    res = run_workload(args.workload, B, args, lib, dev, rank, world, GradientAllReducer, detail=True)
    cfg, mb, kern = res['cfg'], res['mb'], res['kern']
    if res['dumped'] is not None:
        dump_outputs(args.dump_outputs, res['dumped'])
        res['dumped'] = None
    out = None
    if rank == 0:
        head = summarize(res, args, world)
        # dominant kernel: the paired backward products of the hidden layers (dX = dP.W^T and dW = X^T.dP in one launch);
        # models without a hidden layer below the top have no such launch -> the plain layer GEMMs
        pair = kern.get('gemm_pair', (0.0, 0.0, 0))[2] > 0
        g_ms, g_work, g_n = kern['gemm_pair'] if pair else kern['gemm']
        achieved = (g_work / (g_ms * 1e-3)) / 1e12 if g_ms > 0 else 0.0
        traffic, traffic_src = committed_traffic('bx3_kernel|pair' if gemm_mode == 3 else 'gemm3_kernel<false, true') if args.workload == 'tox21_c2' and B == 256 else (None, None)
        prof_steps = res['prof_steps']
        out = {
            'metric': 'molecules/sec fwd+bwd, 2-layer 5-view EAGCN, Tox21 batch' if args.workload == 'tox21_c2'
                      else 'molecules/sec fwd+bwd, EAGCN %s' % args.workload,
            'value': head['value'], 'unit': 'molecules/s', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': head['ms_per_step'], 'higher_is_better': True,
            'scaling': 'weak', 'vs_baseline': None, 'dtype': GEMM_MODES.get(gemm_mode, 'f32 (gemm mode %d)' % gemm_mode), 'data': 'synthetic',
            'repeats': len(res['blocks']), 'value_min': head['value_min'], 'value_max': head['value_max'],
            'timing': '%d timed steps in %d block(s) of %s steps (barrier + synchronize around every block, max over ranks); median block\'s '
                      'time per step; value_min / value_max = slowest / fastest block' % (args.steps, len(res['blocks']),
                                                                                          '/'.join(str(n) for n in block_sizes(args.steps, args.repeats))),
            'config': {'workload': '%s: %s, %d-layer %d-view, widths %s/%s, %d tasks, batch %d per GPU, '
                                   'N_pad %d, dropout %.2f, loss %s' %
                                   (args.workload, cfg['structure'], cfg['n_layers'], len(cfg['widths1']),
                                    cfg['widths1'][0], cfg['widths2'][0], cfg['nclass'], B, mb.N, args.dropout,
                                    'weighted BCE' if cfg['task'] == 'class' else 'MSE'),
                       'input': args.input, 'inputs': 'HBM-resident (%d synthetic batch%s per rank, %s)' % (args.rotate, '' if args.rotate == 1 else 'es', 'reused every step' if args.rotate == 1 else 'round-robin'),
                       'overlap_index': os.environ.get('EAGCN_BENCH_OVERLAP', '1') == '1', 'graph_outputs': 'static', 'validate': 'deferred',
                       'optimizer': 'excluded (SURVEY.md 8d: forward + loss + backward [+ gradient all-reduce])',
                       'global_batch': world * B, 'atoms_per_batch': int(mb.sizes.sum()),
                       'parallelism': 'dp%d' % world},
            'algorithmic_gflop_per_step': head['algorithmic_gflop_per_step'],
            'roofline': {'kernel': (('bx3_kernel<3> (dX = dP.W^T and dW = X^T.dP of a hidden layer in one persistent launch from bf16x3 operand planes: '
                                     '6 x v_mfma_f32_32x32x16_bf16 per fp32-equivalent product: piece products to 3 x 2^-24, fp32 accumulate)' if gemm_mode == 3 else
                                     'gemm3_kernel<false, true, true> (dX = dP.W^T and dW = X^T.dP of a hidden layer in one balanced launch, fp32 MFMA)')
                                    if pair else 'layer GEMMs (flat X.[W_1..W_K] transform and its backward products)'),
                         'bound': 'mfma', 'achieved': round(achieved, 3),
                         # the peak of the instruction actually issued: dense bf16 / 6 piece products in mode 3, the fp32 MFMA rate in mode 0
                         'peak': round(PEAK_BF16_MFMA_TFLOPS / 6.0, 1) if (gemm_mode == 3 and pair) else PEAK_FP32_MFMA_TFLOPS,
                         'peak_fp32_mfma': PEAK_FP32_MFMA_TFLOPS,
                         'unit': 'TFLOP/s',
                         'frac': round(achieved / ((PEAK_BF16_MFMA_TFLOPS / 6.0) if (gemm_mode == 3 and pair) else PEAK_FP32_MFMA_TFLOPS), 4),
                         'frac_of_fp32_mfma_peak': round(achieved / PEAK_FP32_MFMA_TFLOPS, 4),
                         'step_frac': head['step_frac'],
                         'step_frac_note': 'whole step: algorithmic_gflop_per_step / ms_per_step / peak',
                         'hbm': {'algorithmic_mbytes_per_step': head['algorithmic_mbytes_per_step'], 'peak_gbs': PEAK_HBM_GBS,
                                 'step_frac': head['hbm_frac'],
                                 'note': 'whole step against the HBM bound: SURVEY 8(d) algorithmic bytes (dense collate tensors as the '
                                         'signature delivers them, read once + per-layer activation minimum) / ms_per_step / 8 TB/s; the '
                                         'implementation streams adj and gathers the relation channels at the bonds only'},
                         'relevant': head['relevant_roofline'], 'relevant_step_frac': head['relevant_frac'],
                         'hbm_frac_moved': head['hbm_frac_moved'], 'moved_mbytes_per_step': head['moved_mbytes_per_step'],
                         'hbm_frac_moved_note': 'whole step against 8 TB/s on the bytes the design has to move (adjacency once, one sector per '
                                                'bond and relation channel, bond codes, activation minimum): bench.py moved_bytes()',
                         'traffic': None if traffic is None else round(traffic),
                         'traffic_note': None if traffic is None else
                         'bytes per launch, memory-side FETCH_SIZE x2 + WRITE_SIZE from %s' % traffic_src,
                         'launches': int(g_n), 'avg_launch_us': round(g_ms * 1e3 / max(g_n, 1), 3),
                         'measured': 'HIP events on the launch stream, %s' % ('inside the timed region' if res['profile_in_loop'] else
                                     '%d eager steps of the same workload right after the timed graph-replay region' % prof_steps)},
            # second roofline object: the aggregation kernels of all layers, both directions, as one class (HIP events: PROF_AGG)
            'roofline_aggregation': {
                'kernel': 'lagg_kernel<false|true> / agg_kernel / agg_wave_kernel / agg_edge_kernel: every aggregation launch of the step '
                          '(forward Y\' = A^.P, backward dP = A^T.dY\' + edge gradients [+ BatchNorm-backward second pass])',
                'bound': 'hbm', 'unit': 'GB/s', 'peak': PEAK_HBM_GBS,
                'achieved': round(aggregation_bytes(cfg, mb.sizes.sum()) / 1e9 / max(kern['agg'][0] / prof_steps * 1e-3, 1e-12), 1),
                'frac': round(aggregation_bytes(cfg, mb.sizes.sum()) / 1e9 / max(kern['agg'][0] / prof_steps * 1e-3, 1e-12) / PEAK_HBM_GBS, 4),
                'algorithmic_mbytes_per_step': round(aggregation_bytes(cfg, mb.sizes.sum()) / 1e6, 1),
                'ms_per_step': round(kern['agg'][0] / prof_steps, 4), 'launches_per_step': int(kern['agg'][2] / max(prof_steps, 1)),
                'note': 'at Tox21 batch sizes these launches are a few workgroups per CU, each working ONE block of rows through its '
                        'barrier-separated phases: latency, not bytes (DESIGN.md 9 item 1)'},
            'layer_gemm_tflops_all': round(((kern['gemm'][1] + kern.get('gemm_pair', (0, 0, 0))[1]) /
                                            max((kern['gemm'][0] + kern.get('gemm_pair', (0, 0, 0))[0]) * 1e-3, 1e-12)) / 1e12, 3),
            'kernel_ms_per_step': {k: round(v[0] / prof_steps, 4) for k, v in kern.items()},
            'execution': 'eager launches' if args.eager else ('HIP graph replay (forward graph, eager loss kernel, backward graph), eager batch index' if args.separate_graphs else 'one HIP graph per step (forward + fused loss + backward; EAGCN.fused_step), eager batch index'),
        }
        if 'eval_forward' in res:
            out['eval_forward'] = res['eval_forward']
        if world > 1:
            out['rccl_world'] = dist.get_world_size()
            out['ms_per_step_by_rank'] = res['rank_ms']
            out['gradient_allreduce'] = res['allreduce']
            out['batchnorm'] = 'local-BN (every shard = a reference run at batch %d)' % B
    # ---- other single-GPU shapes: same measurement, fewer blocks ------------------------------------------------------
    if world == 1 and not args.no_extras and args.workload == 'tox21_c2' and args.batch is None and not args.eager:
        keep = (args.repeats, args.steps, args.warmup)
        keep_rotate = args.rotate
        keep_opt = args.optimizer
        extra = {}
        M = gemm_mode
        for key, (wname, wb, steps, mode) in (('b1024', ('tox21_c2', 1024, 30, M)), ('hiv_c3', ('hiv_c3', 1024, 10, M)),
                                               ('lipo_c4', ('lipo_c4', 512, 30, M)), ('c5_synth', ('c5_synth', 1024, 6, M)),
                                               # the same steps with the layer products on the fp32 MFMA (gemm mode 0: round 3's path)
                                               ('c2_fp32_mfma', ('tox21_c2', 256, 50, 0)), ('b1024_fp32_mfma', ('tox21_c2', 1024, 30, 0)),
                                               ('hiv_c3_fp32_mfma', ('hiv_c3', 1024, 10, 0)), ('c5_synth_fp32_mfma', ('c5_synth', 1024, 6, 0)),
                                               ('c2_bf16', ('tox21_c2', 256, 50, 4)), ('b1024_bf16', ('tox21_c2', 1024, 30, 4)),
                                               ('c2_rotate4', ('tox21_c2', 256, 50, M)), ('b1024_rotate4', ('tox21_c2', 1024, 30, M)),
                                               # the WHOLE training iteration (train.py:310-334): + Adam(lr, weight_decay)
                                               ('train_step', ('tox21_c2', 256, 50, M)), ('train_step_torch_adam', ('tox21_c2', 256, 50, M)),
                                               ('b1024_train_step', ('tox21_c2', 1024, 30, M))):
            del res
            torch.cuda.empty_cache()
            args.repeats, args.steps, args.warmup = 5, 5 * steps, 4      # 5 blocks of `steps` steps
            args.rotate = 4 if key.endswith('rotate4') else 1
            args.optimizer = 'torch' if key.endswith('torch_adam') else ('flat' if 'train_step' in key else keep_opt)
            old_mode = lib.eagcn_set_gemm_mode(mode)         # fresh model + fresh graphs per workload: captured with this mode
            try:
                res = run_workload(wname, wb, args, lib, dev, rank, world, GradientAllReducer, detail=False)
            finally:
                lib.eagcn_set_gemm_mode(old_mode)
            e = summarize(res, args, world)
            e['workload'] = '%s, batch %d, N_pad %d, %d blocks of %d steps%s' % (wname, wb, res['N'], args.repeats, args.steps // args.repeats,
                                                                                 ', 4 distinct resident batches round-robin (the side-stream index build reads fresh data every step)' if args.rotate > 1 else '')
            e['dtype'] = GEMM_MODES.get(mode, 'gemm mode %d' % mode)
            if mode == 4:
                e['dtype'] += (': hidden-layer products X.W, dP.W^T, X^T.dP from ONE bf16 plane per operand, written by the producers; '
                               'aggregation, BatchNorm, head and first layer fp32; error vs the fp32 oracle in tests/test_gpu_bf16.py')
            if 'train_step' in key:
                e['step'] = ('zero_grad + forward + loss + backward + Adam(lr, weight_decay=1e-4) [train.py:310-334]: ' +
                             ('torch.optim.Adam (foreach) launched by the host behind every step graph' if args.optimizer == 'torch' else
                              'eagcn_amd.optim.FlatAdam, one kernel over the flat parameter buffer, captured as the last launch of the step graph'))
            extra[key] = e
        args.optimizer = keep_opt
        args.repeats, args.steps, args.warmup = keep
        args.rotate = keep_rotate
        out['extra'] = extra
    if rank == 0:
        if world == 1 and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(cfg, mb, args.dropout, bce_w_of(cfg), steps=args.cpu_steps)
            if args.workload == 'tox21_c2':
                # BASELINE.json configs[0] as written: Tox21 single-task, 2-layer 5-view Concate, batch 64, fp32 on the CPU
                from eagcn_amd.synthetic import make_batch
                c1 = dict(WORKLOADS['tox21_c2'], nclass=1)
                mb1 = make_batch(B=64, n_max=c1['n_max'], n_med=c1['n_med'], rel_channels=rel_channels(c1), seed=4321, n_tasks=1, task='class')
                out['cpu_baseline_configs0'] = cpu_baseline(c1, mb1, args.dropout, bce_w_of(c1), steps=args.cpu_steps)
                # the north-star batch (BASELINE.json north_star quotes its >= 10x target at batch 1024; a step is ~10-15 s of CPU
                # work): a 4x larger batch may scale to more threads than batch 256 does, so the count found fastest there, twice and
                # four times it are each tried (one warmed step), and the fastest is timed for three steps; the sweep is in the record
                mb2 = make_batch(B=1024, n_max=cfg['n_max'], n_med=cfg['n_med'], rel_channels=rel_channels(cfg), seed=1234, n_tasks=cfg['nclass'], task=cfg['task'])
                c256 = out['cpu_baseline']['cores']
                out['cpu_baseline_b1024'] = cpu_baseline(cfg, mb2, args.dropout, bce_w_of(cfg), steps=3, warmup=0,
                                                         threads=[c256, 2 * c256, 4 * c256], sweep_steps=1)
        # the numbers DESIGN.md quotes, compact, at the END of the line (the driver keeps the tail of long lines)
        summ = {'c2': [out['ms_per_step'], out['value']], 'roofline_frac': out['roofline']['frac'], 'dominant_kernel_us': out['roofline']['avg_launch_us'],
                'step_frac': out['roofline']['step_frac'], 'hbm_frac_moved': out['roofline']['hbm_frac_moved'],
                'agg_hbm_frac': out['roofline_aggregation']['frac']}
        for k, e in out.get('extra', {}).items():
            summ[k] = [e['ms_per_step'], e['value']]
        for k in ('cpu_baseline', 'cpu_baseline_configs0', 'cpu_baseline_b1024'):
            if k in out:
                summ[k] = [round(out[k]['value'], 1), out[k]['cores']]
        if 'cpu_baseline_b1024' in out and 'extra' in out and 'b1024' in out['extra']:
            summ['b1024_gpu_over_cpu'] = round(out['extra']['b1024']['value'] / out['cpu_baseline_b1024']['value'], 1)
        out['extra_summary'] = summ
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        # orderly teardown: no captured graph (they hold RCCL kernels) and no pending collective outlives the communicator
        import gc
        torch.cuda.synchronize()
        gc.collect()
        dist.barrier()
        torch.cuda.synchronize()
        dist.destroy_process_group()


def bce_w_of(cfg):
    from eagcn_amd.synthetic import bce_weights
    return bce_weights(cfg['nclass'])


if __name__ == '__main__':
    main()
