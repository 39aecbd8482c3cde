"""Time of one evaluation's METRICS over filled evaluation buffers: the torch-op path (training.auc_per_task / training.rmse: a Python
loop of ATen calls with host syncs) against the device path (EvalBuffers.metrics() = two HIP launches, plus one accessor = the one
device-to-host copy).  Both run in this process, alternating, after a warm-up; a repetition is timed by a host clock around work that
ends in a device synchronise.  Inputs come from a seed.  Needs the GPU: there is no CPU fallback to time.

    python tools/eval_metrics_bench.py [--reps 200] [--warmup 20] [--out profiles/eval_metrics_speed.txt]

Shapes (rows x tasks): the validation and training sets of Tox21 (12 tasks, 4 % positives, 15 % missing labels) and HIV (1 task,
3.5 % positives) as train.py evaluates them, and Lipophilicity (regression) for the RMSE / MAE kernels."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [('tox21_val', 783, 12, 'class', 0.04, 0.15), ('tox21_train', 6264, 12, 'class', 0.04, 0.15),
          ('hiv_val', 4113, 1, 'class', 0.035, 0.0), ('hiv_train', 32901, 1, 'class', 0.035, 0.0),
          ('lipo_val', 420, 1, 'reg', 0.0, 0.0), ('lipo_train', 3360, 1, 'reg', 0.0, 0.0)]


def make_buffers(rows, T, task, pos, missing, seed):
    from eagcn_amd.training import EvalBuffers
    rng = np.random.RandomState(seed)
    buf = EvalBuffers(T, task == 'class', torch.device('cuda'), cap=rows)
    if task == 'class':
        u = rng.rand(rows, T)
        y = np.where(u < missing, -1.0, np.where(u < missing + pos * (1.0 - missing), 1.0, 0.0)).astype(np.float32)
        # scores that separate the classes partly, as a trained model's do
        s = (1.0 / (1.0 + np.exp(-(rng.randn(rows, T) + 1.5 * (y == 1))))).astype(np.float32)
        valid = (y != -1)
    else:
        y = rng.randn(rows, T).astype(np.float32)
        s = (y + 0.5 * rng.randn(rows, T)).astype(np.float32)
        valid = np.ones((rows, T), dtype=bool)
    buf.scores[:rows], buf.targets[:rows] = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    buf.valid[:rows] = torch.from_numpy(valid).cuda().to(torch.uint8)
    buf.rows = rows
    return buf


def count_launches(fn):
    """device kernels + memory copies of one call, from the torch profiler (a run of its own, after the timing)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def stats(ts):
    a = np.sort(np.array(ts)) * 1e3
    return float(np.median(a)), float(a[len(a) // 10]), float(a[(9 * len(a)) // 10]), float(a[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-launch-count', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('eval_metrics_bench: needs the GPU (nothing to time without one)')
    if args.reps < 200:
        sys.exit('eval_metrics_bench: at least 200 repetitions per path')
    from eagcn_amd import training
    lines = ['# ms per evaluation of the metrics over filled buffers on %s; %d alternating repetitions per path after %d warm-up;'
             % (torch.cuda.get_device_name(0), args.reps, args.warmup),
             '# median [p10 .. p90] min; spread = p90 - p10; torch = auc_per_task / rmse (ATen ops + host syncs), device = EvalBuffers.metrics()',
             '# + one accessor (two launches + one device-to-host copy).  Condition: device median <= torch median + torch spread.',
             '%-12s %6s %3s | %-34s | %-34s | %7s %s' % ('shape', 'rows', 'T', 'torch ms', 'device ms', 'ratio', 'condition')]
    counts = []
    for name, rows, T, task, pos, missing in SHAPES:
        buf = make_buffers(rows, T, task, pos, missing, args.seed)
        if task == 'class':
            def torch_path(buf=buf):
                return training.auc_per_task(*buf.views())[1]

            def device_path(buf=buf):
                return buf.metrics().mean_auc
        else:
            def torch_path(buf=buf):
                return training.rmse(*buf.views()[:2])

            def device_path(buf=buf):
                return buf.metrics().rmse
        a, b = torch_path(), device_path()
        assert abs(a - b) <= 1e-9, (name, a, b)                    # the two paths time the same number
        tt, td = [], []
        for rep in range(args.warmup + args.reps):
            for fn, acc in ((torch_path, tt), (device_path, td)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    acc.append(time.perf_counter() - t0)
        st, sd = stats(tt), stats(td)
        ok = sd[0] <= st[0] + (st[2] - st[1])
        lines.append('%-12s %6d %3d | %8.4f [%8.4f .. %8.4f] %8.4f | %8.4f [%8.4f .. %8.4f] %8.4f | %6.1fx %s'
                     % (name, rows, T, st[0], st[1], st[2], st[3], sd[0], sd[1], sd[2], sd[3], st[0] / sd[0], 'ok' if ok else 'SLOWER'))
        print(lines[-1], flush=True)
        counts.append((name, torch_path, device_path))

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    write()                                                          # the times are on disk before the profiler runs
    if not args.no_launch_count:
        for name, torch_path, device_path in counts:
            try:
                lines.append('%-12s device operations per call (kernels + copies, torch profiler): torch %d, device %d'
                             % (name, count_launches(torch_path), count_launches(device_path)))
            except Exception as e:                                   # the count is a side note: the times stand without it
                lines.append('%-12s device operations per call: not measured (%s)' % (name, type(e).__name__))
            print(lines[-1], flush=True)
        write()


if __name__ == '__main__':
    main()
