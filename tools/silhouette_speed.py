"""Time of the silhouette coefficients on the device (csrc/silhouette.hip, analysis.silhouette_samples) beside the nearest-neighbour
self-join on the same rows -- existing code with the same distance front end -- and against the route a user had before it.

    python tools/silhouette_speed.py [--reps 5] [--warmup 1] [--limit 120] [--out profiles/silhouette_speed.txt]

 (a) analysis.silhouette_samples at (rows n, F, k) = (32768, 700, 18), (100000, 700, 18) and (100000, 2, 18);
 (b) analysis.knn(X, 16) on the same rows;
 (c) at 32768 rows the torch route in the same process: analysis.sqdist + torch.sqrt (n x n floats), per cluster the fp64 sum of the
     masked columns, then a, b and s in torch.
A sample is one call between two HIP events on the stream; after the warm-up calls the median of the samples is reported with the least
and the largest.  The arithmetic rate is 3 n^2 F / t as in tools/knn_speed.py.  The expectations: (a) <= 1.1 (b) at F = 700, and
(a) <= (c).  Every shape is measured by a child process of its own under a time limit (--limit seconds); after a child that fails or
runs out of time nothing more is started.  Needs the GPU; inputs come from a seed."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32 = 157.3e12                             # FLOP / s, fp32 vector peak of the MI355X (data sheet)
SHAPES = [(32768, 700, 18, True), (100000, 700, 18, False), (100000, 2, 18, False)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out              # ms


def stats(ts):
    a = np.sort(np.array(ts))
    return float(np.median(a)), float(a[0]), float(a[-1])


def make_X(n, F, k, seed):
    """k Gaussian blobs; the labels are the blobs, rows interleaved"""
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    cen = torch.randn(k, F, device='cuda', generator=g) * 2.0
    lab = torch.randint(0, k, (n,), device='cuda', generator=g)
    return cen[lab] + torch.randn(n, F, device='cuda', generator=g), lab


def torch_route(X, lab, k):
    from eagcn_amd.analysis import sqdist
    R = torch.sqrt(sqdist(X))
    S = torch.stack([R[:, lab == c].sum(dim=1, dtype=torch.float64) for c in range(k)], dim=1)
    cnt = torch.bincount(lab, minlength=k).double()
    own = torch.nn.functional.one_hot(lab, k).bool()
    a = S[own] / (cnt[lab] - 1)
    b = torch.where(own | (cnt == 0).unsqueeze(0), torch.full_like(S, float('inf')), S / cnt.unsqueeze(0)).min(dim=1).values
    s = torch.nan_to_num((b - a) / torch.maximum(a, b), nan=0.0)
    return torch.where(cnt[lab] == 1, torch.zeros_like(s), s)


def measure(fn, args):
    ts = []
    for rep in range(args.warmup + args.reps):
        t, out = timed(fn)
        if rep >= args.warmup:
            ts.append(t)
    return stats(ts), out


def step(args, n, F, k, with_torch):
    from eagcn_amd.analysis import knn, knn_slabs, silhouette_samples, silhouette_slabs
    X, lab = make_X(n, F, k, args.seed)
    sa, res = measure(lambda: silhouette_samples(X, lab, k), args)
    sb, _ = measure(lambda: knn(X, 16), args)
    flop = 3.0 * n * n * F
    lines = ['## n = %d, F = %d, k = %d (silhouette slabs %d, knn slabs %d); mean sample %.6f'
             % (n, F, k, silhouette_slabs(n, k), knn_slabs(n, n), float(res.score)),
             '(a) analysis.silhouette_samples  %10.2f ms [%10.2f .. %10.2f]   %6.2f TFLOP/s = %4.1f %% of the fp32 vector peak'
             % (sa + (flop / sa[0] / 1e9, 100.0 * flop / sa[0] * 1e3 / PEAK_FP32)),
             '(b) analysis.knn(X, 16)          %10.2f ms [%10.2f .. %10.2f]   %6.2f TFLOP/s' % (sb + (flop / sb[0] / 1e9,)),
             '(a) / (b) = %.3f%s' % (sa[0] / sb[0], (' -> ok, (a) <= 1.1 (b)' if sa[0] <= 1.1 * sb[0] else ' -> ABOVE 1.1') if F == 700 else '')]
    ok = True
    if with_torch:
        args_t = argparse.Namespace(warmup=1, reps=max(2, args.reps // 2))
        sc, ref = measure(lambda: torch_route(X, lab, k), args_t)
        ok = sa[0] <= sc[0]
        lines += ['(c) torch: sqdist, sqrt, masked sums %7.2f ms [%10.2f .. %10.2f]; worst |sample (a) - sample (c)| = %.3e'
                  % (sc + (float((res.samples - ref).abs().max()),)),
                  '(a) / (c) = %.3f -> %s' % (sa[0] / sc[0], 'ok, (a) <= (c)' if ok else 'SLOWER')]
    print('\n'.join(lines), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--step', type=int, default=None, help='(internal) measure shape number STEP in this process')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('silhouette_speed: needs the GPU (nothing to time without one)')
    if args.step is not None:
        sys.exit(0 if step(args, *SHAPES[args.step]) else 1)
    lines = ['# tools/silhouette_speed.py %s on %s' % (' '.join(sys.argv[1:]), torch.cuda.get_device_name(0)),
             '# ms per call: median [least .. largest] of the samples, one call between two HIP events, %d warm-up call(s); rate = 3 n^2 F / t'
             % args.warmup]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    ok = True
    for i in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', str(i), '--reps', str(args.reps), '--warmup', str(args.warmup),
               '--seed', str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            lines.append('# shape %d: no result within %.0f s; stopped here' % (i, args.limit))
            write()
            sys.exit(2)
        lines += r.stdout.strip().split('\n') if r.stdout.strip() else []
        print(r.stdout, end='', flush=True)
        if r.returncode not in (0, 1):
            lines.append('# shape %d: exit status %d; stopped here\n%s' % (i, r.returncode, r.stderr[-2000:]))
            write()
            sys.exit(2)
        ok = ok and r.returncode == 0
        write()
    lines.append('# (a) <= (c) where (c) was measured: %s' % ('yes' if ok else 'NO'))
    write()
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
