"""Time of the exact nearest-neighbour search on the device (csrc/knn.hip, analysis.knn) against the only route a user had before it,
and of the trustworthiness built on it.

    python tools/knn_speed.py [--reps 5] [--warmup 1] [--torch-budget 40] [--out profiles/knn_speed.txt]

 (a) analysis.knn at (queries m, rows n, F, k) = self-joins (32768, 700, 16), (100000, 700, 16), (100000, 2, 90) and 4096 queries against
     (100000, 700, 16);
 (b) the torch route in the same process: torch.cdist(Q[chunk], X, compute_mode='donot_use_mm_for_euclid_dist') + torch.topk(k, largest=False) (a
     self-join sets the row's own column to inf first), the query rows in chunks of at most 2^24 / n rows: that cdist kernel is launched with one workgroup of 256
     threads per pair, and a launch of 2^32 threads or more is refused (the whole 100000 x 100000 block would be 40 GB besides).  Where a
     whole pass would take longer than --torch-budget seconds, the first chunks are timed and the pass is extrapolated
     from them, and the line says so.
A sample is one call between two HIP events on the stream; after the warm-up calls the median of the samples is reported with the least
and the largest.  The arithmetic rate is 3 n m F / t (a subtraction and a fused multiply-add per pair and column), set beside the chip's
fp32 vector peak.  The expectation: (a) <= (b) at every shape.  Also: trustworthiness(X, pca(X, 2).embedding, 5) at 32768 x 700, whole
call with its one host read, host clock.  Needs the GPU; inputs come from a seed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32 = 157.3e12                             # FLOP / s, fp32 vector peak of the MI355X (data sheet)
SHAPES = [(32768, 32768, 700, 16, True), (100000, 100000, 700, 16, True), (100000, 100000, 2, 90, True), (4096, 100000, 700, 16, False)]


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


def make_X(n, F, seed, blobs=8):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    cen = torch.randn(blobs, F, device='cuda', generator=g) * 2.0
    return cen[torch.randint(0, blobs, (n,), device='cuda', generator=g)] + torch.randn(n, F, device='cuda', generator=g)


def torch_chunk(Q, X, k, lo, hi, self_join):
    d = torch.cdist(Q[lo:hi], X, compute_mode='donot_use_mm_for_euclid_dist')
    if self_join:
        d[torch.arange(hi - lo, device=d.device), torch.arange(lo, hi, device=d.device)] = float('inf')
    return torch.topk(d, k, dim=1, largest=False)


def torch_route(Q, X, k, chunk, self_join, upto=None):
    idx = []
    for lo in range(0, Q.shape[0] if upto is None else min(upto, Q.shape[0]), chunk):
        idx.append(torch_chunk(Q, X, k, lo, min(lo + chunk, Q.shape[0]), self_join).indices)
    return torch.cat(idx)


def bench(args, m, n, F, k, self_join, lines):
    from eagcn_amd.analysis import knn, knn_slabs
    X = make_X(n, F, args.seed)
    Q = X if self_join else make_X(m, F, args.seed + 1)
    chunk = max(64, min(m, ((1 << 24) - 1) // n // 64 * 64))

    def dev():
        return knn(X, k) if self_join else knn(X, k, queries=Q)

    ta = []
    for rep in range(args.warmup + args.reps):
        t, res = timed(dev)
        if rep >= args.warmup:
            ta.append(t)
    t1, _ = timed(lambda: torch_route(Q, X, k, chunk, self_join, upto=chunk))            # warm-up of the torch route: one chunk
    t1, _ = timed(lambda: torch_route(Q, X, k, chunk, self_join, upto=chunk))
    nchunks = -(-m // chunk)
    whole = t1 * nchunks / 1e3 <= args.torch_budget
    tb, note = [], ''
    if whole:
        for rep in range(max(2, args.reps // 2)):
            t, ref = timed(lambda: torch_route(Q, X, k, chunk, self_join))
            tb.append(t)
        rows = m
    else:
        take = max(1, min(nchunks, int(args.torch_budget * 1e3 / 3 / t1)))
        for rep in range(3):
            t, ref = timed(lambda: torch_route(Q, X, k, chunk, self_join, upto=take * chunk))
            tb.append(t * m / min(m, take * chunk))
        rows = min(m, take * chunk)
        note = ' (EXTRAPOLATED from the first %d of %d chunks)' % (take, nchunks)
    same = float((torch.sort(res.indices[:rows].long(), dim=1).values == torch.sort(ref, dim=1).values).all(dim=1).double().mean())
    sa, sb = stats(ta), stats(tb)
    flop = 3.0 * n * m * F
    ok = sa[0] <= sb[0]
    lines += ['## %s m = %d, n = %d, F = %d, k = %d (slabs %d; torch chunks of %d query rows = %.0f MB of distances)%s'
              % ('self-join' if self_join else 'queries', m, n, F, k, knn_slabs(n, m), chunk, 4.0 * chunk * n / 1e6, note),
              '(a) device, analysis.knn       %10.2f ms [%10.2f .. %10.2f]   %6.2f TFLOP/s = %4.1f %% of the fp32 vector peak'
              % (sa + (flop / sa[0] / 1e9, 100.0 * flop / sa[0] * 1e3 / PEAK_FP32)),
              '(b) torch cdist + topk         %10.2f ms [%10.2f .. %10.2f]   %6.2f TFLOP/s' % (sb + (flop / sb[0] / 1e9,)),
              '(a) / (b) = %.3f -> %s; neighbour sets equal on %.4f of the %d compared rows' % (sa[0] / sb[0], 'ok, (a) <= (b)' if ok else 'SLOWER',
                                                                                             same, rows)]
    for ln in lines[-4:]:
        print(ln, flush=True)
    return ok


def bench_trust(args, lines):
    from eagcn_amd.analysis import knn, neighbor_ranks, pca, trustworthiness
    n, F, k = 32768, 700, 5
    X = make_X(n, F, args.seed)
    Y = pca(X, 2).embedding
    ts = []
    for rep in range(args.warmup + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T = trustworthiness(X, Y, k)
        ts.append((time.perf_counter() - t0) * 1e3)
    nb = knn(Y, k).indices
    t_knn = min(timed(lambda: knn(Y, k))[0] for _ in range(3))
    t_rank = min(timed(lambda: neighbor_ranks(X, nb))[0] for _ in range(3))
    lines += ['## trustworthiness(X, pca(X, 2).embedding, %d), X %d x %d: T = %.6f' % (k, n, F, T),
              'whole call with its host read %.2f ms (least of 3, host clock); knn of the embedding %.2f ms, ranks in X %.2f ms = %.2f TFLOP/s'
              % (min(ts[args.warmup:]), t_knn, t_rank, 3.0 * n * n * F / t_rank / 1e9)]
    for ln in lines[-2:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--torch-budget', type=float, default=40.0)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('knn_speed: needs the GPU (nothing to time without one)')
    lines = ['# tools/knn_speed.py %s on %s' % (' '.join(sys.argv[1:]), torch.cuda.get_device_name(0)),
             '# ms per call: median [least .. largest] of the samples, one call between two HIP events, %d warm-up call(s); rate = 3 n m F / t'
             % args.warmup]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    ok = True
    for m, n, F, k, self_join in SHAPES:
        ok = bench(args, m, n, F, k, self_join, lines) and ok
        write()
        torch.cuda.empty_cache()
    bench_trust(args, lines)
    lines.append('# every shape (a) <= (b): %s' % ('yes' if ok else 'NO'))
    write()
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
