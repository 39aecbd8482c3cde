"""Time of one exact t-SNE iteration on the device, and of the one-off stages around it (distances, affinities, PCA).

    python tools/embed_bench.py [--n 16384 4096] [--F 700] [--iters 20] [--warmup 3] [--group 4] [--host-n 2000] [--pca-n 100000]
                                [--out profiles/tsne_speed.txt]

 (a) the device path: eagcn_tsne_iterate (csrc/embed.hip; every element of P read once per iteration);
 (b) the same iteration written with torch ops on the same GPU, what a user would write today: torch.cdist of the embedding, n x n
     temporaries for w, the two weighted sums as matrix-vector products, the update rule element-wise;
 (c) sklearn.manifold.TSNE, method='exact' and 'barnes_hut', on the host at --host-n points (whole fit / iterations), for the record.
(a) and (b) alternate in one process; a sample is a group of `group` iterations between two HIP events on the stream, and the median
of `iters` samples per iteration is reported with p10 .. p90.  The bar is (a) <= (b).  (a) is also given as a share of the read-once
floor 4 n^2 bytes / 6.3 TB/s: that is the HBM floor -- at n = 4096 P (67 MB) stays in the Infinity Cache and the floor does not apply.
Needs the GPU; inputs come from a seed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED = 6.29e12                           # bytes / s: float4 copy measured on the MI355X


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)               # ms


def stats(ts):
    a = np.sort(np.array(ts))
    return float(np.median(a)), float(a[len(a) // 10]), float(a[(9 * len(a)) // 10]), float(a[0])


def make_X(n, F, seed, blobs=8):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    cen = torch.randn(blobs, F, device='cuda', generator=g) * 2.0
    return cen[torch.randint(0, blobs, (n,), device='cuda', generator=g)] + torch.randn(n, F, device='cuda', generator=g)


def torch_iteration(P, Y, U, G, alpha, momentum, lr):
    """one iteration with torch ops: n x n temporaries, the gradient as 4 ((aP - Q) w) (y_i - y_j) summed over j"""
    w = 1.0 / (1.0 + torch.cdist(Y, Y) ** 2)
    w.fill_diagonal_(0.0)
    Z = w.sum(dtype=torch.float64).to(torch.float32)
    t = (alpha * P - w / Z) * w
    grad = 4.0 * (t.sum(1, keepdim=True) * Y - t @ Y)
    inc = U * grad < 0
    G = torch.where(inc, G + 0.2, G * 0.8).clamp_min_(0.01)
    U = momentum * U - lr * (grad * G)
    return Y + U, U, G, grad


def bench_iteration(args, n, lines):
    from eagcn_amd.analysis import _TSNEProblem, sqdist
    X = make_X(n, args.F, args.seed)
    G = args.group
    p = _TSNEProblem(n, 'cuda')
    t_dist = [timed(lambda: sqdist(X)) for _ in range(3)]
    D = sqdist(X)
    t_aff = [timed(lambda: p.affinities(D, 30.0)) for _ in range(3)]
    del D
    g = torch.Generator(device='cuda')
    g.manual_seed(args.seed)
    Y0 = 1e-4 * torch.randn((n, 2), device='cuda', generator=g)
    lr = max(n / 12.0 / 4.0, 50.0)
    Pn = p.P[:, :n].contiguous() if p.ldp != n else p.P

    def dev_group():
        for _ in range(G):
            p.iterate()

    def torch_group():
        Y, U, Gn = Y0, torch.zeros_like(Y0), torch.ones_like(Y0)
        for _ in range(G):
            Y, U, Gn, _g = torch_iteration(Pn, Y, U, Gn, 12.0, 0.5, lr)
        return Y

    # the two paths compute the same iteration: the embedding after `group` steps from Y0
    p.begin(Y0, 12.0, lr, 1000, 300, 1e-7)
    dev_group()
    diff = float((torch_group() - p.Y).abs().max() / p.Y.abs().max())
    ta, tb = [], []
    for rep in range(args.warmup + args.iters):
        p.begin(Y0, 12.0, lr, 1000, 300, 1e-7)
        torch.cuda.synchronize()
        t = timed(dev_group) / G
        if p.state_i[1].item() != G:
            sys.exit('embed_bench: %d of %d timed iterations ran' % (p.state_i[1].item(), G))
        u = timed(torch_group) / G
        if rep >= args.warmup:
            ta.append(t), tb.append(u)
    sa, sb = stats(ta), stats(tb)
    floor = 4.0 * n * n / HBM_MEASURED * 1e3
    lines += ['## one t-SNE iteration, n = %d (P = %.0f MB); ms per iteration, median [p10 .. p90] min of %d samples of %d iterations each'
              % (n, 4.0 * n * p.ldp / 1e6, args.iters, G),
              '## between two HIP events, paths alternating, %d warm-up samples' % args.warmup,
              '(a) device, eagcn_tsne_iterate          %8.4f [%8.4f .. %8.4f] %8.4f' % sa,
              '(b) torch ops (cdist, n x n temporaries) %8.4f [%8.4f .. %8.4f] %8.4f' % sb,
              '(a) / (b) = %.3f -> %s' % (sa[0] / sb[0], 'ok, (a) <= (b)' if sa[0] <= sb[0] else 'SLOWER'),
              'read-once floor 4 n^2 / %.2f TB/s = %.4f ms: (a) runs at %.0f %% of it (the HBM floor; %s)'
              % (HBM_MEASURED / 1e12, floor, 100.0 * floor / sa[0],
                 'P is past the Infinity Cache' if 4.0 * n * n > 256e6 else 'it does not apply here: P stays in the Infinity Cache'),
              'embedding after %d iterations: the paths differ by %.1e of max|Y|' % (G, diff),
              'one-off: distances at F = %d %.3f ms, affinities (perplexity 30) %.3f ms (best of 3)' % (args.F, min(t_dist), min(t_aff))]
    for ln in lines[-8:]:
        print(ln, flush=True)
    return sa[0] <= sb[0]


def bench_pca(args, lines):
    from eagcn_amd.analysis import pca, pca_cov
    X = make_X(args.pca_n, args.F, args.seed)
    tc = [timed(lambda: pca_cov(X)) for _ in range(4)][1:]
    t0 = time.perf_counter()
    pca(X, 2)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) * 1e3
    lines += ['## PCA, %d x %d' % (args.pca_n, args.F),
              'means and covariance on the device %.3f ms (best of 3); whole pca(X, 2) with the host eigh %.1f ms' % (min(tc), whole)]
    for ln in lines[-2:]:
        print(ln, flush=True)


def bench_host(args, lines):
    try:
        from sklearn.manifold import TSNE
        Xh = make_X(args.host_n, args.F, args.seed).cpu().numpy()
        for method in ('exact', 'barnes_hut'):
            t0 = time.perf_counter()
            m = TSNE(method=method, init='random', random_state=0, max_iter=args.host_iters).fit(Xh)
            dt = time.perf_counter() - t0
            lines.append('(c) sklearn TSNE(%s) on the host, n = %d: %.1f ms per iteration (whole fit %.2f s / %d iterations, affinities included)'
                         % (method, args.host_n, dt / (m.n_iter_ + 1) * 1e3, dt, m.n_iter_ + 1))
            print(lines[-1], flush=True)
    except Exception as e:                       # for the record only
        lines.append('(c) sklearn: not measured (%s: %s)' % (type(e).__name__, e))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, nargs='+', default=[16384, 4096])
    ap.add_argument('--F', type=int, default=700)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--group', type=int, default=4)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--host-n', type=int, default=2000)
    ap.add_argument('--host-iters', type=int, default=250)
    ap.add_argument('--pca-n', type=int, default=100000)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('embed_bench: needs the GPU (nothing to time without one)')
    lines = ['# tools/embed_bench.py %s on %s' % (' '.join(sys.argv[1:]), torch.cuda.get_device_name(0))]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    ok = True
    for n in args.n:
        ok = bench_iteration(args, n, lines) and ok
        write()
        torch.cuda.empty_cache()
    bench_pca(args, lines)
    write()
    if not args.no_sklearn:
        bench_host(args, lines)
        write()
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
