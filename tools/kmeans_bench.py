"""Time of one Lloyd iteration over atom representations at the reference's scale, and of the dump that produces them.

    python tools/kmeans_bench.py [--n 100000] [--F 700] [--k 6] [--iters 20] [--warmup 3] [--group 2] [--out profiles/kmeans_speed.txt]

 (a) the device path: eagcn_kmeans_iterate (csrc/reps.hip; three launches, every row of X read once);
 (b) the same iteration written with torch ops on the same GPU, what a user would write today: distances (torch.cdist, and the
     expanded form |x|^2 - 2 x.c + |c|^2 with |x|^2 precomputed -- the faster of the two is (b)), argmin, index_add_, bincount, division;
 (c) sklearn.cluster.KMeans(init=..., n_init=1, algorithm='lloyd') on the host, whole fit / n_iter, for the record.
(a) and (b) alternate in one process; a sample is a group of `group` iterations between two HIP events on the stream, from freshly
set initial centroids (so that every timed iteration is a real one: the tool checks n_iter), and the median of `iters` samples per
iteration is reported with p10 .. p90.  The bar is (a) <= (b).  (a) is also given against the time of ONE pass over X from HBM.

The dump: RepBuffers.append per batch (B = 256, N = 132, Concate 5 x 140) against LazyAtomRep.cpu() plus the reference's Python row
loop (train.py:264-268) on the same batch.  Needs the GPU; inputs come from a seed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12         # bytes / s: float4 copy measured on the MI355X, data sheet


def make_X(n, F, k, sep, seed):
    """overlapping blobs (centres `sep` sigma apart per column), so that Lloyd takes many iterations"""
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    cen = torch.randn(k, F, device='cuda', generator=g) * sep
    lab = torch.randint(0, k, (n,), device='cuda', generator=g)
    X = cen[lab] + torch.randn(n, F, device='cuda', generator=g)
    init = X[torch.randperm(n, device='cuda', generator=g)[:k]].clone()
    return X, init


def torch_iter_cdist(X, x2, C):
    lab = torch.cdist(X, C).argmin(1)
    return torch_update(X, C, lab)


def torch_iter_expanded(X, x2, C):
    d = x2[:, None] - 2.0 * (X @ C.t()) + (C * C).sum(1)[None, :]
    return torch_update(X, C, d.argmin(1))


def torch_update(X, C, lab):
    k = C.shape[0]
    sums = torch.zeros_like(C).index_add_(0, lab, X)
    cnt = torch.bincount(lab, minlength=k)
    Cn = torch.where(cnt[:, None] > 0, sums / cnt.clamp_min(1)[:, None].to(sums.dtype), C)
    return Cn, lab, ((Cn - C) ** 2).sum()


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


def bench_kmeans(args, lines):
    from eagcn_amd.analysis import _Problem
    n, F, k, G = args.n, args.F, args.k, args.group
    X, init = make_X(n, F, k, args.sep, args.seed)
    x2 = (X * X).sum(1)
    p = _Problem(X, k)

    def dev_group():
        for _ in range(G):
            p.iterate()

    def torch_group(step):
        def run():
            C = init
            for _ in range(G):
                C, lab, shift = step(X, x2, C)
        return run

    # the paths compute the same iteration: labels after one step from `init`
    p.begin(init, 0.0)
    p.iterate()
    lab_dev = p.labels.clone()
    agree = [float((step(X, x2, init)[1] == lab_dev).float().mean()) for step in (torch_iter_cdist, torch_iter_expanded)]
    cen_dev = p.centers.clone()
    cerr = float((torch_iter_cdist(X, x2, init)[0] - cen_dev).abs().max() / cen_dev.abs().max())
    ta, tb1, tb2 = [], [], []
    for rep in range(args.warmup + args.iters):
        p.begin(init, 0.0)
        torch.cuda.synchronize()
        t = timed(dev_group) / G
        n_iter = p.state_i[1].item()
        if n_iter != G:
            sys.exit('kmeans_bench: the fit converged after %d of %d timed iterations: lower --group or --sep' % (n_iter, G))
        u = timed(torch_group(torch_iter_cdist)) / G
        v = timed(torch_group(torch_iter_expanded)) / G
        if rep >= args.warmup:
            ta.append(t), tb1.append(u), tb2.append(v)
    sa, s1, s2 = stats(ta), stats(tb1), stats(tb2)
    sb, which = (s1, 'cdist') if s1[0] <= s2[0] else (s2, 'expanded')
    one_pass = n * F * 4.0
    lines += ['## one Lloyd iteration, n = %d, F = %d, k = %d (X = %.1f MB); ms per iteration, median [p10 .. p90] min of %d samples'
              % (n, F, k, one_pass / 1e6, args.iters),
              '## of %d iterations each between two HIP events, paths alternating, %d warm-up samples' % (G, args.warmup),
              '(a) device, eagcn_kmeans_iterate        %8.4f [%8.4f .. %8.4f] %8.4f' % sa,
              '(b) torch ops, cdist distances          %8.4f [%8.4f .. %8.4f] %8.4f' % s1,
              '(b) torch ops, expanded distances       %8.4f [%8.4f .. %8.4f] %8.4f' % s2,
              '(b) = the faster torch form (%s): (a) / (b) = %.3f -> %s' % (which, sa[0] / sb[0], 'ok, (a) <= (b)' if sa[0] <= sb[0] else 'SLOWER'),
              'one pass over X from HBM: %.4f ms at %.2f TB/s (measured copy rate), %.4f ms at %.1f TB/s (data sheet); (a) is %.2fx / %.2fx of it'
              % (one_pass / HBM_MEASURED * 1e3, HBM_MEASURED / 1e12, one_pass / HBM_SPEC * 1e3, HBM_SPEC / 1e12,
                 sa[0] / (one_pass / HBM_MEASURED * 1e3), sa[0] / (one_pass / HBM_SPEC * 1e3)),
              'labels after one iteration equal to the device path: cdist %.6f, expanded %.6f of the rows; centroids differ by %.1e of max|C|'
              % (agree[0], agree[1], cerr)]
    for ln in lines[-8:]:
        print(ln, flush=True)
    if not args.no_sklearn:
        try:
            from sklearn.cluster import KMeans
            Xh, ih = X.cpu().numpy(), init.cpu().numpy()
            t0 = time.perf_counter()
            km = KMeans(n_clusters=k, init=ih, n_init=1, algorithm='lloyd', tol=0.0, max_iter=args.sklearn_iters).fit(Xh)
            dt = time.perf_counter() - t0
            lines.append('(c) sklearn KMeans(lloyd) on the host (%d threads): %.1f ms per iteration (whole fit %.2f s / n_iter %d)'
                         % (os.cpu_count() if not os.environ.get('OMP_NUM_THREADS') else int(os.environ['OMP_NUM_THREADS']),
                            dt / km.n_iter_ * 1e3, dt, km.n_iter_))
        except Exception as e:                   # for the record only
            lines.append('(c) sklearn: not measured (%s: %s)' % (type(e).__name__, e))
        print(lines[-1], flush=True)
    return sa[0] <= sb[0]


def bench_gather(args, lines):
    from eagcn_amd import EAGCN
    from eagcn_amd.analysis import RepBuffers
    from eagcn_amd.models import LazyAtomRep
    from eagcn_amd.synthetic import make_batch
    B, N = 256, 132
    torch.manual_seed(0)
    model = EAGCN(28, 24, widths1=[60] * 5, widths2=[70] * 5, n_den1=64, n_den2=32, nclass=12, dropout=0.0, structure='Concate').cuda().eval()
    mb = make_batch(B=B, n_max=N, n_med=16, rel_channels=(28, 4, 2, 2, 2), seed=args.seed)
    subtype = torch.from_numpy(np.random.RandomState(args.seed).randint(0, 21, size=(B, N)))
    index = torch.arange(B, dtype=torch.int64)
    with torch.no_grad():
        _, rep, _ = model(*[t.cuda() for t in mb.dense()])
    packed, pad, layout = rep.packed
    idx = rep._args[0]
    sub_dev, idx_dev = subtype.cuda().to(torch.int32), index.cuda()

    def fresh():
        return LazyAtomRep(idx, layout, packed, pad)

    def append_once():
        buf.append(fresh(), sub_dev, idx_dev)

    def reference_once():
        dense = fresh().cpu()                                  # the padded [B, N, F] tensor on the host, then one Python step per row
        flat, sub, mol = dense.view(-1, dense.shape[2]), subtype.view(-1), index.repeat_interleave(N)
        rows, subs, mols = [], [], []
        for i in range(sub.shape[0]):
            if 1 <= int(sub[i]) <= 18:
                rows.append(flat[i].numpy())
                subs.append(sub[i].numpy())
                mols.append(mol[i:i + 1].numpy())
        return len(rows)

    ta, tr = [], []
    for rep_no in range(args.warmup + args.gather_reps):
        buf = RepBuffers('cuda', cap=B * N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        append_once()
        torch.cuda.synchronize()
        if rep_no >= args.warmup:
            ta.append((time.perf_counter() - t0) * 1e3)
    n_sel = int(buf.count.item())
    for rep_no in range(1 + args.reference_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_ref = reference_once()
        if rep_no >= 1:
            tr.append((time.perf_counter() - t0) * 1e3)
    assert n_ref == n_sel, (n_ref, n_sel)
    sa, sr = stats(ta), stats(tr)
    lines += ['## the dump of one batch, B = %d, N = %d, F = %d (%d atoms selected); ms per batch, host clock around work that ends in a'
              % (B, N, layout.width, n_sel),
              '## device synchronise; median [p10 .. p90] min',
              'RepBuffers.append (eagcn_rep_gather, %d reps)              %9.4f [%9.4f .. %9.4f] %9.4f' % ((args.gather_reps,) + sa),
              'LazyAtomRep.cpu() + the row loop of train.py:264-268 (%d reps) %9.2f [%9.2f .. %9.2f] %9.2f' % ((args.reference_reps,) + sr),
              'ratio %.0fx' % (sr[0] / sa[0])]
    for ln in lines[-5:]:
        print(ln, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--F', type=int, default=700)
    ap.add_argument('--k', type=int, default=6)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--group', type=int, default=2)
    ap.add_argument('--sep', type=float, default=0.05)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--sklearn-iters', type=int, default=10)
    ap.add_argument('--gather-reps', type=int, default=50)
    ap.add_argument('--reference-reps', type=int, default=3)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--no-gather', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('kmeans_bench: needs the GPU (nothing to time without one)')
    lines = ['# tools/kmeans_bench.py %s on %s' % (' '.join(sys.argv[1:]), torch.cuda.get_device_name(0))]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    ok = bench_kmeans(args, lines)
    write()                                                    # the iteration times are on disk before the dump is timed
    if not args.no_gather:
        bench_gather(args, lines)
        write()
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
