"""Device time of one EvalBuffers.agreement() / threshold_metrics() call (csrc/agree.hip: two launches) over filled evaluation buffers,
and beside it, for context, the host time of the scipy / sklearn calls tests/test_gpu_agreement.py holds them against on copies of
the same buffers.  Device time: device events around a run of back-to-back calls after a warm-up, divided by their number (no
accessor, so no copy to the host is in it).  Inputs come from a seed.  Needs the GPU: there is no CPU fallback to time.

    python tools/agreement_bench.py [--out profiles/agreement_speed.txt]

Shapes (rows x tasks): regression -- ESOL (1128 x 1), Lipophilicity (4200 x 1), a large multi-task set (100 000 x 12);
classification -- Tox21 (7831 x 12, 15 % missing labels), HIV (41 000 x 1)."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [('esol', 1128, 1, 'reg', 0.0, 0.0), ('lipo', 4200, 1, 'reg', 0.0, 0.0), ('large', 100000, 12, 'reg', 0.0, 0.0),
          ('tox21', 7831, 12, 'class', 0.07, 0.15), ('hiv', 41000, 1, 'class', 0.035, 0.0)]


def make_buffers(rows, T, task, pos, missing, seed):
    from eagcn_amd.training import EvalBuffers
    rng = np.random.RandomState(seed)
    buf = EvalBuffers(T, task == 'class', torch.device('cuda'), cap=rows)
    if task == 'class':
        u = rng.rand(rows, T)
        y = np.where(u < missing, -1.0, np.where(u < missing + pos * (1.0 - missing), 1.0, 0.0)).astype(np.float32)
        s = (1.0 / (1.0 + np.exp(-(rng.randn(rows, T) + 1.5 * (y == 1))))).astype(np.float32)
        valid = (y != -1)
    else:
        y = rng.randn(rows, T).astype(np.float32)
        s = (y + 0.5 * rng.randn(rows, T)).astype(np.float32)
        valid = np.ones((rows, T), dtype=bool)
    buf.scores[:rows], buf.targets[:rows] = torch.from_numpy(s).cuda(), torch.from_numpy(y).cuda()
    buf.valid[:rows] = torch.from_numpy(valid).cuda().to(torch.uint8)
    buf.rows = rows
    return buf, s, y, valid


def host_reference(task, s, y, valid):
    """the calls of tests/test_gpu_agreement.py, per task over the valid entries on fp64 copies; returns something to compare"""
    from scipy import stats
    from sklearn import metrics
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for t in range(s.shape[1]):
            m = valid[:, t]
            sd, yd = s[m, t].astype(np.float64), y[m, t].astype(np.float64)
            if task == 'reg':
                out.append((metrics.r2_score(yd, sd), stats.pearsonr(sd, yd)[0], stats.spearmanr(sd, yd)[0], stats.kendalltau(sd, yd)[0]))
            else:
                yi, pred = yd.astype(np.int64), (s[m, t] > np.float32(0.5)).astype(np.int64)
                metrics.confusion_matrix(yi, pred, labels=[0, 1])
                metrics.accuracy_score(yi, pred), metrics.precision_score(yi, pred), metrics.recall_score(yi, pred)
                out.append((metrics.log_loss(yi, sd, labels=[0, 1]), metrics.brier_score_loss(yi, sd), metrics.f1_score(yi, pred),
                            metrics.matthews_corrcoef(yi, pred)))
    return np.array(out).T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('agreement_bench: needs the GPU (nothing to time without one)')
    from eagcn_amd import _lib
    lib = _lib.load()
    lines = ['# device ms of ONE call (two launches, no host copy) on %s: device events around `calls` back-to-back calls after a warm-up,'
             % torch.cuda.get_device_name(0),
             '# median of 5 such runs [min .. max]; host ms: one pass of the scipy / sklearn calls of tests/test_gpu_agreement.py over all',
             '# tasks on the same host (median of 3); splits = workgroups that share a tile\'s rows in the pair kernel (regression only)',
             '%-6s %-6s %7s %3s %6s %6s | %-32s | %10s | %s' % ('shape', 'call', 'rows', 'T', 'splits', 'calls', 'device ms per call', 'host ms',
                                                             'max |device - host|')]
    for name, rows, T, task, pos, missing in SHAPES:
        buf, s, y, valid = make_buffers(rows, T, task, pos, missing, args.seed)
        call = buf.agreement if task == 'reg' else buf.threshold_metrics
        res = call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        once = time.perf_counter() - t0
        calls = int(min(200, max(3, 0.25 / max(once, 1e-5))))         # a quarter of a second of device work per run, at least 3 calls
        runs = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                call()
            b.record()
            b.synchronize()
            runs.append(a.elapsed_time(b) / calls)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = host_reference(task, s, y, valid)
            host.append((time.perf_counter() - t0) * 1e3)
        v = res.values.cpu().numpy()
        got = v[:4 * T].reshape(4, T) if task == 'reg' else v[:11 * T].reshape(11, T)[[0, 1, 9, 10]]
        lines.append('%-6s %-6s %7d %3d %6s %6d | %9.4f [%9.4f .. %9.4f] | %10.2f | %.1e'
                     % (name, 'agree' if task == 'reg' else 'thresh', rows, T,
                        lib.eagcn_eval_agreement_splits(rows, T) if task == 'reg' else '-', calls, float(np.median(runs)), min(runs), max(runs),
                        float(np.median(host)), float(np.abs(got - want).max())))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
