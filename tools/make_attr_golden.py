#!/usr/bin/env python3
"""Generate the attribution vectors tests/golden/attr_*.npz by running the UNMODIFIED reference.

Same setup as tools/make_golden.py (whose parameter initialisation and batch packing it reuses): the reference's
``models.py`` imports as-is behind an empty ``utils`` stub; only data is written.

    python tools/make_attr_golden.py            # rewrites tests/golden/attr_*.npz

Each .npz holds what a model_* vector holds for the forward (meta, batch/*, sd/*, out/*), plus
    gout                 [B, nclass] the cotangent of the attributed scalar sum(out * gout)
    grad/afm             d sum(out * gout) / d afm            (the reference's autograd, afm.requires_grad_(), models.py:96)
    ig8/attr, ig8/score  integrated gradients against a zero baseline, midpoint rule over m = 8 points
                         (alpha_s = (s + 1/2) / 8, one reference forward + autograd per point), eval cases only
The ``attr_`` prefix keeps them out of golden_cases('model' | 'layer').
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg   # noqa: E402  (imports the reference read-only and seeds nothing)

from eagcn_amd.synthetic import make_batch   # noqa: E402

IG_STEPS = 8


def attr_case(name, structure, training, batch_kw, widths1, widths2, dens, nclass, n_bfeat, seed):
    gen = torch.Generator().manual_seed(3000 + seed)
    mb = make_batch(rel_channels=(n_bfeat, 4, 2, 2, 2), seed=seed, n_tasks=nclass, task='reg', **batch_kw)
    adj, afm, r1, r2, r3, r4, r5, size = mb.dense()
    model = mg.ref_models.EAGCN(n_bfeat, 24, *widths1, *widths2, dens[0], dens[1], nclass, 0.0,
                                structure=structure, molfp_mode='sum')
    mg.init_like_train(model, gen)
    data = {}
    data.update(mg.pack_batch(mb))
    data.update(mg.sd_np(model.state_dict(), 'sd/'))
    model.train(training)
    x = afm.clone().requires_grad_(True)
    out, _, graph_rep = model(adj, x, r1, r2, r3, r4, r5, size)
    g = torch.randn(out.shape, generator=gen)
    data['gout'] = g.numpy()
    data['out/out'] = out.detach().numpy().copy()
    (out * g).sum().backward()
    data['grad/afm'] = x.grad.numpy().copy()
    if not training:
        acc = torch.zeros_like(afm)
        for s in range(IG_STEPS):
            xa = ((s + 0.5) / IG_STEPS * afm).requires_grad_(True)
            o, _, _ = model(adj, xa, r1, r2, r3, r4, r5, size)
            (o * g).sum().backward()
            acc += xa.grad / IG_STEPS
        attr = afm * acc
        data['ig8/attr'] = attr.numpy().copy()
        data['ig8/score'] = attr.sum(-1).numpy().copy()
    meta = dict(kind='attr', name=name, structure=structure, molfp='sum', training=training, widths1=list(widths1),
                widths2=list(widths2), dens=list(dens), nclass=nclass, n_bfeat=n_bfeat, n_afeat=24, ig_steps=IG_STEPS,
                torch=torch.__version__)
    data['meta'] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(mg.OUT, name + '.npz'), **data)
    print('wrote', name)


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    small = dict(B=6, n_max=12, n_med=6)
    w1, w2 = (8, 6, 4, 4, 5), (10, 7, 5, 6, 4)
    ws1, ws2 = (3, 2, 2, 2, 3), (4, 3, 2, 2, 3)
    attr_case('attr_concate_eval', 'Concate', False, small, w1, w2, (16, 8), 3, 7, seed=41)
    attr_case('attr_concate_train', 'Concate', True, small, w1, w2, (16, 8), 3, 7, seed=42)
    attr_case('attr_weighted_eval', 'Weighted_sum', False, small, ws1, ws2, (16, 8), 2, 5, seed=43)
    attr_case('attr_weighted_train', 'Weighted_sum', True, small, ws1, ws2, (16, 8), 2, 5, seed=44)
    attr_case('attr_gcn_eval', 'GCN', False, small, w1, w2, (16, 8), 2, 7, seed=45)
    attr_case('attr_gcn_train', 'GCN', True, small, w1, w2, (16, 8), 3, 7, seed=46)
    attr_case('attr_concate_isolated_eval', 'Concate', False, dict(B=6, n_max=12, n_med=6, isolated_frac=0.2), w1, w2, (16, 8),
              3, 7, seed=47)


if __name__ == '__main__':
    main()
