"""CPU checks of the atom-attribution feature: the oracle reproduces the reference's attribution vectors (tests/golden/attr_*),
the new C-ABI symbols are exported and refuse bad arguments without touching a GPU, and the quadrature is the midpoint rule the
header states."""
import ctypes as C

import pytest
import torch

from helpers import Golden, build_oracle_model, golden_cases, rel_err

ATTR_CASES = golden_cases('attr')
NEW_SYMBOLS = ('eagcn_model_input_scratch_bytes', 'eagcn_model_backward_input', 'eagcn_attr_alpha', 'eagcn_attr_weight',
               'eagcn_attr_acc_elems', 'eagcn_attr_pack_input', 'eagcn_attr_step', 'eagcn_attr_finalize')


def _oracle(g):
    ref = build_oracle_model(g.meta)
    ref.load_state_dict(g.state_dict(), strict=True)
    ref.train(g.meta['training'])
    return ref


def _afm_grad(ref, dense, x, gout):
    adj, rels, size = dense[0], dense[2:-1], dense[-1]
    x = x.clone().requires_grad_(True)
    out, _, _ = ref(adj, x, *rels, size)
    g, = torch.autograd.grad((out * gout).sum(), x)
    return g


def test_attr_cases_present():
    assert len(ATTR_CASES) >= 7, ATTR_CASES
    structs = {Golden(n).meta['structure'] for n in ATTR_CASES}
    assert structs == {'Concate', 'Weighted_sum', 'GCN'}


@pytest.mark.parametrize('name', ATTR_CASES)
def test_oracle_reproduces_attr_golden(name):
    g = Golden(name)
    ref = _oracle(g)
    dense = g.batch.dense()
    gout = torch.from_numpy(g.z['gout'])
    grad = _afm_grad(ref, dense, dense[1], gout)
    assert rel_err(grad, g.z['grad/afm'], 'grad/afm') < 1e-5
    if 'ig8/attr' in g.z.files:
        m = g.meta['ig_steps']
        x = dense[1]
        acc = torch.zeros_like(x)
        for s in range(m):
            acc += _afm_grad(ref, dense, (s + 0.5) / m * x, gout) / m
        attr = x * acc
        assert rel_err(attr, g.z['ig8/attr'], 'ig8/attr') < 1e-5
        assert rel_err(attr.sum(-1), g.z['ig8/score'], 'ig8/score') < 1e-5


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from eagcn_amd import _lib
    return _lib, _lib.load()


def test_attr_symbols_exported():
    L, lib = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert lib.eagcn_abi_version() == 8


def test_backward_input_argument_checks_without_gpu():
    L, lib = _lib()
    b, m = L.Batch(), L.Model()
    lg = (L.LayerGrads * 4)()
    hg = L.HeadGrads()
    dummy = C.c_void_p(16)
    args = lambda lgp, hgp, dafm: (C.byref(b), C.byref(m), None, dummy, 1, dummy, 1, dummy, None, lgp, hgp, dafm, None)
    # a NULL dafm
    assert lib.eagcn_model_backward_input(*args(None, None, None)) != 0
    assert b'dafm' in lib.eagcn_last_error()
    # exactly one of lg / hg
    assert lib.eagcn_model_backward_input(*args(lg, None, dummy)) != 0
    assert b'lg and hg' in lib.eagcn_last_error()
    assert lib.eagcn_model_backward_input(*args(None, C.byref(hg), dummy)) != 0
    # a model the engine does not run (no layers: the structure checks reject it before any HIP call)
    assert lib.eagcn_model_backward_input(*args(None, None, dummy)) != 0
    # the IG entry points
    assert lib.eagcn_attr_step(C.byref(b), C.byref(m), None, dummy, 1, dummy, 1, dummy, None, 1.0, 1, None, None) != 0
    assert lib.eagcn_attr_finalize(C.byref(b), C.byref(m), None, None, dummy, dummy, dummy, None) != 0
    assert lib.eagcn_attr_pack_input(None, C.byref(m), dummy, None, 0.5, dummy, 1, None) != 0


@pytest.mark.parametrize('steps', [1, 2, 8, 32, 64])
def test_midpoint_weights(steps):
    _, lib = _lib()
    for s in range(steps):
        assert lib.eagcn_attr_alpha(s, steps) == pytest.approx((s + 0.5) / steps, rel=1e-7)
    assert lib.eagcn_attr_weight(steps) == pytest.approx(1.0 / steps, rel=1e-7)
    assert sum(lib.eagcn_attr_weight(steps) for _ in range(steps)) == pytest.approx(1.0, rel=1e-6)


def test_input_only_aggregation_budget_within_edge_forms(tmp_path):
    """The edge-free transposed aggregation (lagg_in.hip) spends no more registers or LDS than the edge-gradient forms of lagg.hip,
    and spills nothing (three workgroups per CU either way)."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not found')
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'eagcn_amd', 'csrc')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-munsafe-fp-atomics', '-S',
             '--cuda-device-only']

    def kernels(name):
        out = str(tmp_path / (name + '.s'))
        r = subprocess.run([hipcc] + flags + ['-o', out, os.path.join(csrc, name + '.hip')], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        res = {}
        for m in re.finditer(r'- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)', open(out).read(), re.S):
            blk = m.group(0)
            nm = re.search(r'\.name:\s+(\S+)', blk).group(1)
            if 'lagg_kernel' in nm:
                res[nm] = tuple(int(re.search(r'\.%s:\s+(\d+)' % f, blk).group(1))
                                for f in ('private_segment_fixed_size', 'vgpr_count', 'group_segment_fixed_size'))
        return res
    edge, noedge = kernels('lagg'), kernels('lagg_in')
    assert len(noedge) == 4, noedge
    trans_edge = {n: v for n, v in edge.items() if n.startswith('_ZN5eagcn11lagg_kernelILb1E')}
    vmax, lmax = max(v[1] for v in trans_edge.values()), max(v[2] for v in trans_edge.values())
    for name, (scratch, vgpr, lds) in noedge.items():
        assert scratch == 0 and vgpr <= vmax and lds <= lmax, (name, scratch, vgpr, lds, vmax, lmax)
