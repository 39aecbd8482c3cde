"""CPU checks of the bond-attribution feature (csrc/battr.hip, EAGCN.bond_attributions): the closed form the kernel implements
(tests/bond_attr_reference.py) equals the oracle's autograd in float64, the two new C-ABI symbols are exported and refuse bad
arguments without touching a GPU, and the kernel's code objects carry no scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from bond_attr_reference import autograd_scores, formula_scores, target_weights
from helpers import Golden, build_oracle_model

NEW_SYMBOLS = ('eagcn_layer_bond_grad', 'eagcn_bond_attr_finalize')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle64(name):
    g = Golden(name)
    ref = build_oracle_model(g.meta)
    ref.load_state_dict(g.state_dict(), strict=True)
    for k in range(5):                                   # attention logits of O(1): sigmoid' and z must matter
        for l in range(1, 5):
            blk = getattr(getattr(ref, 'layer%d' % l), 'block%d' % (k + 1), None)
            if blk is not None:
                blk.att.weight.data.normal_(0.0, 0.8, generator=torch.Generator().manual_seed(10 * l + k))
    return g, ref.double().eval()


# (the GCN baseline has no relation input: attention mode only)
FORMULA_CASES = [(n, m) for n in ('model_concate_eval', 'model_weighted_eval', 'model_gcn_eval', 'model_concate_isolated')
                 for m in ('attention', 'relation') if not (n == 'model_gcn_eval' and m == 'relation')]


@pytest.mark.parametrize('name,mode', FORMULA_CASES)
def test_closed_form_equals_oracle_autograd_float64(name, mode):
    g, ref = _oracle64(name)
    dense = g.batch.dense()
    B, nclass = g.batch.B, g.meta['nclass']
    for target in (1, torch.randn(B, nclass, generator=torch.Generator().manual_seed(5))):
        dout = target_weights(B, nclass, target)
        truth = autograd_scores(ref, dense, dout, mode)
        got = formula_scores(ref, dense, dout, mode)
        assert truth.dtype == torch.float64 and truth.abs().max() > 0
        assert (got - truth).abs().max().item() <= 1e-10 * truth.abs().max().item()
        assert (truth[:, dense[0] == 0] == 0).all()      # scores live at the bonds only


def test_general_relation_tensors_closed_form_float64():
    """real-valued multi-hot relation vectors: gradient x input of the relation tensor is sigmoid'(z) z dt/dA1"""
    from oracle.eagcn_ref import RefEAGCN
    from eagcn_amd.synthetic import make_batch
    channels = (6, 4, 3)
    mb = make_batch(B=4, n_max=9, n_med=6, rel_channels=channels, seed=3)
    dense = list(mb.dense())
    gen = torch.Generator().manual_seed(8)
    for k, c in enumerate(channels):
        v = torch.randn(mb.B, c, mb.N, mb.N, generator=gen) * (torch.rand(mb.B, c, mb.N, mb.N, generator=gen) < 0.6)
        dense[2 + k] = v * dense[0].unsqueeze(1)
    torch.manual_seed(2)
    ref = RefEAGCN(6, 24, [5, 4, 3], [6, 5, 4], 16, 8, 2, 0.0, structure='Concate', n_layers=2, rel_channels=list(channels)).double().eval()
    dout = target_weights(mb.B, 2, 0)
    truth = autograd_scores(ref, dense, dout, 'relation')
    got = formula_scores(ref, dense, dout, 'relation')
    assert (got - truth).abs().max().item() <= 1e-10 * truth.abs().max().item()


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from eagcn_amd import _lib
    return _lib, _lib.load()


def test_bond_attr_symbols_exported():
    L, lib = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    assert lib.eagcn_abi_version() == 8
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'eagcn_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name


def test_bond_grad_argument_checks_without_gpu():
    L, lib = _lib()
    dummy = C.c_void_p(64)

    def batch(lists=True):
        b = L.Batch()
        b.B, b.N, b.K, b.T, b.E = 1, 4, 1, 4, 4
        b.channels[0] = 2
        if lists:
            b.build_lists = 1
            b.row_ptr = b.row_info = b.row_m = b.meta = b.nbr = b.ecode = 64
        return b

    def params(training=0):
        p = L.LayerParams()
        p.K, p.structure, p.training = 1, 0, training
        p.width[0] = 4
        p.att_w[0] = 64
        return p

    def bufs():
        w = L.LayerBufs()
        w.P = w.Y = w.rscale = w.bn = 64
        return w
    call = lambda b, p, w, dx, mode, acc: lib.eagcn_layer_bond_grad(C.byref(b) if b else None, C.byref(p) if p else None,
                                                                    C.byref(w) if w else None, dx, mode, 1.0, 1, acc, None)
    b, p, w = batch(), params(), bufs()
    for args in ((None, p, w, dummy, 0, dummy), (b, None, w, dummy, 0, dummy), (b, p, None, dummy, 0, dummy),
                 (b, p, w, None, 0, dummy), (b, p, w, dummy, 0, None)):
        assert call(*args) == -1
        assert b'null' in lib.eagcn_last_error()
    assert call(b, p, L.LayerBufs(), dummy, 0, dummy) == -1                  # no saved tensors
    for mode in (-1, 2):
        assert call(b, p, w, dummy, mode, dummy) == -1
        assert b'mode' in lib.eagcn_last_error()
    assert call(b, params(training=1), w, dummy, 0, dummy) == -1
    assert b'eval' in lib.eagcn_last_error()
    assert call(batch(lists=False), p, w, dummy, 0, dummy) == -1
    assert b'bond lists' in lib.eagcn_last_error()
    assert call(b, p, w, dummy, 0, C.c_void_p(68)) == -1                     # a misaligned accumulator
    assert b'aligned' in lib.eagcn_last_error()
    # the finalize launch
    fin = lambda b, acc, K, mol: lib.eagcn_bond_attr_finalize(C.byref(b) if b else None, acc, K, mol, dummy, dummy, dummy, None, None)
    assert fin(None, dummy, 1, dummy) == -1
    assert fin(b, dummy, 1, None) == -1
    assert fin(batch(lists=False), dummy, 1, dummy) == -1
    assert b'bond lists' in lib.eagcn_last_error()
    assert fin(b, dummy, 0, dummy) == -1 and fin(b, dummy, 9, dummy) == -1
    assert fin(b, None, 1, dummy) == -1


def test_bond_grad_kernels_have_no_scratch(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not found')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-munsafe-fp-atomics', '-S',
             '--cuda-device-only']
    out = str(tmp_path / 'battr.s')
    r = subprocess.run([hipcc] + flags + ['-o', out, os.path.join(ROOT, 'eagcn_amd', 'csrc', 'battr.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r'- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)', open(out).read(), re.S):
        blk = m.group(0)
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        seen[name] = (int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk).group(1)),
                      int(re.search(r'\.vgpr_count:\s+(\d+)', blk).group(1)))
    grad = {n: v for n, v in seen.items() if 'bond_grad_kernel' in n}
    assert len(grad) == 5, sorted(seen)                                      # 1, 2, 3, 4, 8 chunks of 256 packed columns
    for name, (scratch, vgpr) in seen.items():
        assert scratch == 0 and vgpr <= 512, (name, scratch, vgpr)           # (512: what one wave per SIMD can hold)
    assert any('bond_attr_finalize_kernel' in n for n in seen)
