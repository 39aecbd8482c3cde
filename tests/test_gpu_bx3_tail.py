"""The tail pass of the dX product (csrc/bx3_epi.h) at the shapes its row-major lane map can get wrong and test_gpu_hidden_bn.py does
not reach.  A lane of the pass owns FOUR adjacent columns of sixteen rows of a wave's 64 x 64 block (lane l: columns 4 (l & 15) .. + 3,
rows 4 t + (l >> 4)); sixteen lanes cover a row, the four row groups of a wave are summed by two exchanges, lanes 0-15 write the slab.

Batches (K = 3 views of exact width 48: packed width 144 = 128 + 16 -- the LAST 64-column block holds 16 valid columns, four lanes of
every row group, the Tox21 case 400 = 3 x 128 + 16 in small; layer 2 runs the plane pair, layer 1 is fused):
  rows65   four ring molecules of 20 + 20 + 13 + 12 atoms: T = 65 packed rows, one full 64-row block and a block of ONE row
  rows5    the T = 5 batch of test_gpu_hidden_bn.py with three views: a single partial block
  tile144  the 24 chains of test_gpu_hidden_bn.py's tile-edges batch with three views: T = 300 (three 128-row tiles, five 64-row blocks,
           the last one of 44 rows) x 144 columns (two 128-column tiles, the second one of 16 columns)
each with dropout 0 and 0.3, in the eager engine and in the captured fused step, through test_gpu_hidden_bn._check: the switch at 1
against the switch at 0 (outputs, loss, running statistics and every gradient but the fused layer's d gamma / d beta bit-identical;
those two at most one fp32 ulp of the tensor's largest magnitude apart) and against the oracle (helpers.assert_grad_parity).

With EAGCN_BX3_WGS=8 (read once by the library: a child process) one workgroup per XCD takes every unit of its eighth: several k-chunks
and several dX tiles per workgroup, so a wave's second walk runs the tail pass of more than one unit.  The child runs the three-layer
dropout case of test_tile_edges, the tile144 case of this file and the direct pair launches below, all at their usual bounds, and
first of all test_the_grid_the_library_runs, which fails there unless the library really launches eight workgroups.

The direct eagcn_gemm_bx3_pair calls, (T, F_in, F_p) = (300, 160, 160) and (65, 144, 160), hold dX and the sum of the
eagcn_bx3_pair_used_splits slabs of dW to float64 as test_gpu_bx3.py does; slabs beyond that count stay unwritten."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_hidden_bn as hb
from test_gpu_bx3 import _err, _planes

pytestmark = pytest.mark.gpu

NARROW = dict(chans=[6, 4, 3], w1=[48] * 3, w2=[48] * 3)


def _ring(n):
    return hb._chain(0, n - 1) + [(0, n - 1)]


def _rows65():
    sizes = [20, 20, 13, 12]
    assert sum(sizes) == 65
    return hb._mol_batch(sizes, [_ring(n) for n in sizes], 20, 21, NARROW['chans'])


def _rows5():
    return hb._mol_batch([2, 3, 1], [[(0, 1)], [(0, 1), (1, 2)], []], 3, 6, NARROW['chans'])


def _tile144():
    sizes = hb.TILE_SIZES
    assert sum(sizes) == 300
    return hb._mol_batch(sizes, [hb._chain(0, n - 1) + ([(0, n - 1)] if n > 8 else []) for n in sizes], 20, 11, NARROW['chans'])


BATCHES = {'rows65': _rows65, 'rows5': _rows5, 'tile144': _tile144}


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'fused_step'])
@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('name', sorted(BATCHES))
def test_sixteen_column_last_block(name, p, graph, monkeypatch):
    # (_check counts the layer calls that took the route `where the widths are test_gpu_hidden_bn.WIDE`: these widths take it too)
    monkeypatch.setattr(hb, 'WIDE', NARROW)
    hb._check(name + '/144', BATCHES[name](), NARROW, 2, p, graph)


def test_three_layers_of_144_columns(monkeypatch):
    """layers 2 and 1 both fused: both ping-pong buffers in both roles, at 65 rows"""
    monkeypatch.setattr(hb, 'WIDE', NARROW)
    hb._check('rows65/144', _rows65(), NARROW, 3, 0.3, False)


@pytest.mark.parametrize('T,FIN,FP', [(300, 160, 160), (65, 144, 160)])
def test_pair_launch_vs_float64(T, FIN, FP):
    from eagcn_amd import _lib as L
    lib = L.load()
    torch.manual_seed(T + FIN + FP)
    splits = 4
    X = torch.randn(T, FIN, device='cuda').relu()
    dP = torch.randn(T, FP, device='cuda')
    W = torch.randn(FIN, FP, device='cuda') * 0.05
    px, sx, rx = _planes(X)
    pp, sp, rp = _planes(dP)
    pw, sw, rw = _planes(W)
    dX = torch.full((T, FIN), float('nan'), device='cuda')
    dW = torch.full((splits, FIN, FP), float('nan'), device='cuda')
    L.check(lib.eagcn_gemm_bx3_pair(T, FIN, FP, C.c_void_p(pp.data_ptr()), sp, FP, rp, C.c_void_p(pw.data_ptr()), sw, FP, rw, C.c_void_p(dX.data_ptr()), FIN,
                                    FIN, FP, T, C.c_void_p(px.data_ptr()), sx, FIN, rx, C.c_void_p(pp.data_ptr()), sp, FP, rp, C.c_void_p(dW.data_ptr()), FP,
                                    splits, FIN * FP, 3, None), 'eagcn_gemm_bx3_pair')
    used = lib.eagcn_bx3_pair_used_splits(splits, FIN, FP, T, T, FIN, FP)
    assert 1 <= used <= splits and torch.isnan(dW[used:]).all() and not torch.isnan(dW[:used]).any()
    ex = _err(dX.double(), dP.double(), W.double(), False)
    ew = _err(dW[:used].double().sum(0), X.double(), dP.double(), True)
    print('pair (%d, %d, %d): %d slabs; dX error %.2e, dW error %.2e of sum |a||b|' % (T, FIN, FP, used, ex, ew))
    assert ex <= 8 * 2.0 ** -24 and ew <= 8 * 2.0 ** -24, (ex, ew)


def test_the_grid_the_library_runs():
    """The chunk count of the Tox21 pair (T = 4809, 400 x 700) depends on the grid the library launches (bx3_grid): 14 slabs at 256
    workgroups, 2 at 8 (one workgroup per XCD; a launch of that size then runs on the 256 x 128 kernel).  In the child process of
    test_one_workgroup_per_xcd this pins that EAGCN_BX3_WGS=8 was read."""
    from eagcn_amd import _lib as L
    used = L.load().eagcn_bx3_pair_used_splits(64, 400, 700, 4809, 4809, 400, 700)
    if os.environ.get('EAGCN_BX3_WGS') == '8':
        assert used == 2, used
    else:
        assert used > 2, used


def test_one_workgroup_per_xcd():
    here = os.path.abspath(__file__)
    ids = [here + '::test_the_grid_the_library_runs', os.path.join(os.path.dirname(here), 'test_gpu_hidden_bn.py') + '::test_tile_edges[3-0.3-eager]',
           here + '::test_sixteen_column_last_block[tile144-0.3-eager]', here + '::test_pair_launch_vs_float64']
    env = dict(os.environ, EAGCN_BX3_WGS='8')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider'] + ids, env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(here)), timeout=300)
    assert r.returncode == 0 and '5 passed' in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
