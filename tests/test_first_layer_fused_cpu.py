"""csrc/lagg_dw.hip -- the transposed aggregation with the first layer's weight gradient in its epilogue -- is held to the limits
tests/test_isa_cpu.py sets for the kernels of lagg.hip: no scratch, at most 168 registers (three waves per SIMD) and an LDS footprint
of which three workgroups fit a CU; and the units whose instantiations other tests count keep their counts (lagg.hip five, lagg_in.hip
four, lagg_top.hip two).  hipcc cross-compiles gfx950 here, no GPU needed."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-munsafe-fp-atomics', '-S', '--cuda-device-only']
FIELDS = ('private_segment_fixed_size', 'vgpr_count', 'group_segment_fixed_size', 'vgpr_spill_count')


def _kernels(tmp, unit):
    out = os.path.join(tmp, unit + '.s')
    r = subprocess.run([HIPCC] + FLAGS + ['-o', out, os.path.join(ROOT, 'eagcn_amd', 'csrc', unit + '.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r'- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)', open(out).read(), re.S):
        blk = m.group(0)
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        if 'lagg_kernel' in name:
            seen[name] = tuple(int(re.search(r'\.%s:\s+(\d+)' % f, blk).group(1)) for f in FIELDS)
    return seen


@pytest.fixture(scope='module')
def units(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not found')
    tmp = str(tmp_path_factory.mktemp('isa_dw'))
    names = ['lagg_dw', 'lagg', 'lagg_in', 'lagg_top']
    with ThreadPoolExecutor(max_workers=4) as ex:
        return dict(zip(names, ex.map(lambda n: _kernels(tmp, n), names)))


def test_fused_forms_have_no_scratch_and_three_workgroups_per_cu(units):
    seen = units['lagg_dw']
    assert len(seen) == 2, seen                   # one chunk | several chunks per workgroup
    for name, (scratch, vgpr, lds, spills) in seen.items():
        assert scratch == 0 and spills == 0 and vgpr <= 168, (name, scratch, spills, vgpr)
        assert 3 * lds <= 160 * 1024, (name, lds)


def test_the_counted_units_keep_their_instantiations_and_limits(units):
    assert (len(units['lagg']), len(units['lagg_in']), len(units['lagg_top'])) == (5, 4, 2), {u: sorted(k) for u, k in units.items()}
    for unit in ('lagg', 'lagg_in', 'lagg_top'):
        for name, (scratch, vgpr, lds, spills) in units[unit].items():
            assert scratch == 0 and spills == 0 and vgpr <= 168 and 3 * lds <= 160 * 1024, (unit, name, scratch, vgpr, lds)
