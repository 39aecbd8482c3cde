"""csrc/lagg_top.hip -- the transposed aggregation of a Concate top layer whose dH is never stored -- is held to the limits
tests/test_isa_cpu.py sets for the kernels of lagg.hip: no scratch, at most 168 registers (three waves per SIMD) and an LDS footprint
of which three workgroups fit a CU.  hipcc cross-compiles gfx950 here, no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-munsafe-fp-atomics', '-S', '--cuda-device-only']


def test_top_layer_aggregation_forms_have_no_scratch_and_three_workgroups_per_cu(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not found')
    out = str(tmp_path / 'lagg_top.s')
    r = subprocess.run([HIPCC] + FLAGS + ['-o', out, os.path.join(ROOT, 'eagcn_amd', 'csrc', 'lagg_top.hip')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for m in re.finditer(r'- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target|\Z)', open(out).read(), re.S):
        blk = m.group(0)
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        if 'lagg_kernel' in name:
            seen[name] = tuple(int(re.search(r'\.%s:\s+(\d+)' % f, blk).group(1))
                               for f in ('private_segment_fixed_size', 'vgpr_count', 'group_segment_fixed_size', 'vgpr_spill_count'))
    assert len(seen) == 2, seen                   # rows of the read-out gradient | the per-molecule gather
    for name, (scratch, vgpr, lds, spills) in seen.items():
        assert scratch == 0 and spills == 0 and vgpr <= 168, (name, scratch, spills, vgpr)
        assert 3 * lds <= 160 * 1024, (name, lds)
