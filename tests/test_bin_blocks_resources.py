"""Register / LDS budgets of the block-entry kernels of the bin plan (bin_entries_kernel, paint_entries_kernel,
readout_entries_kernel), read from the compiler's resource remarks like tests/test_kernel_resources.py: no scratch,
and the CIC regions on double canvases within 40 KB with room for four workgroups per CU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pmesh_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')


def _resources(source):
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math',
           '-I' + os.path.join(ROOT, 'include'), '-c', os.path.join(CSRC, source), '-o', os.devnull,
           '-Rpass-analysis=kernel-resource-usage']
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    table, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            table[name] = {}
            continue
        m = re.search(r'remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)', line)
        if m and name:
            table[name][m.group(1).split(' ')[0]] = int(m.group(2))
    return table


def test_block_entry_kernel_budgets():
    t = _resources('pmx_binned.hip')
    ents = {k: v for k, v in t.items() if 'entries_kernel' in k}
    assert sum('bin_entries_kernel' in k for k in ents) == 1
    assert sum('paint_entries_kernel' in k for k in ents) == 2          # double and float canvases
    assert sum('readout_entries_kernel' in k for k in ents) == 4        # x float / double results
    for k, v in ents.items():
        assert v['ScratchSize'] == 0, (k, v)
        assert v['VGPRs'] <= 128, (k, v)
        if 'ILi5Ed' in k and 'bin_' not in k:
            assert v['LDS'] <= 40960 and v['Occupancy'] >= 4, (k, v)
    # the index-list forms the entry kernels share their bodies with stay free of scratch
    lean = {k: v for k, v in t.items() if 'readout_tile_lean_kernel' in k and 'Li7EdLi768' not in k}
    assert lean and all(v['ScratchSize'] == 0 for v in lean.values()), lean
