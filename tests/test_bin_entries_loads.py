"""The gather loop of readout_entries_kernel (csrc/pmx_binned.hip: tile_gather_lean<..., ENT>) keeps the position
loads of BOTH slots of a trip in front of the masks' branches.  Left to itself the compiler sinks the first slot's loads
behind its mask test (mask -> branch -> block number -> position: three memory round trips in a row where the list form
has two); that cost the entry form's readout 5 % against the index list on rows whose masks are full.
Read from the ISA of the readout part of the file: one straight-line block of the kernel holds both 16-byte position
loads, as it does in readout_tile_lean_kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pmesh_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')


def _kernels(source, part):
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math',
           '-I' + os.path.join(ROOT, 'include'), '-DPMX_BINNED_PART=%d' % part, '--cuda-device-only', '-S',
           os.path.join(CSRC, source), '-o', '-']
    out = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    bodies, name = {}, None
    for line in out.stdout.splitlines():
        m = re.match(r'^(_ZN3pmx\w+):', line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif name is not None:
            bodies[name].append(line)
            if 's_endpgm' in line:
                name = None
    return bodies


def _row_loads_per_block(body):
    """16-byte global loads (the first two doubles of a position row) in every straight-line piece of the kernel"""
    counts, n = [], 0
    for line in body:
        if re.match(r'^\.LBB', line) or 's_cbranch' in line:
            counts.append(n)
            n = 0
        elif 'global_load_dwordx4' in line:
            n += 1
    counts.append(n)
    return counts


def test_entry_readout_loads_both_rows_in_front_of_the_mask_branches():
    k = _kernels('pmx_binned.hip', 3)
    for out_el in ('Li8', 'Li4'):                  # double / float results
        ent = [b for n, b in k.items() if 'readout_entries_kernelILi5EdLi512ELi8E%sELb1' % out_el in n]
        lst = [b for n, b in k.items() if 'readout_tile_lean_kernelILi5EdLi512ELi8E%sELb1' % out_el in n]
        assert len(ent) == 1 and len(lst) == 1, sorted(k)
        if out_el == 'Li8':     # (the pattern this test reads, where the compiler is known to keep it)
            assert max(_row_loads_per_block(lst[0])) == 2, _row_loads_per_block(lst[0])
        assert max(_row_loads_per_block(ent[0])) == 2, _row_loads_per_block(ent[0])
