"""Times the kernels of the Poisson sampler (csrc/pmx_poisson.hip) on one GPU against a device copy of the same bytes
and against what a caller could do with torch alone.

For an N^3 f8 mesh (default 512):
  linear    a constant field with nbar V_cell in {0.1, 1, 8}
  lognormal exp(x) of a unit Gaussian x (mode EXP, bias 1, mean rate 1): a few cells reach the hundreds
Per case pmx_poisson_rate_sum, pmx_poisson_count, pmx_poisson_scan and pmx_poisson_emit alone (HIP events around the
entry, a warm-up call, the median of --reps launches, clocks as found), the algorithmic bytes of each, a device copy
that moves the same bytes (half read, half written), the whole poisson_sample call (host clock, synchronised), and
the composition a caller has without this package: torch.poisson on the rate, repeat_interleave of the cell
coordinates, torch.rand offsets.  One JSON line per case.

    python scripts/mock_probe.py [--mesh 512] [--reps 10] [--no-torch]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/mock_probe.py ...` (a run of its
own).
"""
import argparse
import json
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import _abi, backend  # noqa: E402
from pmesh_amd.mock import poisson_sample  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402

SEG = _abi.PMX_POISSON_SEGMENT


def timed(fn, reps, prep=None):
    """median ms of `reps` launches of fn after one warm-up; prep runs before each, outside the events"""
    ts = []
    for i in range(reps + 1):
        if prep is not None:
            prep()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b))
    return float(numpy.median(ts))


def copy_ms(nbytes, reps, dev):
    """a device copy that moves nbytes in all: nbytes / 2 read and as many written"""
    n = max(int(nbytes) // 2, 1)
    src = torch.empty(n, dtype=torch.uint8, device=dev)
    dst = torch.empty(n, dtype=torch.uint8, device=dev)
    src.zero_()
    t = timed(lambda: dst.copy_(src), reps)
    del src, dst
    torch.cuda.empty_cache()
    return t


def torch_composition(rate, coords, h, reps):
    """what a caller can do today on the device: counts, repeated coordinates, uniform offsets"""
    def run():
        n = torch.poisson(rate).to(torch.int64).reshape(-1)
        rows = torch.repeat_interleave(coords, n, dim=0)
        rows += torch.rand(rows.shape, dtype=torch.float64, device=rows.device) - 0.5
        rows *= h
        return rows
    ts = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = run()
        torch.cuda.synchronize()
        if i:
            ts.append((time.perf_counter() - t0) * 1e3)
        del rows
    return float(numpy.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, default=512)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    be = backend.get()
    dev = be.device
    N, L = args.mesh, 1000.
    pm = ParticleMesh([N, N, N], BoxSize=L, dtype='f8')
    f = pm.create(type='real')
    ncells = N ** 3
    nseg = (ncells + SEG - 1) // SEG
    gen = torch.Generator(device=dev).manual_seed(1)
    cases = [('linear', r, _abi.PMX_POISSON_LINEAR, r, 0.0) for r in (0.1, 1.0, 8.0)]
    cases.append(('lognormal', 1.0, _abi.PMX_POISSON_EXP, 1.0 / numpy.exp(0.5), 1.0))
    for name, mean_rate, mode, scale, bias in cases:
        if mode == _abi.PMX_POISSON_EXP:
            f.value.copy_(torch.randn(f.value.shape, generator=gen, device=dev, dtype=torch.float64))
        else:
            f.value.fill_(1.0)
        x = f.value
        seed = 12345
        counts = torch.empty(tuple(x.shape), dtype=torch.uint32, device=dev)
        seg0 = torch.empty(nseg, dtype=torch.int64, device=dev)
        seg = torch.empty(nseg, dtype=torch.int64, device=dev)
        head = torch.zeros(3, dtype=torch.int64, device=dev)
        rsum = head[2:3].view(torch.float64)
        t_rate = timed(lambda: be.poisson_rate_sum(x, mode, scale, bias, rsum), args.reps)
        t_count = timed(lambda: be.poisson_count(x, f.start, pm.Nmesh, mode, scale, bias, seed, counts, seg0, head[1:2]),
                        args.reps)
        t_scan = timed(lambda: be.poisson_scan(seg, head[0:1]), args.reps, prep=lambda: seg.copy_(seg0))
        total = int(head[0].item())
        assert int(head[1].item()) == 0
        pos = torch.empty((total, 3), dtype=torch.float64, device=dev)
        t_emit = timed(lambda: be.poisson_emit(tuple(x.shape), f.start, pm.Nmesh, pm.BoxSize, seed, counts, seg, pos, None),
                       args.reps)
        cell = torch.empty(total, dtype=torch.int64, device=dev)
        t_emit_cell = timed(lambda: be.poisson_emit(tuple(x.shape), f.start, pm.Nmesh, pm.BoxSize, seed, counts, seg, pos,
                                                    cell), args.reps)
        maxcount = int(counts.view(torch.int32).max().item())
        del pos, cell
        torch.cuda.empty_cache()
        b_rate = 8 * ncells
        b_count = 12 * ncells + 8 * nseg
        b_scan = 16 * nseg
        b_emit = 4 * ncells + 8 * nseg + 24 * total
        b_emit_cell = b_emit + 8 * total
        line = {'case': name, 'mesh': N, 'mean_rate': mean_rate, 'particles': total, 'max_count': maxcount,
                'rate_sum_ms': round(t_rate, 4), 'count_ms': round(t_count, 4), 'scan_ms': round(t_scan, 4),
                'emit_ms': round(t_emit, 4), 'emit_cell_ms': round(t_emit_cell, 4),
                'rate_sum_bytes': b_rate, 'count_bytes': b_count, 'scan_bytes': b_scan, 'emit_bytes': b_emit,
                'emit_cell_bytes': b_emit_cell,
                'rate_sum_GBps': round(b_rate / t_rate / 1e6, 1), 'count_GBps': round(b_count / t_count / 1e6, 1),
                'emit_GBps': round(b_emit / t_emit / 1e6, 1), 'emit_cell_GBps': round(b_emit_cell / t_emit_cell / 1e6, 1),
                'copy_rate_sum_ms': round(copy_ms(b_rate, args.reps, dev), 4),
                'copy_count_ms': round(copy_ms(b_count, args.reps, dev), 4),
                'copy_emit_ms': round(copy_ms(b_emit, args.reps, dev), 4)}

        def whole():
            s = poisson_sample(f, scale=scale, seed=seed, mode='exp' if mode == _abi.PMX_POISSON_EXP else 'linear',
                               bias=bias)
            torch.cuda.synchronize()
            return s
        ts = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = whole()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
            assert s.size == total
            del s
        line['poisson_sample_ms'] = round(float(numpy.median(ts)), 3)
        torch.cuda.empty_cache()
        if not args.no_torch:
            rate = (scale * torch.exp(bias * x)) if mode == _abi.PMX_POISSON_EXP else scale * x
            coords = pm.mesh_coordinates('f8')
            h = torch.as_tensor(pm.BoxSize / pm.Nmesh, dtype=torch.float64, device=dev)
            line['torch_ms'] = round(torch_composition(rate, coords, h, max(3, args.reps // 3)), 3)
            del rate, coords
            torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
