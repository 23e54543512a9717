"""Times pmesh_amd.interlace (csrc/pmx_interlace.hip) on one GPU against its yardstick.

For an N^3 mesh (default 512, f8, CIC) and N^3 particles on a jittered lattice, on one rank, with warm plans and HIP
events around work that is synchronised (median of --reps), prints one JSON line:
    plain_ms             one pm.paint(pos) + r2c(), what a caller without interlacing runs
    plain_x_ms           the same number of plain paint + r2c calls as the interlaced paint makes, per order
    interlaced_ms        paint_interlaced(order) for order 2 and 3 (with and without compensate)
    combine              pmx_phase_combine per (a, deconv_pow): ms (one launch, from --inner launches inside one pair of
                         events) and achieved bytes / s on the algorithmic bytes, modes * (read [+ read] + write)
    accumulate           pmx_ylm_accumulate (l = 2, m = 0) with beta 0 and 1 on the same spectra: the same byte counts
    yardstick_ms         order * plain_ms + (order - 1) * (one accumulate launch with beta = 1: three spectrum sweeps)
    ratio                interlaced_ms over the yardstick
    peak_fields          peak device memory of paint_interlaced over what was allocated before the call (positions in
                         neither), in buffers of one real field

    python scripts/interlace_probe.py [--mesh 512] [--dtype f8] [--resampler cic] [--reps 5] [--inner 10] [--plan-slots 3]
The calls are repeated on one position tensor, so a paint finds its bin plan again while the cache (2 plans) holds it:
the plain paint and order 2 do, order 3 (three transforms) rebuilds every plan in every call unless --plan-slots 3.
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/interlace_probe.py` (a run of its own).
"""
import argparse
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import backend, window  # noqa: E402
from pmesh_amd.interlace import paint_interlaced  # noqa: E402
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, _blank  # noqa: E402


def timed(fn, reps, inner=1):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return float(numpy.median(ts))


def lattice(n, L, device):
    """n^3 positions: the cell centres in memory order, each moved by up to half a cell"""
    i = torch.arange(n ** 3, device=device)
    pos = torch.stack([i // (n * n), (i // n) % n, i % n], dim=1).to(torch.float64)
    g = torch.Generator(device=device).manual_seed(1)
    pos += torch.rand(pos.shape, generator=g, device=device, dtype=torch.float64)
    return pos * (L / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, default=512)
    ap.add_argument('--dtype', default='f8')
    ap.add_argument('--resampler', default='cic')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--plan-slots', type=int, default=None,
                    help='bin plans the cache keeps (default: the package\'s 2; with 3, order 3 finds the plans of '
                         'its three transforms again in a repeated call, as order 2 and the plain paint do with 2)')
    args = ap.parse_args()
    if args.plan_slots:
        window._BinCache.SLOTS = args.plan_slots
    be = backend.get()
    N, L = args.mesh, 1000.
    pm = ParticleMesh([N, N, N], BoxSize=L, dtype=args.dtype, resampler=args.resampler)
    pos = lattice(N, L, be.device)

    rec = {'mesh': N, 'dtype': args.dtype, 'resampler': args.resampler, 'particles': len(pos), 'reps': args.reps,
           'inner': args.inner, 'plan_slots': window._BinCache.SLOTS}
    rec['plain_ms'] = round(timed(lambda: pm.paint(pos).r2c(), args.reps), 3)

    A0 = pm.paint(pos).r2c()
    A = _blank(TransposedComplexField, pm)
    modes, es = A.value.numel(), A.value.element_size()
    half = [0.5] * 3
    rec['combine'], rec['accumulate'] = [], []
    be.phase_combine(A0.value, A.value, A.start, pm.Nmesh, half, 0.0, 1.0, 0)             # finite values to add to
    for a, p in ((0.0, 0), (0.5, 0), (0.5, 2), (0.5, 3)):
        t = timed(lambda: be.phase_combine(A0.value, A.value, A.start, pm.Nmesh, half, a, 0.5, p), args.reps, args.inner)
        rec['combine'].append({'a': a, 'deconv_pow': p, 'ms': round(t, 4),
                               'TBps': round(modes * es * (2 + (a != 0)) / t / 1e9, 3)})
    for beta in (0, 1):
        t = timed(lambda: be.ylm_accumulate(2, 0, beta, A0.value, A.value, A.start, pm.Nmesh, pm.BoxSize), args.reps,
                  args.inner)
        rec['accumulate'].append({'l': 2, 'm': 0, 'beta': beta, 'ms': round(t, 4),
                                  'TBps': round(modes * es * (2 + beta) / t / 1e9, 3)})
    sweep3 = rec['accumulate'][1]['ms']
    field_bytes = A._base.storage.numel() * A._base.storage.element_size()
    del A0, A
    torch.cuda.empty_cache()

    def plain(times):
        for _ in range(times):
            pm.paint(pos).r2c()
    rec['plain_x_ms'], rec['interlaced_ms'], rec['compensated_ms'] = {}, {}, {}
    rec['yardstick_ms'], rec['ratio'] = {}, {}
    for order in (2, 3):
        rec['plain_x_ms'][order] = round(timed(lambda: plain(order), args.reps), 3)
        rec['interlaced_ms'][order] = round(timed(lambda: paint_interlaced(pm, pos, order=order), args.reps), 3)
        rec['compensated_ms'][order] = round(timed(lambda: paint_interlaced(pm, pos, order=order, compensate=True),
                                                   args.reps), 3)
        rec['yardstick_ms'][order] = round(order * rec['plain_ms'] + (order - 1) * sweep3, 3)
        rec['ratio'][order] = round(rec['interlaced_ms'][order] / rec['yardstick_ms'][order], 3)

    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = paint_interlaced(pm, pos, order=3, compensate=True)
    torch.cuda.synchronize()
    rec['peak_fields'] = round((torch.cuda.max_memory_allocated() - base) / field_bytes, 3)
    rec['field_bytes'] = field_bytes
    assert bool(torch.isfinite(torch.view_as_real(r.value)).all())
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
