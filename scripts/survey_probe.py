"""Times pmesh_amd.survey (csrc/pmx_survey.hip) on one GPU against its yardstick.

For an N^3 mesh (default 512, f8) and an observer outside the box, with warm plans and HIP events around work that is
synchronised (median of --reps), prints one JSON line:
    survey_ms            survey_multipoles(poles=(0, 2, 4)): 15 r2c, 14 weight and 14 accumulate passes, 3 cross spectra
    r2c_ms, r2c_inplace_ms   one out-of-place r2c of the field; one in place over the scratch buffer, as the estimator runs it
    power_ms             one cross power_spectrum on the same edges
    weight / accumulate  per (l, m) of --lm and, for accumulate, per beta: ms (one launch, from --inner launches inside
                         one pair of events) and achieved bytes / s on the algorithmic bytes: cells * (read + write) for
                         the weights, modes * (read [+ read] + write) for the accumulation
    yardstick_ms         15 * r2c_inplace_ms + the bytes of the 28 harmonic passes at the copy rates --copy-rate
                         (default 5.3e12 and 5.9e12, what DESIGN.md records for streaming kernels on this device)
    ratio                survey_ms over the yardstick (both ends)
    peak_fields          peak device memory of survey_multipoles over what was allocated before the call (the input
                         field included in neither), in buffers of one real field

    python scripts/survey_probe.py [--mesh 512] [--dtype f8] [--reps 7] [--inner 10]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/survey_probe.py` (a run of its own).
"""
import argparse
import json
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import backend  # noqa: E402
from pmesh_amd.pm import ParticleMesh, RealField, TransposedComplexField, _blank  # noqa: E402
from pmesh_amd.power import power_spectrum  # noqa: E402
from pmesh_amd.survey import multipole_field, survey_multipoles  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, default=512)
    ap.add_argument('--dtype', default='f8')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--lm', type=int, nargs='+', default=[2, 0, 2, -2, 4, 0, 4, 3, 4, -4],
                    help='pairs l m l m ... to time the harmonic kernels on')
    ap.add_argument('--copy-rate', type=float, nargs=2, default=[5.3e12, 5.9e12])
    args = ap.parse_args()
    be = backend.get()
    N, L = args.mesh, 1000.
    pm = ParticleMesh([N, N, N], BoxSize=L, dtype=args.dtype)
    F = pm.create(type='real')
    g = torch.Generator(device=F.value.device).manual_seed(1)
    F.value.copy_(torch.randn(F.value.shape, generator=g, device=F.value.device, dtype=F.value.dtype))
    origin = (-1.5 * L, 0.3 * L, -0.7 * L)
    kf = 2 * numpy.pi / L
    kedges = numpy.arange(0.5 * kf, numpy.pi * N / L, kf)
    es = F.value.element_size()
    cells = F.value.numel()
    field_bytes = F._base.storage.numel() * es

    rec = {'mesh': N, 'dtype': args.dtype, 'reps': args.reps, 'inner': args.inner}
    rec['r2c_ms'] = round(timed(lambda: F.r2c(), args.reps), 4)
    scratch = _blank(RealField, pm)
    spec = TransposedComplexField(pm, base=scratch._base)
    rec['r2c_inplace_ms'] = round(timed(lambda: scratch.r2c(out=spec), args.reps), 4)
    A0 = F.r2c()
    A = _blank(TransposedComplexField, pm)
    modes = A.value.numel()
    rec['power_ms'] = round(timed(lambda: power_spectrum(A0, kedges, other=A0), args.reps), 4)

    rec['weight'], rec['accumulate'] = [], []
    for l, m in zip(args.lm[0::2], args.lm[1::2]):
        t = timed(lambda: be.ylm_weight(l, m, F.value, scratch.value, F.start, pm.Nmesh, pm.BoxSize, origin), args.reps,
                  args.inner)
        rec['weight'].append({'l': l, 'm': m, 'ms': round(t, 4), 'TBps': round(cells * 2 * es / t / 1e9, 3)})
        be.ylm_accumulate(l, m, 0, A0.value, A.value, A.start, pm.Nmesh, pm.BoxSize)      # finite values to add to
        for beta in (0, 1):
            t = timed(lambda: be.ylm_accumulate(l, m, beta, A0.value, A.value, A.start, pm.Nmesh, pm.BoxSize),
                      args.reps, args.inner)
            rec['accumulate'].append({'l': l, 'm': m, 'beta': beta, 'ms': round(t, 4),
                                      'TBps': round(modes * 2 * es * (2 + beta) / t / 1e9, 3)})
    del scratch, spec, A
    torch.cuda.empty_cache()

    rec['multipole_field_ms'] = {l: round(timed(lambda: multipole_field(F, l, origin), args.reps), 3) for l in (2, 4)}
    rec['survey_ms'] = round(timed(lambda: survey_multipoles(F, kedges, origin), args.reps), 3)
    kernel_bytes = 14 * cells * 2 * es + modes * 2 * es * (2 * 2 + 12 * 3)
    rec['kernel_bytes'] = kernel_bytes
    rec['yardstick_ms'] = [round(15 * rec['r2c_inplace_ms'] + kernel_bytes / rate * 1e3, 3) for rate in args.copy_rate]
    rec['ratio'] = [round(rec['survey_ms'] / y, 3) for y in rec['yardstick_ms']]

    del A0
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = survey_multipoles(F, kedges, origin)
    torch.cuda.synchronize()
    rec['peak_fields'] = round((torch.cuda.max_memory_allocated() - base) / field_bytes, 3)
    rec['field_bytes'] = field_bytes
    assert all(numpy.isfinite(r.poles[l][r.modes > 0]).all() for l in (0, 2, 4))
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
