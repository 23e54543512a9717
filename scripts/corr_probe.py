"""Times the kernels of the correlation function (csrc/pmx_corr.hip) on one GPU against the kernels that move the same
bytes, and the whole correlation_function against the calls a caller already has.

For N^3 meshes (default 512) in f8 and f4:
  corr_project  plain, poles (0, 2, 4) and ten mu bins + poles: pmx_corr_project on the real mesh and its adjoint
                pmx_corr_vjp against pmx_power_project with the same options on the half spectrum of the same mesh
                (the same bytes: one read, 8 B per cell in f8).
  product       pmx_spectral_product with and without the window, overwriting and accumulating, against
                pmx_phase_combine with a != 0 and the same deconv_pow (two reads and one write as well).
  whole         correlation_function(real field) against its own r2c + c2r + one power_spectrum of the same options.
One JSON line per case, HIP events around the entry alone, median of --reps launches; rates count the bytes of the
mesh the kernel reads and writes.

    python scripts/corr_probe.py [--mesh 512] [--dtype f8 f4] [--reps 20]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/corr_probe.py ...` (a run of its
own).
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
from pmesh_amd.correlation import CorrResult, correlation_function  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.power import PowerResult, _Binning, power_spectrum  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(numpy.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[512])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    be = backend.get()
    L = 1000.
    for N in args.mesh:
        for dt in args.dtype:
            pm = ParticleMesh([N, N, N], BoxSize=L, dtype=dt)
            f, g = pm.create(type='real'), pm.create(type='real')
            c, c2, c3 = (pm.create(type='complex') for _ in range(3))
            gen = torch.Generator(device=f.value.device).manual_seed(1)
            f.value.copy_(torch.randn(f.value.shape, generator=gen, device=f.value.device, dtype=f.value.dtype))
            for s in (c, c2, c3):
                r = torch.view_as_real(s.value)
                r.copy_(torch.randn(r.shape, generator=gen, device=r.device, dtype=r.dtype))
            real_bytes = f.value.numel() * f.value.element_size()
            spec_bytes = c.value.numel() * c.value.element_size()
            H, kf = L / N, 2 * numpy.pi / L
            re, ke = numpy.arange(N // 2 + 1) * H, numpy.arange(N // 2 + 1) * kf
            me = numpy.linspace(-1, 1, 11)
            for name, mue, poles in (('plain', None, ()), ('poles', None, (0, 2, 4)), ('mu10', me, (0, 2, 4))):
                # the package's own structs, edges and table widths: the real side, and the k side of the same options
                bc = _Binning(3, 'redges', re, mue, None, poles, CorrResult)
                bp = _Binning(3, 'kedges', ke, mue, None, poles, PowerResult, hermitian=1, volume=L ** 3)
                pc, pp, rt, kt, m = bc.p, bp.p, bc.et, bp.et, bc.mt
                accc, accp = bc.zeros(), bp.zeros()
                coef = torch.rand(pc.nk * bc.c1 + pc.nk * pc.nmu * bc.c2, dtype=torch.float64, device=be.device)
                tc = timed(lambda: be.corr_project(pc, f.value, f.start, pm.Nmesh, pm.BoxSize, rt, m, accc), args.reps)
                tv = timed(lambda: be.corr_vjp(pc, g.value, g.start, pm.Nmesh, pm.BoxSize, rt, m, coef), args.reps)
                tp = timed(lambda: be.power_project(pp, c.value, None, c.start, pm.Nmesh, pm.BoxSize, kt, m, accp),
                           args.reps)
                print(json.dumps({'kernel': 'corr_project', 'mesh': N, 'dtype': dt, 'case': name,
                                  'corr_project_ms': round(tc, 4), 'corr_vjp_ms': round(tv, 4),
                                  'power_project_ms': round(tp, 4), 'ratio': round(tc / tp, 3),
                                  'corr_project_GBps': round(real_bytes / tc / 1e6, 1),
                                  'corr_vjp_GBps': round(real_bytes / tv / 1e6, 1),
                                  'power_project_GBps': round(spec_bytes / tp / 1e6, 1)}), flush=True)
            shift = [0.5] * 3
            for p in (2, 0):
                ty = timed(lambda: be.phase_combine(c2.value, c3.value, c.start, pm.Nmesh, shift, 0.5, 0.5, p), args.reps)
                for acc in (False, True):
                    tx = timed(lambda: be.spectral_product(c.value, c2.value, c3.value, c.start, pm.Nmesh, 1.0, True,
                                                           acc, p), args.reps)
                    nb = (4 if acc else 3) * spec_bytes
                    print(json.dumps({'kernel': 'spectral_product', 'mesh': N, 'dtype': dt, 'deconv_pow': p,
                                      'accumulate': acc, 'product_ms': round(tx, 4), 'phase_combine_ms': round(ty, 4),
                                      'ratio': round(tx / ty, 3), 'product_GBps': round(nb / tx / 1e6, 1),
                                      'phase_combine_GBps': round(3 * spec_bytes / ty / 1e6, 1)}), flush=True)
            del c2, c3, g
            torch.cuda.empty_cache()
            for name, mue, poles in (('plain', None, ()), ('mu10', me, (0, 2, 4))):
                tw = timed(lambda: correlation_function(f, re, muedges=mue, poles=poles), max(3, args.reps // 4))

                def yardstick():
                    s = f.r2c()
                    power_spectrum(s, ke, muedges=mue, poles=poles)
                    s.c2r(out=Ellipsis)
                ty = timed(yardstick, max(3, args.reps // 4))
                print(json.dumps({'kernel': 'whole', 'mesh': N, 'dtype': dt, 'case': name,
                                  'correlation_function_ms': round(tw, 3), 'r2c_c2r_power_ms': round(ty, 3),
                                  'ratio': round(tw / ty, 3)}), flush=True)
            del f, c, pm
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
