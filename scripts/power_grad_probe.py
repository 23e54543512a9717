"""Times the gradient kernels of the power spectrum and of the tabulated transfer (csrc/pmx_power_grad.hip,
csrc/pmx_ktable_grad.hip) on one GPU against the forward kernels they mirror.

For N^3 meshes (default 256, 512) in f8 and f4:
  power_vjp   the configurations of power_probe.py (1d, poles, 2d = mu bins + poles), auto and cross: the forward
              entry pmx_power_project, the adjoint pmx_power_vjp, and a torch device copy of the bytes the adjoint
              writes.  goal_ms = 1.25 * (forward + copy).
  ktable      tables of 1000 (linear and log-log) and 8192 (log-log) entries: pmx_apply_ktable out of place,
              pmx_ktable_vjp and pmx_apply_ktable_jvp.  goal_ms = 1.25 * apply_ktable.
One JSON line per case, HIP events around the entry alone, median of --reps launches.

    python scripts/power_grad_probe.py [--mesh 256 512] [--dtype f8 f4] [--reps 20]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/power_grad_probe.py ...` (a run of
its own).
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
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.power import PowerResult, _Binning  # noqa: E402
from pmesh_amd.transfer import Tabulated  # noqa: E402


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


def power_calls(c, other, ga, gb, ke, me, poles):
    """the forward and the adjoint entries alone, on the same fields and bins"""
    be = backend.get()
    pm = c.pm
    bins = _Binning(len(pm.Nmesh), 'kedges', ke, me, None, poles, PowerResult, hermitian=1,
                    volume=numpy.prod(pm.BoxSize))            # the package's own struct, edges and table widths
    p, kt, mt, acc = bins.p, bins.et, bins.mt, bins.zeros()
    coef = torch.rand(p.nk * bins.c1 + p.nk * p.nmu * bins.c2, dtype=torch.float64, device=be.device)
    av, bv = c.value, (other.value if other is not None else None)
    gav, gbv = ga.value, (gb.value if other is not None else None)

    def forward():
        acc.zero_()
        be.power_project(p, av, bv, c.start, pm.Nmesh, pm.BoxSize, kt, mt, acc)

    def adjoint():
        be.power_vjp(p, av, bv, gav, gbv, c.start, pm.Nmesh, pm.BoxSize, kt, mt, coef)
    return forward, adjoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    be = backend.get()
    for N in args.mesh:
        for dt in args.dtype:
            pm = ParticleMesh([N, N, N], BoxSize=1000., dtype=dt)
            c, c2, g1, g2 = (pm.create(type='complex') for _ in range(4))
            gen = torch.Generator(device=c.value.device).manual_seed(1)
            for f in (c, c2):
                r = torch.view_as_real(f.value)
                r.copy_(torch.randn(r.shape, generator=gen, device=r.device, dtype=r.dtype))
            kf = 2 * numpy.pi / 1000.
            ke = numpy.arange(N // 2 + 1) * kf
            me = numpy.linspace(-1, 1, 11)
            nbytes = c.value.numel() * c.value.element_size()
            copy1 = timed(lambda: g1.value.copy_(c.value), args.reps)
            for name, mue, poles in (('1d', None, ()), ('poles', None, (0, 2, 4)), ('2d', me, (0, 2, 4))):
                for other in (None, c2):
                    fwd, adj = power_calls(c, other, g1, g2, ke, mue, poles)
                    tf, ta = timed(fwd, args.reps), timed(adj, args.reps)
                    copy = copy1 * (2 if other is not None else 1)
                    goal = 1.25 * (tf + copy)
                    print(json.dumps({'kernel': 'power_vjp', 'mesh': N, 'dtype': dt, 'case': name,
                                      'cross': other is not None, 'forward_ms': round(tf, 4), 'vjp_ms': round(ta, 4),
                                      'copy_ms': round(copy, 4), 'goal_ms': round(goal, 4), 'met': ta <= goal,
                                      'field_GB': round(nbytes / 1e9, 3)}), flush=True)
            kmax = numpy.sqrt(3.0) * numpy.pi * N / 1000.
            for n, loglog in ((1000, False), (1000, True), (8192, True)):
                k = numpy.geomspace(kf, kmax, n) if loglog else numpy.linspace(kf, kmax, n)
                tab = Tabulated(k, 1.0 + 1.0 / (1.0 + k), loglog=loglog)
                x, y, s = tab._table(be.device)
                grad = torch.zeros(n, dtype=torch.float64, device=be.device)
                dy = torch.rand(n, dtype=torch.float64, device=be.device)
                args3 = (c.start, pm.Nmesh, pm.BoxSize)
                t0 = timed(lambda: be.apply_ktable(s, c.value, g1.value, *args3), args.reps)
                tv = timed(lambda: be.ktable_vjp(s, True, c.value, c2.value, *args3, grad), args.reps)
                tj = timed(lambda: be.apply_ktable_jvp(s, dy, c.value, g1.value, *args3), args.reps)
                print(json.dumps({'kernel': 'ktable', 'mesh': N, 'dtype': dt, 'entries': n, 'loglog': loglog,
                                  'apply_ktable_ms': round(t0, 4), 'ktable_vjp_ms': round(tv, 4),
                                  'ktable_jvp_ms': round(tj, 4), 'goal_ms': round(1.25 * t0, 4),
                                  'vjp_met': tv <= 1.25 * t0, 'jvp_met': tj <= 1.25 * t0}), flush=True)
            del c, c2, g1, g2, pm
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
