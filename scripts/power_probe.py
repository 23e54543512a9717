"""Times pmesh_amd.power.power_spectrum (csrc/pmx_power.hip) on one GPU against its floor and the torch composition.

For N^3 meshes (default 256, 512, 1024) in f8 and f4 and the configurations
    1d      Nk = N/2 uniform k bins of width k_f
    poles   the same with multipoles {0, 2, 4}
    2d      the same with Nmu = 10 mu bins and multipoles {0, 2, 4}
    cross   1d of two fields
prints one JSON line per case: the kernel's time (HIP events, median of --reps launches of the entry alone), the floor
(bytes of the field(s) read once / the copy rate of DESIGN.md section 4, 5.6 TB/s, and / a read rate measured here on
the same array), and the time of the best pure-torch composition a caller has today (bucketize + index_add_ over
materialised |k| and mu; for 1d, poles and 2d).

    python scripts/power_probe.py [--mesh 256 512 1024] [--dtype f8 f4] [--reps 20] [--no-torch]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/power_probe.py ...` (a run of its
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
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.power import PowerResult, _Binning, power_spectrum  # noqa: E402

COPY_RATE = 5.6e12


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


def kernel_call(c, other, ke, me, poles):
    """the entry alone (what power_spectrum launches), on a zeroed accumulator"""
    be = backend.get()
    pm = c.pm
    bins = _Binning(len(pm.Nmesh), 'kedges', ke, me, None, poles, PowerResult, hermitian=1,
                    volume=numpy.prod(pm.BoxSize))            # the package's own struct, edges and table widths
    p, kt, mt, acc = bins.p, bins.et, bins.mt, bins.zeros()
    av, bv = c.value, (other.value if other is not None else None)

    def run():
        acc.zero_()
        be.power_project(p, av, bv, c.start, pm.Nmesh, pm.BoxSize, kt, mt, acc)
    return run


def torch_composition(c, ke, me, poles):
    """P(k) [, multipoles] [, P(k, mu)] with torch operations over materialised |k|, mu and weights"""
    pm = c.pm
    dev = c.value.device
    V = float(numpy.prod(pm.BoxSize))
    nk = len(ke) - 1
    kt = torch.from_numpy(ke).to(dev)
    mt = torch.from_numpy(me).to(dev) if me is not None else None

    def run():
        x = c.x
        kmag = torch.sqrt(x[0].double() ** 2 + x[1].double() ** 2 + x[2].double() ** 2)
        il = c.i[-1]
        w = (1 + ((il != 0) & (il != int(pm.Nmesh[-1]) // 2)).double()).expand_as(kmag)
        v = c.value
        p = (v.real.double() ** 2 + v.imag.double() ** 2) * V
        j = torch.bucketize(kmag, kt, right=True) - 1
        ok = (j >= 0) & (j < nk)
        j = torch.where(ok, j, torch.full_like(j, nk)).reshape(-1)
        wv = (w * ok).reshape(-1)
        out = torch.zeros((3 + len(poles), nk + 1), dtype=torch.float64, device=dev)
        out[0].index_add_(0, j, wv)
        out[1].index_add_(0, j, wv * kmag.reshape(-1))
        out[2].index_add_(0, j, wv * p.reshape(-1))
        if poles or mt is not None:
            mu = torch.where(kmag > 0, x[2].double().expand_as(kmag) / kmag, torch.zeros_like(kmag))
            for q, ell in enumerate(poles):
                L = {0: torch.ones_like(mu), 2: 0.5 * (3 * mu ** 2 - 1), 4: (35 * mu ** 4 - 30 * mu ** 2 + 3) / 8}[ell]
                out[3 + q].index_add_(0, j, (wv * p.reshape(-1)) * L.reshape(-1))
            if mt is not None:
                nmu = len(me) - 1
                m = (torch.bucketize(mu, mt, right=True) - 1).clamp(0, nmu - 1).reshape(-1)
                cell = j * nmu + m
                o2 = torch.zeros((3, (nk + 1) * nmu), dtype=torch.float64, device=dev)
                o2[0].index_add_(0, cell, wv)
                o2[1].index_add_(0, cell, wv * mu.reshape(-1))
                o2[2].index_add_(0, cell, wv * p.reshape(-1))
        return out
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[256, 512, 1024])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--check', action='store_true', help='also run power_spectrum once per case (results unused)')
    args = ap.parse_args()
    for N in args.mesh:
        for dt in args.dtype:
            pm = ParticleMesh([N, N, N], BoxSize=1000., dtype=dt)
            c = pm.create(type='complex')
            c2 = pm.create(type='complex')
            g = torch.Generator(device=c.value.device).manual_seed(1)
            for f in (c, c2):
                r = torch.view_as_real(f.value)
                r.copy_(torch.randn(r.shape, generator=g, device=r.device, dtype=r.dtype))
            kf = 2 * numpy.pi / 1000.
            ke = numpy.arange(N // 2 + 1) * kf
            me = numpy.linspace(-1, 1, 11)
            nbytes = c.value.numel() * c.value.element_size()
            read = timed(lambda: torch.view_as_real(c.value).sum(), args.reps)
            for name, other, mue, poles in (('1d', None, None, ()), ('poles', None, None, (0, 2, 4)),
                                            ('2d', None, me, (0, 2, 4)), ('cross', c2, None, ())):
                nb = nbytes * (2 if other is not None else 1)
                t = timed(kernel_call(c, other, ke, mue, poles), args.reps)
                rec = {'mesh': N, 'dtype': dt, 'case': name, 'kernel_ms': round(t, 4),
                       'floor_ms': round(nb / COPY_RATE * 1e3, 4), 'read_sum_ms': round(read * (2 if other is not None else 1), 4),
                       'x_floor': round(t / (nb / COPY_RATE * 1e3), 2), 'field_GB': round(nb / 1e9, 3)}
                if args.check:
                    power_spectrum(c, ke, other=other, muedges=mue, poles=poles)
                if not args.no_torch and other is None and N <= 512:
                    try:
                        rec['torch_ms'] = round(timed(torch_composition(c, ke, mue, poles), max(3, args.reps // 4)), 3)
                    except torch.cuda.OutOfMemoryError:
                        rec['torch_ms'] = None
                        torch.cuda.empty_cache()
                print(json.dumps(rec), flush=True)
            del c, c2, pm
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
