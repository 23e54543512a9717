"""Times the initial-condition kernels (csrc/pmx_lpt.hip) and pmesh_amd.lpt on one GPU.

For N^3 meshes (default 256, 512, 1024) in f8 and f4, one JSON line per case:
    ktable    Tabulated(loglog=True, 1000 entries) applied in place to the r2c spectrum
    hessian   three Hessian spectra k_i k_j / k^2 delta from one read of delta
    source    the 2LPT source from six real fields, written over the first
each against a device copy (torch copy_) that moves the same number of bytes (half read, half written): the kernel's
time, its bytes / time and the fraction of the copy's rate; then, for each mesh in f8,
    lpt       the whole lpt(order=2) on the lattice (shift 0.5), against the sum of the times of the transforms it runs
              (6 in-place c2r, 1 in-place r2c, 6 c2r with the fused gradient) and of its readout of six fields
    host      Field.apply with a numpy.interp callable (the host slab loop Tabulated replaces), one run
Times are HIP events, median of --reps runs.

    python scripts/lpt_probe.py [--mesh 256 512 1024] [--dtype f8 f4] [--reps 10] [--no-host] [--no-lpt]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/lpt_probe.py --mesh 512 ...` (a run
of its own).
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

from pmesh_amd import backend  # noqa: E402
from pmesh_amd.lpt import lpt  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402
from pmesh_amd.transfer import Tabulated, Transfer  # noqa: E402


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


def copy_time(nbytes, reps):
    """a device copy of nbytes / 2 bytes: nbytes moved"""
    n = int(nbytes // 2 // 8)
    a = torch.empty(n, dtype=torch.float64, device='cuda').fill_(1.0)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), reps)
    del a, b
    return t


def table():
    k = numpy.geomspace(1e-4, 20.0, 1000)
    p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
    return k, p


def report(case, N, dtype, ms, nbytes, reps):
    c = copy_time(nbytes, reps)
    print(json.dumps(dict(case=case, mesh=N, dtype=dtype, ms=round(ms, 4), bytes=int(nbytes),
                          TBps=round(nbytes / ms / 1e9, 3), copy_ms=round(c, 4), copy_TBps=round(nbytes / c / 1e9, 3),
                          of_copy=round(c / ms, 3))), flush=True)


def kernels(N, dtype, reps):
    be = backend.get()
    pm = ParticleMesh([N] * 3, BoxSize=1000., dtype=dtype)
    c = pm.generate_whitenoise(1, unitary=True)
    v = c.value
    cb = v.numel() * v.element_size()
    k, p = table()
    tab = Tabulated(k, numpy.sqrt(p / 1e9), loglog=True)
    x, y, s = tab._table(be.device)
    report('ktable', N, dtype, timed(lambda: be.apply_ktable(s, v, v, c.start, pm.Nmesh, pm.BoxSize), reps), 2 * cb,
           reps)
    outs = [pm.create(type='complex') for _ in range(3)]
    ov = [o.value for o in outs]
    pairs = [(0, 1), (0, 2), (1, 2)]
    report('hessian', N, dtype, timed(lambda: be.lpt_hessian(v, pairs, ov, c.start, pm.Nmesh, pm.BoxSize), reps),
           4 * cb, reps)
    del outs, ov
    reals = [pm.create(type='real') for _ in range(6)]
    for r in reals:
        r.value.fill_(0.5)
    rv = [r.value for r in reals]
    rb = rv[0].numel() * rv[0].element_size()
    report('source', N, dtype, timed(lambda: be.lpt2_source(rv, rv[0], 3.0 / 7.0), reps), 7 * rb, reps)
    del reals, rv, c, v


def whole(N, reps, host):
    pm = ParticleMesh([N] * 3, BoxSize=1000., resampler='cic')
    k, p = table()
    c = pm.generate_whitenoise(1, unitary=True).apply(Tabulated(k, numpy.sqrt(p / 1e9), loglog=True))
    q = pm.generate_uniform_particle_grid(shift=0.5)
    t_lpt = timed(lambda: lpt(c, q, order=2), reps)
    w = pm.create(type='complex')
    w.value.copy_(c.value)
    t_ip = timed(lambda: w.c2r(out=Ellipsis).r2c(out=Ellipsis), reps)      # one in-place c2r + one in-place r2c
    r = pm.create(type='real')
    r.value.fill_(1.0)
    t_r2c = timed(lambda: r.r2c(out=Ellipsis), reps)          # (each run scales the buffer by 1 / N^3: no overflow)
    del r
    t_c2r_ip = t_ip - t_r2c
    t_fused = timed(lambda: c.c2r(transfer=Transfer.dx1(0)), reps)
    fields = [c.c2r(transfer=Transfer.dx1(d % 3)) for d in range(6)]
    t_read = timed(lambda: pm.readout(fields, q), reps)
    del fields
    transforms = 6 * t_c2r_ip + t_r2c + 6 * t_fused
    print(json.dumps(dict(case='lpt', mesh=N, dtype='f8', ms=round(t_lpt, 3), transforms_ms=round(transforms, 3),
                          c2r_inplace_ms=round(t_c2r_ip, 3), r2c_inplace_ms=round(t_r2c, 3),
                          c2r_fused_ms=round(t_fused, 3), readout6_ms=round(t_read, 3),
                          ratio=round(t_lpt / transforms, 3), ratio_without_readout=round((t_lpt - t_read) / transforms, 3))),
          flush=True)
    if host:
        kk, tt = numpy.asarray(k), numpy.sqrt(p / 1e9)

        def interp(kv, v):
            kmag = numpy.sqrt(sum(ki ** 2 for ki in kv))
            with numpy.errstate(divide='ignore'):
                return v * numpy.exp(numpy.interp(numpy.log(kmag), numpy.log(kk), numpy.log(tt), left=-numpy.inf))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.apply(interp)
        torch.cuda.synchronize()
        t_host = (time.perf_counter() - t0) * 1e3
        t_dev = timed(lambda: c.apply(Tabulated(k, numpy.sqrt(p / 1e9), loglog=True), out=Ellipsis), reps)
        print(json.dumps(dict(case='host', mesh=N, dtype='f8', host_apply_ms=round(t_host, 1),
                              tabulated_ms=round(t_dev, 4), speedup=round(t_host / t_dev, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[256, 512, 1024])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-lpt', action='store_true')
    a = ap.parse_args()
    for N in a.mesh:
        for dt in a.dtype:
            kernels(N, dt, a.reps)
            torch.cuda.empty_cache()
        if not a.no_lpt and N <= 512:
            whole(N, a.reps, not a.no_host)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
