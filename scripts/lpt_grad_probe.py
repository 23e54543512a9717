"""Times the 2LPT gradient kernels (csrc/pmx_lpt_grad.hip) and pmesh_amd.lpt.lpt_vjp / lpt_jvp on one GPU.

For N^3 meshes (default 256, 512) in f8 and f4, one JSON line per case:
    contract1   one spectrum times -i k_d / k^2 added into an accumulator (the per-component step of the vjp)
    contract6   six spectra times their Hessian factors summed into the first (the source step of the vjp)
    source_vjp  the six products g dS/dphi_p written over the six real Hessian fields
    source_jvp  dS(phi; phi') from twelve real fields, written over the first tangent
each against a device copy (torch copy_) that moves the same number of bytes (half read, half written): the kernel's
time, its bytes / time and the fraction of the copy's rate; then, for each mesh in f8 and f4,
    grad        lpt(order=2), lpt_vjp(order=2) with both cotangents and lpt_jvp(order=2) along a spectrum, timed in
                the same run, with the vjp split into its 6 paints of one component, its transforms (12 in-place r2c,
                7 in-place c2r) and its new kernels (6 + 1 contractions, 1 source vjp), each timed on its own
Times are HIP events, median of --reps runs.

    python scripts/lpt_grad_probe.py [--mesh 256 512] [--dtype f8 f4] [--reps 10] [--no-whole]
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/lpt_grad_probe.py --mesh 512 ...`
(a run of its own).
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
from pmesh_amd.lpt import lpt, lpt_jvp, lpt_vjp  # noqa: E402
from pmesh_amd.pm import ParticleMesh  # noqa: E402
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


def copy_time(nbytes, reps):
    """a device copy of nbytes / 2 bytes: nbytes moved"""
    n = int(nbytes // 2 // 8)
    a = torch.empty(n, dtype=torch.float64, device='cuda').fill_(1.0)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), reps)
    del a, b
    return t


def report(case, N, dtype, ms, nbytes, reps):
    c = copy_time(nbytes, reps)
    print(json.dumps(dict(case=case, mesh=N, dtype=dtype, ms=round(ms, 4), bytes=int(nbytes),
                          TBps=round(nbytes / ms / 1e9, 3), copy_ms=round(c, 4), copy_TBps=round(nbytes / c / 1e9, 3),
                          of_copy=round(c / ms, 3))), flush=True)


def kernels(N, dtype, reps):
    be = backend.get()
    pm = ParticleMesh([N] * 3, BoxSize=1000., dtype=dtype)
    c = pm.generate_whitenoise(1, unitary=True)
    spectra = [pm.create(type='complex') for _ in range(6)]
    for s in spectra:
        s.value.copy_(c.value)
    del c
    sv = [s.value for s in spectra]
    cb = sv[0].numel() * sv[0].element_size()
    args = (spectra[0].start, pm.Nmesh, pm.BoxSize)
    report('contract1', N, dtype, timed(lambda: be.lpt_contract(sv[1:2], [(0, -1)], sv[0], True, *args), reps),
           3 * cb, reps)
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    report('contract6', N, dtype, timed(lambda: be.lpt_contract(sv, pairs, sv[0], False, *args), reps), 7 * cb, reps)
    del spectra, sv
    reals = [pm.create(type='real') for _ in range(13)]
    for r in reals:
        r.value.fill_(0.5)
    rv = [r.value for r in reals]
    rb = rv[0].numel() * rv[0].element_size()
    # (scale 1: the values stay put from run to run)
    report('source_vjp', N, dtype, timed(lambda: be.lpt2_source_vjp(rv[12], rv[:6], rv[:6], 1.0), reps), 13 * rb,
           reps)
    report('source_jvp', N, dtype, timed(lambda: be.lpt2_source_jvp(rv[:6], rv[6:12], rv[12], 1.0), reps), 13 * rb,
           reps)
    del reals, rv


def table():
    k = numpy.geomspace(1e-4, 20.0, 1000)
    p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
    return k, p


def whole(N, dtype, reps):
    be = backend.get()
    pm = ParticleMesh([N] * 3, BoxSize=1000., resampler='cic', dtype=dtype)
    k, p = table()
    tab = Tabulated(k, numpy.sqrt(p / 1e9), loglog=True)
    c = pm.generate_whitenoise(1, unitary=True).apply(tab)
    u = pm.generate_whitenoise(2, unitary=True).apply(tab)
    q = pm.generate_uniform_particle_grid(shift=0.5)
    v1, v2 = torch.sin(q * 0.01), torch.cos(q * 0.02)
    t_fwd = timed(lambda: lpt(c, q, order=2), reps)
    t_vjp = timed(lambda: lpt_vjp(c, q, v1, v2, order=2), reps)
    t_jvp = timed(lambda: lpt_jvp(c, q, u, order=2), reps)
    m = v1[:, 0].contiguous()
    t_paint = timed(lambda: pm.paint(q, mass=m), reps)
    r = pm.create(type='real')
    r.value.fill_(1.0)
    t_r2c = timed(lambda: r.r2c(out=Ellipsis), reps)          # (each run scales the buffer by 1 / N^3: no overflow)
    del r
    w = pm.create(type='complex')
    w.value.copy_(c.value)
    t_c2r = timed(lambda: w.c2r(out=Ellipsis).r2c(out=Ellipsis), reps) - t_r2c
    a, b = pm.create(type='complex'), pm.create(type='complex')
    t_c1 = timed(lambda: be.lpt_contract([a.value], [(0, -1)], b.value, True, a.start, pm.Nmesh, pm.BoxSize), reps)
    hs = [pm.create(type='complex') for _ in range(5)]
    t_c6 = timed(lambda: be.lpt_contract([b.value] + [h.value for h in hs], [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2),
                                         (1, 2)], b.value, False, a.start, pm.Nmesh, pm.BoxSize), reps)
    del a, b, hs
    reals = [pm.create(type='real') for _ in range(7)]
    rv = [x.value for x in reals]
    t_sv = timed(lambda: be.lpt2_source_vjp(rv[6], rv[:6], rv[:6], 1.0), reps)
    del reals, rv
    paints = 6 * t_paint
    transforms = 12 * t_r2c + 7 * t_c2r
    new = 6 * t_c1 + t_c6 + t_sv
    print(json.dumps(dict(case='grad', mesh=N, dtype=dtype, lpt_ms=round(t_fwd, 3), vjp_ms=round(t_vjp, 3),
                          jvp_ms=round(t_jvp, 3), vjp_of_lpt=round(t_vjp / t_fwd, 3), jvp_of_lpt=round(t_jvp / t_fwd, 3),
                          vjp_paints_ms=round(paints, 3), vjp_transforms_ms=round(transforms, 3),
                          vjp_new_kernels_ms=round(new, 3), paint1_ms=round(t_paint, 3), r2c_inplace_ms=round(t_r2c, 3),
                          c2r_inplace_ms=round(t_c2r, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-whole', action='store_true')
    a = ap.parse_args()
    for N in a.mesh:
        for dt in a.dtype:
            kernels(N, dt, a.reps)
            torch.cuda.empty_cache()
            if not a.no_whole:
                whole(N, dt, a.reps)
                torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
