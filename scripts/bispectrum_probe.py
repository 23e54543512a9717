"""Times pmesh_amd.bispectrum (csrc/pmx_bispec.hip) on one GPU: its stages, the torch composition a caller had before,
and the reduce kernel against its own model.

For N^3 meshes (default 256, 512) with 16 shells (edges k_f * linspace(1, N / 3, 17): the outermost at the alias bound)
in f8 and f4, prints one JSON line per case:
    shells_ms, c2r_ms, reduce_ms   the stages of one half of the estimator (HIP events, median of --reps): the shell
                                   split, the nb in-place c2r, the reduction over all triangle bins
    torch_shells_ms, torch_reduce_ms   the same result through torch: one masked copy of the spectrum per shell, the
                                   same c2r, one (D_i * D_j * D_l).double().sum() per triangle bin (whole fields)
    model_ms                       max(nb cells elsize / HBM rate, 2 ntri cells / f64 vector rate), with what a float4 copy
                                   reaches on an MI355X (6.29 TB/s) and the device's 78.6 TFLOP/s of vector
                                   f64 (an FMA counted as two; the kernel multiplies and adds separately, as the
                                   library is built without contraction)
    max_rel_diff                   kernel against torch composition, relative to the largest |sum|

    python scripts/bispectrum_probe.py [--mesh 256 512] [--dtype f8 f4] [--reps 5] [--no-torch]
    python scripts/bispectrum_probe.py --ntri-sweep [--mesh 256]   reduce_ms for the first 1, 64, 128, 256, 512 and all
                                   triples of the list (f8): what is staging and what is the loop over the triangles
    python scripts/bispectrum_probe.py --f4-error   the yardstick of the f4 tolerance of tests/test_bispectrum.py: per
                                   parity case the error of the composition out of the complex64 c2r of masked copies
                                   and torch products in float64 against the numpy-f8 estimator, in units of
                                   sum_x |D_i D_j D_l| / N, next to that of bispectrum() itself
    python scripts/bispectrum_probe.py --vjp [--mesh 256 512] [--dtype f8 f4]   the stages of bispectrum_vjp
                                   (csrc/pmx_bispec_grad.hip), one JSON line per case: shells_ms, c2r_ms, pairsum_ms (all
                                   entries of adjoint_pairs, in place), r2c_ms (the nb in-place r2c), shells_vjp_ms, next
                                   to reduce_ms of the forward on the same fields; vjp_ms (bispectrum_vjp with result=)
                                   next to forward_half_ms (shells + c2r + reduce, the sums half of bispectrum); then the
                                   yardstick of the f4 tolerance of tests/test_bispectrum_gradients.py: per parity case
                                   the error of the gradient composed from bispec_shells, the complex64 c2r, torch
                                   products in float64, the complex64 r2c and torch.where against the numpy-f8
                                   gradient, relative to its largest modulus, next to that of bispectrum_vjp itself
Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -- python scripts/bispectrum_probe.py --no-torch ...`
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
from pmesh_amd.bispectrum import adjoint_pairs, bispectrum, bispectrum_vjp, triangle_bins  # noqa: E402
from pmesh_amd.pm import ParticleMesh, _blank  # noqa: E402

HBM_RATE = 6.29e12
F64_RATE = 78.6e12


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


def f4_error():
    from tests import test_bispectrum as T
    worst = 0
    for Nmesh, BoxSize in T.PARITY_MESHES:
        for kind in ('T', 'U', 'c2c'):
            for dp in (0, 2):
                e = T.composition_error(kind, Nmesh, BoxSize, dp)
                c, ke = T.parity_field(kind, Nmesh, BoxSize, 'f4')
                tri = triangle_bins(ke)
                S, _, scale = T.numpy_estimator(T.full_spectrum(c), Nmesh, BoxSize, ke, dp, tri)
                r = bispectrum(c, ke, deconv_pow=dp)
                mine = float(numpy.max(numpy.abs(r.sums - S) / scale))
                worst = max(worst, e)
                print('composition f4 error / scale: %s %s deconv %d: %.4g   (bispectrum(): %.4g)'
                      % (Nmesh, kind, dp, e, mine), flush=True)
    print('largest composition error / scale: %.4g' % worst)


def f4_vjp_error():
    from tests import test_bispectrum as T
    from tests import test_bispectrum_gradients as G
    worst = 0
    for Nmesh, BoxSize in T.PARITY_MESHES:
        for kind in ('T', 'U', 'c2c'):
            for dp in (0, 2):
                e = G.composition_error(kind, Nmesh, BoxSize, dp)
                c, ke, r, v, coef = G.parity_case(kind, Nmesh, BoxSize, dp, 'f4')
                want, _, _ = G.reference(c, ke, dp, coef)
                got = bispectrum_vjp(c, ke, v_B=v, deconv_pow=dp, result=r).value.cpu().numpy()
                mine = float(numpy.abs(got - want).max() / numpy.abs(want).max())
                worst = max(worst, e)
                print('composition f4 gradient error / max |grad|: %s %s deconv %d: %.4g   (bispectrum_vjp(): %.4g)'
                      % (Nmesh, kind, dp, e, mine), flush=True)
    print('largest composition gradient error / max |grad|: %.4g' % worst)


def vjp_stages(N, dt, nb, reps):
    """the stages of bispectrum_vjp on an N^3 mesh, each timed on the buffers the stage before left"""
    from pmesh_amd.lpt import _spectrum_of
    be = backend.get()
    pm = ParticleMesh([N, N, N], BoxSize=1000., dtype=dt)
    c = pm.create(type='complex')
    g = torch.Generator(device=c.value.device).manual_seed(1)
    x = pm.create(type='real')
    x.value.copy_(torch.randn(x.value.shape, generator=g, device=x.value.device, dtype=x.value.dtype))
    x.r2c(out=c)
    del x
    kf = 2 * numpy.pi / 1000.
    ke = kf * numpy.linspace(1, N / 3.0, nb + 1)
    tri = triangle_bins(ke)
    kt = torch.from_numpy(ke).to(be.device)
    tt = torch.from_numpy(tri).to(be.device)
    offsets, pairs, weights = adjoint_pairs(tri, numpy.random.RandomState(1).normal(size=len(tri)), nb)
    ot, pt, wt = (torch.from_numpy(a).to(be.device) for a in (offsets, pairs, weights))
    spectra = [_blank(type(c), pm) for _ in range(nb)]

    def shells():
        be.bispec_shells(c.value, [s.value for s in spectra], c.start, pm.Nmesh, pm.BoxSize, kt, 0, False)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    t_shells = timed(shells, reps)
    # (the transforms are in place: the whole chain again for each timed round)
    t_c2r, t_pair, t_r2c = [], [], []
    for _ in range(reps + 1):
        shells()
        t, fields = event_timed(lambda: [s.c2r(out=Ellipsis) for s in spectra])
        t_c2r.append(t)
        values = [f.value for f in fields]
        t, _ = event_timed(lambda: be.bispec_pairsum(values, values, ot, pt, wt))
        t_pair.append(t)
        t, back = event_timed(lambda: [_spectrum_of(f, c) for f in fields])
        t_r2c.append(t)
    out = _blank(type(c), pm)
    t_gather = timed(lambda: be.bispec_shells_vjp([s.value for s in back], out.value, c.start, pm.Nmesh, pm.BoxSize, kt,
                                                  0), reps)
    # the forward's reduction on the same run: shell fields again
    shells()
    values = [s.c2r(out=Ellipsis).value for s in spectra]
    acc = torch.zeros(len(tri), dtype=torch.float64, device=be.device)
    work = torch.empty(be.bispec_work(len(tri), values[0].numel()), dtype=torch.float64, device=be.device)

    def reduce():
        acc.zero_()
        be.bispec_reduce(values, tt, acc, work=work)
    t_reduce = timed(reduce, reps)
    del spectra, fields, values, back, out
    torch.cuda.empty_cache()
    r = bispectrum(c, ke)
    v = numpy.random.RandomState(2).normal(size=len(tri))
    t_vjp = timed(lambda: bispectrum_vjp(c, ke, v_B=v, result=r), reps)
    med = lambda ts: float(numpy.median(ts[1:]))            # noqa: E731
    rec = {'mesh': N, 'dtype': dt, 'shells': nb, 'ntri': len(tri), 'npairs': len(weights),
           'shells_ms': round(t_shells, 3), 'c2r_ms': round(med(t_c2r), 3), 'pairsum_ms': round(med(t_pair), 3),
           'r2c_ms': round(med(t_r2c), 3), 'shells_vjp_ms': round(t_gather, 3), 'reduce_ms': round(t_reduce, 3),
           'vjp_ms': round(t_vjp, 3), 'forward_half_ms': round(t_shells + med(t_c2r) + t_reduce, 3)}
    print(json.dumps(rec), flush=True)
    del c, pm
    torch.cuda.empty_cache()


def ntri_sweep(N, nb, reps):
    be = backend.get()
    fields = [torch.randn((N, N, N + 2), device=be.device, dtype=torch.float64)[..., :N] for _ in range(nb)]
    tri_all = triangle_bins(numpy.linspace(1, N / 3.0, nb + 1))
    for ntri in (1, 64, 128, 256, 512, len(tri_all)):
        tri = torch.from_numpy(tri_all[:ntri].copy()).to(be.device)
        acc = torch.zeros(ntri, dtype=torch.float64, device=be.device)
        work = torch.empty(be.bispec_work(ntri, fields[0].numel()), dtype=torch.float64, device=be.device)
        t = timed(lambda: be.bispec_reduce(fields, tri, acc, work=work), reps)
        print(json.dumps({'mesh': N, 'dtype': 'f8', 'shells': nb, 'ntri': ntri, 'reduce_ms': round(t, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--dtype', nargs='+', default=['f8', 'f4'])
    ap.add_argument('--shells', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--ntri-sweep', action='store_true')
    ap.add_argument('--f4-error', action='store_true')
    ap.add_argument('--vjp', action='store_true')
    args = ap.parse_args()
    be = backend.get()
    nb = args.shells
    if args.f4_error:
        return f4_error()
    if args.vjp:
        for N in args.mesh:
            for dt in args.dtype:
                vjp_stages(N, dt, nb, args.reps)
        return f4_vjp_error()
    if args.ntri_sweep:
        for N in args.mesh:
            ntri_sweep(N, nb, args.reps)
        return
    for N in args.mesh:
        for dt in args.dtype:
            pm = ParticleMesh([N, N, N], BoxSize=1000., dtype=dt)
            c = pm.create(type='complex')
            g = torch.Generator(device=c.value.device).manual_seed(1)
            # the spectrum of a real field (c2r expects its self-conjugate planes consistent)
            x = pm.create(type='real')
            x.value.copy_(torch.randn(x.value.shape, generator=g, device=x.value.device, dtype=x.value.dtype))
            x.r2c(out=c)
            del x
            kf = 2 * numpy.pi / 1000.
            ke = kf * numpy.linspace(1, N / 3.0, nb + 1)
            tri = triangle_bins(ke)
            kt = torch.from_numpy(ke).to(be.device)
            tt = torch.from_numpy(tri).to(be.device)
            spectra = [_blank(type(c), pm) for _ in range(nb)]

            def shells():
                be.bispec_shells(c.value, [s.value for s in spectra], c.start, pm.Nmesh, pm.BoxSize, kt, 0, False)

            def c2rs():
                return [s.c2r(out=Ellipsis) for s in spectra]

            t_shells = timed(shells, args.reps)
            # (the transforms are in place: split again before each timed round)
            ts = []
            for _ in range(args.reps + 1):
                shells()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fields = c2rs()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            t_c2r = float(numpy.median(ts[1:]))
            values = [f.value for f in fields]
            cells = values[0].numel()
            acc = torch.zeros(len(tri), dtype=torch.float64, device=be.device)
            work = torch.empty(be.bispec_work(len(tri), cells), dtype=torch.float64, device=be.device)

            def reduce():
                acc.zero_()
                be.bispec_reduce(values, tt, acc, work=work)

            t_reduce = timed(reduce, args.reps)
            es = values[0].element_size()
            bytes_ms = nb * cells * es / HBM_RATE * 1e3
            flops_ms = 2.0 * len(tri) * cells / F64_RATE * 1e3
            rec = {'mesh': N, 'dtype': dt, 'shells': nb, 'ntri': len(tri), 'shells_ms': round(t_shells, 3),
                   'c2r_ms': round(t_c2r, 3), 'reduce_ms': round(t_reduce, 3),
                   'model_ms': round(max(bytes_ms, flops_ms), 3), 'model_bytes_ms': round(bytes_ms, 3),
                   'model_flops_ms': round(flops_ms, 3), 'model_frac': round(max(bytes_ms, flops_ms) / t_reduce, 3)}
            if not args.no_torch:
                mine = acc.clone()

                def torch_shells():
                    kmag = torch.sqrt(sum(xd.double() ** 2 for xd in c.x))
                    j = torch.bucketize(kmag, kt, right=True) - 1
                    outs = []
                    for i in range(nb):
                        s = pm.create(type=type(c))
                        s.value[...] = torch.where(j == i, c.value, torch.zeros_like(c.value))
                        outs.append(s)
                    return outs

                out = torch.zeros(len(tri), dtype=torch.float64, device=be.device)

                def torch_reduce():
                    for t, (i, j, l) in enumerate(tri):
                        out[t] = (values[i].double() * values[j].double() * values[l].double()).sum()

                rec['torch_shells_ms'] = round(timed(torch_shells, 1), 3)
                rec['torch_reduce_ms'] = round(timed(torch_reduce, 1), 3)
                rec['reduce_speedup'] = round(rec['torch_reduce_ms'] / t_reduce, 1)
                rec['max_rel_diff'] = float((mine - out).abs().max() / out.abs().max())
            print(json.dumps(rec), flush=True)
            del spectra, fields, values, c, pm
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
