"""Bit-level A/B of the spectral entry points between two builds of libpmesh_amd.so.

Runs seeded calls of every entry point that walks a strided block (apply_transfer, apply_ktable and its gradients, the
LPT kernels and their gradients, power_project, power_vjp, bispec_shells, bispec_reduce) on the small shapes at which
the walk can go wrong, in f8 and f4, and prints one line `<case> <entry> <form> <output> <sha256>` per output tensor.
Run it once per library, each in a process of its own, and diff the two outputs:

    PMESH_AMD_LIBRARY=/path/to/other/libpmesh_amd.so python scripts/kspace_ab.py > a.txt
    python scripts/kspace_ab.py > b.txt && diff a.txt b.txt

The sums of power_project and ktable_vjp are added with floating-point atomics, so their last bits can change from call
to call of ONE library: for these the line holds the distinct hashes of REPEATS calls, and two libraries agree when
their sets overlap.  The mode counts of power_project are exact whatever the order and have a line of their own.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pmesh_amd import _abi, backend  # noqa: E402
from pmesh_amd.power import PowerResult, _Binning  # noqa: E402

# (name, shape, Nmesh, start, memory order of the input, of the outputs); memory order: logical axes, slowest first
CASES = [
    ('1d', (7,), (12,), (3,), (0,), (0,)),
    ('2d-transposed', (5, 6), (12, 6), (4, 0), (1, 0), (0, 1)),
    ('3d-transposed', (5, 6, 7), (12, 6, 12), (3, 0, 2), (1, 0, 2), (2, 0, 1)),
    ('3d-unit0', (1, 6, 7), (12, 6, 12), (3, 0, 2), (0, 1, 2), (0, 1, 2)),
    ('3d-unit1', (5, 1, 7), (12, 6, 12), (3, 2, 2), (0, 1, 2), (1, 0, 2)),
    ('3d-unit2', (5, 6, 1), (12, 6, 12), (3, 0, 5), (0, 1, 2), (0, 1, 2)),
    ('3d-wrap', (70000, 2, 3), (70000, 2, 4), (0, 0, 0), (0, 1, 2), (0, 1, 2)),
]
BOX = (100.0, 60.0, 130.0)


def block(gen, shape, order, dtype, device):
    """a seeded block of logical `shape` whose memory order is `order`"""
    mem = [shape[d] for d in order]
    real = dtype in (torch.float32, torch.float64)
    rd = dtype if real else (torch.float32 if dtype == torch.complex64 else torch.float64)
    t = torch.randn(mem + ([] if real else [2]), generator=gen, dtype=torch.float64).to(rd)
    if not real:
        t = torch.view_as_complex(t)
    return t.to(device).permute([order.index(d) for d in range(len(shape))])


def blank(shape, order, dtype, device):
    mem = [shape[d] for d in order]
    return torch.zeros(mem, dtype=dtype, device=device).permute([order.index(d) for d in range(len(shape))])


def report(*what):
    t = what[-1]
    h = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
    print(' '.join(str(w) for w in what[:-1]), h, flush=True)


REPEATS = 8


def report_sums(*what):
    """an output summed with atomics: what[-1]() makes it afresh; the distinct hashes of REPEATS calls"""
    hs = sorted(set(hashlib.sha256(what[-1]().cpu().numpy().tobytes()).hexdigest() for _ in range(REPEATS)))
    print(' '.join(str(w) for w in what[:-1]), ','.join(hs), flush=True)


def ktable(loglog, kmax, device):
    k = numpy.linspace(0.05 * kmax, 0.8 * kmax, 9)
    y = 1.0 + numpy.cos(3 * numpy.arange(9.0)) ** 2
    x, yy = (numpy.log(k), numpy.log(y)) if loglog else (k, y)
    s = _abi.KTable()
    s.n, s.loglog, s.amplitude = 9, int(loglog), 1.5
    s.left, s.right, s.kmin, s.kmax = 0.25, 0.5, float(k[0]), float(k[-1])
    step = numpy.diff(x)
    if numpy.abs(step - step.mean()).max() <= 1e-6 * step.mean():
        s.inv_step = 1.0 / step.mean()
    xt, yt = torch.from_numpy(x).to(device), torch.from_numpy(yy).to(device)
    s.x, s.y = xt.data_ptr(), yt.data_ptr()
    return s, (xt, yt)


def run_case(be, name, shape, nmesh, start, oin, oout, cdt):
    dev = be.device
    nd = len(shape)
    box = BOX[:nd]
    rdt = torch.float32 if cdt == torch.complex64 else torch.float64
    tag = '%s-%s' % (name, 'f4' if cdt == torch.complex64 else 'f8')
    gen = torch.Generator().manual_seed(1234)
    a, b = block(gen, shape, oin, cdt, dev), block(gen, shape, oin, cdt, dev)
    es = a.element_size()
    kny = min(numpy.pi * n / L for n, L in zip(nmesh, box))

    # apply_transfer: SIMPLE and general forms
    forms = [('dx1', dict(laplace_pow=-1, grad_dir=nd - 1, grad_kind=0)), ('potential', dict(amplitude=-1.0, laplace_pow=-1)),
             ('laplace2', dict(laplace_pow=-2)), ('deconv3-gauss', dict(deconv_pow=3, gauss_r=1.5)),
             ('finite4', dict(laplace_pow=-1, grad_dir=0, grad_kind=1))]
    for form, kw in forms:
        t = _abi.Transfer()
        t.amplitude, t.grad_dir = 1.0, -1
        for k, v in kw.items():
            setattr(t, k, v)
        out = blank(shape, oout, cdt, dev)
        be.call('apply_transfer', C.byref(t), nd, es // 2, a.data_ptr(), _abi.i64arr([s * es for s in a.stride()], 3),
                out.data_ptr(), _abi.i64arr([s * es for s in out.stride()], 3), _abi.i64arr(shape, 3),
                _abi.i64arr(start, 3), _abi.i64arr(nmesh, 3), _abi.f64arr(box, 3), be.stream())
        report(tag, 'apply_transfer', form, 'out', out)

    # tabulated transfer and its gradients
    for loglog in (False, True):
        form = 'loglog' if loglog else 'linear'
        s, keep = ktable(loglog, kny, dev)
        out = blank(shape, oout, cdt, dev)
        be.apply_ktable(s, a, out, start, nmesh, box)
        report(tag, 'apply_ktable', form, 'out', out)
        dy = torch.from_numpy(numpy.sin(numpy.arange(9.0))).to(dev)
        out = blank(shape, oout, cdt, dev)
        be.apply_ktable_jvp(s, dy, a, out, start, nmesh, box)
        report(tag, 'apply_ktable_jvp', form, 'out', out)

        def vjp():
            grad = torch.zeros(9, dtype=torch.float64, device=dev)
            be.ktable_vjp(s, True, a, b, start, nmesh, box, grad)
            return grad
        report_sums(tag, 'ktable_vjp', form, 'grad', vjp)
        del keep

    # LPT: Hessian spectra, contraction, and the real-space source with its gradients
    pairs = [(i, j) for i in range(nd) for j in range(i, nd)][:3]
    for n in range(1, len(pairs) + 1):
        outs = [blank(shape, oout, cdt, dev) for _ in range(n)]
        be.lpt_hessian(a, pairs[:n], outs, start, nmesh, box)
        for p, o in enumerate(outs):
            report(tag, 'lpt_hessian', 'nout%d' % n, 'out%d' % p, o)
    ins = [block(gen, shape, oin, cdt, dev) for _ in range(6)]
    factors = [(0, 0), (nd - 1, -1), (0, nd - 1), (nd - 1, nd - 1), (0, -1), (nd // 2, nd // 2)]
    for n in range(1, 7):
        acc = n % 2 == 0
        out = b.clone() if acc else blank(shape, oout, cdt, dev)
        be.lpt_contract(ins[:n], factors[:n], out, acc, start, nmesh, box)
        report(tag, 'lpt_contract', 'nin%d%s' % (n, '-acc' if acc else ''), 'out', out)
    if nd >= 2:
        m = 3 if nd == 2 else 6
        h = [block(gen, shape, oin, rdt, dev) for _ in range(m)]
        t = [block(gen, shape, oin, rdt, dev) for _ in range(m)]
        g = block(gen, shape, oin, rdt, dev)
        out = blank(shape, oout, rdt, dev)
        be.lpt2_source(h, out, -3.0 / 7)
        report(tag, 'lpt2_source', '-', 'out', out)
        outs = [blank(shape, oout, rdt, dev) for _ in range(m)]
        be.lpt2_source_vjp(g, h, outs, -3.0 / 7)
        for p, o in enumerate(outs):
            report(tag, 'lpt2_source_vjp', '-', 'out%d' % p, o)
        out = blank(shape, oout, rdt, dev)
        be.lpt2_source_jvp(h, t, out, -3.0 / 7)
        report(tag, 'lpt2_source_jvp', '-', 'out', out)

    # power spectrum and its adjoint
    nk, nmu = 6, 4
    for form, mu, poles, cross, dp in (('1d-auto', False, (), False, 0), ('poles-auto', False, (0, 2, 4), False, 2),
                                       ('mu-cross', True, (), True, 0), ('mu-poles-cross', True, (0, 1, 2), True, 2)):
        bins = _Binning(nd, 'kedges', numpy.linspace(0, 1.2 * kny, nk + 1),
                        numpy.linspace(-1, 1, nmu + 1) if mu else None, None, poles, PowerResult, hermitian=1,
                        deconv_pow=dp, volume=numpy.prod(box))
        p, ke, me, s1 = bins.p, bins.et, bins.mt, bins.s1
        other = b if cross else None

        def project():
            acc = bins.zeros()
            be.power_project(p, a, other, start, nmesh, box, ke, me, acc)
            return acc
        report_sums(tag, 'power_project', form, 'acc', project)
        acc = project()
        report(tag, 'power_project', form, 'counts', torch.cat([acc[:nk * s1].view(nk, s1)[:, 0],
                                                                acc[nk * s1:].view(-1, 5)[:, 0]]))
        ncoef = nk * bins.c1 + nk * p.nmu * bins.c2
        coef = torch.from_numpy(numpy.cos(numpy.arange(float(ncoef)))).to(dev)
        ga = blank(shape, oout, cdt, dev)
        gb = blank(shape, oout, cdt, dev) if cross else None
        be.power_vjp(p, a, other, ga, gb, start, nmesh, box, ke, me, coef)
        report(tag, 'power_vjp', form, 'grad_a', ga)
        if cross:
            report(tag, 'power_vjp', form, 'grad_b', gb)

    # bispectrum: the shell split (both forms), and the reduction with 5 / 20 / 40 shells for its three chunk sizes
    for unit in (False, True):
        for nb in (5,):
            se = torch.from_numpy(numpy.linspace(0.1 * kny, 1.1 * kny, nb + 1)).to(dev)
            outs = [blank(shape, oout, cdt, dev) for _ in range(nb)]
            be.bispec_shells(a, outs, start, nmesh, box, se, deconv_pow=0 if unit else 2, unit=unit)
            for s_, o in enumerate(outs):
                report(tag, 'bispec_shells', 'unit%d-nb%d' % (unit, nb), 'out%d' % s_, o)
    for nb in (5, 20, 40):
        fields = [block(gen, shape, oout, rdt, dev) for _ in range(nb)]
        tri = torch.tensor([(i, j, (i + j) % nb) for i in range(0, nb, 2) for j in range(i, nb, 3)], dtype=torch.int32,
                           device=dev)
        acc = torch.zeros(len(tri), dtype=torch.float64, device=dev)
        be.bispec_reduce(fields, tri, acc)
        report(tag, 'bispec_reduce', 'nb%d' % nb, 'acc', acc)


def main():
    be = backend.get()
    print('# library', backend.library_path(), file=sys.stderr)
    for case in CASES:
        for cdt in (torch.complex128, torch.complex64):
            run_case(be, *case, cdt)
    be.synchronize()


if __name__ == '__main__':
    main()
