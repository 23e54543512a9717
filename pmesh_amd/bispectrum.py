"""Binned bispectrum of complex fields, measured on the device.

The FFT estimator that bskit-style codes compose from ``ComplexField.apply``, ``c2r`` and products of real fields:
with nb shells from ``kedges`` (``kedges[i] <= |k| < kedges[i + 1]``, the bins of ``power_spectrum``) and, for a field
``a`` in pmesh's normalisation (``r2c`` divides by N = prod(Nmesh), ``c2r`` is the plain sum),

    D_i = c2r(a_m / W_m where shell(m) == i, else 0),    W_m = prod_d sinc(w_d / 2)^deconv_pow,
    I_i = c2r(1 where shell(m) == i, else 0),

the triangle bin t = (i, j, l), i <= j <= l, holds

    S_t = sum_x D_i D_j D_l / N,    C_t = sum_x I_i I_j I_l / N,    B_t = V^2 S_t / C_t,    V = prod(BoxSize).

``power`` and ``Q`` of the result are of the same field a / W: power_spectrum divides the product a conj(a) by its
``deconv_pow``, so they come from ``power_spectrum(field, kedges, deconv_pow=2 * deconv_pow)``.

C_t is the number of ordered mode triples (k1 in i, k2 in j, k3 in l) with k1 + k2 + k3 = 0, an integer.  A bin is
kept only when ``kedges[l] < kedges[i + 1] + kedges[j + 1]``: no other triple of shells holds a closed triangle.  The
product in real space closes triangles modulo Nmesh, so the outermost edge must not exceed
``min_d (2 pi / BoxSize_d) Nmesh_d / 3``: every mode index then satisfies 3 |s_d| < N_d and no wrapped triple exists.

Two kernels (csrc/pmx_bispec.hip, include/pmesh_amd.h): pmx_bispec_shells reads the spectrum once and writes all nb
shell spectra; after the nb distributed ``c2r`` s, pmx_bispec_reduce reads every shell field once and adds
``sum_x D_i D_j D_l`` of every triangle bin into a float64 vector, which is summed once over ``pm.comm`` before any
division.  Memory: the nb shell fields live at once, each in the buffer of an in-place transform (a real field with
its padded last axis, the size of one complex work field), next to the input field; the indicator half reuses the same
amount after the first half is released.  Chunking the shells is not done here.

    from pmesh_amd.bispectrum import bispectrum
    r = bispectrum(delta_k, kedges=kf * numpy.arange(0.5, 17), deconv_pow=2)
    r.triangles, r.k, r.B, r.Q, r.counts
    r2 = bispectrum(other_delta_k, r.kedges, deconv_pow=2, counts=r)       # the counts depend on geometry only

Not here: gradients (a ``bispectrum_vjp`` needs an adjoint kernel of its own), cross-bispectra of different fields, a
line of sight / multipoles, meshes that are not 3-d.
"""
import numpy
import torch

from . import _abi, backend
from .power import _complex, _edges, power_spectrum


class BispectrumResult(object):
    """The binned bispectrum.  ``kedges``; per triangle bin (ntri of them): ``triangles`` ((ntri, 3) shell numbers
    i <= j <= l), ``ntriangles`` (the count of closed mode triples C_t), ``k`` ((ntri, 3) mean |k| of the three shells),
    ``B``, ``Q`` = B / (P_i P_j + P_j P_l + P_l P_i), and the raw ``sums`` S_t and ``counts`` C_t (float64); per shell:
    ``power``, the P(k) of the field whose bispectrum ``B`` is, a / W: ``power_spectrum`` on the same edges with
    ``deconv_pow`` doubled, because it divides the product a conj(a) by prod sinc^deconv_pow where the bispectrum
    divides the amplitude a (real part).  Empty bins hold NaN."""

    def __init__(self, kedges, triangles, sums, counts, pk, boxsize, nmesh):
        self.kedges = kedges
        self.triangles = triangles
        self.sums = sums
        self.counts = counts
        self.Nmesh = tuple(int(n) for n in nmesh)
        self.BoxSize = tuple(float(x) for x in boxsize)
        volume = float(numpy.prod(self.BoxSize))
        self.ntriangles = numpy.rint(counts).astype('i8')
        self.power = pk.power.real
        i, j, l = triangles.T
        self.k = pk.k[triangles]
        with numpy.errstate(invalid='ignore', divide='ignore'):
            self.B = numpy.where(self.ntriangles > 0, volume ** 2 * sums / self.ntriangles, numpy.nan)
            p = self.power
            self.Q = self.B / (p[i] * p[j] + p[j] * p[l] + p[l] * p[i])


def triangle_bins(kedges):
    """the (ntri, 3) triples i <= j <= l of shells that can hold a closed triangle, in lexicographic order"""
    e = numpy.asarray(kedges, dtype='f8')
    nb = len(e) - 1
    i, j, l = numpy.meshgrid(numpy.arange(nb), numpy.arange(nb), numpy.arange(nb), indexing='ij')
    keep = (i <= j) & (j <= l) & (e[l] < e[i + 1] + e[j + 1])
    return numpy.stack([i[keep], j[keep], l[keep]], axis=1).astype('i4')


def alias_bound(pm):
    """the largest outer edge for which the real-space product wraps no triangle: min_d (2 pi / L_d) N_d / 3"""
    return float(min(2 * numpy.pi / float(L) * int(n) / 3.0 for L, n in zip(pm.BoxSize, pm.Nmesh)))


def _shell_sums(a, kt, nb, tri, deconv_pow, unit):
    """sum_x D_i D_j D_l / N per triangle (unit: of the indicator fields), summed over the ranks: a host vector"""
    from .pm import _blank
    be = backend.get()
    pm = a.pm
    # (raw memory: the shells entry writes every mode of every block)
    spectra = [_blank(type(a), pm) for _ in range(nb)]
    acc = torch.zeros(len(tri), dtype=torch.float64, device=be.device)
    try:
        be.bispec_shells(a.value, [s.value for s in spectra], a.start, pm.Nmesh, pm.BoxSize, kt, deconv_pow, unit)
        fields = []
        while spectra:
            fields.append(spectra.pop(0).c2r(out=Ellipsis))          # each in its own buffer
        # (of a complex mesh the real part: the transform of a Hermitian spectrum)
        values = [f.value.real if f.value.is_complex() else f.value for f in fields]
        be.bispec_reduce(values, tri, acc)
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise
    if pm.comm.size > 1:
        acc = pm.comm.allreduce(acc)
    return acc.cpu().numpy() / float(numpy.prod([int(n) for n in pm.Nmesh]))


def bispectrum(field, kedges, deconv_pow=0, counts=None):
    """The binned bispectrum of `field`: see the module docstring.

    field : ComplexField of a 3-d ParticleMesh in any layout (transposed, untransposed, compressed r2c or full c2c),
        complex64 or complex128, or RealField (r2c'd into a temporary).  Of a complex (c2c) mesh the real part of the
        configuration-space field is measured.  Other dimensions raise NotImplementedError.
    kedges : nb + 1 strictly increasing |k| edges, nb <= PMX_BISPEC_MAX_SHELLS, kedges[-1] within the alias bound
        min_d (2 pi / BoxSize_d) Nmesh_d / 3.
    deconv_pow : divide every mode (the amplitude) by W = prod_d sinc(w_d / 2)^deconv_pow (window compensation: 2 for
        a CIC-painted density).  power_spectrum divides |a|^2 by its deconv_pow, so the ``power`` and ``Q`` of the
        result come from power_spectrum(..., deconv_pow=2 * deconv_pow): the P(k) of the same field a / W.
    counts : a BispectrumResult of the same mesh and edges: its counts are reused and the indicator half is skipped.

    Memory: nb shell fields at once, each in the buffer of an in-place transform, next to the input.
    """
    a = _complex(field)
    pm = a.pm
    if len(pm.Nmesh) != 3:
        raise NotImplementedError('bispectra of %d-dimensional meshes: only 3-d meshes' % len(pm.Nmesh))
    if a.value.dtype not in (torch.complex64, torch.complex128):
        raise ValueError('bispectrum measures complex64 or complex128 fields')
    ke = _edges('kedges', kedges)
    nb = len(ke) - 1
    if nb > _abi.PMX_BISPEC_MAX_SHELLS:
        raise ValueError('%d shells: more than PMX_BISPEC_MAX_SHELLS = %d' % (nb, _abi.PMX_BISPEC_MAX_SHELLS))
    if int(deconv_pow) != deconv_pow or deconv_pow < 0:
        raise ValueError('deconv_pow must be a non-negative integer')
    bound = alias_bound(pm)
    if ke[-1] > bound:
        raise ValueError('kedges[-1] = %g is past the alias bound min_d (2 pi / BoxSize_d) Nmesh_d / 3 = %g: triangles '
                         'would close modulo Nmesh' % (ke[-1], bound))
    tri = triangle_bins(ke)
    if counts is not None:
        if not isinstance(counts, BispectrumResult):
            raise TypeError('counts must be a BispectrumResult')
        if counts.Nmesh != tuple(int(n) for n in pm.Nmesh) or counts.BoxSize != tuple(float(x) for x in pm.BoxSize) \
                or counts.kedges.shape != ke.shape or \
                not (counts.kedges == ke).all() or counts.counts.shape != (len(tri),):
            raise ValueError('counts is not the BispectrumResult of this mesh and these kedges')

    be = backend.get()
    kt = torch.from_numpy(ke).to(be.device)
    tt = torch.from_numpy(tri).to(be.device)
    sums = _shell_sums(a, kt, nb, tt, int(deconv_pow), False)
    if counts is not None:
        cnt = counts.counts
    else:
        cnt = numpy.rint(_shell_sums(a, kt, nb, tt, 0, True))
    # P of a / W: power_spectrum divides the product a conj(a), so its exponent is twice the amplitude's
    pk = power_spectrum(a, ke, deconv_pow=2 * int(deconv_pow))
    return BispectrumResult(ke, tri.astype('i8'), sums, cnt, pk, pm.BoxSize, pm.Nmesh)
