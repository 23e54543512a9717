"""Interlaced painting: density spectra whose leading alias images cancel, formed on the device.

A mass-assignment window W suppresses the spectrum and aliases it: the spectrum of a painted mesh at k is the sum over
the images k + 2 pi n N / L of W times the true spectrum.  Deconvolution (``deconv_pow``, ``Transfer.compensation``)
undoes the suppression of the n = 0 term and nothing else.  Interlacing (Hockney & Eastwood 1981; Sefusatti et al. 2016;
what nbodykit paints with ``interlaced=True``) paints the particles again on a mesh displaced by a fraction of a cell and
averages the spectra with the phase that undoes the displacement.

Definition.  With ``r2c`` in the package's convention, w_d the circular frequency of a mode along axis d
(2 pi / N_d times the signed mode number, the Nyquist frequency negative, as ``ComplexField.x`` and nbodykit have it) and
A_j = r2c[paint with the transform ``pm.affine.shift(j / order)``]:

    paint_interlaced = (1 / order) sum_{j = 0}^{order - 1} exp(i (j / order) sum_d w_d) * A_j

The image n of a mode reaches A_j with the factor exp(-2 pi i (j / order) sum_d n_d) once the phase is undone, so the
average removes every image whose sum_d n_d is not a multiple of ``order`` and leaves the others as a plain paint has
them.  order = 2 is nbodykit's scheme: the images with odd sum_d n_d, the largest of them the six nearest, are gone.
order = 3 removes those with sum_d n_d not a multiple of 3.  order = 1 is ``paint(...).r2c()``.

With ``compensate=True`` the result is divided by prod_d sinc(w_d / 2)^p, p the native support of the window (1 NNB, 2
CIC, 3 TSC, 4 PCS): ``Transfer.compensation`` fused into the last combine.

One kernel (csrc/pmx_interlace.hip, include/pmesh_amd.h: pmx_phase_combine), one launch per further mesh:
acc = (a acc + b exp(i theta) in) / window.  The first mesh is painted and transformed into the result; every further
one is painted into one scratch real field, transformed in place there and combined into the result.  Memory: the
result and one scratch buffer.

Nyquist planes.  On an even mesh the mode N_d / 2 stands for +N_d / 2 and -N_d / 2 at once, whose phases differ
(exp(+-i pi / 2) for order 2): with the negative frequency taken for both, as in nbodykit, the combined spectrum is not
Hermitian-consistent on those planes, and ``c2r`` (``interlaced_field``) keeps of them what a complex-to-real transform
keeps: the real part of the self-conjugate modes.

    from pmesh_amd.interlace import paint_interlaced, interlaced_field
    delta_k = paint_interlaced(pm, pos, resampler='tsc', compensate=True)
    P = power_spectrum(delta_k, kedges)
    F = interlaced_field(pm, pos, mass=w)          # a RealField, for survey_multipoles

Not here: gradients (the adjoint of the combine is the same entry with ``-shift`` and exchanged roles; the composition
with paint_vjp is left to a follow-up, as it was for power, bispectrum and lpt); a paint kernel that deposits both
meshes from one read of the positions; any change to ``pm.paint``, ``power_spectrum`` or ``survey_multipoles``.
"""
import numpy

from . import backend
from . import fft as _fft
from .survey import _call

ORDERS = (1, 2, 3)
# window kinds whose transform is sinc^p at native support (pmx_fwindow): the B-splines NNB, CIC, TSC, PCS
_SINC_KINDS = range(0, 8)


def _same_mesh(a, b):
    return a is b or (tuple(a.Nmesh) == tuple(b.Nmesh) and tuple(a.BoxSize) == tuple(b.BoxSize) and a.comm is b.comm
                      and a.np == b.np)


def phase_combine(acc, other, shift, a=0.5, b=0.5, deconv_pow=0):
    """acc = (a * acc + b * exp(i sum_d shift_d w_d) * other) / prod_d sinc(w_d / 2)^deconv_pow, in place on `acc`.

    acc, other : ComplexFields of the same mesh and of the same kind (transposed or untransposed), in different
        buffers.
    shift : the displacement in cells the phase undoes, a number or one per axis.
    a, b : real weights; with a = 0 the values of `acc` are not read.
    deconv_pow : a non-negative integer, 0 for no division.

    Each rank works on its own block.  Returns `acc`."""
    from .pm import BaseComplexField
    if not (isinstance(acc, BaseComplexField) and isinstance(other, BaseComplexField)):
        raise TypeError('acc and other must be ComplexFields')
    pm = acc.pm
    if not _same_mesh(pm, other.pm) or tuple(acc.start) != tuple(other.start) or acc.shape != other.shape:
        raise ValueError('the two fields belong to different meshes')
    if acc.value.dtype != other.value.dtype:
        raise ValueError('the two fields must have the same dtype (%s vs %s)' % (acc.value.dtype, other.value.dtype))
    if int(deconv_pow) != deconv_pow or deconv_pow < 0:
        raise ValueError('deconv_pow must be a non-negative integer, not %r' % (deconv_pow,))
    try:
        s = numpy.empty(len(pm.Nmesh), dtype='f8')
        s[:] = shift
    except (TypeError, ValueError):
        raise ValueError('shift must be a number or one number per axis')
    if not numpy.isfinite(s).all():
        raise ValueError('shift must be finite')
    _call(backend.get().phase_combine, other.value, acc.value, acc.start, pm.Nmesh, s, a, b, int(deconv_pow))
    return acc


def _route_smoothing(resampler, order):
    """how far, in cells, a particle's window reaches on any of the displaced meshes"""
    return 0.5 * resampler.support + (order - 1.0) / order


def paint_interlaced(pm, pos, mass=1.0, resampler=None, order=2, compensate=False, layout=None, out=None, hsml=None):
    """The interlaced spectrum of the particles: see the module docstring.

    pm : a ParticleMesh of a 3-d or 2-d real mesh (f4 or f8), on one or several ranks.
    pos, mass : as for ``pm.paint``.
    resampler : the window, default ``pm.resampler``.
    order : 1, 2 or 3 meshes, displaced by j / order cells along every axis.
    compensate : divide by the window, prod_d sinc(w_d / 2)^nativesupport; refused for windows whose transform is
        not a power of sinc (lanczos, acg, wavelets, B-splines at another support than their own).
    layout : on several ranks, a layout of ``pm.decompose(pos, smoothing=s)`` with s at least
        ``0.5 * support + (order - 1) / order`` cells; default: built here.  Not needed on one rank.
    out : a ComplexField of `pm` (transposed or untransposed) for the result; default a new TransposedComplexField.
    hsml : not supported (a per-particle window has no common transform to cancel images of).

    Returns `out`.  Memory: the result and one scratch buffer."""
    from .pm import BaseComplexField, ParticleMesh, exchange
    from .transfer import Transfer
    from .window import FindResampler
    if not isinstance(pm, ParticleMesh):
        raise TypeError('pm must be a ParticleMesh, not %s' % type(pm).__name__)
    if len(pm.Nmesh) not in (2, 3):
        raise NotImplementedError('interlaced painting of %d-dimensional meshes: only 2-d and 3-d' % len(pm.Nmesh))
    if pm.dtype.kind == 'c':
        raise ValueError('interlaced painting needs a real mesh (dtype f4 or f8)')
    if hsml is not None:
        raise ValueError('interlaced painting does not take hsml')
    try:
        ok = int(order) == order and int(order) in ORDERS
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('order must be among %s, not %r' % (ORDERS, order))
    order = int(order)
    resampler = FindResampler(pm.resampler if resampler is None else resampler)
    p = 0
    if compensate:
        if resampler._k not in _SINC_KINDS or resampler.support != resampler.nativesupport:
            raise ValueError('compensate: the transform of window %r with support %s is not a power of sinc'
                             % (resampler.kind, resampler.support))
        p = resampler.nativesupport
    if out is not None and not (isinstance(out, BaseComplexField) and out.pm is pm):
        raise ValueError('out must be a ComplexField of pm')
    need = _route_smoothing(resampler, order)
    if layout is not None:
        route = getattr(layout, '_route', None)
        if route is None or not numpy.all(route[0] >= need) or \
                route[1] != tuple(float(x) for x in numpy.asarray(pm.affine.scale).ravel()):
            raise ValueError('the layout must come from pm.decompose(pos, smoothing=s) with s >= %g cells '
                             '(0.5 * support + (order - 1) / order)' % need)
    if pm.comm.size > 1:
        # every rank receives the particles whose window reaches its block on any of the meshes, once, and paints them
        # as its own (a displaced transform moves windows relative to the domains: the literal exchange of pm.paint)
        if layout is None:
            layout = pm.decompose(pos, smoothing=need)
        pos, mass = layout.exchange(pos), exchange(layout, mass)

    first = pm.paint(pos, mass=mass, resampler=resampler)
    out = first.r2c(out=out)
    if order == 1:
        if compensate:
            out.apply(Transfer.compensation(resampler), out=Ellipsis)
        return out
    # the real field of the first mesh is the scratch buffer of the others; each spectrum over it in the layout of `out`
    scratch = first
    # (an out-of-place transform leaves the halo merge of the first paint owed on its input, which nobody reads again)
    _fft.forget(scratch._base.storage)
    spec = type(out)(pm, base=scratch._base)
    for j in range(1, order):
        pm.paint(pos, mass=mass, resampler=resampler, transform=pm.affine.shift(j / float(order)), out=scratch)
        scratch.r2c(out=spec)
        last = j == order - 1
        # order 2: (A_0 + e A_1) / 2.  order 3: A_0 + e A_1, then (that + e A_2) / 3.
        w = 1.0 / order if last else 1.0
        phase_combine(out, spec, j / float(order), a=w, b=w, deconv_pow=p if last else 0)
    return out


def interlaced_field(pm, pos, mass=1.0, resampler=None, order=2, compensate=False, layout=None, out=None, hsml=None):
    """``paint_interlaced(...).c2r()``: the interlaced density as a RealField, for callers that start from one
    (``survey_multipoles``).  Arguments as for paint_interlaced; `out` is a ComplexField for the intermediate spectrum.

    On the Nyquist planes of even meshes the combined spectrum is not Hermitian-consistent (module docstring), as in
    nbodykit; ``c2r`` keeps of those modes what a complex-to-real transform keeps."""
    return paint_interlaced(pm, pos, mass=mass, resampler=resampler, order=order, compensate=compensate,
                            layout=layout, out=out, hsml=hsml).c2r()
