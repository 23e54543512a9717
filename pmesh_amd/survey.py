"""Survey power multipoles with a local line of sight, measured on the device.

The FFT form of the Yamamoto estimator (Bianchi et al. 2015, Scoccimarro 2015, Hand et al. 2017; what nbodykit's
``ConvolvedFFTPower`` computes) for data with an observer — a survey, a light cone, a mock: the real field is weighted
by spherical harmonics of the direction to each cell, transformed, and the transforms are summed against the harmonics
of the wavevector.

Mesh and field.  A 3-d mesh has ``Nmesh`` N_d and ``BoxSize`` L_d; F is a real field on it.

Cell position.  Cell g (global index, 0 <= g_d < N_d) sits at x_d = (g_d * L_d) / N_d, in double and in this order of
operations: the position ``paint`` assigns to that cell, not wrapped to negative values.

Direction.  ``origin`` is the observer, in the box coordinates of particle positions.  r = x - origin is never wrapped
periodically; r_hat = r / |r|.

Real orthonormal harmonics Y_lm, without the Condon-Shortley phase.  With
N_lm = sqrt((2l+1) / (4 pi) (l-|m|)! / (l+|m|)!) and P_l^m(c) = (1 - c^2)^(m/2) d^m P_l / dc^m:

    m = 0:  N_l0 P_l(cos th)
    m > 0:  sqrt2 N_lm P_l^m(cos th) cos(m ph)
    m < 0:  sqrt2 N_l|m| P_l^|m|(cos th) sin(|m| ph)

with cos th = z, ph = atan2(y, x) of the unit vector: Y_22 is proportional to +(x^2 - y^2), Y_21 to +xz, Y_2,-1 to
+yz.  For a zero vector (r = 0 or k = 0), Y_00 = 1 / sqrt(4 pi) and every Y_lm with l > 0 is 0.

The multipole field.  With ``r2c`` in the package's convention (divided by prod N, phase exp(-i k.x)):

    A_l(k) = (4 pi / (2l+1)) sum_m Y_lm(k_hat) * r2c[F * Y_lm(r_hat)](k)

By the addition theorem this is (1 / prod N) sum_x F(x) L_l(k_hat . r_hat) exp(-i k.x), with the Legendre polynomial
L_l taken as [l == 0] at k = 0 or r = 0.  A_0 = F.r2c().

The result.  P_l(bin) = (2l+1) * ``power_spectrum(A_0[field], kedges, other=A_l[other or field], deconv_pow=...)``.power,
that is (2l+1) V <A_0 conj(A_l)> with ``power_spectrum``'s bins, counts, Hermitian weighting and rank sum.

Even orders only: l in {0, 2, 4}.  For odd l, A_l is anti-Hermitian and the mirrored-mode rule of ``power_spectrum``
does not hold.

Two kernels (csrc/pmx_survey.hip, include/pmesh_amd.h): pmx_ylm_weight writes F * Y_lm(r_hat) into a scratch real
field, which is transformed in place, and pmx_ylm_accumulate adds (4 pi / (2l+1)) Y_lm(k_hat) times that spectrum to
A_l; 2l+1 such rounds per order.  Each rank weights and accumulates its own block.  Memory of ``multipole_field``: the
input, one scratch buffer (the real field and, in place, its spectrum) and A_l; ``survey_multipoles`` keeps A_0 as
well.

    from pmesh_amd.survey import survey_multipoles
    r = survey_multipoles(F, kedges, origin=[-1500., 0., 0.], poles=(0, 2, 4), deconv_pow=2)
    r.k, r.modes, r.poles[2], r.A0

Not here: gradients, odd orders, and the FKP normalisation and shot-noise terms (sums over catalogue columns: the
caller computes them and scales the result).  An interlaced field comes from ``pmesh_amd.interlace.interlaced_field``.
"""
import numpy

from . import _abi, backend
from .power import power_spectrum

ORDERS = (0, 2, 4)


class SurveyResult(object):
    """The binned multipoles: ``kedges``, ``k`` (mean |k|), ``modes`` (count) of ``power_spectrum``'s 1-d bins,
    ``poles`` (dict ell -> complex array, NaN in empty bins) and ``A0``, the spectrum of the field."""

    def __init__(self, kedges, k, modes, poles, A0):
        self.kedges, self.k, self.modes, self.poles, self.A0 = kedges, k, modes, poles, A0


def _real_field(name, field):
    from .pm import RealField
    if not isinstance(field, RealField):
        raise TypeError('%s must be a RealField, not %s' % (name, type(field).__name__))
    if len(field.pm.Nmesh) != 3:
        raise NotImplementedError('survey multipoles of %d-dimensional meshes: only 3-d meshes' % len(field.pm.Nmesh))
    if field.value.is_complex():
        raise ValueError('%s must belong to a real mesh (dtype f4 or f8)' % name)
    return field.pm


def _order(ell):
    try:
        ok = int(ell) == ell and int(ell) in ORDERS
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('multipole orders must be among %s (odd orders are anti-Hermitian), not %r' % (ORDERS, ell))
    return int(ell)


def _origin(origin):
    try:
        o = numpy.array(origin, dtype='f8').reshape(-1)
    except (TypeError, ValueError):
        raise ValueError('origin must be three finite numbers')
    if o.shape != (3,) or not numpy.isfinite(o).all():
        raise ValueError('origin must be three finite numbers')
    return [float(x) for x in o]


def _new(cls, pm):
    """a field the kernels are about to write all of (only the GPU backend hands out raw memory)"""
    from .pm import _blank
    return _blank(cls, pm) if backend.get().name == 'hip' else pm.create(type=cls)


def _call(fn, *args):
    try:
        fn(*args)
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise


def multipole_field(field, ell, origin, out=None):
    """A_l of the module docstring for the RealField `field` of a 3-d real mesh, as a ComplexField.

    ell : 0, 2 or 4.  ell = 0 is ``field.r2c()``, with no harmonic pass.
    origin : the observer, three finite numbers in box coordinates.
    out : a ComplexField of the same mesh (transposed or untransposed) to hold the result; default a new
        TransposedComplexField.

    `field` is left untouched.  Memory: the input, one scratch buffer and the result."""
    from .pm import BaseComplexField, RealField, TransposedComplexField
    pm = _real_field('field', field)
    ell = _order(ell)
    org = _origin(origin)
    if out is not None and not (isinstance(out, BaseComplexField) and out.pm is pm):
        raise ValueError('out must be a ComplexField of the mesh of field')
    if ell == 0:
        return field.r2c(out=out)
    be = backend.get()
    if out is None:
        out = _new(TransposedComplexField, pm)
    scratch = _new(RealField, pm)
    # the spectrum of the scratch field over the scratch field's own buffer, in the layout of `out`
    spec = type(out)(pm, base=scratch._base)
    for n, m in enumerate(range(-ell, ell + 1)):
        _call(be.ylm_weight, ell, m, field.value, scratch.value, field.start, pm.Nmesh, pm.BoxSize, org)
        scratch.r2c(out=spec)
        _call(be.ylm_accumulate, ell, m, int(n > 0), spec.value, out.value, out.start, pm.Nmesh, pm.BoxSize)
    return out


def survey_multipoles(field, kedges, origin, poles=ORDERS, other=None, deconv_pow=0):
    """The power multipoles of `field` about the local line of sight from `origin`: see the module docstring.

    field : RealField of a 3-d real mesh (f4 or f8), on one or several ranks.
    kedges : Nk + 1 strictly increasing |k| edges, as for power_spectrum.
    origin : the observer, three finite numbers in box coordinates (it may lie outside the box).
    poles : distinct orders among 0, 2, 4.
    other : a second RealField of the same mesh, for cross spectra: A_0 is taken from `field`, A_l from `other`.
    deconv_pow : power_spectrum's window compensation of the product A_0 conj(A_l).

    Returns a SurveyResult.  A_0 is formed once; each A_l is formed, binned by one cross power_spectrum call and
    released before the next."""
    pm = _real_field('field', field)
    if other is not None:
        pmo = _real_field('other', other)
        if pmo is not pm and (tuple(pmo.Nmesh) != tuple(pm.Nmesh) or tuple(pmo.BoxSize) != tuple(pm.BoxSize)
                              or pmo.comm is not pm.comm):
            raise ValueError('the two fields belong to different meshes')
        if other.value.dtype != field.value.dtype:
            raise ValueError('the two fields must have the same dtype (%s vs %s)' % (field.value.dtype, other.value.dtype))
    try:
        ells = [_order(ell) for ell in poles]
    except TypeError:
        raise ValueError('poles must be a sequence of orders among %s' % (ORDERS,))
    if len(set(ells)) != len(ells):
        raise ValueError('poles must be distinct orders among %s' % (ORDERS,))
    org = _origin(origin)
    src = field if other is None else other

    A0 = field.r2c()
    result = {}
    first = None
    for ell in ells:
        if ell == 0 and other is None:
            Al = A0
        else:
            Al = multipole_field(src, ell, org)
        r = power_spectrum(A0, kedges, other=Al, deconv_pow=deconv_pow)
        del Al
        result[ell] = (2 * ell + 1) * r.power
        first = first or r
    if first is None:
        first = power_spectrum(A0, kedges, deconv_pow=deconv_pow)      # the bins alone
    return SurveyResult(first.kedges, first.k, first.modes, result, A0)
