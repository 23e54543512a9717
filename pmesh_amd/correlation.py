"""Binned correlation function: xi(r), xi(r, mu) and multipoles, measured on the device.

What nbodykit's FFTCorr computes next to FFTPower: ``a conj(b)`` transformed back and the real mesh binned by
``RealField.x``.  A caller of the reference forms the product as mesh-sized temporaries and bins with a slab loop of
numpy.digitize + bincount; here one streaming kernel forms the product (pmx_spectral_product), the inverse transform
runs in place, and one kernel bins the real mesh in one read (pmx_corr_project; csrc/pmx_corr.hip,
include/pmesh_amd.h).  The same pass bins any real mesh by separation (``bin_real``), e.g. the window multipoles
Q_l(r) of a survey's randoms.

Definition, for a 1-, 2- or 3-d real mesh (f4 or f8) with the spectra a and b (b = a: the auto correlation):

1. ``S = a conj(b) / prod_d sinc(w_d / 2)^deconv_pow``.
2. ``xi = c2r(S)``: with pmesh's normalisation xi(x) is the mean over y of A(y + x) B(y).  The k = 0 mode is kept;
   removing the mean is the caller's business.
3. Per cell, in double: ``r_d = (s_d * L_d) / N_d`` with the global index s_d counted negative at and beyond
   ``N_d // 2`` — exactly ``RealField.x`` of an f8 mesh — ``|r| = sqrt((r_0^2 + r_1^2) + r_2^2)`` and
   ``mu = ((r_0 los_0 + r_1 los_1) + r_2 los_2) / |r|``, 0 at r = 0.
4. r bins follow numpy.digitize (``redges[j] <= |r| < redges[j + 1]``, outside dropped); mu bins too, the last one
   closed on the right.  Every cell has weight 1: there is no Hermitian doubling on the real side.
5. Raw sums per r bin ``[count, sum |r|, sum x, sum x L_l(mu) per pole]`` and per (r, mu) cell ``[count, sum |r|,
   sum mu, sum x]`` are added over the ranks first, then divided: ``xi_l(r) = (2l + 1) sum x L_l / count``.  Empty bins
   hold NaN.

    from pmesh_amd.correlation import correlation_function
    r = correlation_function(delta, redges=numpy.arange(0, 150., 5.), muedges=numpy.linspace(-1, 1, 11), poles=(0, 2, 4))
    r.r, r.modes, r.corr, r.poles[2], r.corr2d
"""
import numpy
import torch

from . import backend
from .power import (_Binning, _Result, _blank_like, _jvp_terms, _ndim, _same_layout, _same_mesh,
                    _unsupported_is_value_error)


class CorrResult(_Result):
    """The binned mesh.  1-d bins (Nr): ``redges``, ``r`` (mean |r|), ``modes`` (count), ``corr`` (real), ``poles``
    (dict ell -> real array).  (r, mu) bins (Nr x Nmu), None without ``muedges``: ``muedges``, ``r2d``, ``mu2d``,
    ``modes2d``, ``corr2d``.  Means are sums over the count; empty bins hold NaN."""
    _x, _v, _width = 'r', 'corr', 1


class _Bins(_Binning):
    """the checked binning of a real mesh of `pm`"""

    def __init__(self, pm, redges, muedges, los, poles):
        _Binning.__init__(self, _ndim(pm, 'correlation functions'), 'redges', redges, muedges, los, poles, CorrResult,
                          comm=pm.comm)
        self.pm = pm

    def sums(self, field):
        """the raw sums of pmx_corr_project for the RealField `field`"""
        return _Binning.sums(self, lambda acc: backend.get().corr_project(
            self.p, field.value, field.start, self.pm.Nmesh, self.pm.BoxSize, self.et, self.mt, acc))

    def measure(self, field):
        return self.unpack(self.sums(field))

    def measure_zero(self, like):
        """the counts and means of the binning alone: they depend on the geometry, the projection of any mesh has them"""
        zero = _blank_like(like, 'real')
        zero.value[...] = 0
        return self.measure(zero)


def _real(field):
    from .pm import RealField
    if not isinstance(field, RealField):
        raise TypeError('bin_real bins RealField objects, not %s' % type(field).__name__)
    if field.value.dtype not in (torch.float32, torch.float64):
        raise ValueError('bin_real bins float32 or float64 meshes (complex-to-complex meshes are not supported)')
    return field


def bin_real(field, redges, muedges=None, los=None, poles=()):
    """The RealField `field` binned by the separation |r| (and mu, and in multipoles) of its cells: steps 3 to 5 of the
    module docstring on any real mesh; a CorrResult.

    redges : Nr + 1 strictly increasing |r| edges (Nr <= PMX_POWER_MAX_KBINS).
    muedges : Nmu + 1 increasing edges in [-1, 1] (Nmu <= PMX_POWER_MAX_MUBINS), or None for no (r, mu) table.
    los : line of sight (normalised here); default the last axis.
    poles : multipole orders, each in 0..PMX_POWER_MAX_ELL, at most PMX_POWER_MAX_POLES of them.
    """
    field = _real(field)
    return _Bins(field.pm, redges, muedges, los, poles).measure(field)


# ---- the correlation mesh --------------------------------------------------------------------------------------------

def _pair(field, other, deconv_pow, real_ok):
    """the spectra (a, b or None) of the arguments, checked, and whether each is a temporary of this call"""
    from .pm import RealField, BaseComplexField

    def spectrum(f):
        if isinstance(f, RealField):
            if not real_ok:
                raise TypeError('the gradients of correlation_function take ComplexField objects: transform the '
                                'RealField with r2c and back-propagate through it with r2c_vjp')
            if f.value.is_complex():
                raise ValueError('correlation functions of complex-to-complex meshes are not supported')
            return f.r2c(), True                  # a new spectrum: the caller's field is left as it is
        if not isinstance(f, BaseComplexField):
            raise TypeError('correlation_function measures RealField or ComplexField objects, not %s'
                            % type(f).__name__)
        if not f.compressed:
            raise ValueError('correlation functions of complex-to-complex meshes are not supported')
        return f, False
    if int(deconv_pow) != deconv_pow or deconv_pow < 0:
        raise ValueError('deconv_pow must be a non-negative integer')
    if getattr(field, 'pm', None) is not None:
        _ndim(field.pm, 'correlation functions')
    a, mine_a = spectrum(field)
    b, mine_b = None, False
    if other is not None:
        b, mine_b = spectrum(other)
        _same_mesh(a, b)
        _same_layout(a, b)
    return a, b, mine_a, mine_b


def _product(x, y, out, conj_y=False, accumulate=False, deconv_pow=0):
    backend.get().spectral_product(x.value, y.value, out.value, x.start, x.pm.Nmesh, 1.0, conj_y, accumulate, deconv_pow)
    return out


def _to_real(spec, out):
    """c2r of the scratch spectrum `spec`: in place (the result over its buffer) unless the caller gave a field"""
    from .pm import RealField
    if out is None:
        return spec.c2r(out=Ellipsis)
    if not isinstance(out, RealField) or (out.pm is not spec.pm and tuple(out.pm.Nmesh) != tuple(spec.pm.Nmesh)) \
            or out.value.dtype != spec.value.real.dtype:
        raise ValueError('out must be a RealField of the mesh and dtype of the fields')
    return spec.c2r(out=out)


def correlation_field(field, other=None, deconv_pow=0, out=None):
    """The RealField xi of steps 1 and 2 of the module docstring.

    field, other : RealField (r2c'd into a temporary, the caller's field untouched) or compressed ComplexField of one
        ParticleMesh and one layout; 1, 2 or 3 dimensions, f4 or f8.  A complex-to-complex mesh raises ValueError.
    deconv_pow : divide the product by prod_d sinc(w_d / 2)^deconv_pow (window compensation).
    out : a RealField for the result; default a new one over the scratch spectrum (transformed in place), so that the
        memory of the call is the result plus, with `out`, one spectrum-sized scratch.
    """
    a, b, mine_a, mine_b = _pair(field, other, deconv_pow, True)
    # the product goes into a temporary of this call where there is one, else into a new spectrum
    scratch = a if mine_a else (b if mine_b else _blank_like(a))
    _product(a, b if b is not None else a, scratch, conj_y=True, deconv_pow=int(deconv_pow))
    return _to_real(scratch, out)


def correlation_function(field, redges, other=None, muedges=None, los=None, poles=(), deconv_pow=0):
    """The binned auto (other None) or cross correlation function of `field` (and `other`): see the module docstring.
    ``bin_real(correlation_field(field, other, deconv_pow), redges, muedges, los, poles)``."""
    from .pm import Field
    if not isinstance(field, Field):
        raise TypeError('correlation_function measures RealField or ComplexField objects, not %s'
                        % type(field).__name__)
    bins = _Bins(field.pm, redges, muedges, los, poles)         # (the binning is checked before anything is computed)
    return bins.measure(correlation_field(field, other, deconv_pow))


# ---- gradients -----------------------------------------------------------------------------------------------------

def correlation_function_vjp(field, redges, v_corr=None, v_poles=None, v_corr2d=None, other=None, muedges=None,
                             los=None, poles=(), deconv_pow=0, result=None):
    """The gradient of L = sum v xi, summed over ``corr``, every ``poles[ell]`` and ``corr2d`` of
    ``correlation_function(field, redges, other, muedges, los, poles, deconv_pow)``, with respect to the field(s).

    With g the adjoint of the projection (pmx_corr_vjp: per cell the coefficients v / count, and (2l + 1) v / count for
    the poles, of its bin) and G = RealField.c2r_vjp(g): grad_a = G b / D and grad_b = a conj(G) / D, D the window;
    for the auto correlation both terms go into one field.  The products are pmx_spectral_product calls.

    field, other : compressed ComplexField objects (a RealField raises TypeError: go through r2c_vjp).
    v_corr : Nr real values, v_poles : dict ell -> Nr values (keys among `poles`), v_corr2d : (Nr, Nmu) values (needs
        muedges); None counts as zero, and empty bins (NaN in the forward) contribute nothing.  ``r``, ``mu2d`` and the
        counts are piecewise constant and have no gradient.
    result : the CorrResult of the same arguments, for its counts; without it they come from one projection.

    Returns grad_field (other None) or (grad_field, grad_other) in the convention of power_spectrum_vjp:
    ``Re(u.cdot(grad))`` is the derivative of L along u.
    """
    a, b, _, _ = _pair(field, other, deconv_pow, False)
    pm = a.pm
    bins = _Bins(pm, redges, muedges, los, poles)
    coef = bins.coefficients(v_corr, v_poles, v_corr2d, result, lambda: bins.measure_zero(a), real=True)
    g = _blank_like(a, 'real')
    _unsupported_is_value_error(backend.get().corr_vjp, bins.p, g.value, g.start, pm.Nmesh, pm.BoxSize, bins.et, bins.mt,
                                coef)
    from .lpt import _spectrum_of
    G = _spectrum_of(g, a)                                     # r2c over g's own buffer, in the layout of a
    G.value[...] *= float(numpy.prod(pm.Nmesh ** 1.0))         # (RealField.c2r_vjp)
    dp = int(deconv_pow)
    ga = _blank_like(a)
    _product(G, b if b is not None else a, ga, deconv_pow=dp)
    if b is None:
        return _product(a, G, ga, conj_y=True, accumulate=True, deconv_pow=dp)
    return ga, _product(a, G, G, conj_y=True, deconv_pow=dp)   # grad_b over the buffer of G


def correlation_function_jvp(field, redges, v_field=None, v_other=None, other=None, muedges=None, los=None, poles=(),
                             deconv_pow=0):
    """The tangent of correlation_function along v_field (and v_other): a CorrResult whose ``corr``, ``poles`` and
    ``corr2d`` are tangents and whose ``r``, ``modes``, ``r2d``, ``mu2d`` and ``modes2d`` are the forward's.

    xi is bilinear in (a, b): the tangent mesh is c2r((da conj(b) + a conj(db)) / D) — two product calls, the second
    accumulating, one c2r and one projection (for the auto correlation b = a and db = da).
    v_field, v_other : ComplexField objects of the fields' layout; None counts as zero."""
    a, b, _, _ = _pair(field, other, deconv_pow, False)
    terms = _jvp_terms(a, b, v_field, v_other, lambda v: _pair(v, None, 0, False)[0])
    bins = _Bins(a.pm, redges, muedges, los, poles)
    if not terms:
        return bins.measure_zero(a)                             # the forward's counts and means, zero tangents
    scratch = _blank_like(a)
    for n, (x, y) in enumerate(terms):
        _product(x, y, scratch, conj_y=True, accumulate=n > 0, deconv_pow=int(deconv_pow))
    return bins.measure(scratch.c2r(out=Ellipsis))
