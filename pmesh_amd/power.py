"""Binned power spectrum of complex fields: P(k), P(k, mu) and multipoles, measured on the device.

The reference measured spectra with TransferFunction.PowerSpectrum (pmesh/transfer.py:133-181), a slab loop of
numpy.digitize + bincount; callers such as nbodykit's FFTPower do the same on a painted density.  Here one kernel
(csrc/pmx_power.hip, include/pmesh_amd.h: pmx_power_project) reads the local block of the field once, recomputes
every wavenumber from its index and adds per-bin sums into a small float64 vector; on several ranks the vectors are
summed over ``pm.comm`` and only then divided.

Per stored mode, in double: k_d as ``ComplexField.x`` of an f8 mesh, |k| = sqrt((k_0^2 + k_1^2) + k_2^2),
mu = k . los / |k| (0 at k = 0), v = V a conj(b) / prod_d sinc(w_d / 2)^deconv_pow with V = prod(BoxSize).  A mode of a
compressed (r2c) spectrum whose last-axis index is neither 0 nor N // 2 stands for itself and its conjugate: weight 1 at
(|k|, mu) with v and weight 1 at (|k|, -mu) with conj(v) — so the modes-weighted power of the 1-d bins adds up to
V * ``cnorm()``.  k bins follow numpy.digitize (``kedges[j] <= |k| < kedges[j + 1]``, outside dropped); mu bins too,
the last one closed on the right.  Multipoles: P_ell(k) = (2 ell + 1) sum w v L_ell(mu) / sum w.

    from pmesh_amd.power import power_spectrum
    r = power_spectrum(delta_k, kedges=numpy.arange(0, kmax, kf), muedges=numpy.linspace(-1, 1, 11), poles=(0, 2, 4))
    r.k, r.modes, r.power, r.poles[2], r.power2d
"""
import numpy
import torch

from . import _abi, backend


class _Result(object):
    """The binned statistic unpacked from the raw sums `acc` of the tile kernels: per bin ``[count, sum |x|, sum v,
    sum v L_ell per pole]``, then per (bin, mu) cell ``[count, sum |x|, sum mu, sum v]``, every v of ``_width`` columns
    ((re, im) pairs of the complex power, one real column of the correlation).  A subclass names |x| (``_x``: the
    attributes x, xedges, x2d) and v (``_v``: v, v2d)."""

    def __init__(self, edges, muedges, acc, ells):
        w = self._width
        nb = len(edges) - 1
        s1 = 2 + w * (1 + len(ells))

        def v(a, i):
            return a[..., i] + 1j * a[..., i + 1] if w == 2 else a[..., i]
        a1 = acc[:nb * s1].reshape(nb, s1)
        setattr(self, self._x + 'edges', edges)
        self.muedges = muedges
        with numpy.errstate(invalid='ignore', divide='ignore'):
            n = a1[:, 0]
            self.modes = numpy.rint(n).astype('i8')
            setattr(self, self._x, a1[:, 1] / n)
            setattr(self, self._v, v(a1, 2) / n)
            self.poles = {ell: (2 * ell + 1) * v(a1, 2 + w * (1 + p)) / n for p, ell in enumerate(ells)}
            self.mu2d = self.modes2d = None
            setattr(self, self._x + '2d', None)
            setattr(self, self._v + '2d', None)
            if muedges is not None:
                a2 = acc[nb * s1:].reshape(nb, len(muedges) - 1, 3 + w)
                n2 = a2[..., 0]
                self.modes2d = numpy.rint(n2).astype('i8')
                setattr(self, self._x + '2d', a2[..., 1] / n2)
                self.mu2d = a2[..., 2] / n2
                setattr(self, self._v + '2d', v(a2, 3) / n2)


class PowerResult(_Result):
    """The binned spectrum.  1-d bins (Nk): ``kedges``, ``k`` (mean |k|), ``modes`` (count), ``power`` (complex),
    ``poles`` (dict ell -> complex array).  (k, mu) bins (Nk x Nmu), None without ``muedges``: ``muedges``, ``k2d``,
    ``mu2d``, ``modes2d``, ``power2d``.  Means are weighted sums over the count; empty bins hold NaN."""
    _x, _v, _width = 'k', 'power', 2


def _edges(name, edges, lo=None, hi=None):
    e = numpy.array(edges, dtype='f8')
    if e.ndim != 1 or len(e) < 2:
        raise ValueError('%s must be a 1-d array of at least 2 edges' % name)
    if not numpy.isfinite(e).all() or not (numpy.diff(e) > 0).all():
        raise ValueError('%s must be finite and strictly increasing' % name)
    if lo is not None and (e[0] < lo or e[-1] > hi):
        raise ValueError('%s must lie in [%g, %g]' % (name, lo, hi))
    return e


def _complex(field):
    from .pm import RealField, BaseComplexField
    if isinstance(field, RealField):
        return field.r2c()                     # a new spectrum: the caller's field is left as it is
    if not isinstance(field, BaseComplexField):
        raise TypeError('power_spectrum measures RealField or ComplexField objects, not %s' % type(field).__name__)
    return field


def _ndim(pm, what):
    ndim = len(pm.Nmesh)
    if ndim > _abi.PMX_MAXDIM:
        raise NotImplementedError('%s of meshes of more than %d dimensions' % (what, _abi.PMX_MAXDIM))
    return ndim


class _Binning(object):
    """The binning of one two-point statistic on a mesh of ndim dimensions, checked: the edges `name` (kedges; redges
    on the real side) and mu edges (or None) on the host (``edges``, ``me``) and on the device (``et``, ``mt``), the
    multipole orders ``ells``, the filled pmx_power struct ``p`` with the unit line of sight, and the widths of the
    tables the kernels keep per bin and per (bin, mu) cell: ``s1``, ``s2`` doubles of sums and ``c1``, ``c2`` of
    adjoint coefficients.  `result` is the _Result class of the statistic; comm: the ranks whose sums are added."""

    def __init__(self, ndim, name, edges, muedges, los, poles, result, hermitian=0, deconv_pow=0, volume=1.0, comm=None):
        e = _edges(name, edges)
        if len(e) - 1 > _abi.PMX_POWER_MAX_KBINS:
            raise ValueError('%d %s bins: more than PMX_POWER_MAX_KBINS = %d'
                             % (len(e) - 1, name[0], _abi.PMX_POWER_MAX_KBINS))
        me = None
        if muedges is not None:
            me = _edges('muedges', muedges, -1.0, 1.0)
            if len(me) - 1 > _abi.PMX_POWER_MAX_MUBINS:
                raise ValueError('%d mu bins: more than PMX_POWER_MAX_MUBINS = %d'
                                 % (len(me) - 1, _abi.PMX_POWER_MAX_MUBINS))
        ells = [int(ell) for ell in poles]
        if len(ells) > _abi.PMX_POWER_MAX_POLES:
            raise ValueError('%d multipoles: more than PMX_POWER_MAX_POLES = %d' % (len(ells), _abi.PMX_POWER_MAX_POLES))
        if len(set(ells)) != len(ells) or any(ell < 0 or ell > _abi.PMX_POWER_MAX_ELL for ell in ells):
            raise ValueError('poles must be distinct orders in 0..PMX_POWER_MAX_ELL = %d' % _abi.PMX_POWER_MAX_ELL)
        if los is None:
            los = numpy.zeros(ndim)
            los[-1] = 1.0
        los = numpy.array(los, dtype='f8').reshape(-1)
        norm = numpy.sqrt((los ** 2).sum())
        if len(los) != ndim or not numpy.isfinite(norm) or norm == 0:
            raise ValueError('los must be a nonzero vector of %d components' % ndim)
        if int(deconv_pow) != deconv_pow or deconv_pow < 0:
            raise ValueError('deconv_pow must be a non-negative integer')

        p = _abi.Power()
        p.nk = len(e) - 1
        p.nmu = 0 if me is None else len(me) - 1
        p.npoles = len(ells)
        for i, ell in enumerate(ells):
            p.poles[i] = ell
        p.hermitian = int(hermitian)
        p.deconv_pow = int(deconv_pow)
        p.volume = float(volume)
        for d in range(ndim):
            p.los[d] = float(los[d] / norm)

        self.p, self.edges, self.me, self.ells, self.result, self.comm = p, e, me, ells, result, comm
        w = result._width
        self.c1, self.c2 = w * (1 + len(ells)), w
        self.s1, self.s2 = 2 + self.c1, 3 + self.c2
        dev = backend.get().device
        self.et = torch.from_numpy(e).to(dev)
        self.mt = torch.from_numpy(me).to(dev) if me is not None else None

    def zeros(self):
        """the accumulator of the forward kernels, on the device"""
        p = self.p
        return torch.zeros(p.nk * self.s1 + p.nk * p.nmu * self.s2, dtype=torch.float64, device=backend.get().device)

    def unpack(self, acc):
        return self.result(self.edges, self.me, acc, self.ells)

    def sums(self, call):
        """the raw sums `call(acc)` adds into a zeroed accumulator, summed over the ranks: a host vector"""
        acc = self.zeros()
        _unsupported_is_value_error(call, acc)
        # one sum over the ranks of the raw sums, then the division
        if self.comm is not None and self.comm.size > 1:
            acc = self.comm.allreduce(acc)
        return acc.cpu().numpy()

    def coefficients(self, v, v_poles, v2d, result, forward, real=False):
        """The coefficient table of the adjoint kernels on the device, in acc's layout without the count, |x| and mu
        columns: v / count per bin, (2l + 1) v_poles[l] / count per pole, v2d / count per cell, zero in empty bins.
        The cotangents are named after the statistic (v_power, v_corr2d); real: they must be.  result: the forward's
        _Result for its counts, or None for the one `forward()` returns."""
        nb, nmu, ells, name = self.p.nk, self.p.nmu, self.ells, self.result._v

        def cotangent(what, x, shape):
            x = _cotangent(what, x, shape)
            if real and (x.imag != 0).any():
                raise ValueError('%s must be real: the correlation function is' % what)
            return x.real if real else x
        if v2d is not None and self.me is None:
            raise ValueError('v_%s2d needs muedges' % name)
        v_poles = dict(v_poles) if v_poles else {}
        unknown = [ell for ell in v_poles if ell not in ells]
        if unknown:
            raise ValueError('v_poles has orders %s that are not among poles %s' % (unknown, ells))
        cols = [cotangent('v_' + name, v, (nb,))]
        cols += [(2 * ell + 1) * cotangent('v_poles[%d]' % ell, v_poles.get(ell), (nb,)) for ell in ells]
        v2 = cotangent('v_%s2d' % name, v2d, (nb, nmu)) if nmu else None

        if result is None:
            result = forward()
        elif tuple(result.modes.shape) != (nb,) or (nmu > 0) != (result.modes2d is not None) or \
                (nmu and tuple(result.modes2d.shape) != (nb, nmu)):
            raise ValueError('result is not the %s of these arguments' % self.result.__name__)

        def table(x, count):
            x = x * numpy.where(count > 0, 1.0 / numpy.maximum(count, 1), 0.0)
            return x.real if real else numpy.stack([x.real, x.imag], axis=-1)
        coef = numpy.concatenate([numpy.stack([table(c, result.modes) for c in cols], axis=1).reshape(-1)]
                                 + ([table(v2, result.modes2d).reshape(-1)] if nmu else []))
        return torch.from_numpy(coef).to(backend.get().device)


def _unsupported_is_value_error(call, *args):
    """call(*args); what the native library does not support is the caller's ValueError"""
    try:
        return call(*args)
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise


class _Plan(_Binning):
    """the checked arguments of one spectrum: the fields (a, b or None) and their binning"""

    def __init__(self, field, kedges, other, muedges, los, poles, deconv_pow, convert=_complex):
        a = convert(field)
        pm = a.pm
        ndim = _ndim(pm, 'power spectra')
        b = None
        if other is not None:
            b = convert(other)
            _same_mesh(a, b)
            _same_layout(a, b)
        if a.value.dtype not in (torch.complex64, torch.complex128):
            raise ValueError('power_spectrum measures complex64 or complex128 fields')
        _Binning.__init__(self, ndim, 'kedges', kedges, muedges, los, poles, PowerResult, bool(a.compressed), deconv_pow,
                          numpy.prod(pm.BoxSize), pm.comm)
        self.a, self.b, self.pm = a, b, pm

    def sums(self, a, b):
        """the raw sums of pmx_power_project for the fields a and b (None: a) of this plan's layout"""
        return _Binning.sums(self, lambda acc: backend.get().power_project(
            self.p, a.value, b.value if b is not None else None, a.start, self.pm.Nmesh, self.pm.BoxSize, self.et,
            self.mt, acc))



def _same_mesh(a, b):
    if b.pm is not a.pm and (tuple(b.pm.Nmesh) != tuple(a.pm.Nmesh) or tuple(b.pm.BoxSize) != tuple(a.pm.BoxSize)
                             or b.pm.comm is not a.pm.comm):
        raise ValueError('the two fields belong to different meshes')


def _same_layout(a, b):
    if type(b) is not type(a) or tuple(b.start) != tuple(a.start) or tuple(b.value.shape) != tuple(a.value.shape) \
            or b.value.dtype != a.value.dtype:
        raise ValueError('the two fields must have the same layout and dtype (%s %s vs %s %s)'
                         % (type(a).__name__, a.value.dtype, type(b).__name__, b.value.dtype))


def power_spectrum(field, kedges, other=None, muedges=None, los=None, poles=(), deconv_pow=0):
    """The binned auto (other None) or cross power spectrum of `field` (and `other`): see the module docstring.

    field, other : ComplexField of one ParticleMesh and one layout (transposed, untransposed, compressed r2c or full
        c2c), or RealField (r2c'd into a temporary); 1, 2 or 3 dimensions, complex64 or complex128.
    kedges : Nk + 1 strictly increasing |k| edges (Nk <= PMX_POWER_MAX_KBINS).
    muedges : Nmu + 1 increasing edges in [-1, 1] (Nmu <= PMX_POWER_MAX_MUBINS), or None for no (k, mu) table.
    los : line of sight (normalised here); default the last axis.
    poles : multipole orders, each in 0..PMX_POWER_MAX_ELL, at most PMX_POWER_MAX_POLES of them.
    deconv_pow : divide v by prod_d sinc(w_d / 2)^deconv_pow (window compensation).
    """
    plan = _Plan(field, kedges, other, muedges, los, poles, deconv_pow)
    return plan.unpack(plan.sums(plan.a, plan.b))


# ---- gradients -----------------------------------------------------------------------------------------------------

def _complex_only(field):
    from .pm import RealField, BaseComplexField
    if isinstance(field, RealField):
        raise TypeError('the gradients of power_spectrum take ComplexField objects: transform the RealField with r2c '
                        'and back-propagate through it with r2c_vjp')
    if not isinstance(field, BaseComplexField):
        raise TypeError('power_spectrum measures RealField or ComplexField objects, not %s' % type(field).__name__)
    return field


def _cotangent(name, v, shape):
    """a cotangent as a complex array of `shape` (None: zeros)"""
    if v is None:
        return numpy.zeros(shape, dtype='c16')
    v = numpy.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    if v.shape != tuple(shape):
        raise ValueError('%s must have the shape %s of its spectrum, not %s' % (name, tuple(shape), v.shape))
    return v.astype('c16')


def power_spectrum_vjp(field, kedges, v_power=None, v_poles=None, v_power2d=None, other=None, muedges=None, los=None,
                       poles=(), deconv_pow=0, result=None):
    """The gradient of L = Re sum conj(v) P, summed over ``power``, every ``poles[ell]`` and ``power2d`` of
    ``power_spectrum(field, kedges, other, muedges, los, poles, deconv_pow)``, with respect to the field(s): one kernel
    (csrc/pmx_power_grad.hip, include/pmesh_amd.h: pmx_power_vjp), one read of each field and one write of each
    gradient.

    field, other : ComplexField objects as for power_spectrum (a RealField raises TypeError: go through r2c_vjp).
    v_power : Nk real or complex values, v_poles : dict ell -> Nk values (keys among `poles`), v_power2d : (Nk, Nmu)
        values (needs muedges); None counts as zero, and empty bins (NaN in the forward) contribute nothing.  ``k``,
        ``mu2d`` and the counts are piecewise constant and have no gradient.
    result : the PowerResult of the same arguments, for its counts; without it they come from one forward call.

    Returns grad_field (other None) or (grad_field, grad_other): fields of the inputs' type in the form of lpt_vjp
    and of RealField.c2r_vjp before decompress_vjp: ``Re(u.cdot(grad))`` is the derivative of L along u.
    """
    plan = _Plan(field, kedges, other, muedges, los, poles, deconv_pow, convert=_complex_only)
    a, b, pm = plan.a, plan.b, plan.pm
    coef = plan.coefficients(v_power, v_poles, v_power2d, result, lambda: plan.unpack(plan.sums(a, b)))
    ga = _blank_like(a)
    gb = _blank_like(b) if b is not None else None
    _unsupported_is_value_error(backend.get().power_vjp, plan.p, a.value, b.value if b is not None else None, ga.value,
                                gb.value if gb is not None else None, a.start, pm.Nmesh, pm.BoxSize, plan.et, plan.mt,
                                coef)
    return ga if b is None else (ga, gb)


def _blank_like(f, cls=None):
    """a new field of f's mesh, of f's type or of `cls`; raw memory on the device, where the kernels write every
    element of it (only the GPU backend hands out raw memory)"""
    from .pm import _blank, _typestr_to_type
    cls = _typestr_to_type(cls) if cls is not None else type(f)
    return _blank(cls, f.pm) if backend.get().name == 'hip' and f.value.numel() else f.pm.create(type=cls)


def _jvp_terms(a, b, v_field, v_other, check):
    """The pairs (x, y) whose bilinear statistics add up to the tangent of the statistic of (a, b or a) along v_field
    (and v_other), each checked by `check` and against a's layout: (da, b), (a, db) and, for the auto statistic, the
    second half (a, da).  Empty without tangents: the caller measures the forward's counts alone."""
    if v_other is not None and b is None:
        raise ValueError('v_other needs other')
    terms = []
    for v, first in ((v_field, True), (v_other, False)):
        if v is None:
            continue
        v = check(v)
        _same_layout(a, v)
        terms.append((v, b if b is not None else a) if first else (a, v))
    if b is None and terms:
        terms.append((a, terms[0][0]))
    return terms


def power_spectrum_jvp(field, kedges, v_field=None, v_other=None, other=None, muedges=None, los=None, poles=(),
                       deconv_pow=0):
    """The tangent of power_spectrum along v_field (and v_other): a PowerResult whose ``power``, ``poles`` and
    ``power2d`` are tangents and whose ``k``, ``modes``, ``k2d``, ``mu2d`` and ``modes2d`` are the forward's.

    The raw sums are bilinear in (a, b), so the tangent of every power-like column is acc(da, b) + acc(a, db): two
    cross calls of the forward kernel, divided by the forward's counts (for the auto spectrum b = a and db = da).
    v_field, v_other : ComplexField objects of the fields' layout; None counts as zero."""
    plan = _Plan(field, kedges, other, muedges, los, poles, deconv_pow, convert=_complex_only)
    a, b = plan.a, plan.b
    terms = _jvp_terms(a, b, v_field, v_other, _complex_only) or [(a, b)]    # (a, b): for the counts alone
    accs = [plan.sums(x, y) for x, y in terms]
    acc = sum(accs)
    # counts, |k| and mu sums are the same in every term: the forward's
    nk, s1, nmu = plan.p.nk, plan.s1, plan.p.nmu
    t1 = acc[:nk * s1].reshape(nk, s1)
    t1[:, :2] /= len(accs)
    if nmu:
        t2 = acc[nk * s1:].reshape(nk, nmu, 5)
        t2[..., :3] /= len(accs)
    if v_field is None and v_other is None:
        t1[:, 2:] = 0
        if nmu:
            t2[..., 3:] = 0
    return plan.unpack(acc)
