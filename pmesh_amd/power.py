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


class PowerResult(object):
    """The binned spectrum.  1-d bins (Nk): ``kedges``, ``k`` (mean |k|), ``modes`` (count), ``power`` (complex),
    ``poles`` (dict ell -> complex array).  (k, mu) bins (Nk x Nmu), None without ``muedges``: ``muedges``, ``k2d``,
    ``mu2d``, ``modes2d``, ``power2d``.  Means are weighted sums over the count; empty bins hold NaN."""

    def __init__(self, kedges, muedges, acc, ells):
        nk = len(kedges) - 1
        s1 = 4 + 2 * len(ells)
        a1 = acc[:nk * s1].reshape(nk, s1)
        self.kedges = kedges
        self.muedges = muedges
        with numpy.errstate(invalid='ignore', divide='ignore'):
            n = a1[:, 0]
            self.modes = numpy.rint(n).astype('i8')
            self.k = a1[:, 1] / n
            self.power = (a1[:, 2] + 1j * a1[:, 3]) / n
            self.poles = {ell: (2 * ell + 1) * (a1[:, 4 + 2 * p] + 1j * a1[:, 5 + 2 * p]) / n
                          for p, ell in enumerate(ells)}
            self.k2d = self.mu2d = self.modes2d = self.power2d = None
            if muedges is not None:
                a2 = acc[nk * s1:].reshape(nk, len(muedges) - 1, 5)
                n2 = a2[..., 0]
                self.modes2d = numpy.rint(n2).astype('i8')
                self.k2d = a2[..., 1] / n2
                self.mu2d = a2[..., 2] / n2
                self.power2d = (a2[..., 3] + 1j * a2[..., 4]) / n2


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


def _binning(ndim, name, edges, muedges, los, poles):
    """the checked bin edges `name` (kedges; redges on the real side), mu edges (or None), multipole orders and unit
    line of sight of a binned two-point statistic on a mesh of ndim dimensions"""
    ke = _edges(name, edges)
    if len(ke) - 1 > _abi.PMX_POWER_MAX_KBINS:
        raise ValueError('%d %s bins: more than PMX_POWER_MAX_KBINS = %d'
                         % (len(ke) - 1, name[0], _abi.PMX_POWER_MAX_KBINS))
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
    return ke, me, ells, los / norm


class _Plan(object):
    """the checked arguments of one spectrum: the fields, the edges, the multipole orders and the pmx_power struct"""

    def __init__(self, field, kedges, other, muedges, los, poles, deconv_pow, convert=_complex):
        a = convert(field)
        pm = a.pm
        ndim = len(pm.Nmesh)
        if ndim > _abi.PMX_MAXDIM:
            raise NotImplementedError('power spectra of meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
        b = None
        if other is not None:
            b = convert(other)
            if b.pm is not pm and (tuple(b.pm.Nmesh) != tuple(pm.Nmesh) or tuple(b.pm.BoxSize) != tuple(pm.BoxSize)
                                   or b.pm.comm is not pm.comm):
                raise ValueError('the two fields belong to different meshes')
            _same_layout(a, b)
        if a.value.dtype not in (torch.complex64, torch.complex128):
            raise ValueError('power_spectrum measures complex64 or complex128 fields')

        ke, me, ells, los = _binning(ndim, 'kedges', kedges, muedges, los, poles)
        if int(deconv_pow) != deconv_pow or deconv_pow < 0:
            raise ValueError('deconv_pow must be a non-negative integer')

        p = _abi.Power()
        p.nk = len(ke) - 1
        p.nmu = 0 if me is None else len(me) - 1
        p.npoles = len(ells)
        for i, ell in enumerate(ells):
            p.poles[i] = ell
        p.hermitian = int(bool(a.compressed))
        p.deconv_pow = int(deconv_pow)
        p.volume = float(numpy.prod(pm.BoxSize))
        for d in range(ndim):
            p.los[d] = float(los[d])

        self.a, self.b, self.pm, self.p, self.ke, self.me, self.ells = a, b, pm, p, ke, me, ells
        self.s1 = 4 + 2 * len(ells)
        be = backend.get()
        self.kt = torch.from_numpy(ke).to(be.device)
        self.mt = torch.from_numpy(me).to(be.device) if me is not None else None

    def sums(self, a, b):
        """the raw sums of pmx_power_project for the fields a and b (None: a) of this plan's layout, summed over the
        ranks: a host vector"""
        be = backend.get()
        p = self.p
        acc = torch.zeros(p.nk * self.s1 + p.nk * p.nmu * 5, dtype=torch.float64, device=be.device)
        try:
            be.power_project(p, a.value, b.value if b is not None else None, a.start, self.pm.Nmesh, self.pm.BoxSize,
                             self.kt, self.mt, acc)
        except backend.PmxError as e:
            if e.code == _abi.PMX_EUNSUPPORTED:
                raise ValueError(str(e))
            raise
        # one sum over the ranks of the raw sums, then the division
        if self.pm.comm.size > 1:
            acc = self.pm.comm.allreduce(acc)
        return acc.cpu().numpy()

    def result(self, acc):
        return PowerResult(self.ke, self.me, acc, self.ells)


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
    return plan.result(plan.sums(plan.a, plan.b))


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
    p, nk, nmu, ells = plan.p, plan.p.nk, plan.p.nmu, plan.ells
    if v_power2d is not None and plan.me is None:
        raise ValueError('v_power2d needs muedges')
    v_poles = dict(v_poles) if v_poles else {}
    unknown = [ell for ell in v_poles if ell not in ells]
    if unknown:
        raise ValueError('v_poles has orders %s that are not among poles %s' % (unknown, ells))
    v1 = _cotangent('v_power', v_power, (nk,))
    vp = [_cotangent('v_poles[%d]' % ell, v_poles.get(ell), (nk,)) for ell in ells]
    v2 = _cotangent('v_power2d', v_power2d, (nk, nmu)) if nmu else None

    if result is None:
        result = plan.result(plan.sums(plan.a, plan.b))
    elif tuple(result.modes.shape) != (nk,) or (nmu > 0) != (result.modes2d is not None) or \
            (nmu and tuple(result.modes2d.shape) != (nk, nmu)):
        raise ValueError('result is not the PowerResult of these arguments')

    # the coefficient table: acc's layout without the count, |k| and mu columns
    sc = 2 + 2 * len(ells)
    coef = numpy.zeros(nk * sc + nk * nmu * 2)
    c1 = coef[:nk * sc].reshape(nk, sc)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        inv = numpy.where(result.modes > 0, 1.0 / result.modes, 0.0)
        cols = [v1 * inv] + [(2 * ell + 1) * v * inv for ell, v in zip(ells, vp)]
        for i, c in enumerate(cols):
            c1[:, 2 * i], c1[:, 2 * i + 1] = c.real, c.imag
        if nmu:
            inv2 = numpy.where(result.modes2d > 0, 1.0 / result.modes2d, 0.0)
            c2 = coef[nk * sc:].reshape(nk, nmu, 2)
            c2[..., 0], c2[..., 1] = (v2 * inv2).real, (v2 * inv2).imag

    be = backend.get()
    a, b, pm = plan.a, plan.b, plan.pm
    # (the kernel writes every mode of the block: only the GPU backend hands out raw memory)
    from .pm import _blank

    def new(f):
        return _blank(type(f), pm) if be.name == 'hip' and f.value.numel() else pm.create(type=type(f))
    ga = new(a)
    gb = new(b) if b is not None else None
    try:
        be.power_vjp(p, a.value, b.value if b is not None else None, ga.value, gb.value if gb is not None else None,
                     a.start, pm.Nmesh, pm.BoxSize, plan.kt, plan.mt, torch.from_numpy(coef).to(be.device))
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise
    return ga if b is None else (ga, gb)


def power_spectrum_jvp(field, kedges, v_field=None, v_other=None, other=None, muedges=None, los=None, poles=(),
                       deconv_pow=0):
    """The tangent of power_spectrum along v_field (and v_other): a PowerResult whose ``power``, ``poles`` and
    ``power2d`` are tangents and whose ``k``, ``modes``, ``k2d``, ``mu2d`` and ``modes2d`` are the forward's.

    The raw sums are bilinear in (a, b), so the tangent of every power-like column is acc(da, b) + acc(a, db): two
    cross calls of the forward kernel, divided by the forward's counts (for the auto spectrum b = a and db = da).
    v_field, v_other : ComplexField objects of the fields' layout; None counts as zero."""
    plan = _Plan(field, kedges, other, muedges, los, poles, deconv_pow, convert=_complex_only)
    a, b = plan.a, plan.b
    if v_other is not None and b is None:
        raise ValueError('v_other needs other')
    terms = []
    for v, partner, first in ((v_field, b if b is not None else a, True), (v_other, a, False)):
        if v is None:
            continue
        v = _complex_only(v)
        _same_layout(a, v)
        terms.append((v, partner) if first else (partner, v))
    if b is None and terms:
        terms.append((a, terms[0][0]))                       # acc(a, da): the second half of the auto tangent
    if not terms:
        terms = [(a, b)]                                     # for the counts alone
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
    return plan.result(acc)
