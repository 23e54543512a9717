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
    a = _complex(field)
    pm = a.pm
    ndim = len(pm.Nmesh)
    if ndim > _abi.PMX_MAXDIM:
        raise NotImplementedError('power spectra of meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    b = None
    if other is not None:
        b = _complex(other)
        if b.pm is not pm and (tuple(b.pm.Nmesh) != tuple(pm.Nmesh) or tuple(b.pm.BoxSize) != tuple(pm.BoxSize)
                               or b.pm.comm is not pm.comm):
            raise ValueError('the two fields belong to different meshes')
        if type(b) is not type(a) or tuple(b.start) != tuple(a.start) or tuple(b.value.shape) != tuple(a.value.shape) \
                or b.value.dtype != a.value.dtype:
            raise ValueError('the two fields must have the same layout and dtype (%s %s vs %s %s)'
                             % (type(a).__name__, a.value.dtype, type(b).__name__, b.value.dtype))
    if a.value.dtype not in (torch.complex64, torch.complex128):
        raise ValueError('power_spectrum measures complex64 or complex128 fields')

    ke = _edges('kedges', kedges)
    if len(ke) - 1 > _abi.PMX_POWER_MAX_KBINS:
        raise ValueError('%d k bins: more than PMX_POWER_MAX_KBINS = %d' % (len(ke) - 1, _abi.PMX_POWER_MAX_KBINS))
    me = None
    if muedges is not None:
        me = _edges('muedges', muedges, -1.0, 1.0)
        if len(me) - 1 > _abi.PMX_POWER_MAX_MUBINS:
            raise ValueError('%d mu bins: more than PMX_POWER_MAX_MUBINS = %d' % (len(me) - 1, _abi.PMX_POWER_MAX_MUBINS))
    ells = [int(ell) for ell in poles]
    if len(ells) > _abi.PMX_POWER_MAX_POLES:
        raise ValueError('%d multipoles: more than PMX_POWER_MAX_POLES = %d' % (len(ells), _abi.PMX_POWER_MAX_POLES))
    if len(set(ells)) != len(ells) or any(ell < 0 or ell > _abi.PMX_POWER_MAX_ELL for ell in ells):
        raise ValueError('poles must be distinct orders in 0..PMX_POWER_MAX_ELL = %d' % _abi.PMX_POWER_MAX_ELL)
    if int(deconv_pow) != deconv_pow or deconv_pow < 0:
        raise ValueError('deconv_pow must be a non-negative integer')
    if los is None:
        los = numpy.zeros(ndim)
        los[-1] = 1.0
    los = numpy.array(los, dtype='f8').reshape(-1)
    norm = numpy.sqrt((los ** 2).sum())
    if len(los) != ndim or not numpy.isfinite(norm) or norm == 0:
        raise ValueError('los must be a nonzero vector of %d components' % ndim)
    los = los / norm

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

    be = backend.get()
    s1 = 4 + 2 * len(ells)
    acc = torch.zeros(p.nk * s1 + p.nk * p.nmu * 5, dtype=torch.float64, device=be.device)
    kt = torch.from_numpy(ke).to(be.device)
    mt = torch.from_numpy(me).to(be.device) if me is not None else None
    try:
        be.power_project(p, a.value, b.value if b is not None else None, a.start, pm.Nmesh, pm.BoxSize, kt, mt, acc)
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise
    # one sum over the ranks of the raw sums, then the division
    if pm.comm.size > 1:
        acc = pm.comm.allreduce(acc)
    return PowerResult(ke, me, acc.cpu().numpy(), ells)
