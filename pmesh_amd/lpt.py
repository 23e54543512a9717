"""Lagrangian perturbation theory displacements of initial conditions, first and second order, on the device.

The reference's callers build them with one ``Field.apply`` per factor, c2r per component and products of real fields
(nbody/genic.py:121-166; examples/nbody.py:154-160).  Here the factors are kernels of their own
(csrc/pmx_lpt.hip): one pass over delta(k) writes up to three Hessian spectra, one pass over the six real Hessian
components writes the source, and the gradients ride on the fused ``Transfer`` of c2r.

Conventions (k_d as ``ComplexField.x``, k^2 = sum_d k_d^2; every factor is 0 at k = 0):

    dx1_d   = c2r(i k_d / k^2 delta)                  -div dx1 = delta - mean
    phi_ij  = c2r(k_i k_j / k^2 delta)                 d_i d_j phi of phi = -delta / k^2 (Transfer.potential)
    S       = phi_00 phi_11 + phi_11 phi_22 + phi_22 phi_00 - phi_01^2 - phi_02^2 - phi_12^2    (2-d: phi_00 phi_11 - phi_01^2)
    lpt2source(delta) = r2c(3/7 S)
    dx2_d   = c2r(i k_d / k^2 lpt2source(delta))      div dx2 = -3/7 (S - mean)

and the particle at lattice point q moves to ``x = q + D1 dx1 + D2 dx2`` with D2 ~ D1^2 > 0 (Einstein-de Sitter):
Scoccimarro's 2LPT with its negative D2 folded into dx2, the 3/7 of nbody/genic.py:166.  Velocities (the caller's
growth rates times the same displacements) are the caller's.

The whole recipe, for a tabulated linear power spectrum P(k) in a box of volume V:

    delta_k = pm.generate_whitenoise(seed, unitary=True).apply(Tabulated(k, numpy.sqrt(P / V), loglog=True))
    q = pm.generate_uniform_particle_grid(shift=0.5)
    dx1, dx2 = lpt(delta_k, q, order=2)
"""
import numpy
import torch

from . import backend
from .transfer import Transfer


def _pairs(ndim):
    """(diagonal, off-diagonal) index pairs of the Hessian in the order of pmx_lpt2_source"""
    diag = [(d, d) for d in range(ndim)]
    off = [(i, j) for i in range(ndim) for j in range(i + 1, ndim)]
    return diag, off


def _check(dlin_k, q=None, lowest=1):
    from .pm import BaseComplexField
    if not isinstance(dlin_k, BaseComplexField):
        raise TypeError('the linear density must be a ComplexField, not %s' % type(dlin_k).__name__)
    ndim = len(dlin_k.pm.Nmesh)
    if ndim > 3:
        raise NotImplementedError('LPT on meshes of more than 3 dimensions')
    if ndim < lowest:
        raise ValueError('second-order LPT needs a mesh of 2 or 3 dimensions, not %d' % ndim)
    if not dlin_k.compressed:
        raise ValueError('LPT needs the r2c spectrum of a real mesh (not a complex mesh)')
    if q is not None and (len(q.shape) != 2 or q.shape[1] != ndim):
        raise ValueError('q must be an (n, %d) array of positions, not %s' % (ndim, tuple(q.shape)))
    return ndim


def _spectrum(like, base=None):
    from .pm import _blank
    if base is None and backend.get().name == 'hip':
        return _blank(type(like), like.pm)         # (every value of the block is written)
    return like.pm.create(type=type(like), base=base)


def _hessian(dlin_k, pairs):
    """the real fields phi_ij for the given pairs: one kernel pass over delta(k) per three of them, each spectrum
    transformed in place"""
    out = []
    for a in range(0, len(pairs), 3):
        group = pairs[a:a + 3]
        spectra = [_spectrum(dlin_k) for _ in group]
        backend.get().lpt_hessian(dlin_k.value, group, [s.value for s in spectra], dlin_k.start, dlin_k.Nmesh,
                                  dlin_k.BoxSize)
        for s in spectra:
            out.append(s.c2r(out=Ellipsis))
    return out


def lpt2source(dlin_k):
    """r2c of 3/7 S (the module docstring) for the linear density dlin_k: a new TransposedComplexField of the same
    mesh.  dlin_k is left as it is; 2 or 3 dimensions."""
    ndim = _check(dlin_k, lowest=2)
    diag, off = _pairs(ndim)
    phi = _hessian(dlin_k, diag + off)
    src = phi[0]
    backend.get().lpt2_source([f.value for f in phi], src.value, 3.0 / 7.0)
    del phi[1:]
    return src.r2c(out=Ellipsis)


def _gradients(spectrum, ndim):
    """the ndim real fields c2r(i k_d / k^2 spectrum), the factor fused into the first pass of c2r"""
    return [spectrum.c2r(transfer=Transfer.dx1(d)) for d in range(ndim)]


def _positions(pm, q):
    if not isinstance(q, torch.Tensor):
        q = torch.as_tensor(numpy.asarray(q))
    return q.to(backend.get().device)


def _read(pm, fields, q, layout, resampler):
    """all fields at q through one ParticleMesh.readout; on several ranks through one decomposition of q"""
    if layout is None and pm.comm.size > 1:
        layout = pm.decompose(q, smoothing=pm.resampler if resampler is None else resampler)
    return pm.readout(fields, q, resampler=resampler, layout=layout)


def lpt1(dlin_k, q, layout=None, resampler=None):
    """the first-order displacement dx1 at the positions q: an (n, ndim) float64 device tensor.

    dlin_k : the linear density contrast, an r2c ComplexField (either layout); left as it is.
    q : (n, ndim) positions (usually the lattice: pm.generate_uniform_particle_grid).
    layout : a pm.decompose(q) layout (several ranks; one is made when None); resampler : default pm.resampler.
    """
    ndim = _check(dlin_k, q)
    pm = dlin_k.pm
    q = _positions(pm, q)
    fields = _gradients(dlin_k, ndim)
    return _read(pm, fields, q, layout, resampler)


def lpt(dlin_k, q, order=2, layout=None, resampler=None):
    """the LPT displacements (dx1, dx2) at the positions q, each an (n, ndim) float64 device tensor (views of one
    (n, 2 ndim) array); dx2 is None for order 1.  Arguments as lpt1; order 2 needs 2 or 3 dimensions.

    Order 2 makes the six (2-d: three) Hessian fields, folds them into the source in place, transforms it and takes
    its gradient, then the gradient of dlin_k, freeing each intermediate as soon as it is used, and reads all 2 ndim
    displacement fields in one readout."""
    if order not in (1, 2):
        raise ValueError('order must be 1 or 2')
    if order == 1:
        return lpt1(dlin_k, q, layout=layout, resampler=resampler), None
    ndim = _check(dlin_k, q, lowest=2)
    pm = dlin_k.pm
    q = _positions(pm, q)
    src = lpt2source(dlin_k)
    fields = _gradients(src, ndim)
    del src
    fields = _gradients(dlin_k, ndim) + fields
    out = _read(pm, fields, q, layout, resampler)
    del fields
    return out[:, :ndim], out[:, ndim:]
