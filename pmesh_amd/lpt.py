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

Gradients (lpt_vjp, lpt_jvp, lpt2source_vjp, lpt2source_jvp) follow the convention of the reference's pmesh/abopt.py:
a cotangent of a ComplexField is returned in the form RealField.c2r_vjp returns (before decompress_vjp), so that
Re(u.cdot(grad)) is the derivative along u; the adjoint chain runs paint -> r2c -> conj(i k_d / k^2) for the readouts
of gradients, r2c_vjp -> dS/dphi -> r2c -> k_i k_j / k^2 for the source (csrc/pmx_lpt_grad.hip).

The backward chain of a field-level fit of the table values t (band powers, transfer-function nodes) to a measured
spectrum, every step on the device:

    w = pm.generate_whitenoise(seed, unitary=True)
    tab = Tabulated(k, t, loglog=True)
    delta_k = w.apply(tab)
    dx1, dx2 = lpt(delta_k, q)
    x = q + D1 * dx1 + D2 * dx2
    c = pm.paint(x).r2c()
    res = power_spectrum(c, kedges, poles=(0, 2))                     # chi^2 = sum_ell sum_j (Re P_ell - target_ell)^2
    v = {ell: 2 * (res.poles[ell].real - target[ell]) for ell in (0, 2)}
    grad_c = power_spectrum_vjp(c, kedges, v_poles=v, poles=(0, 2), result=res)
    grad_x, _ = pm.paint_vjp(grad_c.r2c_vjp(), x, out_mass=False)
    grad_delta, _ = lpt_vjp(delta_k, q, D1 * grad_x, D2 * grad_x)
    grad_w, grad_t = tab.apply_vjp(w, grad_delta)                     # d chi^2 / d t, summed over the ranks

(pmesh_amd.power.power_spectrum_vjp, transfer.Tabulated.apply_vjp; their tangents power_spectrum_jvp and apply_jvp).
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


def _layout(pm, q, layout, resampler):
    if layout is None and pm.comm.size > 1:
        layout = pm.decompose(q, smoothing=pm.resampler if resampler is None else resampler)
    return layout


def _read(pm, fields, q, layout, resampler, gradient=None):
    """all fields at q through one ParticleMesh.readout; on several ranks through one decomposition of q"""
    layout = _layout(pm, q, layout, resampler)
    return pm.readout(fields, q, resampler=resampler, layout=layout, gradient=gradient)


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


# ---- gradients -------------------------------------------------------------------------------------------------------

def _check_like(dlin_k, v, what):
    from .pm import BaseComplexField
    if not isinstance(v, BaseComplexField) or v.pm is not dlin_k.pm:
        raise TypeError('%s must be a ComplexField of the mesh of dlin_k' % what)


def _cotangent(pm, v, n, ndim, what):
    """an (n, ndim) cotangent or tangent of positions as a float64 device tensor, or None"""
    if v is None:
        return None
    v = _positions(pm, v)
    if tuple(v.shape) != (n, ndim):
        raise ValueError('%s must be an (%d, %d) array, not %s' % (what, n, ndim, tuple(v.shape)))
    return v.to(torch.float64)


def _spectrum_of(real, like):
    """the r2c spectrum of `real` over its own buffer, of the type (layout) of `like`"""
    from .pm import UntransposedComplexField
    if isinstance(like, UntransposedComplexField):
        return real.r2c(out=UntransposedComplexField(real.pm, base=real._base))
    return real.r2c(out=Ellipsis)


def _contract(spectra, factors, out, accumulate):
    backend.get().lpt_contract([s.value for s in spectra], factors, out.value, accumulate, out.start, out.Nmesh,
                               out.BoxSize)


def _paint_contract(pm, q, v, scale, like, acc, layout, resampler):
    """acc + sum_d conj(i k_d / k^2) r2c(paint(q, scale v[:, d])): one component painted at a time into a fresh
    field, transformed in place and contracted into the accumulator (acc None: the first spectrum becomes it)"""
    for d in range(v.shape[1]):
        m = v[:, d] * scale if scale != 1 else v[:, d].contiguous()
        s = _spectrum_of(pm.paint(q, mass=m, resampler=resampler, layout=layout), like)
        del m
        if acc is None:
            _contract([s], [(d, -1)], s, False)
            acc = s
        else:
            _contract([s], [(d, -1)], acc, True)
        del s
    return acc


def _source_adjoint(dlin_k, held, scale):
    """sum_p h_p r2c(scale g dS/dphi_p) for the Hessian fields phi_p of dlin_k and the real field g = held[0] (let
    go of as soon as it is read): dS/dphi written over the recomputed Hessian fields, each transformed in place,
    contracted into the first of them"""
    ndim = len(dlin_k.pm.Nmesh)
    diag, off = _pairs(ndim)
    pairs = diag + off
    phi = _hessian(dlin_k, pairs)
    backend.get().lpt2_source_vjp(held[0].value, [f.value for f in phi], [f.value for f in phi], scale)
    del held[:]
    spectra = []
    while phi:
        spectra.append(_spectrum_of(phi.pop(0), dlin_k))
    _contract(spectra, pairs, spectra[0], False)
    return spectra[0]


def lpt2source_vjp(dlin_k, v):
    """the cotangent of dlin_k for the cotangent v (a ComplexField) of lpt2source(dlin_k), in the form of
    RealField.c2r_vjp (before decompress_vjp): a new ComplexField of dlin_k's type.  2 or 3 dimensions.

    Through r2c_vjp, the derivative of the source and the c2r_vjp of each Hessian component (their 1 / prod(N) and
    prod(N) cancel)."""
    _check(dlin_k, lowest=2)
    _check_like(dlin_k, v, 'v')
    return _source_adjoint(dlin_k, [v.c2r()], 3.0 / 7.0)


def lpt2source_jvp(dlin_k, v_dlin_k):
    """the tangent of lpt2source(dlin_k) along v_dlin_k: r2c(3/7 dS(phi; phi')) with phi the Hessian fields of dlin_k
    and phi' those of v_dlin_k, a new TransposedComplexField (as lpt2source).  2 or 3 dimensions."""
    ndim = _check(dlin_k, lowest=2)
    _check_like(dlin_k, v_dlin_k, 'v_dlin_k')
    diag, off = _pairs(ndim)
    phi = _hessian(dlin_k, diag + off)
    tan = _hessian(v_dlin_k, diag + off)
    backend.get().lpt2_source_jvp([f.value for f in phi], [f.value for f in tan], tan[0].value, 3.0 / 7.0)
    del phi, tan[1:]
    return tan[0].r2c(out=Ellipsis)


def _forward_fields(dlin_k, order, first=True, second=True):
    ndim = len(dlin_k.pm.Nmesh)
    fields = _gradients(dlin_k, ndim) if first else []
    if order == 2 and second:
        src = lpt2source(dlin_k)
        fields += _gradients(src, ndim)
        del src
    return fields


def _read_gradients(pm, fields, q, w, out, layout, resampler):
    """out[:, f] += sum_e w[:, e] d fields[f] / d q_e at q, one readout of all fields per direction e"""
    for e in range(w.shape[1]):
        r = _read(pm, fields, q, layout, resampler, gradient=e)
        out.addcmul_(r, w[:, e:e + 1])
        del r


def lpt_vjp(dlin_k, q, v_dx1, v_dx2=None, order=2, layout=None, resampler=None, out_q=False):
    """the cotangents (grad_dlin_k, grad_q) of lpt(dlin_k, q, order) for the cotangents v_dx1, v_dx2 of its outputs.

    v_dx1, v_dx2 : (n, ndim) arrays (device tensors or numpy) over the rows of q; None counts as zero; v_dx2 only for
    order 2.  Other arguments as lpt.
    grad_dlin_k : a new ComplexField of dlin_k's type in the form of RealField.c2r_vjp (before decompress_vjp):
    Re(u.cdot(grad_dlin_k)) is the derivative of sum(v_dx1 dx1 + v_dx2 dx2) along the spectrum u.
    grad_q : with out_q, the (n, ndim) float64 device tensor sum_f v_f d field_f / d q (readouts with gradient=e of
    the displacement fields); None otherwise.

    The chain is the adjoint of the forward as written, with no masking: on the Nyquist planes the odd factors
    i k_d / k^2 and the off-diagonal k_i k_j / k^2 are not Hermitian (k_d = -k_Nyquist on both partners), so the
    forward maps those modes of dlin_k as c2r happens to treat them, and grad_dlin_k holds there what that adjoint
    gives; Re(u.cdot(grad)) is the derivative along u for spectra u whose Nyquist planes are zero, the convention of
    lpt itself.

    Memory: one painted component at a time; the six (2-d: three) Hessian fields of dlin_k are recomputed and
    overwritten with their cotangents, transformed and contracted in place."""
    if order not in (1, 2):
        raise ValueError('order must be 1 or 2')
    ndim = _check(dlin_k, q, lowest=1 if order == 1 else 2)
    if order == 1 and v_dx2 is not None:
        raise ValueError('v_dx2 is the cotangent of the second order: not for order 1')
    pm = dlin_k.pm
    q = _positions(pm, q)
    n = q.shape[0]
    v1 = _cotangent(pm, v_dx1, n, ndim, 'v_dx1')
    v2 = _cotangent(pm, v_dx2, n, ndim, 'v_dx2')
    layout = _layout(pm, q, layout, resampler)
    grad_q = None
    if out_q:
        grad_q = torch.zeros((n, ndim), dtype=torch.float64, device=q.device)
        vs = [v for v in (v1, v2) if v is not None]
        if vs:
            fields = _forward_fields(dlin_k, order, v1 is not None, v2 is not None)
            vs = torch.cat(vs, dim=1)
            for e in range(ndim):
                r = _read(pm, fields, q, layout, resampler, gradient=e)
                grad_q[:, e] = (r * vs).sum(dim=1)
                del r
            del fields, vs
    nd = float(numpy.prod([float(x) for x in pm.Nmesh]))
    G = None
    if v2 is not None:
        # Gsrc = sum_d conj(t_d) c2r_vjp(P2_d); g = r2c_vjp(Gsrc): the prod(N) of both cancel
        held = [_paint_contract(pm, q, v2, 1.0, dlin_k, None, layout, resampler).c2r(out=Ellipsis)]
        G = _source_adjoint(dlin_k, held, 3.0 / 7.0 * nd)
    if v1 is not None:
        G = _paint_contract(pm, q, v1, nd, dlin_k, G, layout, resampler)
    if G is None:
        G = pm.create(type=type(dlin_k))
    return G, grad_q


def lpt_jvp(dlin_k, q, v_dlin_k=None, v_q=None, order=2, layout=None, resampler=None):
    """the tangents (ddx1, ddx2) of lpt(dlin_k, q, order) along the spectrum v_dlin_k (a ComplexField of dlin_k's
    mesh) and the positions v_q ((n, ndim)); None counts as zero.  Shapes and layout as lpt's outputs: views of one
    (n, 2 ndim) float64 device tensor; ddx2 is None for order 1.

    v_dlin_k contributes readouts of c2r(i k_d / k^2 v_dlin_k) and of the gradients of lpt2source_jvp(dlin_k,
    v_dlin_k); v_q the readouts of the displacement fields of dlin_k with gradient=e."""
    if order not in (1, 2):
        raise ValueError('order must be 1 or 2')
    ndim = _check(dlin_k, q, lowest=1 if order == 1 else 2)
    if v_dlin_k is not None:
        _check_like(dlin_k, v_dlin_k, 'v_dlin_k')
    pm = dlin_k.pm
    q = _positions(pm, q)
    n = q.shape[0]
    w = _cotangent(pm, v_q, n, ndim, 'v_q')
    layout = _layout(pm, q, layout, resampler)
    if v_dlin_k is not None:
        fields = _gradients(v_dlin_k, ndim)
        if order == 2:
            src = lpt2source_jvp(dlin_k, v_dlin_k)
            fields += _gradients(src, ndim)
            del src
        out = _read(pm, fields, q, layout, resampler)
        del fields
    else:
        out = torch.zeros((n, order * ndim), dtype=torch.float64, device=q.device)
    if w is not None:
        fields = _forward_fields(dlin_k, order)
        _read_gradients(pm, fields, q, w, out, layout, resampler)
        del fields
    if order == 1:
        return out[:, :ndim], None
    return out[:, :ndim], out[:, ndim:]
