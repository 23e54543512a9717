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

Gradients.  For L = sum_t v_t B_t put c_t = v_t V^2 / C_t (0 where C_t = 0); the 1 / N of S_t is left out of c_t, it
cancels against the N of ``c2r_vjp``.  Then

    G_s(x) = sum over t and over every position of s in t of c_t (the product of the other two D at x)
           = sum_e w_e D_{p_e} D_{q_e}    over the entries e of shell s in a per-target list (``adjoint_pairs``: the bin
             (i, i, l) gives G_i += 2 c D_i D_l and G_l += c D_i D_i, the bin (i, i, i) gives G_i += 3 c D_i^2),
    grad(m) = r2c(G_shell(m))(m) / W_m,    0 for modes in no shell,

in the form of ``power_spectrum_vjp``, ``lpt_vjp`` and ``RealField.c2r_vjp`` before ``decompress_vjp``:
``Re(u.cdot(grad))`` is the derivative of L along u.  Two more kernels (csrc/pmx_bispec_grad.hip): pmx_bispec_pairsum
reads every shell field once and writes every G_s once, in place, whatever the number of entries, and
pmx_bispec_shells_vjp gathers the nb spectra r2c(G_s) into the gradient.  ``bispectrum_vjp`` keeps the forward's
memory: nb buffers next to the input, plus the output.  S is trilinear in the shell fields, so ``bispectrum_jvp`` is
one pmx_bispec_reduce call over the 2 nb fields [D_0 .., dD_0 ..] with three triples per bin.  Cotangents of ``Q`` and
``power`` are folded on the host into those of ``B`` and of the shells' P(k), which goes through
``power_spectrum_vjp``.

    r = bispectrum(delta_k, kedges, deconv_pow=2)
    g = bispectrum_vjp(delta_k, kedges, v_B=2 * (r.B - target) / sigma2, deconv_pow=2, result=r)   # d chi^2 / d delta_k
    t = bispectrum_jvp(delta_k, kedges, u_k, deconv_pow=2, result=r)       # t.B, t.Q, t.power: tangents along u_k

Not here: cross-bispectra of different fields, a line of sight / multipoles, meshes that are not 3-d.
"""
import numpy
import torch

from . import _abi, backend
from .power import _complex, _edges, _same_layout, power_spectrum, power_spectrum_jvp, power_spectrum_vjp


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


def _checked(a, kedges, deconv_pow):
    """the checks the forward and the gradients share: (kedges as float64, the number of shells, triangle_bins)"""
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
    return ke, nb, triangle_bins(ke)


def _same_bins(name, r, pm, ke, tri):
    """`r` (the argument `name`) must be the BispectrumResult of this mesh and these edges"""
    if not isinstance(r, BispectrumResult):
        raise TypeError('%s must be a BispectrumResult' % name)
    if r.Nmesh != tuple(int(n) for n in pm.Nmesh) or r.BoxSize != tuple(float(x) for x in pm.BoxSize) \
            or r.kedges.shape != ke.shape or \
            not (r.kedges == ke).all() or r.counts.shape != (len(tri),):
        raise ValueError('%s is not the BispectrumResult of this mesh and these kedges' % name)


def _shell_fields(a, kt, nb, deconv_pow, unit):
    """the nb real fields D_i (unit: I_i) of the spectrum a, each in the buffer of an in-place transform"""
    from .pm import _blank
    # (raw memory: the shells entry writes every mode of every block)
    spectra = [_blank(type(a), a.pm) for _ in range(nb)]
    backend.get().bispec_shells(a.value, [s.value for s in spectra], a.start, a.pm.Nmesh, a.pm.BoxSize, kt, deconv_pow,
                                unit)
    fields = []
    while spectra:
        fields.append(spectra.pop(0).c2r(out=Ellipsis))          # each in its own buffer
    return fields


def _real_values(fields):
    """(of a complex mesh the real part: the transform of a Hermitian spectrum)"""
    return [f.value.real if f.value.is_complex() else f.value for f in fields]


def _shell_sums(a, kt, nb, tri, deconv_pow, unit):
    """sum_x D_i D_j D_l / N per triangle (unit: of the indicator fields), summed over the ranks: a host vector"""
    be = backend.get()
    pm = a.pm
    acc = torch.zeros(len(tri), dtype=torch.float64, device=be.device)
    try:
        be.bispec_reduce(_real_values(_shell_fields(a, kt, nb, deconv_pow, unit)), tri, acc)
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
    ke, nb, tri = _checked(a, kedges, deconv_pow)
    if counts is not None:
        _same_bins('counts', counts, pm, ke, tri)

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


# ---- gradients -----------------------------------------------------------------------------------------------------

def _spectrum_only(field):
    from .pm import RealField, BaseComplexField
    if isinstance(field, RealField):
        raise TypeError('the gradients of bispectrum take ComplexField objects: transform the RealField with r2c and '
                        'back-propagate through it with r2c_vjp')
    if not isinstance(field, BaseComplexField):
        raise TypeError('bispectrum measures RealField or ComplexField objects, not %s' % type(field).__name__)
    return field


def adjoint_pairs(triangles, coef, nb):
    """The per-target list of the adjoint of the triangle sums: for L = sum_t coef_t sum_x D_i D_j D_l over the bins
    t = (i, j, l) of `triangles`, dL / dD_s(x) = sum_e weights[e] D_p(x) D_q(x) over the entries
    e in [offsets[s], offsets[s + 1]) with (p, q) = pairs[e], p <= q.

    One merged entry per (triangle, distinct target): weight coef, 2 coef or 3 coef for a shell that the bin names
    once, twice or three times.  Sorted by target, then p, then q (pmx_bispec_pairsum keeps D_p while consecutive
    entries share p).  Bins whose coef is 0 or not finite are dropped.  Returns (offsets int32 (nb + 1), pairs int32
    (npairs, 2), weights float64 (npairs))."""
    tri = numpy.asarray(triangles).astype('i8').reshape(-1, 3)
    c = numpy.asarray(coef, dtype='f8').reshape(-1)
    if len(c) != len(tri):
        raise ValueError('adjoint_pairs: %d coefficients for %d triangles' % (len(c), len(tri)))
    if len(tri) and (tri.min() < 0 or tri.max() >= nb):
        raise ValueError('adjoint_pairs: a triangle names a shell outside [0, %d)' % nb)
    keep = numpy.isfinite(c) & (c != 0)
    tri, c = tri[keep], c[keep]
    tgt, pq, w = [], [], []
    for pos in range(3):
        s = tri[:, pos]
        first = numpy.ones(len(tri), dtype=bool)
        for before in range(pos):
            first &= tri[:, before] != s                     # an earlier position has made this target's entry
        rest = tri[:, [x for x in range(3) if x != pos]]
        tgt.append(s[first])
        pq.append(numpy.sort(rest[first], axis=1))
        w.append(((tri == s[:, None]).sum(axis=1) * c)[first])
    tgt, pq, w = numpy.concatenate(tgt), numpy.concatenate(pq), numpy.concatenate(w)
    order = numpy.lexsort((pq[:, 1], pq[:, 0], tgt))
    offsets = numpy.concatenate([[0], numpy.cumsum(numpy.bincount(tgt, minlength=nb))])
    return offsets.astype('i4'), numpy.ascontiguousarray(pq[order]).astype('i4'), w[order]


def _cotangent(name, v, n):
    """a cotangent as n float64 values (None: zeros)"""
    if v is None:
        return numpy.zeros(n)
    v = numpy.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
    if v.shape != (n,):
        raise ValueError('%s must have the %d values of its column, not the shape %s' % (name, n, v.shape))
    return v.astype('f8')


def _denominator(p, tri):
    """den_t = P_i P_j + P_j P_l + P_l P_i of Q and its formal partial derivatives by P_i, P_j, P_l, (3, ntri)"""
    i, j, l = tri.T
    return p[i] * p[j] + p[j] * p[l] + p[l] * p[i], numpy.stack([p[j] + p[l], p[i] + p[l], p[i] + p[j]])


def bispectrum_vjp(field, kedges, v_B=None, v_Q=None, v_power=None, deconv_pow=0, result=None):
    """The gradient of L = sum_t v_B[t] B_t + sum_t v_Q[t] Q_t + sum_s v_power[s] power_s of
    ``bispectrum(field, kedges, deconv_pow)`` with respect to the field: see the module docstring.

    field : ComplexField as for bispectrum (a RealField raises TypeError: go through r2c_vjp).
    v_B, v_Q : ntri real values, v_power : nb real values; None counts as zero, and empty bins (NaN in the forward)
        contribute nothing.  ``k``, ``counts`` and ``ntriangles`` are piecewise constant and have no gradient.  v_Q and
        v_power are folded on the host: with den = P_i P_j + P_j P_l + P_l P_i, v_B += v_Q / den and
        v_power[s] -= sum_t v_Q[t] B_t / den_t^2 d den_t / d P_s; the power part goes through
        power_spectrum_vjp(field, kedges, v_power=..., deconv_pow=2 * deconv_pow).
    result : the BispectrumResult of the same arguments, for its counts, B and power; without it one forward call is
        made.

    Returns a field of the input's type in the form of power_spectrum_vjp, lpt_vjp and RealField.c2r_vjp before
    decompress_vjp: ``Re(u.cdot(grad))`` is the derivative of L along u.  Memory: the forward's nb buffers next to the
    input, plus the output.  On several ranks every step is local or a distributed transform.
    """
    from .lpt import _spectrum_of
    from .pm import _blank
    a = _spectrum_only(field)
    pm = a.pm
    ke, nb, tri = _checked(a, kedges, deconv_pow)
    ntri = len(tri)
    vb, vq, vp = _cotangent('v_B', v_B, ntri), _cotangent('v_Q', v_Q, ntri), _cotangent('v_power', v_power, nb)
    if result is None:
        result = bispectrum(a, ke, deconv_pow=deconv_pow)
    else:
        _same_bins('result', result, pm, ke, tri)

    # Q and power folded into the cotangents of B and of the shells' P(k)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        vb = numpy.where(numpy.isfinite(result.B), vb, 0.0)
        vp = numpy.where(numpy.isfinite(result.power), vp, 0.0)
        if v_Q is not None:
            den, dden = _denominator(result.power, tri)
            ok = numpy.isfinite(result.Q) & (vq != 0)
            vb = vb + numpy.where(ok, vq / den, 0.0)
            back = numpy.where(ok, vq * result.B / den ** 2, 0.0)
            for pos in range(3):
                numpy.subtract.at(vp, tri[:, pos], numpy.where(ok, back * dden[pos], 0.0))
        volume = float(numpy.prod(result.BoxSize))
        coef = numpy.where(result.counts > 0, vb * volume ** 2 / result.counts, 0.0)
    offsets, pairs, weights = adjoint_pairs(tri, coef, nb)

    be = backend.get()
    grad = None
    if len(weights):
        kt = torch.from_numpy(ke).to(be.device)
        try:
            fields = _shell_fields(a, kt, nb, int(deconv_pow), False)
            for f in fields:
                if f.value.is_complex():
                    f.value.imag.zero_()                     # a complex mesh: the real part is what the forward measures
            values = _real_values(fields)
            be.bispec_pairsum(values, values, torch.from_numpy(offsets).to(be.device),
                              torch.from_numpy(pairs).to(be.device), torch.from_numpy(weights).to(be.device))
            del values
            spectra = []
            while fields:
                spectra.append(_spectrum_of(fields.pop(0), a))   # r2c(G_s), each in its own buffer
            # (the kernel writes every mode of the block: only the GPU backend hands out raw memory)
            grad = _blank(type(a), pm) if be.name == 'hip' and a.value.numel() else pm.create(type=type(a))
            be.bispec_shells_vjp([s.value for s in spectra], grad.value, a.start, pm.Nmesh, pm.BoxSize, kt,
                                 int(deconv_pow))
        except backend.PmxError as e:
            if e.code == _abi.PMX_EUNSUPPORTED:
                raise ValueError(str(e))
            raise
    if vp.any():
        gp = power_spectrum_vjp(a, ke, v_power=vp, deconv_pow=2 * int(deconv_pow))
        if grad is None:
            grad = gp
        else:
            grad.value[...] += gp.value
    if grad is None:
        grad = pm.create(type=type(a))
    return grad


def bispectrum_jvp(field, kedges, v_field, deconv_pow=0, result=None):
    """The tangent of bispectrum along v_field: a BispectrumResult whose ``sums``, ``B``, ``Q`` and ``power`` are
    tangents and whose ``counts``, ``ntriangles``, ``k`` and ``triangles`` are the forward's.

    S is trilinear in the shell fields, so its tangent is the sum of the three triples (dD_i, D_j, D_l), (D_i, dD_j,
    D_l), (D_i, D_j, dD_l) per bin: one pmx_bispec_reduce call over the 2 nb fields [D_0 .., dD_0 ..], which needs
    2 nb <= PMX_BISPEC_MAX_SHELLS.  ``power`` comes from power_spectrum_jvp, dQ = dB / den - B d den / den^2.
    v_field : a ComplexField of the field's layout.  result : as for bispectrum_vjp."""
    a = _spectrum_only(field)
    v = _spectrum_only(v_field)
    pm = a.pm
    ke, nb, tri = _checked(a, kedges, deconv_pow)
    if 2 * nb > _abi.PMX_BISPEC_MAX_SHELLS:
        raise ValueError('%d shells: bispectrum_jvp sums over the 2 nb fields [D, dD] and takes at most '
                         'PMX_BISPEC_MAX_SHELLS / 2 = %d shells' % (nb, _abi.PMX_BISPEC_MAX_SHELLS // 2))
    _same_layout(a, v)
    if result is None:
        result = bispectrum(a, ke, deconv_pow=deconv_pow)
    else:
        _same_bins('result', result, pm, ke, tri)
    ntri = len(tri)
    triples = numpy.concatenate([tri + nb * numpy.eye(3, dtype='i4')[pos] for pos in range(3)]).astype('i4')

    be = backend.get()
    kt = torch.from_numpy(ke).to(be.device)
    acc = torch.zeros(3 * ntri, dtype=torch.float64, device=be.device)
    try:
        fields = _shell_fields(a, kt, nb, int(deconv_pow), False) + _shell_fields(v, kt, nb, int(deconv_pow), False)
        be.bispec_reduce(_real_values(fields), torch.from_numpy(triples).to(be.device), acc)
        del fields
    except backend.PmxError as e:
        if e.code == _abi.PMX_EUNSUPPORTED:
            raise ValueError(str(e))
        raise
    if pm.comm.size > 1:
        acc = pm.comm.allreduce(acc)
    dsums = acc.cpu().numpy().reshape(3, ntri).sum(axis=0) / float(numpy.prod([int(n) for n in pm.Nmesh]))
    dpk = power_spectrum_jvp(a, ke, v_field=v, deconv_pow=2 * int(deconv_pow))
    t = BispectrumResult(ke, tri.astype('i8'), dsums, result.counts, dpk, pm.BoxSize, pm.Nmesh)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        den, dden = _denominator(result.power, tri)
        t.Q = t.B / den - result.B * (dden * t.power[tri.T]).sum(axis=0) / den ** 2
    return t
