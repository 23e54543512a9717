"""pmesh_amd.bispectrum gradients (bispectrum_vjp, bispectrum_jvp, adjoint_pairs; csrc/pmx_bispec_grad.hip).

The checks: the cubic identity Re(u.cdot(vjp)) == (L(a + u) - L(a - u)) / 2 - L(u) of the forward itself (L is a
homogeneous cubic, so the identity is exact and needs no step), the adjoint identity between the vjp and the jvp, the
gradient against a numpy restatement of the module docstring's formulas with double FFTs (reference below), the
per-target list against a triple loop, several ranks against one and, at kernel level, pmx_bispec_pairsum against numpy
sums and pmx_bispec_shells_vjp against the adjoint identity with pmx_bispec_shells.  Under -m "not gpu" the two new
entries are served by numpy (BispecGradOracleBackend) and the host layer runs without a GPU; under -m gpu the same
tests run on the kernels.

Bounds.  f8, whole gradient: |grad - grad_ref|(m) <= 1e-13 scale_m with scale_m = (1 / W_m) sum_x sum_e |w_e| |D_p D_q|(x)
for a mode in a shell (F8_TOL of tests/test_bispectrum.py with its reasoning: numpy's own double route sits at 3e-16 of
this scale); a mode in no shell is exactly 0.  pmx_bispec_pairsum alone: |G - G_ref|(x) <= 1e-13 sum_e |w_e| |D_p D_q|(x),
and for f4 blocks 6e-8 |G_ref(x)| more: 6e-8 rounds up 2^-24, the half-ulp of rounding the double sum to the float
output.  f4, whole gradient (complex64 fields): max |grad - grad_ref| <= F4_VJP_TOL max_m |grad_ref|, twice the largest
error that the same pipeline composed from the parts the package had before the adjoint kernels shows on the parity
cases on the GPU (composition_gradient below: pmx_bispec_shells on the complex64 field, the complex64 c2r, the pair
products in torch float64 rounded to float, the complex64 r2c, the gather with torch.where;
`scripts/bispectrum_probe.py --vjp` prints the table, DESIGN 5.7 records the run) — the margin of F4_TOL of the
forward, because the kernels round in other places than the composition.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd.bispectrum import (BispectrumResult, adjoint_pairs, bispectrum, bispectrum_jvp, bispectrum_vjp,
                                  triangle_bins)
from pmesh_amd.pm import ParticleMesh, UntransposedComplexField
from tests.test_bispectrum import (F8_TOL, PARITY_MESHES, BispecOracleBackend, _all_triples, _shells_of, full_spectrum,
                                   parity_field, shells_full)
from tests.test_power import _sinc_pow, density
from tests.test_power_gradients import PowerGradOracleBackend

# the composition's largest |grad - grad_ref| / max |grad_ref| over the parity cases, measured on the GPU (see the
# module docstring)
F4_VJP_MEASURED = 7.722e-7
F4_VJP_TOL = 2 * F4_VJP_MEASURED
F4_ROUND = 6e-8


# ---- the CPU double ------------------------------------------------------------------------------------------------

class BispecGradOracleBackend(BispecOracleBackend, PowerGradOracleBackend):
    """the CPU test double with pmx_bispec_pairsum / pmx_bispec_shells_vjp served by numpy (and pmx_power_vjp by the
    restatement of tests/test_power_gradients.py, for the cotangents of Q and power)"""
    name = 'oracle-bispec-grad'

    def bispec_pairsum(self, fields, outs, offsets, pairs, weights):
        if fields[0].numel() == 0:
            return
        f = [x.numpy().astype('f8') for x in fields]             # (copies: outs[s] may be fields[s])
        off, pr, w = offsets.numpy(), pairs.numpy(), weights.numpy()
        for s, out in enumerate(outs):
            g = numpy.zeros(f[0].shape)
            for e in range(off[s], off[s + 1]):
                g += w[e] * (f[pr[e, 0]] * f[pr[e, 1]])
            out[...] = torch.from_numpy(g).to(out.dtype)

    def bispec_shells_vjp(self, ins, out, start, nmesh, boxsize, kedges, deconv_pow=0):
        if out.numel() == 0:
            return
        sh, w = _shells_of(start, out.shape, nmesh, boxsize, kedges.numpy())
        v = numpy.zeros(tuple(out.shape), dtype='c16')
        for s, x in enumerate(ins):
            v = numpy.where(sh == s, x.numpy().astype('c16'), v)
        if deconv_pow:
            for wd in w:
                v = v / _sinc_pow(wd, deconv_pow)
        out[...] = torch.from_numpy(v).to(out.dtype)


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def gbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(BispecGradOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def cpu(t):
    return t.detach().cpu().numpy()


# ---- the FFT-form reference ------------------------------------------------------------------------------------------

def shell_fields(full, Nmesh, BoxSize, kedges, deconv_pow):
    """D_i of the module docstring of pmesh_amd.bispectrum by numpy FFTs in double, the shell numbers and W"""
    N = float(numpy.prod(Nmesh))
    _, sh, w = shells_full(Nmesh, BoxSize, kedges)
    W = numpy.ones(tuple(Nmesh))
    if deconv_pow:
        for wd in w:
            W = W * _sinc_pow(wd, deconv_pow)
    v = full / W
    D = [(numpy.fft.ifftn(numpy.where(sh == i, v, 0)) * N).real for i in range(len(kedges) - 1)]
    return D, sh, W


def coefficients(v, counts, BoxSize):
    """c_t = v_t V^2 / C_t, 0 where C_t = 0"""
    V = float(numpy.prod(BoxSize))
    with numpy.errstate(invalid='ignore', divide='ignore'):
        return numpy.where(counts > 0, v * V ** 2 / counts, 0.0)


def pair_sums(D, tri, coef):
    """G_s and sum_e |w_e| |D_p D_q| per shell, from a loop over the bins and the three positions of each"""
    G = [numpy.zeros_like(D[0]) for _ in D]
    A = [numpy.zeros_like(D[0]) for _ in D]
    for c, (i, j, l) in zip(coef, tri):
        if c == 0 or not numpy.isfinite(c):
            continue
        for s, p, q in ((i, j, l), (j, i, l), (l, i, j)):
            G[s] += c * (D[p] * D[q])
            A[s] += abs(c) * numpy.abs(D[p] * D[q])
    return G, A


def reference(c, kedges, deconv_pow, coef):
    """grad_ref and scale_m (0 for a mode in no shell) over the stored modes of the one-rank field c, and the shell of
    every stored mode"""
    pm = c.pm
    Nmesh, BoxSize = [int(n) for n in pm.Nmesh], [float(x) for x in pm.BoxSize]
    N = float(numpy.prod(Nmesh))
    D, sh, W = shell_fields(full_spectrum(c), Nmesh, BoxSize, kedges, deconv_pow)
    G, A = pair_sums(D, triangle_bins(kedges), coef)
    grad = numpy.zeros(tuple(Nmesh), dtype='c16')
    scale = numpy.zeros(tuple(Nmesh))
    for s in range(len(D)):
        grad = numpy.where(sh == s, (numpy.fft.fftn(G[s]) / N) / W, grad)
        scale = numpy.where(sh == s, A[s].sum() / W, scale)
    if c.compressed:
        keep = Nmesh[-1] // 2 + 1
        return grad[..., :keep], scale[..., :keep], sh[..., :keep]
    return grad, scale, sh


def assert_gradient(got, want, scale, sh, tol=F8_TOL):
    err = numpy.abs(got - want)
    print('max |grad - grad_ref| / scale = %.3g (bound %.3g)' % (numpy.max(err[sh >= 0] / scale[sh >= 0]), tol))
    assert (got[sh < 0] == 0).all(), 'a mode in no shell is not exactly 0'
    assert (sh >= 0).sum() > 10 and (scale[sh >= 0] > 0).all()
    bad = numpy.nonzero(~(err <= tol * scale))
    assert len(bad[0]) == 0, (err[bad][:5], scale[bad][:5])


def composition_gradient(c, kedges, deconv_pow, coef):
    """the gradient composed from what the package had before the adjoint kernels (the yardstick of F4_VJP_TOL): the
    shell split of the field as it is stored, its own c2r, the pair products in torch float64 rounded to the field's
    precision, its own r2c, the gather with torch.where"""
    be = backend.get()
    pm = c.pm
    nb = len(kedges) - 1
    dev = c.value.device
    kt = torch.from_numpy(numpy.asarray(kedges, dtype='f8')).to(dev)
    spectra = [pm.create(type=type(c)) for _ in range(nb)]
    be.bispec_shells(c.value, [s.value for s in spectra], c.start, pm.Nmesh, pm.BoxSize, kt, deconv_pow, False)
    D = []
    for s in spectra:
        r = s.c2r().value
        D.append((r.real if r.is_complex() else r).double())
    offsets, pairs, weights = adjoint_pairs(triangle_bins(kedges), coef, nb)
    sh, w = _shells_of(c.start, c.value.shape, pm.Nmesh, pm.BoxSize, numpy.asarray(kedges))
    W = numpy.ones(tuple(c.value.shape))
    if deconv_pow:
        for wd in w:
            W = W * _sinc_pow(wd, deconv_pow)
    sht = torch.from_numpy(sh).to(dev)
    Wt = torch.from_numpy(W).to(dev).to(c.value.real.dtype)
    grad = torch.zeros_like(c.value)
    for s in range(nb):
        g = torch.zeros_like(D[0])
        for e in range(offsets[s], offsets[s + 1]):
            g += float(weights[e]) * (D[pairs[e, 0]] * D[pairs[e, 1]])
        x = pm.create(type='real')
        x.value[...] = g.to(x.value.real.dtype if x.value.is_complex() else x.value.dtype)
        gh = x.r2c(out=pm.create(type=type(c)))
        grad = torch.where(sht == s, gh.value / Wt, grad)
    return cpu(grad)


def parity_case(kind, Nmesh, BoxSize, deconv_pow, dtype):
    """the field, the edges, the forward result, the cotangent of B and c_t of one parity case"""
    c, ke = parity_field(kind, Nmesh, BoxSize, dtype)
    r = bispectrum(c, ke, deconv_pow=deconv_pow)
    v = numpy.random.RandomState(17).normal(size=len(r.triangles))
    return c, ke, r, v, coefficients(v, r.counts, BoxSize)


def composition_error(kind, Nmesh, BoxSize, deconv_pow):
    """max |composition - numpy f8| / max |numpy f8| for one complex64 parity case"""
    c, ke, r, v, coef = parity_case(kind, Nmesh, BoxSize, deconv_pow, 'f4')
    want, _, _ = reference(c, ke, deconv_pow, coef)
    return float(numpy.abs(composition_gradient(c, ke, deconv_pow, coef) - want).max() / numpy.abs(want).max())


# ---- 1., 2. the cubic and the adjoint identity -----------------------------------------------------------------------

BRUTE = ([12, 10, 14], [100., 80., 120.], 2 * numpy.pi / 120. * numpy.array([0.5, 1.5, 2.5, 3.2]))


def brute_fields():
    """the mesh and edges of test_bispectrum.test_brute_force: a field and a direction, both spectra of real fields
    (c2r expects the self-conjugate planes of a compressed spectrum consistent)"""
    Nmesh, BoxSize, ke = BRUTE
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize)
    return pm, density(pm, seed=8).r2c(), density(pm, seed=9).r2c(), ke


def combined(pm, a, u, eps):
    c = pm.create(type=type(a))
    c.value[...] = a.value + eps * u.value
    return c


def triple_scale(Da, Db, Dc, tri, N):
    """sum_x |Da_i Db_j Dc_l| / N per bin"""
    return numpy.array([numpy.abs(Da[i] * Db[j] * Dc[l]).sum() / N for i, j, l in tri])


@pytest.mark.parametrize('deconv_pow', [0, 2])
def test_cubic_identity(gbe, deconv_pow):
    """L(a) = sum_t v_t B_t is a homogeneous cubic in a: (L(a + u) - L(a - u)) / 2 - L(u) is its derivative along u,
    exactly.  Tolerance: 1e-12 of sum_t |c_t| sum_x |D_i D_j D_l| / N at a + u, the sum of the absolute terms of
    L(a + u) (the 1 / N is that of S_t: L = sum_t c_t sum_x D_i D_j D_l / N)"""
    pm, a, u, ke = brute_fields()
    Nmesh, BoxSize, _ = BRUTE
    r = bispectrum(a, ke, deconv_pow=deconv_pow)
    v = numpy.random.RandomState(1).normal(size=len(r.triangles))
    assert (r.counts == 0).any() and (r.counts > 0).sum() >= 8

    def L(c):
        return float(numpy.nansum(v * bispectrum(c, ke, deconv_pow=deconv_pow, counts=r).B))
    before = a.value.clone()
    g = bispectrum_vjp(a, ke, v_B=v, deconv_pow=deconv_pow, result=r)
    assert type(g) is type(a) and torch.equal(a.value, before)
    lhs = u.cdot(g).real
    rhs = (L(combined(pm, a, u, 1.0)) - L(combined(pm, a, u, -1.0))) / 2 - L(u)
    D, _, _ = shell_fields(full_spectrum(combined(pm, a, u, 1.0)), Nmesh, BoxSize, ke, deconv_pow)
    coef = coefficients(v, r.counts, BoxSize)
    tol = 1e-12 * float((numpy.abs(coef) * triple_scale(D, D, D, r.triangles, float(numpy.prod(Nmesh)))).sum())
    print('cubic identity: %.17g against %.17g, |difference| = %.3g (bound %.3g)' % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs) > 1e3 * tol
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize('deconv_pow', [0, 2])
def test_adjoint_identity(gbe, deconv_pow):
    """sum_t v_t jvp(a, u).B_t == Re(u.cdot(vjp(a, v_B=v))), and the same for v_Q and v_power against the tangents of
    Q and power.  Tolerance: 1e-12 of the sum of the absolute terms of the left side: per bin sum_x (|dD_i D_j D_l| +
    |D_i dD_j D_l| + |D_i D_j dD_l|) / N for dB, per shell 2 V mean |a| |u| / W^2 for dP, and for
    dQ = dB / den - B d den / den^2 both through the partial derivatives of Q"""
    pm, a, u, ke = brute_fields()
    Nmesh, BoxSize, _ = BRUTE
    N, V = float(numpy.prod(Nmesh)), float(numpy.prod(BoxSize))
    r = bispectrum(a, ke, deconv_pow=deconv_pow)
    tri, nb = r.triangles, len(ke) - 1
    t = bispectrum_jvp(a, ke, u, deconv_pow=deconv_pow, result=r)
    assert isinstance(t, BispectrumResult)
    assert (t.counts == r.counts).all() and (t.ntriangles == r.ntriangles).all() and (t.triangles == tri).all()
    numpy.testing.assert_allclose(t.k, r.k, rtol=1e-12)
    # no result: one forward call inside, the same tangents (the power sums are float atomics: to rounding)
    t2 = bispectrum_jvp(a, ke, u, deconv_pow=deconv_pow)
    numpy.testing.assert_array_equal(t2.sums, t.sums)
    numpy.testing.assert_allclose(t2.Q, t.Q, rtol=1e-9, equal_nan=True)
    # the absolute terms
    D, sh, W = shell_fields(full_spectrum(a), Nmesh, BoxSize, ke, deconv_pow)
    dD, _, _ = shell_fields(full_spectrum(u), Nmesh, BoxSize, ke, deconv_pow)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        absB = numpy.where(r.counts > 0, V ** 2 / r.counts * (
            triple_scale(dD, D, D, tri, N) + triple_scale(D, dD, D, tri, N) + triple_scale(D, D, dD, tri, N)), 0.0)
        prod = 2 * V * numpy.abs(full_spectrum(a)) * numpy.abs(full_spectrum(u)) / W ** 2
        absP = numpy.array([prod[sh == s].mean() for s in range(nb)])
        i, j, l = tri.T
        p = r.power
        den = p[i] * p[j] + p[j] * p[l] + p[l] * p[i]
        absQ = numpy.where(r.counts > 0, absB / numpy.abs(den) + numpy.abs(r.B) / den ** 2 * (
            numpy.abs(p[j] + p[l]) * absP[i] + numpy.abs(p[i] + p[l]) * absP[j] + numpy.abs(p[i] + p[j]) * absP[l]), 0.0)
    rng = numpy.random.RandomState(2)
    vB, vQ, vP = rng.normal(size=len(tri)), rng.normal(size=len(tri)) * numpy.nanmax(numpy.abs(den)), rng.normal(size=nb)
    for kw, lhs, scale in ((dict(v_B=vB), numpy.nansum(vB * t.B), numpy.nansum(numpy.abs(vB) * absB)),
                           (dict(v_Q=vQ), numpy.nansum(vQ * t.Q), numpy.nansum(numpy.abs(vQ) * absQ)),
                           (dict(v_power=vP), numpy.nansum(vP * t.power), numpy.nansum(numpy.abs(vP) * absP)),
                           (dict(v_B=vB, v_Q=vQ, v_power=vP),
                            numpy.nansum(vB * t.B) + numpy.nansum(vQ * t.Q) + numpy.nansum(vP * t.power),
                            numpy.nansum(numpy.abs(vB) * absB) + numpy.nansum(numpy.abs(vQ) * absQ) +
                            numpy.nansum(numpy.abs(vP) * absP))):
        g = bispectrum_vjp(a, ke, deconv_pow=deconv_pow, result=r, **kw)
        rhs = u.cdot(g).real
        print('adjoint identity %s: %.17g against %.17g, |difference| = %.3g (bound %.3g)'
              % (sorted(kw), lhs, rhs, abs(lhs - rhs), 1e-12 * scale))
        assert abs(lhs) > 1e-9 * scale
        assert abs(lhs - rhs) <= 1e-12 * scale, kw


# ---- 3. parity with the FFT-form reference -----------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('deconv_pow', [0, 2])
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('Nmesh,BoxSize', PARITY_MESHES)
def test_gradient_parity(gbe, Nmesh, BoxSize, kind, deconv_pow, dtype):
    c, ke, r, v, coef = parity_case(kind, Nmesh, BoxSize, deconv_pow, dtype)
    assert len(r.triangles) > 10 and (r.counts > 0).sum() > 10
    want, scale, sh = reference(c, ke, deconv_pow, coef)
    before = c.value.clone()
    g = bispectrum_vjp(c, ke, v_B=v, deconv_pow=deconv_pow, result=r)
    assert torch.equal(c.value, before)
    assert type(g) is type(c) and g.value.dtype == c.value.dtype
    got = cpu(g.value).astype('c16')
    if dtype == 'f8':
        assert_gradient(got, want, scale, sh)
    else:
        err = float(numpy.abs(got - want).max() / numpy.abs(want).max())
        print('f4: max |grad - grad_ref| / max |grad_ref| = %.4g (bound %.4g)' % (err, F4_VJP_TOL))
        assert (got[sh < 0] == 0).all()
        assert err <= F4_VJP_TOL
    # without result= one forward call is made for the counts: the same bits
    g2 = bispectrum_vjp(c, ke, v_B=v, deconv_pow=deconv_pow)
    assert torch.equal(g2.value, g.value)


# ---- 4. the per-target list -----------------------------------------------------------------------------------------------

def test_adjoint_pairs():
    nb = 6
    tri = numpy.array([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 2), (1, 2, 3), (2, 2, 2), (1, 1, 3), (3, 3, 5), (0, 2, 5),
                       (1, 1, 1), (2, 3, 3), (0, 3, 5)])
    coef = numpy.array([1.5, -2.0, 0.25, 3.0, -1.0, 0.5, 7.0, 0.0, numpy.nan, 4.0, numpy.inf, -0.125])
    want = {}
    for c, t in zip(coef, tri):
        if c == 0 or not numpy.isfinite(c):
            continue
        for pos in range(3):
            p, q = sorted(t[x] for x in range(3) if x != pos)
            want[(t[pos], p, q)] = want.get((t[pos], p, q), 0.0) + c
    offsets, pairs, weights = adjoint_pairs(tri, coef, nb)
    assert offsets.dtype == numpy.int32 and pairs.dtype == numpy.int32 and weights.dtype == numpy.float64
    assert offsets.shape == (nb + 1,) and pairs.shape == (len(want), 2) and weights.shape == (len(want),)
    assert offsets[0] == 0 and offsets[-1] == len(want) and (numpy.diff(offsets) >= 0).all()
    got = {}
    keys = []
    for s in range(nb):
        for e in range(offsets[s], offsets[s + 1]):
            key = (s, int(pairs[e, 0]), int(pairs[e, 1]))
            assert key not in got, 'an entry is not merged'
            got[key] = weights[e]
            keys.append(key)
    assert got == want
    assert keys == sorted(keys)                                   # by target, then p, then q
    # the merged weights: c, 2 c and 3 c
    assert got[(0, 0, 0)] == 3 * 1.5 and got[(0, 0, 1)] == 2 * -2.0 and got[(1, 0, 0)] == -2.0
    assert got[(1, 0, 1)] == 2 * 0.25 and got[(0, 1, 1)] == 0.25
    # shell 4 is in no bin, shell 5 only in dropped bins and in (0, 3, 5)
    assert offsets[4] == offsets[5] and offsets[6] - offsets[5] == 1
    # nothing kept: empty arrays of the right shapes
    o, p, w = adjoint_pairs(tri, numpy.zeros(len(tri)), nb)
    assert (o == 0).all() and o.shape == (nb + 1,) and p.shape == (0, 2) and w.shape == (0,)
    with pytest.raises(ValueError):
        adjoint_pairs(tri, coef[:-1], nb)
    with pytest.raises(ValueError):
        adjoint_pairs(tri, coef, 5)


# ---- 5. arguments -------------------------------------------------------------------------------------------------------

def test_gradient_arguments(gbe):
    pm = ParticleMesh([12, 12, 12], BoxSize=100.)
    c = density(pm, seed=1).r2c()
    kf = 2 * numpy.pi / 100.
    ke = [0.5 * kf, 1.5 * kf, 2.5 * kf]
    ntri = len(triangle_bins(ke))
    for fn in (lambda f, e, **kw: bispectrum_vjp(f, e, **kw), lambda f, e, **kw: bispectrum_jvp(f, e, c, **kw)):
        with pytest.raises(TypeError, match='r2c_vjp'):
            fn(pm.create(type='real'), ke)
        with pytest.raises(TypeError):
            fn(numpy.zeros((12, 12, 7), 'c16'), ke)
        with pytest.raises(NotImplementedError):
            fn(ParticleMesh([12, 12], BoxSize=100.).create(type='complex'), ke)
        with pytest.raises(ValueError, match='alias bound'):
            fn(c, [0.5 * kf, 1.5 * kf, 4.001 * kf])
        with pytest.raises(ValueError, match='kedges'):
            fn(c, [0.3, 0.1, 0.2])
        with pytest.raises(ValueError, match='PMX_BISPEC_MAX_SHELLS'):
            fn(c, numpy.linspace(0, 3 * kf, _abi.PMX_BISPEC_MAX_SHELLS + 2))
        with pytest.raises(ValueError, match='deconv_pow'):
            fn(c, ke, deconv_pow=-1)
        # a result of another mesh, of other edges, of another kind
        with pytest.raises(ValueError, match='result'):
            fn(c, ke, result=bispectrum(ParticleMesh([12, 12, 14], BoxSize=100.).create(type='complex'), ke))
        with pytest.raises(ValueError, match='result'):
            fn(c, ke, result=bispectrum(c, [0.5 * kf, 1.5 * kf, 2.6 * kf]))
        with pytest.raises(TypeError):
            fn(c, ke, result=bispectrum(c, ke).counts)
    # cotangents of the wrong length
    with pytest.raises(ValueError, match='v_B'):
        bispectrum_vjp(c, ke, v_B=numpy.ones(ntri + 1))
    with pytest.raises(ValueError, match='v_Q'):
        bispectrum_vjp(c, ke, v_Q=numpy.ones(ntri - 1))
    with pytest.raises(ValueError, match='v_power'):
        bispectrum_vjp(c, ke, v_power=numpy.ones(3))
    # the jvp sums over 2 nb fields: 32 shells at most, and a tangent of the field's layout
    wide = ParticleMesh([12, 12, 12], BoxSize=100.)
    with pytest.raises(ValueError, match='PMX_BISPEC_MAX_SHELLS'):
        bispectrum_jvp(c, numpy.linspace(0.1 * kf, 3.9 * kf, 34), c)
    with pytest.raises(ValueError, match='layout'):
        bispectrum_jvp(c, ke, wide.create(type=UntransposedComplexField))
    with pytest.raises(TypeError, match='r2c_vjp'):
        bispectrum_jvp(c, ke, pm.create(type='real'))
    # no cotangent: a zero gradient of the field's type
    cu = density(pm, seed=1).r2c(out=pm.create(type=UntransposedComplexField))
    g = bispectrum_vjp(cu, ke)
    assert isinstance(g, UntransposedComplexField) and float(g.value.abs().max()) == 0
    # a cotangent on empty bins alone: nothing either
    _, a, _, kb = brute_fields()
    r = bispectrum(a, kb)
    assert (r.counts == 0).any()
    g = bispectrum_vjp(a, kb, v_B=numpy.where(r.counts == 0, 1.0, 0.0), result=r)
    assert float(g.value.abs().max()) == 0


# ---- 6. ranks equal one ------------------------------------------------------------------------------------------------

def _ranks_equal_one(size, np_, Nmesh, edges=(0.5, 1.5, 2.5, 3.5)):
    from tests import thread_comm
    kf = 2 * numpy.pi / 100.
    ke = kf * numpy.array(edges)
    v = numpy.random.RandomState(3).normal(size=len(triangle_bins(ke)))
    results, empty = {}, {}

    def body(comm):
        pm = ParticleMesh(Nmesh, BoxSize=100., comm=comm, np=np_)
        c = density(pm, seed=5).r2c()
        empty[comm.rank] = c.value.numel() == 0 or pm.create(type='real').value.numel() == 0
        g = bispectrum_vjp(c, ke, v_B=v, deconv_pow=2)
        assert type(g) is type(c)
        results[comm.rank] = (tuple(int(s) for s in g.start), cpu(g.value))
    thread_comm.run_ranks(size, body)
    pm1 = ParticleMesh(Nmesh, BoxSize=100.)
    c1 = density(pm1, seed=5).r2c()
    r1 = bispectrum(c1, ke, deconv_pow=2)
    one = cpu(bispectrum_vjp(c1, ke, v_B=v, deconv_pow=2, result=r1).value)
    _, scale, sh = reference(c1, ke, 2, coefficients(v, r1.counts, [100.] * 3))
    assert numpy.abs(one).max() > 0
    assert sum(g.size for _, g in results.values()) == one.size
    for start, g in results.values():
        sel = tuple(slice(s, s + n) for s, n in zip(start, g.shape))
        assert (numpy.abs(g - one[sel]) <= F8_TOL * scale[sel]).all()
        assert (g[sh[sel] < 0] == 0).all()
    return empty


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
def test_ranks_equal_one(size, np_):
    backend.reset()
    backend.use(BispecGradOracleBackend())
    try:
        _ranks_equal_one(size, np_, [16, 16, 12])
    finally:
        backend.reset()


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(4, [4]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _ranks_equal_one(size, np_, [16, 16, 12])


@pytest.mark.gpu
def test_kernel_ranks_with_an_empty_block(hipbe):
    """six planes over eight ranks: two ranks hold no cell and no mode"""
    empty = _ranks_equal_one(8, [8], [6, 16, 12], edges=(0.5, 1.2, 2.0))
    assert any(empty.values())


# ---- 7., 8. pmx_bispec_pairsum ---------------------------------------------------------------------------------------------

def _pairsum_reference(blocks, offsets, pairs, weights):
    """G_s and sum_e |w_e| |D_p D_q| per shell; a pair that names no shell contributes nothing"""
    f = numpy.stack([b.astype('f8').reshape(-1) for b in blocks])
    nb = len(blocks)
    G, A = numpy.zeros_like(f), numpy.zeros_like(f)
    for s in range(nb):
        for a in range(offsets[s], offsets[s + 1], 4096):
            e = slice(a, min(a + 4096, offsets[s + 1]))
            p, q, w = pairs[e, 0], pairs[e, 1], weights[e]
            ok = (p >= 0) & (p < nb) & (q >= 0) & (q < nb)
            t = w[ok, None] * (f[p[ok]] * f[q[ok]])
            G[s] += t.sum(axis=0)
            A[s] += numpy.abs(t).sum(axis=0)
    return G.reshape((nb,) + blocks[0].shape), A.reshape((nb,) + blocks[0].shape)


def _run_pairsum(be, blocks, offsets, pairs, weights):
    """out of place, in place and a second call on last-axis-padded NaN-filled buffers (as the buffers of the in-place
    transforms are): the same bits from all three, the padding still NaN; returns the outputs"""
    dev = be.device
    dt = torch.from_numpy(blocks[0]).dtype
    shape = blocks[0].shape

    def padded(values):
        bufs, views = [], []
        for b in values:
            buf = torch.full(shape[:-1] + (shape[-1] + 3,), float('nan'), dtype=dt, device=dev)
            v = buf[..., :shape[-1]]
            if b is not None:
                v[...] = torch.from_numpy(b).to(dev)
            bufs.append(buf)
            views.append(v)
        return bufs, views
    ot, pt, wt = (torch.from_numpy(x).to(dev) for x in (offsets, pairs, weights))
    _, fields = padded(blocks)
    obufs, outs = padded([None] * len(blocks))
    be.bispec_pairsum(fields, outs, ot, pt, wt)
    for f, b in zip(fields, blocks):
        assert torch.equal(f.cpu(), torch.from_numpy(b)), 'out of place: a field has changed'
    first = [o.clone() for o in outs]
    for o in outs:
        o.fill_(float('nan'))
    be.bispec_pairsum(fields, outs, ot, pt, wt)
    ibufs, inplace = padded(blocks)
    be.bispec_pairsum(inplace, inplace, ot, pt, wt)
    for a, b, c, ob, ib in zip(first, outs, inplace, obufs, ibufs):
        assert torch.equal(a, b), 'two calls on the same input differ'
        assert torch.equal(a, c), 'in place and out of place differ'
        assert torch.isnan(ob[..., shape[-1]:]).all() and torch.isnan(ib[..., shape[-1]:]).all(), 'padding written'
    return numpy.stack([cpu(o) for o in first])


def assert_pairsum(got, G, A, dtype):
    bound = F8_TOL * A + (F4_ROUND * numpy.abs(G) if dtype == 'f4' else 0)
    err = numpy.abs(got.astype('f8') - G)
    assert numpy.isfinite(got).all(), 'a cell not written'
    print('max |G - G_ref| / bound = %.3g' % numpy.max(err / numpy.where(bound > 0, bound, 1)))
    assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('nb', [1, 2, 7, 33, 64])
def test_kernel_pairsum(hipbe, nb, dtype):
    """every triple i <= j <= l of nb shells with random coefficients (6545 triples at nb = 33): nb <= 16, <= 32 and
    above take the three chunk sizes"""
    rng = numpy.random.RandomState(nb)
    tri = _all_triples(nb)
    if nb == 33:
        assert len(tri) == 6545
    offsets, pairs, weights = adjoint_pairs(tri, rng.normal(size=len(tri)), nb)
    assert len(weights) <= 3 * _abi.PMX_BISPEC_MAX_TRIANGLES
    for shape in ([5, 7, 11], [1, 1, 3]):
        blocks = [rng.normal(size=shape).astype(dtype) for _ in range(nb)]
        G, A = _pairsum_reference(blocks, offsets, pairs, weights)
        assert_pairsum(_run_pairsum(hipbe, blocks, offsets, pairs, weights), G, A, dtype)


def _random_list(rng, nb, per_shell, bad=0):
    """a per-target list in random order with repeated entries and unsorted pairs (bad: entries naming no shell)"""
    counts = rng.randint(0, per_shell, size=nb)
    offsets = numpy.concatenate([[0], numpy.cumsum(counts)]).astype('i4')
    pairs = rng.randint(0, nb, size=(offsets[-1], 2)).astype('i4')
    pairs[rng.randint(0, len(pairs), size=len(pairs) // 4)] = pairs[0]
    for e in rng.randint(0, len(pairs), size=bad):
        pairs[e, rng.randint(2)] = (nb, -1, 1 << 20)[rng.randint(3)]
    return offsets, pairs, rng.normal(size=len(pairs))


@pytest.mark.gpu
def test_kernel_pairsum_many_chunks_and_a_random_list(hipbe):
    """more chunks than workgroups (a workgroup walks several), a list in random order with repeated entries and with
    pairs that name no shell; an empty list writes zeros"""
    rng = numpy.random.RandomState(0)
    shape = [70, 64, 65]
    blocks = [rng.normal(size=shape) for _ in range(7)]
    offsets, pairs, weights = _random_list(rng, 7, 40, bad=5)
    assert ((pairs < 0) | (pairs >= 7)).any()
    G, A = _pairsum_reference(blocks, offsets, pairs, weights)
    assert_pairsum(_run_pairsum(hipbe, blocks, offsets, pairs, weights), G, A, 'f8')
    got = _run_pairsum(hipbe, blocks[:3], numpy.zeros(4, 'i4'), numpy.zeros((0, 2), 'i4'), numpy.zeros(0))
    assert (got == 0).all()


@pytest.mark.gpu
def test_kernel_pairsum_edges(hipbe):
    dev = hipbe.device
    offsets, pairs, weights = (torch.from_numpy(x).to(dev) for x in adjoint_pairs(_all_triples(3), numpy.ones(10), 3))
    # an empty block is a no-op
    hipbe.bispec_pairsum([torch.zeros((0, 4, 5), dtype=torch.float64, device=dev)] * 3,
                         [torch.zeros((0, 4, 5), dtype=torch.float64, device=dev)] * 3, offsets, pairs, weights)
    # limits
    one = torch.ones((2, 4, 5), dtype=torch.float64, device=dev)
    out = [torch.empty_like(one) for _ in range(65)]
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_pairsum([one] * 65, out, torch.zeros(66, dtype=torch.int32, device=dev), pairs, weights)
    big = 3 * _abi.PMX_BISPEC_MAX_TRIANGLES + 1
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_pairsum([one] * 3, out[:3], offsets, torch.zeros((big, 2), dtype=torch.int32, device=dev),
                             torch.zeros(big, dtype=torch.float64, device=dev))
    # the bins (0, 0, 0) .. (2, 2, 2) of three fields of ones with unit coefficients: 3 + 2 + 2 + 1 + 1 + 1 per shell
    hipbe.bispec_pairsum([one] * 3, out[:3], offsets, pairs, weights)
    assert all((o == 10).all() for o in out[:3])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernel_pairsum_blocks_of_one_and_two_dimensions(hipbe, dtype):
    """the entry takes blocks of 1 to 3 dimensions: a vector and a matrix with a padded last axis"""
    rng = numpy.random.RandomState(2)
    offsets, pairs, weights = _random_list(rng, 5, 12)
    for shape in ([37], [1], [5, 9], [700, 3]):
        blocks = [rng.normal(size=shape).astype(dtype) for _ in range(5)]
        G, A = _pairsum_reference(blocks, offsets, pairs, weights)
        assert_pairsum(_run_pairsum(hipbe, blocks, offsets, pairs, weights), G, A, dtype)


# ---- 9. pmx_bispec_shells_vjp ------------------------------------------------------------------------------------------------

def _shells_adjoint(be, c, ke, deconv_pow, dtype):
    """sum_s <bispec_shells(a)_s, y_s> == <a, bispec_shells_vjp(y)> for independent random y_s, within 1e-13 of the sum
    of the absolute terms.  With a window, f4 storage rounds a / W on one side and y / W on the other to float: each
    term then carries two half-ulps of float, 2 * 2^-24 <= 1.2e-7 of its modulus, on top (derived, not measured);
    without a window both entries copy and the identity holds as for f8"""
    pm = c.pm
    nb = len(ke) - 1
    kt = torch.from_numpy(ke).to(be.device)
    rng = numpy.random.RandomState(7)
    shape = tuple(c.value.shape)
    ys = [pm.create(type=type(c)) for _ in range(nb)]
    for y in ys:
        y.value[...] = torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape)).to(y.value.dtype)
    outs = [pm.create(type=type(c)) for _ in range(nb)]
    be.bispec_shells(c.value, [o.value for o in outs], c.start, pm.Nmesh, pm.BoxSize, kt, deconv_pow, False)
    g = pm.create(type=type(c))
    torch.view_as_real(g.value).fill_(float('nan'))
    be.bispec_shells_vjp([y.value for y in ys], g.value, c.start, pm.Nmesh, pm.BoxSize, kt, deconv_pow)
    sh, _ = _shells_of(c.start, shape, pm.Nmesh, pm.BoxSize, ke)
    gv = cpu(g.value).astype('c16')
    assert numpy.isfinite(gv.real).all() and numpy.isfinite(gv.imag).all(), 'an element not written'
    assert (sh < 0).sum() > 0 and (gv[sh < 0] == 0).all(), 'a mode in no shell is not exactly 0'
    assert (gv[sh >= 0] != 0).all()
    lhs_terms = sum(numpy.conj(cpu(o.value).astype('c16')) * cpu(y.value).astype('c16') for o, y in zip(outs, ys))
    rhs_terms = numpy.conj(cpu(c.value).astype('c16')) * gv
    tol = F8_TOL + (2 * F4_ROUND if dtype == 'f4' and deconv_pow else 0)
    scale = numpy.abs(rhs_terms).sum()
    print('shells adjoint: |difference| / sum |terms| = %.3g (bound %.3g)'
          % (abs(lhs_terms.sum() - rhs_terms.sum()) / scale, tol))
    assert abs(lhs_terms.sum() - rhs_terms.sum()) <= tol * scale
    if not deconv_pow:
        # the gather itself: y of the mode's shell, bit for bit
        want = numpy.zeros(shape, dtype='c16')
        for s, y in enumerate(ys):
            want = numpy.where(sh == s, cpu(y.value).astype('c16'), want)
        assert (gv == want).all()


def _radius_edges(Nmesh, BoxSize):
    """edges exactly on mode radii (multiples of the fundamental of the longest axis) that leave k = 0 and the corner
    of the mesh outside"""
    kf = 2 * numpy.pi / max(BoxSize)
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(Nmesh, BoxSize)))
    return kf * numpy.arange(1, max(3, int(0.6 * kmax / kf)))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
def test_kernel_shells_vjp(hipbe, kind, dtype):
    Nmesh, BoxSize = [16, 12, 20], [100., 80., 120.]
    c, _ = parity_field(kind, Nmesh, BoxSize, dtype)
    ke = _radius_edges(Nmesh, BoxSize)
    for deconv_pow in (0, 2):
        _shells_adjoint(hipbe, c, ke, deconv_pow, dtype)
    pm = c.pm
    kt = torch.from_numpy(ke).to(hipbe.device)
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_shells_vjp([c.value] * 65, pm.create(type=type(c)).value, c.start, pm.Nmesh, pm.BoxSize, kt, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('Nmesh,BoxSize', [([32], [100.]), ([16, 12], [100., 80.])])
def test_kernel_shells_vjp_of_one_and_two_dimensions(hipbe, Nmesh, BoxSize, dtype):
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=dtype)
    c = density(pm, seed=6).r2c()
    for deconv_pow in (0, 2):
        _shells_adjoint(hipbe, c, _radius_edges(Nmesh, BoxSize), deconv_pow, dtype)


# ---- 10. resources (compiles for gfx950 on the CPU) ----------------------------------------------------------------------

def test_bispec_gradient_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_bispec_grad.hip')
    assert sum('pairsum_kernel' in k for k in t) == 6 and sum('shells_vjp_kernel' in k for k in t) == 2, sorted(t)
    for name, r in t.items():
        assert r['ScratchSize'] == 0, (name, r)
