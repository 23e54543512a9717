"""pmesh_amd.power gradients (power_spectrum_vjp, power_spectrum_jvp; csrc/pmx_power_grad.hip).

The checks are the adjoint identity between the vjp and the jvp, finite differences of power_spectrum itself, the
kernel against a numpy restatement of pmx_power_vjp written from the header text (oracle_vjp below), several ranks
against one, and the whole differentiable chain white noise -> Tabulated -> lpt -> paint -> r2c -> power_spectrum ->
chi^2 against central differences in the table values.  Under -m "not gpu" the entry is served by the restatement
(PowerGradOracleBackend, on test_power.PowerOracleBackend), so the host layer runs without a GPU; under -m gpu the
same tests run on the kernel.
"""
import os
import subprocess
import sys

import numpy
import pytest
import torch
from numpy.polynomial import legendre

from pmesh_amd import _abi, backend
from pmesh_amd import pm as _pm
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.power import power_spectrum, power_spectrum_jvp, power_spectrum_vjp
from tests.test_power import PowerOracleBackend, _sinc_pow, expected, kf_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement -----------------------------------------------------------------------------------------------

def oracle_vjp(a, b, k, idx, nmesh, volume, kedges, coef, muedges=None, los=None, ells=(), deconv_pow=0,
               hermitian=False):
    """numpy restatement of pmx_power_vjp on one block (arguments as test_power.oracle_sums, coef the coefficient
    table of the header): returns (grad_a, grad_b), grad_b None for the auto spectrum"""
    a = numpy.asarray(a).astype('c16')
    cross = b is not None
    b = a if b is None else numpy.asarray(b).astype('c16')
    ndim = a.ndim
    if los is None:
        los = [0.0] * (ndim - 1) + [1.0]
    kedges = numpy.asarray(kedges, dtype='f8')
    nk = len(kedges) - 1
    k2 = 0
    for kd in k:
        k2 = k2 + kd * kd
    kmag = numpy.broadcast_to(numpy.sqrt(k2), a.shape)
    kl = 0
    for kd, ld in zip(k, los):
        kl = kl + kd * ld
    with numpy.errstate(invalid='ignore', divide='ignore'):
        mu = numpy.where(kmag > 0, numpy.broadcast_to(kl, a.shape) / kmag, 0.0)
    D = numpy.ones(a.shape)
    if deconv_pow:
        for d in range(ndim):
            n = int(nmesh[d])
            s = idx[d] - n * (idx[d] >= n // 2)
            D = D * _sinc_pow(s.astype('f8') * (2 * numpy.pi / n), deconv_pow)
    h = numpy.zeros(a.shape)
    if hermitian:
        il = idx[-1]
        h = numpy.broadcast_to(((il != 0) & (il != int(nmesh[-1]) // 2)).astype('f8'), a.shape)
    kb = numpy.digitize(kmag, kedges) - 1
    ok = (kb >= 0) & (kb < nk)
    j = numpy.where(ok, kb, 0)
    sc = 2 + 2 * len(ells)
    nmu = 0 if muedges is None else len(muedges) - 1
    c1 = coef[:nk * sc].reshape(nk, sc)
    c1 = c1[:, 0::2] + 1j * c1[:, 1::2]                 # (nk, 1 + npoles)
    if nmu:
        me = numpy.asarray(muedges, dtype='f8')
        c2 = coef[nk * sc:].reshape(nk, nmu, 2)
        c2 = c2[..., 0] + 1j * c2[..., 1]

    def F(m):
        f = c1[j, 0]
        for p, ell in enumerate(ells):
            f = f + legendre.legval(m, [0] * ell + [1]) * c1[j, 1 + p]
        if nmu:
            mb = numpy.digitize(m, me) - 1
            mb[m == me[-1]] = nmu - 1
            good = (mb >= 0) & (mb < nmu)
            f = f + numpy.where(good, c2[j, numpy.where(good, mb, 0)], 0.0)
        return f
    q = (volume / D) * (numpy.conj(F(mu)) + h * F(-mu))
    q = numpy.where(ok, q, 0.0)
    w = 1.0 + h
    if cross:
        return numpy.conj(q) * b / w, q * a / w
    return 2.0 * q.real * a / w, None


class PowerGradOracleBackend(PowerOracleBackend):
    """PowerOracleBackend with pmx_power_vjp served by oracle_vjp"""
    name = 'oracle-power-grad'

    def power_vjp(self, params, a, b, grad_a, grad_b, start, nmesh, boxsize, kedges, muedges, coef):
        if a.numel() == 0:
            return
        nd = a.dim()
        k, idx = _pm._block_coords(start, tuple(a.shape), nmesh, boxsize, 'f8', 'cpu', True)
        ga, gb = oracle_vjp(a.numpy(), None if b is None else b.numpy(), [x.numpy() for x in k],
                            [i.numpy() for i in idx], nmesh, params.volume, kedges.numpy(), coef.numpy(),
                            None if muedges is None else muedges.numpy(), list(params.los)[:nd],
                            list(params.poles)[:params.npoles], params.deconv_pow, params.hermitian)
        grad_a.copy_(torch.from_numpy(ga))
        if b is not None:
            grad_b.copy_(torch.from_numpy(gb))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def gbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(PowerGradOracleBackend())
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


def make_pm(kind, Nmesh, BoxSize, dtype='f8', **kw):
    cdt = {'f8': 'c16', 'f4': 'c8'}[dtype]
    return ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=cdt if kind == 'c2c' else dtype, **kw)


def ftype(kind):
    return UntransposedComplexField if kind == 'U' else TransposedComplexField


def random_field(pm, kind, seed):
    """a complex field of the layout `kind` ('T', 'U'; 'c2c' on a complex mesh) with random stored modes"""
    c = pm.create(type=ftype(kind))
    rng = numpy.random.RandomState(seed)
    shape = tuple(c.value.shape)
    c.value[...] = torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape)).to(c.value.device)
    return c


def holey_edges(pm):
    """non-uniform k edges that leave k = 0 and the corner of the mesh outside and whose first bin is empty"""
    kmin = 2 * numpy.pi / float(numpy.max(pm.BoxSize))
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(pm.Nmesh, pm.BoxSize)))
    return numpy.concatenate([[0.3 * kmin, 0.6 * kmin], numpy.geomspace(0.95 * kmin, 0.8 * kmax, 9)])


def cotangents(nk, nmu, poles, seed):
    rng = numpy.random.RandomState(seed)

    def c(*shape):
        return rng.normal(size=shape) + 1j * rng.normal(size=shape)
    return dict(v_power=c(nk), v_poles={ell: c(nk) for ell in poles}, v_power2d=c(nk, nmu) if nmu else None)


def pairing(v, res):
    """Re sum conj(v) P over power, poles and power2d of a PowerResult of tangents; empty bins contribute nothing"""
    def dot(x, y, n):
        return float(numpy.sum((numpy.conj(x) * numpy.where(n > 0, y, 0.0)).real))
    s = dot(v['v_power'], res.power, res.modes) if v.get('v_power') is not None else 0.0
    for ell, x in (v.get('v_poles') or {}).items():
        s += dot(x, res.poles[ell], res.modes)
    if v.get('v_power2d') is not None:
        s += dot(v['v_power2d'], res.power2d, res.modes2d)
    return s


def expected_vjp(field, kedges, v, other=None, muedges=None, los=None, poles=(), deconv_pow=0):
    """oracle_vjp for a one-rank field with the oracle's own counts: wavenumbers from the f8 mesh of the geometry"""
    pm = field.pm
    res = expected(field, kedges, other=other, muedges=muedges, los=los, poles=poles, deconv_pow=deconv_pow)
    pm8 = ParticleMesh(pm.Nmesh, BoxSize=pm.BoxSize, comm=pm.comm, np=pm.np,
                       dtype='c16' if not field.compressed else 'f8')
    f8 = pm8.create(type=type(field))
    k = [cpu(x) for x in f8.x]
    idx = [cpu(i) for i in f8.i]
    nk = len(kedges) - 1
    nmu = 0 if muedges is None else len(muedges) - 1
    sc = 2 + 2 * len(poles)
    coef = numpy.zeros(nk * sc + nk * nmu * 2)
    c1 = coef[:nk * sc].reshape(nk, sc)
    inv = numpy.where(res.modes > 0, 1.0 / numpy.maximum(res.modes, 1), 0.0)
    cols = [v['v_power'] * inv] + [(2 * ell + 1) * v['v_poles'][ell] * inv for ell in poles]
    for i, c in enumerate(cols):
        c1[:, 2 * i], c1[:, 2 * i + 1] = c.real, c.imag
    if nmu:
        inv2 = numpy.where(res.modes2d > 0, 1.0 / numpy.maximum(res.modes2d, 1), 0.0)
        c2 = coef[nk * sc:].reshape(nk, nmu, 2)
        c2[..., 0], c2[..., 1] = (v['v_power2d'] * inv2).real, (v['v_power2d'] * inv2).imag
    if los is not None:
        los = numpy.asarray(los, dtype='f8') / numpy.sqrt(numpy.sum(numpy.square(los)))
    return oracle_vjp(cpu(field.value), None if other is None else cpu(other.value), k, idx, pm.Nmesh,
                      float(numpy.prod(pm.BoxSize)), kedges, coef, muedges, los, list(poles), deconv_pow,
                      field.compressed)


def same_field(got, want, storage='f8'):
    """the tolerance of test_power.assert_same (1e-12 of the scale of the result) for f8 storage; a complex64 result
    is a double rounded to float once more: half a unit in the last place of float32 (2^-24) per component on top"""
    got, want = numpy.asarray(got).astype('c16'), numpy.asarray(want)
    scale = numpy.abs(want).max() if want.size else 1.0
    tol = 1e-12 * max(scale, 1e-300)
    if storage == 'f4':
        tol = tol + 2.0 ** -24 * numpy.maximum(numpy.abs(want.real), numpy.abs(want.imag))
    err = numpy.maximum(numpy.abs(got.real - want.real), numpy.abs(got.imag - want.imag))
    assert (err <= tol).all(), (float(err.max()), float(scale))


# ---- arguments (both backends) -------------------------------------------------------------------------------------

def test_gradient_arguments(gbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    c = random_field(pm, 'T', 1)
    e = kf_edges(pm)
    nk = len(e) - 1
    for fn in (power_spectrum_vjp, power_spectrum_jvp):
        # the forward's cases
        for bad in ([1.0], [0.0, 0.0], [0.3, 0.1, 0.2], [0, numpy.nan], [[0, 1], [1, 2]]):
            with pytest.raises(ValueError, match='kedges'):
                fn(c, bad)
        with pytest.raises(ValueError, match='muedges'):
            fn(c, e, muedges=[-1.5, 0, 1])
        with pytest.raises(ValueError, match='muedges'):
            fn(c, e, muedges=[0, 0.5, 0.5, 1])
        with pytest.raises(ValueError, match='PMX_POWER_MAX_MUBINS'):
            fn(c, e, muedges=numpy.linspace(-1, 1, _abi.PMX_POWER_MAX_MUBINS + 2))
        with pytest.raises(ValueError, match='PMX_POWER_MAX_KBINS'):
            fn(c, numpy.arange(_abi.PMX_POWER_MAX_KBINS + 2, dtype='f8'))
        with pytest.raises(ValueError, match='PMX_POWER_MAX_POLES'):
            fn(c, e, poles=(0, 1, 2, 3, 4, 5))
        for bad in ((9,), (0, 0), (-1,)):
            with pytest.raises(ValueError, match='poles'):
                fn(c, e, poles=bad)
        with pytest.raises(ValueError, match='los'):
            fn(c, e, los=[0, 0, 0])
        with pytest.raises(ValueError, match='los'):
            fn(c, e, los=[0, 1])
        with pytest.raises(ValueError, match='deconv_pow'):
            fn(c, e, deconv_pow=-1)
        with pytest.raises(TypeError):
            fn(numpy.zeros((8, 8, 5), 'c16'), e)
        other = ParticleMesh([8, 8, 16], BoxSize=100.).create(type='complex')
        with pytest.raises(ValueError, match='mesh|layout'):
            fn(c, e, other=other)
        with pytest.raises(ValueError, match='layout'):
            fn(c, e, other=pm.create(type=UntransposedComplexField))
        with pytest.raises(ValueError, match='layout'):
            fn(c, e, other=ParticleMesh([8, 8, 8], BoxSize=100., dtype='f4').create(type='complex'))
        # a RealField is not differentiated through its temporary r2c
        with pytest.raises(TypeError, match='r2c_vjp'):
            fn(pm.create(type='real'), e)
        with pytest.raises(TypeError, match='r2c_vjp'):
            fn(c, e, other=pm.create(type='real'))
    with pytest.raises(NotImplementedError):
        power_spectrum_vjp(ParticleMesh([4, 4, 4, 4], BoxSize=1.).create(type='complex'), [0, 1, 2])
    # cotangents
    with pytest.raises(ValueError, match='v_power'):
        power_spectrum_vjp(c, e, v_power=numpy.ones(nk + 1))
    with pytest.raises(ValueError, match='v_poles'):
        power_spectrum_vjp(c, e, v_poles={2: numpy.ones(nk - 1)}, poles=(0, 2))
    with pytest.raises(ValueError, match='v_poles'):
        power_spectrum_vjp(c, e, v_poles={4: numpy.ones(nk)}, poles=(0, 2))
    with pytest.raises(ValueError, match='muedges'):
        power_spectrum_vjp(c, e, v_power2d=numpy.ones((nk, 3)))
    with pytest.raises(ValueError, match='v_power2d'):
        power_spectrum_vjp(c, e, v_power2d=numpy.ones((nk, 3)), muedges=[-1, 0, 1])
    with pytest.raises(ValueError, match='result'):
        power_spectrum_vjp(c, e, v_power=numpy.ones(nk), result=power_spectrum(c, e[:-1]))
    # tangents
    with pytest.raises(ValueError, match='v_other'):
        power_spectrum_jvp(c, e, v_other=c)
    with pytest.raises(ValueError, match='layout'):
        power_spectrum_jvp(c, e, v_field=pm.create(type=UntransposedComplexField))
    # no cotangent: a zero gradient of the field's type; no tangent: zero tangents with the forward's counts
    cu = random_field(pm, 'U', 2)
    g = power_spectrum_vjp(cu, e)
    assert isinstance(g, UntransposedComplexField) and float(g.value.abs().max()) == 0
    ga, gb = power_spectrum_vjp(cu, e, other=cu)
    assert float(ga.value.abs().max()) == 0 and float(gb.value.abs().max()) == 0
    t = power_spectrum_jvp(cu, e, poles=(0,))
    f = power_spectrum(cu, e, poles=(0,))
    # (the sums of |k| are float atomics: equal up to their last bits)
    assert (t.modes == f.modes).all()
    numpy.testing.assert_allclose(t.k, f.k, rtol=1e-12, equal_nan=True)
    assert (t.power[f.modes > 0] == 0).all() and (t.poles[0][f.modes > 0] == 0).all()


# ---- the adjoint identity (both backends) --------------------------------------------------------------------------

ADJOINT = [
    # kind, Nmesh, BoxSize, muedges, poles, deconv_pow, los, cross
    ('T', [16, 12, 10], [40., 30., 50.], [-1, -0.4, 0, 0.3, 1.0], (0, 2, 4), 2, [1, 1, 0.5], True),
    ('T', [16, 12, 10], [40., 30., 50.], None, (0, 2, 4), 0, None, False),
    ('U', [16, 12, 10], [40., 30., 50.], [0, 0.3, 0.7, 1.0], (0, 1, 2), 2, [0.3, -1, 2], False),
    ('U', [12, 10, 16], 60., [-1, 0, 1], (), 0, None, True),
    ('c2c', [10, 12, 8], [40., 30., 50.], [-1, -0.4, 0, 0.3, 1.0], (0, 1, 4), 2, [1, 1, 0.5], True),
    ('c2c', [10, 12, 8], 30., None, (0, 2), 0, None, False),
    ('T', [24, 20], [50., 40.], [-1, -0.2, 0.5, 1.0], (0, 2, 4), 2, [1, 2], False),
    ('U', [20, 24], [50., 40.], [-1, -0.2, 0.5, 1.0], (0, 3), 0, None, True),
    ('c2c', [12, 16], 20., None, (0, 2), 2, [1, -1], True),
    ('T', [64], 10., [-1, 0, 1], (0, 2), 2, None, False),
    ('T', [48], 10., None, (), 0, None, True),
]


@pytest.mark.parametrize('kind,Nmesh,BoxSize,muedges,poles,deconv_pow,los,cross', ADJOINT)
def test_adjoint_identity(gbe, kind, Nmesh, BoxSize, muedges, poles, deconv_pow, los, cross):
    """Re vdot(v, jvp(u)) == Re(u.cdot(vjp(v))), summed over both fields for the cross form; the edges leave modes
    outside and the first bin empty"""
    pm = make_pm(kind, Nmesh, BoxSize)
    a, ua = random_field(pm, kind, 3), random_field(pm, kind, 4)
    b, ub = (random_field(pm, kind, 5), random_field(pm, kind, 6)) if cross else (None, None)
    e = holey_edges(pm)
    nk, nmu = len(e) - 1, 0 if muedges is None else len(muedges) - 1
    v = cotangents(nk, nmu, poles, 7)
    kw = dict(other=b, muedges=muedges, los=los, poles=poles, deconv_pow=deconv_pow)
    before = a.value.clone()
    fwd = power_spectrum(a, e, **kw)
    assert fwd.modes[0] == 0 and 0 < fwd.modes.sum() < numpy.prod(Nmesh)
    tan = power_spectrum_jvp(a, e, v_field=ua, v_other=ub, **kw)
    assert (tan.modes == fwd.modes).all()
    grad = power_spectrum_vjp(a, e, result=fwd, **dict(kw, **v))
    assert torch.equal(a.value, before)
    lhs = pairing(v, tan)
    if cross:
        assert type(grad[0]) is type(a) and type(grad[1]) is type(b)
        rhs = ua.cdot(grad[0]).real + ub.cdot(grad[1]).real
        # one tangent at a time, and the counts from a forward call of its own
        g2 = power_spectrum_vjp(a, e, **dict(kw, **v))
        assert torch.equal(g2[0].value, grad[0].value) and torch.equal(g2[1].value, grad[1].value)
        only_b = pairing(v, power_spectrum_jvp(a, e, v_other=ub, **kw))
        assert abs(only_b - ub.cdot(grad[1]).real) <= 1e-10 * max(abs(lhs), abs(rhs))
    else:
        assert type(grad) is type(a)
        rhs = ua.cdot(grad).real
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    assert abs(lhs) > 0


# ---- finite differences (both backends) ----------------------------------------------------------------------------

def _loss(v, c, e, **kw):
    return pairing(v, power_spectrum(c, e, **kw))


@pytest.mark.parametrize('kind,Nmesh,BoxSize', [('T', [16, 12, 10], [40., 30., 50.]), ('U', [20, 24], [50., 40.]),
                                                ('c2c', [10, 12, 8], 30.)])
@pytest.mark.parametrize('cross', [False, True])
def test_vjp_single_modes(gbe, kind, Nmesh, BoxSize, cross):
    """steps in the real and the imaginary part of single stored modes: L is quadratic (auto) or linear (cross) in
    a field, so the central difference is the derivative up to rounding; along the unit step at a stored mode
    Re(u.cdot(grad)) is its Hermitian weight times the component of grad"""
    pm = make_pm(kind, Nmesh, BoxSize)
    nd = len(Nmesh)
    a = random_field(pm, kind, 8)
    b = random_field(pm, kind, 9) if cross else None
    e = holey_edges(pm)
    muedges = [-1, -0.4, 0, 0.3, 1.0]
    poles = (0, 1, 2)
    los = [1, 1, 0.5][:nd]
    v = cotangents(len(e) - 1, len(muedges) - 1, poles, 10)
    kw = dict(muedges=muedges, los=los, poles=poles, deconv_pow=2)
    grad = power_spectrum_vjp(a, e, other=b, **dict(kw, **v))
    grads = grad if cross else (grad,)
    w = a._hermitian_weight()
    w = numpy.ones(tuple(a.value.shape)) if w is None else numpy.broadcast_to(cpu(w), tuple(a.value.shape))
    shape = tuple(a.value.shape)
    rng = numpy.random.RandomState(11)
    modes = [tuple(int(rng.randint(n)) for n in shape) for _ in range(5)]
    modes += [tuple(0 for _ in shape), tuple(1 if d < nd - 1 else 0 for d in range(nd))]
    dx = 1e-3
    for which, g in enumerate(grads):
        g = cpu(g.value)
        for ind in modes:
            for part in (0, 1):
                def at(eps):
                    fields = [a, b]
                    c = pm.create(type=type(a))
                    c.value[...] = fields[which].value
                    c.value[ind] += eps if part == 0 else 1j * eps
                    fields[which] = c
                    return _loss(v, fields[0], e, other=fields[1], **kw)
                ng = (at(dx) - at(-dx)) / (2 * dx)
                ag = w[ind] * (g[ind].real if part == 0 else g[ind].imag)
                numpy.testing.assert_allclose(ng, ag, rtol=1e-6, atol=1e-6 * numpy.abs(g).max())


@pytest.mark.parametrize('cross', [False, True])
def test_jvp_is_central_difference(gbe, cross):
    """the raw sums are bilinear in (a, b): the central difference of the forward along (ua, ub) is the jvp"""
    pm = make_pm('T', [16, 12, 10], [40., 30., 50.])
    a, ua = random_field(pm, 'T', 12), random_field(pm, 'T', 13)
    b, ub = (random_field(pm, 'T', 14), random_field(pm, 'T', 15)) if cross else (None, None)
    e = holey_edges(pm)
    kw = dict(muedges=[-1, -0.4, 0, 0.3, 1.0], los=[1, 1, 0.5], poles=(0, 1, 2), deconv_pow=2)
    tan = power_spectrum_jvp(a, e, v_field=ua, v_other=ub, other=b, **kw)

    def shifted(c, u, eps):
        if c is None:
            return None
        out = pm.create(type=type(c))
        out.value[...] = c.value + eps * u.value
        return out
    p = power_spectrum(shifted(a, ua, 0.5), e, other=shifted(b, ub, 0.5), **kw)
    m = power_spectrum(shifted(a, ua, -0.5), e, other=shifted(b, ub, -0.5), **kw)
    scale = numpy.nanmax(numpy.abs(p.power))
    numpy.testing.assert_allclose(tan.power, p.power - m.power, rtol=0, atol=1e-11 * scale, equal_nan=True)
    numpy.testing.assert_allclose(tan.power2d, p.power2d - m.power2d, rtol=0, atol=1e-11 * scale, equal_nan=True)
    for ell in kw['poles']:
        numpy.testing.assert_allclose(tan.poles[ell], p.poles[ell] - m.poles[ell], rtol=0,
                                      atol=1e-11 * (2 * ell + 1) * scale, equal_nan=True)
    assert (tan.modes == p.modes).all() and (tan.modes2d == p.modes2d).all()
    numpy.testing.assert_allclose(tan.k, p.k, rtol=1e-12, equal_nan=True)
    numpy.testing.assert_allclose(tan.mu2d, p.mu2d, rtol=0, atol=1e-12, equal_nan=True)


# ---- the kernel against the restatement (GPU) ----------------------------------------------------------------------

def _kernel_fields(kind, dtype, Nmesh=(48, 32, 40), BoxSize=(200., 150., 180.)):
    pm = make_pm(kind, list(Nmesh), list(BoxSize), dtype)
    a, b = random_field(pm, kind, 2), random_field(pm, kind, 3)
    return pm, a, b


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernel_layouts_mu_poles_cross(hipbe, kind, dtype):
    """the layouts, dtypes and arguments of test_power.test_kernel_layouts_mu_poles_cross"""
    pm, a, b = _kernel_fields(kind, dtype)
    e = numpy.concatenate([[0.0], numpy.geomspace(0.01, 0.6, 30)])
    me = numpy.array([-1, -0.7, -0.2, 0, 0.1, 0.5, 0.9, 1.0])
    for other, poles, extra in ((None, (0, 2, 4), {}), (b, (0, 1, 2, 4), {}),
                                (None, (3, 8), dict(los=[0.3, -1, 2], deconv_pow=2)),
                                (b, (3, 8), dict(los=[0.3, -1, 2], deconv_pow=2))):
        v = cotangents(len(e) - 1, len(me) - 1, poles, 20)
        got = power_spectrum_vjp(a, e, other=other, muedges=me, poles=poles, **dict(extra, **v))
        want = expected_vjp(a, e, v, other=other, muedges=me, poles=poles, **extra)
        if other is None:
            same_field(cpu(got.value), want[0], dtype)
        else:
            same_field(cpu(got[0].value), want[0], dtype)
            same_field(cpu(got[1].value), want[1], dtype)
    # no mu table, no poles; and every column alone
    v = cotangents(len(e) - 1, 0, (), 21)
    same_field(cpu(power_spectrum_vjp(a, e, v_power=v['v_power']).value), expected_vjp(a, e, v)[0], dtype)
    v = cotangents(len(e) - 1, len(me) - 1, (0, 2), 22)
    only2d = dict(v_power=0 * v['v_power'], v_poles={ell: 0 * x for ell, x in v['v_poles'].items()},
                  v_power2d=v['v_power2d'])
    got = power_spectrum_vjp(a, e, v_power2d=v['v_power2d'], muedges=me, poles=(0, 2))
    same_field(cpu(got.value), expected_vjp(a, e, only2d, muedges=me, poles=(0, 2))[0], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('Nmesh,BoxSize', [([16, 16, 16], 100.), ([45, 45, 45], 100.), ([32, 48, 64], [100., 120., 200.]),
                                           ([64, 48], [100., 70.]), ([33, 40], 10.), ([64], 80.), ([100], 3.)])
def test_kernel_uniform_edges(hipbe, Nmesh, BoxSize):
    """kedges = arange(0, kmax, k_f): many modes sit exactly on edges and must take the forward's bin"""
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize)
    a = random_field(pm, 'T', 4)
    e = kf_edges(pm)
    v = cotangents(len(e) - 1, 0, (0, 2, 4), 23)
    got = power_spectrum_vjp(a, e, v_power=v['v_power'], v_poles=v['v_poles'], poles=(0, 2, 4))
    same_field(cpu(got.value), expected_vjp(a, e, v, poles=(0, 2, 4))[0])


@pytest.mark.gpu
def test_kernel_fine_edges_take_several_windows(hipbe):
    """the 20 000 bins of test_power.test_kernel_fine_edges_take_several_windows: a tile takes one pass per window of
    coefficient rows and every mode is written by exactly one of them"""
    pm = ParticleMesh([64, 64, 64], BoxSize=100.)
    a, b = random_field(pm, 'T', 5), random_field(pm, 'T', 6)
    e = numpy.linspace(0, 3.5, 20001)
    me = numpy.linspace(-1, 1, 11)
    v = cotangents(len(e) - 1, 0, (), 24)
    got = power_spectrum_vjp(a, e, v_power=v['v_power'])
    same_field(cpu(got.value), expected_vjp(a, e, v)[0])
    e8 = e[::8]
    v = cotangents(len(e8) - 1, len(me) - 1, (0, 2, 4), 25)
    got = power_spectrum_vjp(a, e8, other=b, muedges=me, poles=(0, 2, 4), **v)
    want = expected_vjp(a, e8, v, other=b, muedges=me, poles=(0, 2, 4))
    same_field(cpu(got[0].value), want[0])
    same_field(cpu(got[1].value), want[1])
    # edges that start above and end below the modes of whole tiles: those tiles are zero
    e = numpy.linspace(1.0, 1.6, 5001)
    v = cotangents(len(e) - 1, 0, (), 26)
    got = power_spectrum_vjp(a, e, v_power=v['v_power'])
    same_field(cpu(got.value), expected_vjp(a, e, v)[0])


# ---- ranks equal one -----------------------------------------------------------------------------------------------

def ranks_case(comm=None, np_=None, Nmesh=(16, 16, 12)):
    """the gradients and tangents of one configuration on the mesh of `comm`: (start, grad_a, grad_b, tangent)"""
    kw = {} if comm is None else dict(comm=comm, np=np_)
    pm = ParticleMesh(list(Nmesh), BoxSize=100., **kw)
    a = pm.generate_whitenoise(5, unitary=False, type='complex')
    b = pm.generate_whitenoise(6, unitary=False, type='complex')
    e = holey_edges(pm)
    me = numpy.linspace(-1, 1, 4)
    v = cotangents(len(e) - 1, len(me) - 1, (0, 2), 30)
    ga, gb = power_spectrum_vjp(a, e, other=b, muedges=me, poles=(0, 2), los=[1, 0.5, 1], deconv_pow=2, **v)
    tan = power_spectrum_jvp(a, e, v_field=b, v_other=a, other=b, muedges=me, poles=(0, 2), los=[1, 0.5, 1],
                             deconv_pow=2)
    return tuple(int(s) for s in ga.start), cpu(ga.value), cpu(gb.value), tan


def compare_ranks(one, many, tol=1e-11):
    _, ga1, gb1, t1 = one
    scale = max(numpy.abs(ga1).max(), numpy.abs(gb1).max())
    start, ga, gb, t = many
    sel = tuple(slice(s, s + n) for s, n in zip(start, ga.shape))
    numpy.testing.assert_allclose(ga, ga1[sel], rtol=0, atol=tol * scale)
    numpy.testing.assert_allclose(gb, gb1[sel], rtol=0, atol=tol * scale)
    assert (t.modes == t1.modes).all() and (t.modes2d == t1.modes2d).all()
    pscale = numpy.nanmax(numpy.abs(t1.power))
    numpy.testing.assert_allclose(t.power, t1.power, rtol=0, atol=tol * pscale, equal_nan=True)
    numpy.testing.assert_allclose(t.power2d, t1.power2d, rtol=0, atol=tol * pscale, equal_nan=True)
    for ell in t1.poles:
        numpy.testing.assert_allclose(t.poles[ell], t1.poles[ell], rtol=0, atol=tol * (2 * ell + 1) * pscale,
                                      equal_nan=True)


def _thread_ranks(size, np_, Nmesh):
    from tests import thread_comm
    one = ranks_case(Nmesh=Nmesh)
    results = {}

    def body(comm):
        results[comm.rank] = ranks_case(comm, np_, Nmesh)
    thread_comm.run_ranks(size, body)
    assert sum(r[1].size for r in results.values()) == one[1].size
    for r in results.values():
        compare_ranks(one, r)


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
def test_ranks_equal_one(gbe, size, np_):
    """every rank's block of the gradients is the one-rank block (the counts are the global ones), every rank's
    tangent the one-rank tangent"""
    _thread_ranks(size, np_, [16, 16, 12])


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(4, [4]), (8, [8]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _thread_ranks(size, np_, [64, 64, 48])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize('nproc', [2, 4])
def test_gloo_ranks_equal_one(nproc):
    """the same, and Tabulated.apply_vjp / apply_jvp, with one process per rank over gloo (tests/grad_mp_cases.py)"""
    env = dict(os.environ)
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=%d' % nproc,
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tests', 'grad_mp_cases.py')]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + '\n' + out.stderr[-6000:]
    assert 'ok power gradients on %d ranks' % nproc in out.stdout
    assert 'ok tabulated gradients on %d ranks' % nproc in out.stdout


# ---- the whole chain (both backends) -------------------------------------------------------------------------------

def chain_backend():
    """the CPU double that serves every entry of the chain: the LPT kernels and their gradients, the tabulated
    transfer and its gradients, the power spectrum and its adjoint"""
    from tests.test_lpt_gradients import GradOracleBackend
    from tests.test_tabulated_gradients import TableGradOracleBackend

    class ChainOracleBackend(PowerGradOracleBackend, TableGradOracleBackend, GradOracleBackend):
        name = 'oracle-chain'
    return ChainOracleBackend()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def cbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(chain_backend())
    yield b
    backend.reset()


def test_whole_chain(cbe):
    """white noise -> apply(Tabulated(k, sqrt(P / V))) -> lpt -> x = q + dx1 + dx2 -> paint -> r2c -> power_spectrum
    with poles (0, 2) -> chi^2 against a fixed target: d chi^2 / d t_i through power_spectrum_vjp -> r2c_vjp ->
    paint_vjp -> lpt_vjp -> apply_vjp against central differences of the forward (the tolerance of
    test_lpt_gradients.test_callers_chain)"""
    from pmesh_amd.lpt import lpt, lpt_vjp
    from pmesh_amd.transfer import Tabulated
    from tests.test_lpt import table
    from tests.test_lpt_gradients import nyquist_zero
    N, L = 32, 200.
    pm = ParticleMesh([N] * 3, BoxSize=L, resampler='tsc')
    kt, pk = table(n=24, kmin=1e-2, kmax=5.0)
    t0 = numpy.sqrt(pk / L ** 3)
    w = nyquist_zero(pm.generate_whitenoise(5, unitary=True))
    q = pm.generate_uniform_particle_grid(shift=0.5)
    kf = 2 * numpy.pi / L
    e = numpy.arange(0.5, 14.0, 1.5) * kf
    poles = (0, 2)
    target = {0: 1.3 * (e[:-1] / kf) ** -1.0, 2: 0.1 * numpy.ones(len(e) - 1)}

    def forward(t):
        tab = Tabulated(kt, t, loglog=True)
        delta = w.apply(tab)
        dx1, dx2 = lpt(delta, q)
        x = q + dx1 + dx2
        c = pm.paint(x).r2c()
        return tab, delta, x, c, power_spectrum(c, e, poles=poles)

    def chi2(res):
        return float(sum(((res.poles[ell].real - target[ell]) ** 2).sum() for ell in poles))

    tab, delta, x, c, res = forward(t0)
    assert (res.modes > 0).all()
    v = {ell: 2 * (res.poles[ell].real - target[ell]) for ell in poles}
    grad_c = power_spectrum_vjp(c, e, v_poles=v, poles=poles, result=res)
    grad_rho = grad_c.r2c_vjp()
    grad_x, _ = pm.paint_vjp(grad_rho, x, out_mass=False)
    grad_d, _ = lpt_vjp(delta, q, grad_x, grad_x)
    _, grad_t = tab.apply_vjp(w, grad_d)
    assert grad_t.shape == t0.shape
    scale = numpy.abs(grad_t * t0).max()
    for i in (5, 9, 14, 16):
        dt = 1e-4 * t0[i]
        tp, tm = t0.copy(), t0.copy()
        tp[i] += dt
        tm[i] -= dt
        ng = (chi2(forward(tp)[-1]) - chi2(forward(tm)[-1])) / (2 * dt)
        numpy.testing.assert_allclose(ng * t0[i], grad_t[i] * t0[i], rtol=1e-4, atol=1e-6 * scale)


# ---- 512^3 (GPU) ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_power_vjp_512_memory(hipbe):
    """one vjp with mu bins and poles at 512^3 f8: finite, non-zero, and no more memory than the output and one more
    field over the inputs (the kernel allocates nothing: the only other allocations are the bin tables)"""
    N = 512
    pm = ParticleMesh([N] * 3, BoxSize=1000.)
    a = pm.generate_whitenoise(1, unitary=False, type='complex')
    e = kf_edges(pm)
    me = numpy.linspace(-1, 1, 11)
    v = cotangents(len(e) - 1, len(me) - 1, (0, 2, 4), 40)
    torch.cuda.synchronize()
    field = a._base.storage.numel() * a._base.storage.element_size()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g = power_spectrum_vjp(a, e, muedges=me, poles=(0, 2, 4), **v)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / field
    print('power_spectrum_vjp 512^3 f8: peak %.3f field sizes over the inputs' % peak)
    assert torch.isfinite(torch.view_as_real(g.value)).all() and float(g.value.abs().max()) > 0
    assert peak <= 2.0, peak


# ---- resources (compiles for gfx950 on the CPU) --------------------------------------------------------------------

def test_power_gradient_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_power_grad.hip')
    kernels = {k: v for k, v in t.items() if 'power_vjp_kernel' in k}
    assert len(kernels) == 8, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)      # four waves per SIMD
        assert r['Occupancy'] >= 4, (name, r)    # with the (k, mu) table and the multipoles as well
