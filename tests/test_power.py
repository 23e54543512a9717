"""pmesh_amd.power: the binned power spectrum (csrc/pmx_power.hip) against a numpy restatement of its semantics.

The restatement (oracle_sums below) builds |k| from the wavenumbers of an f8 ParticleMesh (pm._block_coords, what
ComplexField.x returns there), mu, the Hermitian weights with the conjugate at -mu, numpy.digitize and Legendre
polynomials from numpy.polynomial.legendre, and returns the accumulator vector in the layout of pmx_power_project.
Under -m "not gpu" it also serves the entry (PowerOracleBackend), so the host layer — argument handling, RealField
input, layouts, the sum over ranks before the division — runs without a GPU; under -m gpu the kernel is compared with
it.
"""
import numpy
import pytest
import torch
from numpy.polynomial import legendre

from pmesh_amd import _abi, backend
from pmesh_amd import pm as _pm
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.power import PowerResult, power_spectrum
from pmesh_amd.transfer import Transfer
from tests.oracle_backend import OracleBackend


def _sinc_pow(w, p):
    x = 0.5 * w
    small = numpy.abs(x) < 1e-5
    xs = numpy.where(small, 1.0, x)
    s = numpy.where(small, 1.0 - x * x / 6. + x * x * x * x / 120., numpy.sin(xs) / xs)
    sp = s
    for _ in range(1, p):
        sp = sp * s
    return sp


def oracle_sums(a, b, k, idx, nmesh, volume, kedges, muedges=None, los=None, ells=(), deconv_pow=0, hermitian=False):
    """numpy restatement of pmx_power_project on one block: a, b complex arrays of the block (b None: a), k / idx the
    per-axis wavenumbers and global indices of the block (broadcastable); returns the float64 accumulator vector"""
    a = numpy.asarray(a).astype('c16')
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
    # a conj(b) component by component (numpy's complex product may fuse and leave rounding in Im(a conj(a)))
    vr = volume * (a.real * b.real + a.imag * b.imag)
    vi = volume * (a.imag * b.real - a.real * b.imag)
    if deconv_pow:
        for d in range(ndim):
            n = int(nmesh[d])
            s = idx[d] - n * (idx[d] >= n // 2)
            sp = _sinc_pow(s.astype('f8') * (2 * numpy.pi / n), deconv_pow)
            vr, vi = vr / sp, vi / sp
    vr, vi = numpy.broadcast_to(vr, a.shape), numpy.broadcast_to(vi, a.shape)
    h = numpy.zeros(a.shape, dtype=bool)
    if hermitian:
        il = idx[-1]
        h = numpy.broadcast_to((il != 0) & (il != int(nmesh[-1]) // 2), a.shape)
    kb = numpy.digitize(kmag, kedges) - 1
    ok = (kb >= 0) & (kb < nk)
    kb, kmag, mu, vr, vi, h = kb[ok], kmag[ok], mu[ok], vr[ok], vi[ok], h[ok]
    v = vr + 1j * vi
    s1 = 4 + 2 * len(ells)
    nmu = 0 if muedges is None else len(muedges) - 1
    acc = numpy.zeros(nk * s1 + nk * nmu * 5)
    t1 = acc[:nk * s1].reshape(nk, s1)

    def add(col, w):
        t1[:, col] += numpy.bincount(kb, weights=w, minlength=nk)
    one = numpy.ones_like(kmag)
    # the mode at mu with v, and (h) its conjugate at -mu with conj(v)
    add(0, one + h)
    add(1, kmag + h * kmag)
    add(2, v.real + h * v.real)
    add(3, v.imag - h * v.imag)
    for p, ell in enumerate(ells):
        c = [0] * ell + [1]
        z = v * legendre.legval(mu, c) + h * numpy.conj(v) * legendre.legval(-mu, c)
        add(4 + 2 * p, z.real)
        add(5 + 2 * p, z.imag)
    if nmu:
        me = numpy.asarray(muedges, dtype='f8')
        t2 = acc[nk * s1:].reshape(nk, nmu, 5)

        def cells(m, sel, vv):
            mb = numpy.digitize(m, me) - 1
            mb[m == me[-1]] = nmu - 1
            good = sel & (mb >= 0) & (mb < nmu)
            flat = kb[good] * nmu + mb[good]
            for col, w in enumerate((numpy.ones(good.sum()), kmag[good], m[good], vv.real[good], vv.imag[good])):
                t2[..., col] += numpy.bincount(flat, weights=w, minlength=nk * nmu).reshape(nk, nmu)
        cells(mu, numpy.ones_like(h), v)
        cells(-mu, h, numpy.conj(v))
    return acc


class PowerOracleBackend(OracleBackend):
    """the CPU test double with pmx_power_project served by oracle_sums"""
    name = 'oracle-power'

    def power_project(self, params, a, b, start, nmesh, boxsize, kedges, muedges, acc):
        if a.numel() == 0:
            return
        nd = a.dim()
        k, idx = _pm._block_coords(start, tuple(a.shape), nmesh, boxsize, 'f8', 'cpu', True)
        r = oracle_sums(a.numpy(), None if b is None else b.numpy(), [x.numpy() for x in k], [i.numpy() for i in idx],
                        nmesh, params.volume, kedges.numpy(), None if muedges is None else muedges.numpy(),
                        list(params.los)[:nd], list(params.poles)[:params.npoles], params.deconv_pow, params.hermitian)
        acc += torch.from_numpy(r)


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def pbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(PowerOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    """the product backend alone (the kernel tests below are GPU tests)"""
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def expected(field, kedges, other=None, muedges=None, los=None, poles=(), deconv_pow=0):
    """the oracle's PowerResult for a one-rank field: wavenumbers from the f8 mesh of the same geometry"""
    pm = field.pm
    pm8 = ParticleMesh(pm.Nmesh, BoxSize=pm.BoxSize, comm=pm.comm, np=pm.np,
                       dtype='c16' if not field.compressed else 'f8')
    f8 = pm8.create(type=type(field))
    k = [x.cpu().numpy() for x in f8.x]
    idx = [i.cpu().numpy() for i in f8.i]
    assert tuple(f8.value.shape) == tuple(field.value.shape)
    if los is not None:
        los = numpy.asarray(los, dtype='f8') / numpy.sqrt(numpy.sum(numpy.square(los)))
    acc = oracle_sums(field.value.cpu().numpy(), None if other is None else other.value.cpu().numpy(), k, idx,
                      pm.Nmesh, float(numpy.prod(pm.BoxSize)), kedges, muedges, los, list(poles), deconv_pow,
                      field.compressed)
    return PowerResult(numpy.asarray(kedges, dtype='f8'), None if muedges is None else numpy.asarray(muedges, 'f8'),
                       acc, list(poles))


RTOL = 1e-12          # of the scale of a column: the bound of every comparison of binned spectra with their restatement


def assert_same(got, want, rtol=RTOL):
    assert (got.modes == want.modes).all(), numpy.nonzero(got.modes != want.modes)

    def close(x, y, scale=None):
        if scale is None:
            scale = numpy.nanmax(numpy.abs(y)) if numpy.isfinite(y).any() else 1.0
        numpy.testing.assert_allclose(x, y, rtol=rtol, atol=rtol * scale, equal_nan=True)
    close(got.k, want.k)
    close(got.power, want.power)
    assert sorted(got.poles) == sorted(want.poles)
    pscale = numpy.nanmax(numpy.abs(want.power)) if numpy.isfinite(want.power).any() else 1.0
    for ell in want.poles:
        # (odd multipoles of an auto spectrum are sums that cancel: compared on the scale of the power)
        close(got.poles[ell], want.poles[ell], (2 * ell + 1) * pscale)
    if want.power2d is None:
        assert got.power2d is None
    else:
        assert (got.modes2d == want.modes2d).all()
        close(got.k2d, want.k2d)
        close(got.mu2d, want.mu2d)
        close(got.power2d, want.power2d)


def density(pm, seed=1, slope=-2.0):
    """a real field: white noise shaped by a power law, |k|^(slope/2), k = 0 mode zeroed"""
    c = pm.generate_whitenoise(seed, unitary=False, type='complex')

    def shape(k, v):
        k2 = sum(ki ** 2 for ki in k)
        k2[k2 == 0] = 1
        return v * k2 ** (slope / 4)
    c = c.apply(shape)
    return c.c2r()


def kf_edges(pm, nbins=None):
    kf = 2 * numpy.pi / float(numpy.max(pm.BoxSize))
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(pm.Nmesh, pm.BoxSize))) * 1.01
    return numpy.arange(0, kmax + kf, kf)


# ---- argument handling (any backend) ------------------------------------------------------------------------------

def test_bad_arguments(pbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    c = pm.create(type='complex')
    e = kf_edges(pm)
    for bad in ([1.0], [0.0, 0.0], [0.3, 0.1, 0.2], [0, numpy.nan], [[0, 1], [1, 2]]):
        with pytest.raises(ValueError, match='kedges'):
            power_spectrum(c, bad)
    with pytest.raises(ValueError, match='muedges'):
        power_spectrum(c, e, muedges=[-1.5, 0, 1])
    with pytest.raises(ValueError, match='muedges'):
        power_spectrum(c, e, muedges=[0, 0.5, 0.5, 1])
    with pytest.raises(ValueError, match='PMX_POWER_MAX_MUBINS'):
        power_spectrum(c, e, muedges=numpy.linspace(-1, 1, _abi.PMX_POWER_MAX_MUBINS + 2))
    with pytest.raises(ValueError, match='PMX_POWER_MAX_KBINS'):
        power_spectrum(c, numpy.arange(_abi.PMX_POWER_MAX_KBINS + 2, dtype='f8'))
    with pytest.raises(ValueError, match='PMX_POWER_MAX_POLES'):
        power_spectrum(c, e, poles=(0, 1, 2, 3, 4, 5))
    for bad in ((9,), (0, 0), (-1,)):
        with pytest.raises(ValueError, match='poles'):
            power_spectrum(c, e, poles=bad)
    with pytest.raises(ValueError, match='los'):
        power_spectrum(c, e, los=[0, 0, 0])
    with pytest.raises(ValueError, match='los'):
        power_spectrum(c, e, los=[0, 1])
    with pytest.raises(ValueError, match='deconv_pow'):
        power_spectrum(c, e, deconv_pow=-1)
    with pytest.raises(TypeError):
        power_spectrum(numpy.zeros((8, 8, 5), 'c16'), e)
    # mismatched fields: another mesh, another layout, another dtype
    other = ParticleMesh([8, 8, 16], BoxSize=100.).create(type='complex')
    with pytest.raises(ValueError, match='mesh|layout'):
        power_spectrum(c, e, other=other)
    with pytest.raises(ValueError, match='layout'):
        power_spectrum(c, e, other=pm.create(type=UntransposedComplexField))
    with pytest.raises(ValueError, match='layout'):
        power_spectrum(c, e, other=ParticleMesh([8, 8, 8], BoxSize=100., dtype='f4').create(type='complex'))


def test_more_than_three_dimensions(pbe):
    pm = ParticleMesh([4, 4, 4, 4], BoxSize=1.)
    with pytest.raises(NotImplementedError):
        power_spectrum(pm.create(type='complex'), [0, 1, 2])


def test_realfield_input_is_left_alone(pbe):
    pm = ParticleMesh([16, 16, 16], BoxSize=50.)
    r = density(pm)
    before = r.value.clone()
    e = kf_edges(pm)
    got = power_spectrum(r, e, poles=(0, 2))
    assert torch.equal(r.value, before)
    assert_same(got, expected(r.r2c(), e, poles=(0, 2)))


@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
def test_layouts_match_the_oracle(pbe, kind):
    pm = ParticleMesh([16, 12, 10], BoxSize=[40., 30., 50.], dtype='c16' if kind == 'c2c' else 'f8')
    if kind == 'c2c':
        r = pm.create(type='real')
        rng = numpy.random.RandomState(3)
        r.value[...] = torch.from_numpy(rng.normal(size=r.value.shape) + 1j * rng.normal(size=r.value.shape))
        c = r.r2c()
    else:
        c = density(pm).r2c(out=pm.create(type=TransposedComplexField if kind == 'T' else UntransposedComplexField))
    e = kf_edges(pm)
    me = numpy.linspace(-1, 1, 5)
    got = power_spectrum(c, e, muedges=me, poles=(0, 1, 2, 4), los=[1, 1, 0], deconv_pow=2)
    assert_same(got, expected(c, e, muedges=me, poles=(0, 1, 2, 4), los=[1, 1, 0], deconv_pow=2))


def _ranks_equal_one(pbe, size, np_, Nmesh):
    from tests import thread_comm
    e = None
    results = {}

    def body(comm):
        pm = ParticleMesh(Nmesh, BoxSize=100., comm=comm, np=np_)
        c = density(pm, seed=5).r2c()
        kedges = kf_edges(pm)
        results[comm.rank] = power_spectrum(c, kedges, muedges=numpy.linspace(0, 1, 4), poles=(0, 2))
    thread_comm.run_ranks(size, body)
    pm1 = ParticleMesh(Nmesh, BoxSize=100.)
    c1 = density(pm1, seed=5).r2c()
    e = kf_edges(pm1)
    one = power_spectrum(c1, e, muedges=numpy.linspace(0, 1, 4), poles=(0, 2))
    for r in range(size):
        assert_same(results[r], one, rtol=1e-11)


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [4]), (4, [2, 2])])
def test_ranks_sum_then_divide(pbe, size, np_):
    """every rank gets the one-rank result: raw sums over the ranks first, then the division"""
    _ranks_equal_one(pbe, size, np_, [16, 16, 12])


# ---- the kernel against the oracle ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('Nmesh,BoxSize', [([16, 16, 16], 100.), ([64, 64, 64], 500.), ([96, 96, 96], 300.),
                                           ([45, 45, 45], 100.), ([32, 48, 64], [100., 120., 200.]),
                                           ([64, 48], [100., 70.]), ([33, 40], 10.)])
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernel_uniform_edges(hipbe, Nmesh, BoxSize, dtype):
    """kedges = arange(0, kmax, k_f): many modes sit exactly on edges, counts must match exactly"""
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=dtype)
    c = density(pm).r2c()
    e = kf_edges(pm)
    assert_same(power_spectrum(c, e), expected(c, e))
    assert_same(power_spectrum(c, e, poles=(0, 2, 4)), expected(c, e, poles=(0, 2, 4)))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernel_layouts_mu_poles_cross(hipbe, kind, dtype):
    cdt = {'f8': 'c16', 'f4': 'c8'}[dtype]
    pm = ParticleMesh([48, 32, 40], BoxSize=[200., 150., 180.], dtype=cdt if kind == 'c2c' else dtype)
    T = UntransposedComplexField if kind == 'U' else TransposedComplexField
    if kind == 'c2c':
        rng = numpy.random.RandomState(7)
        r = pm.create(type='real')
        r.value[...] = torch.from_numpy(rng.normal(size=r.value.shape) + 1j * rng.normal(size=r.value.shape))
        r2 = pm.create(type='real')
        r2.value[...] = r.value * 0.5 + torch.from_numpy(rng.normal(size=r.value.shape)).to(r.value.device)
    else:
        r, r2 = density(pm, seed=2), density(pm, seed=3)
    a = r.r2c(out=pm.create(type=T))
    b = r2.r2c(out=pm.create(type=T))
    # non-uniform edges
    e = numpy.concatenate([[0.0], numpy.geomspace(0.01, 0.6, 30)])
    me = numpy.array([-1, -0.7, -0.2, 0, 0.1, 0.5, 0.9, 1.0])
    for other, poles in ((None, (0, 2, 4)), (b, (0, 1, 2, 4))):
        got = power_spectrum(a, e, other=other, muedges=me, poles=poles)
        assert_same(got, expected(a, e, other=other, muedges=me, poles=poles))
    got = power_spectrum(a, e, muedges=me, los=[0.3, -1, 2], poles=(3, 8), deconv_pow=2)
    assert_same(got, expected(a, e, muedges=me, los=[0.3, -1, 2], poles=(3, 8), deconv_pow=2))


@pytest.mark.gpu
def test_kernel_fine_edges_take_several_windows(hipbe):
    """k bins far narrower than a tile's |k| range: the tile is read once per window of bins"""
    pm = ParticleMesh([64, 64, 64], BoxSize=100.)
    c = density(pm).r2c()
    e = numpy.linspace(0, 3.5, 20001)
    me = numpy.linspace(-1, 1, 11)
    assert_same(power_spectrum(c, e), expected(c, e))
    assert_same(power_spectrum(c, e[::8], muedges=me, poles=(0, 2, 4)), expected(c, e[::8], muedges=me, poles=(0, 2, 4)))


@pytest.mark.gpu
@pytest.mark.parametrize('Nmesh', [[32, 32, 32], [32, 24], [64]])
def test_invariants(hipbe, Nmesh):
    pm = ParticleMesh(Nmesh, BoxSize=80.)
    r = density(pm, seed=9)
    c = r.r2c()
    V = float(numpy.prod(pm.BoxSize))
    e = numpy.array([0.0] + list(kf_edges(pm)[1:]))
    me = numpy.linspace(-1, 1, 7)
    res = power_spectrum(c, e, muedges=me, poles=(0, 2))
    # edges covering every mode: all prod(N) modes counted, the weighted power is V cnorm
    assert res.modes.sum() == numpy.prod(Nmesh)
    tot = numpy.nansum(res.modes * res.power.real) / V
    assert abs(tot - c.cnorm()) <= 1e-12 * c.cnorm()
    # the (k, mu) table summed over mu is the k table
    assert (res.modes2d.sum(axis=1) == res.modes).all()
    w2 = numpy.nansum(res.modes2d * res.power2d, axis=1)
    numpy.testing.assert_allclose(w2, numpy.nan_to_num(res.modes * res.power), rtol=1e-12,
                                  atol=1e-12 * numpy.nanmax(numpy.abs(res.power)) * res.modes.max())
    # auto == cross with itself; P_0 == P
    cross = power_spectrum(c, e, other=c, muedges=me, poles=(0, 2))
    assert_same(cross, res)
    numpy.testing.assert_allclose(res.poles[0], res.power, rtol=1e-12, equal_nan=True)
    # deconv_pow = 2p equals measuring the field compensated by p
    d = power_spectrum(c, e, deconv_pow=4)
    d2 = power_spectrum(c.apply(Transfer(deconv_pow=2)), e)
    assert (d.modes == d2.modes).all()
    numpy.testing.assert_allclose(d.power, d2.power, rtol=1e-12, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (8, [8]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _ranks_equal_one(hipbe, size, np_, [64, 64, 48])


@pytest.mark.gpu
def test_kernel_512(hipbe):
    """a 512^3 f8 field against the oracle, with exact counts"""
    pm = ParticleMesh([512, 512, 512], BoxSize=1000.)
    c = density(pm, seed=11).r2c()
    e = kf_edges(pm)
    got = power_spectrum(c, e, poles=(0, 2, 4))
    assert_same(got, expected(c, e, poles=(0, 2, 4)))
    assert got.modes.sum() == 512 ** 3


# ---- resources (compiles for gfx950 on the CPU) --------------------------------------------------------------------

def test_power_kernels_compile_without_scratch():
    import os
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_power.hip')
    kernels = {k: v for k, v in t.items() if 'power_kernel' in k}
    assert len(kernels) == 8, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 168, (name, r)      # three or more waves per SIMD
        # power_kernel<T, MU, POLES>: four waves per SIMD without the (k, mu) table and the multipoles, three with either
        assert r['Occupancy'] >= (4 if 'Lb0ELb0E' in name else 3), (name, r)
