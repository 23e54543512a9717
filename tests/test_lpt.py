"""pmesh_amd.lpt and transfer.Tabulated (csrc/pmx_lpt.hip) against a numpy restatement of their conventions.

The restatement builds the wavenumbers of a block from pm._block_coords (what ComplexField.x returns on an f8 mesh),
the tabulated transfer from numpy.interp, the Hessian factors k_i k_j / k^2, the source S and the whole 1LPT / 2LPT
chain from numpy.fft.rfftn / irfftn (r2c normalised by 1 / prod(N), c2r not).  Under -m "not gpu" it also serves the
three entries of the C ABI (LptOracleBackend), so the host layer runs without a GPU; under -m gpu the kernels are
compared with it.
"""
import ctypes as C

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd import pm as _pm
from pmesh_amd.lpt import lpt, lpt1, lpt2source
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.transfer import Tabulated, Transfer
from tests.oracle_backend import OracleBackend


# ---- the restatement -----------------------------------------------------------------------------------------------

def block_k(start, shape, nmesh, boxsize):
    k, _ = _pm._block_coords(list(start), tuple(shape), list(nmesh), list(boxsize), 'f8', 'cpu', True)
    return [x.numpy() for x in k]


def k_squared(k):
    k2 = 0
    for kd in k:
        k2 = k2 + kd * kd
    return k2


def interp_xy(kmag, x, y, loglog, kmin, kmax, left, right):
    """interp(|k|) of include/pmesh_amd.h (pmx_ktable): numpy.interp on (x, y) = (k, t) or (ln k, ln t)"""
    kmag = numpy.asarray(kmag, dtype='f8')
    if not loglog:
        return numpy.interp(kmag, x, y, left=left, right=right)
    inside = (kmag >= kmin) & (kmag <= kmax)
    u = numpy.log(numpy.where(inside, kmag, kmin))
    return numpy.where(inside, numpy.exp(numpy.interp(u, x, y)), numpy.where(kmag < kmin, left, right))


def ref_factor(k, t, kmag, loglog=False, amplitude=1.0, left=0.0, right=0.0):
    """amplitude * interp(|k|) of the issue's conventions, from the table as the caller gives it"""
    k, t = numpy.asarray(k, 'f8'), numpy.asarray(t, 'f8')
    x, y = (numpy.log(k), numpy.log(t)) if loglog else (k, t)
    return amplitude * interp_xy(kmag, x, y, loglog, k[0], k[-1], left, right)


def scaled(f, v):
    """f * v component by component, in double"""
    v = numpy.asarray(v).astype('c16')
    return f * v.real + 1j * (f * v.imag)


def hessian_factor(k, i, j):
    k2 = k_squared(k)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        return numpy.where(k2 == 0, 0.0, (k[i] * k[j]) / numpy.where(k2 == 0, 1.0, k2))


def source(phi, scale):
    """scale * S from the diagonal then off-diagonal components, in the order of operations of pmx_lpt2_source"""
    phi = [numpy.asarray(p, dtype='f8') for p in phi]
    if len(phi) == 3:
        s = phi[0] * phi[1] - phi[2] * phi[2]
    else:
        p00, p11, p22, p01, p02, p12 = phi
        s = p00 * p11 + p11 * p22
        s = s + p22 * p00
        s = s - p01 * p01
        s = s - p02 * p02
        s = s - p12 * p12
    return scale * s


def c2r(c, nmesh):
    return numpy.fft.irfftn(c, s=tuple(nmesh), axes=tuple(range(len(nmesh)))) * float(numpy.prod(nmesh))


def r2c(x):
    return numpy.fft.rfftn(x) / float(numpy.prod(x.shape))


def ref_lpt_fields(delta, nmesh, boxsize):
    """the mesh fields (dx1 components, dx2 components) of the conventions for the full r2c spectrum delta"""
    nd = len(nmesh)
    shape = delta.shape
    k = block_k([0] * nd, shape, nmesh, boxsize)
    k2 = k_squared(k)
    inv = numpy.where(k2 == 0, 0.0, 1.0 / numpy.where(k2 == 0, 1.0, k2))

    def grad(c, d):
        return c2r(1j * (k[d] * inv) * c, nmesh)
    dx1 = [grad(delta, d) for d in range(nd)]
    pairs = [(d, d) for d in range(nd)] + [(i, j) for i in range(nd) for j in range(i + 1, nd)]
    phi = [c2r(scaled(hessian_factor(k, i, j), delta), nmesh) for i, j in pairs]
    src = r2c(source(phi, 3.0 / 7.0))
    dx2 = [grad(src, d) for d in range(nd)]
    return dx1, dx2, src


# ---- the C ABI served by the restatement (CPU) ---------------------------------------------------------------------

def _host_doubles(addr, n):
    return numpy.ctypeslib.as_array((C.c_double * n).from_address(addr)).copy()


class LptOracleBackend(OracleBackend):
    """the CPU test double with pmx_apply_ktable, pmx_lpt_hessian and pmx_lpt2_source served by the restatement"""
    name = 'oracle-lpt'

    def apply_ktable(self, table, v, out, start, nmesh, boxsize):
        x, y = _host_doubles(table.x, table.n), _host_doubles(table.y, table.n)
        k = block_k(start, v.shape, nmesh, boxsize)
        f = table.amplitude * interp_xy(numpy.sqrt(k_squared(k)), x, y, table.loglog, table.kmin, table.kmax,
                                        table.left, table.right)
        out.copy_(torch.from_numpy(scaled(f, v.numpy())))

    def lpt_hessian(self, v, pairs, outs, start, nmesh, boxsize):
        k = block_k(start, v.shape, nmesh, boxsize)
        vals = v.numpy().copy()
        for (i, j), o in zip(pairs, outs):
            o.copy_(torch.from_numpy(scaled(hessian_factor(k, i, j), vals)))

    def lpt2_source(self, ins, out, scale):
        out.copy_(torch.from_numpy(source([a.numpy() for a in ins], scale)))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def lbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(LptOracleBackend())
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


def close(got, want, tol):
    got, want = numpy.asarray(got), numpy.asarray(want)
    scale = numpy.abs(want).max() if want.size else 1.0
    numpy.testing.assert_allclose(got, want, rtol=0, atol=tol * max(scale, 1e-300))


def table(n=200, kmin=1e-3, kmax=20.0):
    """a smooth positive P(k)-like table, log-spaced"""
    k = numpy.geomspace(kmin, kmax, n)
    p = 2e4 * k / (1 + (k / 0.02) ** 2) ** 1.4
    return k, p


def delta_spectrum(pm, seed=1, zero_nyquist=True):
    """the r2c spectrum of a random real field of an f8 mesh, its Nyquist planes zeroed (the odd factors make them
    non-Hermitian, and c2r's treatment of those modes is no part of these conventions)"""
    rng = numpy.random.RandomState(seed)
    r = pm.create(type='real')
    r.value[...] = torch.from_numpy(rng.normal(size=tuple(r.value.shape))).to(r.value.device)
    c = r.r2c()
    if zero_nyquist:
        v = c.value
        for d, n in enumerate(pm.Nmesh):
            n = int(n)
            if n % 2:
                continue
            sel = [slice(None)] * len(pm.Nmesh)
            i = c.i[d].reshape(-1)
            hit = (i == n // 2).nonzero()
            if len(hit):
                sel[d] = int(hit[0])
                v[tuple(sel)] = 0
    return c


def full_spectrum(c):
    """the one-rank spectrum of c in logical (N0, N1, N2 // 2 + 1) order as numpy complex128"""
    return cpu(c.value).astype('c16')


# ---- argument checking (both backends) -----------------------------------------------------------------------------

def test_tabulated_arguments(lbe):
    k, t = table()
    for bad_k, bad_t in (([1.0], [1.0]), (k[::-1], t), (numpy.r_[k[:5], k[4:]], numpy.r_[t[:5], t[4:]]),
                         (k, t[:-1]), (numpy.r_[k[:-1], numpy.nan], t), (k, numpy.r_[t[:-1], numpy.inf]),
                         (numpy.linspace(0, 1, _abi.PMX_KTABLE_MAX + 1), numpy.ones(_abi.PMX_KTABLE_MAX + 1)),
                         ([[0, 1], [1, 2]], [[0, 1], [1, 2]])):
        with pytest.raises(ValueError):
            Tabulated(bad_k, bad_t)
    with pytest.raises(ValueError, match='positive'):
        Tabulated(numpy.r_[0.0, k], numpy.r_[1.0, t], loglog=True)
    with pytest.raises(ValueError, match='positive'):
        Tabulated(k, -t, loglog=True)
    with pytest.raises(ValueError):
        Tabulated(k, t, left=numpy.nan)
    Tabulated(numpy.linspace(0, 1, _abi.PMX_KTABLE_MAX), numpy.ones(_abi.PMX_KTABLE_MAX))   # the limit itself
    assert not Tabulated(k, t).fusable()
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    with pytest.raises(TypeError):
        pm.create(type='real').apply(Tabulated(k, t), kind='relative')


def test_lpt_arguments(lbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    c = pm.create(type='complex')
    q = pm.generate_uniform_particle_grid(shift=0)
    with pytest.raises(ValueError, match='q'):
        lpt(c, q[:, :2])
    with pytest.raises(ValueError, match='q'):
        lpt1(c, q[:, 0])
    with pytest.raises(ValueError, match='order'):
        lpt(c, q, order=3)
    with pytest.raises(TypeError):
        lpt(pm.create(type='real'), q)
    with pytest.raises(TypeError):
        lpt2source(numpy.zeros((8, 8, 5), 'c16'))
    pm1 = ParticleMesh([16], BoxSize=10.)
    c1 = pm1.create(type='complex')
    q1 = pm1.generate_uniform_particle_grid(shift=0)
    with pytest.raises(ValueError):
        lpt2source(c1)
    with pytest.raises(ValueError):
        lpt(c1, q1, order=2)
    assert lpt(c1, q1, order=1)[1] is None        # first order is defined in 1-d
    pm4 = ParticleMesh([4, 4, 4, 4], BoxSize=1.)
    with pytest.raises(NotImplementedError):
        lpt2source(pm4.create(type='complex'))
    pmc = ParticleMesh([8, 8, 8], BoxSize=100., dtype='c16')
    with pytest.raises(ValueError, match='real mesh'):
        lpt2source(pmc.create(type='complex'))


# ---- the tabulated transfer (both backends) ------------------------------------------------------------------------

@pytest.mark.parametrize('loglog', [False, True])
def test_tabulated_call_equals_apply(lbe, loglog):
    pm = ParticleMesh([16, 12, 10], BoxSize=[40., 30., 50.])
    c = delta_spectrum(pm, seed=2, zero_nyquist=False)
    k, t = table(kmin=0.2, kmax=1.5)      # |k| spans 0 .. 1.9: left, inside and right of the table
    tab = Tabulated(k, t, loglog=loglog, amplitude=0.7, left=0.25, right=-3.0)
    got = cpu(c.apply(tab).value)
    called = cpu(tab(c.x, c.value))
    close(got, called, 1e-12)
    kk = block_k(c.start, c.value.shape, pm.Nmesh, pm.BoxSize)
    want = scaled(ref_factor(k, t, numpy.sqrt(k_squared(kk)), loglog, 0.7, 0.25, -3.0), full_spectrum(c))
    close(got, want, 1e-12)
    # c2r(transfer=Tabulated) is apply + c2r
    close(cpu(c.c2r(transfer=tab).value), cpu(c.apply(tab).c2r().value), 1e-12)


# ---- lpt against the restatement (both backends) -------------------------------------------------------------------

@pytest.mark.parametrize('Nmesh,BoxSize', [([16, 16, 16], 100.), ([24, 16, 20], [120., 80., 100.]), ([32, 32], 50.)])
def test_lpt_matches_restatement(lbe, Nmesh, BoxSize):
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, resampler='cic')
    c = delta_spectrum(pm, seed=4)
    before = c.value.clone()
    q = pm.generate_uniform_particle_grid(shift=0)    # on the nodes: CIC reads the node values
    dx1, dx2 = lpt(c, q, order=2)
    assert torch.equal(c.value, before)
    assert tuple(dx1.shape) == (len(q), len(Nmesh)) and tuple(dx2.shape) == (len(q), len(Nmesh))
    r1, r2, src = ref_lpt_fields(full_spectrum(c), Nmesh, pm.BoxSize)
    for d in range(len(Nmesh)):
        close(cpu(dx1[:, d]), r1[d].reshape(-1), 1e-12)
        close(cpu(dx2[:, d]), r2[d].reshape(-1), 1e-12)
    close(cpu(lpt1(c, q)), numpy.stack([r.reshape(-1) for r in r1], axis=1), 1e-12)
    close(full_spectrum(lpt2source(c)), src, 1e-12)
    a, b = lpt(c, q, order=1)
    assert b is None
    close(cpu(a), cpu(dx1), 1e-14)


def _ranks_equal_one(Nmesh, size, np_, tol):
    from tests import thread_comm
    k, t = table()
    V = float(numpy.prod(numpy.broadcast_to(100., len(Nmesh))))
    tab = Tabulated(k, numpy.sqrt(t / V), loglog=True)

    def make(comm=None):
        kw = {} if comm is None else dict(comm=comm, np=np_)
        pm = ParticleMesh(Nmesh, BoxSize=100., resampler='cic', **kw)
        c = pm.generate_whitenoise(7, unitary=False).apply(tab)
        q = pm.generate_uniform_particle_grid(shift=0)
        dx1, dx2 = lpt(c, q)
        idx = numpy.rint(cpu(q) / 100. * numpy.asarray(Nmesh)).astype('i8') % numpy.asarray(Nmesh)
        return numpy.ravel_multi_index(tuple(idx.T), Nmesh), cpu(dx1), cpu(dx2)
    flat1, one1, one2 = make()
    order = numpy.argsort(flat1)
    results = {}

    def body(comm):
        results[comm.rank] = make(comm)
    thread_comm.run_ranks(size, body)
    assert sum(len(r[0]) for r in results.values()) == numpy.prod(Nmesh)
    for flat, d1, d2 in results.values():
        rows = order[numpy.searchsorted(flat1[order], flat)]
        close(d1, one1[rows], tol)
        close(d2, one2[rows], tol)


@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (4, [2, 2])])
def test_ranks_equal_one(lbe, size, np_):
    _ranks_equal_one([16, 16, 16], size, np_, 1e-11)


# ---- the kernels against the restatement (GPU) ---------------------------------------------------------------------

def _block(shape, dtype, form, rng, complex_=True):
    """a block of the given logical shape as a tensor on the device: contiguous ('C'), axes 0 / 1 swapped in memory
    ('T', the transposed layout), padded along the last axis ('pad') or every other element of a larger array
    ('strided'); a 1-d block has no axes to swap, its 'T' is 'C'"""
    dev = backend.get().device
    if form == 'T' and len(shape) == 1:
        form = 'C'
    if form == 'T':
        big = (shape[1], shape[0]) + tuple(shape[2:])
    elif form == 'pad':
        big = tuple(shape[:-1]) + (shape[-1] + 3,)
    elif form == 'strided':
        big = tuple(2 * s for s in shape)
    else:
        big = tuple(shape)
    vals = rng.normal(size=big) + (1j * rng.normal(size=big) if complex_ else 0)
    t = torch.from_numpy(vals.astype(dtype)).to(dev)
    if form == 'T':
        return t.transpose(0, 1)
    if form == 'pad':
        return t[..., :shape[-1]]
    if form == 'strided':
        return t[tuple(slice(None, None, 2) for _ in shape)]
    return t


FORMS = ['C', 'T', 'pad', 'strided']
# The streaming kernels launch min(rows, WRAP) workgroups along the slowest memory axis and walk it in steps of that
# many: in a block with more rows a workgroup makes a second trip.  Tall blocks (a 1-d mesh of 2^17 points, a tall 2-d
# block) reach it; under form 'T' the long axis is the slow one in memory only for the second of them.
WRAP = 65535
TALL = [([65541, 3], [1000, 0], [131072, 4]),
        ([3, 65541], [0, 1000], [4, 131072]),
        ([65541, 2, 3], [1000, 0, 0], [131072, 2, 4])]
TALL_1D = [([65541], [1000], [131072])]                   # for the kernels that take ndim == 1
GEOMS = [([16, 16, 9], [0, 0, 0], [16, 16, 16]),          # an r2c half spectrum
         ([45, 15, 45], [0, 0, 0], [45, 45, 45]),         # odd, a block of a c2c spectrum
         ([12, 48, 25], [36, 0, 0], [48, 48, 48]),        # 3 * 2^k, a slab starting at 36
         ([24, 17], [0, 0], [24, 32])] + TALL + TALL_1D   # 2-d; then more rows than WRAP


def _nan_block(shape, dtype, form, rng, complex_=True):
    """a _block filled with NaN: an output in which an element the kernel never writes cannot pass"""
    t = _block(shape, dtype, form, rng, complex_)
    return t.fill_(complex(float('nan'), float('nan')) if complex_ else float('nan'))


def close_rows(got, want, tol):
    """close on the whole block, then on the rows from WRAP on of an axis that long, on their own scale"""
    close(got, want, tol)
    got, want = numpy.asarray(got), numpy.asarray(want)
    for d, n in enumerate(want.shape):
        if n > WRAP:
            sel = (slice(None),) * d + (slice(WRAP, None),)
            assert numpy.isfinite(got[sel]).all()
            close(got[sel], want[sel], tol)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt,tol', [('c16', 1e-12), ('c8', 1e-5)])
@pytest.mark.parametrize('loglog', [False, True])
def test_ktable_kernel(hipbe, form, cdt, tol, loglog):
    rng = numpy.random.RandomState(5)
    # log-spaced (uniform in log k: the guessed search for loglog) and linear (uniform in k: guessed for linear)
    tables = [table(n=777, kmin=0.05, kmax=1.2), (numpy.linspace(0.05, 1.2, 333), table(n=333, kmin=0.05, kmax=1.2)[1])]
    for (shape, start, nmesh), (k, t) in [(g, tb) for g in GEOMS for tb in tables]:
        box = [100.] * len(nmesh)
        tab = Tabulated(k, t, loglog=loglog, amplitude=1.5, left=0.5, right=2.0)
        v = _block(shape, cdt, form, rng)
        kk = block_k(start, shape, nmesh, box)
        want = scaled(ref_factor(k, t, numpy.sqrt(k_squared(kk)), loglog, 1.5, 0.5, 2.0), cpu(v))
        out = _nan_block(shape, cdt, 'pad' if form != 'pad' else 'C', rng)
        x, y, s = tab._table(hipbe.device)
        hipbe.apply_ktable(s, v, out, start, nmesh, box)
        close_rows(cpu(out), want, tol)
        hipbe.apply_ktable(s, v, v, start, nmesh, box)           # in place
        close_rows(cpu(v), want, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt,tol', [('c16', 1e-12), ('c8', 1e-5)])
def test_hessian_kernel(hipbe, form, cdt, tol):
    rng = numpy.random.RandomState(6)
    for shape, start, nmesh in GEOMS:
        nd = len(nmesh)
        box = [100., 80., 120.][:nd]
        pairs = [(i, j) for i in range(nd) for j in range(i, nd)]
        kk = block_k(start, shape, nmesh, box)
        for group in (pairs[:1], pairs[:2], pairs[-3:]):
            v = _block(shape, cdt, form, rng)
            want = [scaled(hessian_factor(kk, i, j), cpu(v)) for i, j in group]
            outs = [_nan_block(shape, cdt, f, rng) for f in ('C', 'pad', 'T')[:len(group)]]
            hipbe.lpt_hessian(v, group, outs, start, nmesh, box)
            for o, w in zip(outs, want):
                close_rows(cpu(o), w, tol)
            # in place: the last output is the input itself
            hipbe.lpt_hessian(v, group, outs[:-1] + [v], start, nmesh, box)
            close_rows(cpu(v), want[-1], tol)


# the real blocks of the source kernel and its gradients (ndim 2 or 3), the tall ones among them
SOURCE_SHAPES = [[16, 16, 16], [45, 15, 45], [12, 48, 50], [24, 34]] + [g[0] for g in TALL]


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rdt,tol', [('f8', 1e-12), ('f4', 1e-5)])
def test_source_kernel(hipbe, form, rdt, tol):
    rng = numpy.random.RandomState(8)
    for shape in SOURCE_SHAPES:
        nd = len(shape)
        ins = [_block(shape, rdt, f, rng, complex_=False) for f in (FORMS * 2)[:3 if nd == 2 else 6]]
        ins[0] = _block(shape, rdt, form, rng, complex_=False)
        want = source([cpu(a) for a in ins], 0.375)
        out = _nan_block(shape, rdt, 'strided' if form != 'strided' else 'C', rng, complex_=False)
        hipbe.lpt2_source(ins, out, 0.375)
        close_rows(cpu(out), want, tol)
        hipbe.lpt2_source(ins, ins[0], 0.375)                     # out aliases the first input
        close_rows(cpu(ins[0]), want, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_tabulated_on_field_layouts(hipbe, kind, dtype):
    cdt = {'f8': 'c16', 'f4': 'c8'}[dtype]
    pm = ParticleMesh([24, 20, 18], BoxSize=[60., 50., 40.], dtype=cdt if kind == 'c2c' else dtype)
    rng = numpy.random.RandomState(3)
    r = pm.create(type='real')
    vals = rng.normal(size=tuple(r.value.shape))
    if kind == 'c2c':
        vals = vals + 1j * rng.normal(size=tuple(r.value.shape))
    r.value[...] = torch.from_numpy(vals).to(r.value.device)
    c = r.r2c(out=pm.create(type=UntransposedComplexField if kind == 'U' else TransposedComplexField))
    k, t = table(kmin=0.1, kmax=2.0)
    for loglog in (False, True):
        tab = Tabulated(k, t, loglog=loglog, left=1.0, right=0.5)
        got = c.apply(tab)
        kk = [x.cpu().numpy().astype('f8') for x in
              ParticleMesh(pm.Nmesh, BoxSize=pm.BoxSize, dtype='c16' if kind == 'c2c' else 'f8').create(
                  type=type(c)).x]
        want = scaled(ref_factor(k, t, numpy.sqrt(k_squared(kk)), loglog, 1.0, 1.0, 0.5), cpu(c.value))
        close(cpu(got.value), want, 1e-12 if dtype == 'f8' else 1e-5)


# ---- known answers and identities (GPU) ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('B', [0.7, 0.0])
def test_analytic_plane_waves(hipbe, B):
    N, L, A = 32, 100., 1.3
    pm = ParticleMesh([N, N, N], BoxSize=L, resampler='cic')
    k1, k2 = 2 * numpy.pi * 3 / L, 2 * numpy.pi * 5 / L
    q = pm.generate_uniform_particle_grid(shift=0)
    x, y = cpu(q[:, 0]), cpu(q[:, 1])
    r = pm.create(type='real')
    xs = numpy.arange(N) * L / N
    X, Y = numpy.meshgrid(xs, xs, indexing='ij')
    r.value[...] = torch.from_numpy((A * numpy.cos(k1 * X) + B * numpy.cos(k2 * Y))[:, :, None]
                                    * numpy.ones(N)).to(r.value.device)
    c = r.r2c()
    dx1, dx2 = lpt(c, q)
    dx1, dx2 = cpu(dx1), cpu(dx2)
    tol = 1e-12 * A
    numpy.testing.assert_allclose(dx1[:, 0], -A * numpy.sin(k1 * x) / k1, atol=tol / k1)
    numpy.testing.assert_allclose(dx1[:, 1], -B * numpy.sin(k2 * y) / k2, atol=tol / k2)
    numpy.testing.assert_allclose(dx1[:, 2], 0, atol=tol / k1)
    S = A * B * numpy.cos(k1 * x) * numpy.cos(k2 * y)
    src = lpt2source(c).c2r()
    numpy.testing.assert_allclose(cpu(src.value).reshape(-1), 3 / 7 * S, atol=1e-12 * A * A)
    kk = k1 * k1 + k2 * k2
    numpy.testing.assert_allclose(dx2[:, 0], -3 / 7 * A * B * k1 * numpy.sin(k1 * x) * numpy.cos(k2 * y) / kk,
                                  atol=1e-12 * A * A / k1)
    numpy.testing.assert_allclose(dx2[:, 1], -3 / 7 * A * B * k2 * numpy.cos(k1 * x) * numpy.sin(k2 * y) / kk,
                                  atol=1e-12 * A * A / k1)
    numpy.testing.assert_allclose(dx2[:, 2], 0, atol=1e-12 * A * A / k1)
    if B == 0:
        assert numpy.abs(dx2).max() <= 1e-12 * A * A / k1          # one plane wave: no second order


def _nyquist_mask(shape, nmesh):
    """True off the Nyquist planes of an r2c spectrum of the given mesh"""
    m = numpy.ones(shape, dtype=bool)
    for d, n in enumerate(nmesh):
        if n % 2 == 0:
            sel = [slice(None)] * len(nmesh)
            sel[d] = n // 2
            m[tuple(sel)] = False
    return m


@pytest.mark.gpu
def test_divergence_identities(hipbe):
    """-div dx1 = delta and div dx2 = -3/7 S up to the mean, with a spectral divergence of the displacement fields
    read at the nodes; compared off the Nyquist planes, where the odd factors leave non-Hermitian modes"""
    Nmesh, L = [32, 24, 28], [100., 80., 90.]
    pm = ParticleMesh(Nmesh, BoxSize=L, resampler='cic')
    c = pm.generate_whitenoise(3, unitary=False)
    keep = torch.from_numpy(_nyquist_mask(tuple(c.value.shape), Nmesh)).to(c.value.device)
    c.value[...] = torch.where(keep, c.value, torch.zeros_like(c.value))
    q = pm.generate_uniform_particle_grid(shift=0)
    dx1, dx2 = lpt(c, q)
    k = block_k([0, 0, 0], c.value.shape, Nmesh, pm.BoxSize)
    mask = _nyquist_mask(tuple(c.value.shape), Nmesh)
    mask[0, 0, 0] = False

    def div(rows):
        return sum(1j * k[d] * r2c(cpu(rows[:, d]).reshape(Nmesh)) for d in range(3))
    delta = r2c(c2r(full_spectrum(c), Nmesh))     # the real field's spectrum: c2r keeps the Hermitian part of the noise
    close((-div(dx1))[mask], delta[mask], 1e-12)
    S37 = full_spectrum(lpt2source(c))
    close(div(dx2)[mask], -S37[mask], 1e-12)


@pytest.mark.gpu
def test_lpt1_is_c2r_dx1_readout(hipbe):
    pm = ParticleMesh([32, 32, 32], BoxSize=64.)
    c = pm.generate_whitenoise(11, unitary=False)
    rng = numpy.random.RandomState(2)
    q = torch.from_numpy(rng.uniform(0, 64., size=(5000, 3))).to(hipbe.device)
    got = cpu(lpt1(c, q))
    for d in range(3):
        want = cpu(c.c2r(transfer=Transfer.dx1(d)).readout(q))
        close(got[:, d], want, 1e-14)


@pytest.mark.gpu
def test_linear_field_power(hipbe):
    """unitary noise shaped by Tabulated(k, sqrt(P / V), loglog=True): in every bin, power_spectrum is the mean of the
    tabulated P over that bin's modes.  |w| = 1 on every mode but those the Gadget-compatible noise sets to zero; the
    numpy side takes |w|^2 from the noise itself, so those modes count with power 0 on both sides (asserted below to
    be the k = 0 mode and modes of the Nyquist planes only)."""
    from pmesh_amd.power import power_spectrum
    N, L = 128, 1000.
    pm = ParticleMesh([N, N, N], BoxSize=L)
    V = L ** 3
    k, P = table(n=400, kmin=1e-3, kmax=2.0)
    w = pm.generate_whitenoise(42, unitary=True)
    w2 = numpy.abs(full_spectrum(w)) ** 2
    c = w.apply(Tabulated(k, numpy.sqrt(P / V), loglog=True))
    kf = 2 * numpy.pi / L
    kedges = numpy.arange(0.5 * kf, numpy.pi * N / L * numpy.sqrt(3) + kf, kf)
    res = power_spectrum(c, kedges)
    kk = block_k([0, 0, 0], c.value.shape, [N] * 3, [L] * 3)
    kmag = numpy.broadcast_to(numpy.sqrt(k_squared(kk)), w2.shape)
    zero = w2 < 0.5
    nyq = ~_nyquist_mask(w2.shape, [N] * 3)
    nyq[0, 0, 0] = True
    assert not (zero & ~nyq).any(), 'the noise has zero modes off the Nyquist planes'
    assert (numpy.abs(w2[~zero] - 1) < 1e-12).all()
    iz = numpy.arange(w2.shape[2])
    weight = numpy.broadcast_to(1.0 + ((iz != 0) & (iz != N // 2)), w2.shape)
    p = ref_factor(k, P, kmag, loglog=True) * w2
    b = numpy.digitize(kmag, kedges) - 1
    ok = (b >= 0) & (b < len(kedges) - 1)
    num = numpy.bincount(b[ok], weights=(weight * p)[ok], minlength=len(kedges) - 1)
    den = numpy.bincount(b[ok], weights=weight[ok], minlength=len(kedges) - 1)
    assert (res.modes == den).all()
    want = num / den
    numpy.testing.assert_allclose(res.power.real, want, rtol=1e-10)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (8, [8]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _ranks_equal_one([64, 64, 64], size, np_, 1e-11)


# peak - start of lpt(order=2) at 512^3 f8, in real-field sizes: measured 11.8 on an MI355X (six displacement fields and
# the (n, 6) float64 result of their one readout, n = 512^3, live together), held with a margin
LPT_PEAK_FIELDS = 13.0


@pytest.mark.gpu
def test_lpt_512_memory(hipbe):
    N = 512
    pm = ParticleMesh([N] * 3, BoxSize=1000., resampler='cic')
    c = pm.generate_whitenoise(1, unitary=False)
    q = pm.generate_uniform_particle_grid(shift=0.5)
    torch.cuda.synchronize()
    field = pm.create(type='real')._base.storage.numel() * 8
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dx1, dx2 = lpt(c, q)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / field
    print('lpt(order=2) 512^3 f8: peak %.2f real-field sizes over the inputs' % peak)
    assert torch.isfinite(dx1).all() and torch.isfinite(dx2).all()
    assert float(dx1.abs().max()) > 0 and float(dx2.abs().max()) > 0
    assert peak <= LPT_PEAK_FIELDS, peak


# ---- resources (compiles for gfx950 on the CPU) --------------------------------------------------------------------

def test_lpt_kernels_compile_without_scratch():
    import os
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_lpt.hip')
    kernels = {k: v for k, v in t.items() if any(n in k for n in ('ktable_kernel', 'hessian_kernel',
                                                                   'lpt2_source_kernel'))}
    assert len(kernels) == 14, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)
