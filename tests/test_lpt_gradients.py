"""pmesh_amd.lpt gradients (lpt_vjp, lpt_jvp, lpt2source_vjp, lpt2source_jvp; csrc/pmx_lpt_grad.hip).

The checks are the adjoint identity between the vjp and the jvp, finite differences of lpt itself, the same chain
spelled with existing operators (paint, c2r_vjp, r2c_vjp and numpy factors), and the three kernels against a numpy
restatement.  Under -m "not gpu" the kernels' entries of the C ABI are served by that restatement (GradOracleBackend,
built on test_lpt.LptOracleBackend), so the host layer runs without a GPU.
"""
import numpy
import pytest
import torch

from pmesh_amd import backend
from pmesh_amd.lpt import lpt, lpt2source, lpt2source_jvp, lpt2source_vjp, lpt_jvp, lpt_vjp
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.transfer import Tabulated
from tests.test_lpt import (FORMS, GEOMS, SOURCE_SHAPES, WRAP, LptOracleBackend, _block, _nan_block, block_k, close,
                            close_rows, cpu, hessian_factor, k_squared, table)


# ---- the restatement -----------------------------------------------------------------------------------------------

def factor(k, a, b):
    """k_a k_b / k^2 (b >= 0) or -i k_a / k^2 (b < 0), 0 at k = 0"""
    if b >= 0:
        return hessian_factor(k, a, b)
    k2 = k_squared(k)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        return -1j * numpy.where(k2 == 0, 0.0, k[a] / numpy.where(k2 == 0, 1.0, k2))


def source_vjp(g, phi, scale):
    """scale g dS / dphi_p in the order of operations of pmx_lpt2_source_vjp"""
    a = scale * numpy.asarray(g, 'f8')
    phi = [numpy.asarray(p, 'f8') for p in phi]
    if len(phi) == 3:
        p00, p11, p01 = phi
        return [a * p11, a * p00, a * (-2.0 * p01)]
    p00, p11, p22, p01, p02, p12 = phi
    return [a * (p11 + p22), a * (p22 + p00), a * (p00 + p11), a * (-2.0 * p01), a * (-2.0 * p02), a * (-2.0 * p12)]


def source_jvp(phi, tan, scale):
    """scale dS(phi; tan) in the order of operations of pmx_lpt2_source_jvp"""
    p = [numpy.asarray(x, 'f8') for x in phi]
    q = [numpy.asarray(x, 'f8') for x in tan]
    if len(p) == 3:
        s = (p[0] * q[1] + q[0] * p[1]) - 2.0 * (p[2] * q[2])
    else:
        s = (p[0] * q[1] + q[0] * p[1]) + (p[1] * q[2] + q[1] * p[2])
        s = s + (p[2] * q[0] + q[2] * p[0])
        s = s - 2.0 * (p[3] * q[3])
        s = s - 2.0 * (p[4] * q[4])
        s = s - 2.0 * (p[5] * q[5])
    return scale * s


def contract(ins, factors, k, acc=None):
    out = 0 if acc is None else numpy.asarray(acc).astype('c16')
    for v, (a, b) in zip(ins, factors):
        out = out + factor(k, a, b) * numpy.asarray(v).astype('c16')
    return out


class GradOracleBackend(LptOracleBackend):
    """LptOracleBackend with pmx_lpt_contract, pmx_lpt2_source_vjp and pmx_lpt2_source_jvp served by the
    restatement"""
    name = 'oracle-lpt-grad'

    def lpt_contract(self, ins, factors, out, accumulate, start, nmesh, boxsize):
        k = block_k(start, out.shape, nmesh, boxsize)
        vals = [a.numpy().copy() for a in ins]
        out.copy_(torch.from_numpy(contract(vals, factors, k, out.numpy().copy() if accumulate else None)))

    def lpt2_source_vjp(self, g, ins, outs, scale):
        res = source_vjp(g.numpy(), [a.numpy() for a in ins], scale)
        for o, r in zip(outs, res):
            o.copy_(torch.from_numpy(r))

    def lpt2_source_jvp(self, ins, tangents, out, scale):
        out.copy_(torch.from_numpy(source_jvp([a.numpy() for a in ins], [a.numpy() for a in tangents], scale)))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def gbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(GradOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def nyquist_zero(c):
    """c with its Nyquist planes zeroed, in place"""
    keep = torch.ones(tuple(c.value.shape), dtype=torch.bool, device=c.value.device)
    for d, n in enumerate(c.Nmesh):
        n = int(n)
        if n % 2 == 0:
            keep = keep & (c.i[d] != n // 2).to(keep.device)
    c.value[...] = torch.where(keep, c.value, torch.zeros_like(c.value))
    return c


def spectrum(pm, seed, kind='T'):
    """the r2c spectrum (of the given layout) of a random real field, Nyquist planes zero"""
    rng = numpy.random.RandomState(seed)
    r = pm.create(type='real')
    r.value[...] = torch.from_numpy(rng.normal(size=tuple(r.value.shape))).to(r.value.device)
    c = r.r2c(out=pm.create(type=UntransposedComplexField if kind == 'U' else TransposedComplexField))
    return nyquist_zero(c)


def positions(pm, seed, jitter=0.3):
    """the lattice, each point moved by up to `jitter` cells"""
    rng = numpy.random.RandomState(seed)
    q = cpu(pm.generate_uniform_particle_grid(shift=0.5))
    cell = numpy.asarray(pm.BoxSize, 'f8') / numpy.asarray(pm.Nmesh, 'f8')
    return q + rng.uniform(-jitter, jitter, size=q.shape) * cell


def rows(pm, n, seed):
    return numpy.random.RandomState(seed).normal(size=(n, len(pm.Nmesh)))


MESHES = [([32, 32], 50.), ([16, 16, 16], 100.), ([24, 16, 20], [120., 80., 100.])]


# ---- arguments (both backends) -------------------------------------------------------------------------------------

def test_gradient_arguments(gbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    c = spectrum(pm, 1)
    q = pm.generate_uniform_particle_grid(shift=0)
    v = torch.zeros((len(q), 3), dtype=torch.float64, device=q.device)
    with pytest.raises(ValueError, match='order'):
        lpt_vjp(c, q, v, order=3)
    with pytest.raises(ValueError, match='v_dx2'):
        lpt_vjp(c, q, v, v, order=1)
    with pytest.raises(ValueError, match='v_dx1'):
        lpt_vjp(c, q, v[:, :2])
    with pytest.raises(ValueError, match='v_q'):
        lpt_jvp(c, q, v_q=v[:-1])
    with pytest.raises(ValueError, match='q'):
        lpt_vjp(c, q[:, :2], v)
    with pytest.raises(TypeError):
        lpt_vjp(pm.create(type='real'), q, v)
    with pytest.raises(TypeError):
        lpt_jvp(c, q, v_dlin_k=numpy.zeros((8, 8, 5), 'c16'))
    with pytest.raises(TypeError):
        lpt2source_vjp(c, ParticleMesh([8, 8, 8], BoxSize=100.).create(type='complex'))
    pm1 = ParticleMesh([16], BoxSize=10.)
    c1 = spectrum(pm1, 2)
    q1 = pm1.generate_uniform_particle_grid(shift=0)
    with pytest.raises(ValueError):
        lpt_vjp(c1, q1, numpy.zeros((16, 1)), order=2)
    with pytest.raises(ValueError):
        lpt2source_jvp(c1, c1)
    g, gq = lpt_vjp(c1, q1, numpy.ones((16, 1)), order=1)
    assert gq is None and isinstance(g, TransposedComplexField)
    d1, d2 = lpt_jvp(c1, q1, c1, order=1)
    assert d2 is None and tuple(d1.shape) == (16, 1)
    # no cotangent at all: a zero gradient of dlin_k's type
    cu = spectrum(pm, 3, 'U')
    g, gq = lpt_vjp(cu, q, None, out_q=True)
    assert isinstance(g, UntransposedComplexField) and float(g.value.abs().max()) == 0
    assert float(gq.abs().max()) == 0


# ---- the adjoint identity (both backends) --------------------------------------------------------------------------

@pytest.mark.parametrize('order', [1, 2])
@pytest.mark.parametrize('kind', ['T', 'U'])
@pytest.mark.parametrize('Nmesh,BoxSize', MESHES)
def test_adjoint_identity(gbe, Nmesh, BoxSize, kind, order):
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, resampler='tsc')
    nd = len(Nmesh)
    delta = spectrum(pm, 4, kind)
    u = spectrum(pm, 5, kind)
    q = positions(pm, 6)
    n = len(q)
    v1, v2, w = rows(pm, n, 7), rows(pm, n, 8), rows(pm, n, 9)
    if order == 1:
        v2 = None
    before = delta.value.clone()
    ddx1, ddx2 = lpt_jvp(delta, q, u, w, order=order)
    grad, grad_q = lpt_vjp(delta, q, v1, v2, order=order, out_q=True)
    assert torch.equal(delta.value, before)
    assert type(grad) is type(delta) and tuple(grad_q.shape) == (n, nd)
    lhs = float((cpu(ddx1) * v1).sum())
    if order == 2:
        lhs += float((cpu(ddx2) * v2).sum())
    rhs = u.cdot(grad).real + float((cpu(grad_q) * w).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    if nd >= 2:
        V = spectrum(pm, 10, 'T')
        lhs = V.cdot(lpt2source_jvp(delta, u)).real
        rhs = u.cdot(lpt2source_vjp(delta, V)).real
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)


# ---- finite differences (both backends) ----------------------------------------------------------------------------

def _objective(delta, q, v1, v2):
    dx1, dx2 = lpt(delta, q, order=2)
    return float((cpu(dx1) * v1).sum() + (cpu(dx2) * v2).sum())


def _shifted(c, u, eps):
    out = c.pm.create(type=type(c))
    out.value[...] = c.value + eps * u.value
    return out


@pytest.mark.parametrize('Nmesh,BoxSize', MESHES[:2])
def test_jvp_is_central_difference(gbe, Nmesh, BoxSize):
    """dx1 is linear and dx2 quadratic in delta: the central difference along u is the jvp up to rounding"""
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, resampler='tsc')
    delta, u = spectrum(pm, 11), spectrum(pm, 12)
    q = positions(pm, 13)
    ddx1, ddx2 = lpt_jvp(delta, q, u)
    p1, p2 = lpt(_shifted(delta, u, 0.5), q)
    m1, m2 = lpt(_shifted(delta, u, -0.5), q)
    close(cpu(ddx1), cpu(p1 - m1), 1e-11)
    close(cpu(ddx2), cpu(p2 - m2), 1e-11)
    s1, s2 = lpt2source(_shifted(delta, u, 0.5)), lpt2source(_shifted(delta, u, -0.5))
    close(cpu(lpt2source_jvp(delta, u).value), cpu(s1.value - s2.value), 1e-11)


def _partner(ind, nmesh):
    """the stored Hermitian partner of a mode of the self-conjugate plane of the compressed axis, or None"""
    if ind[-1] not in (0, nmesh[-1] // 2):
        return None
    j = tuple((-i) % n for i, n in zip(ind[:-1], nmesh[:-1])) + (ind[-1],)
    return j


@pytest.mark.parametrize('Nmesh,BoxSize', MESHES[:2])
def test_vjp_single_modes(gbe, Nmesh, BoxSize):
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, resampler='tsc')
    nd = len(Nmesh)
    delta = spectrum(pm, 14)
    q = positions(pm, 15)
    n = len(q)
    v1, v2 = rows(pm, n, 16), rows(pm, n, 17)
    grad, _ = lpt_vjp(delta, q, v1, v2)
    grad.decompress_vjp(Ellipsis)
    g = cpu(grad.value)
    modes = [(1, 2, 3), (3, 5, 0), (0, 1, 1), (6, 0, 2)] if nd == 3 else [(1, 2), (3, 0), (30, 5), (0, 7)]
    dx = 1e-3
    for ind in modes:
        for part in (0, 1):
            if part == 1 and _partner(ind, Nmesh) == ind:
                continue

            def obj(eps):
                c = pm.create(type=type(delta))
                c.value[...] = delta.value
                step = eps if part == 0 else 1j * eps
                c.value[ind] += step
                j = _partner(ind, Nmesh)
                if j is not None and j != ind:
                    c.value[j] += numpy.conj(step)
                return _objective(c, q, v1, v2)
            ng = (obj(dx) - obj(-dx)) / (2 * dx)
            ag = g[ind].real if part == 0 else g[ind].imag
            numpy.testing.assert_allclose(ng, ag, rtol=1e-6, atol=1e-6 * numpy.abs(g).max())


def test_vjp_positions(gbe):
    pm = ParticleMesh([16, 16, 16], BoxSize=100., resampler='tsc')
    delta = spectrum(pm, 18)
    q = positions(pm, 19, jitter=0.2)            # the lattice at cell centres, kept away from the nodes
    n = len(q)
    v1, v2 = rows(pm, n, 20), rows(pm, n, 21)
    _, grad_q = lpt_vjp(delta, q, v1, v2, out_q=True)
    grad_q = cpu(grad_q)
    dx = 1e-5
    for ind in [(0, 0), (77, 1), (1000, 2), (4095, 0)]:
        qp, qm = q.copy(), q.copy()
        qp[ind] += dx
        qm[ind] -= dx
        ng = (_objective(delta, qp, v1, v2) - _objective(delta, qm, v1, v2)) / (2 * dx)
        numpy.testing.assert_allclose(ng, grad_q[ind], rtol=1e-4, atol=1e-8 * numpy.abs(grad_q).max())


# ---- the same chain spelled with existing operators (oracle) -------------------------------------------------------

@pytest.mark.parametrize('Nmesh,BoxSize', MESHES)
def test_vjp_is_the_composition(Nmesh, BoxSize):
    backend.reset()
    backend.use(GradOracleBackend())
    try:
        pm = ParticleMesh(Nmesh, BoxSize=BoxSize, resampler='tsc')
        nd = len(Nmesh)
        delta = spectrum(pm, 22)
        q = positions(pm, 23)
        n = len(q)
        v1, v2 = rows(pm, n, 24), rows(pm, n, 25)
        k = block_k(delta.start, delta.value.shape, pm.Nmesh, pm.BoxSize)

        def times(c, f):
            out = c.pm.create(type=type(c))
            out.value[...] = c.value * torch.from_numpy(numpy.asarray(f, 'c16') * numpy.ones(c.value.shape))
            return out

        def grad_of(v):
            acc = 0
            for d in range(nd):
                p = pm.paint(torch.from_numpy(q), mass=torch.from_numpy(v[:, d].copy()))
                acc = acc + cpu(times(p.c2r_vjp(), factor(k, d, -1)).value)     # conj(i k_d / k^2)
            return acc
        G = grad_of(v1)
        Gsrc = pm.create(type=type(delta))
        Gsrc.value[...] = torch.from_numpy(grad_of(v2))
        g = Gsrc.r2c_vjp()
        pairs = [(d, d) for d in range(nd)] + [(i, j) for i in range(nd) for j in range(i + 1, nd)]
        phi = [cpu(times(delta, hessian_factor(k, i, j)).c2r().value) for i, j in pairs]
        dphi = source_vjp(cpu(g.value), phi, 3.0 / 7.0)
        for (i, j), dp in zip(pairs, dphi):
            r = pm.create(type='real')
            r.value[...] = torch.from_numpy(dp)
            G = G + cpu(times(r.c2r_vjp(), hessian_factor(k, i, j)).value)
        got, _ = lpt_vjp(delta, q, v1, v2)
        close(cpu(got.value), G, 1e-11)
        V = spectrum(pm, 26)
        gs = numpy.zeros_like(G)
        g = V.c2r()
        g.value[...] = g.value / float(numpy.prod(pm.Nmesh))            # r2c_vjp
        for (i, j), dp in zip(pairs, source_vjp(cpu(g.value), phi, 3.0 / 7.0)):
            r = pm.create(type='real')
            r.value[...] = torch.from_numpy(dp)
            gs = gs + cpu(times(r.c2r_vjp(), hessian_factor(k, i, j)).value)
        close(cpu(lpt2source_vjp(delta, V).value), gs, 1e-11)
    finally:
        backend.reset()


# ---- the kernels against the restatement (GPU) ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt,tol', [('c16', 1e-12), ('c8', 1e-5)])
def test_contract_kernel(hipbe, form, cdt, tol):
    rng = numpy.random.RandomState(30)
    for shape, start, nmesh in GEOMS:
        nd = len(nmesh)
        box = [100., 80., 120.][:nd]
        kk = block_k(start, shape, nmesh, box)
        pool = [(i, j) for i in range(nd) for j in range(i, nd)] + [(d, -1) for d in range(nd)]
        # (every number of inputs on the small blocks; the fewest and the most on the tall ones, whose point is the
        # walk over the rows, the same in every instantiation)
        for nin in (range(1, 7) if max(shape) <= WRAP else (1, 6)):
            factors = [pool[(3 * c + nin) % len(pool)] for c in range(nin)]
            ins = [_block(shape, cdt, (FORMS * 2)[c], rng) for c in range(nin)]
            ins[0] = _block(shape, cdt, form, rng)
            vals = [cpu(a) for a in ins]
            for accumulate in (False, True):
                # (without accumulation the output starts as NaN: an element never written cannot pass)
                out = (_block if accumulate else _nan_block)(shape, cdt, 'pad' if form != 'pad' else 'strided', rng)
                acc = cpu(out).copy() if accumulate else None
                hipbe.lpt_contract(ins, factors, out, accumulate, start, nmesh, box)
                close_rows(cpu(out), contract(vals, factors, kk, acc), tol)
            # out aliases the first input, with and without accumulation
            for accumulate in (False, True):
                a0 = cpu(ins[0])
                want = contract([a0] + vals[1:], factors, kk, a0 if accumulate else None)
                hipbe.lpt_contract(ins, factors, ins[0], accumulate, start, nmesh, box)
                close_rows(cpu(ins[0]), want, tol)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rdt,tol', [('f8', 1e-12), ('f4', 1e-5)])
def test_source_gradient_kernels(hipbe, form, rdt, tol):
    rng = numpy.random.RandomState(31)
    for shape in SOURCE_SHAPES:
        nc = 3 if len(shape) == 2 else 6
        phi = [_block(shape, rdt, f, rng, complex_=False) for f in (FORMS * 2)[:nc]]
        tan = [_block(shape, rdt, f, rng, complex_=False) for f in (FORMS * 2)[1:nc + 1]]
        phi[0] = _block(shape, rdt, form, rng, complex_=False)
        g = _block(shape, rdt, form, rng, complex_=False)
        # jvp, out of place and over tan[0]
        want = source_jvp([cpu(a) for a in phi], [cpu(a) for a in tan], 0.375)
        out = _nan_block(shape, rdt, 'strided' if form != 'strided' else 'C', rng, complex_=False)
        hipbe.lpt2_source_jvp(phi, tan, out, 0.375)
        close_rows(cpu(out), want, tol)
        hipbe.lpt2_source_jvp(phi, tan, tan[0], 0.375)
        close_rows(cpu(tan[0]), want, tol)
        # vjp, out of place and over phi
        want = source_vjp(cpu(g), [cpu(a) for a in phi], -1.25)
        outs = [_nan_block(shape, rdt, f, rng, complex_=False) for f in (FORMS * 2)[2:nc + 2]]
        hipbe.lpt2_source_vjp(g, phi, outs, -1.25)
        for o, w in zip(outs, want):
            close_rows(cpu(o), w, tol)
        hipbe.lpt2_source_vjp(g, phi, phi, -1.25)
        for o, w in zip(phi, want):
            close_rows(cpu(o), w, tol)


# ---- ranks equal one -----------------------------------------------------------------------------------------------

def _ranks_equal_one(Nmesh, size, np_, tol):
    from tests import thread_comm
    k, t = table()
    tab = Tabulated(k, numpy.sqrt(t / 1e6), loglog=True)

    def cot(q):
        x = cpu(q)
        return numpy.sin(0.1 * x) + 0.3, numpy.cos(0.07 * x[:, ::-1])

    def make(comm=None):
        kw = {} if comm is None else dict(comm=comm, np=np_)
        pm = ParticleMesh(Nmesh, BoxSize=100., resampler='cic', **kw)
        c = nyquist_zero(pm.generate_whitenoise(7, unitary=False).apply(tab))
        u = nyquist_zero(pm.generate_whitenoise(8, unitary=False).apply(tab))
        q = pm.generate_uniform_particle_grid(shift=0.25)
        v1, v2 = cot(q)
        grad, grad_q = lpt_vjp(c, q, v1, v2, out_q=True)
        d1, d2 = lpt_jvp(c, q, u, v2)
        idx = numpy.floor(cpu(q) / 100. * numpy.asarray(Nmesh)).astype('i8') % numpy.asarray(Nmesh)
        return (numpy.ravel_multi_index(tuple(idx.T), Nmesh), tuple(int(s) for s in grad.start), cpu(grad.value),
                cpu(grad_q), cpu(d1), cpu(d2))
    flat1, _, g1, gq1, a1, b1 = make()
    order = numpy.argsort(flat1)
    results = {}

    def body(comm):
        results[comm.rank] = make(comm)
    thread_comm.run_ranks(size, body)
    assert sum(len(r[0]) for r in results.values()) == numpy.prod(Nmesh)
    scale = numpy.abs(g1).max()
    for flat, start, g, gq, d1, d2 in results.values():
        sel = tuple(slice(s, s + n) for s, n in zip(start, g.shape))
        numpy.testing.assert_allclose(g, g1[sel], rtol=0, atol=tol * scale)
        rows_ = order[numpy.searchsorted(flat1[order], flat)]
        close(gq, gq1[rows_], tol)
        close(d1, a1[rows_], tol)
        close(d2, b1[rows_], tol)


@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (4, [2, 2])])
def test_ranks_equal_one(size, np_):
    backend.reset()
    backend.use(GradOracleBackend())
    try:
        _ranks_equal_one([16, 16, 16], size, np_, 1e-11)
    finally:
        backend.reset()


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (8, [8]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _ranks_equal_one([64, 64, 64], size, np_, 1e-11)


# ---- f4 meshes (GPU) -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_f4_gradients(hipbe):
    out = {}
    for dtype in ('f8', 'f4'):
        pm = ParticleMesh([32, 32, 32], BoxSize=100., resampler='cic', dtype=dtype)
        delta, u = spectrum(pm, 40), spectrum(pm, 41)
        q = positions(pm, 42)
        v1, v2 = rows(pm, len(q), 43), rows(pm, len(q), 44)
        g, gq = lpt_vjp(delta, q, v1, v2, out_q=True)
        d1, d2 = lpt_jvp(delta, q, u, v1)
        out[dtype] = [cpu(g.value).astype('c16'), cpu(gq), cpu(d1), cpu(d2),
                      cpu(lpt2source_vjp(delta, lpt2source(u)).value).astype('c16')]
    for a, b in zip(out['f4'], out['f8']):
        close(a, b, 1e-5)


# ---- a caller's chain (GPU) ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_callers_chain(hipbe):
    """white noise -> Tabulated -> lpt -> paint of q + dx1 + dx2 -> cnorm: the gradient with respect to the noise modes
    from vjps alone against central differences"""
    N, L = 32, 200.
    pm = ParticleMesh([N] * 3, BoxSize=L, resampler='tsc')
    k, t = table(kmin=1e-3, kmax=5.0)
    tab = Tabulated(k, numpy.sqrt(t / L ** 3), loglog=True)
    w = nyquist_zero(pm.generate_whitenoise(5, unitary=True))
    q = pm.generate_uniform_particle_grid(shift=0.5)

    def loss(w):
        dx1, dx2 = lpt(w.apply(tab), q)
        return pm.paint(q + dx1 + dx2).cnorm()
    delta = w.apply(tab)
    dx1, dx2 = lpt(delta, q)
    x = q + dx1 + dx2
    rho = pm.paint(x)
    grad_x, _ = pm.paint_vjp(rho * 2, x, out_mass=False)
    grad_d, _ = lpt_vjp(delta, q, grad_x, grad_x)
    grad_w = grad_d.apply(tab)                       # a real factor: its own vjp
    grad_w.decompress_vjp(Ellipsis)
    g = cpu(grad_w.value)
    dx = 1e-4
    for ind in [(1, 2, 3), (5, 30, 1), (2, 3, 0), (0, 0, 4)]:
        for part in (0, 1):
            def at(eps):
                c = pm.create(type=type(w))
                c.value[...] = w.value
                step = eps if part == 0 else 1j * eps
                c.value[ind] += step
                j = _partner(ind, [N] * 3)
                if j is not None and j != ind:
                    c.value[j] += numpy.conj(step)
                return loss(c)
            ng = (at(dx) - at(-dx)) / (2 * dx)
            ag = g[ind].real if part == 0 else g[ind].imag
            numpy.testing.assert_allclose(ng, ag, rtol=1e-4, atol=1e-6 * numpy.abs(g).max())


# ---- memory (GPU) --------------------------------------------------------------------------------------------------

# peak - start of lpt_vjp(order=2) at 512^3 f8 with both cotangents, in real-field sizes: measured 7.0 on an MI355X (the
# six recomputed Hessian fields with g, or with their transforms in place), held with a margin
LPT_VJP_PEAK_FIELDS = 8.0


@pytest.mark.gpu
def test_lpt_vjp_512_memory(hipbe):
    N = 512
    pm = ParticleMesh([N] * 3, BoxSize=1000., resampler='cic')
    c = nyquist_zero(pm.generate_whitenoise(1, unitary=False))
    q = pm.generate_uniform_particle_grid(shift=0.5)
    v1 = torch.sin(q * 0.01)
    v2 = torch.cos(q * 0.02)
    torch.cuda.synchronize()
    field = pm.create(type='real')._base.storage.numel() * 8
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g, _ = lpt_vjp(c, q, v1, v2)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / field
    print('lpt_vjp(order=2) 512^3 f8: peak %.2f real-field sizes over the inputs' % peak)
    assert torch.isfinite(g.value).all() and float(g.value.abs().max()) > 0
    assert peak <= LPT_VJP_PEAK_FIELDS, peak


# ---- resources (compiles for gfx950 on the CPU) --------------------------------------------------------------------

def test_lpt_gradient_kernels_compile_without_scratch():
    import os
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_lpt_grad.hip')
    kernels = {k: v for k, v in t.items() if any(n in k for n in ('contract_kernel', 'lpt2_source_vjp_kernel',
                                                                   'lpt2_source_jvp_kernel'))}
    assert len(kernels) == 20, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)
