"""Gradients of transfer.Tabulated with respect to the field and the table values (Tabulated.apply_vjp, apply_jvp;
csrc/pmx_ktable_grad.hip).

The checks are the adjoint identity between apply_vjp and apply_jvp, central differences of ``field.apply(table)`` in
single table entries and single stored modes, the two kernels against a numpy restatement of pmx_ktable_vjp and
pmx_apply_ktable_jvp written from the header text, and several ranks against one.  Under -m "not gpu" the entries are
served by the restatement (TableGradOracleBackend, on test_lpt.LptOracleBackend); under -m gpu the same tests run on
the kernels.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.transfer import Tabulated
from tests.test_lpt import (FORMS, TALL, TALL_1D, WRAP, LptOracleBackend, _block, _host_doubles, _nan_block, block_k,
                            k_squared, table)


# ---- the restatement -----------------------------------------------------------------------------------------------

def table_position(kmag, x, loglog, kmin, kmax, real='f8', kmag_real=None):
    """per mode: inside (kmin <= |k| <= kmax), u, the entry j and the fraction f of the header (numpy.interp's rules:
    u <= x[0] sits on entry 0, u >= x[n - 1] on entry n - 1).  kmag_real: |k| in the arithmetic `real` (the decisions,
    inside and j, stay those of the float64 |k|)"""
    n = len(x)
    kmag = numpy.asarray(kmag, dtype='f8')
    inside = (kmag >= kmin) & (kmag <= kmax)
    safe = numpy.where(inside, kmag, kmin)
    u8 = numpy.log(safe) if loglog else safe
    safe = numpy.where(inside, kmag if kmag_real is None else kmag_real, kmin).astype(real)
    u = numpy.log(safe) if loglog else safe
    xr = x.astype(real)
    j = numpy.clip(numpy.searchsorted(x, u8, side='right') - 1, 0, n - 2)
    f = (u - xr[j]) / (xr[j + 1] - xr[j])
    f = numpy.where(u8 <= x[0], 0.0, numpy.where(u8 >= x[n - 1], 1.0, f))
    return inside, u, j, f


def lerp(u, j, f, x, y, real='f8'):
    """g(u) of the header from the entry already found"""
    xr, yr = x.astype(real), y.astype(real)
    s = (yr[j + 1] - yr[j]) / (xr[j + 1] - xr[j])
    g = s * (u - xr[j]) + yr[j]
    return numpy.where(f <= 0, yr[j], numpy.where(f >= 1, yr[j + 1], g))


def ktable_vjp_ref(x, y, loglog, kmin, kmax, field, v, k, last_index, nlast, hermitian, real='f8', kmag_real=None):
    """numpy restatement of pmx_ktable_vjp on one block: the n sums"""
    n = len(x)
    a, v = numpy.asarray(field).astype('c16'), numpy.asarray(v).astype('c16')
    kmag = numpy.broadcast_to(numpy.sqrt(k_squared(k)), a.shape)
    inside, u, j, f = table_position(kmag, x, loglog, kmin, kmax, real, kmag_real)
    r = (v.real * a.real + v.imag * a.imag).astype(real)
    if hermitian:
        r = r * numpy.broadcast_to(1 + ((last_index != 0) & (last_index != nlast // 2)), a.shape)
    if loglog:
        r = r * numpy.exp(lerp(u, j, f, x, y, real))
    r = numpy.where(inside, r, 0)
    out = numpy.zeros(n, dtype=real)
    numpy.add.at(out, j.ravel(), ((1 - f) * r).ravel())
    numpy.add.at(out, j.ravel() + 1, (f * r).ravel())
    return out


def ktable_jvp_ref(x, y, dy, loglog, amplitude, kmin, kmax, field, k, real='f8', kmag_real=None):
    """numpy restatement of pmx_apply_ktable_jvp on one block"""
    a = numpy.asarray(field).astype('c16')
    kmag = numpy.broadcast_to(numpy.sqrt(k_squared(k)), a.shape)
    inside, u, j, f = table_position(kmag, x, loglog, kmin, kmax, real, kmag_real)
    t = lerp(u, j, f, x, dy, real)
    if loglog:
        t = numpy.exp(lerp(u, j, f, x, y, real)) * t
    t = (amplitude * numpy.where(inside, t, 0)).astype('f8')
    return t * a.real + 1j * (t * a.imag)


def _last_index(start, shape):
    nd = len(shape)
    il = numpy.arange(shape[-1]) + int(start[nd - 1])
    return il.reshape((1,) * (nd - 1) + (-1,))


class TableGradOracleBackend(LptOracleBackend):
    """LptOracleBackend with pmx_ktable_vjp and pmx_apply_ktable_jvp served by the restatement"""
    name = 'oracle-table-grad'

    def ktable_vjp(self, table, hermitian, field, v, start, nmesh, boxsize, grad):
        x = _host_doubles(table.x, table.n)
        y = _host_doubles(table.y, table.n)
        k = block_k(start, field.shape, nmesh, boxsize)
        nd = field.dim()
        grad += torch.from_numpy(ktable_vjp_ref(x, y, table.loglog, table.kmin, table.kmax, field.numpy(), v.numpy(),
                                                k, _last_index(start, field.shape), int(nmesh[nd - 1]), hermitian))

    def apply_ktable_jvp(self, table, dy, v, out, start, nmesh, boxsize):
        x = _host_doubles(table.x, table.n)
        y = _host_doubles(table.y, table.n)
        k = block_k(start, v.shape, nmesh, boxsize)
        out.copy_(torch.from_numpy(ktable_jvp_ref(x, y, dy.numpy(), table.loglog, table.amplitude, table.kmin,
                                                  table.kmax, v.numpy(), k)))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def tbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(TableGradOracleBackend())
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


def random_field(pm, kind, seed):
    c = pm.create(type=UntransposedComplexField if kind == 'U' else TransposedComplexField)
    rng = numpy.random.RandomState(seed)
    shape = tuple(c.value.shape)
    c.value[...] = torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape)).to(c.value.device)
    return c


def mesh_k_range(pm):
    kmin = 2 * numpy.pi / float(numpy.max(pm.BoxSize))
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(pm.Nmesh, pm.BoxSize)))
    return kmin, kmax


def inner_table(pm, n, loglog, uniform, seed=0, **kw):
    """a table that covers [1.5 kmin, 0.7 kmax] of the mesh: modes fall below it (left), above it (right) and on it;
    uniform in k (linear) or in ln k (loglog) when asked, irregular otherwise"""
    kmin, kmax = mesh_k_range(pm)
    lo, hi = 1.5 * kmin, 0.7 * kmax
    rng = numpy.random.RandomState(seed)
    if uniform:
        k = numpy.geomspace(lo, hi, n) if loglog else numpy.linspace(lo, hi, n)
    else:
        s = numpy.arange(n, dtype='f8')
        s[1:-1] += rng.uniform(-0.4, 0.4, n - 2)             # steps between 0.2 and 1.8 of the mean
        k = lo + (hi - lo) * s / (n - 1)
    t = (1.0 + 0.5 * numpy.sin(7 * k / hi)) * (k / lo) ** -0.7
    return Tabulated(k, t, loglog=loglog, **kw)


def real_pairing(v, out):
    """Re sum w conj(v) out: the scalar whose gradients apply_vjp returns"""
    return out.cdot(v).real


# ---- arguments (both backends) -------------------------------------------------------------------------------------

def test_gradient_arguments(tbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    c, v = random_field(pm, 'T', 1), random_field(pm, 'T', 2)
    tab = inner_table(pm, 5, False, True)
    with pytest.raises(TypeError):
        tab.apply_vjp(pm.create(type='real'), v)
    with pytest.raises(TypeError):
        tab.apply_vjp(c, numpy.zeros((8, 8, 5), 'c16'))
    with pytest.raises(ValueError, match='layout'):
        tab.apply_vjp(c, random_field(pm, 'U', 3))
    with pytest.raises(ValueError, match='layout'):
        tab.apply_vjp(c, ParticleMesh([8, 8, 8], BoxSize=100., dtype='f4').create(type='complex'))
    with pytest.raises(TypeError):
        tab.apply_jvp(pm.create(type='real'), v_t=numpy.ones(5))
    with pytest.raises(ValueError, match='layout'):
        tab.apply_jvp(c, v_field=random_field(pm, 'U', 3))
    with pytest.raises(ValueError, match='v_t'):
        tab.apply_jvp(c, v_t=numpy.ones(4))
    with pytest.raises(ValueError, match='v_t'):
        tab.apply_jvp(c, v_t=[1, 2, numpy.nan, 4, 5])
    with pytest.raises(NotImplementedError):
        f4 = ParticleMesh([4, 4, 4, 4], BoxSize=1.).create(type='complex')
        tab.apply_vjp(f4, f4)
    g, gt = tab.apply_vjp(c, v, out_t=False)
    assert gt is None and type(g) is type(c)
    z = tab.apply_jvp(c)
    assert type(z) is type(c) and float(z.value.abs().max()) == 0
    before = c.value.clone()
    g, gt = tab.apply_vjp(c, v)
    assert torch.equal(c.value, before) and gt.shape == (5,) and gt.dtype == numpy.float64
    numpy.testing.assert_array_equal(cpu(g.value), cpu(v.apply(tab).value))


# ---- the adjoint identity (both backends) --------------------------------------------------------------------------

ADJOINT = [('T', [16, 12, 10], [40., 30., 50.]), ('U', [16, 12, 10], [40., 30., 50.]), ('c2c', [10, 12, 8], 30.),
           ('T', [24, 20], [50., 40.]), ('U', [20, 24], 30.), ('c2c', [12, 16], [20., 25.]), ('T', [64], 10.),
           ('c2c', [48], 10.)]


@pytest.mark.parametrize('kind,Nmesh,BoxSize', ADJOINT)
@pytest.mark.parametrize('loglog', [False, True])
@pytest.mark.parametrize('uniform', [False, True])
def test_adjoint_identity(tbe, kind, Nmesh, BoxSize, loglog, uniform):
    """Re(V.cdot-pairing of apply_jvp(u, u_t)) == Re(u.cdot(grad_field)) + u_t . grad_t, with modes below, on and
    above the table"""
    pm = make_pm(kind, Nmesh, BoxSize)
    c, u, V = random_field(pm, kind, 3), random_field(pm, kind, 4), random_field(pm, kind, 5)
    tab = inner_table(pm, 9, loglog, uniform, seed=6, amplitude=1.7, left=0.4, right=-0.3)
    kmag = numpy.sqrt(k_squared([cpu(x) for x in c.x]))
    assert (kmag < tab.k[0]).any() and (kmag > tab.k[-1]).any() and ((kmag >= tab.k[0]) & (kmag <= tab.k[-1])).any()
    u_t = numpy.random.RandomState(7).normal(size=9)
    tan = tab.apply_jvp(c, v_field=u, v_t=u_t)
    assert type(tan) is type(c)
    grad_field, grad_t = tab.apply_vjp(c, V)
    lhs = real_pairing(V, tan)
    rhs = u.cdot(grad_field).real + float((u_t * grad_t).sum())
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    # each part alone
    lhs_t = real_pairing(V, tab.apply_jvp(c, v_t=u_t))
    assert abs(lhs_t - float((u_t * grad_t).sum())) <= 1e-10 * max(abs(lhs), abs(rhs))
    assert abs(lhs_t) > 0


# ---- finite differences (both backends) ----------------------------------------------------------------------------

@pytest.mark.parametrize('kind,Nmesh,BoxSize', [ADJOINT[0], ADJOINT[4], ADJOINT[2]])
@pytest.mark.parametrize('loglog', [False, True])
def test_vjp_table_entries_and_single_modes(tbe, kind, Nmesh, BoxSize, loglog):
    """central differences of L = Re sum w conj(V) apply(table)(field) in single table entries (L is linear in a
    linear table's entries and smooth in a log-log table's) and in single stored modes (L is linear in the field)"""
    pm = make_pm(kind, Nmesh, BoxSize)
    c, V = random_field(pm, kind, 8), random_field(pm, kind, 9)
    kw = dict(amplitude=0.8, left=0.4, right=-0.3)
    tab = inner_table(pm, 7, loglog, False, seed=10, **kw)
    grad_field, grad_t = tab.apply_vjp(c, V)

    def loss(t, field=c):
        return real_pairing(V, field.apply(Tabulated(tab.k, t, loglog=loglog, **kw)))
    for i in range(7):
        dt = 1e-4 * tab.t[i]
        tp, tm = tab.t.copy(), tab.t.copy()
        tp[i] += dt
        tm[i] -= dt
        ng = (loss(tp) - loss(tm)) / (2 * dt)
        numpy.testing.assert_allclose(ng, grad_t[i], rtol=1e-6, atol=1e-6 * numpy.abs(grad_t).max())
    g = cpu(grad_field.value)
    w = c._hermitian_weight()
    w = numpy.ones(g.shape) if w is None else numpy.broadcast_to(cpu(w), g.shape)
    rng = numpy.random.RandomState(11)
    dx = 1e-3
    for ind in [tuple(int(rng.randint(n)) for n in g.shape) for _ in range(6)]:
        for part in (0, 1):
            def at(eps):
                f = pm.create(type=type(c))
                f.value[...] = c.value
                f.value[ind] += eps if part == 0 else 1j * eps
                return loss(tab.t, f)
            ng = (at(dx) - at(-dx)) / (2 * dx)
            ag = w[ind] * (g[ind].real if part == 0 else g[ind].imag)
            numpy.testing.assert_allclose(ng, ag, rtol=1e-6, atol=1e-6 * numpy.abs(g).max())


def test_last_entry_and_outside(tbe):
    """a mode exactly on the last tabulated k puts weight 1 on the last entry, one on the first tabulated k weight 1
    on the first; modes outside the table none (left and right are constants)"""
    pm = ParticleMesh([16], BoxSize=2 * numpy.pi, dtype='c16')          # |k| = 0 .. 8 (as the mesh rounds them)
    c = random_field(pm, 'c2c', 12)
    p = numpy.abs(cpu(c.value)) ** 2
    kk = numpy.abs(cpu(c.x[0]))
    ks = numpy.unique(kk)
    assert len(ks) == 9
    tab = Tabulated([ks[2], 3.5, ks[5]], [1.0, 2.0, 4.0], left=9.0, right=9.0)
    _, gt = tab.apply_vjp(c, c)
    want = numpy.zeros(3)
    want[0] += p[kk == ks[2]].sum()
    want[2] += p[kk == ks[5]].sum()
    for kval, lo in ((ks[3], 0), (ks[4], 1)):
        fr = (kval - tab.k[lo]) / (tab.k[lo + 1] - tab.k[lo])
        want[lo] += (1 - fr) * p[kk == kval].sum()
        want[lo + 1] += fr * p[kk == kval].sum()
    numpy.testing.assert_allclose(gt, want, rtol=1e-13)


# ---- the kernels against the restatement (GPU) ---------------------------------------------------------------------

def _refs(tab, c, V, dy):
    x, y = tab._x, tab._y
    k = [cpu(t) for t in _f8_coords(c)]
    il = cpu(c.i[-1])
    args = (x, y, tab.loglog, float(tab.k[0]), float(tab.k[-1]), cpu(c.value), cpu(V.value), k, il,
            int(c.Nmesh[-1]), c.compressed)
    sums = ktable_vjp_ref(*args)
    # the same in longdouble from the integer mode numbers on: |k| = 2 pi |s / L| without the roundings of float64
    ld = numpy.longdouble
    pi = ld(4) * numpy.arctan(ld(1))
    k2 = 0
    for i, n, L in zip(c.i, c.Nmesh, c.BoxSize):
        i = cpu(i).astype('i8')
        sgn = (i - int(n) * (i >= int(n) // 2)).astype(ld)
        k2 = k2 + (sgn * (2 * pi / ld(float(L)))) ** 2
    kld = numpy.broadcast_to(numpy.sqrt(k2), tuple(c.value.shape))
    sums_ld = ktable_vjp_ref(*args, real=ld, kmag_real=kld)
    jargs = (x, y, dy, tab.loglog, tab.amplitude, float(tab.k[0]), float(tab.k[-1]), cpu(c.value), k)
    return sums, sums_ld, ktable_jvp_ref(*jargs), ktable_jvp_ref(*jargs, real=ld, kmag_real=kld)


def _f8_coords(c):
    """the wavenumbers of the field's block from the f8 mesh of its geometry (what the kernels recompute)"""
    pm = c.pm
    pm8 = ParticleMesh(pm.Nmesh, BoxSize=pm.BoxSize, comm=pm.comm, np=pm.np, dtype='c16' if not c.compressed else 'f8')
    return pm8.create(type=type(c)).x


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('loglog', [False, True])
def test_kernels_against_restatement(hipbe, kind, dtype, loglog):
    """tables of 2, 1000 and 8192 entries, uniform and not.  Sums and tangents are held to test_power.assert_same's
    1e-12 of their scale (a complex64 tangent also to half a unit in the last place of float32, 2^-24, per component:
    it is a double rounded once more) plus four times the restatement's own rounding, measured as its distance from
    the same arithmetic in longdouble from the integer mode numbers on: the fraction f = (u - x[j]) / (x[j + 1] - x[j])
    divides the rounding of |k| (or ln |k|) by the step of the table, 1e-4 of the range with 8192 entries, so units in
    the last place of |k| alone move f by 1e-12.  (With |k| taken from float64 the restatement stood 3e-16 of the
    scale from longdouble and the kernel 1.7e-13 / 1.6e-12 from the restatement for 1000 / 8192 linear entries: the
    kernel and numpy round |k| differently in the last place.)  The figures are printed."""
    pm = make_pm(kind, [48, 32, 40], [200., 150., 180.], dtype)
    c, V = random_field(pm, kind, 20), random_field(pm, kind, 21)
    for n in (2, 1000, 8192):
        for uniform in (True, False):
            tab = inner_table(pm, n, loglog, uniform, seed=n, amplitude=1.3, left=0.2, right=0.1)
            v_t = numpy.random.RandomState(n + 1).normal(size=n) * tab.t
            sums, sums_ld, jvp, jvp_ld = _refs(tab, c, V, v_t / tab.t if loglog else v_t)
            per_t = tab.amplitude / (tab.t if loglog else 1.0)
            want = sums * per_t
            own = numpy.abs((sums - sums_ld.astype('f8')) * per_t).max()
            _, got = tab.apply_vjp(c, V)
            scale = numpy.abs(want).max()
            err = numpy.abs(got - want).max()
            print('ktable_vjp %s %s loglog=%d n=%d uniform=%d: err %.2e of scale, restatement vs longdouble %.2e'
                  % (kind, dtype, loglog, n, uniform, err / scale, own / scale))
            assert err <= 1e-12 * scale + 4 * own, (n, uniform, err / scale, own / scale)
            out = cpu(tab.apply_jvp(c, v_t=v_t).value).astype('c16')
            jscale = numpy.abs(jvp).max()
            jown = max(numpy.abs(jvp.real - jvp_ld.real).max(), numpy.abs(jvp.imag - jvp_ld.imag).max())
            for got_c, want_c in ((out.real, jvp.real), (out.imag, jvp.imag)):
                tol = 1e-12 * jscale + 4 * jown + (2.0 ** -24 * numpy.abs(want_c) if dtype == 'f4' else 0.0)
                jerr = numpy.abs(got_c - want_c)
                assert (jerr <= tol).all(), (n, uniform, jerr.max() / jscale, jown / jscale)
            print('ktable_jvp %s %s loglog=%d n=%d uniform=%d: restatement vs longdouble %.2e of scale'
                  % (kind, dtype, loglog, n, uniform, jown / jscale))


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('loglog', [False, True])
def test_kernels_on_tall_blocks(hipbe, form, cdt, loglog):
    """pmx_ktable_vjp and pmx_apply_ktable_jvp called on blocks whose slowest axis has more rows than the launch grid
    (test_lpt.WRAP), in every memory form: against the restatement, the tangent also row by row into an output that
    starts as NaN, and the sums of the rows from WRAP on alone against the whole block's less its first WRAP rows'.
    Tables of 40 entries: a rounding of |k| in the last place moves the fraction f by 40 units in the last place, so
    sums and tangents are held to the 1e-12 of their scale of test_kernels_against_restatement without its allowance
    for the restatement's own rounding (a complex64 tangent also to 2^-24 per component: a double rounded once)."""
    rng = numpy.random.RandomState(22)
    n = 40
    for gi, (shape, start, nmesh) in enumerate(TALL + TALL_1D):
        nd = len(shape)
        box = [100., 80., 120.][:nd]
        long = int(numpy.argmax(shape))
        k = block_k(start, shape, nmesh, box)
        kmag = numpy.broadcast_to(numpy.sqrt(k_squared(k)), tuple(shape))
        lo, hi = 1.5 * kmag[kmag > 0].min(), 0.995 * kmag.max()
        if gi % 2:                                              # uniform (the guessed search) and irregular tables
            kt = numpy.geomspace(lo, hi, n) if loglog else numpy.linspace(lo, hi, n)
        else:
            steps = numpy.arange(n, dtype='f8')
            steps[1:-1] += rng.uniform(-0.4, 0.4, n - 2)
            kt = lo + (hi - lo) * steps / (n - 1)
        tab = Tabulated(kt, (1.0 + 0.5 * numpy.sin(7 * kt / hi)) * (kt / lo) ** -0.7, loglog=loglog, amplitude=1.3,
                        left=0.2, right=0.1)
        past = numpy.take(kmag, numpy.arange(WRAP, shape[long]), axis=long)
        assert ((past >= kt[0]) & (past <= kt[-1])).all() and (kmag < kt[0]).any() and (kmag > kt[-1]).any()
        hermitian = gi % 2 == 0
        a = _block(shape, cdt, form, rng)
        V = _block(shape, cdt, 'pad' if form != 'pad' else 'C', rng)
        x, y, s = tab._table(hipbe.device)

        def sums(rows, first):
            sel = (slice(None),) * long + (rows,)
            st = list(start)
            st[long] += first
            g = torch.zeros(n, dtype=torch.float64, device=hipbe.device)
            hipbe.ktable_vjp(s, hermitian, a[sel], V[sel], st, nmesh, box, g)
            return cpu(g)
        whole, head, tail = sums(slice(None), 0), sums(slice(0, WRAP), 0), sums(slice(WRAP, None), WRAP)
        want = ktable_vjp_ref(tab._x, tab._y, loglog, float(kt[0]), float(kt[-1]), cpu(a), cpu(V), k,
                              _last_index(start, shape), int(nmesh[-1]), hermitian)
        scale = numpy.abs(want).max()
        assert numpy.abs(whole - want).max() <= 1e-12 * scale, (shape, numpy.abs(whole - want).max() / scale)
        assert numpy.abs(tail).max() > 1e-6 * scale
        assert numpy.abs((whole - head) - tail).max() <= 1e-12 * scale, (shape, whole - head, tail)
        # the tangent, out of place and in place
        dy = rng.normal(size=n)
        dyd = torch.from_numpy(dy).to(hipbe.device)
        jvp = ktable_jvp_ref(tab._x, tab._y, dy, loglog, tab.amplitude, float(kt[0]), float(kt[-1]), cpu(a), k)
        jscale = numpy.abs(jvp).max()
        out = _nan_block(shape, cdt, 'strided' if form != 'strided' else 'C', rng)
        hipbe.apply_ktable_jvp(s, dyd, a, out, start, nmesh, box)
        hipbe.apply_ktable_jvp(s, dyd, a, a, start, nmesh, box)
        for got in (cpu(out).astype('c16'), cpu(a).astype('c16')):
            for got_c, want_c in ((got.real, jvp.real), (got.imag, jvp.imag)):
                tol = 1e-12 * jscale + (2.0 ** -24 * numpy.abs(want_c) if cdt == 'c8' else 0.0)
                assert (numpy.abs(got_c - want_c) <= tol).all(), (shape, numpy.abs(got_c - want_c).max() / jscale)
            assert numpy.isfinite(numpy.take(got, numpy.arange(WRAP, shape[long]), axis=long)).all()


# ---- ranks equal one -----------------------------------------------------------------------------------------------

def ranks_case(comm=None, np_=None, Nmesh=(16, 16, 12), loglog=True):
    kw = {} if comm is None else dict(comm=comm, np=np_)
    pm = ParticleMesh(list(Nmesh), BoxSize=100., **kw)
    c = pm.generate_whitenoise(5, unitary=False, type='complex')
    V = pm.generate_whitenoise(6, unitary=False, type='complex')
    tab = inner_table(pm, 11, loglog, False, seed=3, amplitude=1.2, left=0.5, right=0.25)
    g, gt = tab.apply_vjp(c, V)
    tan = tab.apply_jvp(c, v_field=V, v_t=numpy.cos(numpy.arange(11.0)) * tab.t)
    return tuple(int(s) for s in g.start), cpu(g.value), gt, cpu(tan.value)


def compare_ranks(one, many, tol=1e-11):
    _, g1, gt1, tan1 = one
    start, g, gt, tan = many
    sel = tuple(slice(s, s + n) for s, n in zip(start, g.shape))
    numpy.testing.assert_allclose(g, g1[sel], rtol=0, atol=tol * numpy.abs(g1).max())
    numpy.testing.assert_allclose(tan, tan1[sel], rtol=0, atol=tol * numpy.abs(tan1).max())
    numpy.testing.assert_allclose(gt, gt1, rtol=0, atol=tol * numpy.abs(gt1).max())       # equal after the sum


def _thread_ranks(size, np_, Nmesh, loglog):
    from tests import thread_comm
    one = ranks_case(Nmesh=Nmesh, loglog=loglog)
    results = {}

    def body(comm):
        results[comm.rank] = ranks_case(comm, np_, Nmesh, loglog)
    thread_comm.run_ranks(size, body)
    assert sum(r[1].size for r in results.values()) == one[1].size
    for r in results.values():
        compare_ranks(one, r)


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
@pytest.mark.parametrize('loglog', [False, True])
def test_ranks_equal_one(tbe, size, np_, loglog):
    _thread_ranks(size, np_, [16, 16, 12], loglog)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(4, [4]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _thread_ranks(size, np_, [64, 64, 48], True)


# ---- 512^3 (GPU) ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_apply_vjp_512_memory(hipbe):
    """one apply_vjp at 512^3 f8 with a table of 1000 entries: finite, non-zero, and no more memory than the output
    field and one more field over the inputs (the kernel allocates nothing)"""
    N = 512
    pm = ParticleMesh([N] * 3, BoxSize=1000.)
    c = pm.generate_whitenoise(1, unitary=False, type='complex')
    V = pm.generate_whitenoise(2, unitary=False, type='complex')
    tab = inner_table(pm, 1000, True, True)
    torch.cuda.synchronize()
    field = c._base.storage.numel() * c._base.storage.element_size()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    g, gt = tab.apply_vjp(c, V)
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / field
    print('Tabulated.apply_vjp 512^3 f8: peak %.3f field sizes over the inputs' % peak)
    assert numpy.isfinite(gt).all() and numpy.abs(gt).max() > 0
    # which entries can receive anything: the table is uniform in ln k and far finer than the mesh at its low end, so
    # most pairs of low entries have no mode between them and their gradient is exactly zero.  An entry must be
    # non-zero when a mode lies well inside one of its two intervals, and may be only when one lies in or at them.
    x = c.x
    kmag = torch.sqrt(x[0].double() ** 2 + x[1].double() ** 2 + x[2].double() ** 2).reshape(-1)
    kt = torch.from_numpy(tab.k).to(kmag.device)
    n = len(tab.k)

    def touched(lo_edges, hi_edges, sel):
        j = (torch.bucketize(kmag[sel], kt, right=True) - 1).clamp(0, n - 2)
        ok = (kmag[sel] > lo_edges[j]) & (kmag[sel] < hi_edges[j + 1])
        hit = torch.zeros(n, dtype=torch.bool, device=kmag.device)
        hit[j[ok]] = True
        hit[j[ok] + 1] = True
        return hit.cpu().numpy()
    inside = (kmag >= kt[0]) & (kmag <= kt[-1])
    must = touched(kt * (1 + 1e-9), kt * (1 - 1e-9), inside)
    wide = (kmag >= kt[0] * (1 - 1e-9)) & (kmag <= kt[-1] * (1 + 1e-9))
    j = (torch.bucketize(kmag[wide], kt, right=True) - 1).clamp(0, n - 2)
    may = torch.zeros(n, dtype=torch.bool, device=kmag.device)
    for d in (-1, 0, 1, 2):                                # (a mode within rounding of a knot may fall to either side)
        may[(j + d).clamp(0, n - 1)] = True
    may = may.cpu().numpy()
    print('Tabulated.apply_vjp 512^3 f8: %d of %d entries non-zero, %d must be, %d may be'
          % ((gt != 0).sum(), n, must.sum(), may.sum()))
    assert must.sum() > 100
    assert (gt[must] != 0).all() and (gt[~may] == 0).all()
    assert torch.isfinite(torch.view_as_real(g.value)).all() and float(g.value.abs().max()) > 0
    assert peak <= 2.0, peak


# ---- resources (compiles for gfx950 on the CPU) --------------------------------------------------------------------

def test_table_gradient_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_ktable_grad.hip')
    kernels = {k: v for k, v in t.items() if 'ktable_vjp_kernel' in k or 'ktable_jvp_kernel' in k}
    assert len(kernels) == 8, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)
