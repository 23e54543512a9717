"""pmesh_amd.survey (csrc/pmx_survey.hip) against a numpy restatement of its definitions.

The restatement builds the real orthonormal harmonics Y_lm (no Condon-Shortley phase) from the associated-Legendre
recurrence and arctan2, the cell positions x_d = (g_d * L_d) / N_d, the wavenumbers of a block from pm._block_coords,
and the two entries of the C ABI (pmx_ylm_weight, pmx_ylm_accumulate) from them.  The multipole field itself is checked
against the brute-force Legendre sum over all cell / mode pairs, which uses no harmonics at all.  Under -m "not gpu"
the restatement serves the two entries (SurveyOracleBackend), so the host layer runs without a GPU; under -m gpu the
kernels are compared with it.
"""
import math

import numpy
import pytest
import torch
from numpy.polynomial import legendre

from pmesh_amd import backend
from pmesh_amd.pm import ParticleMesh, RealField, TransposedComplexField, UntransposedComplexField
from pmesh_amd.power import power_spectrum
from pmesh_amd.survey import SurveyResult, multipole_field, survey_multipoles
from tests.test_lpt import FORMS, _block, _nan_block, block_k, close, close_rows, cpu
from tests.test_power import PowerOracleBackend, density, kf_edges


# ---- the restatement -----------------------------------------------------------------------------------------------

def assoc_legendre(l, m, c, s):
    """P_l^m = s^m d^m P_l / dc^m for c = cos th, s = sin th >= 0 (no Condon-Shortley phase): P_m^m = (2m-1)!! s^m,
    P_{m+1}^m = (2m+1) c P_m^m, (n-m) P_n^m = (2n-1) c P_{n-1}^m - (n+m-1) P_{n-2}^m"""
    prev = numpy.ones_like(c)
    for j in range(1, m + 1):
        prev = prev * (2 * j - 1) * s
    if l == m:
        return prev
    cur = (2 * m + 1) * c * prev
    for n in range(m + 2, l + 1):
        prev, cur = cur, ((2 * n - 1) * c * cur - (n + m - 1) * prev) / (n - m)
    return cur


def ylm(l, m, v):
    """Y_lm of the direction of v = [x, y, z] (broadcastable arrays); a zero vector has Y_00 alone"""
    x, y, z = numpy.broadcast_arrays(*[numpy.asarray(a, dtype='f8') for a in v])
    r = numpy.sqrt((x * x + y * y) + z * z)
    zero = r == 0
    rs = numpy.where(zero, 1.0, r)
    c, s = z / rs, numpy.hypot(x, y) / rs
    ph = numpy.arctan2(y, x)
    am = abs(m)
    norm = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - am) / math.factorial(l + am))
    val = norm * assoc_legendre(l, am, c, s)
    if m > 0:
        val = math.sqrt(2.0) * val * numpy.cos(am * ph)
    elif m < 0:
        val = math.sqrt(2.0) * val * numpy.sin(am * ph)
    return numpy.where(zero, norm if l == 0 else 0.0, val)


def cell_positions(start, shape, nmesh, boxsize):
    """x_d = (g_d * L_d) / N_d per axis, shaped to broadcast"""
    out = []
    for d in range(3):
        g = (numpy.arange(int(shape[d])) + int(start[d])).astype('f8')
        along = [int(shape[d]) if dd == d else 1 for dd in range(3)]
        out.append(((g * float(boxsize[d])) / float(nmesh[d])).reshape(along))
    return out


def ref_weight(l, m, vals, start, nmesh, boxsize, origin):
    """pmx_ylm_weight: in * Y_lm(r_hat), r = x - origin"""
    x = cell_positions(start, vals.shape, nmesh, boxsize)
    return numpy.asarray(vals, dtype='f8') * ylm(l, m, [x[d] - float(origin[d]) for d in range(3)])


def ref_accumulate(l, m, beta, vals, acc, start, nmesh, boxsize):
    """pmx_ylm_accumulate: beta * acc + (4 pi / (2l+1)) Y_lm(k_hat) * in, component by component in double"""
    f = 4 * math.pi / (2 * l + 1) * ylm(l, m, block_k(start, vals.shape, nmesh, boxsize))
    vals = numpy.asarray(vals).astype('c16')
    out = f * vals.real + 1j * (f * vals.imag)
    return out + numpy.asarray(acc).astype('c16') if beta else out


def brute_multipole(F, nmesh, boxsize, origin, l):
    """(1 / prod N) sum_x F(x) L_l(k_hat . r_hat) exp(-i k.x) over every cell / mode pair of the one-rank r2c
    spectrum, L_l taken as [l == 0] at k = 0 or r = 0"""
    nmesh = [int(n) for n in nmesh]
    cshape = (nmesh[0], nmesh[1], nmesh[2] // 2 + 1)
    x = cell_positions([0, 0, 0], nmesh, nmesh, boxsize)
    r = numpy.stack([numpy.broadcast_to(x[d] - float(origin[d]), nmesh).reshape(-1) for d in range(3)], axis=1)
    k = block_k([0, 0, 0], cshape, nmesh, boxsize)
    k = numpy.stack([numpy.broadcast_to(k[d], cshape).reshape(-1) for d in range(3)], axis=1)
    rn, kn = numpy.sqrt((r * r).sum(axis=1)), numpy.sqrt((k * k).sum(axis=1))
    rh = r / numpy.where(rn == 0, 1.0, rn)[:, None]
    kh = k / numpy.where(kn == 0, 1.0, kn)[:, None]
    mu = numpy.clip(kh @ rh.T, -1.0, 1.0)                               # (modes, cells)
    L = legendre.legval(mu, [0] * l + [1])
    L[(kn == 0)[:, None] | (rn == 0)[None, :]] = 1.0 if l == 0 else 0.0
    # the phase from integer arithmetic: k.x = 2 pi sum_d i_d g_d / N_d
    ph = numpy.zeros((len(k), len(r)))
    for d in range(3):
        i = numpy.broadcast_to(numpy.arange(cshape[d]).reshape([-1 if dd == d else 1 for dd in range(3)]),
                               cshape).reshape(-1)
        g = numpy.broadcast_to(numpy.arange(nmesh[d]).reshape([-1 if dd == d else 1 for dd in range(3)]),
                               nmesh).reshape(-1)
        ph += (numpy.outer(i, g) % nmesh[d]) / float(nmesh[d])
    A = (L * numpy.exp(-2j * numpy.pi * ph)) @ numpy.asarray(F, dtype='f8').reshape(-1)
    return (A / float(numpy.prod(nmesh))).reshape(cshape)


# ---- the C ABI served by the restatement (CPU) ---------------------------------------------------------------------

class SurveyOracleBackend(PowerOracleBackend):
    """the CPU test double with pmx_ylm_weight and pmx_ylm_accumulate served by the restatement"""
    name = 'oracle-survey'

    def ylm_weight(self, ell, m, v, out, start, nmesh, boxsize, origin):
        want = ref_weight(ell, m, v.numpy(), start, nmesh, boxsize, origin)
        out.copy_(torch.from_numpy(want))

    def ylm_accumulate(self, ell, m, beta, v, acc, start, nmesh, boxsize):
        want = ref_accumulate(ell, m, beta, v.numpy(), acc.numpy().copy(), start, nmesh, boxsize)
        acc.copy_(torch.from_numpy(want))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def sbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(SurveyOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


BOX = [100., 80., 120.]
MESHES = [(8, 6, 10), (9, 8, 6)]
ORDERS = (0, 2, 4)


def origins(nmesh):
    """outside the box; exactly on cell (2, 3, 4), the r = 0 case; inside, on no cell"""
    return [(-30., 40., -250.), tuple((g * L) / n for g, L, n in zip((2, 3, 4), BOX, nmesh)), (50., 40., 60.)]


def field_values(nmesh, seed=11, single=False):
    """the global values of a random real field (single: representable in float32)"""
    v = numpy.random.RandomState(seed).normal(size=tuple(nmesh))
    return v.astype('f4').astype('f8') if single else v


def real_field(pm, values):
    r = pm.create(type='real')
    r.value[...] = torch.from_numpy(numpy.ascontiguousarray(values[r.slices])).to(r.value.device)
    return r


_BRUTE = {}


def brute(nmesh, which, l, single=False):
    """brute_multipole of field_values(nmesh) for origins(nmesh)[which], computed once per session"""
    key = (tuple(nmesh), which, l, single)
    if key not in _BRUTE:
        _BRUTE[key] = brute_multipole(field_values(nmesh, single=single), nmesh, BOX, origins(nmesh)[which], l)
    return _BRUTE[key]


# ---- 1. the addition theorem (both backends) -----------------------------------------------------------------------

def test_restated_harmonics_are_orthonormal():
    """the restatement itself: orthonormal on a Gauss-Legendre x uniform-phi quadrature, the stated signs"""
    c, w = legendre.leggauss(12)
    ph = (numpy.arange(16) + 0.5) * (2 * numpy.pi / 16)
    C, P = numpy.meshgrid(c, ph, indexing='ij')
    S = numpy.sqrt(1 - C * C)
    v = [S * numpy.cos(P), S * numpy.sin(P), C]
    W = w[:, None] * (2 * numpy.pi / 16)
    lm = [(l, m) for l in ORDERS for m in range(-l, l + 1)]
    Y = numpy.array([ylm(l, m, v) for l, m in lm])
    gram = numpy.einsum('aij,bij,ij->ab', Y, Y, W)
    numpy.testing.assert_allclose(gram, numpy.eye(len(lm)), atol=1e-13)
    x, y, z = 0.3, -0.5, 0.7
    assert ylm(2, 2, [x, y, z]) * (x * x - y * y) > 0 and ylm(2, 1, [x, y, z]) * (x * z) > 0
    assert ylm(2, -1, [x, y, z]) * (y * z) > 0
    assert ylm(0, 0, [0., 0., 0.]) == 1 / math.sqrt(4 * math.pi) and ylm(4, 0, [0., 0., 0.]) == 0


@pytest.mark.parametrize('nmesh', MESHES)
@pytest.mark.parametrize('which', [0, 1, 2])
def test_addition_theorem(sbe, nmesh, which):
    pm = ParticleMesh(nmesh, BoxSize=BOX, dtype='f8')
    F = real_field(pm, field_values(nmesh))
    before = F.value.clone()
    org = origins(nmesh)[which]
    scale = numpy.abs(brute(nmesh, which, 0)).max()
    for l in ORDERS:
        got = cpu(multipole_field(F, l, org).value)
        want = brute(nmesh, which, l)
        err = numpy.abs(got - want).max() / scale
        print('Nmesh %s origin %d l = %d: error %.2e of the maximum of A_0' % (nmesh, which, l, err))
        close(got, want, 1e-12)
        assert torch.equal(F.value, before)
    close(cpu(multipole_field(F, 0, org).value), cpu(F.r2c().value), 1e-15)


# ---- 2. the kernels against the restatement (GPU) ------------------------------------------------------------------

LM = [(l, m) for l in ORDERS for m in range(-l, l + 1)]               # all 15 pairs
TALL = ([65541, 2, 3], [1000, 0, 0], [131072, 2, 4])                   # more rows than the 65535-row launch wrap
REAL_GEOMS = [([16, 16, 16], [0, 0, 0], [16, 16, 16]),
              ([45, 15, 45], [0, 0, 0], [45, 45, 45]),
              ([12, 48, 50], [36, 0, 0], [48, 48, 50]),
              TALL]
COMPLEX_GEOMS = [([16, 16, 9], [0, 0, 0], [16, 16, 16]),                # an r2c half spectrum, k = 0 in it
                 ([45, 15, 45], [0, 0, 0], [45, 45, 45]),
                 ([12, 48, 25], [36, 0, 0], [48, 48, 48]),
                 TALL]
# Real blocks sit in the anisotropic box BOX.  Complex blocks take a box of anisotropic cells instead: in BOX the modes of
# the tall block, 131072 x 2 x 4, all point along the x axis to 1e-5, where every harmonic with odd or negative m
# vanishes, and the rows past the launch wrap, compared on their own scale, would measure the restatement's own
# sin(m * arctan2(0, -1)) = 4e-16 against values of 1e-9
CELL = (6.25, 5.0, 7.5)


def complex_box(nmesh):
    return [c * n for c, n in zip(CELL, nmesh)]


# the first real block holds the origin's cell (r = 0); the others see the observer from outside or inside the box
KERNEL_ORIGINS = [tuple((g * L) / n for g, L, n in zip((3, 5, 7), BOX, (16, 16, 16))), (-30., 40., -250.),
                  (50., 40., 60.), (-30., 40., -250.)]


def pairs_of(gi):
    """every (l, m) runs on one geometry, every geometry runs a few (l, m)"""
    return [lm for j, lm in enumerate(LM) if j % 4 == gi]


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rdt,tol', [('f8', 1e-12), ('f4', 1e-5)])
def test_weight_kernel(hipbe, form, rdt, tol):
    rng = numpy.random.RandomState(21)
    ran = []
    for gi, (shape, start, nmesh) in enumerate(REAL_GEOMS):
        org = KERNEL_ORIGINS[gi]
        if gi == 0:
            x = cell_positions(start, shape, nmesh, BOX)
            assert all((x[d].reshape(-1) == org[d]).any() for d in range(3))
        for l, m in pairs_of(gi):
            v = _block(shape, rdt, form, rng, complex_=False)
            want = ref_weight(l, m, cpu(v), start, nmesh, BOX, org)
            out = _nan_block(shape, rdt, 'pad' if form != 'pad' else 'C', rng, complex_=False)
            hipbe.ylm_weight(l, m, v, out, start, nmesh, BOX, org)
            close_rows(cpu(out), want, tol)
            hipbe.ylm_weight(l, m, v, v, start, nmesh, BOX, org)              # in place
            close_rows(cpu(v), want, tol)
            ran.append((l, m))
    assert sorted(ran) == sorted(LM)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt,tol', [('c16', 1e-12), ('c8', 1e-5)])
def test_accumulate_kernel(hipbe, form, cdt, tol):
    rng = numpy.random.RandomState(22)
    ran = []
    for gi, (shape, start, nmesh) in enumerate(COMPLEX_GEOMS):
        pairs = pairs_of(gi)
        box = complex_box(nmesh)
        for j, (l, m) in enumerate(pairs):
            l2, m2 = pairs[(j + 1) % len(pairs)]
            v = _block(shape, cdt, form, rng)
            v2 = _block(shape, cdt, 'strided' if form != 'strided' else 'T', rng)
            first = ref_accumulate(l, m, 0, cpu(v), None, start, nmesh, box)
            acc = _nan_block(shape, cdt, 'pad' if form != 'pad' else 'C', rng)
            hipbe.ylm_accumulate(l, m, 0, v, acc, start, nmesh, box)         # beta = 0 into NaN memory
            got = cpu(acc)
            close_rows(got, first, tol)
            want = ref_accumulate(l2, m2, 1, cpu(v2), got, start, nmesh, box)
            hipbe.ylm_accumulate(l2, m2, 1, v2, acc, start, nmesh, box)      # then beta = 1 onto it
            close_rows(cpu(acc), want, tol)
            ran.append((l, m))
    assert sorted(ran) == sorted(LM)


@pytest.mark.gpu
def test_kernels_refuse_what_they_do_not_do(hipbe):
    from pmesh_amd import _abi
    rng = numpy.random.RandomState(1)
    r = _block([4, 4, 4], 'f8', 'C', rng, complex_=False)
    c = _block([4, 4, 3], 'c16', 'C', rng)
    for l, m in ((1, 0), (3, 1), (6, 0), (2, 3), (0, 1), (4, -5)):
        with pytest.raises(backend.PmxError) as e:
            hipbe.ylm_weight(l, m, r, r, [0] * 3, [4] * 3, BOX, (0., 0., 0.))
        assert e.value.code == _abi.PMX_EUNSUPPORTED
        with pytest.raises(backend.PmxError) as e:
            hipbe.ylm_accumulate(l, m, 0, c, c, [0] * 3, [4] * 3, BOX)
        assert e.value.code == _abi.PMX_EUNSUPPORTED
    with pytest.raises(backend.PmxError) as e:
        hipbe.ylm_weight(2, 0, r[0], r[0], [0] * 2, [4] * 2, BOX[:2], (0., 0., 0.))
    assert e.value.code == _abi.PMX_EUNSUPPORTED
    with pytest.raises(backend.PmxError) as e:
        hipbe.ylm_accumulate(2, 0, 0, c[0], c[0], [0] * 2, [4] * 2, BOX[:2])
    assert e.value.code == _abi.PMX_EUNSUPPORTED


# ---- 3. result assembly (both backends) ----------------------------------------------------------------------------

def assembly_edges(pm):
    """k_f-spaced edges, then a bin too narrow to hold a mode and one past every mode: empty bins"""
    e = kf_edges(pm)
    return numpy.concatenate([e[:6], [e[5] + 1e-9], [e[-1] + 1.0, e[-1] + 2.0]])


def test_result_assembly(sbe):
    nmesh = (12, 10, 8)
    pm = ParticleMesh(nmesh, BoxSize=BOX, dtype='f8')
    F = real_field(pm, field_values(nmesh, seed=3))
    G = real_field(pm, field_values(nmesh, seed=4))
    org = (-30., 40., -250.)
    e = assembly_edges(pm)
    res = survey_multipoles(F, e, org)
    assert isinstance(res, SurveyResult) and sorted(res.poles) == [0, 2, 4]
    A0 = F.r2c()
    close(cpu(res.A0.value), cpu(A0.value), 1e-15)
    base = power_spectrum(A0, e)
    assert (res.kedges == e).all() and (res.modes == base.modes).all()
    empty = base.modes == 0
    assert empty.any() and not empty.all()
    close(res.k[~empty], base.k[~empty], 1e-13)               # (sums of the device's float atomics: not bit for bit)
    assert numpy.isnan(res.k[empty]).all()
    for l in ORDERS:
        want = (2 * l + 1) * power_spectrum(A0, e, other=multipole_field(F, l, org)).power
        assert numpy.isnan(res.poles[l][empty]).all() and numpy.isfinite(res.poles[l][~empty]).all()
        close(res.poles[l][~empty], want[~empty], 1e-13)
    close(res.poles[0][~empty], base.power[~empty], 1e-13)
    # a subset of the orders, in the caller's order
    sub = survey_multipoles(F, e, org, poles=(4, 0))
    assert list(sub.poles) == [4, 0]
    close(sub.poles[4][~empty], res.poles[4][~empty], 1e-13)
    # other: A_0 of the field against A_l of the other
    cross = survey_multipoles(F, e, org, other=G)
    for l in ORDERS:
        want = (2 * l + 1) * power_spectrum(A0, e, other=multipole_field(G, l, org)).power
        close(cross.poles[l][~empty], want[~empty], 1e-13)
    assert numpy.abs(cross.poles[2][~empty] - res.poles[2][~empty]).max() > 1e-3 * numpy.abs(res.poles[2][~empty]).max()
    # deconv_pow reaches the binning
    dec = survey_multipoles(F, e, org, poles=(2,), deconv_pow=2)
    want = 5 * power_spectrum(A0, e, other=multipole_field(F, 2, org), deconv_pow=2).power
    close(dec.poles[2][~empty], want[~empty], 1e-13)
    assert numpy.abs(dec.poles[2][~empty] - res.poles[2][~empty]).max() > 1e-3 * numpy.abs(res.poles[2][~empty]).max()


# ---- 4. the plane-parallel limit (both backends) -------------------------------------------------------------------

def test_plane_parallel_limit(sbe):
    """An observer at distance 1e8 L below the box centre sees every cell within sqrt(2)/2 * 1e-8 rad of the z axis;
    L_l changes by at most l (l + 1) / 2 times that, and the cancellation in x - origin costs about 1e-8 more: the
    multipoles are those about the global line of sight z within 1e-6 of their maximum."""
    L = 100.
    pm = ParticleMesh([16, 16, 16], BoxSize=L, dtype='f8')
    F = density(pm, seed=6)
    e = kf_edges(pm)
    res = survey_multipoles(F, e, (L / 2, L / 2, -1e8 * L))
    want = power_spectrum(F, e, poles=ORDERS, los=[0, 0, 1])
    assert (res.modes == want.modes).all()
    for l in ORDERS:
        ok = want.modes > 0
        err = numpy.abs(res.poles[l][ok] - want.poles[l][ok]).max() / numpy.abs(want.poles[l][ok]).max()
        print('plane-parallel l = %d: error %.2e of the maximum' % (l, err))
        close(res.poles[l][ok], want.poles[l][ok], 1e-6)


# ---- 5. layouts and precision (GPU) --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('nmesh', MESHES)
@pytest.mark.parametrize('kind', ['T', 'U'])
def test_layouts_and_precision(hipbe, nmesh, kind):
    """f8 against the brute-force sum; f4 against f8 within 4 (2l + 1) times the error of the f4 r2c of the same field
    against its f8 r2c: one transform's rounding per m, with a margin of 4 for the rounding of the weights"""
    T = UntransposedComplexField if kind == 'U' else TransposedComplexField
    org = origins(nmesh)[0]
    vals = field_values(nmesh, single=True)
    pm8 = ParticleMesh(nmesh, BoxSize=BOX, dtype='f8')
    pm4 = ParticleMesh(nmesh, BoxSize=BOX, dtype='f4')
    F8, F4 = real_field(pm8, vals), real_field(pm4, vals)
    assert F4.value.dtype == torch.float32
    r2c_err = numpy.abs(cpu(F4.r2c(out=pm4.create(type=T)).value).astype('c16')
                        - cpu(F8.r2c(out=pm8.create(type=T)).value)).max()
    assert r2c_err > 0
    for l in ORDERS:
        out8 = pm8.create(type=T)
        got8 = multipole_field(F8, l, org, out=out8)
        assert got8 is out8
        a8 = cpu(got8.value)
        close(a8, brute(nmesh, 0, l, single=True), 1e-12)
        got4 = multipole_field(F4, l, org, out=pm4.create(type=T))
        assert got4.value.dtype == torch.complex64 and isinstance(got4, T)
        err = numpy.abs(cpu(got4.value).astype('c16') - a8).max()
        print('Nmesh %s %s l = %d: f4 error %.3e = %.2f x the f4 r2c error %.3e (bound %d)'
              % (nmesh, kind, l, err, err / r2c_err, r2c_err, 4 * (2 * l + 1)))
        assert err <= 4 * (2 * l + 1) * r2c_err


# ---- 6. ranks (both backends) --------------------------------------------------------------------------------------

@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (4, [2, 2])])
def test_ranks_equal_one(sbe, size, np_):
    from tests import thread_comm
    nmesh, org = [16, 16, 16], (-30., 40., -250.)

    def run(comm=None):
        kw = {} if comm is None else dict(comm=comm, np=np_)
        pm = ParticleMesh(nmesh, BoxSize=BOX, **kw)
        return survey_multipoles(density(pm, seed=5), kf_edges(pm), org, deconv_pow=2)
    one = run()
    results = {}

    def body(comm):
        results[comm.rank] = run(comm)
    thread_comm.run_ranks(size, body)
    assert len(results) == size
    ok = one.modes > 0
    for r in results.values():
        assert (r.modes == one.modes).all()
        close(r.k[ok], one.k[ok], 1e-11)
        for l in ORDERS:
            close(r.poles[l][ok], one.poles[l][ok], 1e-11)
            assert numpy.isnan(r.poles[l][~ok]).all()


# ---- 7. arguments (both backends) ----------------------------------------------------------------------------------

def test_arguments(sbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    F = pm.create(type='real')
    e = kf_edges(pm)
    org = (0., 0., -500.)
    for bad in (pm.create(type='complex'), numpy.zeros((8, 8, 8)), None):
        with pytest.raises(TypeError):
            survey_multipoles(bad, e, org)
        with pytest.raises(TypeError):
            multipole_field(bad, 2, org)
    with pytest.raises(TypeError):
        survey_multipoles(F, e, org, other=pm.create(type='complex'))
    for n in ([16, 16], [4, 4, 4, 4]):
        low = ParticleMesh(n, BoxSize=10.).create(type='real')
        with pytest.raises(NotImplementedError):
            survey_multipoles(low, e, org)
        with pytest.raises(NotImplementedError):
            multipole_field(low, 2, org)
    for bad in ((1,), (0, 3), (6,), (-2,), (0, 2, 2), (2.5,), ('a',)):
        with pytest.raises(ValueError, match='poles|orders'):
            survey_multipoles(F, e, org, poles=bad)
    for bad in (1, 3, 6, -2, 2.5):
        with pytest.raises(ValueError, match='orders'):
            multipole_field(F, bad, org)
    for bad in ((0., 0.), (0., 0., 0., 0.), (0., numpy.nan, 0.), (0., 0., numpy.inf), 1.0, 'here', None):
        with pytest.raises(ValueError, match='origin'):
            survey_multipoles(F, e, bad)
        with pytest.raises(ValueError, match='origin'):
            multipole_field(F, 2, bad)
    for other in (ParticleMesh([8, 8, 16], BoxSize=100.).create(type='real'),
                  ParticleMesh([8, 8, 8], BoxSize=[100., 100., 50.]).create(type='real')):
        with pytest.raises(ValueError, match='mesh'):
            survey_multipoles(F, e, org, other=other)
    with pytest.raises(ValueError):
        survey_multipoles(F, e, org, other=ParticleMesh([8, 8, 8], BoxSize=100., dtype='f4').create(type='real'))
    with pytest.raises(ValueError, match='kedges'):
        survey_multipoles(F, [0.3, 0.1], org)
    with pytest.raises(ValueError, match='out'):
        multipole_field(F, 2, org, out=ParticleMesh([8, 8, 16], BoxSize=100.).create(type='complex'))
    with pytest.raises(ValueError, match='real mesh'):
        multipole_field(ParticleMesh([8, 8, 8], BoxSize=100., dtype='c16').create(type='real'), 2, org)
    assert isinstance(F, RealField)


# ---- 8. resources (compiles for gfx950 on the CPU) -----------------------------------------------------------------

def test_survey_kernels_compile_without_scratch():
    import os
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_survey.hip')
    # ylm_weight_kernel<T> for f4 / f8, ylm_accumulate_kernel<T, BETA> for f4 / f8 and beta 0 / 1
    kernels = {k: v for k, v in t.items() if 'ylm_weight_kernel' in k or 'ylm_accumulate_kernel' in k}
    assert len(kernels) == 6, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)
