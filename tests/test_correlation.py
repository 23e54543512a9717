"""pmesh_amd.correlation (csrc/pmx_corr.hip) against a numpy restatement of its definition and against known answers.

The restatement builds the separations of a block as pm._block_coords does on the real side (the signed index times
L / N, what RealField.x of an f8 mesh holds), |r| and mu in the stated order of additions, numpy.digitize and Legendre
polynomials from numpy.polynomial.legendre, and sums every bin in extended precision, so that the bound on a sum
covers the kernel's rounding alone.  Under -m "not gpu" it serves pmx_corr_project, pmx_corr_vjp and
pmx_spectral_product (CorrOracleBackend), so the host layer — argument handling, the scratch spectrum, the in-place
transform, the sum over ranks before the division — runs without a GPU; under -m gpu the kernels are compared with it.
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
from pmesh_amd.correlation import CorrResult, bin_real, correlation_field, correlation_function
from pmesh_amd.pm import ParticleMesh, RealField, TransposedComplexField, UntransposedComplexField
from pmesh_amd.transfer import Transfer
from tests.test_interlace import BLOCKS, InterlaceOracleBackend, window_of
from tests.test_lpt import FORMS, _block, _nan_block, cpu
from tests.test_power import density

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53            # 1.1e-16: half a unit in the last place of a double
SUM_BOUND = 2 * 2.3e-16     # two summations in different orders, per unit of sum |x| of a bin


# ---- the restatement -----------------------------------------------------------------------------------------------

def separations(start, shape, nmesh, box, los=None):
    """|r| and mu of every cell of a block, in the arithmetic of the definition"""
    nd = len(shape)
    box = numpy.ones(nd) * numpy.asarray(box, dtype='f8')
    r, _ = _pm._block_coords([int(s) for s in start], tuple(int(s) for s in shape), [int(n) for n in nmesh],
                             [float(b) for b in box], 'f8', 'cpu', False)
    r = [x.numpy() for x in r]
    if los is None:
        los = [0.0] * (nd - 1) + [1.0]
    r2, rl = 0, 0
    for rd, ld in zip(r, los):
        r2 = r2 + rd * rd
        rl = rl + rd * float(ld)
    shape = tuple(int(s) for s in shape)
    rmag = numpy.broadcast_to(numpy.sqrt(r2), shape)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        mu = numpy.where(rmag > 0, numpy.broadcast_to(rl, shape) / rmag, 0.0)
    return rmag, mu


def unit(los):
    return None if los is None else numpy.asarray(los, dtype='f8') / numpy.sqrt(numpy.sum(numpy.square(los)))


def bin_sums(keys, w, n):
    """sum of w per key in 0..n-1, every bin summed on its own in extended precision (rounded to double once)"""
    out = numpy.zeros(n)
    if len(keys) == 0:
        return out
    order = numpy.argsort(keys, kind='stable')
    k = keys[order]
    first = numpy.flatnonzero(numpy.concatenate([[True], k[1:] != k[:-1]]))
    out[k[first]] = numpy.add.reduceat(w[order].astype(numpy.longdouble), first).astype('f8')
    return out


def mu_bins(mu, me):
    mb = numpy.digitize(mu, me) - 1
    mb[mu == me[-1]] = len(me) - 2
    return mb


def chain_bound(shape):
    """the |r| and mu sums are sums of one sign, for which the issue sets no bound: the kernel adds a bin's terms in a
    chain of at most 64 (a thread's run) + 256 (the LDS adds of a tile) + ntiles (the global adds) additions, each
    rounding by at most EPS of the sum; ntiles at most prod ceil(n / 16)"""
    return (64 + 256 + int(numpy.prod([(int(n) + 15) // 16 for n in shape]))) * EPS


def ref_project(x, start, nmesh, box, redges, muedges=None, los=None, ells=(), volume=1.0):
    """pmx_corr_project on one block: the accumulator vector and, in the same layout, the bound on the difference of
    the kernel's (0 for the counts: equal exactly)"""
    x = numpy.asarray(x).astype('f8')
    redges = numpy.asarray(redges, dtype='f8')
    nr = len(redges) - 1
    rmag, mu = separations(start, x.shape, nmesh, box, los)
    rb = numpy.digitize(rmag, redges) - 1
    ok = (rb >= 0) & (rb < nr)
    rb, rmag, mu, v = rb[ok], rmag[ok], mu[ok], volume * x[ok]
    s1 = 3 + len(ells)
    nmu = 0 if muedges is None else len(muedges) - 1
    acc = numpy.zeros(nr * s1 + nr * nmu * 4)
    bound = numpy.zeros_like(acc)
    t1, b1 = acc[:nr * s1].reshape(nr, s1), bound[:nr * s1].reshape(nr, s1)
    chain = chain_bound(x.shape)
    t1[:, 0] = numpy.bincount(rb, minlength=nr)
    t1[:, 1] = bin_sums(rb, rmag, nr)
    t1[:, 2] = bin_sums(rb, v, nr)
    absv = bin_sums(rb, numpy.abs(v), nr)
    b1[:, 1] = chain * t1[:, 1]
    b1[:, 2] = SUM_BOUND * absv
    for p, ell in enumerate(ells):
        t1[:, 3 + p] = bin_sums(rb, v * legendre.legval(mu, [0] * ell + [1]), nr)
        b1[:, 3 + p] = (2 * ell + 1) * SUM_BOUND * absv
    if nmu:
        me = numpy.asarray(muedges, dtype='f8')
        mb = mu_bins(mu, me)
        good = (mb >= 0) & (mb < nmu)
        flat = rb[good] * nmu + mb[good]
        t2, b2 = acc[nr * s1:].reshape(nr * nmu, 4), bound[nr * s1:].reshape(nr * nmu, 4)
        t2[:, 0] = numpy.bincount(flat, minlength=nr * nmu)
        t2[:, 1] = bin_sums(flat, rmag[good], nr * nmu)
        t2[:, 2] = bin_sums(flat, mu[good], nr * nmu)
        t2[:, 3] = bin_sums(flat, v[good], nr * nmu)
        b2[:, 1] = chain * t2[:, 1]
        b2[:, 2] = chain * bin_sums(flat, numpy.abs(mu[good]), nr * nmu)
        b2[:, 3] = SUM_BOUND * bin_sums(flat, numpy.abs(v[good]), nr * nmu)
    return acc, bound


def ref_vjp(shape, start, nmesh, box, redges, coef, muedges=None, los=None, ells=(), volume=1.0):
    """pmx_corr_vjp on one block: the value of every cell, the bound on the kernel's difference, and the cells outside
    the edges.  The bound: 8 EPS of the sum of the |terms| for the products and additions, and per pole of order l
    12 EPS l^2 |c|: each of the l - 1 steps of the recurrence (n + 1) L_{n+1} = (2n + 1) mu L_n - n L_{n-1} rounds three
    times on terms of at most 3 in all (12 EPS, with as much again for legval's Clenshaw sum), and an error made at step
    k reaches L_l multiplied by a solution of the same recurrence that starts from 1 at k and grows at most linearly
    inside [-1, 1], so the steps add up to at most l^2 / 2 of them twice"""
    redges = numpy.asarray(redges, dtype='f8')
    nr = len(redges) - 1
    nmu = 0 if muedges is None else len(muedges) - 1
    sc = 1 + len(ells)
    rmag, mu = separations(start, shape, nmesh, box, los)
    rb = numpy.digitize(rmag, redges) - 1
    ok = (rb >= 0) & (rb < nr)
    j = numpy.where(ok, rb, 0)
    c1 = coef[:nr * sc].reshape(nr, sc)
    f = c1[j, 0]
    mag, leg = numpy.abs(f), 0.0
    for p, ell in enumerate(ells):
        term = c1[j, 1 + p] * legendre.legval(mu, [0] * ell + [1])
        f = f + term
        mag = mag + numpy.abs(c1[j, 1 + p])
        leg = leg + 12 * EPS * ell * ell * numpy.abs(c1[j, 1 + p])
    if nmu:
        me = numpy.asarray(muedges, dtype='f8')
        mb = mu_bins(mu, me)
        good = (mb >= 0) & (mb < nmu)
        c2 = coef[nr * sc:].reshape(nr, nmu)[j, numpy.where(good, mb, 0)]
        f = f + numpy.where(good, c2, 0.0)
        mag = mag + numpy.where(good, numpy.abs(c2), 0.0)
    f = numpy.where(ok, volume * f, 0.0)
    return f, numpy.where(ok, abs(volume) * (8 * EPS * mag + leg), 0.0), ~ok


def ref_product(x, y, out, start, nmesh, scale, conj_y, accumulate, p):
    """pmx_spectral_product: [out +] scale x (conj) y / prod_d sinc(w_d / 2)^p"""
    x, y = numpy.asarray(x).astype('c16'), numpy.asarray(y).astype('c16')
    r = scale * (x * (numpy.conj(y) if conj_y else y)) / window_of(start, x.shape, nmesh, p)
    return r + numpy.asarray(out).astype('c16') if accumulate else r


class CorrOracleBackend(InterlaceOracleBackend):
    """the CPU test double with the three entries of csrc/pmx_corr.hip served by the restatement"""
    name = 'oracle-corr'

    @staticmethod
    def _options(params, nd, muedges):
        return dict(muedges=None if muedges is None else muedges.numpy(), los=list(params.los)[:nd],
                    ells=list(params.poles)[:params.npoles], volume=params.volume)

    def corr_project(self, params, x, start, nmesh, boxsize, redges, muedges, acc):
        if x.numel() == 0:
            return
        assert params.hermitian == 0 and params.deconv_pow == 0
        r, _ = ref_project(x.numpy(), start, nmesh, boxsize, redges.numpy(), **self._options(params, x.dim(), muedges))
        acc += torch.from_numpy(r)

    def corr_vjp(self, params, g, start, nmesh, boxsize, redges, muedges, coef):
        if g.numel() == 0:
            return
        f, _, _ = ref_vjp(tuple(g.shape), start, nmesh, boxsize, redges.numpy(), coef.numpy(),
                          **self._options(params, g.dim(), muedges))
        g.copy_(torch.from_numpy(f))

    def spectral_product(self, x, y, out, start, nmesh, scale=1.0, conj_y=False, accumulate=False, deconv_pow=0):
        if x.numel() == 0:
            return
        out.copy_(torch.from_numpy(ref_product(x.numpy(), y.numpy(), out.numpy().copy(), start, nmesh, scale, conj_y,
                                               accumulate, deconv_pow)))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def cbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(CorrOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def params_of(nr, muedges, los, ells, nd, volume=1.0):
    p = _abi.Power()
    p.nk = nr
    p.nmu = 0 if muedges is None else len(muedges) - 1
    p.npoles = len(ells)
    for i, ell in enumerate(ells):
        p.poles[i] = ell
    p.volume = volume
    los = unit(los) if los is not None else [0.0] * (nd - 1) + [1.0]
    for d in range(nd):
        p.los[d] = float(los[d])
    return p


def dev(a, be):
    return None if a is None else torch.from_numpy(numpy.asarray(a, dtype='f8')).to(be.device)


def assert_sums(got, want, bound, what=''):
    """counts (bound 0) equal exactly, every other sum within its bound"""
    err = numpy.abs(got - want)
    bad = numpy.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]], bound[bad[:5]])


def expected(field, redges, muedges=None, los=None, poles=()):
    """the restatement's CorrResult of a one-rank RealField, and the bound on its raw sums"""
    pm = field.pm
    acc, bound = ref_project(cpu(field.value), field.start, pm.Nmesh, pm.BoxSize, redges, muedges, unit(los), list(poles))
    me = None if muedges is None else numpy.asarray(muedges, 'f8')
    return CorrResult(numpy.asarray(redges, 'f8'), me, acc, list(poles)), bound


def assert_result(got, want, bound, slack=0.0):
    """a CorrResult against the restatement's: counts equal, the NaN bins exactly the restatement's empty bins and at
    least half of the bins populated, every value within the bound on its raw sum (plus `slack` per cell)"""
    nr, ells = len(want.modes), sorted(want.poles)
    s1 = 3 + len(ells)
    b1 = bound[:nr * s1].reshape(nr, s1)
    assert (got.modes == want.modes).all()
    empty = want.modes == 0
    assert 2 * (~empty).sum() >= nr
    n = want.modes[~empty]

    def close(x, y, b, scale=1.0):
        assert (numpy.isnan(x) == empty).all()
        err = numpy.abs(x[~empty] - y[~empty]) * n
        assert (err <= scale * (b[~empty] + slack * n)).all(), (err.max(), b.max())
    close(got.r, want.r, b1[:, 1])
    close(got.corr, want.corr, b1[:, 2])
    assert sorted(got.poles) == ells
    for ell in ells:
        # (poles is listed in the caller's order in the raw sums; the bound of every pole column is (2l + 1) that of x)
        close(got.poles[ell], want.poles[ell], (2 * ell + 1) * b1[:, 2], 2 * ell + 1)
    if want.corr2d is None:
        assert got.corr2d is None
        return
    nmu = want.modes2d.shape[1]
    b2 = bound[nr * s1:].reshape(nr, nmu, 4)
    assert (got.modes2d == want.modes2d).all()
    e2 = want.modes2d == 0
    n2 = want.modes2d[~e2]
    for x, y, col in ((got.r2d, want.r2d, 1), (got.mu2d, want.mu2d, 2), (got.corr2d, want.corr2d, 3)):
        assert (numpy.isnan(x) == e2).all()
        assert (numpy.abs(x[~e2] - y[~e2]) * n2 <= b2[..., col][~e2] + (slack * n2 if col == 3 else 0)).all()


# ---- 1. pmx_corr_project against the restatement (GPU) -------------------------------------------------------------

def rmax_of(nmesh, box, nd):
    box = numpy.ones(nd) * numpy.asarray(box, dtype='f8')
    return float(numpy.sqrt(((box / 2) ** 2).sum()))


def uniform_edges(nmesh, box):
    """arange(0, rmax + H, H), H = L / N: many cells sit exactly on edges"""
    nd = len(nmesh)
    H = float((numpy.ones(nd) * numpy.asarray(box, dtype='f8'))[0]) / int(nmesh[0])
    return numpy.arange(0, rmax_of(nmesh, box, nd) + H, H)


def geometric_edges(nmesh, box):
    """leaves r = 0 and the far corners outside"""
    nd = len(nmesh)
    H = float((numpy.ones(nd) * numpy.asarray(box, dtype='f8'))[0]) / int(nmesh[0])
    return numpy.geomspace(0.9 * H, 0.8 * rmax_of(nmesh, box, nd), 12)


MU7 = numpy.array([-1, -0.7, -0.2, 0, 0.1, 0.5, 0.9, 1.0])
MU64 = numpy.linspace(-1, 1, 65)
LOS = [0.3, -1, 2]
# (edges, muedges, los, poles)
OPTIONS = [(uniform_edges, None, None, ()),
           (geometric_edges, MU7, LOS, (0, 2, 4)),
           (uniform_edges, MU64, None, (0, 1, 2, 4)),
           (geometric_edges, None, LOS, (3, 8)),
           (uniform_edges, MU7, None, ())]

# (shape, start, nmesh, box): whole meshes — no extent a multiple of the 16 x 16 x 64 tile and every axis crossing
# N // 2 inside a tile; odd N; an anisotropic box; 2-d; 1-d — and blocks at a nonzero start inside a larger mesh, every
# axis crossing N // 2 (a larger one and the half-spectrum blocks of test_interlace)
MESHES = [([20, 18, 70], [0, 0, 0], [20, 18, 70], 50.),
          ([9, 45, 33], [0, 0, 0], [9, 45, 33], [30., 40., 50.]),
          ([32, 48, 64], [0, 0, 0], [32, 48, 64], [100., 120., 200.]),
          ([33, 40], [0, 0], [33, 40], 10.),
          ([64], [0], [64], 80.)]
OFFSET = [([20, 18, 70], [25, 10, 90], [64, 36, 256], [100., 90., 300.])] + \
         [(shape, start, nmesh, [40., 30., 50.]) for shape, start, nmesh in BLOCKS[:2]]


def project_case(be, rng, geom, dtype, form, option):
    shape, start, nmesh, box = geom
    nd = len(shape)
    edges, me, los, ells = option
    e = edges(nmesh, box)
    x = _block(shape, dtype, form, rng, complex_=False)
    before = cpu(x).copy()
    p = params_of(len(e) - 1, me, los[:nd] if los else None, ells, nd, volume=1.5)
    acc = torch.zeros(p.nk * (3 + len(ells)) + p.nk * p.nmu * 4, dtype=torch.float64, device=be.device)
    be.corr_project(p, x, start, nmesh, numpy.ones(nd) * box, dev(e, be), dev(me, be), acc)
    assert (cpu(x) == before).all()
    want, bound = ref_project(before, start, nmesh, box, e, me, unit(los[:nd]) if los else None, ells, 1.5)
    assert want[0::3 + len(ells)][:p.nk].sum() > 0
    assert_sums(cpu(acc), want, bound, (geom, dtype, form, option[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_project_kernel(hipbe, dtype, form):
    """every mesh and block with every option, in every memory form: C order, axes swapped in memory (a transposed
    view), a padded last axis, every other element of a larger array"""
    rng = numpy.random.RandomState(41)
    for geom in MESHES + OFFSET:
        for option in OPTIONS:
            project_case(hipbe, rng, geom, dtype, form, option)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_project_kernel_128(hipbe, dtype):
    """128^3 with uniform edges: 8 x 8 x 2 tiles add into every bin"""
    rng = numpy.random.RandomState(42)
    project_case(hipbe, rng, ([128, 128, 128], [0, 0, 0], [128, 128, 128], 1000.), dtype, 'C', OPTIONS[0])


@pytest.mark.gpu
def test_project_kernel_fine_edges_take_several_windows(hipbe):
    """20001 edges on 64^3, far narrower than a tile's |r| range: the tile is read once per window of bins.  Raw sums,
    so no bin is skipped; then the same number of edges laid through the distinct separations of an anisotropic box,
    where every bin is populated, through the host layer"""
    rng = numpy.random.RandomState(43)
    geom = ([64, 64, 64], [0, 0, 0], [64, 64, 64], 100.)

    def fine(nmesh, box):
        return numpy.linspace(0, rmax_of(nmesh, box, 3), 20001)

    def coarser(nmesh, box):
        return fine(nmesh, box)[::8]
    project_case(hipbe, rng, geom, 'f8', 'C', (fine, None, None, ()))
    project_case(hipbe, rng, geom, 'f8', 'C', (coarser, numpy.linspace(-1, 1, 11), None, (0, 2, 4)))
    pm = ParticleMesh([64, 64, 64], BoxSize=[100., 117.3, 131.9])
    f = density(pm, seed=3)
    radii = numpy.unique(separations([0, 0, 0], [64, 64, 64], pm.Nmesh, pm.BoxSize)[0])
    e = radii[numpy.linspace(0, len(radii) - 1, 20001).astype(int)]
    want, bound = expected(f, e)
    assert (want.modes > 0).all()
    assert_result(bin_real(f, e), want, bound)


# ---- 2. pmx_spectral_product against the restatement (GPU) ---------------------------------------------------------

def product_bound(x, y, out, scale, accumulate, comp):
    """the form of test_interlace.bound_f8: one complex multiply-add and one division, each a few 1e-16 of the
    operands: 1e-14 * max(|scale x y| / min |comp| + |out|)"""
    big = (abs(scale) * numpy.abs(x) * numpy.abs(y)).max() / numpy.abs(comp).min()
    return 1e-14 * (big + (numpy.abs(out).max() if accumulate else 0.0))


def assert_within(got, want, tol8, single):
    """the f8 bound; in single precision one rounding of the result to float more, 6e-8 |want|"""
    got, want = numpy.asarray(got).astype('c16'), numpy.asarray(want)
    assert numpy.isfinite(got.real).all() and numpy.isfinite(got.imag).all()
    err = numpy.abs(got - want)
    assert (err <= tol8 + (6e-8 * numpy.abs(want) if single else 0.0)).all(), (err.max(), tol8)


@pytest.mark.gpu
@pytest.mark.parametrize('form_out', FORMS)
@pytest.mark.parametrize('form_in', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
def test_product_kernel(hipbe, cdt, form_in, form_out):
    """the half-spectrum blocks of test_interlace, deconv_pow 0, 2, 3, every flag combination; out-of-place into NaN
    memory (or onto values when accumulating), in place on x and on y"""
    rng = numpy.random.RandomState(51)
    for shape, start, nmesh in BLOCKS:
        for p in (0, 2, 3):
            comp = window_of(start, shape, nmesh, p)
            for conj_y in (False, True):
                for accumulate in (False, True):
                    x = _block(shape, cdt, form_in, rng)
                    y = _block(shape, cdt, form_out, rng)
                    out = (_block if accumulate else _nan_block)(shape, cdt, form_out, rng)
                    xv, yv, ov = cpu(x).copy(), cpu(y).copy(), cpu(out).copy()
                    for target, scale in ((out, 0.75), (x, -1.25), (y, 1.0)):
                        prev = cpu(target).copy() if accumulate else ov
                        want = ref_product(cpu(x), cpu(y), prev, start, nmesh, scale, conj_y, accumulate, p)
                        tol = product_bound(cpu(x), cpu(y), prev, scale, accumulate, comp)
                        hipbe.spectral_product(x, y, target, start, nmesh, scale, conj_y, accumulate, p)
                        assert_within(cpu(target), want, tol, cdt == 'c8')
                        if target is out:
                            assert (cpu(x) == xv).all() and (cpu(y) == yv).all()


@pytest.mark.gpu
def test_product_kernel_refuses_what_it_does_not_do(hipbe):
    from pmesh_amd.backend import _byte_strides
    rng = numpy.random.RandomState(52)
    x = _block([4, 4, 3], 'c16', 'C', rng)
    y = _block([4, 4, 3], 'c16', 'C', rng)
    o = _block([4, 4, 3], 'c16', 'C', rng)
    before = cpu(o).copy()

    def raw(ndim=3, elsize=8, x_=None, y_=None, out=None, pow_=0, strides=True, geom=True, out_strides=None):
        args = [ndim, elsize, x.data_ptr() if x_ is None else x_, _byte_strides(x) if strides else None,
                y.data_ptr() if y_ is None else y_, _byte_strides(y) if strides else None,
                o.data_ptr() if out is None else out,
                (_byte_strides(o) if out_strides is None else out_strides) if strides else None]
        args += [_abi.i64arr([4, 4, 3], 3), _abi.i64arr([0] * 3, 3), _abi.i64arr([4, 4, 4], 3)] if geom else [None] * 3
        args += [1.0, 1, 0, pow_, hipbe.stream()]
        with pytest.raises(backend.PmxError) as e:
            hipbe.call('spectral_product', *args)
        return e.value.code

    # partial overlap with x or with y: a block that starts inside the other, or the same start with other strides
    assert raw(out=x.data_ptr() + 16 * 5) == _abi.PMX_EINVAL
    assert raw(out=y.data_ptr() + 16) == _abi.PMX_EINVAL
    assert raw(out=x.data_ptr(), out_strides=_abi.i64arr([16, 64, 256], 3)) == _abi.PMX_EINVAL
    assert raw(elsize=2) == _abi.PMX_EINVAL
    assert raw(ndim=4) == _abi.PMX_EINVAL
    assert raw(ndim=0) == _abi.PMX_EINVAL
    assert raw(pow_=-1) == _abi.PMX_EINVAL
    assert raw(x_=0) == _abi.PMX_EINVAL
    assert raw(y_=0) == _abi.PMX_EINVAL
    assert raw(out=0) == _abi.PMX_EINVAL
    assert raw(strides=False) == _abi.PMX_EINVAL
    assert raw(geom=False) == _abi.PMX_EINVAL
    assert (cpu(o) == before).all()


@pytest.mark.gpu
def test_project_kernel_refuses_what_it_does_not_do(hipbe):
    rng = numpy.random.RandomState(53)
    x = _block([8, 8, 8], 'f8', 'C', rng, complex_=False)
    e = dev([0., 1., 2.], hipbe)
    acc = torch.zeros(8, dtype=torch.float64, device=hipbe.device)
    for field, value in (('hermitian', 1), ('deconv_pow', 2), ('nk', 0), ('nmu', -1)):
        p = params_of(2, None, None, (), 3)
        setattr(p, field, value)
        with pytest.raises(backend.PmxError) as err:
            hipbe.corr_project(p, x, [0] * 3, [8] * 3, [1.] * 3, e, None, acc)
        assert err.value.code == _abi.PMX_EINVAL
        with pytest.raises(backend.PmxError) as err:
            hipbe.corr_vjp(p, x, [0] * 3, [8] * 3, [1.] * 3, e, None, acc)
        assert err.value.code == _abi.PMX_EINVAL
    p = params_of(2, None, None, (), 3)
    p.nmu = 3                                   # mu bins without muedges
    with pytest.raises(backend.PmxError) as err:
        hipbe.corr_project(p, x, [0] * 3, [8] * 3, [1.] * 3, e, None, acc)
    assert err.value.code == _abi.PMX_EINVAL
    p = params_of(2, None, None, (), 3)
    p.npoles = _abi.PMX_POWER_MAX_POLES + 1
    with pytest.raises(backend.PmxError) as err:
        hipbe.corr_project(p, x, [0] * 3, [8] * 3, [1.] * 3, e, None, acc)
    assert err.value.code == _abi.PMX_EUNSUPPORTED
    assert (cpu(acc) == 0).all()


# ---- 3. pmx_corr_vjp against the restatement (GPU) -----------------------------------------------------------------

def vjp_case(be, rng, geom, dtype, form, option):
    shape, start, nmesh, box = geom
    nd = len(shape)
    edges, me, los, ells = option
    e = edges(nmesh, box)
    nr, nmu = len(e) - 1, 0 if me is None else len(me) - 1
    coef = rng.normal(size=nr * (1 + len(ells)) + nr * nmu)
    g = _nan_block(shape, dtype, form, rng, complex_=False)
    p = params_of(nr, me, los[:nd] if los else None, ells, nd, volume=1.5)
    be.corr_vjp(p, g, start, nmesh, numpy.ones(nd) * box, dev(e, be), dev(me, be), dev(coef, be))
    want, bound, outside = ref_vjp(shape, start, nmesh, box, e, coef, me, unit(los[:nd]) if los else None, ells, 1.5)
    got = cpu(g).astype('f8')
    assert numpy.isfinite(got).all()
    assert (got[outside] == 0).all()
    if dtype == 'f4':
        bound = bound + 6e-8 * numpy.abs(want)
    assert (numpy.abs(got - want) <= bound).all(), (geom, dtype, form, numpy.abs(got - want).max())
    return outside


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_vjp_kernel(hipbe, dtype, form):
    """every cell of every mesh and block of item 1 into NaN memory; cells outside the edges exactly 0"""
    rng = numpy.random.RandomState(61)
    some_outside = False
    for geom in MESHES + OFFSET:
        for option in OPTIONS:
            some_outside |= bool(vjp_case(hipbe, rng, geom, dtype, form, option).any())
    assert some_outside


@pytest.mark.gpu
def test_vjp_kernel_fine_edges_take_several_windows(hipbe):
    """a tile takes one pass per window of coefficient rows and every cell is written by exactly one of them; then
    edges that start above and end below the separations of whole tiles: those tiles are zero"""
    rng = numpy.random.RandomState(62)
    geom = ([64, 64, 64], [0, 0, 0], [64, 64, 64], 100.)
    vjp_case(hipbe, rng, geom, 'f8', 'C', (lambda n, b: numpy.linspace(0, rmax_of(n, b, 3), 20001), None, None, ()))
    vjp_case(hipbe, rng, geom, 'f8', 'C', (lambda n, b: numpy.linspace(0, rmax_of(n, b, 3), 2501),
                                            numpy.linspace(-1, 1, 11), None, (0, 2, 4)))
    outside = vjp_case(hipbe, rng, geom, 'f8', 'C', (lambda n, b: numpy.linspace(30., 45., 5001), None, None, ()))
    assert outside.any() and not outside.all()


# ---- 4. invariants (GPU) -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('Nmesh', [[32, 32, 32], [32, 24], [64]])
def test_invariants(hipbe, Nmesh):
    pm = ParticleMesh(Nmesh, BoxSize=80.)
    f = density(pm, seed=9)
    c = f.r2c()
    H = 80. / Nmesh[0]
    e = numpy.arange(0, rmax_of(Nmesh, 80., len(Nmesh)) + 2 * H, H)
    me = numpy.linspace(-1, 1, 7)
    res = correlation_function(c, e, muedges=me, poles=(0, 2))
    # edges covering every cell: all prod(N) cells counted
    assert res.modes.sum() == numpy.prod(Nmesh)
    # the (r, mu) table summed over mu is the r table
    assert (res.modes2d.sum(axis=1) == res.modes).all()
    w2 = numpy.nansum(res.modes2d * res.corr2d, axis=1)
    numpy.testing.assert_allclose(w2, numpy.nan_to_num(res.modes * res.corr), rtol=1e-12,
                                  atol=1e-12 * numpy.nanmax(numpy.abs(res.corr)) * res.modes.max())
    # xi_0 == xi; auto == cross with itself
    numpy.testing.assert_allclose(res.poles[0], res.corr, rtol=1e-12, equal_nan=True)
    cross = correlation_function(c, e, other=c, muedges=me, poles=(0, 2))
    assert (cross.modes == res.modes).all() and (cross.modes2d == res.modes2d).all()
    scale = numpy.nanmax(numpy.abs(res.corr))
    numpy.testing.assert_allclose(cross.corr, res.corr, rtol=1e-12, atol=1e-12 * scale, equal_nan=True)
    numpy.testing.assert_allclose(cross.corr2d, res.corr2d, rtol=1e-12, atol=1e-12 * scale, equal_nan=True)
    numpy.testing.assert_allclose(cross.poles[2], res.poles[2], rtol=1e-12, atol=5e-12 * scale, equal_nan=True)
    # Parseval: the cell at r = 0 is the sum of |a|^2 over every mode
    zero = correlation_function(c, [0, H / 2])
    assert zero.modes[0] == 1
    assert abs(zero.corr[0] - c.cnorm()) <= 1e-12 * c.cnorm()
    # deconv_pow = 2p equals correlating the field compensated by p
    d = correlation_function(c, e, deconv_pow=4)
    d2 = correlation_function(c.apply(Transfer(deconv_pow=2)), e)
    assert (d.modes == d2.modes).all()
    numpy.testing.assert_allclose(d.corr, d2.corr, rtol=1e-12, atol=1e-12 * numpy.nanmax(numpy.abs(d2.corr)),
                                  equal_nan=True)


# ---- 5. known answers (both backends) ------------------------------------------------------------------------------

KNOWN = (16, 24, 32)
# the transform bound of tests/test_fft_kernels.py: 2e-15 * log2(n) of the largest value per 1-d pass of length n, so
# 2e-15 * (log2 16 + log2 24 + log2 32) = 2.72e-14 for one 3-d transform of these lengths; three times over (r2c, the
# product, c2r): 8.2e-14 of max |xi|
KNOWN_TOL = 3 * 2e-15 * sum(numpy.log2(n) for n in KNOWN)


def test_plane_wave(cbe):
    """delta = A cos(2 pi m.x / L + phi): xi = A^2 / 2 cos(k.r) cell by cell within KNOWN_TOL * A^2 / 2 (8.2e-14: see
    KNOWN_TOL), and correlation_function equals the restatement's binning of that analytic mesh (the bound of the
    sums plus KNOWN_TOL * A^2 / 2 per cell)"""
    box = numpy.array([100., 80., 120.])
    pm = ParticleMesh(KNOWN, BoxSize=box, dtype='f8')
    A, phi, m = 1.7, 0.4, numpy.array([1, -2, 3])
    f = pm.create(type='real')
    idx = numpy.meshgrid(*[numpy.arange(n) for n in KNOWN], indexing='ij')
    phase = 2 * numpy.pi * sum(mi * i / float(n) for mi, i, n in zip(m, idx, KNOWN))
    f.value[...] = torch.from_numpy(A * numpy.cos(phase + phi)).to(f.value.device)
    before = f.value.clone()
    analytic = A * A / 2 * numpy.cos(phase)           # periodic in every index: the signed separation gives the same
    tol = KNOWN_TOL * A * A / 2
    xi = correlation_field(f)
    assert isinstance(xi, RealField) and torch.equal(f.value, before)
    err = numpy.abs(cpu(xi.value) - analytic).max()
    print('plane wave: max error %.2e of the tolerance' % (err / tol))
    assert err <= tol
    e = numpy.arange(0, 90., 5.)
    me = numpy.linspace(-1, 1, 6)
    ref = pm.create(type='real')
    ref.value[...] = torch.from_numpy(analytic).to(ref.value.device)
    want, bound = expected(ref, e, muedges=me, los=[1, 1, 0.5], poles=(0, 2, 4))
    got = correlation_function(f, e, muedges=me, los=[1, 1, 0.5], poles=(0, 2, 4))
    assert_result(got, want, bound, slack=tol)
    assert torch.equal(f.value, before)


def test_power_law_noise_against_numpy_fft(cbe):
    """xi of a power-law noise field against numpy.fft in double: irfftn(|rfftn(f) / N|^2) * N, within
    KNOWN_TOL * max |xi| (8.2e-14 of it: see KNOWN_TOL); auto and cross, and through a caller's `out`"""
    pm = ParticleMesh(KNOWN, BoxSize=[100., 80., 120.], dtype='f8')
    f, h = density(pm, seed=4), density(pm, seed=5)
    N = float(numpy.prod(KNOWN))
    a, b = numpy.fft.rfftn(cpu(f.value)) / N, numpy.fft.rfftn(cpu(h.value)) / N
    for other, spec in ((None, a * numpy.conj(a)), (h, a * numpy.conj(b))):
        want = numpy.fft.irfftn(spec, s=KNOWN, axes=(0, 1, 2)) * N
        tol = KNOWN_TOL * numpy.abs(want).max()
        xi = correlation_field(f, other=other)
        err = numpy.abs(cpu(xi.value) - want).max()
        print('noise: max error %.2e of the tolerance' % (err / tol))
        assert err <= tol
        # from spectra, transposed and untransposed, into a field of the caller's; the spectra are left alone
        for T in (TransposedComplexField, UntransposedComplexField):
            ca = f.r2c(out=pm.create(type=T))
            cb = None if other is None else other.r2c(out=pm.create(type=T))
            before = ca.value.clone()
            out = pm.create(type='real')
            assert correlation_field(ca, other=cb, out=out) is out
            assert torch.equal(ca.value, before)
            assert numpy.abs(cpu(out.value) - want).max() <= tol
        e = numpy.arange(0, 90., 5.)
        ref = pm.create(type='real')
        ref.value[...] = torch.from_numpy(want).to(ref.value.device)
        res, bound = expected(ref, e, poles=(0, 2))
        assert_result(correlation_function(f, e, other=other, poles=(0, 2)), res, bound, slack=tol)


def test_f4_mesh_and_bin_real(cbe):
    """an f4 mesh: bin_real of the f4 xi equals the restatement's binning of the same values (loaded as float and
    widened), in 2 dimensions too; the padded view of the in-place transform is what is binned"""
    for nmesh, box in (((12, 10, 14), [40., 30., 50.]), ((12, 10), [40., 30.]), ((64,), 10.)):
        pm = ParticleMesh(nmesh, BoxSize=box, dtype='f4')
        xi = correlation_field(density(pm, seed=6))
        assert xi.value.dtype == torch.float32
        e = uniform_edges(nmesh, pm.BoxSize)
        me = MU7 if len(nmesh) > 1 else [-1, 0, 1]
        want, bound = expected(xi, e, muedges=me, poles=(0, 2))
        assert_result(bin_real(xi, e, muedges=me, poles=(0, 2)), want, bound)


# ---- 6. ranks ------------------------------------------------------------------------------------------------------

def ranks_case(comm=None, np_=None, Nmesh=(16, 16, 12)):
    kw = {} if comm is None else dict(comm=comm, np=np_)
    pm = ParticleMesh(list(Nmesh), BoxSize=100., **kw)
    f, h = density(pm, seed=5), density(pm, seed=6)
    e = numpy.arange(0, 100., 100. / Nmesh[0])
    return correlation_function(f, e, other=h.r2c(), muedges=numpy.linspace(0, 1, 4), poles=(0, 2), deconv_pow=2)


def compare_ranks(got, want, rtol=1e-11):
    """the form and tolerance of test_power._ranks_equal_one (assert_same with rtol 1e-11)"""
    assert (got.modes == want.modes).all() and (got.modes2d == want.modes2d).all()

    def close(x, y, scale=None):
        if scale is None:
            scale = numpy.nanmax(numpy.abs(y))
        numpy.testing.assert_allclose(x, y, rtol=rtol, atol=rtol * scale, equal_nan=True)
    close(got.r, want.r)
    close(got.corr, want.corr)
    close(got.r2d, want.r2d)
    close(got.mu2d, want.mu2d)
    close(got.corr2d, want.corr2d)
    for ell in want.poles:
        close(got.poles[ell], want.poles[ell], (2 * ell + 1) * numpy.nanmax(numpy.abs(want.corr)))


def _thread_ranks(size, np_, Nmesh):
    from tests import thread_comm
    results = {}

    def body(comm):
        results[comm.rank] = ranks_case(comm, np_, Nmesh)
    thread_comm.run_ranks(size, body)
    one = ranks_case(Nmesh=Nmesh)
    assert len(results) == size and one.modes.sum() > 0
    for r in results.values():
        compare_ranks(r, one)


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
def test_ranks_sum_then_divide(size, np_):
    """every rank gets the one-rank result: raw sums over the ranks first, then the division"""
    backend.reset()
    backend.use(CorrOracleBackend())
    try:
        _thread_ranks(size, np_, [16, 16, 12])
    finally:
        backend.reset()


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (8, [8]), (8, [2, 4])])
def test_kernel_ranks_equal_one(hipbe, size, np_):
    _thread_ranks(size, np_, [64, 64, 48])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gloo_ranks_equal_one():
    """the same, and the gradients, with one process per rank over gloo (tests/corr_mp_cases.py)"""
    env = dict(os.environ)
    env['OMP_NUM_THREADS'] = '1'
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()),
           os.path.join(ROOT, 'tests', 'corr_mp_cases.py')]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + '\n' + out.stderr[-6000:]
    assert 'ok correlation function on 2 ranks' in out.stdout
    assert 'ok correlation gradients on 2 ranks' in out.stdout


# ---- 8. argument errors (both backends) ----------------------------------------------------------------------------

def test_bad_arguments(cbe):
    pm = ParticleMesh([8, 8, 8], BoxSize=100.)
    f = density(pm, seed=1)
    c = f.r2c()
    before = f.value.clone()
    e = numpy.arange(0, 90., 12.5)
    for fn, x in ((correlation_function, f), (correlation_function, c), (bin_real, f)):
        for bad in ([1.0], [0.0, 0.0], [0.3, 0.1, 0.2], [0, numpy.nan], [[0, 1], [1, 2]]):
            with pytest.raises(ValueError, match='redges'):
                fn(x, bad)
        with pytest.raises(ValueError, match='muedges'):
            fn(x, e, muedges=[-1.5, 0, 1])
        with pytest.raises(ValueError, match='muedges'):
            fn(x, e, muedges=[0, 0.5, 0.5, 1])
        with pytest.raises(ValueError, match='PMX_POWER_MAX_MUBINS'):
            fn(x, e, muedges=numpy.linspace(-1, 1, _abi.PMX_POWER_MAX_MUBINS + 2))
        with pytest.raises(ValueError, match='PMX_POWER_MAX_KBINS'):
            fn(x, numpy.arange(_abi.PMX_POWER_MAX_KBINS + 2, dtype='f8'))
        with pytest.raises(ValueError, match='PMX_POWER_MAX_POLES'):
            fn(x, e, poles=(0, 1, 2, 3, 4, 5))
        for bad in ((9,), (0, 0), (-1,)):
            with pytest.raises(ValueError, match='poles'):
                fn(x, e, poles=bad)
        with pytest.raises(ValueError, match='los'):
            fn(x, e, los=[0, 0, 0])
        with pytest.raises(ValueError, match='los'):
            fn(x, e, los=[0, 1])
    with pytest.raises(ValueError, match='deconv_pow'):
        correlation_function(c, e, deconv_pow=-1)
    with pytest.raises(ValueError, match='deconv_pow'):
        correlation_field(c, deconv_pow=1.5)
    for fn in (lambda x: correlation_function(x, e), correlation_field, lambda x: bin_real(x, e)):
        with pytest.raises(TypeError):
            fn(numpy.zeros((8, 8, 5), 'c16'))
    with pytest.raises(TypeError):
        bin_real(c, e)
    # mismatched fields: another mesh, another layout, another dtype
    with pytest.raises(ValueError, match='mesh|layout'):
        correlation_function(c, e, other=ParticleMesh([8, 8, 16], BoxSize=100.).create(type='complex'))
    with pytest.raises(ValueError, match='layout'):
        correlation_function(c, e, other=pm.create(type=UntransposedComplexField))
    with pytest.raises(ValueError, match='layout'):
        correlation_function(c, e, other=ParticleMesh([8, 8, 8], BoxSize=100., dtype='f4').create(type='complex'))
    with pytest.raises(ValueError, match='out'):
        correlation_field(c, out=ParticleMesh([8, 8, 16], BoxSize=100.).create(type='real'))
    with pytest.raises(ValueError, match='out'):
        correlation_field(c, out=pm.create(type='complex'))
    # a complex-to-complex mesh is out of scope, as a RealField and as a spectrum
    pmc = ParticleMesh([8, 8, 8], BoxSize=100., dtype='c16')
    for x in (pmc.create(type='real'), pmc.create(type='complex')):
        with pytest.raises(ValueError, match='complex-to-complex'):
            correlation_function(x, e)
        with pytest.raises(ValueError, match='complex-to-complex'):
            correlation_field(x)
    with pytest.raises(ValueError, match='complex-to-complex'):
        bin_real(pmc.create(type='real'), e)
    with pytest.raises(NotImplementedError):
        correlation_function(ParticleMesh([4, 4, 4, 4], BoxSize=1.).create(type='complex'), [0, 1, 2])
    assert torch.equal(f.value, before)


def test_realfield_input_is_left_alone(cbe):
    pm = ParticleMesh([16, 12, 10], BoxSize=[40., 30., 50.])
    f, h = density(pm, seed=2), density(pm, seed=3)
    bf, bh = f.value.clone(), h.value.clone()
    e = numpy.arange(0, 36., 2.5)
    got = correlation_function(f, e, other=h, poles=(0, 2), deconv_pow=2)
    assert torch.equal(f.value, bf) and torch.equal(h.value, bh)
    # from the spectra: the same mesh xi, binned with float atomics in another order; both within the bound of the
    # restatement's binning of it
    same = correlation_function(f.r2c(), e, other=h.r2c(), poles=(0, 2), deconv_pow=2)
    want, bound = expected(correlation_field(f, other=h, deconv_pow=2), e, poles=(0, 2))
    assert_result(got, want, bound)
    assert_result(same, want, bound)


# ---- 9. resources (compiles for gfx950 on the CPU) -----------------------------------------------------------------

def test_corr_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_corr.hip')
    # corr_kernel / corr_vjp_kernel<T, MU, POLES> for f4 / f8, with and without the (r, mu) table and the multipoles;
    # product_kernel<T, CONJ, ACC, WIN> for f4 / f8 and every flag
    counts = {'corr_kernel': 8, 'corr_vjp_kernel': 8, 'product_kernel': 16}
    for key, n in counts.items():
        assert len([k for k in t if key in k]) == n, sorted(t)
    assert len(t) == sum(counts.values()), sorted(t)
    for name, r in t.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 168, (name, r)      # the bound of test_power.py: three or more waves per SIMD
        # waves per SIMD of <T, MU, POLES> without options / with the (r, mu) table or the multipoles / with both
        options = ('Lb1ELb' in name) + ('ELb1EEE' in name)
        if 'corr_kernel' in name:
            assert r['Occupancy'] >= (8, 5, 4)[options], (name, r)
        elif 'corr_vjp_kernel' in name:
            assert r['Occupancy'] >= (8, 7, 7)[options], (name, r)
