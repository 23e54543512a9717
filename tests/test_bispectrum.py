"""pmesh_amd.bispectrum: the binned bispectrum (csrc/pmx_bispec.hip) against a brute-force sum over mode pairs, a numpy
FFT restatement of the estimator, an analytic three-wave field and, at kernel level, numpy.einsum.

Wavenumbers in the restatements follow include/pmesh_amd.h (pmx_power_project): k_d = ((s_d (2 pi / N_d)) N_d) / L_d and
|k| = sqrt((k_0^2 + k_1^2) + k_2^2) in double, so a mode that sits on an edge lands on the same side here and in the
kernels.  Under -m "not gpu" the two entry points are served by numpy (BispecOracleBackend) and the host layer runs
without a GPU; under -m gpu the kernels are compared with the same references.

Bounds.  f8: |S - S_ref| <= 1e-13 sum_x |D_i D_j D_l| / N per triangle bin — double rounding over a few thousand cells
stays orders of magnitude below it (numpy's own FFT form is within 3.1e-16 of that scale on the brute-force mesh).
f4 (a complex64 field): F4_TOL of the same scale, twice the largest error that the composition out of the parts the
package had before — the complex64 c2r of masked copies of the spectrum and torch products in float64 — shows on the
parity meshes on the GPU (composition_error below returns it per case; `scripts/bispectrum_probe.py --f4-error` prints
the table, DESIGN 5.7 records the run).
"""
import itertools
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd import pm as _pm
from pmesh_amd.bispectrum import BispectrumResult, alias_bound, bispectrum, triangle_bins
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.power import power_spectrum
from tests.test_power import PowerOracleBackend, _sinc_pow, density

F8_TOL = 1e-13
# twice the composition's largest error / scale over the parity cases, measured on the GPU (see the module docstring)
F4_MEASURED = 1.131e-7
F4_TOL = 2 * F4_MEASURED


# ---- the CPU double ------------------------------------------------------------------------------------------------

def _shells_of(start, shape, nmesh, boxsize, kedges):
    """shell number (-1: outside) and the per-axis window factors of the modes of a block"""
    _, idx = _pm._block_coords(start, tuple(shape), nmesh, boxsize, 'f8', 'cpu', True)
    k2, w = None, []
    for d, ii in enumerate(idx):
        n, L = int(nmesh[d]), float(boxsize[d])
        s = ii.numpy().astype('f8')
        s = s - n * (ii.numpy() >= n // 2)
        wd = s * (2 * numpy.pi / n)
        kd = (wd * float(n)) / L
        k2 = kd * kd if k2 is None else k2 + kd * kd
        w.append(wd)
    kmag = numpy.broadcast_to(numpy.sqrt(k2), tuple(shape))
    sh = numpy.digitize(kmag, kedges) - 1
    sh[(sh < 0) | (sh >= len(kedges) - 1)] = -1
    return sh, w


class BispecOracleBackend(PowerOracleBackend):
    """the CPU test double with pmx_bispec_shells / pmx_bispec_reduce served by numpy"""
    name = 'oracle-bispec'

    def bispec_shells(self, a, outs, start, nmesh, boxsize, kedges, deconv_pow=0, unit=False):
        o = outs[0]
        if o.numel() == 0:
            return
        sh, w = _shells_of(start, o.shape, nmesh, boxsize, kedges.numpy())
        if unit:
            v = numpy.ones(tuple(o.shape), dtype='c16')
        else:
            v = a.numpy().astype('c16')
            if deconv_pow:
                for wd in w:
                    v = v / _sinc_pow(wd, deconv_pow)
        for s, out in enumerate(outs):
            out[...] = torch.from_numpy(numpy.where(sh == s, v, 0)).to(out.dtype)

    def bispec_reduce(self, fields, triangles, acc, work=None):
        if fields[0].numel() == 0 or len(triangles) == 0:
            return
        f = numpy.stack([x.numpy().astype('f8').reshape(-1) for x in fields])
        t = triangles.numpy()
        acc += torch.from_numpy(numpy.einsum('tx,tx,tx->t', f[t[:, 0]], f[t[:, 1]], f[t[:, 2]]))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def bbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(BispecOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- numpy restatements ---------------------------------------------------------------------------------------------

def mode_grid(Nmesh, BoxSize):
    """signed integer indices s (3, N0, N1, N2), |k| and the circular frequencies w_d of the full spectrum"""
    axes = []
    for n in Nmesh:
        i = numpy.arange(n)
        axes.append(i - n * (i >= n // 2))
    s = numpy.stack(numpy.meshgrid(*axes, indexing='ij'))
    w = [s[d].astype('f8') * (2 * numpy.pi / Nmesh[d]) for d in range(3)]
    k = [(w[d] * float(Nmesh[d])) / float(BoxSize[d]) for d in range(3)]
    return s, numpy.sqrt((k[0] * k[0] + k[1] * k[1]) + k[2] * k[2]), w


def shells_full(Nmesh, BoxSize, kedges):
    s, kmag, w = mode_grid(Nmesh, BoxSize)
    sh = numpy.digitize(kmag, kedges) - 1
    sh[(sh < 0) | (sh >= len(kedges) - 1)] = -1
    return s, sh, w


def full_spectrum(c):
    """the full (N0, N1, N2) complex128 spectrum of a one-rank ComplexField"""
    v = c.value.cpu().numpy().astype('c16')
    N = [int(n) for n in c.pm.Nmesh]
    if not c.compressed:
        return v
    return numpy.fft.fftn(numpy.fft.irfftn(v, s=N, axes=(0, 1, 2)))


def numpy_estimator(full, Nmesh, BoxSize, kedges, deconv_pow, tri):
    """S_t, C_t and the scale sum_x |D_i D_j D_l| / N of the module docstring of pmesh_amd.bispectrum, by numpy FFTs
    in double"""
    N = float(numpy.prod(Nmesh))
    _, sh, w = shells_full(Nmesh, BoxSize, kedges)
    v = full
    if deconv_pow:
        for wd in w:
            v = v / _sinc_pow(wd, deconv_pow)
    nb = len(kedges) - 1
    D = [(numpy.fft.ifftn(numpy.where(sh == i, v, 0)) * N).real for i in range(nb)]
    I = [(numpy.fft.ifftn(numpy.where(sh == i, 1.0, 0)) * N).real for i in range(nb)]
    S = numpy.array([(D[i] * D[j] * D[l]).sum() / N for i, j, l in tri])
    C = numpy.array([(I[i] * I[j] * I[l]).sum() / N for i, j, l in tri])
    scale = numpy.array([numpy.abs(D[i] * D[j] * D[l]).sum() / N for i, j, l in tri])
    return S, C, scale


def numpy_power(full, Nmesh, BoxSize, kedges, deconv_pow):
    """P_i = V <|a / W|^2> and the mean |k| over the modes of every shell of the full spectrum: the P(k) of the field
    whose shells numpy_estimator transforms (the amplitude divided by W = prod sinc^deconv_pow)"""
    _, kmag, w = mode_grid(Nmesh, BoxSize)
    _, sh, _ = shells_full(Nmesh, BoxSize, kedges)
    v = full
    if deconv_pow:
        for wd in w:
            v = v / _sinc_pow(wd, deconv_pow)
    p2 = float(numpy.prod(BoxSize)) * (v.real ** 2 + v.imag ** 2)
    nb = len(kedges) - 1
    with numpy.errstate(invalid='ignore', divide='ignore'):
        return (numpy.array([p2[sh == i].mean() for i in range(nb)]),
                numpy.array([kmag[sh == i].mean() for i in range(nb)]))


def assert_power_and_q(r, full, Nmesh, BoxSize, kedges, deconv_pow):
    """`power`, `k` and `Q` of a result against numpy's P of the deconvolved shells: sums of a few thousand positive
    terms in double agree to 1e-12 (the bound of tests/test_power.py); Q's denominator is three products of two such
    values, so 1e-11 covers it"""
    P, kmean = numpy_power(full, Nmesh, BoxSize, kedges, deconv_pow)
    numpy.testing.assert_allclose(r.power, P, rtol=1e-12)
    i, j, l = r.triangles.T
    numpy.testing.assert_allclose(r.k, kmean[r.triangles], rtol=1e-12)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        Q = r.B / (P[i] * P[j] + P[j] * P[l] + P[l] * P[i])
    assert numpy.isfinite(Q).sum() > 10
    numpy.testing.assert_allclose(r.Q, Q, rtol=1e-11, equal_nan=True)


def brute_force(full, Nmesh, BoxSize, kedges, nb):
    """S and C of EVERY triple of shells (nb, nb, nb), from a loop over all ordered pairs of modes inside the shells,
    the third mode from the integer indices: k3 = -(k1 + k2)"""
    s, sh, _ = shells_full(Nmesh, BoxSize, kedges)
    N = numpy.array(Nmesh)
    modes = [(tuple(s[:, a, b, c]), sh[a, b, c], full[a, b, c]) for a, b, c in zip(*numpy.nonzero(sh >= 0))]
    S = numpy.zeros((nb, nb, nb), dtype='c16')
    C = numpy.zeros((nb, nb, nb), dtype='i8')
    half = [(n // 2, (n - 1) // 2) for n in Nmesh]           # the signed indices run from -n // 2 to (n - 1) // 2
    for (s1, i, a1), (s2, j, a2) in itertools.product(modes, modes):
        s3 = [-(x + y) for x, y in zip(s1, s2)]
        if any(x < -lo or x > hi for x, (lo, hi) in zip(s3, half)):
            continue                                          # (no such mode: nothing wraps under the alias bound)
        p = tuple(numpy.mod(s3, N))
        l = sh[p]
        if l < 0:
            continue
        S[i, j, l] += a1 * a2 * full[p]
        C[i, j, l] += 1
    return S, C


def composition_sums(c, kedges, deconv_pow, tri):
    """the estimator's raw sums composed from what the package had before the kernels: a masked copy of the spectrum
    per shell (torch), the field's own c2r, torch products in float64"""
    pm = c.pm
    sh, w = _shells_of(c.start, c.value.shape, pm.Nmesh, pm.BoxSize, numpy.asarray(kedges))
    W = numpy.ones(tuple(c.value.shape))
    if deconv_pow:
        for wd in w:
            W = W * _sinc_pow(wd, deconv_pow)
    dev = c.value.device
    sht = torch.from_numpy(sh).to(dev)
    Wt = torch.from_numpy(W).to(dev).to(c.value.real.dtype)
    D = []
    for i in range(len(kedges) - 1):
        ci = pm.create(type=type(c))
        ci.value[...] = torch.where(sht == i, c.value / Wt, torch.zeros_like(c.value))
        r = ci.c2r().value
        D.append((r.real if r.is_complex() else r).double())
    N = float(numpy.prod(pm.Nmesh))
    return numpy.array([float((D[i] * D[j] * D[l]).sum()) / N for i, j, l in tri])


def composition_error(kind, Nmesh, BoxSize, deconv_pow):
    """max over the triangle bins of |composition - numpy f8| / scale for one complex64 parity case"""
    c, ke = parity_field(kind, Nmesh, BoxSize, 'f4')
    tri = triangle_bins(ke)
    S, _, scale = numpy_estimator(full_spectrum(c), Nmesh, BoxSize, ke, deconv_pow, tri)
    got = composition_sums(c, ke, deconv_pow, tri)
    return float(numpy.max(numpy.abs(got - S) / scale))


# ---- inputs ---------------------------------------------------------------------------------------------------------

PARITY_MESHES = [([16, 12, 20], [100., 80., 120.]), ([15, 9, 21], [90., 60., 130.])]


def parity_edges(Nmesh, BoxSize):
    kf = 2 * numpy.pi / max(BoxSize)
    bound = min(2 * numpy.pi / L * n / 3.0 for L, n in zip(BoxSize, Nmesh))
    e = kf * numpy.arange(0.5, 40)
    return numpy.concatenate([e[e < bound * 0.97], [bound]])


def parity_field(kind, Nmesh, BoxSize, dtype):
    cdt = {'f8': 'c16', 'f4': 'c8'}[dtype]
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=cdt if kind == 'c2c' else dtype)
    if kind == 'c2c':
        # a real-valued field on a complex mesh: its spectrum is Hermitian
        rng = numpy.random.RandomState(4)
        r = pm.create(type='real')
        r.value[...] = torch.from_numpy(rng.normal(size=tuple(r.value.shape)) + 0j).to(r.value.dtype)
        c = r.r2c()
    else:
        c = density(pm, seed=3).r2c(out=pm.create(type=UntransposedComplexField if kind == 'U'
                                                  else TransposedComplexField))
    return c, parity_edges(Nmesh, BoxSize)


def assert_sums(got, want, scale, tol):
    err = numpy.abs(got - want)
    bad = numpy.nonzero(~(err <= tol * scale))[0]
    print('max |S - S_ref| / scale = %.3g (bound %.3g)' % (numpy.max(err / numpy.where(scale > 0, scale, 1)), tol))
    assert len(bad) == 0, (bad[:5], err[bad[:5]], scale[bad[:5]])


# ---- 1. brute force -------------------------------------------------------------------------------------------------

def test_brute_force(bbe):
    Nmesh, BoxSize = [12, 10, 14], [100., 80., 120.]
    kf = 2 * numpy.pi / 120.
    ke = kf * numpy.array([0.5, 1.5, 2.5, 3.2])
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize)
    c = density(pm, seed=8).r2c()
    full = full_spectrum(c)
    S, C = brute_force(full, Nmesh, BoxSize, ke, 3)
    _, sh, _ = shells_full(Nmesh, BoxSize, ke)
    assert (sh >= 0).sum() == 74
    r = bispectrum(c, ke)
    tri = r.triangles
    assert [tuple(t) for t in tri] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 1, 2), (0, 2, 2), (1, 1, 1),
                                       (1, 1, 2), (1, 2, 2), (2, 2, 2)]
    want = numpy.array([C[i, j, l] for i, j, l in tri])
    assert (r.ntriangles == want).all(), (r.ntriangles, want)
    assert list(want) == [0, 12, 0, 64, 38, 48, 252, 254, 184, 240]
    assert (r.counts == want).all()
    _, _, scale = numpy_estimator(full, Nmesh, BoxSize, ke, 0, tri)
    Sb = numpy.array([S[i, j, l] for i, j, l in tri])
    assert numpy.abs(Sb.imag).max() <= F8_TOL * scale.max()
    assert_sums(r.sums, Sb.real, scale, F8_TOL)
    # triples outside the closed-triangle filter hold no triangle
    kept = set(tuple(t) for t in tri)
    for t in itertools.product(range(3), repeat=3):
        if tuple(sorted(t)) not in kept:
            assert C[t] == 0, t
    # B, Q and the per-shell columns
    V = float(numpy.prod(BoxSize))
    pk = power_spectrum(c, ke)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        B = V ** 2 * r.sums / want
    numpy.testing.assert_allclose(r.B, numpy.where(want > 0, B, numpy.nan), rtol=1e-14, equal_nan=True)
    assert numpy.isnan(r.B[[0, 2]]).all()
    # (the power kernel adds with float atomics: two calls agree to rounding, not to the bit)
    numpy.testing.assert_allclose(r.power, pk.power.real, rtol=1e-12)
    numpy.testing.assert_allclose(r.k, pk.k[tri], rtol=1e-12)
    p = r.power
    i, j, l = tri.T
    numpy.testing.assert_allclose(r.Q, r.B / (p[i] * p[j] + p[j] * p[l] + p[l] * p[i]), rtol=1e-14, equal_nan=True)


# ---- 2. estimator parity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('deconv_pow', [0, 2])
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
@pytest.mark.parametrize('Nmesh,BoxSize', PARITY_MESHES)
def test_estimator_parity(bbe, Nmesh, BoxSize, kind, deconv_pow, dtype):
    c, ke = parity_field(kind, Nmesh, BoxSize, dtype)
    tri = triangle_bins(ke)
    S, C, scale = numpy_estimator(full_spectrum(c), Nmesh, BoxSize, ke, deconv_pow, tri)
    before = c.value.clone()
    r = bispectrum(c, ke, deconv_pow=deconv_pow)
    assert torch.equal(c.value, before)
    assert (r.triangles == tri).all() and len(tri) > 10
    assert (r.ntriangles == numpy.rint(C)).all()
    assert numpy.abs(C - numpy.rint(C)).max() < 1e-6
    assert_sums(r.sums, S, scale, F8_TOL if dtype == 'f8' else F4_TOL)
    # power and Q belong to the same field as B: a / W
    assert_power_and_q(r, full_spectrum(c), Nmesh, BoxSize, ke, deconv_pow)
    # counts= reuse: the same result without the indicator half
    r2 = bispectrum(c, ke, deconv_pow=deconv_pow, counts=r)
    assert (r2.counts == r.counts).all()
    numpy.testing.assert_array_equal(r2.sums, r.sums)
    numpy.testing.assert_array_equal(r2.B, r.B)


@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_realfield_input(bbe, dtype):
    Nmesh, BoxSize = PARITY_MESHES[0]
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=dtype)
    x = density(pm, seed=3)
    before = x.value.clone()
    ke = parity_edges(Nmesh, BoxSize)
    r = bispectrum(x, ke, deconv_pow=2)
    assert torch.equal(x.value, before)
    c = x.r2c()
    S, C, scale = numpy_estimator(full_spectrum(c), Nmesh, BoxSize, ke, 2, r.triangles)
    assert (r.ntriangles == numpy.rint(C)).all()
    assert_sums(r.sums, S, scale, F8_TOL if dtype == 'f8' else F4_TOL)


# ---- 3. known answer ---------------------------------------------------------------------------------------------------

def test_three_plane_waves(bbe):
    Nmesh, L = [16, 16, 16], 100.
    kf = 2 * numpy.pi / L
    ke = kf * numpy.array([0.5, 1.5, 2.7, 3.5, 4.5])
    waves = [((1, 0, 0), 0.7 * numpy.exp(0.3j)), ((1, 2, 1), 1.3 * numpy.exp(-1.1j)), ((-2, -2, -1), 0.4 * numpy.exp(2.0j))]
    pm = ParticleMesh(Nmesh, BoxSize=L)
    x = numpy.stack(numpy.meshgrid(*[numpy.arange(n) * (L / n) for n in Nmesh], indexing='ij'))
    delta = numpy.zeros(Nmesh)
    for s, A in waves:
        phase = kf * sum(sd * xd for sd, xd in zip(s, x))
        delta += 2 * (A * numpy.exp(1j * phase)).real
    r = pm.create(type='real')
    r.value[...] = torch.from_numpy(delta).to(r.value.device)
    res = bispectrum(r.r2c(), ke)
    A3 = waves[0][1] * waves[1][1] * waves[2][1]
    amax = 1.3
    tol = F8_TOL * 8 * amax ** 3
    hit = [tuple(t) for t in res.triangles].index((0, 1, 2))
    assert abs(res.sums[hit] - 2 * A3.real) <= tol
    assert res.ntriangles[hit] > 0
    assert abs(res.B[hit] - L ** 6 * 2 * A3.real / res.ntriangles[hit]) <= tol * L ** 6
    for t in range(len(res.triangles)):
        if t == hit:
            continue
        assert abs(res.sums[t]) <= tol, (res.triangles[t], res.sums[t])
        assert numpy.isnan(res.B[t]) if res.ntriangles[t] == 0 else abs(res.B[t]) <= tol * L ** 6


# ---- 4. arguments ----------------------------------------------------------------------------------------------------

def test_bad_arguments(bbe):
    pm = ParticleMesh([12, 12, 12], BoxSize=100.)
    c = pm.create(type='complex')
    kf = 2 * numpy.pi / 100.
    for bad in ([1.0], [0.0, 0.0], [0.3, 0.1, 0.2], [0, numpy.nan], [[0, 1], [1, 2]]):
        with pytest.raises(ValueError, match='kedges'):
            bispectrum(c, bad)
    with pytest.raises(ValueError, match='PMX_BISPEC_MAX_SHELLS'):
        bispectrum(c, numpy.linspace(0, 3 * kf, _abi.PMX_BISPEC_MAX_SHELLS + 2))
    assert alias_bound(pm) == pytest.approx(4 * kf)
    with pytest.raises(ValueError, match='alias bound'):
        bispectrum(c, [0.5 * kf, 1.5 * kf, 4.001 * kf])
    bispectrum(c, [0.5 * kf, 1.5 * kf, alias_bound(pm)])          # the bound itself is allowed
    with pytest.raises(ValueError, match='deconv_pow'):
        bispectrum(c, [0.5 * kf, 1.5 * kf], deconv_pow=-1)
    with pytest.raises(TypeError):
        bispectrum(numpy.zeros((12, 12, 7), 'c16'), [0.5 * kf, 1.5 * kf])
    with pytest.raises(NotImplementedError):
        bispectrum(ParticleMesh([12, 12], BoxSize=100.).create(type='complex'), [0.5 * kf, 1.5 * kf])
    # counts of other edges, of another mesh, of another kind
    r = bispectrum(c, [0.5 * kf, 1.5 * kf, 2.5 * kf])
    assert isinstance(r, BispectrumResult)
    with pytest.raises(ValueError, match='counts'):
        bispectrum(c, [0.5 * kf, 1.5 * kf, 2.5 * kf, 3.5 * kf], counts=r)
    with pytest.raises(ValueError, match='counts'):
        bispectrum(c, [0.5 * kf, 1.5 * kf, 2.6 * kf], counts=r)
    with pytest.raises(ValueError, match='counts'):
        bispectrum(ParticleMesh([12, 12, 14], BoxSize=100.).create(type='complex'), r.kedges, counts=r)
    with pytest.raises(ValueError, match='counts'):
        bispectrum(ParticleMesh([12, 12, 12], BoxSize=[100., 100., 90.]).create(type='complex'), r.kedges, counts=r)
    with pytest.raises(TypeError):
        bispectrum(c, r.kedges, counts=r.counts)


# ---- 5. ranks equal one ------------------------------------------------------------------------------------------------

def _ranks_equal_one(size, np_, Nmesh, edges=(0.5, 1.5, 2.5, 3.5)):
    from tests import thread_comm
    kf = 2 * numpy.pi / 100.
    ke = kf * numpy.array(edges)
    results, empty = {}, {}

    def body(comm):
        pm = ParticleMesh(Nmesh, BoxSize=100., comm=comm, np=np_)
        c = density(pm, seed=5).r2c()
        empty[comm.rank] = c.value.numel() == 0 or pm.create(type='real').value.numel() == 0
        results[comm.rank] = bispectrum(c, ke, deconv_pow=2)
    thread_comm.run_ranks(size, body)
    pm1 = ParticleMesh(Nmesh, BoxSize=100.)
    c1 = density(pm1, seed=5).r2c()
    one = bispectrum(c1, ke, deconv_pow=2)
    _, _, scale = numpy_estimator(full_spectrum(c1), Nmesh, [100.] * 3, ke, 2, one.triangles)
    for r in range(size):
        assert (results[r].counts == one.counts).all()
        assert_sums(results[r].sums, one.sums, scale, F8_TOL)
        numpy.testing.assert_array_equal(results[r].power, results[0].power)
    return empty


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
def test_ranks_equal_one(size, np_):
    backend.reset()
    backend.use(BispecOracleBackend())
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
    """six planes over eight ranks: two ranks hold no cell and no mode (the decompositions of [16, 16, 12] above leave
    no rank empty)"""
    empty = _ranks_equal_one(8, [8], [6, 16, 12], edges=(0.5, 1.2, 2.0))
    assert any(empty.values())


# ---- 6. kernel level ---------------------------------------------------------------------------------------------------

def _reduce_reference(blocks, tri):
    f = numpy.stack([b.astype('f8').reshape(-1) for b in blocks])
    want = numpy.empty(len(tri))
    scale = numpy.empty(len(tri))
    for a in range(0, len(tri), 512):
        t = tri[a:a + 512]
        p = f[t[:, 0]] * f[t[:, 1]] * f[t[:, 2]]
        want[a:a + 512] = numpy.einsum('tx->t', p)
        scale[a:a + 512] = numpy.einsum('tx->t', numpy.abs(p))
    return want, scale


def _all_triples(nb):
    return numpy.array([t for t in itertools.combinations_with_replacement(range(nb), 3)], dtype='i4')


def _run_reduce(be, blocks, tri):
    dev = be.device
    # a padded last axis: views [..., :n] of longer buffers, as the in-place transform buffers are
    bufs = [torch.full(b.shape[:-1] + (b.shape[-1] + 3,), float('nan'), dtype=torch.from_numpy(b).dtype, device=dev)
            for b in blocks]
    views = []
    for buf, b in zip(bufs, blocks):
        v = buf[..., :b.shape[-1]]
        v[...] = torch.from_numpy(b).to(dev)
        views.append(v)
    tt = torch.from_numpy(tri).to(dev)
    acc = torch.zeros(len(tri), dtype=torch.float64, device=dev)
    be.bispec_reduce(views, tt, acc)
    acc2 = torch.zeros(len(tri), dtype=torch.float64, device=dev)
    be.bispec_reduce(views, tt, acc2)
    assert torch.equal(acc, acc2), 'two calls on the same input differ'
    return acc.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('nb', [1, 2, 7, 33, 64])
def test_kernel_reduce(hipbe, nb, dtype):
    rng = numpy.random.RandomState(nb)
    lists = [_all_triples(nb)[-1:], triangle_bins(numpy.arange(nb + 1) + 0.5)]
    if nb == 33:
        lists.append(_all_triples(33))
        assert len(lists[-1]) == 6545
    for shape in ([5, 7, 11], [1, 1, 3]):
        blocks = [rng.normal(size=shape).astype(dtype) for _ in range(nb)]
        for tri in lists:
            want, scale = _reduce_reference(blocks, tri)
            assert_sums(_run_reduce(hipbe, blocks, tri), want, scale, F8_TOL)


@pytest.mark.gpu
def test_kernel_reduce_many_chunks_unsorted_list_and_acc_adds(hipbe):
    """more chunks than workgroups (a workgroup walks several), a list in random order with repeats, and acc is
    added to, not overwritten"""
    rng = numpy.random.RandomState(0)
    shape = [70, 64, 65]
    blocks = [rng.normal(size=shape) for _ in range(7)]
    tri = _all_triples(7)[rng.randint(0, 84, size=150)]
    want, scale = _reduce_reference(blocks, tri)
    dev = hipbe.device
    ts = [torch.from_numpy(b).to(dev) for b in blocks]
    tt = torch.from_numpy(tri).to(dev)
    acc = torch.zeros(len(tri), dtype=torch.float64, device=dev)
    hipbe.bispec_reduce(ts, tt, acc)
    assert_sums(acc.cpu().numpy(), want, scale, F8_TOL)
    once = acc.clone()
    hipbe.bispec_reduce(ts, tt, acc)
    assert torch.equal(acc, once + once)
    # a small work vector: fewer workgroups, the same sums to the bound
    acc2 = torch.zeros(len(tri), dtype=torch.float64, device=dev)
    hipbe.bispec_reduce(ts, torch.from_numpy(tri).to(dev), acc2,
                        work=torch.empty(3 * len(tri), dtype=torch.float64, device=dev))
    assert_sums(acc2.cpu().numpy(), want, scale, F8_TOL)


@pytest.mark.gpu
def test_kernel_reduce_edges(hipbe):
    dev = hipbe.device
    tri = torch.from_numpy(_all_triples(3)).to(dev)
    acc = torch.zeros(len(tri), dtype=torch.float64, device=dev)
    # an empty block, and an empty list
    hipbe.bispec_reduce([torch.zeros((0, 4, 5), dtype=torch.float64, device=dev)] * 3, tri, acc)
    assert (acc == 0).all()
    hipbe.bispec_reduce([torch.ones((2, 4, 5), dtype=torch.float64, device=dev)] * 3, tri[:0], acc[:0])
    # limits
    one = torch.ones((2, 4, 5), dtype=torch.float64, device=dev)
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_reduce([one] * 65, tri, acc)
    big = torch.zeros((_abi.PMX_BISPEC_MAX_TRIANGLES + 1, 3), dtype=torch.int32, device=dev)
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_reduce([one] * 3, big, torch.zeros(len(big), dtype=torch.float64, device=dev))
    # a triple that names no shell gives NaN and leaves the others alone
    t = torch.tensor([[0, 1, 2], [0, 1, 3], [2, 2, 2]], dtype=torch.int32, device=dev)
    a = torch.zeros(3, dtype=torch.float64, device=dev)
    hipbe.bispec_reduce([one] * 3, t, a)
    assert a[0] == 40 and a[2] == 40 and torch.isnan(a[1])


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('kind', ['T', 'U', 'c2c'])
def test_kernel_shells(hipbe, kind, dtype):
    Nmesh, BoxSize = [16, 12, 20], [100., 80., 120.]
    c, _ = parity_field(kind, Nmesh, BoxSize, dtype)
    pm = c.pm
    kf = 2 * numpy.pi / 120.
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(Nmesh, BoxSize))) * 1.01
    ke = numpy.arange(0, kmax + kf, kf)                        # covers every mode; many modes sit on edges
    nb = len(ke) - 1
    kt = torch.from_numpy(ke).to(hipbe.device)
    modes = power_spectrum(c, ke).modes
    w = numpy.ones(tuple(c.value.shape))
    if c.compressed:
        il = c.i[-1].cpu().numpy()
        w = numpy.broadcast_to(1.0 + ((il != 0) & (il != Nmesh[-1] // 2)), w.shape)
    def shells(unit):
        outs = [pm.create(type=type(c)) for _ in range(nb)]
        for o in outs:
            torch.view_as_real(o.value).fill_(float('nan'))
        hipbe.bispec_shells(None if unit else c.value, [o.value for o in outs], c.start, pm.Nmesh, pm.BoxSize, kt, 0,
                            unit)
        vals = [o.value.cpu().numpy() for o in outs]
        assert all(numpy.isfinite(v.real).all() and numpy.isfinite(v.imag).all() for v in vals), 'an element not written'
        return vals
    # the indicator: every mode in exactly one shell, the shell power_spectrum counts it in
    ind = shells(True)
    assert (sum(ind) == 1).all()
    got = numpy.array([int(numpy.rint((v.real * w).sum())) for v in ind])
    assert (got == modes).all(), (got, modes)
    # the modes: the input where the shell's indicator is 1, zero elsewhere; their sum is the input
    vals = shells(False)
    cv = c.value.cpu().numpy()
    assert (sum(vals) == cv).all()
    for v, u in zip(vals, ind):
        assert (v == numpy.where(u == 1, cv, 0)).all()
    # the window: the double's division axis by axis
    outs = [pm.create(type=type(c)) for _ in range(nb)]
    hipbe.bispec_shells(c.value, [o.value for o in outs], c.start, pm.Nmesh, pm.BoxSize, kt, 2, False)
    ref = [torch.zeros_like(o.value).cpu() for o in outs]
    BispecOracleBackend.bispec_shells(None, c.value.cpu(), ref, c.start, pm.Nmesh, pm.BoxSize, kt.cpu(), 2, False)
    eps = 1e-6 if dtype == 'f4' else 1e-14
    for o, r_ in zip(outs, ref):
        numpy.testing.assert_allclose(o.value.cpu().numpy(), r_.numpy(), rtol=eps, atol=0)
    with pytest.raises(backend.PmxError, match='PMX_EUNSUPPORTED'):
        hipbe.bispec_shells(c.value, [outs[0].value] * 65, c.start, pm.Nmesh, pm.BoxSize, kt, 0, False)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernel_reduce_blocks_of_one_and_two_dimensions(hipbe, dtype):
    """the entry takes blocks of 1 to 3 dimensions: a vector and a matrix with a padded last axis"""
    rng = numpy.random.RandomState(2)
    tri = _all_triples(5)
    for shape in ([37], [1], [5, 9], [700, 3]):
        blocks = [rng.normal(size=shape).astype(dtype) for _ in range(5)]
        want, scale = _reduce_reference(blocks, tri)
        assert_sums(_run_reduce(hipbe, blocks, tri), want, scale, F8_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('Nmesh,BoxSize', [([32], [100.]), ([16, 12], [100., 80.])])
def test_kernel_shells_of_one_and_two_dimensions(hipbe, Nmesh, BoxSize, dtype):
    """the entry takes blocks of 1 to 3 dimensions: every mode in the shell power_spectrum counts it in, the values
    those of the numpy double"""
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=dtype)
    c = density(pm, seed=6).r2c()
    kf = 2 * numpy.pi / max(BoxSize)
    kmax = numpy.sqrt(sum((numpy.pi * n / L) ** 2 for n, L in zip(Nmesh, BoxSize))) * 1.01
    ke = numpy.arange(0, kmax + kf, kf)
    nb = len(ke) - 1
    kt = torch.from_numpy(ke).to(hipbe.device)
    il = c.i[-1].cpu().numpy()
    w = numpy.broadcast_to(1.0 + ((il != 0) & (il != Nmesh[-1] // 2)), tuple(c.value.shape))
    for deconv_pow, unit in ((0, True), (0, False), (2, False)):
        outs = [pm.create(type=type(c)) for _ in range(nb)]
        for o in outs:
            torch.view_as_real(o.value).fill_(float('nan'))
        hipbe.bispec_shells(None if unit else c.value, [o.value for o in outs], c.start, pm.Nmesh, pm.BoxSize, kt,
                            deconv_pow, unit)
        ref = [torch.zeros_like(o.value).cpu() for o in outs]
        BispecOracleBackend.bispec_shells(None, c.value.cpu(), ref, c.start, pm.Nmesh, pm.BoxSize, kt.cpu(), deconv_pow,
                                          unit)
        for o, r_ in zip(outs, ref):
            got = o.value.cpu().numpy()
            if deconv_pow:
                numpy.testing.assert_allclose(got, r_.numpy(), rtol=1e-6 if dtype == 'f4' else 1e-14, atol=0)
            else:
                assert (got == r_.numpy()).all()
        if unit:
            got = numpy.array([int(numpy.rint((o.value.real.cpu().numpy() * w).sum())) for o in outs])
            assert (got == power_spectrum(c, ke).modes).all()


# ---- 7. resources (compiles for gfx950 on the CPU) ----------------------------------------------------------------------

def test_bispec_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_bispec.hip')
    assert sum('reduce_kernel' in k for k in t) == 6 and sum('shells_kernel' in k for k in t) == 2, sorted(t)
    for name, r in t.items():
        assert r['ScratchSize'] == 0, (name, r)
