"""pmesh_amd.interlace (csrc/pmx_interlace.hip) against a numpy restatement of its definition and against known answers.

The restatement builds the circular frequencies of a block as pm._block_coords does (the signed mode number times
2 pi / N, the Nyquist frequency negative), the phase as exp(1j * theta) in double and the window from test_power's
sinc power.  Under -m "not gpu" it serves pmx_phase_combine (InterlaceOracleBackend), so the host layer — the order of
the paints, the scratch buffer, the weights, the routing on several ranks — runs without a GPU; under -m gpu the kernel
is compared with it.  The known answer is a plane wave of masses on a lattice finer than the mesh: its spectrum on the
mesh consists of one class of alias images, which interlacing removes or keeps as a whole.
"""
import numpy
import pytest
import torch

from pmesh_amd import _abi, backend, window
from pmesh_amd.interlace import interlaced_field, paint_interlaced, phase_combine
from pmesh_amd.pm import ParticleMesh, RealField, TransposedComplexField, UntransposedComplexField
from pmesh_amd.power import power_spectrum
from pmesh_amd.survey import survey_multipoles
from tests.test_lpt import FORMS, TALL, TALL_1D, _block, _nan_block, close_rows, cpu
from tests.test_power import _sinc_pow, kf_edges
from tests.test_survey import SurveyOracleBackend


# ---- the restatement -----------------------------------------------------------------------------------------------

def block_w(start, shape, nmesh):
    """the circular frequencies of a block per axis, shaped to broadcast: pm._block_coords' `signed * (2 pi / N)`"""
    nd = len(shape)
    out = []
    for d in range(nd):
        n = int(nmesh[d])
        m = numpy.arange(int(shape[d]), dtype='f8') + int(start[d])
        m[m >= n // 2] -= n
        out.append((m * (2 * numpy.pi / n)).reshape([-1 if dd == d else 1 for dd in range(nd)]))
    return out


def window_of(start, shape, nmesh, p):
    """prod_d sinc(w_d / 2)^p, 1 for p = 0"""
    comp = numpy.ones(tuple(int(s) for s in shape))
    if p:
        for w in block_w(start, shape, nmesh):
            comp = comp * _sinc_pow(w, p)
    return comp


def ref_combine(vals, acc, start, nmesh, shift, a, b, p):
    """pmx_phase_combine: (a acc + b exp(i theta) in) / prod_d sinc(w_d / 2)^p, theta = sum_d shift_d w_d; acc is not
    looked at when a == 0"""
    vals = numpy.asarray(vals).astype('c16')
    theta = 0
    for s, w in zip(shift, block_w(start, vals.shape, nmesh)):
        theta = theta + float(s) * w
    out = b * (numpy.exp(1j * theta) * vals)
    if a != 0:
        out = out + a * numpy.asarray(acc).astype('c16')
    return out / window_of(start, vals.shape, nmesh, p)


class InterlaceOracleBackend(SurveyOracleBackend):
    """the CPU test double (a PowerOracleBackend with the survey entries, for the downstream tests) with
    pmx_phase_combine served by the restatement"""
    name = 'oracle-interlace'

    def phase_combine(self, v, acc, start, nmesh, shift, a, b, deconv_pow=0):
        want = ref_combine(v.numpy(), acc.numpy().copy(), start, nmesh, shift, a, b, deconv_pow)
        acc.copy_(torch.from_numpy(want))


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def ibe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(InterlaceOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- 1. the kernel against the restatement (GPU) -------------------------------------------------------------------

# the half spectra of the meshes (8, 6, 10) and (9, 8, 6), each at a start inside a larger mesh such that every axis
# crosses the change of sign at N // 2, and once where they belong
BLOCKS = [([8, 6, 6], [3, 2, 6], [16, 12, 20]),
          ([9, 8, 4], [4, 1, 2], [18, 11, 9]),
          ([8, 6, 6], [0, 0, 0], [8, 6, 10]),
          ([9, 8, 4], [0, 0, 0], [9, 8, 6])]
SHIFTS = [(0.5, 0.5, 0.5), (1 / 3., 1 / 3., 1 / 3.), (0.25, -0.5, 0.)]
POWS = (0, 2, 3)
WEIGHTS = [(0.0, 1.0), (0.5, 0.5), (1.0, 1.0), (1 / 3., 1 / 3.), (-0.75, 1.25)]


def bound_f8(vals, acc, a, b, comp):
    """1e-14 * max(|a acc| + |b in|) / min|comp|: a phase error of at most 2e-15 (three rounded terms and sincospi),
    one complex multiply-add and one division, each a few 1e-16 of the operands"""
    big = numpy.abs(b) * numpy.abs(vals)
    if a != 0:
        big = big + numpy.abs(a) * numpy.abs(acc)
    return 1e-14 * big.max() / numpy.abs(comp).min()


def assert_within(got, want, tol8, single):
    """the f8 bound; in single precision one rounding of the result to float more, 6e-8 |want|"""
    got, want = numpy.asarray(got).astype('c16'), numpy.asarray(want)
    assert numpy.isfinite(got.real).all() and numpy.isfinite(got.imag).all()
    slack = tol8 + (6e-8 * numpy.abs(want) if single else 0.0)
    err = numpy.abs(got - want)
    assert (err <= slack).all(), (err.max(), tol8)


def run_case(be, rng, shape, start, nmesh, cdt, form_in, form_acc, shift, a, b, p):
    nd = len(shape)
    v = _block(shape, cdt, form_in, rng)
    acc = _nan_block(shape, cdt, form_acc, rng) if a == 0 else _block(shape, cdt, form_acc, rng)
    vals, before = cpu(v).copy(), cpu(acc).copy()
    want = ref_combine(vals, before, start, nmesh, shift[:nd], a, b, p)
    tol8 = bound_f8(vals, before, a, b, window_of(start, shape, nmesh, p))
    be.phase_combine(v, acc, start, nmesh, shift[:nd], a, b, p)
    assert (cpu(v) == vals).all()
    return cpu(acc), want, tol8


@pytest.mark.gpu
@pytest.mark.parametrize('form_acc', FORMS)
@pytest.mark.parametrize('form_in', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
def test_combine_kernel(hipbe, cdt, form_in, form_acc):
    rng = numpy.random.RandomState(31)
    n = 0
    for shape, start, nmesh in BLOCKS:
        for shift in SHIFTS:
            for p in POWS:
                # a == 0 into NaN memory and a != 0 for every shift and power; the weights in turn
                for a, b in (WEIGHTS[0], WEIGHTS[1 + n % (len(WEIGHTS) - 1)]):
                    got, want, tol8 = run_case(hipbe, rng, shape, start, nmesh, cdt, form_in, form_acc, shift, a, b, p)
                    assert_within(got, want, tol8, cdt == 'c8')
                n += 1


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
def test_combine_kernel_past_the_row_wrap(hipbe, cdt, form):
    """blocks with more rows than the 65535-row launch wrap: the rows of the second trip on their own scale"""
    rng = numpy.random.RandomState(32)
    other = 'pad' if form != 'pad' else 'C'
    for gi, (shape, start, nmesh) in enumerate(TALL + TALL_1D):
        shift, p = SHIFTS[gi % len(SHIFTS)], POWS[gi % len(POWS)]
        for a, b in ((0.0, 1.0), (0.5, 0.5)):
            got, want, tol8 = run_case(hipbe, rng, shape, start, nmesh, cdt, form, other, shift, a, b, p)
            assert_within(got, want, tol8, cdt == 'c8')
            scale = numpy.abs(want).max()
            close_rows(got, want, tol8 / scale + (6e-8 if cdt == 'c8' else 0.0))


@pytest.mark.gpu
def test_phase_at_every_mode_number(hipbe):
    """a 1-d mesh of 131072 points: the phase at m = -65536 .. 65535 within the f8 bound.  A phase formed as
    sincos(pi * (2 shift m / N)) with a rounded pi, or from an unreduced angle, misses it at large |m|."""
    n = 131072
    rng = numpy.random.RandomState(33)
    for shift in (0.5, 1 / 3., -0.25, 2.75):
        got, want, tol8 = run_case(hipbe, rng, [n], [0], [n], 'c16', 'C', 'C', (shift,), 0.0, 1.0, 0)
        assert_within(got, want, tol8, False)
        got, want, tol8 = run_case(hipbe, rng, [n], [0], [n], 'c16', 'C', 'C', (shift,), 1.0, 1.0, 2)
        assert_within(got, want, tol8, False)


# ---- 2. refusals (GPU) ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_kernel_refuses_what_it_does_not_do(hipbe):
    from pmesh_amd.backend import _byte_strides
    rng = numpy.random.RandomState(1)
    c = _block([4, 4, 3], 'c16', 'C', rng)
    d = _block([4, 4, 3], 'c16', 'C', rng)
    before = cpu(d).copy()

    def raw(ndim=3, elsize=8, in_=None, acc=None, pow_=0, strides=True, geom=True, shift=True):
        args = [ndim, elsize, c.data_ptr() if in_ is None else in_, _byte_strides(c) if strides else None,
                d.data_ptr() if acc is None else acc, _byte_strides(d) if strides else None]
        args += [_abi.i64arr([4, 4, 3], 3), _abi.i64arr([0] * 3, 3), _abi.i64arr([4, 4, 4], 3)] if geom else [None] * 3
        args += [_abi.f64arr([0.5] * 3, 3) if shift else None, 0.5, 0.5, pow_, hipbe.stream()]
        with pytest.raises(backend.PmxError) as e:
            hipbe.call('phase_combine', *args)
        return e.value.code

    assert raw(acc=c.data_ptr()) == _abi.PMX_EINVAL                          # the same block
    assert raw(acc=c.data_ptr() + 16 * 5) == _abi.PMX_EINVAL                 # a block that starts inside the other
    assert raw(elsize=2) == _abi.PMX_EINVAL
    assert raw(ndim=4) == _abi.PMX_EINVAL
    assert raw(ndim=0) == _abi.PMX_EINVAL
    assert raw(pow_=-1) == _abi.PMX_EINVAL
    assert raw(in_=0) == _abi.PMX_EINVAL
    assert raw(acc=0) == _abi.PMX_EINVAL
    assert raw(strides=False) == _abi.PMX_EINVAL
    assert raw(geom=False) == _abi.PMX_EINVAL
    assert raw(shift=False) == _abi.PMX_EINVAL
    with pytest.raises(backend.PmxError) as e:
        hipbe.phase_combine(c, c, [0] * 3, [4] * 3, [0.5] * 3, 0.5, 0.5, 0)
    assert e.value.code == _abi.PMX_EINVAL
    with pytest.raises(backend.PmxError) as e:
        hipbe.phase_combine(c, d, [0] * 3, [4] * 3, [0.5] * 3, 0.5, 0.5, -2)
    assert e.value.code == _abi.PMX_EINVAL
    assert (cpu(d) == before).all()


# ---- 3. alias cancellation, the known answer (both backends) -------------------------------------------------------

MESH = (8, 6, 10)
BOX = [100., 80., 120.]
K0 = (1, 2, 1)


def image_particles(order, image):
    """particles on the lattice of order * N_d points per axis, offset by 0.37 / order cell, with the masses
    cos(q.x + 0.3), q = 2 pi / L * (K0 + N * image): on the mesh, the modes +-K0 made of the alias images
    image + order * Z^3 alone"""
    N, L = numpy.array(MESH), numpy.array(BOX)
    axes = [(numpy.arange(order * n) + 0.37) / order * (l / n) for n, l in zip(N, L)]
    pos = numpy.stack([g.reshape(-1) for g in numpy.meshgrid(*axes, indexing='ij')], axis=1)
    q = 2 * numpy.pi / L * (numpy.array(K0) + N * numpy.array(image))
    return pos, numpy.cos(pos @ q + 0.3)


def scale_of(mass, nmesh):
    """S = sum |mass| / prod N: what no mode of a painted spectrum exceeds"""
    return numpy.abs(mass).sum() / float(numpy.prod(nmesh))


# order -> (images that vanish, images that are kept as a plain paint has them)
IMAGES = {2: ([(1, 0, 0)], [(1, 1, 0), (0, -1, 1)]),
          3: ([(1, 0, 0), (1, 1, 0)], [(1, 1, 1), (0, -1, 1)])}


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('resampler', ['cic', 'tsc'])
def test_alias_images_cancel(ibe, resampler, order):
    """In numpy with a CIC restatement the cancelled images gave 1e-15 to 4e-15 against S of 5 to 17 and the kept ones
    differed from the plain spectrum by less than 3e-15: 1e-13 * S leaves a margin of about 100 in f8."""
    pm = ParticleMesh(MESH, BoxSize=BOX, dtype='f8')
    gone, kept = IMAGES[order]
    for image in gone:
        pos, mass = image_particles(order, image)
        S = scale_of(mass, MESH)
        plain = numpy.abs(cpu(pm.paint(pos, mass=mass, resampler=resampler).r2c().value)).max()
        left = numpy.abs(cpu(paint_interlaced(pm, pos, mass=mass, resampler=resampler, order=order).value)).max()
        print('%s order %d image %s: plain %.3e S, interlaced %.3e S' % (resampler, order, image, plain / S, left / S))
        # the plain paint holds the image: the nearest one at more than 1e-3 S, every one far above the bound
        assert plain > (1e-3 if image == (1, 0, 0) and order == 2 else 1e-10) * S
        assert left <= 1e-13 * S
    for image in kept:
        pos, mass = image_particles(order, image)
        S = scale_of(mass, MESH)
        plain = cpu(pm.paint(pos, mass=mass, resampler=resampler).r2c().value)
        got = cpu(paint_interlaced(pm, pos, mass=mass, resampler=resampler, order=order).value)
        err = numpy.abs(got - plain).max()
        print('%s order %d image %s: plain %.3e S, difference %.3e S' % (resampler, order, image,
                                                                         numpy.abs(plain).max() / S, err / S))
        assert numpy.abs(plain).max() > 1e-10 * S          # (there is something to keep, far above the bound)
        assert err <= 1e-13 * S


@pytest.mark.parametrize('order', [2, 3])
@pytest.mark.parametrize('resampler', ['cic', 'tsc'])
def test_alias_images_cancel_in_single_precision(ibe, resampler, order):
    """f4 meshes: the bound is 8 times the measured max |A_f4 - A_f8| of the plain spectrum of the same particles
    (one f4 paint and transform per mesh, up to three of them, and the combine's rounding).  Measured with the
    restated combine over the CPU double of the paint and the transform: max |A_f4 - A_f8| between 2.9e-10 S and
    7.6e-9 S over the fourteen cases (CIC and TSC, orders 2 and 3; 4.4e-9 S for CIC, order 2, image (1, 0, 0)), and the
    interlaced f4 spectrum off its answer by 0.50 to 0.93 of it, cancelled and kept images alike."""
    pm8 = ParticleMesh(MESH, BoxSize=BOX, dtype='f8')
    pm4 = ParticleMesh(MESH, BoxSize=BOX, dtype='f4')
    gone, kept = IMAGES[order]
    for image in gone + kept:
        pos, mass = image_particles(order, image)
        S = scale_of(mass, MESH)
        plain8 = cpu(pm8.paint(pos, mass=mass, resampler=resampler).r2c().value)
        plain4 = cpu(pm4.paint(pos, mass=mass, resampler=resampler).r2c().value).astype('c16')
        f4err = numpy.abs(plain4 - plain8).max()
        assert 0 < f4err < 1e-5 * S
        got = paint_interlaced(pm4, pos, mass=mass, resampler=resampler, order=order)
        assert got.value.dtype == torch.complex64
        want = 0 * plain8 if image in gone else plain8
        err = numpy.abs(cpu(got.value).astype('c16') - want).max()
        print('%s order %d image %s: max |A_f4 - A_f8| = %.3e S, interlaced f4 error %.2f of it'
              % (resampler, order, image, f4err / S, err / f4err))
        assert err <= 8 * f4err


# ---- 4. composition (both backends) --------------------------------------------------------------------------------

def random_particles(pm, n, seed):
    """positions inside and outside the box, masses of both signs"""
    rng = numpy.random.RandomState(seed)
    L = numpy.asarray(pm.BoxSize)
    return rng.uniform(-0.3, 1.3, size=(n, len(L))) * L, rng.normal(size=n)


def restated(pm, pos, mass, resampler, order, compensate, T=TransposedComplexField):
    """the definition, term by term: (1 / order) sum_j exp(i (j / order) sum_d w_d) r2c[paint shifted by j / order],
    divided by the window, from pm.paint and r2c of the backend under test and the restated combine"""
    p = window.FindResampler(resampler).nativesupport if compensate else 0
    nd = len(pm.Nmesh)
    total = None
    for j in range(order):
        A = pm.paint(pos, mass=mass, resampler=resampler, transform=pm.affine.shift(j / float(order)))
        A = A.r2c(out=pm.create(type=T))
        term = ref_combine(cpu(A.value), None, A.start, pm.Nmesh, [j / float(order)] * nd, 0.0, 1.0 / order, 0)
        total = term if total is None else total + term
    return total / window_of(A.start, total.shape, pm.Nmesh, p)


def composition_bound(mass, nmesh, resampler, compensate):
    """1e-13 * S / min |window|: up to three combines of 1e-14 (|a acc| + |b in|) / min |window| each, with every
    operand below S = sum |mass| / prod N, and the atomic adds of two paints of the same particles in another order,
    a few 1e-16 S"""
    p = window.FindResampler(resampler).nativesupport if compensate else 0
    return 1e-13 * scale_of(mass, nmesh) / numpy.abs(window_of([0] * len(nmesh), nmesh, nmesh, p)).min()


@pytest.mark.parametrize('order', [1, 2, 3])
@pytest.mark.parametrize('compensate', [False, True])
@pytest.mark.parametrize('nmesh,box', [((8, 6, 10), BOX), ((9, 8, 6), BOX), ((12, 10), BOX[:2])])
def test_composition(ibe, nmesh, box, compensate, order):
    pm = ParticleMesh(nmesh, BoxSize=box, dtype='f8')
    pos, mass = random_particles(pm, 500, seed=41)
    for resampler in ('cic', 'tsc'):
        tol = composition_bound(mass, nmesh, resampler, compensate)
        for T in (TransposedComplexField, UntransposedComplexField):
            want = restated(pm, pos, mass, resampler, order, compensate, T)
            out = pm.create(type=T)
            got = paint_interlaced(pm, pos, mass=mass, resampler=resampler, order=order, compensate=compensate, out=out)
            assert got is out
            err = numpy.abs(cpu(got.value) - want).max()
            print('%s %s order %d compensate %d %s: error %.2e of the bound' % (nmesh, resampler, order, compensate,
                                                                             T.__name__[:1], err / tol))
            assert err <= tol
        new = paint_interlaced(pm, pos, mass=mass, resampler=resampler, order=order, compensate=compensate)
        assert isinstance(new, TransposedComplexField)
        want = restated(pm, pos, mass, resampler, order, compensate)
        assert numpy.abs(cpu(new.value) - want).max() <= tol
    # the default window is the mesh's, a scalar mass is a scalar mass
    want = restated(pm, pos, 2.5, pm.resampler, order, compensate)
    got = paint_interlaced(pm, pos, mass=2.5, order=order, compensate=compensate)
    assert numpy.abs(cpu(got.value) - want).max() <= composition_bound(numpy.full(len(pos), 2.5), nmesh, 'cic', compensate)


def test_phase_combine_on_fields(ibe):
    """the public combine: in place on acc, the other field untouched, transposed and untransposed"""
    pm = ParticleMesh((8, 6, 10), BoxSize=BOX, dtype='f8')
    for T in (TransposedComplexField, UntransposedComplexField):
        A = pm.generate_whitenoise(5, type=T)
        B = pm.generate_whitenoise(6, type=T)
        a0, b0 = cpu(A.value).copy(), cpu(B.value).copy()
        want = ref_combine(b0, a0, A.start, pm.Nmesh, (0.25, -0.5, 0.), 0.5, 0.5, 2)
        r = phase_combine(A, B, (0.25, -0.5, 0.), deconv_pow=2)
        assert r is A
        assert (cpu(B.value) == b0).all()
        assert numpy.abs(cpu(A.value) - want).max() <= bound_f8(b0, a0, 0.5, 0.5, window_of(A.start, a0.shape, pm.Nmesh, 2))
        want = ref_combine(b0, None, A.start, pm.Nmesh, (0.5, 0.5, 0.5), 0.0, 2.0, 0)
        phase_combine(A, B, 0.5, a=0, b=2.0)
        assert numpy.abs(cpu(A.value) - want).max() <= bound_f8(b0, None, 0.0, 2.0, numpy.ones(1))


@pytest.mark.gpu
def test_tile_binned_paint_of_the_displaced_mesh(hipbe):
    """enough particles that the tile-binned kernels paint the fractional translate: equal to the direct kernels
    within the tolerance of the binned paint, 1e-12 of the largest cell (tests/test_binned.py) — a mode is a mean of
    the cells times phases, so no mode differs by more than the largest cell difference"""
    # (16, 32, 64): the smallest whole periodic mesh the tile kernels take, 2 x 2 x 2 tiles of (8, 16, 32) cells
    pm = ParticleMesh((16, 32, 64), BoxSize=BOX, dtype='f8')
    pos, mass = random_particles(pm, 40000, seed=42)
    mass = numpy.abs(mass)
    pos, mass = torch.from_numpy(pos).to(hipbe.device), torch.from_numpy(mass).to(hipbe.device)
    old = window.BINNED
    try:
        window.BINNED = 'never'
        direct = {o: cpu(paint_interlaced(pm, pos, mass=mass, order=o).value) for o in (2, 3)}
        cell = float(pm.paint(pos, mass=mass).value.abs().max())
        window.BINNED = 'always'
        window.clear_bin_cache()
        for o in (2, 3):
            binned = cpu(paint_interlaced(pm, pos, mass=mass, order=o).value)
            assert any(e[3] for e in window.bin_cache().entries), 'the tile-binned path was not taken'
            err = numpy.abs(binned - direct[o]).max()
            print('order %d: binned against direct %.2e of the largest cell %.3g' % (o, err / cell, cell))
            assert err <= 1e-12 * max(1.0, cell)
    finally:
        window.BINNED = old
        window.clear_bin_cache()


# ---- 5. ranks (both backends) --------------------------------------------------------------------------------------

@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [4]), (4, [2, 2])])
def test_ranks_equal_one(ibe, size, np_):
    from tests import thread_comm
    nmesh = [16, 16, 16]
    pos, mass = random_particles(ParticleMesh(nmesh, BoxSize=BOX), 3000, seed=51)
    S = scale_of(mass, nmesh)
    cases = [(2, 'cic', True), (3, 'tsc', False)]

    def run(pm, pos, mass, **kw):
        return [paint_interlaced(pm, pos, mass=mass, resampler=res, order=order, compensate=comp, **kw)
                for order, res, comp in cases]
    one = [cpu(f.value) for f in run(ParticleMesh(nmesh, BoxSize=BOX), pos, mass)]
    comp_min = numpy.abs(window_of([0] * 3, nmesh, nmesh, 2)).min()
    results, refused = {}, {}

    def body(comm):
        pm = ParticleMesh(nmesh, BoxSize=BOX, comm=comm, np=np_)
        mine = slice(comm.rank, None, comm.size)
        fields = run(pm, pos[mine], mass[mine])
        # a layout of the caller's with the smoothing the displaced windows need
        layout = pm.decompose(pos[mine], smoothing=0.5 * 3 + 2 / 3.)
        given = paint_interlaced(pm, pos[mine], mass=mass[mine], resampler='tsc', order=3, layout=layout)
        results[comm.rank] = [(f.slices, cpu(f.value)) for f in fields + [given]]
        # the routing of a plain paint does not reach the displaced windows
        try:
            paint_interlaced(pm, pos[mine], mass=mass[mine], layout=pm.decompose(pos[mine]))
        except ValueError as e:
            refused[comm.rank] = str(e)
    thread_comm.run_ranks(size, body)
    assert len(results) == size and len(refused) == size and all('smoothing' in r for r in refused.values())
    for blocks in results.values():
        for (sl, got), want, (order, res, comp) in zip(blocks, one + [one[1]], cases + [cases[1]]):
            tol = 1e-13 * S / (comp_min if comp else 1.0)
            assert numpy.abs(got - want[sl]).max() <= tol


def test_one_rank_layouts(ibe):
    """on one rank a layout is not needed; one that is given is held to the same smoothing"""
    pm = ParticleMesh(MESH, BoxSize=BOX)
    pos, mass = random_particles(pm, 200, seed=52)
    want = cpu(paint_interlaced(pm, pos, mass=mass).value)
    got = paint_interlaced(pm, pos, mass=mass, layout=pm.decompose(pos, smoothing=1.5))
    assert numpy.abs(cpu(got.value) - want).max() <= 1e-13 * scale_of(mass, MESH)
    with pytest.raises(ValueError, match='smoothing'):
        paint_interlaced(pm, pos, mass=mass, layout=pm.decompose(pos))
    with pytest.raises(ValueError, match='smoothing'):
        paint_interlaced(pm, pos, mass=mass, order=3, layout=pm.decompose(pos, smoothing=1.5))
    paint_interlaced(pm, pos, mass=mass, order=1, layout=pm.decompose(pos))


# ---- 6. downstream (both backends) ---------------------------------------------------------------------------------

def test_power_spectrum_of_the_cancelled_image(ibe):
    """the particles of the image (1, 0, 0) hold no power at any mode of the mesh: the interlaced, compensated spectrum
    has P below 1e-24 V S^2 in every bin ((1e-13 S)^2 over the window, at most 1 / 0.017^2 for CIC here), the plain
    compensated one has not"""
    pm = ParticleMesh(MESH, BoxSize=BOX, dtype='f8')
    pos, mass = image_particles(2, (1, 0, 0))
    S, V = scale_of(mass, MESH), float(numpy.prod(BOX))
    edges = kf_edges(pm)
    r = power_spectrum(paint_interlaced(pm, pos, mass=mass, compensate=True), edges)
    ok = r.modes > 0
    assert ok.sum() > 3
    print('interlaced: max P = %.3e V S^2' % (numpy.abs(r.power[ok]).max() / (V * S * S)))
    assert (numpy.abs(r.power[ok]) < 1e-24 * V * S * S).all()
    plain = power_spectrum(pm.paint(pos, mass=mass).r2c(), edges, deconv_pow=2)
    assert (plain.modes == r.modes).all()
    print('plain: max P = %.3e V S^2' % (numpy.abs(plain.power[ok]).max() / (V * S * S)))
    assert not (numpy.abs(plain.power[ok]) < 1e-24 * V * S * S).all()


def test_interlaced_field_feeds_survey_multipoles(ibe):
    pm = ParticleMesh((8, 8, 8), BoxSize=BOX, dtype='f8')
    pos, mass = random_particles(pm, 300, seed=61)
    F = interlaced_field(pm, pos, mass=numpy.abs(mass), resampler='tsc')
    assert isinstance(F, RealField)
    want = paint_interlaced(pm, pos, mass=numpy.abs(mass), resampler='tsc').c2r()
    assert numpy.abs(cpu(F.value) - cpu(want.value)).max() <= 1e-12 * numpy.abs(cpu(want.value)).max()
    # the mean survives: interlacing leaves the k = 0 mode as the paint made it
    assert abs(float(cpu(F.value).mean()) - numpy.abs(mass).sum() / 512.) <= 1e-12
    res = survey_multipoles(F, kf_edges(pm), (-30., 40., -250.), deconv_pow=3)
    ok = res.modes > 0
    for ell in (0, 2, 4):
        assert numpy.isfinite(res.poles[ell][ok]).all()
    assert (res.poles[0][ok].real[1:] > 0).all()


# ---- 7. arguments (both backends) ----------------------------------------------------------------------------------

def test_arguments(ibe):
    pm = ParticleMesh((8, 8, 8), BoxSize=100.)
    pos, mass = random_particles(pm, 50, seed=71)
    for bad in (0, 4, -1, 2.5, 'two', None):
        with pytest.raises(ValueError, match='order'):
            paint_interlaced(pm, pos, order=bad)
    with pytest.raises(ValueError, match='hsml'):
        paint_interlaced(pm, pos, hsml=numpy.ones(len(pos)))
    with pytest.raises(ValueError, match='hsml'):
        interlaced_field(pm, pos, hsml=1.0)
    with pytest.raises(ValueError, match='real mesh'):
        paint_interlaced(ParticleMesh((8, 8, 8), BoxSize=100., dtype='c16'), pos)
    for n in ([16], [4, 4, 4, 4]):
        with pytest.raises(NotImplementedError):
            paint_interlaced(ParticleMesh(n, BoxSize=10.), pos[:, :1].repeat(len(n), axis=1))
    with pytest.raises(TypeError):
        paint_interlaced(pm.create(type='real'), pos)
    # windows whose transform is no power of sinc
    for res in ('lanczos2', 'db6', window.FindResampler('cic').resize(4)):
        with pytest.raises(ValueError, match='sinc'):
            paint_interlaced(pm, pos, resampler=res, compensate=True)
    paint_interlaced(pm, pos, resampler=window.FindResampler('cic').resize(4))       # fine without compensation
    for bad in (pm.create(type='real'), ParticleMesh((8, 8, 16), BoxSize=100.).create(type='complex'), 3):
        with pytest.raises(ValueError, match='out'):
            paint_interlaced(pm, pos, out=bad)
    # phase_combine: fields of different meshes, kinds, dtypes
    A, B = pm.create(type='complex'), pm.create(type='complex')
    for other in (ParticleMesh((8, 8, 16), BoxSize=100.).create(type='complex'),
                  ParticleMesh((8, 8, 8), BoxSize=[100., 100., 50.]).create(type='complex')):
        with pytest.raises(ValueError, match='mesh'):
            phase_combine(A, other, 0.5)
    with pytest.raises(ValueError, match='dtype'):
        phase_combine(A, ParticleMesh((8, 8, 8), BoxSize=100., dtype='f4').create(type='complex'), 0.5)
    for bad in (pm.create(type='real'), numpy.zeros((8, 8, 5), dtype='c16'), None):
        with pytest.raises(TypeError):
            phase_combine(A, bad, 0.5)
        with pytest.raises(TypeError):
            phase_combine(bad, A, 0.5)
    for bad in ((0.5, 0.5), numpy.nan, 'half', (0.5, numpy.inf, 0.)):
        with pytest.raises(ValueError, match='shift'):
            phase_combine(A, B, bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='deconv_pow'):
            phase_combine(A, B, 0.5, deconv_pow=bad)


# ---- 8. resources (compiles for gfx950 on the CPU) -----------------------------------------------------------------

def test_interlace_kernels_compile_without_scratch():
    import os
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_interlace.hip')
    # phase_combine_kernel<T, ACC, DECONV> for f4 / f8, a == 0 / a != 0 and deconv_pow == 0 / > 0
    kernels = {k: v for k, v in t.items() if 'phase_combine_kernel' in k}
    assert len(kernels) == 8, sorted(t)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 128, (name, r)
