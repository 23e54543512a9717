"""The tile-binned (LDS-tiled) paint / readout kernels against the direct kernels,
the CPU oracle and size-independent properties.  GPU only: the binned path exists
only in the HIP library (there is nothing to test on the oracle double).

  * readout_binned == pmx_readout bit for bit (same per-particle summation order);
  * paint_binned == pmx_paint within the f8/f4 tolerance (the order of additions
    into a cell differs), and bit for bit on dyadic inputs (exact partial sums),
    which pins the cell indexing of the binning, the tile-local addressing, the
    owned/halo split and the periodic flush;
  * slab-local blocks (size < period, translate), non-periodic canvases, particles
    outside the box, random order, overwrite vs accumulate;
  * full-size properties at the BASELINE workload: mass conservation, paint
    linearity, readout of a constant field.
"""
import numpy
import pytest
import torch
from numpy.testing import assert_array_equal, assert_allclose

from pmesh_amd import window
from pmesh_amd.window import Affine, windows

pytestmark = pytest.mark.gpu

TUNED = ['nnb', 'cic', 'tsc', 'pcs']


@pytest.fixture
def hip():
    from pmesh_amd import backend
    backend.reset()
    b = backend.get()
    old, oldw, olds, olde, oldb = window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS
    yield b
    window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS = old, oldw, olds, olde, oldb
    window.clear_bin_cache()
    backend.reset()


@pytest.fixture(params=['tiles', 'sorted', 'chunks', 'blocks'])
def form(request, hip):
    """the forms of the binned kernels: the tile kernels through the index list
    (csrc/pmx_binned.hip), the tile kernels on the plan's tile-ordered copy of the positions, the
    tile kernels with the chunk form of the single-pass rebuild (bin_count_kernel<MODE 1> instead of
    bin_block_kernel, which 'tiles' takes), and the block entries (bin_entries_kernel, paint_entries_kernel,
    readout_entries_kernel) wherever they apply — CIC on a whole periodic mesh with dense rows of doubles; every other
    batch of that variant is served by the list, and check_form asserts which"""
    window.WALK = {'chunks': 'chunks'}.get(request.param, 'never')
    window.SORTED = 'always' if request.param == 'sorted' else 'never'
    window.BLOCKS = 'always' if request.param == 'blocks' else 'never'
    window.bin_cache().destroy(hip)          # (plan state of earlier tests is sticky: start from none)
    yield request.param
    window.bin_cache().destroy(hip)


def clear_plans():
    """forget the cached batches; under BLOCKS = 'always' the plans themselves, whose history a consumer of the index
    list has taken out of the entry form (pmx_binplan_blocks)"""
    if window.BLOCKS == 'always':
        from pmesh_amd import backend
        window.bin_cache().destroy(backend.get())
    else:
        window.clear_bin_cache()


def entries_apply(name, shape, period, ptype='f8'):
    """where the block-entry form serves: CIC, the whole periodic mesh, dense rows of doubles"""
    return name == 'cic' and tuple(shape) == tuple(period) and ptype == 'f8'


def check_form(form, entries):
    """in the 'blocks' variant: the plan used last is in block-entry form exactly when the form applies (read through
    pmx_binplan_blocks before any consumer of the index list has run)"""
    if form != 'blocks':
        return
    from pmesh_amd import backend
    cache = window.bin_cache()
    built = [e for e in cache.entries if e[3]]
    last = max(range(len(built)), key=lambda i: built[i][4])
    assert cache.block_plans(backend.get())[last][0] == entries, 'expected the %s' % (
        'block-entry form' if entries else 'index list')


def both(W, fn):
    """run fn under the direct and under the binned kernels"""
    window.BINNED = 'never'
    a = fn()
    window.BINNED = 'always'
    clear_plans()
    b = fn()
    return a, b


CASES = [
    # shape, period, scale, translate
    ((64, 64, 64), (64, 64, 64), 1.0, 0.0),                              # full periodic block
    ((40, 48, 96), (40, 48, 96), (0.5, 1.0, 0.75), (0.3, 0.0, -0.25)),   # anisotropic, several tiles
    ((24, 48, 64), (96, 48, 64), 1.0, (-32.0, 0.0, 0.0)),                # slab-local block of a bigger mesh
    ((24, 40, 70), (0, 0, 0), 1.0, 0.0),                                 # non periodic, ragged tiles
    ((20, 48, 45), (64, 0, 128), 1.0, (0.0, 2.0, -5.0)),                 # mixed
    ((24, 32, 96), (24, 32, 96), (0.25, 0.5, 1.5), (1.5, -0.75, 3.0)),   # whole periodic, 3 x 2 x 3 tiles
    ((16, 32, 64), (16, 32, 64), 1.0, 0.0),                              # whole periodic, the smallest: 2 x 2 x 2 tiles
]


def assert_binned_ran():
    assert any(e[3] for e in window.bin_cache().entries), 'the tile-binned path was not taken'


@pytest.mark.parametrize('name', TUNED)
@pytest.mark.parametrize('case', range(len(CASES)))
def test_binned_equals_direct(hip, form, oracle, name, case):
    window.EXACT = True            # the bit-identical form of the binned readout (pmx_binplan_exact)
    shape, period, scale, translate = CASES[case]
    W = windows[name]
    rs = numpy.random.RandomState(100 + case)
    n = 20000
    pos_h = rs.uniform(-40, 110, size=(n, 3))
    mass_h = rs.uniform(0.5, 1.5, size=n)
    aff = Affine(3, scale=scale, translate=translate, period=period)
    oaff = oracle.Affine(3, scale=scale, translate=translate, period=period)
    for dt, tdt, tol in (('f8', torch.float64, 1e-12), ('f4', torch.float32, 2e-6)):
        for ptype in ('f8', 'f4'):
            pos = torch.from_numpy(pos_h.astype(ptype)).to(hip.device)
            mass = torch.from_numpy(mass_h).to(hip.device)
            field_h = rs.normal(size=shape).astype(dt)
            field = torch.from_numpy(field_h).to(hip.device)
            for diffdir in (None, 1):
                def paint():
                    c = torch.zeros(shape, dtype=tdt, device=hip.device)
                    W.paint(c, pos, mass=mass, diffdir=diffdir, transform=aff)
                    return c.cpu().numpy()
                d, b = both(W, paint)
                assert_binned_ran()
                check_form(form, entries_apply(name, shape, period, ptype))
                s = max(1.0, abs(d).max())
                assert_allclose(b, d, rtol=0, atol=tol * s)
                if ptype == 'f8' and diffdir is None and dt == 'f8':
                    want = numpy.zeros(shape)
                    oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oaff)
                    assert_allclose(b, want, rtol=0, atol=tol * s)

                def readout():
                    return W.readout(field, pos, diffdir=diffdir, transform=aff).cpu().numpy()
                d, b = both(W, readout)
                assert_array_equal(b, d)                  # bit-identical gather
    # overwrite == zero + accumulate; accumulate really accumulates
    pos = torch.from_numpy(pos_h).to(hip.device)
    window.BINNED = 'always'
    clear_plans()
    c1 = torch.full(shape, 7.0, dtype=torch.float64, device=hip.device)
    W.paint(c1, pos, transform=aff, _overwrite=True)
    check_form(form, entries_apply(name, shape, period))
    c2 = torch.zeros(shape, dtype=torch.float64, device=hip.device)
    W.paint(c2, pos, transform=aff)
    assert_allclose(c1.cpu().numpy(), c2.cpu().numpy(), rtol=0, atol=1e-12 * max(1, float(c2.abs().max())))
    c3 = torch.full(shape, 7.0, dtype=torch.float64, device=hip.device)
    W.paint(c3, pos, transform=aff)
    assert_allclose(c3.cpu().numpy(), c2.cpu().numpy() + 7.0, rtol=0, atol=1e-11)


@pytest.mark.parametrize('name', ['cic', 'tsc', 'pcs'])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_default_readout_within_tolerance_of_the_exact_form(hip, form, oracle, name, case):
    """The DEFAULT binned readout (window.EXACT = False): the cell indices are the reference's bit for bit, the
    weights come from FMA polynomials in the canvas' precision and the S^3 products are summed as nested FMAs.
    Against the oracle (= the exact form) on every geometry of CASES, f8 / f4 canvases, f8 / f4 positions, plain and
    gradient weights: within 1e-13 (f8 canvas) / 2e-6 (f4 canvas) of the largest |cell| x the bound of the
    weights' absolute sum — and WHICH particles read zero (dropped outside the block) is the same exactly."""
    shape, period, scale, translate = CASES[case]
    W = windows[name]
    rs = numpy.random.RandomState(300 + case)
    n = 20000
    pos_h = rs.uniform(-40, 110, size=(n, 3))
    aff = Affine(3, scale=scale, translate=translate, period=period)
    oaff = oracle.Affine(3, scale=scale, translate=translate, period=period)
    window.BINNED = 'always'
    for dt, tdt, tol in (('f8', torch.float64, 1e-13), ('f4', torch.float32, 2e-6)):
        field_h = rs.normal(size=shape).astype(dt)
        field = torch.from_numpy(field_h).to(hip.device)
        for ptype in ('f8', 'f4'):
            ph = pos_h.astype(ptype)
            pos = torch.from_numpy(ph).to(hip.device)
            for diffdir in (None, 1):
                want = oracle.Window(W.kind).readout(field_h, ph, diffdir=diffdir, transform=oaff)
                window.EXACT = False
                clear_plans()
                got = W.readout(field, pos, diffdir=diffdir, transform=aff).cpu().numpy()
                assert_binned_ran()
                check_form(form, entries_apply(name, shape, period, ptype))
                window.EXACT = True
                clear_plans()
                exact = W.readout(field, pos, diffdir=diffdir, transform=aff).cpu().numpy()
                assert_array_equal(exact, want)
                sc = numpy.atleast_1d(numpy.asarray(scale, dtype='f8'))
                wb = 1.0 if diffdir is None else 2.0 * abs(sc[min(diffdir, len(sc) - 1)]) + 2.0
                assert_allclose(got, want, rtol=0, atol=tol * wb * abs(field_h).max())
                assert_array_equal(got == 0, want == 0)
                if dt == 'f8':
                    assert abs(got - want).max() > 0 or name == 'cic'        # (it IS another arithmetic)


@pytest.mark.parametrize('name', ['cic', 'tsc', 'pcs'])
@pytest.mark.parametrize('period', [(16, 32, 256), (0, 0, 0)])
def test_sparse_clusters_across_tile_faces(hip, form, oracle, name, period):
    """paint_tile_kernel carries the z-halo of a tile in LDS into the next tile of its z segment
    (4 tiles) and stages it only at the end of a segment.  Small clusters that straddle a z face
    inside a segment, at a segment end and at the periodic wrap, with every other tile EMPTY (the
    tile behind a cluster is processed only because of the carry), accumulate (hold) and overwrite
    mode: dyadic positions and masses, so CIC and TSC must equal the oracle bit for bit."""
    shape = (16, 32, 256)           # 2 x 2 x 8 tiles of 8 x 16 x 32: two z segments per column
    W = windows[name]
    aff = Affine(3, scale=1.0, translate=0.0, period=period)
    oaff = oracle.Affine(3, scale=1.0, translate=0.0, period=period)
    rs = numpy.random.RandomState(3)
    for zc in (31.5, 32.0, 63.75, 127.5, 128.0, 255.5, 0.25, 95.0, 223.5):
        # a cluster of 200 particles within +-1.5 cells of z = zc in ONE (x, y) tile column
        pos_h = numpy.empty((200, 3))
        pos_h[:, 0] = 3.0 + rs.randint(0, 32, size=200) / 16.0
        pos_h[:, 1] = 20.0 + rs.randint(0, 64, size=200) / 16.0
        pos_h[:, 2] = (zc + rs.randint(-24, 25, size=200) / 16.0) % 256
        mass_h = rs.randint(1, 5, size=200).astype('f8')
        pos = torch.from_numpy(pos_h).to(hip.device)
        mass = torch.from_numpy(mass_h).to(hip.device)
        base = rs.randint(-3, 4, size=shape).astype('f8')
        want = base.copy()
        oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oaff)
        window.BINNED = 'always'
        clear_plans()
        c = torch.from_numpy(base.copy()).to(hip.device)
        W.paint(c, pos, mass=mass, transform=aff)                       # accumulate
        assert_binned_ran()
        check_form(form, entries_apply(name, shape, period))
        # (the cubic weights carry a 1/6: exact sums only for CIC and TSC)
        check = assert_array_equal if name != 'pcs' else (lambda a, b: assert_allclose(a, b, rtol=0, atol=1e-12))
        check(c.cpu().numpy(), want)
        c = torch.full(shape, 9.0, dtype=torch.float64, device=hip.device)
        W.paint(c, pos, mass=mass, transform=aff, _overwrite=True)      # every cell written once
        check(c.cpu().numpy(), want - base)


@pytest.mark.parametrize('name', ['cic', 'tsc', 'pcs'])
def test_crowded_tile_is_split(hip, oracle, name):
    """A tile that holds many times the mean population (a halo) is cut into pieces for separate
    workgroups (paint_heavy_kernel / readout_heavy_kernel: everything beyond the first 16384 list
    entries): 70000 particles inside one tile and across its faces, 2000 elsewhere; dyadic positions
    and masses, so CIC / TSC paint must equal the oracle bit for bit, accumulate and overwrite;
    readout bit-identical."""
    window.EXACT = True            # the bit-identical form of the binned readout (pmx_binplan_exact)
    W = windows[name]
    N = 64
    rs = numpy.random.RandomState(12)
    heavy = numpy.stack([rs.randint(8 * 16, 18 * 16, size=70000), rs.randint(16 * 16, 34 * 16, size=70000),
                         rs.randint(30 * 16, 66 * 16, size=70000)], axis=1) / 16.0
    pos_h = numpy.concatenate([heavy, rs.randint(0, N * 16, size=(2000, 3)) / 16.0])
    mass_h = rs.randint(1, 5, size=len(pos_h)).astype('f8')
    aff, oaff = Affine(3, period=N), oracle.Affine(3, period=N)
    base = rs.randint(-3, 4, size=(N, N, N)).astype('f8')
    want = base.copy()
    oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oaff)
    window.BINNED, window.WALK = 'always', 'never'
    check = assert_array_equal if name != 'pcs' else (lambda a, b: assert_allclose(a, b, rtol=0, atol=1e-10))
    for srt in ('never', 'always'):
        window.SORTED = srt
        window.clear_bin_cache()
        pos = torch.from_numpy(pos_h).to(hip.device)
        mass = torch.from_numpy(mass_h).to(hip.device)
        c = torch.from_numpy(base.copy()).to(hip.device)
        W.paint(c, pos, mass=mass, transform=aff)
        assert_binned_ran()
        check(c.cpu().numpy(), want)
        c = torch.full((N, N, N), 9.0, dtype=torch.float64, device=hip.device)
        W.paint(c, pos, mass=mass, transform=aff, _overwrite=True)
        check(c.cpu().numpy(), want - base)
        field_h = rs.normal(size=(N, N, N))
        got = W.readout(torch.from_numpy(field_h).to(hip.device), pos, transform=aff).cpu().numpy()
        assert_array_equal(got, oracle.Window(W.kind).readout(field_h, pos_h, transform=oaff))


@pytest.mark.parametrize('name', ['tsc', 'pcs'])
@pytest.mark.parametrize('case', ['one_cell', 'blob', 'signed', 'gradient', 'big_masses', 'tiny_masses'])
def test_float_canvas_regions_retry_on_overflow(hip, oracle, name, case):
    """[r5] The 32-bit fixed-point regions of float canvases (paint_tile32_kernel): the scale is optimistic (room for 16 x
    the mean density of a segment's tiles), every add is checked through the value the atomic returns, and a tile that
    comes within a factor 2 of the 32 bits is deposited again IN TWO PARTS at the same scale (v >> sh, flushed, then
    v & (2^sh - 1) added on top: every contribution still rounded once to 2^-f) — here made to happen: thousands of
    particles on ONE cell (identical contributions: their roundings do not cancel, the case that a coarser retry scale
    fails) / in a tight blob inside an otherwise thin set, masses of either sign and derivative weights (the signed
    guard), masses of 1e6 and 1e-9 (the scale follows the largest |mass|).  Against the oracle within the tolerance of a float canvas; the sum of the mesh to 1e-6
    of the summed |mass|."""
    W = windows[name]
    N = 64
    rs = numpy.random.RandomState({'one_cell': 1, 'blob': 2, 'signed': 3, 'gradient': 4, 'big_masses': 5, 'tiny_masses': 6}[case])
    thin = rs.uniform(0, N, size=(30000, 3))
    if case == 'one_cell':
        dense = numpy.tile(numpy.array([[20.3, 33.6, 40.2]]), (12000, 1))
    else:
        dense = numpy.array([[20.3, 33.6, 40.2]]) + rs.normal(scale=0.7, size=(15000, 3))
    pos_h = numpy.concatenate([thin, dense]).astype('f4')
    mass_h = rs.uniform(0.5, 1.5, size=len(pos_h))
    diffdir = None
    if case == 'signed':
        mass_h *= rs.choice([-1.0, 1.0], size=len(pos_h))
    elif case == 'gradient':
        diffdir = 1
    elif case == 'big_masses':
        mass_h *= 1.0e6
    elif case == 'tiny_masses':
        mass_h *= 1.0e-9
    aff, oaff = Affine(3, period=N), oracle.Affine(3, period=N)
    want = numpy.zeros((N, N, N))
    oracle.Window(W.kind).paint(want, pos_h.astype('f8'), mass=mass_h, transform=oaff, diffdir=diffdir)
    window.BINNED = 'always'
    pos = torch.from_numpy(pos_h).to(hip.device)
    mass = torch.from_numpy(mass_h).to(hip.device)
    got = []
    for scalar in (False, True):
        if scalar and case in ('signed', 'big_masses', 'tiny_masses'):
            continue
        for _ in range(2):
            window.clear_bin_cache()
            c = torch.zeros((N, N, N), dtype=torch.float32, device=hip.device)
            W.paint(c, pos, mass=None if scalar else mass, diffdir=diffdir, transform=aff)
            assert_binned_ran()
            got.append(c.cpu().numpy().astype('f8'))
        w = want
        if scalar:
            w = numpy.zeros((N, N, N))
            oracle.Window(W.kind).paint(w, pos_h.astype('f8'), transform=oaff, diffdir=diffdir)
        # (two runs agree to the rounding of the float adds that merge the staged halo cells: the REGION sums are integers)
        assert_allclose(got[-1], got[-2], rtol=0, atol=2.5e-7 * max(1.0, abs(got[-1]).max()))
        scale = abs(w).max()
        assert scale > 100 * (abs(mass_h).mean() if not scalar else 1.0) or case in ('gradient', 'signed')     # the blob really is a blob
        assert_allclose(got[-1], w, rtol=0, atol=2e-6 * max(1.0, scale) if case != 'tiny_masses' else 2e-6 * scale)
        if diffdir is None and case != 'signed':
            total = mass_h.sum() if not scalar else float(len(pos_h))
            assert abs(got[-1].sum() - total) <= 1e-6 * abs(total) + 1e-5 * scale


@pytest.mark.parametrize('name', ['nnb', 'cic', 'tsc'])
def test_binned_dyadic_bit_exact(hip, form, oracle, name):
    """positions on a 1/16-cell lattice, small integer masses: exact partial sums =>
    the binned scatter must reproduce the reference bit for bit (indexing parity)."""
    W = windows[name]
    rs = numpy.random.RandomState(4)
    N = 64
    pos_h = rs.randint(-64 * 16, 3 * N * 16, size=(50000, 3)) / 16.0
    mass_h = rs.randint(1, 5, size=len(pos_h)).astype('f8')
    want = numpy.zeros((N, N, N))
    oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oracle.Affine(3, period=N))
    window.BINNED = 'always'
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    W.paint(c, torch.from_numpy(pos_h).to(hip.device), mass=torch.from_numpy(mass_h).to(hip.device),
            transform=Affine(3, period=N))
    assert_binned_ran()
    check_form(form, entries_apply(name, (N, N, N), (N, N, N)))
    assert_array_equal(c.cpu().numpy(), want)


def test_sorted_copy_is_chosen_for_incoherent_rows(hip, oracle):
    """SORTED='auto': rows in lattice order keep the index list, the same rows shuffled make the first build
    of the plan switch to the tile-ordered copy; results are the same either way."""
    import ctypes as C
    from pmesh_amd._arrays import vec
    N, L = 128, 1000.0
    W = windows['tsc']
    window.BINNED, window.WALK, window.SORTED = 'always', 'never', 'auto'
    pos = torch.empty((N ** 3, 3), dtype=torch.float64, device=hip.device)
    pv = vec(pos)
    hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, N ** 3, hip.stream())
    aff = Affine(3, scale=N / L, period=N)
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(7)
    perm = torch.randperm(N ** 3, device=hip.device, generator=gen)
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    res = []
    # (rows only PARTLY out of order — the lattice with two cells of jitter, 28 breaks of the tile sequence per 64 rows —
    # keep the index list: measured, scripts/r05/order_threshold.sh, the copy only pays for rows in no order at all)
    jittered = pos + torch.randn(pos.shape, dtype=torch.float64, device=hip.device, generator=gen) * (2.0 * L / N)
    for p, want_sorted in ((pos, 0), (pos[perm].contiguous(), 1), (jittered, 0)):
        for build in range(3):
            # (a plan that is rebuilt from its history learns of a change of the row order one build late)
            window.clear_bin_cache()
            c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
            W.paint(c, p, transform=aff)
            torch.cuda.synchronize()
        assert window.bin_cache().sorted_plans(hip) == want_sorted, (want_sorted, window.bin_cache().entries)
        res.append((c, W.readout(field, p, transform=aff)))
    assert float((res[0][0] - res[1][0]).abs().max()) <= 1e-12 * float(res[0][0].abs().max())
    assert torch.equal(res[0][1][perm], res[1][1])              # readout: bit-identical, row by row


def test_plan_survives_a_changing_particle_count(hip, oracle):
    """A rank of a time-stepping run gains and loses a few particles every step (they migrate between ranks): a new
    position tensor of a slightly different length takes over the plan of the previous step and rebuilds it in ONE
    pass (pmx_binplan_builds), as long as the count stays within an eighth of the previous one; a jump starts over.
    Results are those of the direct kernels every time.  (The reference keeps no state between calls: pm.py:1795-1869.)"""
    import ctypes as C
    W = windows['cic']
    window.BINNED = 'always'
    window.clear_bin_cache()
    window.bin_cache().destroy(hip)
    N = 64
    aff = Affine(3, period=N)
    rs = numpy.random.RandomState(12)
    allpos = torch.from_numpy(rs.uniform(0, N, size=(260000, 3))).to(hip.device)
    field = torch.from_numpy(rs.normal(size=(N, N, N))).to(hip.device)

    def builds():
        tot = [0, 0]
        for e in window.bin_cache().entries:
            a, b = C.c_uint32(0), C.c_uint32(0)
            hip.call('binplan_builds', e[1], C.byref(a), C.byref(b))
            tot[0] += int(a.value)
            tot[1] += int(b.value)
        return tot
    counts = [200000, 200700, 199100, 203000, 215000, 260000, 259000]
    want_single = [False, True, True, True, True, False, True]          # (260000 is 21 % more than 215000: starts over)
    for n, single in zip(counts, want_single):
        before = builds()
        pos = (allpos[:n] + 0.01).contiguous()            # a new tensor every step, the old one dropped
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, transform=aff)
        got = W.readout(field, pos, transform=aff)
        after = builds()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if single else (0, 1)), (n, before, after)
        window.BINNED = 'never'
        c2 = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c2, pos, transform=aff)
        want = W.readout(field, pos, transform=aff)
        window.BINNED = 'always'
        assert float((c - c2).abs().max()) <= 1e-12 * float(c2.abs().max())
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        del pos
    assert len(window.bin_cache().entries) <= 2          # (the jump opened a second plan; the steps around it reuse theirs)


def test_plan_is_shared_and_invalidated(hip):
    """paint and readout on the same position tensor share one plan; an in-place change of
    the positions (version counter) rebuilds it."""
    W = windows['cic']
    window.BINNED = 'always'
    window.clear_bin_cache()
    rs = numpy.random.RandomState(1)
    pos = torch.from_numpy(rs.uniform(0, 64, size=(5000, 3))).to(hip.device)
    aff = Affine(3, period=64)
    c = torch.zeros((64, 64, 64), dtype=torch.float64, device=hip.device)
    W.paint(c, pos, transform=aff)
    assert_binned_ran()
    built = [e[3] for e in window.bin_cache().entries]
    W.readout(c, pos, transform=aff)
    assert [e[3] for e in window.bin_cache().entries] == built
    keys = [e[0] for e in window.bin_cache().entries]
    pos += 1.0                                    # in place: version changes
    c2 = torch.zeros((64, 64, 64), dtype=torch.float64, device=hip.device)
    W.paint(c2, pos, transform=aff)
    assert [e[0] for e in window.bin_cache().entries] != keys
    window.BINNED = 'never'
    c3 = torch.zeros((64, 64, 64), dtype=torch.float64, device=hip.device)
    W.paint(c3, pos, transform=aff)
    assert_allclose(c2.cpu().numpy(), c3.cpu().numpy(), rtol=0, atol=1e-12 * float(c3.abs().max()))


@pytest.mark.parametrize('name', ['cic', 'tsc'])
def test_stale_plan_is_counted_warned_and_rebuilt(hip, oracle, name):
    """Positions rewritten in place WITHOUT torch noticing (through `.data`: the version counter of the tensor the
    cache keys on does not move): the plan is for other positions.  On a block that is not the whole periodic mesh the
    tile kernels skip — and count — the particles they find outside the region their list entry names
    (pmx_binplan_stale); the next use of the plan warns and rebuilds it, and is right again."""
    W = windows[name]
    window.BINNED = 'always'
    window.clear_bin_cache()
    shape, period, scale, translate = CASES[2]                  # a slab-local block of a bigger mesh
    aff = Affine(3, scale=scale, translate=translate, period=period)
    oaff = oracle.Affine(3, scale=scale, translate=translate, period=period)
    rs = numpy.random.RandomState(77)
    pos_h = rs.uniform(30, 60, size=(20000, 3))
    pos = torch.from_numpy(pos_h).to(hip.device)
    field_h = rs.normal(size=shape)
    field = torch.from_numpy(field_h).to(hip.device)
    a = W.readout(field, pos, transform=aff).cpu().numpy()
    assert_binned_ran()
    v = pos._version
    pos.data.add_(17.0)                                         # behind the cache's back
    assert pos._version == v
    W.readout(field, pos, transform=aff)                        # the stale plan: skips what left its regions, memory-safe
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match='stale bin plan'):
        b = W.readout(field, pos, transform=aff).cpu().numpy()
    want = oracle.Window(W.kind).readout(field_h, pos_h + 17.0, transform=oaff)
    assert_allclose(b, want, rtol=0, atol=1e-12 * abs(field_h).max() * 8)
    assert abs(a - b).max() > 0


@pytest.mark.parametrize('name,dt', [('cic', 'f8'), ('tsc', 'f4'), ('pcs', 'f8'), ('nnb', 'f8')])
def test_deterministic_paint(hip, oracle, name, dt):
    """window.DETERMINISTIC (the reference's scatter is a serial loop, _window.pyx:157-165: same call, same bits):
    every sum of the paint is a 64-bit integer, so the result is the same bit for bit run after run AND for any
    order of the rows; hold / overwrite, per-particle masses of both signs, crowded cells, slab-local blocks;
    within 1e-12 (f8) of the oracle; a NaN mass falls back to the floating-point kernels and poisons only its cells"""
    W = windows[name]
    tdt = torch.float64 if dt == 'f8' else torch.float32
    saved = window.DETERMINISTIC
    try:
        for shape, period, scale, translate in (((64, 64, 64), (64, 64, 64), 1.0, 0.0), ((24, 48, 64), (96, 48, 64), 1.0, (-32.0, 0.0, 0.0))):
            rs = numpy.random.RandomState(17)
            n = 120000
            pos_h = numpy.concatenate([rs.uniform(-10, 100, size=(n - 30000, 3)), rs.normal(40.0, 0.7, size=(30000, 3))])
            mass_h = rs.uniform(-1.0, 3.0, size=n)
            aff = Affine(3, scale=scale, translate=translate, period=period)
            oaff = oracle.Affine(3, scale=scale, translate=translate, period=period)
            pos = torch.from_numpy(pos_h).to(hip.device)
            mass = torch.from_numpy(mass_h).to(hip.device)
            perm = torch.randperm(n, device=hip.device)
            pos2, mass2 = pos[perm].contiguous(), mass[perm].contiguous()
            window.BINNED = 'always'
            for hold in (False, True):
                outs = []
                for P, M in ((pos, mass), (pos, mass), (pos2, mass2)):
                    window.DETERMINISTIC = True
                    window.clear_bin_cache()
                    c = torch.full(shape, 0.5 if hold else 7.0, dtype=tdt, device=hip.device)
                    W.paint(c, P, mass=M, transform=aff, _overwrite=not hold)
                    outs.append(c)
                assert torch.equal(outs[0], outs[1]), 'two runs differ'
                assert torch.equal(outs[0], outs[2]), 'the order of the rows matters'
                want = numpy.full(shape, 0.5 if hold else 0.0)
                oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oaff)
                tol = 1e-12 if dt == 'f8' else 2e-6
                assert_allclose(outs[0].cpu().numpy().astype('f8'), want, rtol=0, atol=tol * max(1.0, abs(want).max()))
            # scalar mass
            window.clear_bin_cache()
            a = torch.zeros(shape, dtype=tdt, device=hip.device)
            b = torch.zeros(shape, dtype=tdt, device=hip.device)
            W.paint(a, pos, mass=2.5, transform=aff)
            W.paint(b, pos2, mass=2.5, transform=aff)
            assert torch.equal(a, b)
        # a NaN mass: the floating-point kernels serve the batch, the NaN stays in its own cells
        window.clear_bin_cache()
        mass_bad = mass.clone()
        mass_bad[5] = float('nan')
        c = torch.zeros((64, 64, 64), dtype=tdt, device=hip.device)
        W.paint(c, pos, mass=mass_bad, transform=Affine(3, period=64))
        nbad = int(torch.isnan(c).sum())
        assert 1 <= nbad <= W.support ** 3, nbad
    finally:
        window.DETERMINISTIC = saved
        window.clear_bin_cache()


@pytest.mark.parametrize('name', ['tsc', 'pcs'])
@pytest.mark.parametrize('scale_m', [1e-290, 1.0, 1e250])
def test_fixed_point_regions_over_the_range_of_masses(hip, oracle, name, scale_m):
    """the S >= 3 paint accumulates 64-bit integers in units of 2^-f chosen from the largest |mass|: masses of
    1e-290 and of 1e250, scalar and per particle, gradient paint (derivative weights carry the scale), against the
    oracle to 1e-12 of the largest cell"""
    W = windows[name]
    N = 64
    rs = numpy.random.RandomState(23)
    pos_h = rs.uniform(0, 64, size=(50000, 3))
    mass_h = rs.uniform(0.1, 1.0, size=50000) * scale_m
    aff = Affine(3, scale=3.0, period=N * 3)
    oaff = oracle.Affine(3, scale=3.0, period=N * 3)
    shape = (3 * N, 3 * N, 3 * N)
    pos = torch.from_numpy(pos_h).to(hip.device)
    window.BINNED = 'always'
    for mass, mh in ((torch.from_numpy(mass_h).to(hip.device), mass_h), (0.7 * scale_m, 0.7 * scale_m)):
        for diffdir in (None, 2):
            window.clear_bin_cache()
            c = torch.zeros(shape, dtype=torch.float64, device=hip.device)
            W.paint(c, pos, mass=mass, diffdir=diffdir, transform=aff)
            assert_binned_ran()
            want = numpy.zeros(shape)
            oracle.Window(W.kind).paint(want, pos_h, mass=mh, diffdir=diffdir, transform=oaff)
            assert_allclose(c.cpu().numpy(), want, rtol=0, atol=1e-12 * abs(want).max())


@pytest.mark.parametrize('name', ['tsc', 'pcs'])
@pytest.mark.parametrize('ratio', [1e-3, 1e-6, 1e-7, 1e-20])
def test_fixed_point_regions_with_two_species(hip, oracle, name, ratio):
    """per-particle masses of two species in ONE batch, heavy (1) in one half of the box and light (ratio) in the
    other, so that there are cells only light particles reach.  The fixed-point regions take their unit from the
    LARGEST |mass| (2^-50 of it per contribution): up to a spread of 2^20 the batch stays in fixed point and every
    cell is within 64 adds x 2^-50 x max |m| of the oracle (the bound INTEGRATION.md section 1 states); beyond it
    the floating-point form of the kernels serves the batch and every cell — also those of the light species alone,
    20 decades below the heavy one — agrees to 1e-12 of ITS OWN sum, as with the reference's floating adds.  The
    statistics come from pmx_mass_stats (mass tensors) and from the paint's own pass (numpy masses)."""
    W = windows[name]
    N = 64
    rs = numpy.random.RandomState(29)
    n = 60000
    pos_h = rs.uniform(0, N, size=(n, 3))
    heavy = pos_h[:, 0] < N / 2
    pos_h[heavy, 0] = rs.uniform(4, N / 2 - 4, size=int(heavy.sum()))           # (a gap of 8 cells between the species)
    pos_h[~heavy, 0] = rs.uniform(N / 2 + 4, N - 4, size=int((~heavy).sum()))
    mass_h = numpy.where(heavy, 1.0, ratio)
    aff = Affine(3, period=N)
    oaff = oracle.Affine(3, period=N)
    want = numpy.zeros((N, N, N))
    oracle.Window(W.kind).paint(want, pos_h, mass=mass_h, transform=oaff)
    light_cells = numpy.zeros((N, N, N), dtype=bool)
    light_cells[N // 2 + 2:N - 2] = True
    assert (want[light_cells] > 0).mean() > 0.5 and want[light_cells].max() < 100 * ratio
    pos = torch.from_numpy(pos_h).to(hip.device)
    window.BINNED = 'always'
    for mass in (torch.from_numpy(mass_h).to(hip.device), mass_h):
        window.clear_bin_cache()
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, mass=mass, transform=aff)
        assert_binned_ran()
        got = c.cpu().numpy()
        err = abs(got - want)
        if ratio >= 2.0 ** -20:
            assert (err <= 64 * 2.0 ** -50 + 1e-13 * want).all(), err.max()
        else:
            assert (err <= 1e-12 * want).all(), (err / numpy.maximum(want, 1e-300)).max()


def test_two_live_particle_sets_keep_their_plans(hip):
    """two live position tensors of equal shape on one geometry (two species; probes at as many points
    as there are particles) each keep a plan slot: alternating between them finds both plans again
    instead of stealing and rebuilding; a tensor the caller dropped hands its plan to the next one"""
    W = windows['cic']
    N, n = 64, 50000
    window.BINNED = 'always'
    window.clear_bin_cache()
    aff = Affine(3, period=N)
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(5)
    a = torch.rand((n, 3), dtype=torch.float64, device=hip.device, generator=gen) * N
    b = torch.rand((n, 3), dtype=torch.float64, device=hip.device, generator=gen) * N
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    W.paint(c, a, transform=aff)
    W.paint(c, b, transform=aff)
    cache = window.bin_cache()
    keys = sorted(str(e[0]) for e in cache.entries if e[3])
    assert len(keys) == 2
    W.readout(c, a, transform=aff)
    W.readout(c, b, transform=aff)
    W.paint(c, a, transform=aff)
    assert sorted(str(e[0]) for e in cache.entries if e[3]) == keys      # nothing was rebuilt
    assert abs(float(c.sum()) - 3 * n) < 1e-6
    # a time-stepping caller: the new tensor replaces the old one, which nobody holds any more
    plan_of_a = [e[1].value for e in cache.entries if e[2] is a][0]
    a = a + 0.01
    W.paint(c, a, transform=aff)
    assert [e[1].value for e in cache.entries if e[2] is a] == [plan_of_a]
    with torch.inference_mode():                      # tensors without a version counter: never cached, never fail
        q = torch.rand((n, 3), dtype=torch.float64, device=hip.device) * N
        out = torch.empty(n, dtype=torch.float64, device=hip.device)
        one = torch.ones((N, N, N), dtype=torch.float64, device=hip.device)
        W.readout(one, q, transform=aff, out=out)
        assert float((out - 1).abs().max()) < 1e-13


@pytest.mark.parametrize('name', ['nnb', 'cic', 'tsc', 'pcs'])
def test_rebuild_from_history_and_overflow(hip, form, oracle, name):
    """A plan that already served the same geometry and particle count rebuilds in a single
    pass into the slot ranges of its previous build (time-stepping callers).  Results must
    not depend on that: (1) slightly moved particles (ranges hold), (2) a completely different
    distribution of the same size (ranges overflow -> exact two-pass build on the device),
    (3) the builds after the overflow (back-off), all against the oracle; readout bit-exact.  In the 'blocks' variant
    the readout is the default one (the exact form reads the index list: the plan would leave the entry form for good),
    within the bound of test_default_readout_within_tolerance_of_the_exact_form, and CIC keeps the entries throughout."""
    window.EXACT = form != 'blocks'    # the bit-identical form of the binned readout (pmx_binplan_exact)
    W = windows[name]
    N, n = 64, 60000
    window.BINNED = 'always'
    clear_plans()
    aff = Affine(3, period=N)
    oaff = oracle.Affine(3, period=N)
    rs = numpy.random.RandomState(11)
    field_h = rs.normal(size=(N, N, N))
    field = torch.from_numpy(field_h).to(hip.device)
    base = rs.uniform(0, N, size=(n, 3))
    clustered = numpy.concatenate([rs.normal(20.0, 1.5, size=(n - 100, 3)), rs.uniform(-N, 2 * N, size=(100, 3))])
    steps = [base, base + rs.normal(0, 0.05, size=(n, 3)), clustered, clustered + 0.01, base, base + 0.02,
             clustered, base]
    pos = torch.zeros((n, 3), dtype=torch.float64, device=hip.device)
    for k, ph in enumerate(steps):
        pos.copy_(torch.from_numpy(ph))               # in place: same tensor, new version -> rebuild
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, transform=aff)
        assert_binned_ran()
        check_form(form, entries_apply(name, (N, N, N), (N, N, N)))
        want = numpy.zeros((N, N, N))
        oracle.Window(W.kind).paint(want, ph, transform=oaff)
        assert_allclose(c.cpu().numpy(), want, rtol=0, atol=1e-12 * abs(want).max(), err_msg='step %d' % k)
        got = W.readout(field, pos, transform=aff).cpu().numpy()
        want = oracle.Window(W.kind).readout(field_h, ph, transform=oaff)
        if window.EXACT:
            assert_array_equal(got, want, err_msg='step %d' % k)
        else:
            assert_allclose(got, want, rtol=0, atol=1e-13 * abs(field_h).max(), err_msg='step %d' % k)
            assert_array_equal(got == 0, want == 0)
        check_form(form, entries_apply(name, (N, N, N), (N, N, N)))
        if k == 0:
            serving = [e[1].value for e in window.bin_cache().entries if e[3]]
        # one plan (the pool keeps earlier ones) served every step
        assert [e[1].value for e in window.bin_cache().entries if e[3]] == serving


@pytest.mark.parametrize('name,strided,n', [('cic', False, 100000), ('pcs', False, 100000), ('tsc', True, 70001), ('cic', True, 5)])
def test_block_rebuild_with_more_tiles_than_table_entries(hip, oracle, name, strided, n, monkeypatch):
    """the block form of the single-pass rebuild counts a block of 4096 rows per tile in an LDS table
    of 128 entries; rows in random order over a 128^3 mesh (512 tiles) overflow it, and the groups
    that find no entry go to the global counters themselves"""
    window.EXACT = True            # the bit-identical form of the binned readout (pmx_binplan_exact)
    W = windows[name]
    N = 128
    window.BINNED, window.WALK, window.SORTED = 'always', 'never', 'never'
    window.clear_bin_cache()
    aff = Affine(3, period=N)
    oaff = oracle.Affine(3, period=N)
    rs = numpy.random.RandomState(8)
    field_h = rs.normal(size=(N, N, N))
    field = torch.from_numpy(field_h).to(hip.device)
    # strided: rows of a wider array (the kernel's path without the dense staging), a row count that
    # is no multiple of anything, and a batch far smaller than one block
    pos = (torch.zeros((n, 5), dtype=torch.float64, device=hip.device)[:, 1:4] if strided
           else torch.zeros((n, 3), dtype=torch.float64, device=hip.device))
    ph = rs.uniform(0, N, size=(n, 3))
    for k in range(3):
        ph = ph + rs.normal(0, 0.2, size=(n, 3))
        pos.copy_(torch.from_numpy(ph))
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, transform=aff)
        want = numpy.zeros((N, N, N))
        oracle.Window(W.kind).paint(want, ph, transform=oaff)
        assert_allclose(c.cpu().numpy(), want, rtol=0, atol=1e-12 * abs(want).max(), err_msg='step %d' % k)
        got = W.readout(field, pos, transform=aff).cpu().numpy()
        assert_array_equal(got, oracle.Window(W.kind).readout(field_h, ph, transform=oaff), err_msg='step %d' % k)
    assert window.bin_cache().overflows(hip) >= 0


@pytest.mark.parametrize('seed', range(int(__import__('os').environ.get('PMESH_AMD_FUZZ_SEEDS', '10'))))
def test_random_geometries_over_moving_particles(hip, seed):
    """Randomly drawn block geometries — extents that are and are not multiples of the tile, every axis
    the whole periodic mesh / a block of a bigger periodic mesh / not periodic, scales and translations,
    particles partly outside — over three steps of moving particles (first build, then single-pass
    rebuilds): binned paint equals direct paint within the fp64 tolerance, binned readout equals direct
    readout bit for bit."""
    window.EXACT = True            # the bit-identical form of the binned readout (pmx_binplan_exact)
    rs = numpy.random.RandomState(1000 + seed)
    name = TUNED[seed % 4]
    W = windows[name]
    S = {'nnb': 1, 'cic': 2, 'tsc': 3, 'pcs': 4}[name]
    T = (8, 16, 32)
    shape, period = [], []
    for d in range(3):
        kind = rs.randint(3)
        if kind == 0:                                   # the whole periodic mesh: a multiple of the tile
            n = T[d] * rs.randint(2, 5)
            shape.append(n); period.append(n)
        elif kind == 1:                                 # a block of a bigger periodic mesh
            n = rs.randint(T[d] + S, 3 * T[d] + 5)
            shape.append(n); period.append(n + rs.randint(S, 40))
        else:                                           # not periodic
            shape.append(rs.randint(T[d] + S, 3 * T[d] + 5)); period.append(0)
    scale = rs.uniform(0.5, 2.0, size=3)
    translate = rs.uniform(-10, 10, size=3)
    aff = Affine(3, scale=list(scale), translate=list(translate), period=period)
    n = int(rs.randint(1, 40000))
    lo = (-0.2 * numpy.array(shape) - translate) / scale
    hi = (1.2 * numpy.array(shape) - translate) / scale
    pos_h = rs.uniform(lo, hi, size=(n, 3))
    mass = torch.from_numpy(rs.uniform(0.5, 1.5, size=n)).to(hip.device)
    field = torch.from_numpy(rs.normal(size=shape)).to(hip.device)
    pos = torch.zeros((n, 3), dtype=torch.float64, device=hip.device)
    window.clear_bin_cache()
    for step in range(3):
        pos_h = pos_h + rs.normal(0, 0.3, size=(n, 3)) / scale
        pos.copy_(torch.from_numpy(pos_h))
        out = {}
        for mode in ('always', 'never'):
            window.BINNED = mode
            c = torch.zeros(shape, dtype=torch.float64, device=hip.device)
            W.paint(c, pos, mass=mass, transform=aff)
            out[mode] = (c.cpu().numpy(), W.readout(field, pos, transform=aff).cpu().numpy())
            if mode == 'always':
                assert_binned_ran()
        ref = max(1.0, abs(out['never'][0]).max())
        assert_allclose(out['always'][0], out['never'][0], rtol=0, atol=1e-12 * ref,
                        err_msg='%s shape %s period %s step %d' % (name, shape, period, step))
        assert_array_equal(out['always'][1], out['never'][1], err_msg='%s shape %s period %s step %d' % (name, shape, period, step))


def test_rebuild_drops_and_nonperiodic(hip, form, oracle):
    """history rebuilds with particles that touch no local cell (their own bucket) on a
    non-periodic sub-block: dropped particles read 0 and paint nothing.  (TSC on a block that is not the whole mesh:
    the 'blocks' variant is served by the list, and asserts so; test_rebuild_drops_on_the_whole_periodic_mesh is the
    entry form's.)"""
    window.EXACT = True            # the bit-identical form of the binned readout (pmx_binplan_exact)
    W = windows['tsc']
    window.BINNED = 'always'
    clear_plans()
    N, n = 48, 30000
    aff = Affine(3, translate=[-8, 0, -4], period=[0, 96, 0])
    oaff = oracle.Affine(3, translate=[-8, 0, -4], period=[0, 96, 0])
    rs = numpy.random.RandomState(5)
    field_h = rs.normal(size=(N, N, N))
    field = torch.from_numpy(field_h).to(hip.device)
    pos = torch.zeros((n, 3), dtype=torch.float64, device=hip.device)
    for k in range(4):
        ph = rs.uniform(-20, 120, size=(n, 3)) if k != 2 else rs.uniform(10, 12, size=(n, 3))
        pos.copy_(torch.from_numpy(ph))
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, transform=aff)
        assert_binned_ran()
        check_form(form, False)
        want = numpy.zeros((N, N, N))
        oracle.Window(W.kind).paint(want, ph, transform=oaff)
        assert_allclose(c.cpu().numpy(), want, rtol=0, atol=1e-12 * max(1.0, abs(want).max()))
        got = W.readout(field, pos, transform=aff).cpu().numpy()
        assert_array_equal(got, oracle.Window(W.kind).readout(field_h, ph, transform=oaff))


def test_rebuild_drops_on_the_whole_periodic_mesh(hip, form, oracle):
    """history rebuilds of CIC on the whole periodic mesh (where the 'blocks' variant takes the entries) with rows in no
    cell: NaN rows inside 32-row blocks read 0 and paint nothing, rows far outside wrap; paint against the oracle,
    the default readout within its bound"""
    W = windows['cic']
    window.BINNED = 'always'
    clear_plans()
    N, n = 64, 40000
    aff = Affine(3, scale=0.5, translate=0.25, period=N)
    oaff = oracle.Affine(3, scale=0.5, translate=0.25, period=N)
    rs = numpy.random.RandomState(6)
    field_h = rs.normal(size=(N, N, N))
    field = torch.from_numpy(field_h).to(hip.device)
    pos = torch.zeros((n, 3), dtype=torch.float64, device=hip.device)
    ph = numpy.sort(rs.uniform(0, 2 * N, size=(n, 3)), axis=0)
    for k in range(4):
        ph = ph + rs.normal(0, 0.3, size=(n, 3))
        q = ph.copy()
        q[k::13 + k] = numpy.nan
        q[5::31] += 2 * N * rs.randint(-50, 50, size=(len(q[5::31]), 3))
        pos.copy_(torch.from_numpy(q))
        ok = numpy.isfinite(q).all(axis=1)
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, pos, transform=aff)
        assert_binned_ran()
        check_form(form, True)
        want = numpy.zeros((N, N, N))
        oracle.Window(W.kind).paint(want, q[ok], transform=oaff)
        assert_allclose(c.cpu().numpy(), want, rtol=0, atol=1e-12 * max(1.0, abs(want).max()), err_msg='step %d' % k)
        got = W.readout(field, pos, transform=aff).cpu().numpy()
        check_form(form, True)
        assert (got[~ok] == 0).all()
        assert_allclose(got[ok], oracle.Window(W.kind).readout(field_h, q[ok], transform=oaff), rtol=0,
                        atol=1e-13 * abs(field_h).max(), err_msg='step %d' % k)


@pytest.mark.parametrize('name,dtype', [('cic', 'f8'), ('tsc', 'f4')])
def test_full_size_properties(hip, name, dtype):
    """BASELINE sizes (512^3 mesh, 512^3 particles; config 3 in f4): size-independent
    properties of the tile-binned kernels."""
    import ctypes as C
    from pmesh_amd._arrays import vec
    from pmesh_amd.pm import ParticleMesh
    window.BINNED = 'auto'
    N, L = 512, 1000.0
    tdt = torch.float64 if dtype == 'f8' else torch.float32
    pos = torch.empty((N ** 3, 3), dtype=tdt, device=hip.device)
    pv = vec(pos)
    hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, N ** 3, hip.stream())
    pm = ParticleMesh(BoxSize=L, Nmesh=[N, N, N], dtype=dtype, resampler=name)
    rho = pm.paint(pos)
    tol = 1e-10 if dtype == 'f8' else 2e-4
    assert abs(rho.csum(dtype='f8') / N ** 3 - 1.0) < tol           # mass conservation
    assert float(rho.value.min()) >= 0.0
    rho2 = pm.paint(pos, mass=2.0)                                   # linearity in the mass
    assert float((rho2.value - 2 * rho.value).abs().max()) <= (1e-12 if dtype == 'f8' else 1e-5) * float(rho2.value.max())
    window.BINNED = 'never'                                          # direct == binned at full size
    rho3 = pm.paint(pos)
    assert float((rho3.value - rho.value).abs().max()) <= (1e-12 if dtype == 'f8' else 4e-6) * float(rho.value.max())
    window.BINNED = 'auto'
    one = pm.create('real', value=1.0)
    v = one.readout(pos)                                             # partition of unity
    assert float((v - 1.0).abs().max()) < (1e-14 if dtype == 'f8' else 1e-6)
    g = one.readout(pos, gradient=0)                                 # gradient of a constant
    assert float(g.abs().max()) < (1e-12 if dtype == 'f8' else 1e-4)
    # checksum of checksums: readout of the painted density, weighted back, is symmetric
    f1 = rho.readout(pos)
    lhs = float((f1.to(torch.float64)).sum())
    rhs = float((rho.value.to(torch.float64) ** 2).sum())          # <paint(1), rho> == <1, readout(rho)>
    assert abs(lhs - rhs) <= (1e-10 if dtype == 'f8' else 1e-3) * abs(rhs)


@pytest.mark.parametrize('N,name,dtype,gradient,tol,data', [
    (64, 'cic', 'f8', None, 1e-11, 'uniform'),      # BASELINE config 1 (the reference's own CPU-runnable case)
    (256, 'cic', 'f8', None, 1e-11, 'uniform'),     # BASELINE config 2 (measured 2.6e-15)
    (512, 'cic', 'f8', None, 1e-11, 'uniform'),     # the headline workload of bench.py (measured 3.9e-15)
    (512, 'tsc', 'f4', 0, 2e-5, 'uniform'),         # BASELINE config 3: TSC + gradient readout, fp32 (1.3e-6)
    (512, 'cic', 'f8', None, 1e-11, 'clustered'),   # the headline on the Zel'dovich-displaced set
    (256, 'pcs', 'f8', None, 1e-11, 'clustered'),   # config 5's window on the clustered set
])
def test_baseline_cycle_equals_oracle(hip, oracle, N, name, dtype, gradient, tol, data):
    """BASELINE.json's single-GPU configurations at their FULL size — uniform particles (the
    bench's lattice + hashed jitter), one per cell — through the production form of the cycle
    (tile-binned paint/readout, LDS row/column FFT on the padded layout, transfer fused into
    c2r), every particle compared with the CPU oracle (reference kernels + numpy.fft)."""
    import ctypes as C
    from pmesh_amd._arrays import vec
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Transfer
    window.BINNED = 'auto'
    L = 1000.0
    tdt = torch.float64 if dtype == 'f8' else torch.float32
    pos = torch.empty((N ** 3, 3), dtype=tdt, device=hip.device)
    pv = vec(pos)
    if data == 'uniform':
        hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, N ** 3, hip.stream())
    else:
        modes = oracle.zeldovich_modes(N, L)                        # 3-cell rms displacement, 16 plane waves
        hip.call('synth_clustered', C.byref(pv), N, L, modes.ctypes.data_as(C.POINTER(C.c_double)), len(modes),
                 0.0, 0, N ** 3, hip.stream())
    pm = ParticleMesh(BoxSize=L, Nmesh=[N, N, N], dtype=dtype, resampler=name)
    rho = pm.paint(pos)
    assert_binned_ran()
    peak = float(rho.value.max())                                   # before the in-place transforms
    f = rho.r2c(out=Ellipsis).c2r(out=Ellipsis, transfer=Transfer.dx1(0)).readout(pos, gradient=gradient)
    pos_h = pos.cpu().numpy()
    if data == 'uniform':
        assert numpy.array_equal(pos_h, oracle.synth_uniform(N, L, dtype=dtype))   # bit for bit the oracle's set
    else:
        print('clustered set: densest cell holds %.1f particles (mean 1)' % peak)
        assert peak > 10                                            # density contrast >> 1
    t = oracle.make_transfer(laplace_pow=-1, grad_dir=0, grad_kind=0)
    real, ck, back, want = oracle.pm_cycle(N, L, pos_h, kind='tuned' + name, transfer=t, gradient=gradient,
                                           dtype=dtype)
    got = f.cpu().numpy()
    err = abs(got - want).max() / abs(want).max()
    print('full-size cycle N=%d %s %s %s: max |error| / max |value| = %.3e' % (N, name, dtype, data, err))
    assert err <= tol

@pytest.mark.parametrize('N,name,dtype,tol', [(256, 'cic', 'f8', 1e-11), (256, 'tsc', 'f4', 2e-5)])
def test_time_stepping_cycles_equal_oracle(hip, oracle, N, name, dtype, tol):
    """What bench.py times: consecutive cycles on positions that moved by a fraction of a cell, so
    that every cycle after the first REBUILDS the bin plan in a single pass from the slot ranges
    of the previous one (bin_block_kernel at full size).  Three steps of a 0.1-cell random walk
    at config 2's size, every particle of every step against the CPU oracle."""
    import ctypes as C
    from pmesh_amd._arrays import vec
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Transfer
    window.BINNED = 'auto'
    window.bin_cache().destroy(hip)           # (no plan state of earlier tests: see test_bin_blocks.py)
    L = 1000.0
    tdt = torch.float64 if dtype == 'f8' else torch.float32
    pos = torch.empty((N ** 3, 3), dtype=tdt, device=hip.device)
    pv = vec(pos)
    hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, N ** 3, hip.stream())
    pm = ParticleMesh(BoxSize=L, Nmesh=[N, N, N], dtype=dtype, resampler=name)
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(99)
    t = oracle.make_transfer(laplace_pow=-1, grad_dir=0, grad_kind=0)
    served = []
    for step in range(3):
        if step:
            pos = pos + torch.randn(pos.shape, dtype=tdt, device=hip.device, generator=gen) * (0.1 * L / N)
        rho = pm.paint(pos)
        assert_binned_ran()
        served += [e[1].value for e in window.bin_cache().entries if e[3] and e[2] is pos]
        if window.BLOCKS == 'auto':
            # the benchmark's form: the first build measures the (lattice) row order, the next ones take the block
            # entries (CIC, dense rows of doubles, the whole periodic mesh) — asserted before the readout runs
            built = [e for e in window.bin_cache().entries if e[3]]
            forms = [f for e, f in zip(built, window.bin_cache().block_plans(hip)) if e[2] is pos]
            assert forms == [(step > 0 and name == 'cic' and dtype == 'f8', 0)], (step, forms)
        f = rho.r2c(out=Ellipsis).c2r(out=Ellipsis, transfer=Transfer.dx1(0)).readout(pos)
        real, ck, back, want = oracle.pm_cycle(N, L, pos.cpu().numpy(), kind='tuned' + name, transfer=t, dtype=dtype)
        err = abs(f.cpu().numpy() - want).max() / abs(want).max()
        print('step %d N=%d %s %s: max |error| / max |value| = %.3e' % (step, N, name, dtype, err))
        assert err <= tol
    # one pooled plan served all three position tensors (the rebuilds had the previous slot ranges)
    assert len(set(served)) == 1, served


@pytest.mark.parametrize('name', TUNED)
@pytest.mark.parametrize('dtype,odtype', [('f8', 'f8'), ('f4', 'f4'), ('f8', 'f4')])
def test_readout_of_several_fields_equals_field_by_field(hip, oracle, name, dtype, odtype):
    """pmx_readout_binned_multi (ResampleWindow.readout_many / ParticleMesh.readout): out[i, f] = field f at x_i from
    one launch == the lean readout of every field on its own, bit for bit (the same loop per canvas), == the oracle
    within the readout's tolerance; rows of `out` with a pitch, float and double results, a slab-local block with
    particles outside it (they read 0), and the fallbacks (exact arithmetic, one field) give the same numbers."""
    W = windows[name]
    rs = numpy.random.RandomState(12)
    shape = (24, 48, 64)
    aff = Affine(3, scale=[1.0, 0.5, 2.0], translate=[-4.0, 0.0, 0.0], period=[64, 48, 64])
    n = 60000
    pos_h = rs.uniform([-2, 0, 0], [34, 96, 32], size=(n, 3))
    tdt = torch.float64 if dtype == 'f8' else torch.float32
    fields_h = [rs.normal(size=shape).astype(dtype) for _ in range(3)]
    fields = [torch.from_numpy(f).to(hip.device) for f in fields_h]
    pos = torch.from_numpy(pos_h).to(hip.device)
    window.BINNED = 'always'
    window.clear_bin_cache()
    wide = torch.full((n, 5), 7.0, dtype=torch.float64 if odtype == 'f8' else torch.float32, device=hip.device)
    got = W.readout_many(fields, pos, out=wide[:, 1:4], transform=aff)
    assert got.data_ptr() == wide[:, 1:4].data_ptr()
    assert float(wide[:, 0].min()) == 7.0 and float(wide[:, 4].max()) == 7.0          # the neighbours of the rows are untouched
    for f in range(3):
        one = torch.empty(n, dtype=wide.dtype, device=hip.device)
        W.readout(fields[f], pos, out=one, transform=aff)
        assert torch.equal(got[:, f], one), (name, f)
        want = oracle.Window(W.kind).readout(fields_h[f].astype('f8'), pos_h, transform=oracle.Affine(3, scale=aff.scale, translate=aff.translate, period=aff.period))
        tol = 1e-13 if (dtype == 'f8' and odtype == 'f8') else 2e-6
        assert float(abs(got[:, f].double().cpu().numpy() - want).max()) <= tol * 64 * float(abs(fields_h[f]).max())
    # gradient weights, a new tensor for the results
    g2 = W.readout_many(fields[:2], pos, diffdir=1, transform=aff)
    assert g2.shape == (n, 2) and g2.dtype == torch.float64
    for f in range(2):
        assert torch.equal(g2[:, f], W.readout(fields[f], pos, diffdir=1, transform=aff))
    # exact arithmetic is not what the fused entry serves: the same call falls back to field by field
    window.EXACT = True
    window.clear_bin_cache()
    ge = W.readout_many(fields, pos, transform=aff)
    for f in range(3):
        assert torch.equal(ge[:, f], W.readout(fields[f], pos, transform=aff))
    window.EXACT = False


def test_particlemesh_readout_of_several_fields(hip):
    """ParticleMesh.readout(fields, pos): the three force components of a PM step into the rows of one array"""
    from pmesh_amd.pm import ParticleMesh
    from pmesh_amd.transfer import Transfer
    N = 64
    pm = ParticleMesh(BoxSize=float(N), Nmesh=[N, N, N], dtype='f8', resampler='cic')
    Q = pm.generate_uniform_particle_grid(shift=0.5)
    g = torch.Generator(device=Q.device).manual_seed(5)
    X = (Q + 0.3 * torch.randn(Q.shape, generator=g, dtype=Q.dtype, device=Q.device)) % float(N)
    rhok = pm.paint(X).r2c()
    comps = [rhok.c2r(transfer=Transfer.force(d)) for d in range(3)]
    F = pm.readout(comps, X)
    assert F.shape == (len(X), 3)
    for d in range(3):
        assert torch.equal(F[:, d], comps[d].readout(X))
    with pytest.raises(TypeError):
        pm.readout([rhok], X)
