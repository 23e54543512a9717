"""The block-entry form of the bin plan (csrc/pmx_binned.hip: bin_entries_kernel, paint_entries_kernel,
readout_entries_kernel, plan_to_list) against the index list — readout bit-identical, paint equal up to the order of its
sums — and against the CPU oracle in float64 at the edges of the entry addressing: row counts around a block of 32,
coherent and single-row masks, float canvases, float and column results, mass vectors, gradients, accumulation, counts
that change between builds, every consumer that turns the plan into the list, and the 'auto' rule.  Every case asserts
the plan's form through pmx_binplan_blocks."""
import ctypes as C

import numpy
import pytest
import torch
from numpy.testing import assert_array_equal

from pmesh_amd import window
from pmesh_amd._arrays import vec, vec_ref
from pmesh_amd.window import Affine, windows

pytestmark = pytest.mark.gpu


@pytest.fixture
def hip():
    from pmesh_amd import backend
    backend.reset()
    b = backend.get()
    old = window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS
    window.BINNED, window.WALK, window.SORTED = 'always', 'never', 'auto'
    yield b
    window.BINNED, window.WALK, window.SORTED, window.EXACT, window.BLOCKS = old
    window.clear_bin_cache()
    backend.reset()


def lattice(hip, N, L, n=None):
    from pmesh_amd._arrays import vec
    n = N ** 3 if n is None else n
    pos = torch.empty((n, 3), dtype=torch.float64, device=hip.device)
    pv = vec(pos)
    hip.call('synth_uniform', C.byref(pv), N, L, 42, 0, n, hip.stream())
    return pos


def run(hip, sets, N, L, field, blocks, exact_last=False):
    """paint + readout of every position set in turn through ONE plan history (single-pass rebuilds)"""
    window.BLOCKS = blocks
    window.EXACT = False
    window.clear_bin_cache()
    W = windows['cic']
    aff = Affine(3, scale=N / L, period=N)
    out = []
    for k, p in enumerate(sets):
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        W.paint(c, p, transform=aff)
        if exact_last and k == len(sets) - 1:
            window.EXACT = True            # a consumer of the index list: the plan leaves the entry form
        out.append((c, W.readout(field, p, transform=aff)))
    torch.cuda.synchronize()
    return out


def check(a, b, exact_readout=True):
    for (ca, ra), (cb, rb) in zip(a, b):
        assert float((ca - cb).abs().max()) <= 1e-12 * max(1.0, float(ca.abs().max()))
        if exact_readout:
            assert torch.equal(ra, rb)
        else:
            assert float((ra - rb).abs().max()) <= 1e-12 * max(1.0, float(ra.abs().max()))


@pytest.mark.parametrize('drift', [0.0, 0.1, 1.0, 4.0])
def test_blocks_equal_list_on_drifted_lattices(hip, drift):
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(3)
    pos = lattice(hip, N, L)
    sets = [pos]
    for _ in range(3):
        sets.append(sets[-1] + torch.randn(pos.shape, dtype=torch.float64, device=hip.device, generator=gen) * (drift * L / N))
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'always'))


def test_blocks_partial_block_outside_rows_and_changing_count(hip):
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(5)
    n = N ** 3 - 45                     # the last block of 32 rows is partial
    pos = lattice(hip, N, L, n)
    pos[::97] = float('nan')            # rows that touch no cell: read 0
    sets = [pos, pos[:n - 1000].clone() + 0.05, pos + 0.1]
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    a, b = run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'always')
    check(a, b)
    assert float(b[0][1][::97].abs().max()) == 0.0


def test_blocks_overflow_is_repaired(hip):
    """a step that moves many rows into one tile outgrows its entry range: the gated repair fixes it and
    bin_overflows counts it"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(9)
    pos = lattice(hip, N, L)
    moved = pos.clone()
    moved[: N ** 3 // 8] = moved[: N ** 3 // 8] * 0.1      # an eighth of the rows into a corner of the box
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    a = run(hip, [pos, pos + 0.01, moved], N, L, field, 'never')
    b = run(hip, [pos, pos + 0.01, moved], N, L, field, 'always')
    check(a, b)
    assert window.bin_cache().overflows(hip) > 0


def test_blocks_fall_back_to_the_list(hip):
    """a consumer of the index list (the readout in the reference's arithmetic) turns the plan into the list"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(11)
    pos = lattice(hip, N, L)
    sets = [pos, pos + 0.02, pos + 0.04]
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never', exact_last=True), run(hip, sets, N, L, field, 'always', exact_last=True))


def test_shuffled_rows_do_not_take_blocks(hip):
    """'auto' never gives rows in no order the entry form; results equal the list's"""
    N, L = 64, 100.0
    gen = torch.Generator(device=hip.device)
    gen.manual_seed(13)
    pos = lattice(hip, N, L)
    perm = torch.randperm(N ** 3, device=hip.device, generator=gen)
    sets = [pos[perm].contiguous()] * 3
    field = torch.randn((N, N, N), dtype=torch.float64, device=hip.device, generator=gen)
    check(run(hip, sets, N, L, field, 'never'), run(hip, sets, N, L, field, 'auto'))


# ---- against the oracle, through ONE plan driven by the C ABI (its history is exactly the builds of the test) ----------
KIND = windows['cic'].kind


class Plan(object):
    def __init__(self, hip, blocks='always', sort_pref=0):
        self.be = hip
        self.h = C.c_void_p()
        hip.call('binplan_create', C.byref(self.h))
        self.configure(blocks)
        hip.call('binplan_sorted', self.h, sort_pref, None)

    def configure(self, blocks):
        self.be.call('binplan_configure', self.h, window._BLOCKS[blocks] << 8)       # (and the tile form)

    def close(self):
        self.be.call('binplan_destroy', self.h)

    def form(self):
        """(in block-entry form, drops): host state, read before any consumer of the list runs"""
        f, d = C.c_int32(0), C.c_uint32(0)
        self.be.call('binplan_blocks', self.h, C.byref(f), C.byref(d))
        return bool(f.value), int(d.value)

    @staticmethod
    def painter(real, aff, diffdir=None):
        order = numpy.zeros(3, dtype=int)
        if diffdir is not None:
            order[diffdir] = 1
        return windows['cic']._painter(real, order, aff)

    def build(self, real, pos, aff):
        torch.cuda.synchronize()          # (the 'auto' rule reads what the previous build measured: make it final)
        self.be.call('binplan_build', self.h, C.byref(self.painter(real, aff)), C.byref(vec(pos)), pos.shape[0],
                     self.be.stream())

    def paint(self, canvas, pos, aff, mass=None, ms=1.0, diffdir=None, overwrite=False):
        self.be.call('paint_binned', self.h, C.byref(self.painter(canvas, aff, diffdir)), canvas.data_ptr(),
                     C.byref(vec(pos)), vec_ref(vec(mass) if mass is not None else None), ms, int(overwrite),
                     self.be.stream())
        return canvas

    def readout(self, field, pos, aff, out=None, diffdir=None):
        if out is None:
            out = torch.full((pos.shape[0],), 7.0, dtype=torch.float64, device=pos.device)
        self.be.call('readout_binned', self.h, C.byref(self.painter(field, aff, diffdir)), field.data_ptr(),
                     C.byref(vec(pos)), C.byref(vec(out)), self.be.stream())
        return out


@pytest.fixture
def plan(hip):
    made = []

    def make(blocks='always', sort_pref=0):
        made.append(Plan(hip, blocks, sort_pref))
        return made[-1]
    yield make
    torch.cuda.synchronize()
    for p in made:
        p.close()


def oracle_paint(oracle, shape, pos_h, oaff, mass=None, diffdir=None, base=None):
    ok = numpy.isfinite(pos_h).all(axis=1)
    want = numpy.zeros(shape) if base is None else base.copy()
    oracle.Window(KIND).paint(want, numpy.ascontiguousarray(pos_h[ok]), transform=oaff, diffdir=diffdir,
                              mass=None if mass is None or numpy.isscalar(mass) else numpy.ascontiguousarray(mass[ok]))
    if mass is not None and numpy.isscalar(mass):
        want = (want - (0 if base is None else base)) * mass + (0 if base is None else base)
    return want


def oracle_readout(oracle, field_h, pos_h, oaff, diffdir=None):
    """the reference's values; rows in no cell (NaN) read 0"""
    ok = numpy.isfinite(pos_h).all(axis=1)
    want = numpy.zeros(len(pos_h))
    want[ok] = oracle.Window(KIND).readout(field_h.astype('f8'), numpy.ascontiguousarray(pos_h[ok]), transform=oaff,
                                           diffdir=diffdir)
    return want


def close_paint(got, want, f4=False, what=''):
    got = got.double().cpu().numpy() if torch.is_tensor(got) else got
    err = float(abs(got - want).max())
    assert err <= (2e-6 if f4 else 1e-12) * max(1.0, float(abs(want).max())), (what, err)


def close_readout(got, want, fmax, wb=1.0, f4=False, what=''):
    """within the bound of test_binned.py::test_default_readout_within_tolerance_of_the_exact_form, and the rows that
    read zero are the oracle's"""
    got = got.double().cpu().numpy() if torch.is_tensor(got) else got
    err = float(abs(got - want).max())
    assert err <= (2e-6 if f4 else 1e-13) * wb * fmax, (what, err)
    assert_array_equal(got == 0, want == 0, err_msg=what)


def drifted_lattice(hip, N, L, drift, seed, n=None):
    """rows in lattice order (dense entries), moved by N(0, drift) cells"""
    pos = lattice(hip, N, L, n)
    g = torch.Generator(device=hip.device)
    g.manual_seed(seed)
    return pos + torch.randn(pos.shape, dtype=torch.float64, device=hip.device, generator=g) * (drift * L / N)


def geometry(oracle, N, L):
    return Affine(3, scale=N / L, period=N), oracle.Affine(3, scale=N / L, period=N)


def rand_field(shape, seed, dtype='f8'):
    return numpy.random.RandomState(seed).normal(size=shape).astype(dtype)


@pytest.mark.parametrize('n', [1, 31, 32, 33, 63, 65, 4095, 4097, 64 ** 3 - 45])
def test_blocks_row_counts_against_the_oracle(hip, oracle, plan, n):
    """a plan of n rows in entry form: blocks of 32 with a partial last one, NaN rows inside blocks (in no tile: read 0,
    paint nothing) and rows many boxes outside the mesh (they wrap)"""
    N, L = 64, 100.0
    aff, oaff = geometry(oracle, N, L)
    pos = drifted_lattice(hip, N, L, 0.3, 17, n=max(n, 1))[:n].contiguous()
    rs = numpy.random.RandomState(n)
    if n > 3:
        pos[1::7] = float('nan')
        far = torch.from_numpy(rs.randint(-1000, 1000, size=(len(range(2, n, 5)), 3)) * L).to(hip.device)
        pos[2::5] += far
    pos_h = pos.cpu().numpy()
    field_h = rand_field((N, N, N), 3)
    field = torch.from_numpy(field_h).to(hip.device)
    p = plan()
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff), what='paint n=%d' % n)
    got = p.readout(field, pos, aff)
    assert p.form() == (True, 0)
    want = oracle_readout(oracle, field_h, pos_h, oaff)
    close_readout(got, want, abs(field_h).max(), what='readout n=%d' % n)
    if n > 3:
        assert float(got[1::7].abs().max()) == 0.0


@pytest.mark.parametrize('order', ['lattice', 'drifted', 'shuffled'])
@pytest.mark.parametrize('shape,L', [((64, 64, 64), 100.0), ((16, 32, 64), 16.0), ((24, 32, 96), 12.0),
                                     ((40, 48, 96), 40.0)])
def test_blocks_coherent_and_shuffled_rows_against_the_oracle(hip, oracle, plan, order, shape, L):
    """rows in lattice order (entries of 32 rows), drifted (entries split at tile faces) and shuffled ('always': almost
    every entry holds one row) on cubic and non-cubic whole periodic meshes with a scale and a translation, down to the
    smallest the tile kernels take (2 x 2 x 2 tiles: a mesh of one tile is PMX_EUNSUPPORTED)"""
    rs = numpy.random.RandomState(21)
    n = int(numpy.prod(shape))
    scale = tuple(s / L for s in shape)
    translate = (0.25, -3.0, 7.5)
    aff = Affine(3, scale=scale, translate=translate, period=shape)
    oaff = oracle.Affine(3, scale=scale, translate=translate, period=shape)
    idx = numpy.indices(shape).reshape(3, -1).T.astype('f8')
    pos_h = numpy.ascontiguousarray((idx + 0.5) / numpy.asarray(scale))
    if order != 'lattice':
        pos_h = pos_h + rs.normal(0, 0.7, size=pos_h.shape) / numpy.asarray(scale)
    if order == 'shuffled':
        pos_h = pos_h[rs.permutation(n)]
    pos = torch.from_numpy(numpy.ascontiguousarray(pos_h)).to(hip.device)
    field_h = rand_field(shape, 5)
    field = torch.from_numpy(field_h).to(hip.device)
    p = plan()
    c = torch.zeros(shape, dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, shape, pos_h, oaff))
    close_readout(p.readout(field, pos, aff), oracle_readout(oracle, field_h, pos_h, oaff), abs(field_h).max())
    assert p.form() == (True, 0)


def test_blocks_canvas_and_result_types(hip, oracle, plan):
    """float canvases with double positions (T = float of paint_entries_kernel and readout_entries_kernel), a float
    result (OE_ = 4) and a column F[:, 1] of an (n, 3) array (ostride): the other columns stay untouched"""
    N, L = 64, 100.0
    aff, oaff = geometry(oracle, N, L)
    pos = drifted_lattice(hip, N, L, 0.5, 23)
    pos_h = pos.cpu().numpy()
    n = pos.shape[0]
    p = plan()
    c4 = torch.zeros((N, N, N), dtype=torch.float32, device=hip.device)
    p.build(c4, pos, aff)
    p.paint(c4, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c4, oracle_paint(oracle, (N, N, N), pos_h, oaff), f4=True, what='f4 canvas')
    f4_h = rand_field((N, N, N), 7, 'f4')
    got = p.readout(torch.from_numpy(f4_h).to(hip.device), pos, aff)
    close_readout(got, oracle_readout(oracle, f4_h, pos_h, oaff), abs(f4_h).max(), f4=True, what='f4 field')
    f8_h = rand_field((N, N, N), 8)
    field = torch.from_numpy(f8_h).to(hip.device)
    want = oracle_readout(oracle, f8_h, pos_h, oaff)
    out4 = torch.empty(n, dtype=torch.float32, device=hip.device)
    p.readout(field, pos, aff, out=out4)
    close_readout(out4, want, abs(f8_h).max(), f4=True, what='f4 out')
    F = torch.full((n, 3), 7.0, dtype=torch.float64, device=hip.device)
    p.readout(field, pos, aff, out=F[:, 1])
    close_readout(F[:, 1], want, abs(f8_h).max(), what='column out')
    assert float(F[:, 0].min()) == 7.0 and float(F[:, 0].max()) == 7.0
    assert float(F[:, 2].min()) == 7.0 and float(F[:, 2].max()) == 7.0
    assert p.form() == (True, 0)          # every one of these was served by the entry kernels


def test_blocks_masses_gradients_and_accumulation(hip, oracle, plan):
    """a mass vector with zeros and a +-1e250 range, diffdir 0 / 1 / 2 for paint and readout, _overwrite against
    accumulating into a canvas that holds values"""
    N, L = 64, 64.0
    aff, oaff = geometry(oracle, N, L)
    pos = drifted_lattice(hip, N, L, 0.4, 29)
    pos_h = pos.cpu().numpy()
    n = len(pos_h)
    rs = numpy.random.RandomState(31)
    huge = numpy.sign(rs.normal(size=n)) * 10.0 ** rs.uniform(-250, 250, size=n)
    huge[rs.rand(n) < 0.1] = 0.0
    plain = rs.uniform(0.5, 1.5, size=n)
    field_h = rand_field((N, N, N), 9)
    field = torch.from_numpy(field_h).to(hip.device)
    p = plan()
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff, mass=torch.from_numpy(huge).to(hip.device))
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff, mass=huge), what='+-1e250 masses')
    m = torch.from_numpy(plain).to(hip.device)
    for d in range(3):
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        p.paint(c, pos, aff, mass=m, diffdir=d)
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff, mass=plain, diffdir=d), what='paint diffdir %d' % d)
        got = p.readout(field, pos, aff, diffdir=d)
        close_readout(got, oracle_readout(oracle, field_h, pos_h, oaff, diffdir=d), abs(field_h).max(), wb=4.0,
                      what='readout diffdir %d' % d)
    assert p.form() == (True, 0)
    base = rs.normal(size=(N, N, N))
    acc = torch.from_numpy(base.copy()).to(hip.device)
    p.paint(acc, pos, aff, mass=m)
    close_paint(acc, oracle_paint(oracle, (N, N, N), pos_h, oaff, mass=plain, base=base), what='accumulate')
    ow = torch.full((N, N, N), 7.0, dtype=torch.float64, device=hip.device)
    p.paint(ow, pos, aff, mass=m, overwrite=True)
    close_paint(ow, oracle_paint(oracle, (N, N, N), pos_h, oaff, mass=plain), what='overwrite')
    ow.fill_(7.0)
    p.paint(ow, pos, aff, ms=-2.5, overwrite=True)
    close_paint(ow, oracle_paint(oracle, (N, N, N), pos_h, oaff, mass=-2.5), what='overwrite, scalar mass')
    assert p.form() == (True, 0)


@pytest.mark.parametrize('order', ['cells', 'random'])
@pytest.mark.parametrize('shape', [(64, 64, 64), (16, 32, 64), (24, 32, 96), (40, 48, 96)])
def test_blocks_dyadic_paint_bit_exact(hip, oracle, plan, order, shape):
    """positions on a 1/16-cell grid, masses multiples of 2^-6 (as test_halo_defer.particles(dyadic=True)): every
    partial sum is exact, so the entry paint equals the oracle bit for bit only if each masked row lands on its cells"""
    rs = numpy.random.RandomState(37)
    n = 3 * int(numpy.prod(shape)) // 4
    pos_h = rs.randint(-2 * 16 * max(shape), 3 * 16 * max(shape), size=(n, 3)) / 16.0
    if order == 'cells':                    # rows in the order of their cells: dense masks
        cell = numpy.floor(pos_h).astype(numpy.int64) % numpy.asarray(shape)
        pos_h = pos_h[numpy.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))]
    mass_h = rs.randint(1, 65, size=n) / 64.0
    aff = Affine(3, period=shape)
    oaff = oracle.Affine(3, period=shape)
    pos = torch.from_numpy(numpy.ascontiguousarray(pos_h)).to(hip.device)
    p = plan()
    c = torch.zeros(shape, dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff, mass=torch.from_numpy(mass_h).to(hip.device))
    assert p.form() == (True, 0)
    assert_array_equal(c.cpu().numpy(), oracle_paint(oracle, shape, pos_h, oaff, mass=mass_h))


def test_blocks_counts_that_change_between_builds(hip, oracle, plan):
    """one plan history: n, n + n/8, 2n (the entries are reallocated), n/3 — every build against the oracle"""
    N, L = 64, 100.0
    aff, oaff = geometry(oracle, N, L)
    big = drifted_lattice(hip, N, L, 0.2, 41)
    field_h = rand_field((N, N, N), 11)
    field = torch.from_numpy(field_h).to(hip.device)
    n = 96000
    p = plan()
    for k, m in enumerate([n, n + n // 8, 2 * n, n // 3, n // 3 + 5]):
        pos = (big[-m:] + 0.05 * k).contiguous()
        pos_h = pos.cpu().numpy()
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        p.build(c, pos, aff)
        p.paint(c, pos, aff)
        assert p.form() == (True, 0), k
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff), what='step %d' % k)
        close_readout(p.readout(field, pos, aff), oracle_readout(oracle, field_h, pos_h, oaff), abs(field_h).max(),
                      what='step %d' % k)


def host_tiles(pos_h, N):
    """the tile (8 x 16 x 32 cells, C order) of CIC's first cell floor(x) of every row"""
    c = numpy.floor(pos_h).astype(numpy.int64) % N
    nt = (N // 8, N // 16, N // 32)
    return ((c[:, 0] // 8) * nt[1] + c[:, 1] // 16) * nt[2] + c[:, 2] // 32


@pytest.mark.parametrize('consumer', ['deterministic', 'exact', 'many', 'order', 'strided'])
def test_blocks_list_consumers_against_the_oracle(hip, oracle, plan, consumer):
    """after an entry build, each consumer of the index list turns the plan into the list (plan_to_list: entry_rows_kernel,
    entry_fill_kernel) and is served from it: the deterministic paint, the exact readout, the readout of 3 fields,
    pmx_binplan_order, and rows with a pitch (a strided view of the same positions, reachable through the C ABI only:
    the window API keys plans on dtype and stride).  The plan then stays on the list for its history; another particle
    set (a count outside an eighth) starts a new one and takes the entries again."""
    N = 64
    aff = Affine(3, period=N)
    oaff = oracle.Affine(3, period=N)
    pos = drifted_lattice(hip, N, float(N), 0.3, 43)
    pos_h = pos.cpu().numpy()
    n = len(pos_h)
    fields_h = [rand_field((N, N, N), 50 + f) for f in range(3)]
    fields = [torch.from_numpy(f).to(hip.device) for f in fields_h]
    fmax = max(abs(f).max() for f in fields_h)
    p = plan()
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff))
    if consumer == 'deterministic':
        hip.call('binplan_deterministic', p.h, 1)
        c.zero_()
        p.paint(c, pos, aff)
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff))
        hip.call('binplan_deterministic', p.h, 0)
    elif consumer == 'exact':
        hip.call('binplan_exact', p.h, 1)
        assert_array_equal(p.readout(fields[0], pos, aff).cpu().numpy(), oracle_readout(oracle, fields_h[0], pos_h, oaff))
        hip.call('binplan_exact', p.h, 0)
    elif consumer == 'many':
        out = torch.full((n, 3), 7.0, dtype=torch.float64, device=hip.device)
        ptrs = (C.c_void_p * 3)(*[f.data_ptr() for f in fields])
        hip.call('readout_binned_multi', p.h, C.byref(Plan.painter(fields[0], aff)), ptrs, 3, C.byref(vec(pos)),
                 C.byref(vec(out)), hip.stream())
        for f in range(3):
            close_readout(out[:, f], oracle_readout(oracle, fields_h[f], pos_h, oaff), fmax, what='field %d' % f)
    elif consumer == 'order':
        order = torch.empty(n, dtype=torch.int64, device=hip.device)
        hip.call('binplan_order', p.h, order.data_ptr(), hip.stream())
        o = order.cpu().numpy()
        assert_array_equal(numpy.sort(o), numpy.arange(n))                 # a permutation
        assert (numpy.diff(host_tiles(pos_h[o], N)) >= 0).all()             # tile by tile
    else:
        wide = torch.full((n, 5), 7.0, dtype=torch.float64, device=hip.device)
        wide[:, 1:4] = pos
        c.zero_()
        p.paint(c, wide[:, 1:4], aff)
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff))
    assert p.form() == (False, 0), 'the consumer left the plan in entry form'
    for k in range(2):                         # the builds of this history keep the list
        pos = pos + 0.01
        pos_h = pos.cpu().numpy()
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        p.build(c, pos, aff)
        p.paint(c, pos, aff)
        assert p.form() == (False, 0)
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff))
        close_readout(p.readout(fields[1], pos, aff), oracle_readout(oracle, fields_h[1], pos_h, oaff), fmax)
    pos = pos[: n // 2].contiguous()            # another particle set: a new history
    pos_h = pos.cpu().numpy()
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff))
    close_readout(p.readout(fields[2], pos, aff), oracle_readout(oracle, fields_h[2], pos_h, oaff), fmax)


def test_blocks_auto_rule(hip, oracle, plan):
    """'auto' decides at a build from what the PREVIOUS build measured (breaks of the tile sequence per 64 rows among
    the sampled rows, more than 4096 of them: 128^3 rows give ~16k): take the entries at <= PMX_BLOCKS_TAKE_BREAKS (6),
    give them up above PMX_BLOCKS_DROP_BREAKS (10), keep the list after two drops.  A lattice drifted by 0.1 cell
    shows a few breaks, shuffled rows ~63: far from both thresholds.  Every transition lags the rows by one build."""
    N, L = 128, 128.0
    aff, oaff = geometry(oracle, N, L)
    base = lattice(hip, N, L)
    n = base.shape[0]
    g = torch.Generator(device=hip.device)
    g.manual_seed(47)
    perm = torch.randperm(n, device=hip.device, generator=g)
    field_h = rand_field((N, N, N), 13)
    field = torch.from_numpy(field_h).to(hip.device)
    p = plan('auto', sort_pref=-1)
    #            rows        form after the build (entries, drops)
    steps = [('coherent', (False, 0)),     # the first build: nothing measured yet
             ('coherent', (True, 0)),      # the first build measured coherent rows
             ('shuffled', (True, 0)),      # (decided on the coherent rows before)
             ('coherent', (False, 1)),     # the shuffled rows before: dropped once
             ('coherent', (True, 1)),      # taken again
             ('shuffled', (True, 1)),
             ('coherent', (False, 2)),     # dropped twice: the plan keeps the list ...
             ('coherent', (False, 2)),     # ... however coherent the rows are
             ('coherent', (False, 2))]
    for k, (rows, want) in enumerate(steps):
        pos = base + 0.1 * torch.randn(base.shape, dtype=torch.float64, device=hip.device, generator=g)
        if rows == 'shuffled':
            pos = pos[perm].contiguous()
        pos_h = pos.cpu().numpy()
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        p.build(c, pos, aff)
        p.paint(c, pos, aff)
        assert p.form() == want, (k, rows)
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff), what='step %d' % k)
        close_readout(p.readout(field, pos, aff), oracle_readout(oracle, field_h, pos_h, oaff), abs(field_h).max(),
                      what='step %d' % k)
    # another particle set (a count outside an eighth of the last) starts a new history: the drops are forgotten
    pos = (base[: n // 2] + 0.05).contiguous()
    c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
    p.build(c, pos, aff)
    p.paint(c, pos, aff)
    assert p.form() == (True, 0)
    close_paint(c, oracle_paint(oracle, (N, N, N), pos.cpu().numpy(), oaff))


def test_blocks_auto_keeps_the_list_after_a_crowded_tile(hip, oracle, plan):
    """a build that sees a crowded tile (more rows than a workgroup's share: the list splits it, an entry tile cannot)
    makes 'auto' keep the list however coherent the rows; a change of BLOCKS resets the plan's history"""
    N, L = 128, 128.0
    aff, oaff = geometry(oracle, N, L)
    base = lattice(hip, N, L)
    crowded = base.clone()
    crowded[: 2 * N * N] *= torch.tensor([8.0 / N, 16.0 / N, 32.0 / N], dtype=torch.float64, device=hip.device)  # 32k rows in tile 0
    field_h = rand_field((N, N, N), 15)
    field = torch.from_numpy(field_h).to(hip.device)
    p = plan('auto', sort_pref=-1)

    def step(pos, want, what):
        pos_h = pos.cpu().numpy()
        c = torch.zeros((N, N, N), dtype=torch.float64, device=hip.device)
        p.build(c, pos, aff)
        p.paint(c, pos, aff)
        assert p.form() == want, what
        close_paint(c, oracle_paint(oracle, (N, N, N), pos_h, oaff), what=what)
        close_readout(p.readout(field, pos, aff), oracle_readout(oracle, field_h, pos_h, oaff), abs(field_h).max(),
                      what=what)
    for k in range(3):
        step(crowded + 0.01 * k, (False, 0), 'crowded %d' % k)
    step(base + 0.03, (False, 0), 'coherent after a crowded tile')
    p.configure('never')
    step(base + 0.04, (False, 0), 'never')
    p.configure('auto')
    step(base + 0.05, (True, 0), 'auto again: a new history')
    p.configure('always')
    step(crowded + 0.06, (True, 0), "'always' on the crowded rows")
