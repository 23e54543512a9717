"""pmesh_amd.mock (csrc/pmx_poisson.hip) against a numpy restatement of its sampling rule.

The rule is pinned to a counter-based generator (Philox4x32-10 on the global cell index), so the restatement — a
vectorised Philox, the chunked inversion, the offsets — gives the very counts, positions and order the kernels must
give.  Under -m "not gpu" it serves pmx_poisson_rate_sum, pmx_poisson_count, pmx_poisson_scan and pmx_poisson_emit
(MockOracleBackend), so the host layer — arguments, the allocation between scan and emit, the sums over ranks, the
lognormal normalisation — runs without a GPU; under -m gpu the kernels are compared with it.

The comparison rule for counts: the device's exp may differ from numpy's in the last place.  The restatement therefore
also draws with u - 1e-13 and u + 1e-13 (the count is monotone in u), which covers one ulp of exp on p and on the rate
and at most 128 rounded additions on s <= 1.  Every input of the kernel tests has lo == hi in ALL cells — a condition
on the inputs, checked without a GPU by test_kernel_inputs_are_decided and asserted again before every comparison —
and then the counts must equal lo exactly.  Positions involve no transcendental function and are compared exactly.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import backend
from pmesh_amd.mock import (LognormalCatalog, PoissonSample, lognormal_catalog, philox4x32, poisson_sample,
                            poisson_seed)
from pmesh_amd.pm import ParticleMesh
from pmesh_amd.power import power_spectrum
from pmesh_amd.transfer import Tabulated
from tests.test_correlation import CorrOracleBackend
from tests.test_interlace import BLOCKS
from tests.test_lpt import FORMS, LptOracleBackend, cpu, table

SEG = 4096
MAXRATE = 2.0 ** 20
DU = 1e-13
LINEAR, EXP = 0, 1


# ---- the restatement -----------------------------------------------------------------------------------------------

_U = numpy.uint64
MASK = _U(0xffffffff)
M0, M1, W0, W1 = _U(0xD2511F53), _U(0xCD9E8D57), _U(0x9E3779B9), _U(0xBB67AE85)
S32 = _U(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64: the four output words"""
    c0, c1, c2, c3, k0, k1 = numpy.broadcast_arrays(*[numpy.asarray(v).astype('u8') & MASK
                                                      for v in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def cell_words(g, j, stream, seed):
    g = numpy.asarray(g).astype('u8')
    return philox(g & MASK, g >> S32, j, stream, int(seed) & 0xffffffff, int(seed) >> 32)


def count_uniform(w):
    """u in (0, 1] of a chunk from the first two words"""
    return ((w[0] >> _U(5)).astype('f8') * 2.0 ** 26 + (w[1] >> _U(6)).astype('f8') + 1.0) * 2.0 ** -53


def invert(u, lam):
    """inversion by sequential search, every element on its own: p * lam / k rounds twice"""
    u, lam = numpy.asarray(u, dtype='f8'), numpy.asarray(lam, dtype='f8')
    k = numpy.zeros(u.shape, dtype='i8')
    p = numpy.exp(-lam)
    s = p.copy()
    live = numpy.flatnonzero(u > s)              # the elements still searching, with their own u, lam, p and s
    u, lam, p, s = u[live], lam[live], p[live], s[live]
    for step in range(1, 129):
        if live.size == 0:
            break
        p = p * lam / step
        s = s + p
        k[live] = step
        go = u > s
        live, u, lam, p, s = live[go], u[go], lam[go], p[go], s[go]
    return k


def global_index(shape, start, nmesh):
    """the global C-order index of every cell of a block, and its global index per axis"""
    axes = [numpy.arange(n, dtype='i8') + int(s) for n, s in zip(shape, start)]
    idx = numpy.meshgrid(*axes, indexing='ij')
    g = numpy.zeros(tuple(shape), dtype='i8')
    for i, n in zip(idx, nmesh):
        g = g * int(n) + i
    return g, idx


def rates(x, mode, scale, bias):
    x = numpy.asarray(x).astype('f8')
    with numpy.errstate(all='ignore'):
        return scale * numpy.exp(bias * x) if mode == EXP else scale * x


def ref_counts(x, start, nmesh, mode, scale, bias, seed):
    """(lo, mid, hi) counts of the block drawn with u - DU, u, u + DU, and the mask of the refused cells"""
    lam = rates(x, mode, scale, bias)
    shape = lam.shape
    g, _ = global_index(shape, start, nmesh)
    with numpy.errstate(invalid='ignore'):
        good = (lam >= 0) & (lam <= MAXRATE)
    lamg, gg = lam[good], g[good]
    n = numpy.maximum(1, numpy.ceil(lamg / 16.0)).astype('i8')
    owner = numpy.repeat(numpy.arange(len(n)), n)
    j = numpy.arange(len(owner)) - numpy.repeat(numpy.cumsum(n) - n, n)
    lj = numpy.repeat(lamg / n, n)
    u = count_uniform(cell_words(numpy.repeat(gg, n), j, 0, seed))
    out = []
    for du in (-DU, 0.0, DU):
        k = numpy.bincount(owner, weights=invert(u + du, lj), minlength=len(n))
        c = numpy.zeros(shape, dtype='i8')
        c[good] = numpy.rint(k).astype('i8')
        out.append(c)
    return out[0], out[1], out[2], ~good


def seg_sums(counts):
    flat = numpy.asarray(counts).reshape(-1).astype('i8')
    nseg = (len(flat) + SEG - 1) // SEG
    return numpy.concatenate([flat, numpy.zeros(nseg * SEG - len(flat), 'i8')]).reshape(nseg, SEG).sum(axis=1)


def offsets(w, nd):
    """u_d in (0, 1) per axis from the words of a particle"""
    return [(w[d].astype('f8') + 0.5) * 2.0 ** -32 for d in range(nd)]


def ref_emit(counts, start, nmesh, box, seed):
    """the rows and global cell indices of the particles of a block of counts"""
    counts = numpy.asarray(counts).astype('i8')
    nd = counts.ndim
    box = numpy.ones(nd) * numpy.asarray(box, dtype='f8')
    g, idx = global_index(counts.shape, start, nmesh)
    c = counts.reshape(-1)
    cells = numpy.repeat(g.reshape(-1), c)
    p = numpy.arange(len(cells)) - numpy.repeat(numpy.cumsum(c) - c, c)
    w = cell_words(cells, p, 1, seed)
    pos = numpy.empty((len(cells), nd))
    for d, u in enumerate(offsets(w, nd)):
        i = numpy.repeat(numpy.broadcast_to(idx[d], counts.shape).reshape(-1), c).astype('f8')
        L = float(box[d])
        x = ((i - 0.5) + u) * (L / float(int(nmesh[d])))
        x = numpy.where(x < 0, x + L, x)
        pos[:, d] = numpy.where(x >= L, 0.0, x)
    return pos, cells


class MockOracleBackend(CorrOracleBackend, LptOracleBackend):
    """the CPU test double (with the spectra of tests/test_correlation.py and the tabulated transfer of
    tests/test_lpt.py, for the downstream steps) with the four entries of csrc/pmx_poisson.hip served by the
    restatement"""
    name = 'oracle-mock'

    def poisson_rate_sum(self, x, mode, scale, bias, total):
        if x.numel():
            total += float(rates(x.numpy(), mode, scale, bias).sum())

    def poisson_count(self, x, start, nmesh, mode, scale, bias, seed, counts, seg_sums_, flagged):
        if x.numel() == 0:
            return
        _, mid, _, bad = ref_counts(x.numpy(), start, nmesh, mode, scale, bias, seed)
        counts.copy_(torch.from_numpy(mid.astype('u4')))
        seg_sums_.copy_(torch.from_numpy(seg_sums(mid)))
        flagged += int(bad.sum())

    def poisson_scan(self, seg_sums_, total):
        s = seg_sums_.numpy().copy()
        seg_sums_.copy_(torch.from_numpy(numpy.cumsum(s) - s))
        total[0] = int(s.sum())

    def poisson_emit(self, shape, start, nmesh, boxsize, seed, counts, seg_offsets, pos, cell=None):
        if pos.shape[0] == 0:
            return
        c = counts.numpy().reshape(tuple(shape))
        assert (seg_offsets.numpy() == numpy.cumsum(seg_sums(c)) - seg_sums(c)).all()
        p, g = ref_emit(c, start, nmesh, boxsize, seed)
        pos.copy_(torch.from_numpy(p))
        if cell is not None:
            cell.copy_(torch.from_numpy(g))


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(MockOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def mbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(MockOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- 1. the restatement itself --------------------------------------------------------------------------------------

KNOWN = [((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          'd16cfe09 94fdcceb 5001e420 24126ea1')]


def test_philox_known_answers():
    """the known answers of Philox4x32-10 (the Random123 test vectors), from the restatement and from the host's own
    implementation (which derives the Poisson seed of a lognormal catalogue)"""
    for ctr, key, want in KNOWN:
        w = philox(*[numpy.array([c]) for c in ctr], *[numpy.array([k]) for k in key])
        assert ' '.join('%08x' % int(x[0]) for x in w) == want
        assert ' '.join('%08x' % x for x in philox4x32(ctr, key)) == want
    # all three at once: the vectorised form
    w = philox(*[numpy.array([k[0][i] for k in KNOWN]) for i in range(4)],
               *[numpy.array([k[1][i] for k in KNOWN]) for i in range(2)])
    assert [' '.join('%08x' % int(x[i]) for x in w) for i in range(3)] == [k[2] for k in KNOWN]
    assert poisson_seed(7) != 7 and poisson_seed(7) == poisson_seed(7) and poisson_seed(7) != poisson_seed(8)


NSTAT = 200000


def stat_counts(lam, seed):
    x = numpy.full(NSTAT, lam)
    lo, mid, hi, bad = ref_counts(x, [0], [NSTAT], LINEAR, 1.0, 0.0, seed)
    assert not bad.any()
    return lo, mid, hi


@pytest.mark.parametrize('lam', [0.05, 1.0, 7.3, 16.0, 40.0, 300.0])
def test_counts_are_poisson(lam):
    """mean and variance of 2e5 counts within 5 standard errors of lambda: sqrt(lam / n) for the mean and
    sqrt((lam + 2 lam^2) / n) for the variance (the fourth central moment of a Poisson variate is lam + 3 lam^2); and
    no count depends on a perturbation of u by 1e-13"""
    lo, c, hi = stat_counts(lam, seed=11)
    assert (lo == hi).all()
    mean, var = c.mean(), c.var(ddof=1)
    print('lambda %g: mean %.5f variance %.5f' % (lam, mean, var))
    assert abs(mean - lam) <= 5 * numpy.sqrt(lam / NSTAT)
    assert abs(var - lam) <= 5 * numpy.sqrt((lam + 2 * lam * lam) / NSTAT)


def test_histogram_at_rate_one():
    """chi^2 of the lambda = 1 histogram over the 8 bins 0..6 and >= 7 against the Poisson probabilities: 7 degrees of
    freedom, below 24.32, the 0.999 quantile"""
    from math import exp, factorial
    _, c, _ = stat_counts(1.0, seed=12)
    prob = [exp(-1.0) / factorial(k) for k in range(7)]
    prob.append(1.0 - sum(prob))
    hist = numpy.bincount(numpy.minimum(c, 7), minlength=8)
    chi2 = float((((hist - NSTAT * numpy.array(prob)) ** 2) / (NSTAT * numpy.array(prob))).sum())
    print('chi^2 = %.2f on 8 bins' % chi2)
    assert chi2 < 24.32


def test_offsets_and_positions_are_inside():
    """offsets in (0, 1) at the extreme words, positions in [0, L) with the cells of index 0 wrapped"""
    w = [numpy.array([0, 0xffffffff], dtype='u8')] * 3
    for u in offsets(w, 3):
        assert (u > 0).all() and (u < 1).all()
    rng = numpy.random.RandomState(1)
    counts = rng.poisson(3.0, size=(5, 4, 6))
    box = [40., 30., 50.]
    pos, cells = ref_emit(counts, [0, 0, 0], [5, 4, 6], box, 99)
    assert len(pos) == counts.sum() and (numpy.diff(cells) >= 0).all()
    assert (pos >= 0).all() and (pos < numpy.array(box)).all()
    # a nearest-grid-point assignment of the positions returns the counts
    i = numpy.rint(pos * (numpy.array([5, 4, 6]) / numpy.array(box))).astype('i8') % numpy.array([5, 4, 6])
    back = numpy.zeros_like(counts)
    numpy.add.at(back, tuple(i.T), 1)
    assert (back == counts).all()
    assert (pos[:, 0] > 40. - 4.).any()          # some particle of a cell at index 0 lies below the grid point


# ---- 2. the inputs of the kernel tests ------------------------------------------------------------------------------

BOX = [40., 30., 50.]


def uniform_rates(shape, dtype, seed, top=2.0):
    rng = numpy.random.RandomState(seed)
    x = rng.uniform(0, top, size=tuple(shape))
    x[rng.uniform(size=tuple(shape)) < 0.1] = 0.0          # exact zeros
    return x.astype(dtype)


def special_rates():
    """(17, 16, 19): 5168 cells, two segments, the second partial; a cell of rate 5000 on either side of the segment
    boundary (313 chunks, its particles wider than a wave), a rate of exactly 16 (one chunk) and the next double above
    it (two chunks)"""
    x = uniform_rates((17, 16, 19), 'f8', 21, top=3.0).reshape(-1)
    x[SEG - 1] = 5000.0
    x[SEG + 1] = 5000.0
    x[100] = 16.0
    x[101] = numpy.nextafter(16.0, 17.0)
    x[5167] = 2.5
    return x.reshape(17, 16, 19)


def kernel_cases():
    """name -> (values, start, nmesh, mode, scale, bias, seed): every input of the kernel tests"""
    cases = {}
    for dtype in ('f8', 'f4'):
        for n, (shape, start, nmesh) in enumerate(BLOCKS):
            cases['block%d-%s' % (n, dtype)] = (uniform_rates(shape, dtype, 30 + n), start, nmesh, LINEAR, 1.5, 0.0,
                                                (0x9e3779b97f4a7c15 + n) & (2 ** 64 - 1))
    cases['special'] = (special_rates(), [0, 0, 0], [17, 16, 19], LINEAR, 1.0, 0.0, 5)
    cases['special-offset'] = (special_rates(), [3, 0, 1], [21, 16, 20], LINEAR, 1.0, 0.0, 2 ** 63 + 12345)
    cases['1d'] = (uniform_rates((4099,), 'f8', 41, top=3.0), [7], [5000], LINEAR, 1.0, 0.0, 6)
    cases['2d'] = (uniform_rates((65, 64), 'f8', 42, top=3.0), [3, 0], [70, 64], LINEAR, 1.0, 0.0, 7)
    cases['2d-f4'] = (uniform_rates((65, 64), 'f4', 43, top=3.0), [0, 0], [65, 64], LINEAR, 1.0, 0.0, 8)
    gauss = numpy.random.RandomState(44).normal(size=(17, 16, 19))
    cases['exp'] = (gauss, [0, 0, 0], [17, 16, 19], EXP, 0.8, 1.7, 9)
    cases['exp-f4'] = (gauss.astype('f4'), [0, 0, 0], [17, 16, 19], EXP, 0.8, 1.7, 10)
    cases['dense'] = (numpy.full((16, 16, 16), 20.0), [0, 0, 0], [16, 16, 16], LINEAR, 1.0, 0.0, 11)
    return cases


CASES = kernel_cases()
_REFERENCE = {}


def reference(name):
    """the restatement's (lo, hi, refused, rows, cells) of a case, computed once"""
    if name not in _REFERENCE:
        x, start, nmesh, mode, scale, bias, seed = CASES[name]
        lo, _, hi, bad = ref_counts(x, start, nmesh, mode, scale, bias, seed)
        pos, cells = ref_emit(lo, start, nmesh, BOX[:x.ndim], seed)
        _REFERENCE[name] = (lo, hi, bad, pos, cells)
    return _REFERENCE[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_inputs_are_decided(name):
    """the condition of the comparison rule: lo == hi in all cells of every input; and the cases hold what they are
    for"""
    lo, hi, bad, pos, cells = reference(name)
    assert (lo == hi).all() and not bad.any()
    assert lo.sum() > 0
    if name.startswith('special'):
        flat = lo.reshape(-1)
        assert flat[SEG - 1] > 4000 and flat[SEG + 1] > 4000 and (flat == 0).any()
    if name == 'dense':
        assert lo.sum() > 65536


def place(vals, form, dev):
    """the values as a device tensor in one of the memory forms of tests/test_lpt.py:_block"""
    shape = vals.shape
    if form == 'T' and len(shape) == 1:
        form = 'C'
    if form == 'T':
        big = torch.zeros((shape[1], shape[0]) + tuple(shape[2:]), dtype=torch.from_numpy(vals).dtype, device=dev)
        t = big.transpose(0, 1)
    elif form == 'pad':
        big = torch.full(tuple(shape[:-1]) + (shape[-1] + 3,), float('nan'), dtype=torch.from_numpy(vals).dtype,
                         device=dev)
        t = big[..., :shape[-1]]
    elif form == 'strided':
        big = torch.full(tuple(2 * s for s in shape), float('nan'), dtype=torch.from_numpy(vals).dtype, device=dev)
        t = big[tuple(slice(None, None, 2) for _ in shape)]
    else:
        t = torch.empty(tuple(shape), dtype=torch.from_numpy(vals).dtype, device=dev)
    t.copy_(torch.from_numpy(numpy.ascontiguousarray(vals)).to(dev))
    return t


def run_kernels(be, x, start, nmesh, box, mode, scale, bias, seed, cells=True):
    """the four entries on the device tensor x: (counts, segment sums, flagged, segment offsets, total, rows, cells)"""
    dev = be.device
    ncells = x.numel()
    nseg = (ncells + SEG - 1) // SEG
    counts = torch.full(tuple(x.shape), 0xdeadbeef, dtype=torch.int64, device=dev).to(torch.uint32)
    seg = torch.full((nseg,), -7, dtype=torch.int64, device=dev)
    head = torch.zeros(2, dtype=torch.int64, device=dev)
    be.poisson_count(x, start, nmesh, mode, scale, bias, seed, counts, seg, head[1:2])
    sums = cpu(seg).copy()
    be.poisson_scan(seg, head[0:1])
    total, flagged = [int(v) for v in cpu(head)]
    pos = torch.full((total, x.dim()), float('nan'), dtype=torch.float64, device=dev)
    cell = torch.full((total,), -1, dtype=torch.int64, device=dev) if cells else None
    be.poisson_emit(tuple(x.shape), start, nmesh, box, seed, counts, seg, pos, cell)
    return cpu(counts).astype('i8'), sums, flagged, cpu(seg), total, cpu(pos), None if cell is None else cpu(cell)


def check_case(be, name, form):
    x, start, nmesh, mode, scale, bias, seed = CASES[name]
    lo, hi, bad, want_pos, want_cells = reference(name)
    assert (lo == hi).all()                                     # the condition of the comparison rule
    t = place(x, form, be.device)
    before = cpu(t).copy()
    counts, sums, flagged, offs, total, pos, cells = run_kernels(be, t, start, nmesh, BOX[:x.ndim], mode, scale, bias,
                                                                 seed)
    assert numpy.array_equal(cpu(t), before)
    assert flagged == 0
    assert numpy.array_equal(counts, lo), (name, form, numpy.abs(counts - lo).max())
    assert numpy.array_equal(sums, seg_sums(lo))
    assert numpy.array_equal(offs, numpy.cumsum(sums) - sums) and total == lo.sum()
    assert numpy.array_equal(cells, want_cells)
    assert numpy.array_equal(pos, want_pos), (name, form)
    # the rate sum: one rounding per addition of a sum of one sign, in any order (5168 cells: 1.2e-12 of the sum)
    want = rates(x, mode, scale, bias).astype(numpy.longdouble).sum()
    rsum = torch.zeros(1, dtype=torch.float64, device=be.device)
    be.poisson_rate_sum(t, mode, scale, bias, rsum)
    assert abs(float(cpu(rsum)[0]) - float(want)) <= (x.size * 2.0 ** -53 + 4e-16) * float(want)


# ---- 3. the kernels against the restatement (GPU) -------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_kernels_on_blocks(hipbe, dtype, form):
    """offset blocks inside larger meshes in every memory form, f8 and f4, a scale of 1.5 and seeds beyond 2^32"""
    for n in range(len(BLOCKS)):
        check_case(hipbe, 'block%d-%s' % (n, dtype), form)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', ['special', 'special-offset', '1d', '2d', '2d-f4', 'exp', 'exp-f4', 'dense'])
def test_kernels_on_cases(hipbe, name, form):
    """two segments with the second partial, exact zeros, cells of rate 5000 at the segment boundary, the rates 16 and
    the next double; 1-d (4099,) and 2-d (65, 64); mode EXP with bias 1.7 on a Gaussian field; a segment of more than
    65536 particles"""
    check_case(hipbe, name, form)


@pytest.mark.gpu
def test_refused_rates_are_counted(hipbe):
    """NaN, -1, inf and 2^20 + 1 cells, in both segments: count 0 and flagged == 4, every other cell as the restatement
    has it; the host layer raises ValueError"""
    x = uniform_rates((17, 16, 19), 'f8', 51, top=3.0)
    flat = x.reshape(-1)
    where = [5, SEG - 2, SEG + 7, 5100]
    flat[where] = [numpy.nan, -1.0, numpy.inf, MAXRATE + 1]
    lo, _, hi, bad = ref_counts(x, [0, 0, 0], [17, 16, 19], LINEAR, 1.0, 0.0, 13)
    assert (lo == hi).all() and bad.sum() == 4 and (lo.reshape(-1)[where] == 0).all()
    t = place(x, 'C', hipbe.device)
    counts, sums, flagged, offs, total, pos, cells = run_kernels(hipbe, t, [0] * 3, [17, 16, 19], BOX, LINEAR, 1.0, 0.0,
                                                                 13)
    assert flagged == 4
    assert numpy.array_equal(counts, lo) and numpy.array_equal(sums, seg_sums(lo))
    want_pos, want_cells = ref_emit(lo, [0] * 3, [17, 16, 19], BOX, 13)
    assert numpy.array_equal(pos, want_pos) and numpy.array_equal(cells, want_cells)
    # the host layer raises
    pm = ParticleMesh([17, 16, 19], BoxSize=BOX)
    f = pm.create(type='real')
    f.value[...] = t
    with pytest.raises(ValueError, match='4 cells'):
        poisson_sample(f, scale=1.0, seed=13)


@pytest.mark.gpu
def test_scan_kernel_passes_2_to_the_32(hipbe):
    """3000 segment sums of 2^21 each: the offsets pass 2^32 and the total is exact; three tiles of the scan, the last
    partial.  Then sums of every size, and the empty array"""
    dev = hipbe.device
    for sums in (numpy.full(3000, 2 ** 21, dtype='i8'),
                 numpy.random.RandomState(3).randint(0, 2 ** 40, size=2049).astype('i8'),
                 numpy.array([5], dtype='i8'), numpy.zeros(0, dtype='i8')):
        seg = torch.from_numpy(sums.copy()).to(dev)
        total = torch.full((1,), -1, dtype=torch.int64, device=dev)
        hipbe.poisson_scan(seg, total)
        assert numpy.array_equal(cpu(seg), numpy.cumsum(sums) - sums)
        assert int(cpu(total)[0]) == int(sums.sum())
    assert 3000 * 2 ** 21 > 2 ** 32


@pytest.mark.gpu
def test_two_launches_give_identical_arrays(hipbe):
    x, start, nmesh, mode, scale, bias, seed = CASES['special']
    t = place(x, 'C', hipbe.device)
    a = run_kernels(hipbe, t, start, nmesh, BOX, mode, scale, bias, seed)
    b = run_kernels(hipbe, t, start, nmesh, BOX, mode, scale, bias, seed)
    for u, v in zip(a, b):
        assert numpy.array_equal(u, v)
    # and without the cell indices: the same rows
    c = run_kernels(hipbe, t, start, nmesh, BOX, mode, scale, bias, seed, cells=False)
    assert c[6] is None and numpy.array_equal(c[5], a[5])


def two_blocks_case(be):
    """the same mesh sampled through two blocks of different start: the cells both hold get the same counts and the
    same particles"""
    nmesh = [12, 10, 14]
    full = uniform_rates(nmesh, 'f8', 61, top=3.0)
    out = []
    for start, shape in (([0, 0, 0], [8, 6, 10]), ([3, 2, 4], [8, 6, 10])):
        sl = tuple(slice(s, s + n) for s, n in zip(start, shape))
        t = place(full[sl], 'C', be.device)
        counts, _, flagged, _, _, pos, cells = run_kernels(be, t, start, nmesh, BOX, LINEAR, 1.0, 0.0, 17)
        assert flagged == 0
        mesh = numpy.full(nmesh, -1, dtype='i8')
        mesh[sl] = counts
        out.append((mesh, pos, cells))
    (ma, pa, ca), (mb, pb, cb) = out
    both = (ma >= 0) & (mb >= 0)
    assert both.sum() == 5 * 4 * 6 and (ma[both] == mb[both]).all() and ma[both].sum() > 0
    shared = numpy.flatnonzero(both.reshape(-1))
    ka, kb = numpy.isin(ca, shared), numpy.isin(cb, shared)
    assert numpy.array_equal(ca[ka], cb[kb]) and numpy.array_equal(pa[ka], pb[kb])


def test_two_blocks_agree_where_they_overlap(mbe):
    two_blocks_case(mbe)


# ---- 4. poisson_sample ----------------------------------------------------------------------------------------------

def analytic_field(pm, dtype=None):
    """a positive field that is a function of the global cell index alone: the same values on every decomposition"""
    f = pm.create(type='real')
    g, _ = global_index(tuple(f.value.shape), f.start, pm.Nmesh)
    vals = 1.0 + 0.8 * numpy.sin(0.37 * g) * numpy.cos(0.011 * g * g)
    f.value[...] = torch.from_numpy(vals).to(f.value.device).to(f.value.dtype)
    return f


@pytest.mark.parametrize('Nmesh', [[8, 6, 10], [32, 32, 32], [9, 14], [50]])
def test_nnb_paint_returns_the_counts(mbe, Nmesh):
    """end to end: pm.paint(pos, resampler='nnb') equals counts exactly; csize, size and the shapes"""
    pm = ParticleMesh(Nmesh, BoxSize=BOX[:len(Nmesh)])
    f = analytic_field(pm)
    before = f.value.clone()
    s = poisson_sample(f, nbar=2.0 / (numpy.prod(pm.BoxSize) / numpy.prod(pm.Nmesh)), seed=23, return_cells=True)
    assert isinstance(s, PoissonSample) and torch.equal(f.value, before)
    assert s.pos.dtype == torch.float64 and tuple(s.pos.shape) == (s.size, len(Nmesh)) and s.pos.is_contiguous()
    assert s.counts.dtype == torch.uint32 and tuple(s.counts.shape) == tuple(f.value.shape)
    counts = cpu(s.counts).astype('i8')
    assert s.size == s.csize == counts.sum() and s.size > numpy.prod(Nmesh)
    assert abs(s.expected - 2.0 * float(cpu(f.value).sum())) <= 1e-12 * s.expected
    assert abs(s.size - s.expected) <= 5 * numpy.sqrt(s.expected)
    painted = pm.paint(s.pos, resampler='nnb')
    assert numpy.array_equal(cpu(painted.value), counts.astype('f8'))
    assert numpy.array_equal(cpu(s.cells), numpy.repeat(numpy.arange(counts.size), counts.reshape(-1)))
    pos = cpu(s.pos)
    assert (pos >= 0).all() and (pos < numpy.asarray(pm.BoxSize)).all()
    # without the cells: the same rows; another seed: other rows
    again = poisson_sample(f, scale=2.0, seed=23)
    assert again.cells is None and torch.equal(again.pos, s.pos) and torch.equal(again.counts, s.counts)
    other = poisson_sample(f, scale=2.0, seed=24)
    assert not numpy.array_equal(cpu(other.counts), cpu(s.counts))


def test_f4_field_and_exp_mode(mbe):
    pm = ParticleMesh([8, 6, 10], BoxSize=BOX, dtype='f4')
    f = analytic_field(pm)
    assert f.value.dtype == torch.float32
    s = poisson_sample(f, scale=1.5, seed=3, mode='exp', bias=0.7, return_cells=True)
    x = cpu(f.value)
    lo, mid, hi, bad = ref_counts(x, [0, 0, 0], [8, 6, 10], EXP, 1.5, 0.7, 3)
    assert (lo == hi).all() and not bad.any()
    assert numpy.array_equal(cpu(s.counts).astype('i8'), lo)
    want_pos, want_cells = ref_emit(lo, [0, 0, 0], [8, 6, 10], BOX, 3)
    assert numpy.array_equal(cpu(s.pos), want_pos) and numpy.array_equal(cpu(s.cells), want_cells)
    assert abs(s.expected - rates(x, EXP, 1.5, 0.7).sum()) <= 1e-12 * s.expected


def test_empty_result(mbe):
    pm = ParticleMesh([8, 6, 10], BoxSize=BOX)
    f = pm.create(type='real')
    f.value[...] = 0
    s = poisson_sample(f, nbar=1.0, seed=1, return_cells=True)
    assert tuple(s.pos.shape) == (0, 3) and s.size == 0 and s.csize == 0 and s.expected == 0
    assert tuple(s.cells.shape) == (0,) and int(cpu(s.counts).astype('i8').sum()) == 0


def test_bad_arguments(obe):
    pm = ParticleMesh([8, 6, 10], BoxSize=BOX)
    f = analytic_field(pm)
    with pytest.raises(TypeError):
        poisson_sample(numpy.ones((8, 6, 10)), nbar=1.0)
    with pytest.raises(TypeError):
        poisson_sample(f.r2c(), nbar=1.0)
    with pytest.raises(NotImplementedError):
        poisson_sample(ParticleMesh([4, 4, 4, 4], BoxSize=1.).create(type='real'), nbar=1.0)
    with pytest.raises(ValueError, match='nbar'):
        poisson_sample(f)
    with pytest.raises(ValueError, match='nbar'):
        poisson_sample(f, nbar=1.0, scale=2.0)
    with pytest.raises(ValueError, match='mode'):
        poisson_sample(f, nbar=1.0, mode='log')
    with pytest.raises(ValueError, match='seed'):
        poisson_sample(f, nbar=1.0, seed=-1)
    with pytest.raises(ValueError, match='seed'):
        poisson_sample(f, nbar=1.0, seed=2 ** 64)
    with pytest.raises(ValueError, match='finite'):
        poisson_sample(f, nbar=numpy.inf)
    with pytest.raises(ValueError, match='complex-to-complex'):
        poisson_sample(ParticleMesh([8, 8, 8], BoxSize=1., dtype='c16').create(type='real'), nbar=1.0)
    # refused cells: one of each kind
    for bad in (numpy.nan, -1.0, numpy.inf, MAXRATE + 1):
        h = analytic_field(pm)
        h.value[2, 3, 4] = bad
        with pytest.raises(ValueError, match='1 cells'):
            poisson_sample(h, scale=1.0)
    h = analytic_field(pm)
    h.value[2, 3, 4] = MAXRATE                     # the largest rate itself is drawn
    assert abs(int(cpu(poisson_sample(h, scale=1.0).counts)[2, 3, 4]) - MAXRATE) < 6 * 1024
    # lognormal_catalog
    k, p = table()
    tab = Tabulated(k, numpy.sqrt(p / numpy.prod(pm.BoxSize)), loglog=True)
    with pytest.raises(TypeError, match='transfer'):
        lognormal_catalog(pm, lambda k, v: v, 1.0, 1)
    with pytest.raises(NotImplementedError):
        lognormal_catalog(ParticleMesh([4, 4, 4, 4], BoxSize=1.), tab, 1.0, 1)
    with pytest.raises(ValueError, match='seed'):
        lognormal_catalog(pm, tab, 1.0, 2 ** 32)
    with pytest.raises(ValueError, match='nbar'):
        lognormal_catalog(pm, tab, -1.0, 1)


def sample_ranks_case(comm=None, np_=None, Nmesh=(8, 6, 10)):
    kw = {} if comm is None else dict(comm=comm, np=np_)
    pm = ParticleMesh(list(Nmesh), BoxSize=BOX, **kw)
    s = poisson_sample(analytic_field(pm), scale=1.7, seed=2 ** 40 + 9, return_cells=True)
    return cpu(s.pos), cpu(s.cells), s.size, s.csize, s.expected


def gather_rows(results):
    """the rows of all ranks sorted by cell and then by order of appearance"""
    pos = numpy.concatenate([results[r][0] for r in sorted(results)])
    cells = numpy.concatenate([results[r][1] for r in sorted(results)])
    order = numpy.argsort(cells, kind='stable')
    return pos[order], cells[order]


def thread_ranks(size, case, **kw):
    from tests import thread_comm
    results = {}

    def body(comm):
        results[comm.rank] = case(comm, **kw)
    thread_comm.run_ranks(size, body)
    assert len(results) == size
    return results


@pytest.mark.parametrize('size,np_', [(2, [2]), (3, [3]), (4, [2, 2])])
def test_ranks_give_the_one_rank_rows(obe, size, np_):
    """the rows of all ranks, sorted by cell and then by order of appearance, equal the one-rank rows exactly; csize and
    expected are equal on every rank"""
    results = thread_ranks(size, sample_ranks_case, np_=np_)
    pos1, cells1, size1, csize1, expected1 = sample_ranks_case()
    pos, cells = gather_rows(results)
    assert numpy.array_equal(cells, cells1) and numpy.array_equal(pos, pos1)
    assert sum(r[2] for r in results.values()) == size1 == csize1
    assert len(set(r[2] for r in results.values())) > 1 or size == 1
    for r in results.values():
        assert r[3] == csize1 and r[4] == results[0][4]
        assert abs(r[4] - expected1) <= 1e-12 * expected1


def test_ranks_raise_together(obe):
    """a refused cell on one rank raises on every rank"""
    raised = []

    def case(comm, np_):
        pm = ParticleMesh([8, 6, 10], BoxSize=BOX, comm=comm, np=np_)
        f = analytic_field(pm)
        if comm.rank == 1:
            f.value[0, 0, 0] = -1.0
        with pytest.raises(ValueError, match='1 cells'):
            poisson_sample(f, scale=1.0)
        raised.append(comm.rank)
    thread_ranks(2, case, np_=[2])
    assert sorted(raised) == [0, 1]


def test_shot_noise(obe):
    """a constant field on a 16^3 mesh with nbar V_cell = 2, painted with NNB: the counts of the cells are independent,
    so delta = counts / mean - 1 is white with P = V / N in every bin, within 5 P sqrt(2 / modes)"""
    pm = ParticleMesh([16, 16, 16], BoxSize=100.)
    f = pm.create(type='real')
    f.value[...] = 1.0
    vcell = 100. ** 3 / 16 ** 3
    s = poisson_sample(f, nbar=2.0 / vcell, seed=31)
    assert abs(s.expected - 2.0 * 16 ** 3) <= 1e-9 and abs(s.size - s.expected) <= 5 * numpy.sqrt(s.expected)
    delta = pm.paint(s.pos, resampler='nnb')
    delta.value[...] *= 16 ** 3 / float(s.size)
    delta.value[...] -= 1.0
    kf = 2 * numpy.pi / 100.
    res = power_spectrum(delta, numpy.arange(0.5, 9.0, 1.0) * kf)
    shot = 100. ** 3 / s.size
    assert (res.modes > 0).all()
    dev = numpy.abs(res.power.real - shot) / (shot * numpy.sqrt(2.0 / res.modes))
    print('shot noise: deviations in sigma', numpy.round(dev, 2))
    assert (dev <= 5).all()
    assert (numpy.abs(res.power.imag) <= 1e-9 * shot).all()


# ---- 5. lognormal_catalog -------------------------------------------------------------------------------------------

def lognormal_case(comm=None, np_=None, Nmesh=(16, 12, 10), displacement=True, seed=77):
    kw = {} if comm is None else dict(comm=comm, np=np_)
    pm = ParticleMesh(list(Nmesh), BoxSize=200., **kw)
    k, p = table()
    tab = Tabulated(k, numpy.sqrt(100 * p / numpy.prod(pm.BoxSize)), loglog=True)
    nbar = 3.0 * numpy.prod(pm.Nmesh) / numpy.prod(pm.BoxSize)
    cat = lognormal_catalog(pm, tab, nbar, seed, bias=1.5, displacement=displacement, return_cells=True)
    assert isinstance(cat, LognormalCatalog)
    disp = None if cat.displacement is None else cat.displacement
    if disp is not None:
        assert tuple(disp.shape) == tuple(cat.pos.shape) and disp.dtype == cat.pos.dtype
    return (cpu(cat.pos), cpu(cat.cells), cat.size, cat.csize, cat.expected, None if disp is None else cpu(disp),
            cat.mean, cat.poisson_seed, cpu(cat.delta_k.c2r().value), cpu(cat.counts).astype('i8'))


def check_lognormal(Nmesh):
    pos, cells, size, csize, expected, disp, mean, pseed, delta_g, counts = lognormal_case(Nmesh=Nmesh)
    ncells = int(numpy.prod(Nmesh))
    assert size == csize == len(pos) and pseed == poisson_seed(77)
    # the normalisation: the expected number is nbar V = 3 per cell, whatever the field
    assert abs(expected - 3.0 * ncells) <= 1e-9 * expected
    assert abs(size - expected) <= 5 * numpy.sqrt(expected)
    assert delta_g.std() > 0.05 and abs(mean - numpy.exp(1.5 * delta_g).mean()) <= 1e-12 * mean
    assert disp.shape == pos.shape and numpy.isfinite(disp).all() and numpy.abs(disp).max() > 0
    # the catalogue is the rule applied to the field it reports, under the derived seed
    scale = 3.0 / mean
    lo, _, hi, bad = ref_counts(delta_g, [0] * 3, Nmesh, EXP, scale, 1.5, pseed)
    assert (lo == hi).all() and not bad.any()                   # the condition of the comparison rule
    assert numpy.array_equal(counts, lo)
    want_pos, want_cells = ref_emit(counts, [0] * 3, Nmesh, [200.] * 3, pseed)
    assert numpy.array_equal(pos, want_pos) and numpy.array_equal(cells, want_cells)
    return pos, cells, disp, expected


def test_lognormal_catalog(obe):
    check_lognormal([16, 12, 10])
    # no displacement unless asked for; 2-d and 1-d meshes
    assert lognormal_case(displacement=False)[5] is None
    for Nmesh in ([12, 10], [32]):
        pos = lognormal_case(Nmesh=Nmesh, displacement=False)[0]
        assert pos.shape[1] == len(Nmesh) and len(pos) > 0


def check_lognormal_ranks(size, np_, Nmesh):
    """the thread-rank catalogue equals the one-rank catalogue row for row after sorting by cell (the displacement,
    read from fields that were transformed along another schedule, within 1e-9 of its largest value)"""
    results = thread_ranks(size, lognormal_case, np_=np_, Nmesh=Nmesh)
    one = lognormal_case(Nmesh=Nmesh)
    pos, cells = gather_rows(results)
    assert numpy.array_equal(cells, one[1]) and numpy.array_equal(pos, one[0])
    disp = numpy.concatenate([results[r][5] for r in sorted(results)])
    order = numpy.argsort(numpy.concatenate([results[r][1] for r in sorted(results)]), kind='stable')
    assert numpy.abs(disp[order] - one[5]).max() <= 1e-9 * numpy.abs(one[5]).max()
    for r in results.values():
        assert r[3] == one[3] and abs(r[4] - one[4]) <= 1e-9 * one[4]


@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [2, 2])])
def test_lognormal_ranks(obe, size, np_):
    check_lognormal_ranks(size, np_, (16, 12, 10))


@pytest.mark.gpu
def test_lognormal_catalog_on_the_device(hipbe):
    """a 32^3 mesh: size within 5 sqrt(expected) of expected, the displacement of the shape and dtype of pos, and the
    catalogue equal to the rule applied to its own Gaussian field"""
    check_lognormal([32, 32, 32])


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', [(2, [2]), (4, [2, 2])])
def test_lognormal_ranks_on_the_device(hipbe, size, np_):
    check_lognormal_ranks(size, np_, (32, 32, 32))


# ---- 6. resources (compiles for gfx950 on the CPU) ------------------------------------------------------------------

def test_poisson_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_poisson.hip')
    # rate_sum_kernel / count_kernel<T, EXP> for f4 / f8 and both modes, emit_kernel<NDIM, CELL>, one scan_kernel
    counts = {'rate_sum_kernel': 4, 'count_kernel': 4, 'emit_kernel': 6, 'scan_kernel': 1}
    for key, n in counts.items():
        assert len([k for k in t if key in k]) == n, sorted(t)
    assert len(t) == sum(counts.values()), sorted(t)
    for name, r in t.items():
        assert r['ScratchSize'] == 0, (name, r)
        assert r['VGPRs'] <= 64, (name, r)           # seven or eight waves per SIMD
        if 'emit_kernel' in name:
            assert r['LDS'] <= 16384 + 1024 + 64, (name, r)   # the segment's offsets and the threads' sums
