"""The statistics kernels at kernel level, on offset blocks, in every memory form and past the 65535-row launch grid:
pmx_power_project, pmx_power_vjp (csrc/pmx_power.hip, pmx_power_grad.hip), pmx_bispec_shells, pmx_bispec_shells_vjp,
pmx_bispec_reduce and pmx_bispec_pairsum (csrc/pmx_bispec.hip, pmx_bispec_grad.hip), each against a numpy restatement.

Coordinates.  `coords` below builds the global indices and wavenumbers of a block from numpy.arange alone, in the
rounding sequence csrc/pmx_block_dev.h documents as k_divided: s = i - N [i >= N // 2], w = s (2 pi / N), k = (w N) / L.
The CPU test asserts that it equals pm._block_coords bit for bit on every geometry used here, so the restatements of
tests/test_power.py and test_power_gradients.py (oracle_sums, oracle_vjp), which take k and idx as arguments, stand on
nothing of the package; and that oracle_sums is additive over the blocks of a tiling (counts equal, sums within 1e-13
of the scale S below), so a block with a non-zero start is restated as correctly as a whole field.

Forms.  The input, the second input, the outputs and the gradients of one call are in different forms of
tests/test_lpt.py (FORMS: contiguous, axes swapped, padded, strided), rotated through the list: no two arguments of a
call share strides (but in 1-d, where 'T' is 'C').  The values of a geometry are drawn once per dtype and copied into
every form, so one restatement serves all forms.

Bounds.
* power_project.  Counts (integers below 2^53 in double) are equal.  Every power, pole and (k, mu)-power column, per
  bin or cell: |got - want| <= 1e-12 S with S the same column of oracle_sums(|a|, |b|, ells=[0]), the sum of
  V |a| |b| (1 + h) / D over the modes of the bin, which bounds every column since |L_ell(mu)| <= 1.  1e-12 is the
  bound of test_power.assert_same; sqrt(n) 2^-53 for the at most 5e5 modes of a bin here is 8e-14.  The sums of |k|
  and of mu: 1e-12 count max|k| and 1e-12 count.  complex64 inputs take the same bounds: the kernel accumulates the
  same float values in double.  The accumulator starts at small non-zero integers (the kernel adds; integers keep the
  counts exact) which the comparison subtracts; the rounding of that addition, 2^-51 at most, is far below 1e-12 S.
* power_vjp.  test_power_gradients.same_field: 1e-12 of the largest |want| of the block, plus 2^-24 |component| for
  complex64 storage (a double rounded to float once).  Modes in no bin are exactly 0; an element left NaN fails.
* bispec_shells / shells_vjp.  The indicator and deconv_pow = 0 are copies: bit-equal.  deconv_pow = 2 divides the
  double by the window axis by axis as the restatement does: same_field.  The adjoint identity
  Re sum_s <outs_s, u_s> = Re <a, vjp(u)>: 1e-12 of sum |a| |u| for complex128, and for complex64 without a window
  (both kernels copy).  With complex64 storage and a window 1e-12 cannot hold: outs_s holds a / W and vjp(u) holds
  u / W rounded to float component by component, an error of at most 2^-24 |a| |u| / W per term on either side, so
  2 * 2^-24 sum |a| |u| / W is added to the bound (W is as small as 1 / 15 at the Nyquist corner).
* bispec_reduce: test_bispectrum.F8_TOL of sum |D_i D_j D_l| per triangle; bispec_pairsum:
  test_bispectrum_gradients.assert_pairsum.  Both as the existing kernel tests of the contiguous and padded forms.

The Hermitian weight.  power_kernel and power_vjp_kernel take the last-axis index of a mode from the fastest memory axis
(alast == 2), the middle one (1) or the slowest (0).  FORMS never moves the last logical axis away from the fastest
position, so the form tests reach alast == 2 only, and alast == 0 where the last axis has extent 1 (axes of extent 1
count as slowest: the last-axis planes il = 0 and il = 8 of the tiling test).  One more test swaps axes 1 and 2 in
memory and reaches alast == 1.

The tail of a tall block.  On the geometries with more rows than WRAP the rows from WRAP on are also compared alone,
on their own scale.  For power_project that is a second call on the view [WRAP:] with `start` advanced, against the
restatement of those rows (restated directly: the difference of the restatements of the whole block and of its first
WRAP rows carries the rounding of two sums 1e4 times larger than the tail's).  The test first asserts that every mode
of those rows lies inside a bin: they hold the largest |k| of the block, and edges that end below it would leave the
comparison empty.  shells_kernel and shells_vjp_kernel walk rows under the 65535-row cap of the launch grid with the
axes of extent 1 slowest, so of the tall blocks only the 3-d one, with outputs whose axis 0 is the slow one in memory
(every form but 'T'), makes a workgroup take a second trip; NaN-filled outputs show a row that no trip reached.
"""
import functools
import itertools

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd import pm as _pm
from pmesh_amd.bispectrum import triangle_bins
from tests.test_bispectrum import F8_TOL, _all_triples, _reduce_reference, assert_sums
from tests.test_bispectrum_gradients import _pairsum_reference, _random_list, assert_pairsum
from tests.test_lpt import FORMS, TALL, TALL_1D, WRAP, _block, _nan_block, cpu
from tests.test_power import _sinc_pow, oracle_sums
from tests.test_power_gradients import oracle_vjp, same_field

BOX = [100., 80., 120.]
GEOMS = [([16, 16, 9], [0, 0, 0], [16, 16, 16]),          # an r2c half spectrum
         ([45, 15, 45], [0, 30, 0], [45, 45, 45]),        # odd, a c2c block off the origin
         ([12, 48, 25], [36, 0, 0], [48, 48, 48]),        # slab in the negative half
         ([1, 48, 25], [24, 0, 0], [48, 48, 48]),         # the Nyquist plane alone: an extent-1 axis with nonzero start
         ([12, 24, 7], [36, 24, 18], [48, 48, 48]),       # pencil block; last axis 18..24 ends on Nyquist, never holds 0
         ([70, 3, 130], [0, 0, 0], [70, 3, 258]),         # more than one 16 x 16 x 64 tile along two axes, ragged tiles
         ([24, 17], [0, 0], [24, 32]),                    # 2-d
         ([300], [0], [598])] + TALL + TALL_1D            # 1-d; then more rows than WRAP
IDS = ['x'.join(str(n) for n in g[0]) + '@' + '.'.join(str(s) for s in g[1]) for g in GEOMS]
NG = len(GEOMS)
FINE = ([70, 3, 130], [12, 24, 7])                        # the geometries of the fine-edge parameter set
MUEDGES = numpy.array([-1, -0.7, -0.2, 0, 0.1, 0.5, 0.9, 1.0])
# the tiling of the additivity tests: one-plane slabs at and beside the Nyquist index 12 of axis 0, last-axis planes
# that hold only il = 0 and only the Nyquist il = 8
ADD_GEOM = ([24, 20, 9], [0, 0, 0], [24, 20, 16])
ADD_CUTS = ([0, 11, 12, 13, 24], [0, 7, 20], [0, 1, 8, 9])


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- 0. coordinates of a block, from numpy alone ---------------------------------------------------------------------

def _axes(shape, start, nmesh, box):
    """per axis (global index, w, k) of a block, each shaped to broadcast along its own axis"""
    nd = len(shape)
    out = []
    for d in range(nd):
        N, L = int(nmesh[d]), float(box[d])
        i = numpy.arange(int(shape[d]), dtype='i8') + int(start[d])
        s = (i - N * (i >= N // 2)).astype('f8')
        w = s * (2 * numpy.pi / N)
        k = (w * float(N)) / L
        along = [-1 if e == d else 1 for e in range(nd)]
        out.append((i.reshape(along), w.reshape(along), k.reshape(along)))
    return out


def coords(shape, start, nmesh, box):
    """(k, idx): per axis the wavenumbers and the global indices of a block"""
    ax = _axes(shape, start, nmesh, box)
    return [a[2] for a in ax], [a[0] for a in ax]


def kmag_of(shape, start, nmesh):
    k, _ = coords(shape, start, nmesh, BOX[:len(shape)])
    k2 = 0
    for kd in k:
        k2 = k2 + kd * kd
    return numpy.broadcast_to(numpy.sqrt(k2), tuple(shape))


def krange(geom):
    """the smallest non-zero and the largest |k| of a block"""
    km = kmag_of(*geom)
    return float(km[km > 0].min()), float(km.max())


def tiling(geom, cuts):
    """the blocks of a tiling of `geom`: (slices, (shape, start, nmesh))"""
    out = []
    for c in itertools.product(*[range(len(x) - 1) for x in cuts]):
        lo = [cuts[d][j] for d, j in enumerate(c)]
        hi = [cuts[d][j + 1] for d, j in enumerate(c)]
        sl = tuple(slice(a, b) for a, b in zip(lo, hi))
        out.append((sl, ([b - a for a, b in zip(lo, hi)], [s + a for s, a in zip(geom[1], lo)], geom[2])))
    return out


def tail_of(geom):
    """the rows from WRAP on of a tall block: (slices, (shape, start, nmesh))"""
    shape, start, nmesh = geom
    d = [n > WRAP for n in shape].index(True)
    sl = tuple(slice(WRAP, None) if e == d else slice(None) for e in range(len(shape)))
    return sl, ([n - WRAP if e == d else n for e, n in enumerate(shape)],
                [s + WRAP if e == d else s for e, s in enumerate(start)], nmesh)


def is_tall(geom):
    return max(geom[0]) > WRAP


# ---- parameter sets and restatements of the power kernels --------------------------------------------------------------

def holey_edges(kmin, kmax):
    """non-uniform k edges for a block whose non-zero |k| span [kmin, kmax]: the first edge above 0, the last below
    kmax, the first bin empty"""
    e = numpy.concatenate([[0.3 * kmin, 0.6 * kmin], numpy.geomspace(0.95 * kmin, 0.8 * kmax, 9)])
    assert (numpy.diff(e) > 0).all()
    return e


def param_sets(geom):
    nd = len(geom[0])
    kmin, kmax = krange(geom)
    last = numpy.zeros(nd)
    last[-1] = 1.0
    los = numpy.array([0.3, -0.5, 0.8][:nd])
    los = los / numpy.sqrt((los ** 2).sum())
    sets = [dict(cross=False, ke=numpy.linspace(0, kmax * 1.0001, 13), me=None, los=last, ells=(), deconv_pow=0,
                 hermitian=False),
            dict(cross=True, ke=holey_edges(kmin, kmax), me=MUEDGES, los=los, ells=(0, 1, 2, 4), deconv_pow=2,
                 hermitian=True)]
    if geom[0] in FINE:
        sets.append(dict(cross=False, ke=numpy.linspace(0, kmax, 4001), me=None, los=last, ells=(0, 2), deconv_pow=0,
                         hermitian=True))
    return sets


def power_params(nd, ps):
    p = _abi.Power()
    p.nk = len(ps['ke']) - 1
    p.nmu = 0 if ps['me'] is None else len(ps['me']) - 1
    p.npoles = len(ps['ells'])
    for i, ell in enumerate(ps['ells']):
        p.poles[i] = ell
    p.hermitian = int(ps['hermitian'])
    p.deconv_pow = ps['deconv_pow']
    p.volume = float(numpy.prod(BOX[:nd]))
    for d in range(nd):
        p.los[d] = float(ps['los'][d])
    return p


def restate_sums(av, bv, geom, ps):
    """(want, bound, counts): oracle_sums of the block, the bound of every entry of the accumulator (module docstring)
    and the mask of the count columns"""
    shape, start, nmesh = geom
    nd = len(shape)
    k, idx = coords(shape, start, nmesh, BOX[:nd])
    V = float(numpy.prod(BOX[:nd]))
    kw = dict(muedges=ps['me'], los=list(ps['los']), deconv_pow=ps['deconv_pow'], hermitian=ps['hermitian'])
    want = oracle_sums(av, bv if ps['cross'] else None, k, idx, nmesh, V, ps['ke'], ells=list(ps['ells']), **kw)
    sc = oracle_sums(numpy.abs(av), numpy.abs(bv) if ps['cross'] else None, k, idx, nmesh, V, ps['ke'], ells=[0], **kw)
    nk = len(ps['ke']) - 1
    nmu = 0 if ps['me'] is None else len(ps['me']) - 1
    s1 = 4 + 2 * len(ps['ells'])
    kmax = float(kmag_of(*geom).max())
    S1 = sc[:nk * 6].reshape(nk, 6)
    bound = numpy.zeros_like(want)
    counts = numpy.zeros(want.shape, dtype=bool)
    b1, c1 = bound[:nk * s1].reshape(nk, s1), counts[:nk * s1].reshape(nk, s1)
    c1[:, 0] = True
    b1[:, 1] = 1e-12 * S1[:, 0] * kmax
    b1[:, 2:] = 1e-12 * S1[:, 2][:, None]
    if nmu:
        S2 = sc[nk * 6:].reshape(nk, nmu, 5)
        b2, c2 = bound[nk * s1:].reshape(nk, nmu, 5), counts[nk * s1:].reshape(nk, nmu, 5)
        c2[..., 0] = True
        b2[..., 1] = 1e-12 * S2[..., 0] * kmax
        b2[..., 2] = 1e-12 * S2[..., 0]
        b2[..., 3:] = 1e-12 * S2[..., 3][..., None]
        assert (want[nk * s1:].reshape(nk, nmu, 5)[..., 0] == S2[..., 0]).all()
    assert (want[:nk * s1].reshape(nk, s1)[:, 0] == S1[:, 0]).all()
    return want, bound, counts


def assert_sums_within(got, want, bound, counts, what=''):
    assert numpy.isfinite(got).all()
    assert (got[counts] == want[counts]).all(), (what, numpy.nonzero(counts & (got != want))[0][:8])
    err = numpy.abs(got - want)
    pos = bound > 0
    print('%s: largest |got - want| / bound = %.3g over %d sums' % (what, (err[pos] / bound[pos]).max(), pos.sum()))
    bad = numpy.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, (what, bad[:8], err[bad[:8]], bound[bad[:8]])


_SHARED = []
_HELD = [None]


def shared(fn):
    """a function whose results the tests of one geometry and dtype share (see `hold`)"""
    fn = functools.lru_cache(maxsize=None)(fn)
    _SHARED.append(fn)
    return fn


def hold(key):
    """The drawn values and the restatements are computed once and shared by the tests that run one after the other
    on one geometry and dtype (the four forms: the parametrisations below put the form last); they are dropped when a
    test of another geometry or dtype begins, so no more than one geometry's worth is ever kept."""
    if _HELD[0] != key:
        for fn in _SHARED:
            fn.cache_clear()
        _HELD[0] = key


@shared
def values(shape, dtype, which):
    """the values of a block, drawn once per shape, dtype and role (shared: never written to)"""
    rng = numpy.random.RandomState(7919 * which + sum((i + 1) * n for i, n in enumerate(shape)))
    v = rng.normal(size=shape)
    if dtype in ('c16', 'c8'):
        v = v + 1j * rng.normal(size=shape)
    v = v.astype(dtype)
    v.setflags(write=False)
    return v


def gvalues(gi, dtype, which):
    return values(tuple(GEOMS[gi][0]), dtype, which)


@shared
def project_reference(gi, cdt, si):
    geom = GEOMS[gi]
    return restate_sums(gvalues(gi, cdt, 0), gvalues(gi, cdt, 1), geom, param_sets(geom)[si])


@shared
def vjp_reference(gi, cdt, si):
    """(coef, grad_a, grad_b, inside): a random coefficient table, non-zero in every bin, the gradients of oracle_vjp
    and the mask of the modes that lie in a k bin"""
    shape, start, nmesh = geom = GEOMS[gi]
    nd = len(shape)
    ps = param_sets(geom)[si]
    nk = len(ps['ke']) - 1
    nmu = 0 if ps['me'] is None else len(ps['me']) - 1
    coef = numpy.random.RandomState(100 + 10 * gi + si).normal(size=nk * (2 + 2 * len(ps['ells'])) + nk * nmu * 2)
    assert (coef != 0).all()
    k, idx = coords(shape, start, nmesh, BOX[:nd])
    ga, gb = oracle_vjp(gvalues(gi, cdt, 0), gvalues(gi, cdt, 1) if ps['cross'] else None, k, idx, nmesh,
                        float(numpy.prod(BOX[:nd])), ps['ke'], coef, ps['me'], list(ps['los']), list(ps['ells']),
                        ps['deconv_pow'], ps['hermitian'])
    kb = numpy.digitize(kmag_of(*geom), ps['ke']) - 1
    return coef, ga, gb, (kb >= 0) & (kb < nk)


# ---- blocks in the forms of tests/test_lpt.py ---------------------------------------------------------------------------

def form_after(form, n):
    return FORMS[(FORMS.index(form) + n) % len(FORMS)]


def place(vals, form, rng):
    """_block in `form` holding `vals`"""
    t = _block(tuple(vals.shape), vals.dtype, form, rng, complex_=vals.dtype.kind == 'c')
    t.copy_(torch.from_numpy(numpy.array(vals)))
    return t


def _root(t):
    return t if t._base is None else t._base


def like(t, vals=None):
    """a new block of the shape, dtype and strides of `t` in a buffer of its own: `vals`, or NaN, in the block and a
    sentinel in the elements of the buffer that the block does not name"""
    base = torch.full_like(_root(t), -7.0)
    v = torch.as_strided(base, t.size(), t.stride(), t.storage_offset())
    if vals is not None:
        v.copy_(torch.from_numpy(numpy.array(vals)))
    else:
        v.fill_(complex(float('nan'), float('nan')) if t.is_complex() else float('nan'))
    return v


def snapshot(ts):
    return [_root(t).clone() for t in ts]


def assert_rest_untouched(ts, before, what):
    """the elements of the buffers under the views `ts` that the views do not name still hold what `before` holds"""
    for t, b in zip(ts, before):
        now, b = _root(t).clone(), b.clone()
        for x in (now, b):
            torch.as_strided(x, t.size(), t.stride(), t.storage_offset()).zero_()
        assert torch.equal(now, b), what


def dev_f8(be, x):
    return None if x is None else torch.from_numpy(numpy.asarray(x, dtype='f8')).to(be.device)


# ---- 0. CPU: the coordinates and the additivity of the restatement -----------------------------------------------------

def test_coords_equal_block_coords_and_the_restatement_is_additive():
    hold('cpu')
    geoms = GEOMS + [ADD_GEOM] + [g for _, g in tiling(ADD_GEOM, ADD_CUTS)] + [tail_of(g)[1] for g in TALL + TALL_1D]
    for shape, start, nmesh in geoms:
        nd = len(shape)
        k, idx = coords(shape, start, nmesh, BOX[:nd])
        pk, pi = _pm._block_coords(list(start), tuple(shape), list(nmesh), BOX[:nd], 'f8', 'cpu', True)
        for d in range(nd):
            assert k[d].dtype == numpy.float64 and pk[d].numpy().dtype == numpy.float64
            assert k[d].shape == tuple(pk[d].shape) and idx[d].shape == tuple(pi[d].shape)
            assert (k[d].view('u8') == pk[d].numpy().view('u8')).all(), (shape, start, d)
            assert (idx[d] == pi[d].numpy()).all(), (shape, start, d)
    # oracle_sums over the 24 blocks of the tiling adds up to oracle_sums of the whole half spectrum
    blocks = tiling(ADD_GEOM, ADD_CUTS)
    assert len(blocks) == 24
    a, b = values(tuple(ADD_GEOM[0]), 'c16', 0), values(tuple(ADD_GEOM[0]), 'c16', 1)
    ps = param_sets(ADD_GEOM)[1]
    whole, bound, counts = restate_sums(a, b, ADD_GEOM, ps)
    total = sum(restate_sums(a[sl], b[sl], g, ps)[0] for sl, g in blocks)
    assert whole[counts].sum() > 0 and (total[counts] == whole[counts]).all()
    pos = bound > 0
    rel = numpy.abs(total - whole)[pos] / (bound[pos] / 1e-12)
    print('additivity of oracle_sums: largest difference / scale = %.3g' % rel.max())
    assert (numpy.abs(total - whole) <= 0.1 * bound).all()          # 1e-13 of the scale


# ---- 2. pmx_power_project ----------------------------------------------------------------------------------------------

def _project(be, ps, a, b, geom, acc):
    shape, start, nmesh = geom
    nd = len(shape)
    be.power_project(power_params(nd, ps), a, b if ps['cross'] else None, list(start), list(nmesh), BOX[:nd],
                     dev_f8(be, ps['ke']), dev_f8(be, ps['me']), acc)


def _projected(be, ps, a, b, geom, rng, n):
    """the sums the kernel adds to a non-zero accumulator"""
    acc0 = rng.randint(1, 4, size=n).astype('f8')
    acc = torch.tensor(acc0, device=be.device)
    _project(be, ps, a, b, geom, acc)
    return cpu(acc) - acc0


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', range(NG), ids=IDS)
def test_power_project(hipbe, form, cdt, gi):
    hold((gi, cdt))
    rng = numpy.random.RandomState(11)
    geom = GEOMS[gi]
    a = place(gvalues(gi, cdt, 0), form, rng)
    b = place(gvalues(gi, cdt, 1), form_after(form, 1), rng)
    for si, ps in enumerate(param_sets(geom)):
        want, bound, counts = project_reference(gi, cdt, si)
        assert want[counts].sum() > 0
        if si == 1:
            # the holey edges: the first bin empty, modes above the last edge (and k = 0, where the block holds it,
            # below the first)
            assert ps['ke'][0] > 0 and want[0] == 0 and (kmag_of(*geom) >= ps['ke'][-1]).any()
        got = _projected(hipbe, ps, a, b, geom, rng, want.size)
        assert_sums_within(got, want, bound, counts, 'set %d' % si)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', [i for i in range(NG) if is_tall(GEOMS[i])], ids=[i for i, g in zip(IDS, GEOMS) if is_tall(g)])
def test_power_project_rows_past_the_launch_grid(hipbe, form, cdt, gi):
    """the rows from WRAP on alone: a call on the view [WRAP:] with `start` advanced"""
    hold((gi, cdt))
    rng = numpy.random.RandomState(12)
    geom = GEOMS[gi]
    sl, tail = tail_of(geom)
    av, bv = gvalues(gi, cdt, 0), gvalues(gi, cdt, 1)
    a = place(av, form, rng)
    b = place(bv, form_after(form, 1), rng)
    auto, cross = param_sets(geom)[:2]
    cross = dict(cross, ke=auto['ke'])                   # edges that end above the largest |k| of the block
    for ps in (auto, cross):
        nk = len(ps['ke']) - 1
        kb = numpy.digitize(kmag_of(*tail), ps['ke']) - 1
        assert ((kb >= 0) & (kb < nk)).all(), 'a mode of the rows from WRAP on lies in no bin'
        want, bound, counts = restate_sums(av[sl], bv[sl], tail, ps)
        got = _projected(hipbe, ps, a[sl], b[sl], tail, rng, want.size)
        assert_sums_within(got, want, bound, counts, 'rows from WRAP on')


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
def test_power_project_is_additive_over_blocks(hipbe, form, cdt):
    """the 24 blocks of a tiling of a half spectrum, each a view of the whole tensor with its `start`, projected into
    one accumulator: the single call on the whole field; and each block alone: oracle_sums of that block"""
    hold(('tiling', cdt))
    rng = numpy.random.RandomState(13)
    av, bv = values(tuple(ADD_GEOM[0]), cdt, 0), values(tuple(ADD_GEOM[0]), cdt, 1)
    a = place(av, form, rng)
    b = place(bv, form_after(form, 1), rng)
    ps = param_sets(ADD_GEOM)[1]
    want, bound, counts = restate_sums(av, bv, ADD_GEOM, ps)
    whole = _projected(hipbe, ps, a, b, ADD_GEOM, rng, want.size)
    assert_sums_within(whole, want, bound, counts, 'whole')
    acc0 = rng.randint(1, 4, size=want.size).astype('f8')
    acc = torch.tensor(acc0, device=hipbe.device)
    for sl, g in tiling(ADD_GEOM, ADD_CUTS):
        w1, b1, c1 = restate_sums(av[sl], bv[sl], g, ps)
        assert_sums_within(_projected(hipbe, ps, a[sl], b[sl], g, rng, want.size), w1, b1, c1, 'block %s' % (g[1],))
        _project(hipbe, ps, a[sl], b[sl], g, acc)
    assert_sums_within(cpu(acc) - acc0, whole, bound, counts, 'sum of the blocks')


# ---- 3. pmx_power_vjp --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', range(NG), ids=IDS)
def test_power_vjp(hipbe, form, cdt, gi):
    hold((gi, cdt))
    rng = numpy.random.RandomState(14)
    shape, start, nmesh = geom = GEOMS[gi]
    nd = len(shape)
    storage = {'c16': 'f8', 'c8': 'f4'}[cdt]
    a = place(gvalues(gi, cdt, 0), form, rng)
    b = place(gvalues(gi, cdt, 1), form_after(form, 1), rng)
    a0, b0 = a.clone(), b.clone()
    for si, ps in enumerate(param_sets(geom)[:2]):
        coef, wa, wb, inside = vjp_reference(gi, cdt, si)
        assert inside.all() if si == 0 else (0 < inside.sum() < inside.size)
        ga = _nan_block(shape, cdt, form_after(form, 2), rng)
        gb = _nan_block(shape, cdt, form_after(form, 3), rng) if ps['cross'] else None
        outs = [ga] + ([gb] if ps['cross'] else [])
        before = snapshot(outs)
        hipbe.power_vjp(power_params(nd, ps), a, b if ps['cross'] else None, ga, gb, list(start), list(nmesh), BOX[:nd],
                        dev_f8(hipbe, ps['ke']), dev_f8(hipbe, ps['me']), dev_f8(hipbe, coef))
        for got, want in zip(outs, [wa, wb]):
            got = cpu(got)
            same_field(got, want, storage)
            assert (got[~inside] == 0).all(), 'a mode in no bin is not exactly 0'
            if is_tall(geom):
                sl, _ = tail_of(geom)
                same_field(got[sl], want[sl], storage)
        assert_rest_untouched(outs, before, 'an element outside the gradient block was written')
    assert torch.equal(a, a0) and torch.equal(b, b0)


# ---- the Hermitian weight with the last axis in the middle of memory ---------------------------------------------------

def place_12(vals, rng):
    """a 3-d block with axes 1 and 2 swapped in memory (not among FORMS): the last logical axis is the middle one"""
    n0, n1, n2 = vals.shape
    big = (rng.normal(size=(n0, n2, n1)) + 1j * rng.normal(size=(n0, n2, n1))).astype(vals.dtype)
    t = torch.from_numpy(big).to(backend.get().device).transpose(1, 2)
    t.copy_(torch.from_numpy(numpy.array(vals)))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', [0, 4], ids=[IDS[0], IDS[4]])
def test_power_hermitian_weight_last_axis_in_the_middle(hipbe, gi, cdt):
    """In every form of FORMS the last logical axis is the fastest in memory (alast == 2 in power_kernel and
    power_vjp_kernel), or the slowest when its extent is 1 (alast == 0: the one-plane blocks of the tiling test).  With
    axes 1 and 2 swapped in memory it is the middle one (alast == 1) and the row index carries the Hermitian weight: the
    half spectrum and the pencil block that ends on the Nyquist index, parameter set 2, project and vjp"""
    hold((gi, cdt))
    rng = numpy.random.RandomState(19)
    shape, start, nmesh = geom = GEOMS[gi]
    storage = {'c16': 'f8', 'c8': 'f4'}[cdt]
    a = place_12(gvalues(gi, cdt, 0), rng)
    assert a.stride(1) < a.stride(2) < a.stride(0)
    b = place(gvalues(gi, cdt, 1), 'pad', rng)
    ps = param_sets(geom)[1]
    assert ps['hermitian']
    want, bound, counts = project_reference(gi, cdt, 1)
    assert_sums_within(_projected(hipbe, ps, a, b, geom, rng, want.size), want, bound, counts, 'set 1')
    coef, wa, wb, inside = vjp_reference(gi, cdt, 1)
    ga, gb = like(a), _nan_block(shape, cdt, 'strided', rng)
    hipbe.power_vjp(power_params(3, ps), a, b, ga, gb, list(start), list(nmesh), BOX, dev_f8(hipbe, ps['ke']),
                    dev_f8(hipbe, ps['me']), dev_f8(hipbe, coef))
    for got, w in ((cpu(ga), wa), (cpu(gb), wb)):
        same_field(got, w, storage)
        assert (got[~inside] == 0).all(), 'a mode in no bin is not exactly 0'


# ---- 4. pmx_bispec_shells and pmx_bispec_shells_vjp --------------------------------------------------------------------

def shell_edge_sets(geom):
    """nb = 1, 5 and 64 shells that cover every mode of the block, and 5 uneven shells that leave modes outside
    (nb = 64 not on the tall blocks: 64 outputs of 4e5 complex128 are 400 MB)"""
    kmin, kmax = krange(geom)
    sets = [numpy.linspace(0, kmax * 1.0001, nb + 1) for nb in ((1, 5) if is_tall(geom) else (1, 5, 64))]
    sets.append(kmin + (kmax - kmin) * numpy.array([0.1, 0.15, 0.4, 0.45, 0.7, 0.9]))
    return sets


@shared
def shell_map(gi, ei):
    """the shell of every mode of a block (-1: none) by numpy.digitize of |k|, and whether the edges cover the block"""
    geom = GEOMS[gi]
    ke = shell_edge_sets(geom)[ei]
    sh = numpy.digitize(kmag_of(*geom), ke) - 1
    sh[(sh < 0) | (sh >= len(ke) - 1)] = -1
    covers = ei < len(shell_edge_sets(geom)) - 1
    assert (sh >= 0).all() if covers else ((sh < 0).any() and (sh >= 0).any())
    return sh


def over_window(v, geom, p):
    """v / prod_d sinc(w_d / 2)^p, divided axis by axis, component by component, in double"""
    shape, start, nmesh = geom
    v = numpy.asarray(v).astype('c16')
    re, im = v.real.copy(), v.imag.copy()
    if p:
        for _, w, _ in _axes(shape, start, nmesh, BOX[:len(shape)]):
            sp = _sinc_pow(w, p)
            re, im = re / sp, im / sp
    return re + 1j * im


def bit_equal(got, want):
    got, want = numpy.ascontiguousarray(got), numpy.ascontiguousarray(want).astype(got.dtype)
    return ((got.real == want.real) & (got.imag == want.imag)).all()


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', range(NG), ids=IDS)
def test_bispec_shells(hipbe, form, cdt, gi):
    hold((gi, cdt))
    rng = numpy.random.RandomState(15)
    shape, start, nmesh = geom = GEOMS[gi]
    nd = len(shape)
    storage = {'c16': 'f8', 'c8': 'f4'}[cdt]
    av = gvalues(gi, cdt, 0)
    a = place(av, form, rng)
    a0 = a.clone()
    first = _nan_block(shape, cdt, form_after(form, 1), rng)
    for ei, ke in enumerate(shell_edge_sets(geom)):
        nb = len(ke) - 1
        sh = shell_map(gi, ei)
        outs = [first] + [like(first) for _ in range(nb - 1)]
        before = snapshot(outs)
        for unit, p in ((True, 0), (False, 0), (False, 2)):
            for o in outs:
                o.fill_(complex(float('nan'), float('nan')))
            hipbe.bispec_shells(None if unit else a, outs, list(start), list(nmesh), BOX[:nd], dev_f8(hipbe, ke), p, unit)
            src = numpy.ones(tuple(shape), dtype='c16') if unit else over_window(av, geom, p)
            for s, o in enumerate(outs):
                got = cpu(o)
                assert numpy.isfinite(got.real).all() and numpy.isfinite(got.imag).all(), 'an element not written'
                want = numpy.where(sh == s, src, 0)
                if p:
                    same_field(got, want, storage)
                    assert (got[sh != s] == 0).all()
                else:
                    assert bit_equal(got, want), (nb, s, unit)
        assert_rest_untouched(outs, before, 'an element outside an output block was written')
    assert torch.equal(a, a0)


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', range(NG), ids=IDS)
def test_bispec_shells_vjp(hipbe, form, cdt, gi):
    hold((gi, cdt))
    rng = numpy.random.RandomState(16)
    shape, start, nmesh = geom = GEOMS[gi]
    nd = len(shape)
    storage = {'c16': 'f8', 'c8': 'f4'}[cdt]
    av = gvalues(gi, cdt, 0)
    a = place(av, form_after(form, 2), rng)
    for ei, ke in enumerate(shell_edge_sets(geom)):
        nb = len(ke) - 1
        sh = shell_map(gi, ei)
        kt = dev_f8(hipbe, ke)
        uv = [gvalues(gi, cdt, 2 + s) for s in range(nb)]
        first = place(uv[0], form, rng)
        ins = [first] + [like(first, u) for u in uv[1:]]
        picked = numpy.zeros(tuple(shape), dtype='c16')
        for s, u in enumerate(uv):
            picked = numpy.where(sh == s, u, picked)
        for p in (0, 2):
            out = _nan_block(shape, cdt, form_after(form, 1), rng)
            before = snapshot([out])
            hipbe.bispec_shells_vjp(ins, out, list(start), list(nmesh), BOX[:nd], kt, p)
            got = cpu(out)
            want = over_window(picked, geom, p)
            if p:
                same_field(got, want, storage)
            else:
                assert bit_equal(got, want)
            assert (got[sh < 0] == 0).all(), 'a mode in no shell is not exactly 0'
            if is_tall(geom):
                sl, _ = tail_of(geom)
                assert numpy.isfinite(got[sl].real).all() and numpy.isfinite(got[sl].imag).all()
                same_field(got[sl], want[sl], storage)
            assert_rest_untouched([out], before, 'an element outside the output block was written')
            # the adjoint identity with the forward on this block: Re sum_s <outs_s, u_s> == Re <a, vjp(u)>
            outs = [like(out) for _ in range(nb)]
            hipbe.bispec_shells(a, outs, list(start), list(nmesh), BOX[:nd], kt, p, False)
            lhs = sum(float((numpy.conj(cpu(o).astype('c16')) * u.astype('c16')).real.sum()) for o, u in zip(outs, uv))
            rhs = float((numpy.conj(av.astype('c16')) * got.astype('c16')).real.sum())
            scale = float((numpy.abs(av.astype('c16')) * numpy.abs(picked)).sum())
            bound = 1e-12 * scale
            if storage == 'f4' and p:
                # a departure from 1e-12, which float storage cannot meet: outs_s holds a / W and vjp(u) holds u / W
                # rounded to float, component by component, so each term of either side is off by at most
                # 2^-24 |a| |u| / W (want = picked / W carries the 1 / W, up to 15 at the Nyquist corner)
                bound += 2 * 2.0 ** -24 * float((numpy.abs(av.astype('c16')) * numpy.abs(want)).sum())
            print('adjoint identity: |lhs - rhs| = %.3g, bound %.3g, sum |a| |u| = %.3g' % (abs(lhs - rhs), bound, scale))
            assert abs(lhs - rhs) <= bound and scale > 0
        for t, u in zip(ins, uv):
            assert torch.equal(t.cpu(), torch.from_numpy(numpy.array(u))), 'an input has changed'


# ---- 5. pmx_bispec_reduce and pmx_bispec_pairsum in every form of real block ---------------------------------------------

REAL_SHAPES = [(5, 7, 11), (9, 10, 13), (700, 3), (37,)]   # (9, 10, 13): three ragged chunks at K = 8, more at 4 and 2


def real_blocks(shape, rdt, nb):
    return [values(shape, rdt, s) for s in range(nb)]


def triangle_lists(nb):
    """the lists of test_bispectrum.test_kernel_reduce"""
    lists = [_all_triples(nb)[-1:], triangle_bins(numpy.arange(nb + 1) + 0.5)]
    if nb == 33:
        lists.append(_all_triples(33))
    return lists


@shared
def reduce_reference(shape, rdt, nb, li):
    return _reduce_reference(real_blocks(shape, rdt, nb), triangle_lists(nb)[li])


@shared
def pair_list(nb):
    return _random_list(numpy.random.RandomState(nb), nb, 12, bad=3)


@shared
def pairsum_reference(shape, rdt, nb):
    return _pairsum_reference(real_blocks(shape, rdt, nb), *pair_list(nb))


def placed_fields(blocks, form, rng):
    first = place(blocks[0], form, rng)
    return [first] + [like(first, b) for b in blocks[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rdt', ['f8', 'f4'])
@pytest.mark.parametrize('nb', [7, 33, 64])
def test_bispec_reduce_forms(hipbe, form, rdt, nb):
    hold((rdt, nb))
    rng = numpy.random.RandomState(17)
    for shape in REAL_SHAPES:
        fields = placed_fields(real_blocks(shape, rdt, nb), form, rng)
        before = snapshot(fields)
        for li, tri in enumerate(triangle_lists(nb)):
            want, scale = reduce_reference(shape, rdt, nb, li)
            acc = torch.zeros(len(tri), dtype=torch.float64, device=hipbe.device)
            hipbe.bispec_reduce(fields, torch.from_numpy(tri).to(hipbe.device), acc)
            assert_sums(cpu(acc), want, scale, F8_TOL)
        for t, b in zip(fields, before):
            assert torch.equal(_root(t), b), 'a field has changed'


@pytest.mark.gpu
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('rdt', ['f8', 'f4'])
@pytest.mark.parametrize('nb', [7, 33, 64])
def test_bispec_pairsum_forms(hipbe, form, rdt, nb):
    hold((rdt, nb))
    rng = numpy.random.RandomState(18)
    offsets, pairs, weights = pair_list(nb)
    assert ((pairs < 0) | (pairs >= nb)).any()
    ot, pt, wt = (torch.from_numpy(x).to(hipbe.device) for x in (offsets, pairs, weights))
    for shape in REAL_SHAPES:
        blocks = real_blocks(shape, rdt, nb)
        G, A = pairsum_reference(shape, rdt, nb)
        # out of place into NaN outputs: every cell written, nothing else, the fields as they were
        fields = placed_fields(blocks, form, rng)
        outs = [like(fields[0]) for _ in range(nb)]
        fbefore, obefore = snapshot(fields), snapshot(outs)
        hipbe.bispec_pairsum(fields, outs, ot, pt, wt)
        assert_pairsum(numpy.stack([cpu(o) for o in outs]), G, A, rdt)
        assert_rest_untouched(outs, obefore, 'an element outside an output block was written')
        for t, b in zip(fields, fbefore):
            assert torch.equal(_root(t), b), 'out of place: a field has changed'
        # in place: outs[s] is fields[s]
        hipbe.bispec_pairsum(fields, fields, ot, pt, wt)
        assert_pairsum(numpy.stack([cpu(f) for f in fields]), G, A, rdt)
        assert_rest_untouched(fields, fbefore, 'in place: an element outside a block was written')
        for f, o in zip(fields, outs):
            assert torch.equal(f, o), 'in place and out of place differ'
