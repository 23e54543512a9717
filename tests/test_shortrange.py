"""pmesh_amd.shortrange (csrc/pmx_shortrange.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/shortrange.py, include/pmesh_amd.h).  Rows are (n, 3), wrapped into [0, L_d) by FoF's rule; dx_d
= x_i,d - x_j,d is the minimum image of the wrapped rows; all arithmetic is double; r2 = dx_0^2 + dx_1^2 + dx_2^2 in
that order.  Source j is a neighbour of primary i when 0 < r2 < rc2, rc2 = r_cut * r_cut; pairs with r2 == 0
contribute nothing.  With r = sqrt(r2), u = r / (2 r_split), s2 = r2 + softening^2 and fac = erfc(u) + (2 / sqrt(pi))
u exp(-u^2): acc_i,d = -G sum_j m_j dx_d fac / (s2 sqrt(s2)), pot_i = -G sum_j m_j erfc(u) / sqrt(s2), neighbours_i
the number of neighbours.

The restatement is brute force: the full (n1, n2) matrices, scipy.special.erfc.  Under -m "not gpu" it serves
pmx_short_range (ShortRangeOracleBackend), so the host layer and the thread ranks run without a GPU; under -m gpu the
kernel is compared with it.

neighbours is compared by exact integer equality everywhere.  acc and pot are compared per row and component within
|got - ref| <= (M_i + 64) 2^-52 S_i: M_i the row's neighbour count, S_i the sum of the absolute values of its terms:
the worst case of a double sum in any order, plus 64 ulp for one term.  The 64 ulp are derived, not measured: OpenCL's
full-profile bounds for erfc (16 ulp) and exp (3 ulp), the latter conditioned by 2 u^2 <= 10.2 at u <= 2.25 on about
2 ulp of u, plus the square roots, the division and the products.  The tests therefore keep r_cut <= 4.5 r_split.

The condition on random inputs: no pair with |r2 - rc2| < 1e-9 rc2 (a contracted multiply-add could otherwise move a
pair across the cut); test_inputs_are_decided asserts it without a GPU for every random case.  The lattice cases are
exact; their pairs on the cut and at r2 == 0 test the two strict comparisons themselves.
"""
import os

import numpy
import pytest
import torch
from scipy.special import erfc

from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid, cell_sort
from pmesh_amd.shortrange import RCUT, local_force, short_range_force
from pmesh_amd.transfer import Transfer
from tests.test_fof import (GRIDS, PERIODIC, RANKS, ROW_FORMS, SLAB, UNIT, WAVE_NS, FofOracleBackend, crowded,
                            face_pairs, lattice, mesh, place, split, thread_ranks, uniform, wrap)
from tests.test_lpt import cpu

U = 2.0 ** -52
ULPS = 64                                # of one term: the derivation of the module docstring
CHUNK = 512                              # primaries per block of the brute-force matrices


# ---- the restatement -----------------------------------------------------------------------------------------------

def force_core(w1, w2, box, m2, G, r_split, rc2, eps2):
    """The sums of the wrapped rows w1 from the wrapped rows w2 with the masses m2 (None: 1).  Returns a dict: acc
    (n1, 3), pot (n1,), neighbours (n1,) int64; Sacc, Spot: the sums of the absolute values of the terms; margin: the
    smallest |r2 - rc2| / rc2 over all pairs."""
    n1, n2 = len(w1), len(w2)
    out = dict(acc=numpy.zeros((n1, 3)), pot=numpy.zeros(n1), neighbours=numpy.zeros(n1, dtype='i8'),
               Sacc=numpy.zeros((n1, 3)), Spot=numpy.zeros(n1), margin=numpy.inf)
    if n1 == 0 or n2 == 0:
        return out
    m = numpy.ones(n2) if m2 is None else numpy.asarray(m2).astype('f8').reshape(-1)
    for lo in range(0, n1, CHUNK):
        a = w1[lo:lo + CHUNK]
        dx = []
        for d in range(3):
            x = a[:, None, d] - w2[None, :, d]
            dx.append(x - box[d] * numpy.rint(x / box[d]))
        r2 = dx[0] * dx[0]
        r2 = r2 + dx[1] * dx[1]
        r2 = r2 + dx[2] * dx[2]
        keep = (r2 > 0) & (r2 < rc2)
        out['margin'] = min(out['margin'], float(numpy.abs(r2 - rc2).min() / rc2))
        safe = numpy.where(keep, r2, 1.0)
        s2 = safe + eps2
        ss = numpy.sqrt(s2)
        r = numpy.sqrt(safe)
        u = r / (2 * r_split)
        ec = erfc(u)
        fac = ec + 2 / numpy.sqrt(numpy.pi) * u * numpy.exp(-(u * u))
        f = numpy.where(keep, m[None, :] * fac / (s2 * ss), 0.0)
        p = numpy.where(keep, m[None, :] * ec / ss, 0.0)
        sl = slice(lo, lo + len(a))
        for d in range(3):
            out['acc'][sl, d] = -G * (dx[d] * f).sum(axis=1)
            out['Sacc'][sl, d] = abs(G) * numpy.abs(dx[d] * f).sum(axis=1)
        out['pot'][sl] = -G * p.sum(axis=1)
        out['Spot'][sl] = abs(G) * numpy.abs(p).sum(axis=1)
        out['neighbours'][sl] = keep.sum(axis=1)
    return out


def ref_force(pos, box, r_split, r_cut=None, mass=None, pos2=None, mass2=None, softening=0.0, G=1.0):
    """the restatement of short_range_force(mesh(box), pos, r_split, r_cut, mass, pos2, mass2, softening, G)"""
    box = numpy.asarray(box, dtype='f8')
    rc = RCUT * r_split if r_cut is None else float(r_cut)
    a = wrap(pos, box)
    auto = pos2 is None
    return force_core(a, a if auto else wrap(pos2, box), box, mass if auto else mass2, float(G), float(r_split),
                      rc * rc, float(softening) ** 2)


class ShortRangeOracleBackend(FofOracleBackend):
    """the CPU test double with pmx_short_range served by the restatement"""
    name = 'oracle-shortrange'

    def short_range(self, spos1, order1, cell_of1, spos2, order2, cell_start2, mass2, ncell, periodic, boxsize, G,
                    r_split, rc2, eps2, acc, pot=None, neighbours=None):
        n1, n2 = spos1.shape[0], spos2.shape[0]
        if n1 == 0:
            return
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell))
        # the rows back in row order: the masses come in row order, and the outputs go there
        a, b = numpy.empty((n1, 3)), numpy.empty((n2, 3))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = force_core(a, b, numpy.asarray(boxsize, dtype='f8'), None if mass2 is None else mass2.numpy(), G,
                         r_split, rc2, eps2)
        acc.copy_(torch.from_numpy(got['acc']))
        if pot is not None:
            pot.copy_(torch.from_numpy(got['pot']))
        if neighbours is not None:
            neighbours.copy_(torch.from_numpy(got['neighbours']))


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(ShortRangeOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def fbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(ShortRangeOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def arr(x):
    return x if isinstance(x, numpy.ndarray) else cpu(x)


def check(got, ref, what='', rows=None):
    """(acc, pot, neighbours), pot and neighbours possibly None, against the restatement's dict (rows: of these rows of
    it)"""
    acc, pot, nb = got
    sel = slice(None) if rows is None else rows
    M = ref['neighbours'][sel].astype('f8')
    acc = arr(acc)
    assert acc.dtype == numpy.float64 and acc.shape == ref['acc'][sel].shape, (what, acc.shape)
    if nb is not None:
        nb = arr(nb)
        assert nb.dtype == numpy.int64 and numpy.array_equal(nb, ref['neighbours'][sel]), (what, nb[:8])
    d = numpy.abs(acc - ref['acc'][sel])
    bound = (M[:, None] + ULPS) * U * ref['Sacc'][sel]
    assert (d <= bound).all(), (what, float((d / numpy.maximum(bound, 1e-300)).max()))
    if pot is not None:
        pot = arr(pot)
        assert pot.dtype == numpy.float64 and pot.shape == M.shape
        d = numpy.abs(pot - ref['pot'][sel])
        bound = (M + ULPS) * U * ref['Spot'][sel]
        assert (d <= bound).all(), (what, float((d / numpy.maximum(bound, 1e-300)).max()))


# ---- the inputs ----------------------------------------------------------------------------------------------------

def wave_rc(n1, n2):
    return min(0.45, 0.6 * max(n1, n2, 1) ** (-1 / 3.))


def wave_case(n1, n2, dtype):
    return uniform(n1, 3, 300 + n1).astype(dtype), uniform(n2, 3, 500 + n2).astype(dtype), wave_rc(n1, n2)


def masses(n, seed, dtype='f8'):
    return numpy.random.RandomState(seed).uniform(0.5, 1.5, n).astype(dtype)


QUEUE_NS = [63, 64, 65, 128, 129]
QUEUE_RC = 0.05


def queue_rows(k):
    """one primary at the centre of the box, k sources inside r_cut = 0.05 of it and 300 - k between 1.2 and 1.9 r_cut
    (in its neighbouring cells, outside the cut), shuffled"""
    rng = numpy.random.RandomState(900 + k)
    v = rng.normal(size=(300, 3))
    v /= numpy.sqrt((v * v).sum(axis=1))[:, None]
    rad = numpy.concatenate([QUEUE_RC * rng.uniform(0.05, 0.95, k), QUEUE_RC * rng.uniform(1.2, 1.9, 300 - k)])
    return numpy.array([[0.5, 0.5, 0.5]]), (0.5 + v * rad[:, None])[rng.permutation(300)]


def random_cases():
    """name -> keyword arguments of ref_force: every random input of the tests below.  r_split = r_cut / 4.5 where the
    case names none."""
    cases = {}
    for dtype in ('f8', 'f4'):
        for n1 in WAVE_NS:
            for n2 in WAVE_NS:
                p1, p2, rc = wave_case(n1, n2, dtype)
                cases['wave-%d-%d-%s' % (n1, n2, dtype)] = dict(pos=p1, pos2=p2, box=UNIT, r_cut=rc)
            p1, p2, rc = wave_case(n1, n1, dtype)
            cases['wave-mass-%d-%s' % (n1, dtype)] = dict(pos=p1, pos2=p2, box=UNIT, r_cut=rc,
                                                          mass2=masses(n1, 70 + n1, dtype), softening=0.1 * rc)
            cases['wave-auto-%d-%s' % (n1, dtype)] = dict(pos=p1, box=UNIT, r_cut=rc)
            cases['wave-auto-mass-%d-%s' % (n1, dtype)] = dict(pos=p1, box=UNIT, r_cut=rc,
                                                               mass=masses(n1, 80 + n1, dtype), G=0.25 / numpy.pi)
    for k in QUEUE_NS:
        p1, p2 = queue_rows(k)
        cases['queue-%d' % k] = dict(pos=p1, pos2=p2, box=UNIT, r_cut=QUEUE_RC, mass2=masses(300, 90 + k))
    cases['crowded'] = dict(pos=crowded(), box=UNIT, r_cut=0.05, mass=masses(650, 60), softening=0.002)
    cases['faces'] = dict(pos=numpy.concatenate([face_pairs(SLAB, 0.05), uniform(300, 3, 61, SLAB)]), box=SLAB,
                          r_cut=0.05)
    cases['open'] = dict(pos=uniform(2000, 3, 12), box=UNIT, r_cut=0.05)
    cases['slab'] = dict(pos=uniform(900, 3, 46, SLAB), box=SLAB, r_cut=0.125, r_split=0.03, mass=masses(900, 9),
                         softening=0.004, G=2.5)
    cases['third-law'] = dict(pos=uniform(1500, 3, 31), box=UNIT, r_cut=0.12, mass=masses(1500, 5))
    cases['cross'] = dict(pos=uniform(700, 3, 32), pos2=uniform(500, 3, 33), box=UNIT, r_cut=0.15,
                          mass=masses(700, 6), mass2=masses(500, 7, 'f4'), softening=0.01)
    cases['ranks'] = dict(pos=uniform(900, 3, 44), pos2=uniform(700, 3, 45), box=UNIT, r_cut=0.1,
                          mass2=masses(700, 8))
    cases['ranks-auto'] = dict(pos=uniform(900, 3, 44), box=UNIT, r_cut=0.1, mass=masses(900, 10), softening=0.005)
    cases['ranks-slab'] = dict(pos=uniform(900, 3, 46, SLAB), box=SLAB, r_cut=0.125)
    for kw in cases.values():
        kw.setdefault('r_split', kw['r_cut'] / RCUT)
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_force(**RANDOM[name])
    return _REFERENCE[name]


def run(be, kw, form='C', potential=True, neighbours=True, **over):
    """short_range_force of the keyword arguments of ref_force on one rank: always the triple (acc, pot, neighbours)"""
    kw = dict(kw, **over)
    dev = be.device
    t = lambda x: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)
    p = lambda x: None if x is None else place(x, form, dev)
    out = short_range_force(mesh(kw['box']), p(kw['pos']), kw['r_split'], kw.get('r_cut'), mass=t(kw.get('mass')),
                            pos2=p(kw.get('pos2')), mass2=t(kw.get('mass2')), softening=kw.get('softening', 0.0),
                            G=kw.get('G', 1.0), potential=potential, neighbours=neighbours)
    out = list(out) if isinstance(out, tuple) else [out]
    return out[0], (out[1] if potential else None), (out[-1] if neighbours else None)


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_gives_plummer_where_the_split_is_far():
    """two rows with r_split = 1e6 r: fac is 1 to 1e-15, so acc = -G m dx / (r2 + eps2)^(3/2), with and without
    softening; and pot = -G m / sqrt(r2 + eps2) to the 1e-6 of erfc(5e-7)"""
    pos = numpy.array([[0.1, 0.2, 0.3], [0.13, 0.18, 0.34]])
    dx = pos[0] - pos[1]
    r2 = (dx * dx).sum()
    for eps in (0.0, 0.02):
        ref = ref_force(pos, UNIT, 1e6 * numpy.sqrt(r2), r_cut=0.4, mass=[3.0, 5.0], softening=eps, G=0.7)
        assert ref['neighbours'].tolist() == [1, 1]
        want = -0.7 * 5.0 * dx / (r2 + eps * eps) ** 1.5
        assert (numpy.abs(ref['acc'][0] - want) <= 4e-15 * numpy.abs(want)).all()
        want = 0.7 * 3.0 * dx / (r2 + eps * eps) ** 1.5
        assert (numpy.abs(ref['acc'][1] - want) <= 4e-15 * numpy.abs(want)).all()
        assert abs(ref['pot'][0] / (-0.7 * 5.0 / numpy.sqrt(r2 + eps * eps)) - 1) < 1e-6
    # across the face of the box: the minimum image
    far = numpy.array([[0.99, 0.5, 0.5], [0.02, 0.5, 0.5]])
    ref = ref_force(far, UNIT, 1e3, r_cut=0.4)
    assert abs(ref['acc'][0, 0] - 1 / 0.03 ** 2) < 1e-9 / 0.03 ** 2 and ref['acc'][0, 1] == 0


def test_restatement_on_the_lattice():
    """the full 8^3 lattice, unit masses, r_cut = 2.5 spacings: every row has exactly 80 neighbours (the lattice
    vectors with 0 < |n|^2 <= 6: 6 + 12 + 8 + 6 + 24 + 24; |n|^2 = 7 does not occur), and by symmetry no force: acc is
    0 within the bound, S_i from the restatement"""
    ref = ref_force(lattice(3), UNIT, 2.5 / 8 / RCUT, r_cut=2.5 / 8)
    assert (ref['neighbours'] == 80).all()
    assert (ref['Sacc'] > 100).all()
    assert (numpy.abs(ref['acc']) <= (80 + ULPS) * U * ref['Sacc']).all()
    assert (ref['pot'] < 0).all() and numpy.ptp(ref['pot']) <= (80 + ULPS) * U * ref['Spot'].max()


EWALD = [(0.03, 0.0, 0.0), (0.02, 0.025, 0.03), (0.01, -0.04, 0.02)]


def test_the_split_sums_to_newton():
    """the Ewald identity: for two unit masses in the unit box and r_split = 0.02 the short-range force of the rule
    plus the exact k-space sum of 4 pi G m / (V k^2) exp(-k^2 r_split^2) over |n_d| <= 64 is -G m r / r^3 (1 - 4 pi
    r^3 / (3 V)) within 5e-6 (what remains is the l = 4 term of the periodic images).  The long-range factor is what
    Transfer.long_range(d, r_split, 'spectral') gives on the k grid as a func(k, v): the sqrt(2) of the pairing between
    gauss_r and r_split is pinned here."""
    rs, G = 0.02, 1.0
    n = numpy.arange(-64, 65) * 2 * numpy.pi
    k = [n.reshape(-1, 1, 1), n.reshape(1, -1, 1), n.reshape(1, 1, -1)]
    one = numpy.ones((1, 1, 1))
    t = [Transfer.long_range(d, rs, grad_kind='spectral')(k, one) for d in range(3)]
    assert t[0].shape == (129, 129, 129) and Transfer.long_range(1, rs).gauss_r == numpy.sqrt(2.0) * rs
    assert Transfer.long_range(1, rs).grad_kind == 'finite4' and Transfer.long_range(1, rs).laplace_pow == -1
    for sep in EWALD:
        sep = numpy.asarray(sep)
        pos = numpy.array([0.4, 0.5, 0.6]) + numpy.array([sep, 0 * sep])
        short = ref_force(pos, UNIT, rs, G=G)
        assert short['neighbours'].tolist() == [1, 1]
        phase = numpy.exp(1j * (k[0] * sep[0] + k[1] * sep[1] + k[2] * sep[2]))
        mesh_part = numpy.array([4 * numpy.pi * G * (t[d] * phase).sum().real for d in range(3)])
        r = numpy.sqrt((sep * sep).sum())
        want = -G * sep / r ** 3 * (1 - 4 * numpy.pi * r ** 3 / 3)
        err = numpy.abs(short['acc'][0] + mesh_part - want).max() / numpy.sqrt((want * want).sum())
        print('separation %s: relative error %.2g' % (sep.tolist(), err))
        assert err < 5e-6, (sep, err)
        # and the short-range part alone is far from it: the check is not vacuous
        assert numpy.abs(short['acc'][0] - want).max() > 0.05 * numpy.abs(want).max()


@pytest.mark.parametrize('group', ['wave-f8', 'wave-f4', 'other'])
def test_inputs_are_decided(group):
    names = [n for n in sorted(RANDOM) if (n.startswith('wave') and n.endswith(group[-2:])) or
             (group == 'other' and not n.startswith('wave'))]
    assert len(names) >= 12
    for name in names:
        kw = RANDOM[name]
        ref = reference(name)
        assert ref['margin'] >= 1e-9, (name, ref['margin'])
        assert 2 * kw['r_cut'] <= min(kw['box']) and kw['r_cut'] <= RCUT * kw['r_split'] * (1 + 1e-12), name
        assert len(kw['pos']) <= 2500
        if not name.startswith('wave') and not name.startswith('queue'):
            assert (ref['neighbours'] > 0).sum() >= len(kw['pos']) // 2, name
    if group == 'other':
        for k in QUEUE_NS:
            assert reference('queue-%d' % k)['neighbours'].tolist() == [k]


# ---- 2. the cut and the zero -------------------------------------------------------------------------------------------

def test_the_cut_and_the_zero(fbe):
    """lattice rows with r_cut exactly a lattice distance: a pair at r2 == rc2 is out (26 = 6 + 12 + 8 neighbours at
    r_cut = 2 spacings, 80 at 2.5); coincident rows and the self pairs of the auto form contribute nothing, and
    neighbours excludes them; the cross form with a copy of the rows is the auto form"""
    pos = lattice(3)
    for rc, count in ((2 / 8., 26), (2.5 / 8, 80), (1 / 8., 0), (3 / 8., 92)):
        kw = dict(pos=pos, box=UNIT, r_cut=rc, r_split=rc / RCUT)
        ref = ref_force(**kw)
        assert (ref['neighbours'] == count).all()
        got = run(fbe, kw)
        check(got, ref, what=rc)
        if count == 0:
            assert not arr(got[0]).any() and not arr(got[1]).any()
    # seven rows twice, and a row at the corner given as 1 and as 0
    pos = numpy.concatenate([uniform(100, 3, 2), uniform(100, 3, 2)[:7], [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]])
    m = masses(109, 3)
    kw = dict(pos=pos, box=UNIT, r_cut=0.2, r_split=0.05, mass=m)
    ref = ref_force(**kw)
    assert ref['margin'] >= 1e-9
    auto = run(fbe, kw)
    check(auto, ref)
    cross = run(fbe, dict(kw, pos2=pos.copy(), mass2=m, mass=None))
    check(cross, ref)
    assert torch.equal(auto[2], cross[2])
    # a row and its twin see the same neighbours and not each other: the count of the row without the twins, plus
    # the twins of the others among them
    assert numpy.array_equal(ref['neighbours'][:7], ref['neighbours'][100:107])
    r2 = ((pos[:7, None, :] - pos[None, :100, :] - numpy.rint(pos[:7, None, :] - pos[None, :100, :])) ** 2).sum(axis=2)
    near = (r2 > 0) & (r2 < 0.04)
    assert numpy.array_equal(ref['neighbours'][:7], near.sum(axis=1) + near[:, :7].sum(axis=1))
    # a lone pair of coincident rows: no neighbour, no force
    got = run(fbe, dict(pos=numpy.array([[0.3, 0.3, 0.3], [0.3, 0.3, 0.3]]), box=UNIT, r_cut=0.2, r_split=0.05))
    assert arr(got[2]).tolist() == [0, 0] and not arr(got[0]).any() and not arr(got[1]).any()


# ---- 3. grid edge shapes -----------------------------------------------------------------------------------------------

def grid_of(ncell, box):
    return (list(ncell[:3]), [0.0] * 3, [ncell[d] / box[d] for d in range(3)], PERIODIC[3])


def run_local(be, kw, grid, pos=None, pos2=None):
    """local_force on a forced grid"""
    dev = be.device
    rc, eps = kw['r_cut'], kw.get('softening', 0.0)
    p1 = torch.from_numpy(kw['pos'] if pos is None else pos).to(dev)
    p2 = None if pos2 is None else torch.from_numpy(pos2).to(dev)
    return local_force(be, p1, p2, None, grid, kw['box'], kw.get('G', 1.0), kw['r_split'], rc * rc, eps * eps, True,
                       True)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(fbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes: no pair is visited twice, none is missed"""
    kw = RANDOM['faces']
    assert all(kw['box'][d] / grid[d] >= kw['r_cut'] for d in range(3))
    ref = reference('faces')
    assert (ref['neighbours'][:14] >= 1).all()
    check(run_local(fbe, kw, grid_of(grid, kw['box'])), ref, what=grid)
    if grid == GRIDS[0]:
        # and the grid the host layer lays through the cell cap: few rows and a large r_cut
        pos = face_pairs(SLAB, 0.05)
        assert cell_grid(len(pos), 0.05, SLAB)[0] == [6, 3, 1]
        small = dict(pos=pos, box=SLAB, r_cut=0.05, r_split=0.05 / RCUT)
        check(run(fbe, small), ref_force(**small))


def test_open_axes(fbe):
    """a grid that is open along two axes (a rank's block): the rows of the block against all rows, nothing wraps on
    the open axes, rows outside the extent sit in the end cells and are no neighbours of anything"""
    kw = RANDOM['open']
    pos, rc = kw['pos'], kw['r_cut']
    grid = cell_grid(len(pos), rc, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2 and grid[1][0] == 0.25 - rc
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    assert 100 < inside.sum() < 1000
    ref = ref_force(pos[inside], UNIT, kw['r_split'], r_cut=rc, pos2=pos)
    assert ref['margin'] >= 1e-9 and ref['neighbours'].sum() > 100
    check(run_local(fbe, kw, grid, pos=pos[inside], pos2=pos), ref)


# ---- 4. wave, queue and workgroup edges ----------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_wave_and_workgroup_edges(fbe, dtype, form):
    """n1 and n2 independently from 0, 1, 2, 63, 64, 65, 257 and 1025 uniform rows, float64 and float32, contiguous,
    strided and transposed rows, cross and auto, without and with masses (and a softening, and G = 1 / (4 pi))"""
    for n1 in WAVE_NS:
        for n2 in WAVE_NS:
            name = 'wave-%d-%d-%s' % (n1, n2, dtype)
            kw = RANDOM[name]
            t1 = place(kw['pos'], form, fbe.device)
            before = cpu(t1).copy()
            got = run(fbe, kw, form)
            check(got, reference(name), what=name)
            assert tuple(got[0].shape) == (n1, 3) and tuple(got[1].shape) == tuple(got[2].shape) == (n1,)
            assert numpy.array_equal(cpu(t1), before, equal_nan=True)
        for kind in ('wave-mass', 'wave-auto', 'wave-auto-mass'):
            name = '%s-%d-%s' % (kind, n1, dtype)
            check(run(fbe, RANDOM[name], form), reference(name), what=name)
        if form == 'C' and n1 in (0, 65):
            # numpy rows in, device tensors out
            name = 'wave-auto-mass-%d-%s' % (n1, dtype)
            kw = RANDOM[name]
            got = short_range_force(mesh(UNIT), kw['pos'], kw['r_split'], kw['r_cut'], mass=kw['mass'], G=kw['G'])
            assert isinstance(got, torch.Tensor) and got.device == fbe.device
            check((got, None, None), reference(name), what=name)


@pytest.mark.parametrize('k', QUEUE_NS)
def test_the_queue_at_its_capacity(fbe, k):
    """one primary with exactly 63, 64, 65, 128 and 129 neighbours among 300 sources of its neighbouring cells: the
    flush of the wave's queue at and around its 64 entries, with masses"""
    name = 'queue-%d' % k
    got = run(fbe, RANDOM[name])
    assert arr(got[2]).tolist() == [k]
    check(got, reference(name), what=name)
    # and without the masses
    kw = dict(RANDOM[name], mass2=None)
    check(run(fbe, kw), ref_force(**kw), what=name)


@pytest.mark.parametrize('name', ['crowded', 'slab', 'cross'])
def test_random_cases(fbe, name):
    """600 rows in one cell (every walk fills the queue many times); the box [1, 0.5, 0.25] at r_cut = L_z / 2 with
    r_split above r_cut / 4.5, masses, a softening and G; a cross case with float32 masses"""
    ref = reference(name)
    if name == 'crowded':
        assert ref['neighbours'].max() >= 599
    check(run(fbe, RANDOM[name]), ref, what=name)


# ---- 5. outputs optional -------------------------------------------------------------------------------------------------

def test_optional_outputs_do_not_change_acc(fbe):
    """pot and neighbours NULL or not, in every combination, on the same sorted inputs: the same acc bit for bit; two
    launches give identical neighbours (and pot)"""
    kw = RANDOM['third-law']
    dev = fbe.device
    pos = torch.from_numpy(kw['pos']).to(dev)
    m = torch.from_numpy(kw['mass']).to(dev)
    rc = kw['r_cut']
    grid = cell_grid(len(kw['pos']), rc, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(fbe, pos, grid, UNIT)
    results = []
    for want_pot, want_nb in ((True, True), (False, False), (True, False), (False, True), (True, True)):
        acc = torch.full((len(pos), 3), float('nan'), dtype=torch.float64, device=dev)
        pot = torch.full((len(pos),), float('nan'), dtype=torch.float64, device=dev) if want_pot else None
        nb = torch.full((len(pos),), -1, dtype=torch.int64, device=dev) if want_nb else None
        fbe.short_range(spos, order, cell_of, spos, order, cell_start, m, grid[0], grid[3], UNIT, 1.0, kw['r_split'],
                        rc * rc, 0.0, acc, pot, nb)
        results.append((acc, pot, nb))
        check((acc, pot, nb), reference('third-law'))
    for acc, pot, nb in results[1:]:
        assert torch.equal(acc, results[0][0])
    assert torch.equal(results[0][1], results[4][1]) and torch.equal(results[0][2], results[4][2])
    assert torch.equal(results[0][2], results[3][2]) and torch.equal(results[0][1], results[2][1])


# ---- 6. box and symmetry -------------------------------------------------------------------------------------------------

def test_newtons_third_law(fbe):
    """auto form with masses: sum_i m_i acc_i is zero within the sum of the rows' bounds (each times m_i), plus n
    2^-52 sum_i |m_i acc_i| for the sum formed here"""
    kw = RANDOM['third-law']
    ref = reference('third-law')
    acc = arr(run(fbe, kw)[0])
    m = kw['mass']
    total = (m[:, None] * acc).sum(axis=0)
    bound = (m[:, None] * (ref['neighbours'][:, None] + ULPS) * U * ref['Sacc']).sum(axis=0)
    bound += len(m) * U * numpy.abs(m[:, None] * acc).sum(axis=0)
    assert (numpy.abs(total) <= bound).all(), (total, bound)
    assert (numpy.abs(m[:, None] * acc).sum(axis=0) > 1e6 * bound).all()        # (not vacuous)


def test_cross_with_the_sets_swapped(fbe):
    """the cross form with the two sets swapped in role equals the restatement swapped likewise; mass is validated but
    does not enter a cross force"""
    kw = RANDOM['cross']
    swapped = dict(kw, pos=kw['pos2'], pos2=kw['pos'], mass=kw['mass2'], mass2=kw['mass'])
    ref = ref_force(**swapped)
    assert ref['margin'] >= 1e-9
    check(run(fbe, swapped), ref)
    a, b = run(fbe, kw), run(fbe, dict(kw, mass=None))
    assert torch.equal(a[2], b[2])
    check(b, reference('cross'))


# ---- 7. ranks ------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """short_range_force on thread ranks holding both sets split unevenly (one rank holds no rows): what every rank
    got, and its slice of the primaries"""
    kw = RANDOM[name]
    p1, p2, m1, m2 = kw['pos'], kw.get('pos2'), kw.get('mass'), kw.get('mass2')
    s1 = split(len(p1), size)
    s2 = split(len(p2), size)[::-1] if p2 is not None else None

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a = s1[comm.rank]
        c = s2[comm.rank] if p2 is not None else None
        acc, pot, nb = short_range_force(pm, p1[a], kw['r_split'], kw['r_cut'], mass=None if m1 is None else m1[a],
                                         pos2=None if p2 is None else p2[c], mass2=None if m2 is None else m2[c],
                                         softening=kw.get('softening', 0.0), G=kw.get('G', 1.0), potential=True,
                                         neighbours=True)
        return cpu(acc), cpu(pot), cpu(nb), a
    return thread_ranks(size, body)


def check_ranks(name, size, np_):
    results = ranks_case(name, size, np_)
    ref = reference(name)
    assert ref['margin'] >= 1e-9
    sizes = [len(results[r][0]) for r in range(size)]
    assert 0 in sizes and len(set(sizes)) > 1 and sum(sizes) == len(RANDOM[name]['pos'])
    for r in range(size):
        acc, pot, nb, rows = results[r]
        # in this rank's row order: its slice of the rows of all ranks
        check((acc, pot, nb), ref, what=(name, size, r), rows=rows)


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_force(obe, size, np_):
    """cross with masses, auto with masses and a softening, and r_cut = 1/8 on the box [1, 0.5, 0.25] (with np = [2, 2]
    the block plus 2 r_cut covers the box along y and z): neighbours of every rank's rows equal the restatement of all
    rows exactly, acc and pot within the bound, in the rank's own row order"""
    for name in ('ranks', 'ranks-auto', 'ranks-slab'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    for name in ('ranks', 'ranks-auto', 'ranks-slab'):
        check_ranks(name, size, np_)


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank: a wrong shape, a wrong type, a coordinate that is not finite,
    2 r_cut > L, masses of the wrong length"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        with pytest.raises(ValueError):
            short_range_force(pm, mine[:, :2] if comm.rank == 1 else mine, 0.02)
        with pytest.raises(TypeError):
            short_range_force(pm, (mine * 8).astype('i8') if comm.rank == 2 else mine, 0.02)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            short_range_force(pm, bad, 0.02)
        with pytest.raises(ValueError, match='r_cut'):
            short_range_force(pm, mine, 0.02, r_cut=0.6)
        with pytest.raises(ValueError):
            short_range_force(pm, mine, 0.02, mass=numpy.ones(29 if comm.rank == 1 else 30))
        nb = short_range_force(pm, mine, 0.02, neighbours=True)[1]
        want = ref_force(pos, UNIT, 0.02)['neighbours'][30 * comm.rank:30 * comm.rank + 30]
        assert numpy.array_equal(cpu(nb), want)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 8. bad arguments ----------------------------------------------------------------------------------------------------

def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    with pytest.raises(NotImplementedError):
        short_range_force(mesh(UNIT[:2]), pos[:, :2], 0.02)
    for rs in (0.0, -0.01, numpy.nan, numpy.inf, 'wide'):
        with pytest.raises(ValueError, match='r_split'):
            short_range_force(pm, pos, rs)
    for rc in (0.0, -0.1, numpy.nan, numpy.inf, 0.51):
        with pytest.raises(ValueError, match='r_cut'):
            short_range_force(pm, pos, 0.02, r_cut=rc)
    with pytest.raises(ValueError, match='r_cut'):
        short_range_force(pm, pos, 0.12)                         # the default 4.5 r_split > L / 2
    with pytest.raises(ValueError, match='r_cut'):
        short_range_force(mesh(SLAB), pos, 0.02, r_cut=0.13)     # 2 r_cut > the shortest side
    assert tuple(short_range_force(mesh(SLAB), pos, 0.03, r_cut=0.125).shape) == (50, 3)
    for eps in (-1e-3, numpy.nan, numpy.inf):
        with pytest.raises(ValueError, match='softening'):
            short_range_force(pm, pos, 0.02, softening=eps)
    with pytest.raises(ValueError, match='G'):
        short_range_force(pm, pos, 0.02, G=numpy.inf)
    with pytest.raises(ValueError, match='mass2'):
        short_range_force(pm, pos, 0.02, mass2=numpy.ones(50))
    with pytest.raises(ValueError, match='shape'):
        short_range_force(pm, pos[:, :2], 0.02)
    with pytest.raises(ValueError, match='shape'):
        short_range_force(pm, pos, 0.02, pos2=pos.reshape(-1))
    with pytest.raises(TypeError):
        short_range_force(pm, (pos * 100).astype('i8'), 0.02)
    with pytest.raises(ValueError, match='mass'):
        short_range_force(pm, pos, 0.02, mass=numpy.ones(49))
    with pytest.raises(ValueError, match='mass2'):
        short_range_force(pm, pos, 0.02, pos2=pos[:40], mass2=numpy.ones(50))
    with pytest.raises(TypeError):
        short_range_force(pm, pos, 0.02, mass=numpy.ones(50, dtype='i4'))
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows'):
        short_range_force(pm, bad, 0.02)
    with pytest.raises(ValueError, match='3 rows'):
        short_range_force(pm, bad, 0.02, pos2=bad[5:8])
    # empty sets are legal
    acc, pot, nb = short_range_force(pm, numpy.zeros((0, 3)), 0.02, potential=True, neighbours=True)
    assert tuple(acc.shape) == (0, 3) and tuple(pot.shape) == (0,) and nb.dtype == torch.int64
    acc, nb = short_range_force(pm, pos, 0.02, pos2=numpy.zeros((0, 3)), neighbours=True)
    assert tuple(acc.shape) == (50, 3) and not cpu(acc).any() and not cpu(nb).any()
    # the forms of the result
    assert isinstance(short_range_force(pm, pos, 0.02), torch.Tensor)
    assert len(short_range_force(pm, pos, 0.02, potential=True)) == 2


@pytest.mark.gpu
def test_no_sources_on_the_device(hipbe):
    """no source at all: the outputs are overwritten with zeros, not left as they were"""
    pos = uniform(70, 3, 1)
    acc, pot, nb = short_range_force(mesh(UNIT), pos, 0.02, pos2=numpy.zeros((0, 3)), potential=True, neighbours=True)
    assert not cpu(acc).any() and not cpu(pot).any() and not cpu(nb).any()


# ---- 9. the ABI and the resources ----------------------------------------------------------------------------------------

def test_the_entry_is_bound():
    assert 'short_range' in _abi.DEVICE_ONLY
    lib = backend.load_library()
    assert hasattr(lib, 'pmx_short_range')
    import pmesh_amd
    assert 'short_range_force' in pmesh_amd.__doc__
    from tests.test_abi import declared_symbols, generator, header_text
    assert 'pmx_short_range' in declared_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pyx, abi, fnptrs = generator().generate(header_text())
    assert open(os.path.join(root, 'pmesh_amd', '_pmx.pyx')).read() == pyx
    assert open(os.path.join(root, 'pmesh_amd', '_abi_gen.py')).read() == abi
    assert open(os.path.join(root, 'pmesh_amd', 'csrc', 'pmx_fnptrs.h')).read() == fnptrs
    assert 'pmx_short_range' in pyx and "'short_range'" in abi


def test_short_range_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_shortrange.hip')
    # short_kernel<MASS>: without and with masses; and no others
    assert sorted(t) == ['_ZN3pmx12short_kernelILb0EEEvNS_5SArgsE', '_ZN3pmx12short_kernelILb1EEEvNS_5SArgsE'], sorted(t)
    for name, r in t.items():
        mass = 'Lb1E' in name
        assert r['ScratchSize'] == 0, (name, r)
        # a ring of 128 entries per wave, four waves: 3 x 8 bytes per entry, and 4 for the slot with masses
        assert r['LDS'] == 4 * 128 * (28 if mass else 24), (name, r)
        # measured at compile time: 126 without masses (four waves per SIMD), 134 with (three); the device's double
        # erfc holds about 40 of them
        assert r['VGPRs'] <= (136 if mass else 128), (name, r)
        assert r['Occupancy'] >= (3 if mass else 4), (name, r)
