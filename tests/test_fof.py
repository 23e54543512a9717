"""pmesh_amd.fof (csrc/pmx_fof.hip) against a numpy restatement of its rule.

The restatement is brute force: the wrapped rows, the full matrix of minimum-image squared distances accumulated in
the order d = 0, 1, 2, the friendship matrix d^2 <= b^2, and minimum-label propagation over it to a fixed point.  All
comparisons of minid, labels, length, cell_start and roots are exact integer equality.  Under -m "not gpu" the
restatement serves the six entries of csrc/pmx_fof.hip (FofOracleBackend), so the host layer — the grid, the numbering
of the groups, the merge loop over thread ranks, the catalogue — runs without a GPU; under -m gpu the kernels are
compared with it.

The condition on random inputs: the restatement finds no pair with |d^2 - b^2| < 1e-9 b^2 (a contracted multiply-add
could otherwise flip a friendship).  test_kernel_inputs_are_decided asserts it without a GPU for every random case;
the seeds were picked so that it holds.  The lattice cases are dyadic: their differences and squares are exact, and
pairs at exactly b test the <= itself.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import backend
from pmesh_amd.fof import FOFCatalog, FOFResult, cell_grid, cell_sort, fof, fof_catalog, local_groups
from pmesh_amd.mock import lognormal_catalog
from pmesh_amd.pm import ParticleMesh
from pmesh_amd.transfer import Tabulated
from tests.test_lpt import cpu, table
from tests.test_mock import MockOracleBackend

PERIODIC = {1: 1, 2: 3, 3: 7}


# ---- the restatement -----------------------------------------------------------------------------------------------

def wrap(x, box):
    x = numpy.asarray(x).astype('f8')
    box = numpy.asarray(box, dtype='f8')
    with numpy.errstate(invalid='ignore'):
        w = x - box * numpy.floor(x / box)
        w = numpy.where(w < 0, w + box, w)
        return numpy.where(w < box, w, 0.0)


def dist2(w, box):
    """the (n, n) minimum-image squared distances of wrapped rows, accumulated in the order of the axes"""
    r2 = numpy.zeros((len(w), len(w)))
    for d in range(w.shape[1]):
        dx = w[:, None, d] - w[None, :, d]
        dx = dx - box[d] * numpy.rint(dx / box[d])
        r2 = r2 + dx * dx
    return r2


def components(adj):
    """minimum-label propagation over the friendship matrix to a fixed point: the smallest row index of the component
    of every row.  Between the sweeps every row takes the label of the row its label names (a row of the same
    component), which shortens long chains; the fixed point is the same."""
    n = len(adj)
    label = numpy.arange(n)
    while True:
        new = numpy.minimum(numpy.where(adj, label[None, :], n).min(axis=1), label)
        while True:
            jumped = new[new]
            if (jumped == new).all():
                break
            new = jumped
        if (new == label).all():
            return label.astype('i8')
        label = new


def ref_groups(pos, b, box, gid=None):
    """(minid of every row, the smallest |d^2 - b^2| / b^2 over the pairs); gid: global indices other than 0 .. n - 1"""
    w = wrap(pos, box)
    n = len(w)
    if n == 0:
        return numpy.zeros(0, dtype='i8'), numpy.inf
    r2 = dist2(w, numpy.asarray(box, dtype='f8'))
    off = r2[~numpy.eye(n, dtype=bool)]
    margin = float(numpy.abs(off - b * b).min() / (b * b)) if off.size else numpy.inf
    root = components(r2 <= b * b)
    if gid is None:
        return root, margin
    best = numpy.full(n, numpy.iinfo('i8').max)
    numpy.minimum.at(best, root, numpy.asarray(gid, dtype='i8'))
    return best[root], margin


def ref_labels(minid, nmin):
    """(labels, ngroups, length): groups of at least nmin rows by length descending, ties by ascending minid"""
    minid = numpy.asarray(minid)
    groups = {}
    for m in minid.tolist():
        groups[m] = groups.get(m, 0) + 1
    kept = sorted([(-c, m) for m, c in groups.items() if c >= nmin])
    number = {m: k + 1 for k, (_, m) in enumerate(kept)}
    labels = numpy.array([number.get(m, 0) for m in minid.tolist()], dtype='i8')
    length = numpy.array([0] + [-c for c, _ in kept], dtype='i8')
    length[0] = len(minid) - length[1:].sum()
    return labels, len(kept), length


def ref_catalog(pos, box, minid, labels, ngroups, mass=None, vel=None):
    w = wrap(pos, box)
    box = numpy.asarray(box, dtype='f8')
    n, nd = w.shape
    mass = numpy.ones(n) if mass is None else numpy.asarray(mass).astype('f8').reshape(-1)
    vel = numpy.zeros((n, nd)) if vel is None else numpy.asarray(vel).astype('f8')
    M, cm, cv = numpy.zeros(ngroups + 1), numpy.zeros((ngroups + 1, nd)), numpy.zeros((ngroups + 1, nd))
    for g in range(1, ngroups + 1):
        rows = numpy.flatnonzero(labels == g)
        ref = w[minid[rows[0]]]
        dx = w[rows] - ref
        dx = dx - box * numpy.rint(dx / box)
        M[g] = mass[rows].sum()
        cm[g] = wrap(ref + (mass[rows, None] * dx).sum(axis=0) / M[g], box)
        cv[g] = (mass[rows, None] * vel[rows]).sum(axis=0) / M[g]
    return M, cm, cv


def ref_cells(w, grid, box):
    """the flat cell of wrapped rows on a grid of pmesh_amd.fof.cell_grid"""
    ncell, origin, inv_side, mask = grid
    flat = numpy.zeros(len(w), dtype='i8')
    for d in range(w.shape[1]):
        r = w[:, d] - origin[d]
        r = numpy.where(r < 0, r + box[d], r)
        last = ncell[d] - 1
        t = r * inv_side[d]
        c = numpy.where(t >= last, last, numpy.where(t >= 0, t, 0).astype('i8'))
        if not (mask >> d) & 1:
            extent = ncell[d] / inv_side[d]
            c = numpy.where(r >= extent, numpy.where(box[d] - r < r - extent, 0, last), c)
        flat = flat * ncell[d] + c
    return flat


class FofOracleBackend(MockOracleBackend):
    """the CPU test double with the six entries of csrc/pmx_fof.hip served by the restatement"""
    name = 'oracle-fof'

    def fof_cells(self, pos, boxsize, origin, inv_side, ncell, periodic, wpos, cell_of, counts, flagged):
        if pos.shape[0] == 0:
            return
        x = pos.numpy().astype('f8')
        w = wrap(x, boxsize)
        c = ref_cells(w, (ncell, origin, inv_side, periodic), boxsize)
        wpos.copy_(torch.from_numpy(w))
        cell_of.copy_(torch.from_numpy(c.astype('i4')))
        counts += torch.from_numpy(numpy.bincount(c, minlength=counts.numel()).astype('i4'))
        flagged += int((~numpy.isfinite(x)).any(axis=1).sum())

    def fof_fill(self, wpos, cell_of, cell_start, cursor, order, spos):
        if wpos.shape[0] == 0:
            return
        c = cell_of.numpy()
        count = numpy.bincount(c, minlength=cursor.numel())
        assert numpy.array_equal(cell_start.numpy(), numpy.concatenate([[0], numpy.cumsum(count)]))
        assert not cursor.numpy().any()
        o = numpy.argsort(c, kind='stable')
        order.copy_(torch.from_numpy(o.astype('i4')))
        spos.copy_(wpos[torch.from_numpy(o)])
        cursor.copy_(torch.from_numpy(count.astype('i4')))

    def fof_link(self, spos, order, cell_of, cell_start, ncell, periodic, boxsize, b2, parent):
        n = spos.shape[0]
        if n == 0:
            return
        w = numpy.empty((n, spos.shape[1]))
        w[order.numpy()] = spos.numpy()
        adj = dist2(w, numpy.asarray(boxsize, dtype='f8')) <= b2
        parent.copy_(torch.from_numpy(components(adj).astype('i4')))

    def fof_flatten(self, parent):
        p = parent.numpy()
        assert (p[p] == p).all()

    def fof_minlabel(self, root, val, work, changed):
        if val.numel() == 0:
            return
        r, v = root.numpy().astype('i8'), val.numpy()
        best = v.copy()
        numpy.minimum.at(best, r, v)
        new = best[r]
        changed += int((new != v).sum())
        val.copy_(torch.from_numpy(new))

    def fof_group_sums(self, pos, labels, mass, vel, ref, boxsize, out):
        if pos.shape[0] == 0 or out.shape[0] <= 1:
            return
        nd = ref.shape[1]
        box = numpy.asarray(boxsize, dtype='f8')[:nd]
        lab = labels.numpy()
        m = numpy.ones(len(lab)) if mass is None else mass.numpy().astype('f8').reshape(-1)
        dx = wrap(pos.numpy(), box) - wrap(ref.numpy(), box)[lab]
        dx = dx - box * numpy.rint(dx / box)
        cols = [m] + [m * dx[:, d] for d in range(nd)]
        cols += [m * (vel.numpy()[:, d].astype('f8') if vel is not None else 0.0) for d in range(nd)]
        o = out.numpy()
        keep = lab > 0
        for c, col in enumerate(cols):
            numpy.add.at(o[:, c], lab[keep], numpy.broadcast_to(col, lab.shape)[keep])


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(FofOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def fbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(FofOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- the inputs ----------------------------------------------------------------------------------------------------

UNIT = [1.0, 1.0, 1.0]
SLAB = [1.0, 0.5, 0.25]


def lattice(nd):
    axes = numpy.meshgrid(*[numpy.arange(8) / 8.0] * nd, indexing='ij')
    return numpy.stack([a.reshape(-1) for a in axes], axis=1)


def chain(n, b, start, step_dir, order='row'):
    """n rows spaced 0.9 b from `start` along `step_dir`, wrapped by the rule"""
    u = numpy.asarray(step_dir, dtype='f8')
    u = u / numpy.sqrt((u * u).sum())
    pos = numpy.asarray(start, dtype='f8') + 0.9 * b * numpy.arange(n)[:, None] * u
    if order == 'reversed':
        pos = pos[::-1].copy()
    elif order == 'shuffled':
        pos = pos[numpy.random.RandomState(5).permutation(n)]
    return pos


CHAIN_B = 0.003


def two_chains():
    """two chains 1.5 b apart, their rows interleaved"""
    a = chain(150, CHAIN_B, [0.8, 0.3, 0.4], [1, 0, 0])
    pos = numpy.empty((300, 3))
    pos[0::2] = a
    pos[1::2] = a + [0, 1.5 * CHAIN_B, 0]
    return pos


def crowded():
    """600 rows inside a ball of radius b / 2 around the centre and 50 isolated rows, b = 0.05"""
    rng = numpy.random.RandomState(8)
    v = rng.normal(size=(600, 3))
    v *= (0.025 * rng.uniform(size=600) ** (1 / 3.) / numpy.sqrt((v * v).sum(axis=1)))[:, None]
    k = numpy.stack(numpy.unravel_index(rng.permutation(64)[:50], (4, 4, 4)), axis=1)
    lone = 0.1 + 0.25 * k + rng.uniform(-0.02, 0.02, size=(50, 3))
    pos = numpy.concatenate([0.5 + v, lone])
    return pos[rng.permutation(650)]


def face_pairs(box, b):
    """a pair straddling every face, edge and corner of the box, 0.6 b apart, the pairs more than b from each other:
    the pairs that cross the x face sit at the middle of the axes they do not cross, the others at x = 1/4, 1/2, 3/4"""
    box = numpy.asarray(box)
    nd = len(box)
    rows, free = [], 0
    for m in range(1, 2 ** nd):
        axes = [d for d in range(nd) if (m >> d) & 1]
        h = 0.3 * b / numpy.sqrt(len(axes))
        lo = box / 2.0
        if 0 not in axes:
            free += 1
            lo[0] = 0.25 * free * box[0]
        hi = lo.copy()
        for d in axes:
            lo[d], hi[d] = box[d] - h, h
        rows += [lo, hi]
    return numpy.array(rows)


def clusters(sizes, b, box, seed, corner_first=True):
    """tight clusters (all rows within 0.4 b of their centre) far apart, the first around the corner of the box; rows
    shuffled"""
    rng = numpy.random.RandomState(seed)
    box = numpy.asarray(box, dtype='f8')
    nd = len(box)
    rows = []
    side = int(numpy.ceil(len(sizes) ** (1.0 / nd)))
    assert (box / side > 4 * b).all()
    for k, s in enumerate(sizes):
        centre = (numpy.array(numpy.unravel_index(k, (side,) * nd)) + (0.0 if k == 0 and corner_first else 0.5)) * box / side
        rows.append(centre + rng.uniform(-0.4 * b / numpy.sqrt(nd), 0.4 * b / numpy.sqrt(nd), size=(s, nd)))
    pos = numpy.concatenate(rows)
    return pos[rng.permutation(len(pos))]


_LOGNORMAL = {}


def lognormal_rows():
    """the rows of a small lognormal catalogue (Nmesh = 16^3, about 2000 rows), made once by the rule of
    pmesh_amd.mock under the CPU test double: a clustered input"""
    if 'pos' not in _LOGNORMAL:
        previous = backend._current
        backend.use(MockOracleBackend())
        try:
            pm = ParticleMesh([16, 16, 16], BoxSize=200.)
            k, p = table()
            tab = Tabulated(k, numpy.sqrt(300 * p / numpy.prod(pm.BoxSize)), loglog=True)
            cat = lognormal_catalog(pm, tab, 2000.0 / 200. ** 3, 77, bias=2.0)
            _LOGNORMAL['pos'] = cpu(cat.pos).copy()
        finally:
            backend.use(previous)
    return _LOGNORMAL['pos']


def uniform(n, nd, seed, box=None):
    box = numpy.ones(nd) if box is None else numpy.asarray(box)
    return numpy.random.RandomState(seed).uniform(size=(n, nd)) * box


WAVE_NS = [0, 1, 2, 63, 64, 65, 257, 1025]


def all_cases():
    """name -> (rows, box, b, random): every input of the kernel tests"""
    cases = {}
    for nd in (3, 2, 1):
        cases['lattice%dd-linked' % nd] = (lattice(nd), UNIT[:nd], 1 / 8., False)
        cases['lattice%dd-apart' % nd] = (lattice(nd), UNIT[:nd], 1 / 8. - 2.0 ** -30, False)
    for order in ('row', 'reversed', 'shuffled'):
        cases['chain-' + order] = (chain(300, CHAIN_B, [0.5, 0.3, 0.4], [1, 0, 0], order), UNIT, CHAIN_B, True)
    cases['two-chains'] = (two_chains(), UNIT, CHAIN_B, True)
    cases['crowded'] = (crowded(), UNIT, 0.05, True)
    cases['faces'] = (face_pairs(SLAB, 0.05), SLAB, 0.05, True)
    cases['faces-2d'] = (face_pairs(SLAB[:2], 0.05), SLAB[:2], 0.05, True)
    cases['faces-1d'] = (face_pairs(SLAB[:1], 0.05), SLAB[:1], 0.05, True)
    for n in WAVE_NS:
        b = 0.2 * max(n, 1) ** (-1 / 3.)
        for dtype in ('f8', 'f4'):
            cases['wave%d-%s' % (n, dtype)] = (uniform(n, 3, 100 + n).astype(dtype), UNIT, b, True)
    cases['random-0.2'] = (uniform(2000, 3, 11), UNIT, 0.2 * 2000 ** (-1 / 3.), True)
    cases['random-0.28'] = (uniform(2000, 3, 12), UNIT, 0.28 * 2000 ** (-1 / 3.), True)
    cases['random-2d'] = (uniform(1500, 2, 13, SLAB[:2]), SLAB[:2], 0.28 * (0.5 / 1500) ** 0.5, True)
    cases['random-1d'] = (uniform(700, 1, 14), UNIT[:1], 0.6 / 700, True)
    cases['lognormal'] = (lognormal_rows, [200.] * 3, 0.2 * 200. / 2000 ** (1 / 3.), True)
    return cases


CASES = all_cases()
_REFERENCE = {}


def case(name):
    pos, box, b, random = CASES[name]
    if callable(pos):
        pos = pos()
    return pos, box, b, random


def reference(name):
    """the restatement's (minid, margin) of a case, computed once"""
    if name not in _REFERENCE:
        pos, box, b, _ = case(name)
        _REFERENCE[name] = ref_groups(pos, b, box)
    return _REFERENCE[name]


def mesh(box, comm=None, np_=None):
    kw = {} if comm is None else dict(comm=comm, np=np_)
    return ParticleMesh([8] * len(box), BoxSize=list(box), **kw)


def place(pos, form, dev):
    """the rows as a device tensor: contiguous ('C'), every other row and column of a larger array ('strided'), or the
    transposed storage ('T')"""
    t = torch.from_numpy(numpy.ascontiguousarray(pos)).to(dev)
    n, nd = pos.shape
    if form == 'strided':
        big = torch.full((2 * n + 1, 2 * nd), float('nan'), dtype=t.dtype, device=dev)
        view = big[1::2, ::2]
    elif form == 'T':
        view = torch.full((nd, n), float('nan'), dtype=t.dtype, device=dev).t()
    else:
        return t
    view.copy_(t)
    return view


ROW_FORMS = ['C', 'strided', 'T']


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_inputs_are_decided(name):
    """no pair of a random case has |d^2 - b^2| < 1e-9 b^2; and the cases hold what they are for"""
    pos, box, b, random = case(name)
    minid, margin = reference(name)
    print('%s: %d rows, %d groups, margin %.3g' % (name, len(pos), len(set(minid.tolist())), margin))
    assert 2 * b <= min(box)
    if random:
        assert margin >= 1e-9
    groups = numpy.unique(minid, return_counts=True)[1] if len(pos) else numpy.zeros(0)
    if name.endswith('-linked'):
        assert margin == 0 and (minid == 0).all()              # one group, through pairs at exactly b
    if name.endswith('-apart'):
        assert numpy.array_equal(minid, numpy.arange(len(pos)))
    if name.startswith('chain-'):
        assert (minid == 0).all() and wrap(pos, box)[:, 0].min() < 0.1 < 0.9 < wrap(pos, box)[:, 0].max()
    if name == 'two-chains':
        assert sorted(groups) == [150, 150]
    if name == 'crowded':
        assert sorted(groups) == [1] * 50 + [600]
    if name.startswith('faces'):
        assert (groups == 2).all() and len(groups) == 2 ** len(box) - 1
    if name.startswith('random') or name == 'lognormal':
        assert groups.max() >= 3 and (groups == 1).any() and len(pos) <= 2500
    if name == 'lognormal':
        assert len(pos) > 1000


def test_restatement_on_a_known_answer():
    """five rows on a line of the unit box: 0.95 and 0.02 are friends through the boundary at b = 0.08, 0.5 is alone"""
    pos = numpy.array([[0.95], [0.5], [0.02], [0.09], [0.41]])
    minid, margin = ref_groups(pos, 0.08, [1.0])
    assert minid.tolist() == [0, 1, 0, 0, 4] and margin > 1e-3
    assert ref_groups(pos, 0.095, [1.0])[0].tolist() == [0, 1, 0, 0, 1]
    labels, ngroups, length = ref_labels([0, 1, 0, 0, 4, 5, 5, 5], 2)
    assert labels.tolist() == [1, 0, 1, 1, 0, 2, 2, 2] and ngroups == 2 and length.tolist() == [2, 3, 3]
    # global indices other than the row numbers
    assert ref_groups(pos, 0.08, [1.0], gid=[9, 3, 7, 8, 1])[0].tolist() == [7, 3, 7, 7, 1]


def test_cell_grid():
    """cells of side >= b, at most two per row (and one); open axes only where the block plus 2 b leaves a gap"""
    for n, b, box in ((512, 1 / 8., UNIT), (2000, 0.016, UNIT), (14, 0.1, SLAB), (3, 0.125, SLAB), (1, 0.01, UNIT),
                      (0, 0.01, UNIT), (100000, 1e-4, SLAB[:2]), (5, 0.1, UNIT[:1])):
        ncell, origin, inv_side, mask = cell_grid(n, b, box)
        assert mask == PERIODIC[len(box)] and origin == [0.0] * len(box)
        assert numpy.prod(ncell) <= max(1, 2 * n)
        for d in range(len(box)):
            assert ncell[d] >= 1 and box[d] / ncell[d] >= b and inv_side[d] == ncell[d] / box[d]
    assert cell_grid(512, 1 / 8., UNIT)[0] == [8, 8, 8]
    ncell, origin, inv_side, mask = cell_grid(100, 0.05, UNIT, lo=[0.5, 0.0, 0.0], hi=[1.0, 1.0, 0.95])
    assert mask == 6 and origin == [0.45, 0.0, 0.0] and abs(ncell[0] / inv_side[0] - 0.6) < 1e-15
    assert 0.6 / ncell[0] >= 0.05
    assert cell_grid(100, 0.05, UNIT, lo=[0.0] * 3, hi=[0.5] * 3)[1] == [0.95] * 3


# ---- 2. the passes one by one ------------------------------------------------------------------------------------------

GRIDS = [[1, 1, 1], [2, 2, 2], [3, 3, 3], [3, 2, 1], [1, 2, 3], [2, 1, 2], [9, 4, 2]]


def run_passes(be, pos, b, box, grid, form='C'):
    """(cell_of, cell_start, order, spos, wpos, root, flagged) of the passes on a given grid, as numpy arrays"""
    t = place(pos, form, be.device)
    wpos, cell_of, cell_start, order, spos, flagged = cell_sort(be, t, grid, box)
    root, _ = local_groups(be, t, b, box, grid)
    return cpu(cell_of), cpu(cell_start), cpu(order), cpu(spos), cpu(wpos), cpu(root), int(cpu(flagged)[0])


def check_passes(be, name, grid, form='C'):
    pos, box, b, _ = case(name)
    minid, _ = reference(name)
    nd = len(box)
    if isinstance(grid[0], int):
        assert all(box[d] / grid[d] >= b for d in range(nd))
        grid = (grid[:nd], [0.0] * nd, [grid[d] / box[d] for d in range(nd)], PERIODIC[nd])
    cell_of, cell_start, order, spos, wpos, root, flagged = run_passes(be, pos, b, box, grid, form)
    w = wrap(pos, box)
    want = ref_cells(w, grid, box)
    ncells = int(numpy.prod(grid[0]))
    assert flagged == 0
    assert numpy.array_equal(wpos, w)
    assert numpy.array_equal(cell_of, want)
    assert numpy.array_equal(cell_start, numpy.concatenate([[0], numpy.cumsum(numpy.bincount(want, minlength=ncells))]))
    # the rows in cell order: every row once, the cells ascending, the wrapped rows with them (the order inside a cell
    # is free)
    assert numpy.array_equal(numpy.sort(order), numpy.arange(len(pos)))
    assert (numpy.diff(want[order]) >= 0).all() and numpy.array_equal(spos, w[order])
    # the root of a row is the smallest local index of its component: on one rank its minid
    assert numpy.array_equal(root, minid), (name, grid[0], numpy.flatnonzero(root != minid)[:10])


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(fbe, grid):
    """pairs straddling every face and corner of the box [1, 0.5, 0.25] on grids of 1, 2 and 3 cells along periodic
    axes (in 3-d, 2-d and 1-d): every pair found, none twice over (the groups are the pairs), nothing else linked"""
    for name in ('faces', 'faces-2d', 'faces-1d'):
        check_passes(fbe, name, grid)
    # and through the cell cap: few rows and a large b
    pos, box, b, _ = case('faces')
    assert cell_grid(len(pos), b, box)[0] == [6, 3, 1] and cell_grid(3, 0.125, SLAB)[0] == [3, 1, 1]
    assert cell_grid(4, 0.1, SLAB)[0] == [4, 2, 1]
    check_passes(fbe, 'faces', cell_grid(len(pos), b, box))


@pytest.mark.parametrize('name', ['lattice3d-linked', 'lattice3d-apart', 'lattice2d-linked', 'lattice2d-apart',
                                  'lattice1d-linked', 'lattice1d-apart', 'chain-row', 'chain-reversed',
                                  'chain-shuffled', 'two-chains', 'crowded', 'random-0.2', 'random-0.28', 'random-2d',
                                  'random-1d', 'lognormal'])
def test_passes_on_cases(fbe, name):
    """cell_of, cell_start, order and the roots of every case on the grid the host layer lays, and on a coarser one"""
    pos, box, b, _ = case(name)
    check_passes(fbe, name, cell_grid(len(pos), b, box))
    check_passes(fbe, name, [2] * len(box))


def test_open_axes(fbe):
    """a grid that is open along two axes: rows outside the extent go to the nearer end cell, nothing wraps there, and
    the rows inside are grouped as on the periodic grid"""
    pos, box, b, _ = case('random-0.28')
    grid = cell_grid(len(pos), b, box, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2 and grid[1][0] == 0.25 - b
    cell_of, cell_start, order, spos, wpos, root, flagged = run_passes(fbe, pos, b, box, grid)
    want = ref_cells(wpos, grid, box)
    assert numpy.array_equal(cell_of, want) and cell_start[-1] == len(pos)
    inside = ((wpos[:, 0] >= 0.25) & (wpos[:, 0] < 0.75) & (wpos[:, 2] >= 0.5) & (wpos[:, 2] < 0.75))
    # components of the rows within b of the block, as far as the pairs with a row inside go: those pairs are all found
    r2 = dist2(wpos, numpy.asarray(box))
    pairs = numpy.argwhere((r2 <= b * b) & inside[:, None])
    assert len(pairs) > inside.sum()
    assert (root[pairs[:, 0]] == root[pairs[:, 1]]).all()
    # and nothing is linked that the rule does not link
    minid, _ = reference('random-0.28')
    assert (minid[root] == minid).all()


@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_wave_and_workgroup_edges(fbe, dtype, form):
    """n = 0, 1, 2, 63, 64, 65, 257 and 1025 uniform rows at b = 0.2 n^(-1/3), float64 and float32, contiguous,
    strided and transposed rows: minid and labels of fof()"""
    pm = mesh(UNIT)
    for n in WAVE_NS:
        name = 'wave%d-%s' % (n, dtype)
        pos, box, b, _ = case(name)
        minid, _ = reference(name)
        t = place(pos, form, fbe.device)
        before = cpu(t).copy()
        res = fof(pm, t, b, nmin=2)
        assert numpy.array_equal(cpu(t), before)
        assert res.minid.dtype == torch.int64 and res.labels.dtype == torch.int64 and res.iterations == 0
        assert numpy.array_equal(cpu(res.minid), minid), name
        labels, ngroups, length = ref_labels(minid, 2)
        assert numpy.array_equal(cpu(res.labels), labels) and res.ngroups == ngroups
        assert numpy.array_equal(cpu(res.length), length) and res.csize == n
        # the same rows as a numpy array
        if form == 'C' and n in (0, 65):
            assert numpy.array_equal(cpu(fof(pm, pos, b, nmin=2).minid), minid)


def test_minlabel(fbe):
    """the minimum of an int64 value over every component, the number of rows that changed; a second call changes
    nothing"""
    rng = numpy.random.RandomState(3)
    for n in (1, 64, 1000, 4097):
        root = numpy.minimum(rng.randint(0, n, size=n), numpy.arange(n))
        root = root[root][root[root]]
        for _ in range(20):
            root = root[root]
        val = rng.randint(-2 ** 62, 2 ** 62, size=n)
        best = numpy.full(n, numpy.iinfo('i8').max)
        numpy.minimum.at(best, root, val)
        want = best[root]
        dev = fbe.device
        r = torch.from_numpy(root.astype('i4')).to(dev)
        v = torch.from_numpy(val.copy()).to(dev)
        work = torch.empty_like(v)
        changed = torch.full((1,), 5, dtype=torch.int64, device=dev)
        fbe.fof_minlabel(r, v, work, changed)
        assert numpy.array_equal(cpu(v), want) and int(cpu(changed)[0]) == 5 + int((want != val).sum())
        fbe.fof_minlabel(r, v, work, changed)
        assert numpy.array_equal(cpu(v), want) and int(cpu(changed)[0]) == 5 + int((want != val).sum())


# ---- 3. fof() ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['lattice3d-linked', 'lattice3d-apart', 'lattice2d-linked', 'lattice2d-apart',
                                  'lattice1d-linked', 'lattice1d-apart', 'chain-row', 'chain-reversed',
                                  'chain-shuffled', 'two-chains', 'crowded', 'faces', 'faces-2d', 'faces-1d',
                                  'random-0.2', 'random-0.28', 'random-2d', 'random-1d', 'lognormal'])
def test_fof_on_cases(fbe, name):
    pos, box, b, _ = case(name)
    minid, _ = reference(name)
    res = fof(mesh(box), torch.from_numpy(pos).to(fbe.device), b, nmin=3)
    assert isinstance(res, FOFResult) and res.linking_length == b and res.offset == 0
    assert numpy.array_equal(cpu(res.minid), minid)
    labels, ngroups, length = ref_labels(minid, 3)
    assert numpy.array_equal(cpu(res.labels), labels) and res.ngroups == ngroups
    assert numpy.array_equal(cpu(res.length), length) and int(cpu(res.length).sum()) == res.csize == len(pos)
    if name == 'lattice3d-linked':
        assert res.ngroups == 1 and cpu(res.length).tolist() == [0, 512]
    if name == 'lattice3d-apart':
        assert res.ngroups == 0 and cpu(res.length).tolist() == [512]


@pytest.mark.parametrize('name', ['chain-shuffled', 'crowded'])
def test_two_launches_give_identical_arrays(fbe, name):
    pos, box, b, _ = case(name)
    grid = cell_grid(len(pos), b, box)
    a = run_passes(fbe, pos, b, box, grid)
    c = run_passes(fbe, pos, b, box, grid)
    for k in (0, 1, 4, 5, 6):                                   # (order and spos are free inside a cell)
        assert numpy.array_equal(a[k], c[k])
    t = torch.from_numpy(pos).to(fbe.device)
    r1, r2 = fof(mesh(box), t, b, nmin=2), fof(mesh(box), t, b, nmin=2)
    assert torch.equal(r1.minid, r2.minid) and torch.equal(r1.labels, r2.labels) and torch.equal(r1.length, r2.length)


LABEL_SIZES = [5, 7, 5, 4, 3, 5, 1, 1, 4, 3]
LABEL_B = 0.04


def label_rows():
    return clusters(LABEL_SIZES, LABEL_B, UNIT, 21)


def test_labels(fbe):
    """groups of equal length (the tie goes to the smaller minid), a group of exactly nmin rows and one of nmin - 1,
    length[0] plus the rest = csize, and absolute=False"""
    pos = label_rows()
    minid, margin = ref_groups(pos, LABEL_B, UNIT)
    assert margin >= 1e-9 and sorted(numpy.unique(minid, return_counts=True)[1]) == sorted(LABEL_SIZES)
    pm = mesh(UNIT)
    t = torch.from_numpy(pos).to(fbe.device)
    res = fof(pm, t, LABEL_B, nmin=4)
    labels, ngroups, length = ref_labels(minid, 4)
    assert ngroups == 6 and length.tolist() == [8, 7, 5, 5, 5, 4, 4]
    assert res.ngroups == 6 and numpy.array_equal(cpu(res.length), length)
    assert numpy.array_equal(cpu(res.labels), labels) and numpy.array_equal(cpu(res.minid), minid)
    got = cpu(res.labels)
    firsts = [minid[got == g][0] for g in range(1, 7)]
    assert firsts[1] < firsts[2] < firsts[3] and firsts[4] < firsts[5]       # the ties, by ascending minid
    assert int(cpu(res.length).sum()) == res.csize == len(pos)
    # the default nmin = 20: nothing is labelled
    res20 = fof(pm, t, LABEL_B)
    assert res20.ngroups == 0 and cpu(res20.length).tolist() == [len(pos)] and not cpu(res20.labels).any()
    # in units of the mean separation
    rel = fof(pm, t, LABEL_B / (1.0 / len(pos)) ** (1 / 3.), nmin=4, absolute=False)
    assert abs(rel.linking_length - LABEL_B) <= 1e-15
    assert numpy.array_equal(cpu(rel.minid), minid) and numpy.array_equal(cpu(rel.labels), labels)


def check_catalog(cat, pos, box, minid, labels, ngroups, length, mass, vel):
    assert isinstance(cat, FOFCatalog)
    M, cm, cv = ref_catalog(pos, box, minid, labels, ngroups, mass, vel)
    nd = len(box)
    assert tuple(cat.CMPosition.shape) == (ngroups + 1, nd) == tuple(cat.CMVelocity.shape)
    assert cat.Mass.dtype == cat.CMPosition.dtype == cat.CMVelocity.dtype == torch.float64
    assert cat.Length.dtype == torch.int64 and numpy.array_equal(cpu(cat.Length), length)
    dm = numpy.abs(cpu(cat.Mass) - M)
    dv = numpy.abs(cpu(cat.CMVelocity) - cv)
    dx = numpy.abs(cpu(cat.CMPosition) - cm)
    print('catalogue: mass %.3g velocity %.3g position %.3g' % (dm.max(), dv.max(), dx.max()))
    assert (dm <= 1e-12 * numpy.abs(M)).all()
    assert (dv <= 1e-12 * numpy.abs(cv)).all()
    assert (dx <= 1e-12 * max(box)).all()
    return cm


@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_catalog(fbe, dtype):
    """Length exact, Mass and CMVelocity within 1e-12 relative, CMPosition within 1e-12 max(L) of the restatement:
    double sums of at most 2500 terms of order one, in any order.  The first group straddles the corner of the box:
    its centre lies within b of the corner, not in the middle of the box."""
    pos = label_rows().astype(dtype)
    rng = numpy.random.RandomState(4)
    mass = rng.uniform(0.5, 1.5, size=len(pos)).astype(dtype)
    vel = rng.uniform(0.5, 1.5, size=pos.shape).astype(dtype)
    minid, _ = ref_groups(pos, LABEL_B, UNIT)
    labels, ngroups, length = ref_labels(minid, 4)
    pm = mesh(UNIT)
    dev = fbe.device
    t = torch.from_numpy(pos).to(dev)
    res = fof(pm, t, LABEL_B, nmin=4)
    assert numpy.array_equal(cpu(res.labels), labels)
    cat = fof_catalog(pm, t, res, mass=torch.from_numpy(mass).to(dev), vel=place(vel, 'strided', dev))
    cm = check_catalog(cat, pos, UNIT, minid, labels, ngroups, length, mass, vel)
    w = wrap(pos, UNIT)
    corner = [g for g in range(1, ngroups + 1) if numpy.ptp(w[labels == g], axis=0).min() > 0.5]
    assert len(corner) == 1
    c = cm[corner[0]]
    assert (numpy.minimum(c, 1 - c) <= LABEL_B).all()
    got = cpu(cat.CMPosition)[corner[0]]
    assert (numpy.minimum(got, 1 - got) <= LABEL_B).all()
    # unit masses, no velocities; numpy rows
    plain = fof_catalog(pm, pos, res)
    check_catalog(plain, pos, UNIT, minid, labels, ngroups, length, None, None)
    assert not cpu(plain.CMVelocity).any() and numpy.array_equal(cpu(plain.Mass), length * (numpy.arange(ngroups + 1) > 0))


def test_catalog_of_random_rows(fbe):
    """2000 uniform rows at 0.28 mean separations, 2-d rows in a box of unequal sides, and the clustered case"""
    for name in ('random-0.28', 'random-2d', 'lognormal'):
        pos, box, b, _ = case(name)
        minid, _ = reference(name)
        labels, ngroups, length = ref_labels(minid, 3)
        rng = numpy.random.RandomState(6)
        mass, vel = rng.uniform(0.5, 1.5, size=len(pos)), rng.uniform(0.5, 1.5, size=pos.shape)
        pm = mesh(box)
        res = fof(pm, pos, b, nmin=3)
        check_catalog(fof_catalog(pm, pos, res, mass=mass, vel=vel), pos, box, minid, labels, ngroups, length, mass, vel)


def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    for b in (0.0, -0.1, numpy.nan, numpy.inf, 0.51):
        with pytest.raises(ValueError, match='linking length'):
            fof(pm, pos, b)
    with pytest.raises(ValueError, match='linking length'):
        fof(mesh(SLAB), pos, 0.13)                             # 2 b > the shortest side
    assert fof(mesh(SLAB), pos, 0.125).csize == 50
    with pytest.raises(ValueError, match='shape'):
        fof(pm, pos[:, :2], 0.1)
    with pytest.raises(ValueError, match='shape'):
        fof(pm, pos.reshape(-1), 0.1)
    with pytest.raises(TypeError):
        fof(pm, (pos * 100).astype('i8'), 0.1)
    with pytest.raises(ValueError, match='nmin'):
        fof(pm, pos, 0.1, nmin=0)
    with pytest.raises(ValueError, match='nmin'):
        fof(pm, pos, 0.1, nmin=2.5)
    with pytest.raises(NotImplementedError):
        fof(ParticleMesh([4, 4, 4, 4], BoxSize=1.), numpy.zeros((3, 4)), 0.1)
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows'):
        fof(pm, bad, 0.1)
    res = fof(pm, pos, 0.1, nmin=2)
    with pytest.raises(TypeError, match='FOFResult'):
        fof_catalog(pm, pos, cpu(res.labels))
    with pytest.raises(ValueError, match='rows'):
        fof_catalog(pm, pos[:40], res)
    with pytest.raises(ValueError, match='mass'):
        fof_catalog(pm, pos, res, mass=numpy.ones((50, 2)))
    with pytest.raises(ValueError, match='vel'):
        fof_catalog(pm, pos, res, vel=numpy.ones((50, 2)))
    with pytest.raises(TypeError):
        fof_catalog(pm, pos, res, mass=numpy.ones(50, dtype='i4'))
    # no rows at all
    empty = fof(pm, numpy.zeros((0, 3)), 0.1)
    assert empty.ngroups == 0 and cpu(empty.length).tolist() == [0] and tuple(empty.minid.shape) == (0,)
    cat = fof_catalog(pm, numpy.zeros((0, 3)), empty)
    assert tuple(cat.CMPosition.shape) == (1, 3)


# ---- 4. ranks ----------------------------------------------------------------------------------------------------------

RANKS = [(2, [2]), (3, [3]), (4, [2, 2])]
SPLITS = {2: [1.0, 0.0], 3: [0.7, 0.0, 0.3], 4: [0.5, 0.2, 0.0, 0.3]}


def u_chain():
    """300 rows spaced 0.9 b along three sides of a square of side 0.4 that crosses the periodic boundary of both
    axes: with the box cut in two along x, in three along x, or in four along x and y, the chain passes through every
    rank's block and comes back to the first; rows in chain order, so that minid = 0 has to travel block by block"""
    b = 0.4 / 90
    k = numpy.arange(100) * 0.9 * b
    z = numpy.full(100, 0.4)
    a = numpy.stack([0.7 + k, numpy.full(100, 0.65), z], axis=1)
    c = numpy.stack([numpy.full(100, a[-1, 0] + 0.9 * b), 0.65 + k, z], axis=1)
    e = numpy.stack([c[-1, 0] - k, numpy.full(100, c[-1, 1] + 0.9 * b), z], axis=1)
    return numpy.concatenate([a, c, e]), b


def split(n, size):
    cuts = numpy.rint(numpy.cumsum([0.0] + SPLITS[size]) * n).astype('i8')
    return [slice(int(cuts[r]), int(cuts[r + 1])) for r in range(size)]


def thread_ranks(size, body):
    from tests import thread_comm
    results = {}

    def run(comm):
        results[comm.rank] = body(comm)
    thread_comm.run_ranks(size, run)
    assert len(results) == size
    return results


def ranks_case(pos, box, b, nmin, mass, vel, size, np_):
    """fof and fof_catalog on thread ranks holding the rows split unevenly: what every rank got"""
    parts = split(len(pos), size)

    def body(comm):
        pm = mesh(box, comm, np_)
        dev = backend.get().device
        sl = parts[comm.rank]
        t = torch.from_numpy(pos[sl]).to(dev)
        res = fof(pm, t, b, nmin=nmin)
        cat = fof_catalog(pm, t, res, mass=None if mass is None else mass[sl], vel=None if vel is None else vel[sl])
        assert res.offset == sl.start and res.csize == len(pos)
        return (cpu(res.minid), cpu(res.labels), res.ngroups, cpu(res.length), res.iterations, cpu(cat.Mass),
                cpu(cat.CMPosition), cpu(cat.CMVelocity), cpu(cat.Length))
    return thread_ranks(size, body)


def check_ranks(size, np_, name=None, rows=None, nmin=3):
    pos, box, b = rows if rows is not None else case(name)[:3]
    minid, margin = ref_groups(pos, b, box) if rows is not None else reference(name)
    assert margin >= 1e-9 or not (rows is not None or CASES[name][3])
    rng = numpy.random.RandomState(9)
    mass, vel = rng.uniform(0.5, 1.5, size=len(pos)), rng.uniform(0.5, 1.5, size=pos.shape)
    results = ranks_case(pos, box, b, nmin, mass, vel, size, np_)
    sizes = [len(results[r][0]) for r in range(size)]
    assert 0 in sizes and len(set(sizes)) > 1
    labels, ngroups, length = ref_labels(minid, nmin)
    assert numpy.array_equal(numpy.concatenate([results[r][0] for r in range(size)]), minid)
    assert numpy.array_equal(numpy.concatenate([results[r][1] for r in range(size)]), labels)
    M, cm, cv = ref_catalog(pos, box, minid, labels, ngroups, mass, vel)
    for r in range(size):
        got = results[r]
        assert got[2] == ngroups and numpy.array_equal(got[3], length) and numpy.array_equal(got[8], length)
        assert got[4] == results[0][4] >= 1
        assert (numpy.abs(got[5] - M) <= 1e-12 * numpy.abs(M)).all()
        assert (numpy.abs(got[7] - cv) <= 1e-12 * numpy.abs(cv)).all()
        assert (numpy.abs(got[6] - cm) <= 1e-12 * max(box)).all()
        for k in (5, 6, 7):
            assert numpy.array_equal(got[k], results[0][k])     # identical on every rank
    return results[0][4]


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_groups(obe, size, np_):
    """minid, labels and the catalogue of thread ranks equal the restatement of all rows (= the one-rank results, by
    test_fof_on_cases) after undoing the split; one rank holds no rows"""
    for name in ('random-0.28', 'lognormal', 'lattice3d-linked', 'faces'):
        check_ranks(size, np_, name)


@pytest.mark.parametrize('size,np_', RANKS)
def test_chain_through_every_rank(obe, size, np_):
    """the periodic chain through every rank's block: one group with minid 0, after several merge rounds that end"""
    pos, b = u_chain()
    iterations = check_ranks(size, np_, rows=(pos, UNIT, b), nmin=20)
    print('%d ranks: %d merge rounds' % (size, iterations))
    assert 2 <= iterations <= 300
    assert (ref_groups(pos, b, UNIT)[0] == 0).all()
    # every rank owns a part of it
    pm = mesh(UNIT)
    cells = numpy.floor(wrap(pos, UNIT) * 8).astype('i8')
    for d, n in enumerate(np_):
        edges = pm.domain.edges[d] if len(np_) == 1 and size == pm.comm.size else None
        assert len(numpy.unique(cells[:, d] * n // 8)) == n, edges


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    check_ranks(size, np_, 'random-0.28')
    pos, b = u_chain()
    assert check_ranks(size, np_, rows=(pos, UNIT, b), nmin=20) >= 2


def test_ranks_raise_together(obe):
    """bad rows on one rank raise on every rank: a wrong shape (ValueError), a wrong type (TypeError), a coordinate
    that is not finite"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        with pytest.raises(ValueError):
            fof(pm, mine[:, :2] if comm.rank == 1 else mine, 0.05)
        with pytest.raises(TypeError):
            fof(pm, (mine * 8).astype('i8') if comm.rank == 2 else mine, 0.05)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            fof(pm, bad, 0.05)
        with pytest.raises(ValueError, match='linking length'):
            fof(pm, mine, 0.6)
        res = fof(pm, mine, 0.05, nmin=2)
        with pytest.raises(ValueError):
            fof_catalog(pm, mine, res, mass=numpy.ones(29 if comm.rank == 1 else 30))
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


def gather_min_case(size, np_):
    """Layout.gather(mode='min') against mode=numpy.minimum on random int64 data, with ghosts"""
    def body(comm):
        pm = mesh(UNIT, comm, np_)
        dev = backend.get().device
        pos = torch.from_numpy(uniform(400, 3, 30 + comm.rank)).to(dev)
        layout = pm.decompose(pos, smoothing=1.5)
        assert layout.recvlength > 0 and int(layout.sendcounts.sum()) > len(pos)
        rng = numpy.random.RandomState(40 + comm.rank)
        for shape in ((layout.recvlength,), (layout.recvlength, 2)):
            data = torch.from_numpy(rng.randint(-2 ** 62, 2 ** 62, size=shape)).to(dev)
            got = layout.gather(data, mode='min')
            want = layout.gather(data, mode=numpy.minimum)
            assert got.dtype == torch.int64 and tuple(got.shape) == (len(pos),) + shape[1:]
            assert torch.equal(got, want)
        fl = torch.from_numpy(rng.normal(size=layout.recvlength)).to(dev)
        assert torch.equal(layout.gather(fl, mode='min'), layout.gather(fl, mode=numpy.minimum))
        return True
    thread_ranks(size, body)


@pytest.mark.parametrize('size,np_', RANKS)
def test_gather_min(fbe, size, np_):
    gather_min_case(size, np_)


# ---- 5. resources (compiles for gfx950 on the CPU) ------------------------------------------------------------------

def test_fof_kernels_compile_without_scratch():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_fof.hip')
    # cells_kernel / sums_kernel<NDIM, PE> for 1 to 3 dimensions and f4 / f8 rows, fill_kernel / link_kernel<NDIM>
    counts = {'cells_kernel': 6, 'fill_kernel': 3, 'init_kernel': 1, 'link_kernel': 3, 'flatten_kernel': 1,
              'min_kernel': 1, 'gather_kernel': 1, 'sums_kernel': 6}
    for key, n in counts.items():
        assert len([k for k in t if key in k]) == n, sorted(t)
    assert len(t) == sum(counts.values()), sorted(t)
    for name, r in t.items():
        assert r['ScratchSize'] == 0 and r['LDS'] == 0, (name, r)
        # measured at compile time: link_kernel<3> 46, sums_kernel<3> 32, cells_kernel<3> 22, the others below 20 —
        # eight waves per SIMD for all of them
        assert r['VGPRs'] <= (48 if 'link_kernel' in name else 32), (name, r)
        assert r['Occupancy'] == 8, (name, r)
