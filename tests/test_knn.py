"""pmesh_amd.knn (csrc/pmx_knn.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/knn.py, include/pmesh_amd.h).  Rows are (n, ndim), wrapped into [0, L_d) by FoF's rule; dx_d = x_i,d
- x_j,d is the minimum image of the wrapped rows; all arithmetic is double, every operation rounded once; r2 = sum_d
dx_d^2 accumulated in the order d = 0, 1, 2.  Source j is a candidate of primary i when r2 < rmax2 = rmax * rmax.
dist2[i, :] are the k smallest candidate r2 ascending, +inf where there are fewer; index[i, c] names a source with that
r2 (-1 where inf), distinct within a row, unspecified among ties; found[i] counts the finite columns.  The auto form is
the cross form of the rows against themselves without the row's own index.

The restatement is brute force: the full (n1, n2) matrices of r2 and numpy.sort.  Under -m "not gpu" it serves pmx_knn
(KnnOracleBackend), so the host layer and the thread ranks run without a GPU; under -m gpu the kernel is compared with
it.

dist2, count and found are compared by exact equality of the float64 values (inf equals inf): the k smallest values
of a multiset depend on no order.  index is compared as a witness: r2 recomputed by the rule for (i, index[i, c]) is
exactly dist2[i, c]; the indices of a row are distinct; -1 stands exactly where dist2 is inf; the auto form never names
the row itself.  No tolerance appears in the kernel tests.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd import knn as knn_module
from pmesh_amd.fof import cell_grid
from pmesh_amd.knn import KNNResult, ball_volume, first_radius, knn, knn_cdf, knn_density, local_knn
from tests.test_fof import (GRIDS, PERIODIC, RANKS, ROW_FORMS, SLAB, UNIT, WAVE_NS, FofOracleBackend, crowded,
                            face_pairs, lattice, mesh, place, split, thread_ranks, uniform, wrap)
from tests.test_lpt import cpu

INF = numpy.inf
KS = [1, 2, 31, 32, 33, 63, 64]


# ---- the restatement -----------------------------------------------------------------------------------------------

def r2_matrix(w1, w2, box):
    """the (n1, n2) squared minimum-image distances of wrapped rows, accumulated in the order of the axes"""
    r2 = numpy.zeros((len(w1), len(w2)))
    for d in range(w1.shape[1]):
        x = w1[:, None, d] - w2[None, :, d]
        dx = x - box[d] * numpy.rint(x / box[d])
        r2 = r2 + dx * dx
    return r2


def knn_core(w1, w2, box, r2max, k, exclude_diagonal=False):
    """(dist2 (n1, k), index (n1, k), count (n1,)) of the wrapped rows w1 among the wrapped rows w2"""
    r2 = r2_matrix(w1, w2, numpy.asarray(box, dtype='f8'))
    cand = r2 < r2max
    if exclude_diagonal:
        cand[numpy.arange(len(w1)), numpy.arange(len(w1))] = False
    v = numpy.concatenate([numpy.where(cand, r2, INF), numpy.full((len(w1), k), INF)], axis=1)
    d = numpy.sort(v, axis=1)[:, :k]
    idx = numpy.argsort(v, axis=1, kind='stable')[:, :k]
    return d, numpy.where(numpy.isfinite(d), idx, -1), cand.sum(axis=1).astype('i8')


def ref_knn(pos, box, k, pos2=None, rmax=None):
    """the restatement of knn(mesh(box), pos, k, pos2, rmax): a dict of dist2, index, found and r2 (the matrix)"""
    box = numpy.asarray(box, dtype='f8')
    rm = box.min() / 2 if rmax is None else float(rmax)
    a = wrap(pos, box)
    b = a if pos2 is None else wrap(pos2, box)
    d, idx, _ = knn_core(a, b, box, rm * rm, k, exclude_diagonal=pos2 is None)
    return dict(dist2=d, index=idx, found=numpy.isfinite(d).sum(axis=1), r2=r2_matrix(a, b, box))


class KnnOracleBackend(FofOracleBackend):
    """the CPU test double with pmx_knn served by the restatement"""
    name = 'oracle-knn'

    def knn(self, spos1, order1, cell_of1, spos2, order2, cell_start2, ncell, periodic, boxsize, r2max, k, dist2,
            index=None, count=None):
        n1, n2, nd = spos1.shape[0], spos2.shape[0], spos1.shape[1]
        if n1 == 0:
            return
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell)) and 1 <= k <= 64
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        d, idx, cnt = knn_core(a, b, boxsize[:nd], r2max, k)
        dist2.copy_(torch.from_numpy(d))
        if index is not None:
            index.copy_(torch.from_numpy(idx.astype('i4')))
        if count is not None:
            count.copy_(torch.from_numpy(cnt))


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(KnnOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def fbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(KnnOracleBackend())
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


def check_witness(d, idx, r2, what='', me=None):
    """index against dist2 and the matrix r2 of the rule (me: the global indices of the rows, which must not appear)"""
    assert idx.shape == d.shape and idx.dtype in (numpy.int64, numpy.int32), (what, idx.dtype)
    assert numpy.array_equal(idx == -1, numpy.isinf(d)), what
    assert (idx >= -1).all() and (idx < max(r2.shape[1], 1)).all(), what
    rows = numpy.broadcast_to(numpy.arange(len(d))[:, None], d.shape)
    named = idx >= 0
    assert numpy.array_equal(r2[rows[named], idx[named]], d[named]), what
    s = numpy.sort(numpy.where(named, idx, -1 - numpy.arange(d.shape[1])[None, :]), axis=1)
    assert (numpy.diff(s, axis=1) != 0).all(), what
    if me is not None:
        assert not (idx == numpy.asarray(me)[:, None]).any(), what


def check_values(d, want, what=''):
    d = arr(d)
    assert d.dtype == numpy.float64 and d.shape == want.shape, (what, d.shape, want.shape)
    assert numpy.array_equal(d, want), (what, numpy.argwhere(d != want)[:4])


def run_local(be, p1, p2, grid, box, radius, k, form='C', what=''):
    """local_knn at the radius on the grid against the restatement: (dist2, index, count) as numpy arrays"""
    dev = be.device
    t1 = place(p1, form, dev)
    t2 = None if p2 is None else place(p2, form, dev)
    d, idx, cnt = local_knn(be, t1, t2, grid, box, radius * radius, k)
    a = wrap(p1, box)
    b = a if p2 is None else wrap(p2, box)
    wd, _, wcnt = knn_core(a, b, box, radius * radius, k)
    assert tuple(d.shape) == (len(p1), k) and idx.dtype == torch.int32 and cnt.dtype == torch.int64
    check_values(d, wd, what)
    assert numpy.array_equal(arr(cnt), wcnt), what
    check_witness(arr(d), arr(idx), r2_matrix(a, b, numpy.asarray(box, dtype='f8')), what)
    return arr(d), arr(idx), arr(cnt)


def run_sorted(be, primary, sources, radius, k, index=True):
    """pmx_knn itself on one periodic cell of the unit box with the sources in the order given (cell_sort keeps no order
    within a cell): (dist2, index, count) of the one primary"""
    dev = be.device
    n2 = len(sources)
    t = lambda x, dt: torch.from_numpy(numpy.ascontiguousarray(x, dtype=dt)).to(dev)
    d = torch.full((1, k), float('nan'), dtype=torch.float64, device=dev)
    idx = torch.full((1, k), -7, dtype=torch.int32, device=dev) if index else None
    cnt = torch.full((1,), -7, dtype=torch.int64, device=dev)
    be.knn(t(primary.reshape(1, 3), 'f8'), t([0], 'i4'), t([0], 'i4'), t(sources.reshape(n2, 3), 'f8'),
           t(numpy.arange(n2), 'i4'), t([0, n2], 'i4'), [1, 1, 1], PERIODIC[3], UNIT, radius * radius, k, d, idx, cnt)
    return arr(d), (arr(idx) if index else None), arr(cnt)


# ---- the inputs ----------------------------------------------------------------------------------------------------

RING_R = 0.05
RING_NS = [63, 64, 65, 127, 128, 129, 257]


def ring_rows(m, descending, extra=40):
    """one primary at the centre of the box, m sources inside the radius 0.05 of it at distinct distances, ascending or
    descending in the order given, and `extra` sources between 1.2 and 1.9 radii mixed in between"""
    rng = numpy.random.RandomState(700 + m)
    v = rng.normal(size=(m + extra, 3))
    v /= numpy.sqrt((v * v).sum(axis=1))[:, None]
    rad = RING_R * numpy.linspace(0.05, 0.95, m)
    if descending:
        rad = rad[::-1]
    out = RING_R * rng.uniform(1.2, 1.9, extra)
    where = numpy.sort(rng.permutation(m + extra)[:extra])
    radii = numpy.empty(m + extra)
    mask = numpy.zeros(m + extra, dtype=bool)
    mask[where] = True
    radii[mask] = out
    radii[~mask] = rad
    return numpy.array([0.5, 0.5, 0.5]), 0.5 + v * radii[:, None]


def void_rows():
    """a tight cluster of 800 rows (inside a ball of radius 0.01) and three isolated rows: 0.15 and 0.3 from the
    cluster, and one farther than rmax = 1/2 from everything"""
    rng = numpy.random.RandomState(21)
    v = rng.normal(size=(800, 3))
    v *= (0.01 * rng.uniform(size=800) ** (1 / 3.) / numpy.sqrt((v * v).sum(axis=1)))[:, None]
    lone = numpy.array([[0.25, 0.40, 0.25], [0.55, 0.25, 0.25], [0.75, 0.75, 0.75]])
    return numpy.concatenate([0.25 + v, lone])


VOID_K = 2
_REFERENCE = {}


def reference(name, make):
    """a restatement computed once and shared"""
    if name not in _REFERENCE:
        _REFERENCE[name] = make()
    return _REFERENCE[name]


def run_knn(be, pos, box, k, pos2=None, rmax=None, index=True, form='C'):
    dev = be.device
    res = knn(mesh(box), place(pos, form, dev), k, pos2=None if pos2 is None else place(pos2, form, dev), rmax=rmax,
              index=index)
    assert isinstance(res, KNNResult) and res.k == k and res.dist2.device == dev
    return res


def check_result(res, ref, what='', offset=0, rows=None, index=True):
    """a KNNResult against the dict of ref_knn (rows: this slice of its rows; offset: the global index of row 0 in the
    auto form, None in the cross form)"""
    sel = slice(None) if rows is None else rows
    check_values(res.dist2, ref['dist2'][sel], what)
    assert res.found.dtype == torch.int64 and numpy.array_equal(arr(res.found), ref['found'][sel]), what
    if index:
        n = len(ref['dist2'][sel])
        me = None if offset is None else numpy.arange(offset, offset + n)
        assert res.index.dtype == torch.int64
        check_witness(arr(res.dist2), arr(res.index), ref['r2'][sel], what, me)
    else:
        assert res.index is None


# ---- 1. the restatement (no GPU) -----------------------------------------------------------------------------------------

def test_restatement_on_the_lattice():
    """the 8^3 lattice: every row has 6 neighbours at 1/64, 12 at 2/64, 8 at 3/64 exactly; a radius of exactly one
    spacing leaves no candidate but the row itself"""
    ref = ref_knn(lattice(3), UNIT, 27)
    want = numpy.array([1.0] * 6 + [2.0] * 12 + [3.0] * 8 + [4.0]) / 64
    assert numpy.array_equal(ref['dist2'], numpy.broadcast_to(want, (512, 27)))
    assert (ref['found'] == 27).all()
    ref = ref_knn(lattice(3), UNIT, 3, rmax=1 / 8.)
    assert numpy.isinf(ref['dist2']).all() and (ref['index'] == -1).all() and not ref['found'].any()
    # across the face of the box, and the padding
    ref = ref_knn(numpy.array([[0.99, 0.5, 0.5]]), UNIT, 2, pos2=numpy.array([[0.02, 0.5, 0.5], [0.5, 0.5, 0.5]]),
                  rmax=0.1)
    assert abs(ref['dist2'][0, 0] - 0.03 ** 2) < 1e-15 and numpy.isinf(ref['dist2'][0, 1])
    assert ref['index'].tolist() == [[0, -1]] and ref['found'].tolist() == [1]


def test_first_radius():
    """the ball of R_0 holds 2 (k + 1) sources at the mean density, in every dimension"""
    for box in (UNIT, SLAB, UNIT[:2], SLAB[:2], UNIT[:1], [0.25]):
        for n, k in ((1000, 8), (50, 1), (10 ** 6, 32)):
            r = first_radius(n, k, box)
            assert abs(ball_volume(r, len(box)) * n / numpy.prod(box) / (2 * (k + 1)) - 1) < 1e-12
    assert first_radius(0, 3, UNIT) == INF


# ---- 2. grid edge shapes -----------------------------------------------------------------------------------------------

def grid_of(ncell, box):
    nd = len(box)
    return (list(ncell[:nd]), [0.0] * nd, [ncell[d] / box[d] for d in range(nd)], PERIODIC[nd])


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(fbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes: no source is named twice, none is missed (index is distinct, count exact)"""
    pos = numpy.concatenate([face_pairs(SLAB, 0.05), uniform(300, 3, 61, SLAB)])
    assert all(SLAB[d] / grid[d] >= 0.05 for d in range(3))
    d, _, cnt = run_local(fbe, pos, None, grid_of(grid, SLAB), SLAB, 0.05, 6, what=grid)
    assert (cnt[:14] >= 2).all() and (d[:14, 1] < 0.05 ** 2).all()          # the partner across the face
    run_local(fbe, pos[:100], pos, grid_of(grid, SLAB), SLAB, 0.05, 3, what=grid)


def test_open_axes(fbe):
    """a grid that is open along two axes (a rank's block): the rows of the block against all rows, nothing wraps on
    the open axes, rows outside the extent sit in the end cells and are no neighbours of anything"""
    pos, radius = uniform(2000, 3, 12), 0.05
    grid = cell_grid(len(pos), radius, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2 and grid[1][0] == 0.25 - radius
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    assert 100 < inside.sum() < 1000
    _, _, cnt = run_local(fbe, pos[inside], pos, grid, UNIT, radius, 4)
    assert cnt.sum() > 300


# ---- 3. dimensions, boxes, row forms -----------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_dimensions_boxes_and_row_forms(fbe, dtype, form):
    """ndim 1, 2 and 3, the unit box and [1, 0.5, 0.25], float64 and float32 rows, contiguous, strided and transposed,
    cross and auto, with rows outside [0, L) that the rule wraps; the rows are left as they were"""
    for nd in (1, 2, 3):
        for box in (UNIT[:nd], SLAB[:nd]):
            p1 = (uniform(257, nd, 40 + nd, box) * 3 - numpy.asarray(box)).astype(dtype)
            p2 = uniform(400, nd, 50 + nd, box).astype(dtype)
            radius = min(0.45 * min(box), first_radius(400, 1.5, box))           # five sources at the mean density
            grid = cell_grid(400, radius, box)
            t1 = place(p1, form, fbe.device)
            before = cpu(t1).copy()
            _, _, cnt = run_local(fbe, p1, p2, grid, box, radius, 5, form, what=(nd, box))
            assert (cnt > 5).any() and (cnt < 5).any()
            run_local(fbe, p2, None, grid, box, radius, 7, form, what=(nd, box, 'auto'))
            assert numpy.array_equal(cpu(t1), before)


# ---- 4. k and the number of sources --------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', KS)
def test_k_and_source_counts(fbe, k):
    """k from 1 to 64 with 0, 1, k - 1, k, k + 1 and 2, 63, 64, 65, 257, 1025 sources, 65 primaries: fewer than k
    candidates give the inf / -1 padding, and count stays exact"""
    p1 = uniform(65, 3, 3)
    for n2 in sorted(set([0, 1, k - 1, k, k + 1] + WAVE_NS)):
        p2 = uniform(n2, 3, 600 + n2)
        d, idx, cnt = run_local(fbe, p1, p2, cell_grid(max(65, n2), 0.45, UNIT), UNIT, 0.45, k, what=(k, n2))
        assert numpy.array_equal(numpy.isfinite(d).sum(axis=1), numpy.minimum(cnt, k))
        if n2 < k:
            assert numpy.isinf(d[:, n2:]).all() and (idx[:, n2:] == -1).all()
    for n1 in WAVE_NS:
        run_local(fbe, uniform(n1, 3, 5), uniform(300, 3, 6), cell_grid(300, 0.2, UNIT), UNIT, 0.2, k, what=(k, n1))


# ---- 5. the ring and the merge -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('descending', [False, True], ids=['ascending', 'descending'])
@pytest.mark.parametrize('m', RING_NS)
def test_ring_and_merge_edges(fbe, m, descending):
    """one primary with exactly 63 .. 257 candidates inside the radius, all in one cell, given in ascending and in
    descending order of distance (descending: tau falls with every batch, and every batch is merged)"""
    primary, sources = ring_rows(m, descending)
    r2 = r2_matrix(primary[None, :], sources, numpy.asarray(UNIT))
    assert (r2 < RING_R ** 2).sum() == m and len(numpy.unique(r2)) == len(sources)
    inside = r2[0][r2[0] < RING_R ** 2]
    assert (numpy.diff(inside) < 0).all() if descending else (numpy.diff(inside) > 0).all()
    for k in (1, 32, 63, 64):
        want, _, wcnt = knn_core(primary[None, :], sources, UNIT, RING_R ** 2, k)
        d, idx, cnt = run_sorted(fbe, primary, sources, RING_R, k)
        check_values(d, want, (m, k))
        assert cnt.tolist() == [m] == wcnt.tolist()
        check_witness(d, idx, r2, (m, k))


def test_the_nearest_come_last(fbe):
    """300 candidates of which only the last 3 are the nearest; and without the optional outputs"""
    rng = numpy.random.RandomState(4)
    v = rng.normal(size=(300, 3))
    v /= numpy.sqrt((v * v).sum(axis=1))[:, None]
    rad = numpy.concatenate([RING_R * rng.uniform(0.5, 0.95, 297), RING_R * numpy.array([0.1, 0.3, 0.2])])
    primary, sources = numpy.array([0.5, 0.5, 0.5]), 0.5 + v * rad[:, None]
    r2 = r2_matrix(primary[None, :], sources, numpy.asarray(UNIT))
    for k in (3, 5):
        want, _, _ = knn_core(primary[None, :], sources, UNIT, RING_R ** 2, k)
        d, idx, cnt = run_sorted(fbe, primary, sources, RING_R, k)
        check_values(d, want, k)
        check_witness(d, idx, r2, k)
        assert cnt.tolist() == [300] and sorted(idx[0, :3].tolist()) == [297, 298, 299]
        d2, none, _ = run_sorted(fbe, primary, sources, RING_R, k, index=False)
        assert none is None and numpy.array_equal(d, d2)


# ---- 6. ties and the strict radius ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('nd', [1, 2, 3])
def test_ties_on_the_lattice(fbe, nd):
    """the lattice of 8^nd rows has many equal r2: the values are exact, the indices witnesses"""
    pos = lattice(nd)
    for radius, k in ((2.5 / 8, 10), (3 / 8., 64), (0.5, 33)):
        run_local(fbe, pos, None, cell_grid(len(pos), radius, UNIT[:nd]), UNIT[:nd], radius, k, what=(nd, radius))


def test_a_candidate_on_the_radius(fbe):
    """a lattice spacing equal to the radius: r2 < r2max is strict, so the six rows at exactly one spacing are neither
    counted nor kept; at two spacings 27 = 1 + 6 + 12 + 8 rows are inside, the 6 at r2 = 4 / 64 are not"""
    pos = lattice(3)
    d, idx, cnt = run_local(fbe, pos, None, cell_grid(512, 1 / 8., UNIT), UNIT, 1 / 8., 4)
    assert (cnt == 1).all() and (d[:, 0] == 0).all() and numpy.isinf(d[:, 1:]).all()
    assert numpy.array_equal(idx[:, 0], numpy.arange(512))
    d, _, cnt = run_local(fbe, pos, None, cell_grid(512, 2 / 8., UNIT), UNIT, 2 / 8., 30)
    assert (cnt == 27).all() and (d[:, 26] == 3 / 64.).all() and numpy.isinf(d[:, 27:]).all()


@pytest.mark.parametrize('copies', [1, 8, 13])
def test_coincident_rows(fbe, copies):
    """1, k and k + 5 sources at the place of a primary (k = 8), among 200 others: their r2 is 0 exactly"""
    k = 8
    p1 = uniform(70, 3, 9)
    p2 = numpy.concatenate([uniform(200, 3, 10), numpy.repeat(p1[3:4], copies, axis=0)])
    d, idx, cnt = run_local(fbe, p1, p2, cell_grid(213, 0.3, UNIT), UNIT, 0.3, k, what=copies)
    assert (d[3, :min(copies, k)] == 0).all() and (idx[3, :min(copies, k)] >= 200).all()
    assert (d[3, copies:] > 0).all()


def test_auto_form_with_coincident_rows(fbe):
    """k + 5 rows at one place, auto form: the k + 1 nearest of each of them at r2 = 0 need not name the row itself
    (rule 4: otherwise the last column is dropped); the row itself is never named, the values are those of the other
    rows"""
    k = 8
    pos = numpy.concatenate([uniform(150, 3, 11), numpy.repeat([[0.3, 0.6, 0.9]], k + 5, axis=0), uniform(50, 3, 12)])
    ref = ref_knn(pos, UNIT, k)
    assert (ref['dist2'][150:150 + k + 5] == 0).all()
    check_result(run_knn(fbe, pos, UNIT, k), ref)
    # and a lone pair of coincident rows: each names the other
    res = run_knn(fbe, numpy.array([[0.3, 0.3, 0.3], [0.3, 0.3, 0.3]]), UNIT, 2)
    assert arr(res.index).tolist() == [[1, -1], [0, -1]] and arr(res.dist2)[:, 0].tolist() == [0, 0]
    assert arr(res.found).tolist() == [1, 1]


def test_two_launches_give_identical_arrays(fbe):
    pos = crowded()
    grid = cell_grid(len(pos), 0.05, UNIT)
    a = run_local(fbe, pos, None, grid, UNIT, 0.05, 32)
    b = run_local(fbe, pos, None, grid, UNIT, 0.05, 32)
    assert numpy.array_equal(a[0], b[0]) and numpy.array_equal(a[2], b[2])
    assert a[2].max() >= 600


# ---- 7. the host layer ---------------------------------------------------------------------------------------------------

def test_void_case_needs_three_rounds():
    """conditions on the input, checked without a GPU: the second isolated row has fewer than k + 1 rows within 2 R_0 <
    rmax (two rounds do not resolve it), and the far row has nothing within rmax"""
    pos = void_rows()
    ref = reference('void', lambda: ref_knn(pos, UNIT, VOID_K))
    r0 = first_radius(len(pos), VOID_K, UNIT)
    assert 2 * r0 < 0.5 and (ref['dist2'][:, VOID_K - 1] >= (2 * r0) ** 2).sum() >= 2
    assert ref['found'][-1] == 0 and ref['found'][:-1].min() == VOID_K


@pytest.mark.parametrize('name', ['uniform', 'uniform-cross', 'crowded', 'void', 'slab-2d'])
def test_knn_on_cases(fbe, name):
    """knn equals the restatement on uniform rows (auto and cross), on 600 rows in one cell, on a cluster with voids
    (at least three rounds; the far row ends with nothing) and on a two-dimensional box"""
    if name == 'uniform':
        pos, kw = uniform(1500, 3, 30), dict(box=UNIT, k=8)
    elif name == 'uniform-cross':
        pos, kw = uniform(700, 3, 32), dict(box=UNIT, k=5, pos2=uniform(900, 3, 33))
    elif name == 'crowded':
        pos, kw = crowded(), dict(box=UNIT, k=32)
    elif name == 'void':
        pos, kw = void_rows(), dict(box=UNIT, k=VOID_K)
    else:
        pos, kw = uniform(800, 2, 34, SLAB[:2]), dict(box=SLAB[:2], k=63)
    ref = reference(name, lambda: ref_knn(pos, **kw))
    res = run_knn(fbe, pos, kw['box'], kw['k'], pos2=kw.get('pos2'))
    check_result(res, ref, name, offset=None if 'pos2' in kw else 0)
    assert res.rmax == min(kw['box']) / 2 and res.rounds >= 1
    assert torch.equal(res.dist, torch.sqrt(res.dist2))
    if name == 'void':
        assert res.rounds >= 3 and int(res.found[-1]) == 0 and numpy.isinf(arr(res.dist2)[-1]).all()


@pytest.mark.parametrize('factor', [0.25, 4.0])
def test_the_schedule_does_not_matter(fbe, factor, monkeypatch):
    """R_0 replaced by R_0 / 4 and by 4 R_0: identical dist2 and found (rule 3), other round counts"""
    real = first_radius
    monkeypatch.setattr(knn_module, 'first_radius', lambda n, k, box: factor * real(n, k, box))
    for name, pos, k in (('uniform', uniform(1500, 3, 30), 8), ('void', void_rows(), VOID_K)):
        ref = reference(name, lambda: ref_knn(pos, UNIT, k))
        res = run_knn(fbe, pos, UNIT, k)
        check_result(res, ref, (name, factor), offset=0)
        if name == 'void':
            assert res.rounds >= (5 if factor < 1 else 2)


def test_rmax_and_index(fbe):
    """an rmax smaller than most k-th distances: the rows keep what lies inside, inf-padded; index=False; numpy rows in,
    device tensors out; empty sets"""
    pos, pos2 = uniform(500, 3, 35), uniform(400, 3, 36)
    for kw in (dict(k=8, rmax=0.08), dict(k=8, rmax=0.08, pos2=pos2), dict(k=3, rmax=0.5)):
        ref = ref_knn(pos, UNIT, **kw)
        if kw['rmax'] < 0.5:
            assert (ref['found'] < 8).sum() > 250 and (ref['found'] > 0).sum() > 250
        for index in (True, False):
            res = run_knn(fbe, pos, UNIT, kw['k'], pos2=kw.get('pos2'), rmax=kw['rmax'], index=index)
            check_result(res, ref, kw['k'], offset=None if 'pos2' in kw else 0, index=index)
            assert res.rmax == kw['rmax']
    res = knn(mesh(UNIT), pos, 4, pos2=pos2.astype('f4'))
    assert res.dist2.device == fbe.device
    check_result(res, ref_knn(pos, UNIT, 4, pos2=pos2.astype('f4')), offset=None)
    res = knn(mesh(UNIT), numpy.zeros((0, 3)), 4)
    assert tuple(res.dist2.shape) == (0, 4) and tuple(res.index.shape) == (0, 4) and tuple(res.found.shape) == (0,)
    res = knn(mesh(UNIT), pos, 4, pos2=numpy.zeros((0, 3)))
    assert numpy.isinf(arr(res.dist2)).all() and (arr(res.index) == -1).all() and not arr(res.found).any()
    res = knn(mesh(UNIT), pos[:1], 4)
    assert numpy.isinf(arr(res.dist2)).all() and arr(res.index).tolist() == [[-1] * 4]


@pytest.mark.parametrize('nd', [1, 2, 3])
def test_knn_density(fbe, nd):
    """rho = M / V_ndim(d_k) against the formula applied to the restatement's d_k.  The bound: dist2 is exact and both
    square roots are correctly rounded, so d_k is the same double; V takes at most five roundings (the constant, the
    powers of r, the product) and the division one, on either side: 8 ulp in all without masses.  With masses M is a
    sum of k positive terms in any order, within (k - 1) 2^-53 of the exact sum on either side: (k - 1) ulp more."""
    box = SLAB[:nd]
    pos, pos2 = uniform(400, nd, 70 + nd, box), uniform(300, nd, 80 + nd, box)
    m2 = numpy.random.RandomState(7).uniform(0.5, 1.5, 300)
    k = 6
    rmax = 0.4 * min(box)
    const = {1: 2.0, 2: numpy.pi, 3: 4 * numpy.pi / 3}[nd]
    for auto in (False, True):
        src = pos if auto else pos2
        mass = numpy.random.RandomState(8).uniform(0.5, 1.5, len(src))
        ref = ref_knn(pos, box, k, pos2=None if auto else pos2, rmax=rmax)
        ok = ref['found'] >= k
        assert ok.sum() > 100
        dk = numpy.sqrt(ref['dist2'][:, k - 1])
        with numpy.errstate(invalid='ignore'):
            plain = numpy.where(ok, k / (const * dk ** nd), 0.0)
        got = arr(knn_density(mesh(box), pos, k=k, pos2=None if auto else pos2, rmax=rmax))
        assert got.dtype == numpy.float64 and (got[~ok] == 0).all()
        assert (numpy.abs(got - plain) <= 8 * 2.0 ** -52 * plain).all()
        # with masses: the sum over the neighbours the result itself names (ties aside, those of the restatement)
        got = arr(knn_density(mesh(box), pos, k=k, pos2=None if auto else pos2, mass2=mass, rmax=rmax))
        M = numpy.where(ref['index'] >= 0, mass[numpy.maximum(ref['index'], 0)], 0.0).sum(axis=1)
        with numpy.errstate(invalid='ignore'):
            want = numpy.where(ok, M / (const * dk ** nd), 0.0)
        assert (got[~ok] == 0).all()
        assert (numpy.abs(got - want) <= (k + 7) * 2.0 ** -52 * want).all()
    with pytest.raises(ValueError, match='mass2'):
        knn_density(mesh(box), pos, k=k, pos2=pos2, mass2=m2[:-1])


def test_knn_cdf(fbe):
    """the cumulative counts against counts made from the restatement; query rows on lattice sites see their second
    data row at exactly one spacing, and the edge 1/8 does not count it (strict, no square root)"""
    data = numpy.concatenate([lattice(3), uniform(200, 3, 90)])
    query = numpy.concatenate([lattice(3)[:60], uniform(140, 3, 91)])
    ks, redges = [1, 2, 8], numpy.array([0.0, 0.0625, 0.125, 0.2, 0.3])
    ref = ref_knn(query, UNIT, 8, pos2=data, rmax=0.3)
    want = numpy.array([[(ref['dist2'][:, a - 1] < e * e).sum() for e in redges] for a in ks])
    assert (ref['dist2'][:60, 1] == 1 / 64.).sum() >= 10 and want[1, 2] + 10 <= (ref['dist2'][:, 1] <= 1 / 64.).sum()
    for rmax in (None, 0.45):
        N, nquery = knn_cdf(mesh(UNIT), data, query, ks, redges, rmax=rmax)
        assert N.dtype == numpy.int64 and N.shape == (3, 5) and nquery == 200
        assert numpy.array_equal(N, want), (N, want)
    for bad in (dict(ks=[]), dict(ks=[0]), dict(ks=[65]), dict(ks=[1.5]), dict(redges=[0.2, 0.1]), dict(redges=[]),
                dict(redges=[0.1, numpy.nan]), dict(redges=[0.0]), dict(rmax=0.2), dict(redges=[0.1, 0.6])):
        with pytest.raises(ValueError):
            knn_cdf(mesh(UNIT), data, query, **dict(dict(ks=ks, redges=redges), **bad))


# ---- 8. ranks ------------------------------------------------------------------------------------------------------------

RANK_CASES = {
    'cross': dict(pos=uniform(600, 3, 44), pos2=uniform(500, 3, 45), box=UNIT, k=6),
    'auto': dict(pos=uniform(700, 3, 46), box=UNIT, k=5),
    'slab': dict(pos=uniform(600, 3, 47, SLAB), box=SLAB, k=4, rmax=0.1),
    'void': dict(pos=void_rows()[numpy.random.RandomState(3).permutation(803)], box=UNIT, k=VOID_K),
}


def rank_reference(name):
    kw = RANK_CASES[name]
    return reference('ranks-' + name, lambda: ref_knn(kw['pos'], kw['box'], kw['k'], kw.get('pos2'), kw.get('rmax')))


def test_rank_inputs():
    """conditions on the inputs of the rank tests, checked without a GPU: a primary whose k-th neighbour lies across
    the cut at x = 1/2 (another rank's block for two ranks and for 2 x 2), and one that needs a second round"""
    for name, kw in RANK_CASES.items():
        ref = rank_reference(name)
        src = kw.get('pos2', kw['pos'])
        kth = ref['index'][:, kw['k'] - 1]
        ok = kth >= 0
        side1, side2 = kw['pos'][ok, 0] % 1.0 < 0.5, src[kth[ok], 0] % 1.0 < 0.5
        assert (side1 != side2).sum() >= 1, name
        r0 = first_radius(len(src), kw['k'], kw['box'])
        column = kw['k'] - 1
        if r0 < (kw.get('rmax') or min(kw['box']) / 2):
            assert (ref['dist2'][:, column] >= r0 * r0).sum() >= 1, name


def check_ranks(name, size, np_):
    """knn on thread ranks holding both sets split unevenly (one rank holds no rows) against the one-rank restatement
    of all rows: dist2 and found exactly, the indices valid global witnesses"""
    kw = RANK_CASES[name]
    p1, p2 = kw['pos'], kw.get('pos2')
    s1 = split(len(p1), size)
    s2 = split(len(p2), size) if p2 is not None else None
    ref = rank_reference(name)

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a = s1[comm.rank]
        res = knn(pm, p1[a], kw['k'], pos2=None if p2 is None else p2[s2[comm.rank]], rmax=kw.get('rmax'))
        return res, a
    results = thread_ranks(size, body)
    sizes = [results[r][0].dist2.shape[0] for r in range(size)]
    assert 0 in sizes and sum(sizes) == len(p1)
    for r in range(size):
        res, rows = results[r]
        check_result(res, ref, (name, size, r), offset=None if p2 is not None else rows.start, rows=rows)
    assert len(set(results[r][0].rounds for r in range(size))) == 1
    if name == 'void':
        assert results[0][0].rounds >= 3


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_result(obe, size, np_):
    for name in RANK_CASES:
        check_ranks(name, size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    for name in RANK_CASES:
        check_ranks(name, size, np_)


def test_ranks_density_and_cdf(obe):
    """knn_density with masses and knn_cdf over three ranks: the masses follow the global indices, the counts are summed"""
    kw = RANK_CASES['cross']
    mass = numpy.random.RandomState(5).uniform(0.5, 1.5, len(kw['pos2']))
    ref = rank_reference('cross')
    k = kw['k']
    dk = numpy.sqrt(ref['dist2'][:, k - 1])
    want = mass[ref['index']].sum(axis=1) / (4 * numpy.pi / 3 * dk ** 3)
    redges = [0.05, 0.1, 0.2]
    cdf = numpy.array([[(ref['dist2'][:, a - 1] < e * e).sum() for e in redges] for a in (1, k)])
    s1, s2 = split(600, 3), split(500, 3)

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        a, b = s1[comm.rank], s2[comm.rank]
        rho = cpu(knn_density(pm, kw['pos'][a], k=k, pos2=kw['pos2'][b], mass2=mass[b]))
        assert (numpy.abs(rho - want[a]) <= (k + 7) * 2.0 ** -52 * want[a]).all()
        N, nquery = knn_cdf(pm, kw['pos2'][b], kw['pos'][a], [1, k], redges)
        assert nquery == 600 and numpy.array_equal(N, cdf)
        return True
    thread_ranks(3, body)


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        for k in (0, 65):
            with pytest.raises(ValueError):
                knn(pm, mine, k if comm.rank == 1 else 4, pos2=mine)
        with pytest.raises(ValueError):
            knn(pm, mine, 64 if comm.rank == 0 else 4)
        with pytest.raises(ValueError):
            knn(pm, mine, 4, rmax=0.51 if comm.rank == 2 else 0.3)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            knn(pm, bad, 4)
        with pytest.raises(ValueError):
            knn(pm, mine, 4, pos2=mine[:, :2] if comm.rank == 1 else mine)
        with pytest.raises(TypeError):
            knn(pm, (mine * 8).astype('i8') if comm.rank == 2 else mine, 4)
        res = knn(pm, mine, 4)
        check_values(res.dist2, ref_knn(pos, UNIT, 4)['dist2'][30 * comm.rank:30 * comm.rank + 30])
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 9. bad arguments ----------------------------------------------------------------------------------------------------

def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    with pytest.raises(NotImplementedError):
        knn(mesh([1.0] * 4), uniform(20, 4, 1), 3)
    with pytest.raises(NotImplementedError):
        knn_density(mesh([1.0] * 4), uniform(20, 4, 1), 3)
    for k in (0, 65, -1, 2.5, 'many', None):
        with pytest.raises(ValueError, match='k must'):
            knn(pm, pos, k, pos2=pos)
    with pytest.raises(ValueError, match='k must'):
        knn(pm, pos, 64)                                         # the auto form asks for k + 1
    assert tuple(knn(pm, pos, 63).dist2.shape) == (50, 63) and tuple(knn(pm, pos, 64, pos2=pos).dist2.shape) == (50, 64)
    for rmax in (0.0, -0.1, numpy.nan, numpy.inf, 0.51, 'far'):
        with pytest.raises(ValueError, match='rmax'):
            knn(pm, pos, 3, rmax=rmax)
    with pytest.raises(ValueError, match='rmax'):
        knn(mesh(SLAB), pos, 3, rmax=0.13)                       # 2 rmax > the shortest side
    assert knn(mesh(SLAB), pos, 3).rmax == 0.125
    with pytest.raises(ValueError, match='shape'):
        knn(pm, pos[:, :2], 3)
    with pytest.raises(ValueError, match='shape'):
        knn(pm, pos, 3, pos2=pos[:, :2])
    with pytest.raises(TypeError):
        knn(pm, (pos * 100).astype('i8'), 3)
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows'):
        knn(pm, bad, 3)
    with pytest.raises(ValueError, match='3 rows'):
        knn(pm, bad, 3, pos2=bad[5:8])


# ---- 10. the ABI and the resources ---------------------------------------------------------------------------------------

def test_the_entry_is_bound():
    assert 'knn' in _abi.DEVICE_ONLY and _abi.PMX_KNN_MAX_K == 64 == knn_module.MAX_K
    lib = backend.load_library()
    assert hasattr(lib, 'pmx_knn')
    import pmesh_amd
    assert 'knn_density' in pmesh_amd.__doc__ and 'knn_cdf' in pmesh_amd.__doc__
    from tests.test_abi import declared_symbols, generator, header_text
    assert 'pmx_knn' in declared_symbols()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pyx, abi, fnptrs = generator().generate(header_text())
    assert open(os.path.join(root, 'pmesh_amd', '_pmx.pyx')).read() == pyx
    assert open(os.path.join(root, 'pmesh_amd', '_abi_gen.py')).read() == abi
    assert open(os.path.join(root, 'pmesh_amd', 'csrc', 'pmx_fnptrs.h')).read() == fnptrs
    assert 'pmx_knn' in pyx and "'knn'" in abi


def test_knn_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_knn.hip')
    # knn_kernel<NDIM>, NDIM = 1, 2, 3; and no others
    assert sorted(t) == ['_ZN3pmx10knn_kernelILi%dEEEvNS_5KArgsE' % nd for nd in (1, 2, 3)], sorted(t)
    for name, r in t.items():
        # a spilled sort network would defeat the kernel
        assert r['ScratchSize'] == 0, (name, r)
        # a ring of 128 entries per wave, four waves: 8 bytes for r2 and 4 for the slot
        assert r['LDS'] == 4 * 128 * 12, (name, r)
        # measured at compile time: 46, 52 and 58 VGPRs for NDIM = 1, 2, 3, eight waves per SIMD
        assert r['VGPRs'] <= 64, (name, r)
        assert r['Occupancy'] >= 8, (name, r)
