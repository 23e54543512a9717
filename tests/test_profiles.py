"""pmesh_amd.profiles (csrc/pmx_pairs_rows.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/profiles.py, include/pmesh_amd.h) is that of the modes 1d and projected of pmesh_amd.paircount
with one histogram per centre: the bin of a pair (centre i, source j) is (i * nr + rbin) * nsub + subbin.  There is no
row identity: a centre that coincides with a source is a pair at r2 == 0.

The restatement is brute force over the full (n1, n2) matrix with the comparisons of tests.test_paircount.count_core
(profile_core; test_restatement_is_count_core_per_row holds it to count_core applied row by row).  Under -m "not gpu"
it serves the two new modes of pmx_pair_counts (ProfilesOracleBackend; the old modes go to its parent), so the host
layer and the thread ranks run without a GPU; under -m gpu the kernel is compared with it.

npart is compared by exact integer equality everywhere.  mass and rsum are held per (centre, bin) within the bound of
tests.test_paircount.check: |got - ref| <= (M + 4) 2^-52 S, M the pairs of that bin of that centre, S the sum of the
absolute values of its terms; where the weights are multiples of 1/8 and the rows lie on a 2^-12 lattice, mass is
compared by equality.  Random inputs keep every pair at least 1e-9 (relative) from an edge, as in tests.test_paircount.

so_masses is compared with a numpy restatement of its rule on the restatement's own cumulative masses.  With unit
masses both sides read the same integers, and what is left are the roundings of the elementary functions: the bound
is worked out in so_bound.
"""
import math
import os

import numpy
import pytest
import torch

import pmesh_amd
from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid, cell_sort
from pmesh_amd.knn import ball_volume
from pmesh_amd.paircount import bin_volumes, pair_counts
from pmesh_amd.profiles import (MAX_BINS, ROW_MODES, ProfileResult, SOResult, local_profiles, radial_profiles,
                                so_masses)
from tests.test_fof import (GRIDS, RANKS, ROW_FORMS, SLAB, UNIT, face_pairs, lattice, mesh, place, split,
                            thread_ranks, uniform, wrap)
from tests.test_lpt import cpu
from tests.test_paircount import (U, PairsOracleBackend, check, count_core, dyadic_weights, grid_of, lattice_rows)

RWAVES = 4               # centres per workgroup of rows_kernel (csrc/pmx_pairs_rows.hip)
CODES = {v: k for k, v in ROW_MODES.items()}


# ---- the restatement -----------------------------------------------------------------------------------------------

def profile_core(w1, w2, box, mode, los, e2, sub, wt1=None, wt2=None):
    """The sums over the pairs of every wrapped row of w1 with the wrapped rows w2: a dict of npairs, wnpairs, rsum
    of the shape (n1, nr * nsub), and margin: the comparisons of count_core, the row of w1 kept in the bin index"""
    n1, n2, nd = len(w1), len(w2), w1.shape[1]
    nr, nsub = len(e2) - 1, (1 if mode == '1d' else len(sub) - 1)
    nbins = nr * nsub
    out = dict(npairs=numpy.zeros((n1, nbins), dtype='i8'), wnpairs=numpy.zeros((n1, nbins)),
               rsum=numpy.zeros((n1, nbins)), margin=numpy.inf)
    if n1 == 0 or n2 == 0:
        return out
    dx = []
    for d in range(nd):
        x = w1[:, None, d] - w2[None, :, d]
        dx.append(x - box[d] * numpy.rint(x / box[d]))
    q = numpy.zeros((n1, n2))
    for d in range(nd):
        if mode != 'projected' or d != los:
            q = q + dx[d] * dx[d]
    keep = (q >= e2[0]) & (q < e2[-1])
    rbin = numpy.searchsorted(e2, q, side='right') - 1
    margin = numpy.inf
    pe = e2[e2 > 0]
    for shift in (1, 0):
        near = pe[numpy.clip(numpy.searchsorted(pe, q) - shift, 0, len(pe) - 1)]
        margin = min(margin, float((numpy.abs(q - near) / near).min()))
    sbin = numpy.zeros((n1, n2), dtype='i8')
    if mode == 'projected':
        a = numpy.abs(dx[los])
        for k in range(1, nsub + 1):
            if k < nsub:
                sbin += a >= sub[k]
            if keep.any():
                margin = min(margin, float(numpy.abs(a - sub[k])[keep].min()))
        keep &= a < sub[-1]
    w = numpy.ones((n1, n2))
    if wt1 is not None:
        w = w * numpy.asarray(wt1).astype('f8').reshape(-1)[:, None]
    if wt2 is not None:
        w = w * numpy.asarray(wt2).astype('f8').reshape(-1)[None, :]
    flat = (numpy.arange(n1)[:, None] * nbins + rbin * nsub + sbin)[keep]
    out['npairs'] = numpy.bincount(flat, minlength=n1 * nbins).astype('i8').reshape(n1, nbins)
    out['wnpairs'] = numpy.bincount(flat, weights=w[keep], minlength=n1 * nbins).reshape(n1, nbins)
    out['rsum'] = numpy.bincount(flat, weights=(w * numpy.sqrt(q))[keep], minlength=n1 * nbins).reshape(n1, nbins)
    out['margin'] = margin
    return out


def ref_profiles(centres, pos, box, edges, mass=None, weight=None, mode='1d', sub=None, los=2):
    """the restatement of radial_profiles(mesh(box), centres, pos, edges, mass, weight, mode, piedges=sub, los=los)"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    s = None if sub is None else numpy.asarray(sub, dtype='f8')
    return profile_core(wrap(centres, box), wrap(pos, box), box, mode, los, e * e, s, weight, mass)


def flat(ref):
    """the restatement's dict in the form tests.test_paircount.check takes: every (centre, bin) is a bin of its own"""
    return dict(npairs=ref['npairs'].reshape(-1), wnpairs=ref['wnpairs'].reshape(-1), rsum=ref['rsum'].reshape(-1))


def check_profiles(got, ref, exact_w=False, what=''):
    """a ProfileResult (or a triple of arrays) against the restatement's dict"""
    if isinstance(got, ProfileResult):
        n1 = ref['npairs'].shape[0]
        assert got.npart.dtype == torch.int64 and got.npart.shape[0] == n1
        assert got.npart.shape == got.mass.shape == got.rsum.shape == got.rmean.shape
        got = (got.npart, got.mass, got.rsum)
    if ref['npairs'].size == 0:                                 # (no centres: tests.test_paircount.check wants a bin)
        assert all(x.shape[0] == 0 for x in got)
        return
    check(tuple(got), flat(ref), exact_w=exact_w, what=what)


class ProfilesOracleBackend(PairsOracleBackend):
    """the CPU test double with the two row modes of pmx_pair_counts served by the restatement"""
    name = 'oracle-profiles'

    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        if mode not in CODES:
            return PairsOracleBackend.pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2,
                                                  cell_start2, weight2, ncell, periodic, boxsize, e2, sub, npairs,
                                                  wnpairs, rsum)
        n1, n2, nd = spos1.shape[0], spos2.shape[0], spos1.shape[1]
        if n1 == 0 or n2 == 0:
            return
        nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
        assert nbins <= MAX_BINS and npairs.numel() == wnpairs.numel() == rsum.numel() == n1 * nbins
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell))
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = profile_core(a, b, numpy.asarray(boxsize, dtype='f8'), CODES[mode], los, e2.numpy(),
                           None if sub is None else sub.numpy(), None if weight1 is None else weight1.numpy(),
                           None if weight2 is None else weight2.numpy())
        npairs += torch.from_numpy(got['npairs']).reshape(npairs.shape)
        wnpairs += torch.from_numpy(got['wnpairs']).reshape(wnpairs.shape)
        rsum += torch.from_numpy(got['rsum']).reshape(rsum.shape)


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(ProfilesOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def rbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(ProfilesOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    torch.cuda.synchronize()
    backend.reset()


# ---- the inputs ----------------------------------------------------------------------------------------------------

def clustered(n, seed, nblob=6, sigma=0.012, share=0.7):
    """rows of the unit box: `share` of them in `nblob` Gaussian blobs, the rest uniform; and the blob centres"""
    rng = numpy.random.RandomState(seed)
    c = rng.uniform(0.1, 0.9, size=(nblob, 3))
    m = int(share * n)
    rows = numpy.concatenate([c[rng.randint(0, nblob, size=m)] + sigma * rng.normal(size=(m, 3)),
                              rng.uniform(size=(n - m, 3))])
    return rows[rng.permutation(n)] % 1.0, c


def bins_case(nr):
    pos = uniform(1500, 3, 200 + nr)
    return dict(centres=numpy.concatenate([pos[:200], uniform(100, 3, 300 + nr)]), pos=pos, box=UNIT,
                edges=numpy.linspace(0.0, 0.12, nr + 1))


def random_cases():
    """name -> keyword arguments of ref_profiles: every random input of the tests below"""
    cases = {}
    for nr in (1, 8, 9, 128, 129, 256):
        cases['bins-%d' % nr] = bins_case(nr)
    cases['bins-16x16'] = dict(bins_case(16), mode='projected', sub=numpy.linspace(0.0, 0.1, 17), los=1)
    cases['bins-2x128'] = dict(bins_case(2), mode='projected', sub=numpy.linspace(0.0, 0.1, 129), los=0)
    cases['bins-1x129'] = dict(bins_case(1), mode='projected', sub=numpy.linspace(0.0, 0.1, 130), los=2)
    cases['edges-above-0'] = dict(bins_case(4), edges=[0.01, 0.015, 0.04, 0.1, 0.11])
    rows, blobs = clustered(3000, 11)
    cases['clustered'] = dict(centres=numpy.concatenate([blobs, rows[:300]]), pos=rows, box=UNIT,
                              edges=numpy.geomspace(0.002, 0.08, 13))
    cases['weights'] = dict(centres=uniform(400, 3, 12), pos=uniform(1200, 3, 13), box=UNIT,
                            edges=numpy.linspace(0.0, 0.15, 7),
                            weight=numpy.random.RandomState(5).uniform(0.5, 1.5, 400),
                            mass=numpy.random.RandomState(6).uniform(0.5, 1.5, 1200).astype('f4'))
    cases['projected'] = dict(centres=uniform(300, 3, 14, SLAB), pos=uniform(900, 3, 15, SLAB), box=SLAB,
                              edges=[0.0, 0.02, 0.05, 0.08], mode='projected', sub=[0.0, 0.03, 0.06, 0.09], los=0,
                              mass=numpy.random.RandomState(7).uniform(0.5, 1.5, 900))
    for nd in (3, 2, 1):
        rows = numpy.concatenate([face_pairs(SLAB[:nd], 0.05), uniform(300, nd, 61, SLAB[:nd])])
        cases['faces-%dd' % nd] = dict(centres=rows[::2].copy(), pos=rows, box=SLAB[:nd],
                                       edges=[0.0, 0.02, 0.04, 0.05])
    cases['open'] = dict(centres=uniform(2000, 3, 12), pos=uniform(2000, 3, 12), box=UNIT, edges=[0.01, 0.03, 0.05])
    cases['ranks'] = dict(centres=uniform(500, 3, 44), pos=uniform(900, 3, 45), box=UNIT,
                          edges=numpy.linspace(0, 0.1, 5), weight=numpy.random.RandomState(7).uniform(0.5, 1.5, 500),
                          mass=numpy.random.RandomState(8).uniform(0.5, 1.5, 900))
    cases['ranks-slab'] = dict(centres=uniform(400, 3, 46, SLAB), pos=uniform(900, 3, 47, SLAB), box=SLAB,
                               edges=[0.0, 0.04, 0.08, 0.1], mode='projected', sub=[0.0, 0.03, 0.07])
    # one crowded cell: 3000 sources in a ball of radius 0.02, 60 of them centres, and a thin background
    rng = numpy.random.RandomState(21)
    v = rng.normal(size=(3000, 3))
    v *= (0.02 * rng.uniform(size=3000) ** (1 / 3.) / numpy.sqrt((v * v).sum(axis=1)))[:, None]
    rows = numpy.concatenate([0.5 + v, uniform(200, 3, 22)])
    cases['crowded'] = dict(centres=numpy.concatenate([rows[:60], uniform(10, 3, 23)]), pos=rows, box=UNIT,
                            edges=numpy.linspace(0.0, 0.05, 7))
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_profiles(**RANDOM[name])
    return _REFERENCE[name]


def run_case(be, name, **over):
    """radial_profiles of a random case on one rank"""
    kw = dict(RANDOM[name], **over)
    t = lambda x: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(be.device)
    return radial_profiles(mesh(kw['box']), t(kw['centres']), t(kw['pos']), kw['edges'], mass=t(kw.get('mass')),
                           weight=t(kw.get('weight')), mode=kw.get('mode', '1d'), piedges=kw.get('sub'),
                           los=kw.get('los', 2))


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_is_count_core_per_row():
    """profile_core is count_core applied to one centre at a time: the same integers, and the same sums to the bound
    of a double sum in any order; and its sum over the centres is count_core of all of them"""
    for name in ('weights', 'projected'):
        kw = RANDOM[name]
        box = numpy.asarray(kw['box'], dtype='f8')
        mode, los = kw.get('mode', '1d'), kw.get('los', 2)
        e = numpy.asarray(kw['edges'], dtype='f8')
        sub = None if kw.get('sub') is None else numpy.asarray(kw['sub'], dtype='f8')
        a, b = wrap(kw['centres'], box), wrap(kw['pos'], box)
        ref = reference(name)
        for i in range(0, len(a), 7):
            w1 = None if kw.get('weight') is None else kw['weight'][i:i + 1]
            one = count_core(a[i:i + 1], b, box, mode, los, e * e, sub, w1, kw.get('mass'))
            check((ref['npairs'][i], ref['wnpairs'][i], ref['rsum'][i]), one, what=(name, i))
        whole = count_core(a, b, box, mode, los, e * e, sub, kw.get('weight'), kw.get('mass'))
        assert numpy.array_equal(ref['npairs'].sum(axis=0), whole['npairs']) and whole['npairs'].sum() > 1000
        assert ref['margin'] == whole['margin']


def test_restatement_on_known_answers():
    """the 8^3 lattice of spacing 1/8 about one of its points: the point itself in [0, 1/8), then r3(1..3) = 6 + 12 +
    8, r3(4..8) = 66 and r3(9..15) = 158 neighbours; pairs at exactly an edge go to the bin above, pairs at exactly
    the last edge are out; five rows on a line"""
    pos = lattice(3)
    got = ref_profiles(pos[[0, 77]], pos, UNIT, [0, 1 / 8., 2 / 8., 3 / 8., 1 / 2.])
    assert got['npairs'].tolist() == [[1, 26, 66, 158]] * 2 and got['rsum'][0, 0] == 0.0
    assert ref_profiles(pos[[5]], pos, UNIT, [1 / 8., 2 / 8., 3 / 8.])['npairs'].tolist() == [[26, 66]]
    assert ref_profiles(pos[[5]] + 1 / 16., pos, UNIT, [0, 0.1])['npairs'].tolist() == [[0]]
    line = numpy.array([[0.95], [0.5], [0.02], [0.09], [0.41]])
    got = ref_profiles(numpy.array([[0.0], [0.45]]), line, [1.0], [0.0, 0.06, 0.1])
    assert got['npairs'].tolist() == [[2, 1], [2, 0]]           # 0.95 and 0.02 | 0.09; 0.5 and 0.41 | none
    assert abs(got['rsum'][0, 0] - 0.07) < 1e-15


@pytest.mark.parametrize('name', sorted(RANDOM))
def test_inputs_are_decided(name):
    kw = RANDOM[name]
    ref = reference(name)
    assert ref['margin'] >= 1e-9, (name, ref['margin'])
    b = numpy.hypot(kw['edges'][-1], kw['sub'][-1]) if kw.get('mode') == 'projected' else kw['edges'][-1]
    assert 2 * b <= min(kw['box']) and len(kw['pos']) <= 3200 and len(kw['centres']) <= 2000
    assert (ref['npairs'].sum(axis=0) > 0).sum() >= min(ref['npairs'].shape[1], 3), name


# ---- 2. known answers ----------------------------------------------------------------------------------------------------

def test_known_answer(rbe):
    """the lattice about lattice points, its squared edges exact, so that pairs sit on edges: [1, 26, 66, 158] per
    centre; without weights mass = npart; rmean of the first shell bin is the mean over its three shells; the 2-d and
    1-d lattices"""
    pm = mesh(UNIT)
    pos = torch.from_numpy(lattice(3)).to(rbe.device)
    edges = [0, 1 / 8., 2 / 8., 3 / 8., 1 / 2.]
    res = radial_profiles(pm, pos[[0, 77, 511]], pos, edges)
    assert isinstance(res, ProfileResult) and res.mode == '1d' and tuple(res.npart.shape) == (3, 4)
    assert cpu(res.npart).tolist() == [[1, 26, 66, 158]] * 3
    assert cpu(res.mass).tolist() == [[1.0, 26.0, 66.0, 158.0]] * 3
    check_profiles(res, ref_profiles(lattice(3)[[0, 77, 511]], lattice(3), UNIT, edges))
    assert (numpy.abs(cpu(res.rmean)[:, 1] - (6 + 12 * 2 ** 0.5 + 8 * 3 ** 0.5) / 26 / 8) <= 1e-14).all()
    assert (cpu(res.rmean)[:, 0] == 0).all()
    res = radial_profiles(pm, pos, pos, [1 / 8., 2 / 8., 3 / 8.])
    assert cpu(res.npart).tolist() == [[26, 66]] * 512
    for nd in (2, 1):
        ref = ref_profiles(lattice(nd)[3:8], lattice(nd), UNIT[:nd], edges)
        assert ref['npairs'].tolist() == [[1, 8, 16, 20] if nd == 2 else [1, 2, 2, 2]] * 5
        check_profiles(radial_profiles(mesh(UNIT[:nd]), lattice(nd)[3:8], lattice(nd), edges), ref)


def test_coincident_and_empty(rbe):
    """a centre that coincides with a source counts it in bin 0 when edges[0] == 0 and nowhere when edges[0] > 0 (there
    is no row identity); a centre with nothing around it has zeros and rmean nan; no centres and no sources"""
    pos = numpy.concatenate([uniform(300, 3, 2) * 0.4, [[0.25, 0.25, 0.25]] * 3])
    centres = numpy.array([[0.25, 0.25, 0.25], [0.8, 0.8, 0.8], [1.25, 0.25, 0.25]])
    pm = mesh(UNIT)
    ref = ref_profiles(centres, pos, UNIT, [0.0, 1e-4, 0.05])
    assert ref['npairs'][:, 0].tolist() == [3, 0, 3] and ref['npairs'][1].sum() == 0 and ref['npairs'][0, 1] > 0
    res = radial_profiles(pm, centres, pos, [0.0, 1e-4, 0.05])
    check_profiles(res, ref)
    assert cpu(res.rsum)[[0, 2], 0].tolist() == [0.0, 0.0]
    assert numpy.isnan(cpu(res.rmean)[1]).all() and not numpy.isnan(cpu(res.rmean)[0]).any()
    res = radial_profiles(pm, centres, pos, [1e-6, 1e-4, 0.05])
    assert cpu(res.npart)[:, 0].tolist() == [0, 0, 0]
    check_profiles(res, ref_profiles(centres, pos, UNIT, [1e-6, 1e-4, 0.05]))
    res = radial_profiles(pm, centres, pos, [0.0, 1e-4], mode='projected', piedges=[0.0, 0.1, 0.2], los=1)
    assert cpu(res.npart)[0, 0, 0] >= 3
    check_profiles(res, ref_profiles(centres, pos, UNIT, [0.0, 1e-4], mode='projected', sub=[0.0, 0.1, 0.2], los=1))
    none = radial_profiles(pm, numpy.zeros((0, 3)), pos, [0.0, 0.1, 0.2])
    assert tuple(none.npart.shape) == (0, 2) and tuple(none.rmean.shape) == (0, 2)
    none = radial_profiles(pm, centres, numpy.zeros((0, 3)), [0.0, 0.1, 0.2])
    assert cpu(none.npart).tolist() == [[0, 0]] * 3 and numpy.isnan(cpu(none.rmean)).all()


# ---- 3. the kernel's paths -------------------------------------------------------------------------------------------------

def neighbourhood(nc, m, seed):
    """nc centres and their sources: centre 0 at the middle of the box with exactly m sources within 0.09 of it and
    nothing else within 0.3, the other centres among 200 sources in the slab x < 0.15"""
    rng = numpy.random.RandomState(seed)
    v = rng.normal(size=(m, 3))
    v *= (0.09 * rng.uniform(size=m) ** (1 / 3.) / numpy.sqrt((v * v).sum(axis=1)))[:, None]
    far = uniform(200, 3, seed + 1) * [0.15, 1.0, 1.0]
    centres = numpy.concatenate([[[0.5, 0.5, 0.5]], far[:nc - 1] + 0.003])
    pos = numpy.concatenate([0.5 + v, far])
    return centres, pos[rng.permutation(len(pos))]


@pytest.mark.parametrize('nc', [1, RWAVES - 1, RWAVES, RWAVES + 1])
def test_wave_and_workgroup_edges(rbe, nc):
    """1, waves-per-workgroup - 1, waves-per-workgroup and waves-per-workgroup + 1 centres; 0, 1, 63, 64, 65 and
    64 * 5 + 1 sources in the 27 cells of the first centre: the strides of the wave over the ranges laid end to end"""
    pm = mesh(UNIT)
    edges = [0.0, 0.03, 0.06, 0.1]
    for m in (0, 1, 63, 64, 65, 64 * 5 + 1):
        centres, pos = neighbourhood(nc, m, 400 + m)
        ref = ref_profiles(centres, pos, UNIT, edges)
        assert ref['margin'] >= 1e-9 and ref['npairs'][0].sum() == m
        res = radial_profiles(pm, centres, pos, edges)
        check_profiles(res, ref, what=(nc, m))
        assert int(cpu(res.npart)[0].sum()) == m


def test_crowded(rbe):
    """3000 sources in one cell about 60 centres inside it: the histogram of a wave under contention, in six bins
    (sixteen copies); two launches give identical npart; with lattice rows and dyadic weights every sum of mass is
    exact"""
    ref = reference('crowded')
    assert ref['npairs'][:60].sum() > 100000
    a, b = run_case(rbe, 'crowded'), run_case(rbe, 'crowded')
    check_profiles(a, ref)
    check_profiles(b, ref)
    assert torch.equal(a.npart, b.npart)
    pos = 0.5 + (lattice_rows(3000, 3, 51) - 0.5) * 2.0 ** -5
    centres = pos[:40].copy()
    m, w = dyadic_weights(3000, 52), dyadic_weights(40, 53)
    e = numpy.array([0.0, 1 / 128., 1 / 64., 1 / 32.])
    check_profiles(radial_profiles(mesh(UNIT), centres, pos, e, mass=m, weight=w),
                   ref_profiles(centres, pos, UNIT, e, mass=m, weight=w), exact_w=True)


@pytest.mark.parametrize('name', ['bins-1', 'bins-8', 'bins-9', 'bins-128', 'bins-129', 'bins-256', 'bins-16x16',
                                  'bins-2x128', 'bins-1x129', 'edges-above-0', 'clustered', 'weights', 'projected'])
def test_random_cases(rbe, name):
    """1, 8 and 9 bins (the linear walk over the edges and the bisection), 128 and 129 (edges in LDS and in global
    memory), 256 = PMX_PAIRS_ROWS_MAX_BINS (one copy of the histogram); the projected mode with nr * npi = 256 as 16 x
    16 and 2 x 128, and with 129 pi edges; edges[0] > 0; clustered rows about their blobs; weights on both sides"""
    res = run_case(rbe, name)
    kw = RANDOM[name]
    nr = len(kw['edges']) - 1
    nc = len(kw['centres'])
    assert tuple(res.npart.shape) == ((nc, nr) if kw.get('mode', '1d') == '1d' else (nc, nr, len(kw['sub']) - 1))
    if name in ('bins-256', 'bins-16x16', 'bins-2x128'):
        assert res.npart[0].numel() == MAX_BINS == 256
    check_profiles(res, reference(name), what=name)


def test_too_many_bins(obe):
    pm, pos = mesh(UNIT), uniform(50, 3, 1)
    with pytest.raises(ValueError, match='bins'):
        radial_profiles(pm, pos, pos, numpy.linspace(0, 0.2, MAX_BINS + 2))
    with pytest.raises(ValueError, match='bins'):
        radial_profiles(pm, pos, pos, numpy.linspace(0, 0.2, 17), mode='projected', piedges=numpy.linspace(0, 0.1, 18))
    assert tuple(radial_profiles(pm, pos, pos, numpy.linspace(0, 0.2, MAX_BINS + 1)).npart.shape) == (50, 256)


@pytest.mark.gpu
def test_the_entry_refuses_more_than_256_bins(hipbe):
    """257 bins: PMX_EINVAL from the entry itself, in both modes; 256 are taken; the old modes still take 4096"""
    from pmesh_amd.backend import PmxError
    dev = hipbe.device
    pos = torch.from_numpy(uniform(50, 3, 1)).to(dev)
    grid = cell_grid(50, 0.2, UNIT)
    e = lambda n, top: torch.from_numpy(numpy.linspace(0, top, n + 1) ** 2).to(dev)
    with pytest.raises(PmxError):
        local_profiles(hipbe, '1d', 2, pos, pos, None, None, grid, UNIT, e(257, 0.2), None)
    with pytest.raises(PmxError):
        local_profiles(hipbe, 'projected', 2, pos, pos, None, None, grid, UNIT, e(1, 0.1), torch.sqrt(e(257, 0.1)))
    got = local_profiles(hipbe, '1d', 2, pos, pos, None, None, grid, UNIT, e(256, 0.2), None)
    assert tuple(got[0].shape) == (50, 256, 1) and int(got[0][:, 0, 0].sum()) == 50
    assert tuple(pair_counts(mesh(UNIT), pos, numpy.linspace(0, 0.2, 4097)).npairs.shape) == (4096,)


def run_local(be, kw, grid, centres=None, pos=None):
    """local_profiles on a forced grid"""
    dev = be.device
    e = numpy.asarray(kw['edges'], dtype='f8')
    c = torch.from_numpy(kw['centres'] if centres is None else centres).to(dev)
    p = torch.from_numpy(kw['pos'] if pos is None else pos).to(dev)
    return local_profiles(be, kw.get('mode', '1d'), kw.get('los', 2), c, p, None, None, grid, kw['box'],
                          torch.from_numpy(e * e).to(dev), None)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(rbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes (in 3-d, 2-d and 1-d): no source is visited twice by a centre, none is missed"""
    for nd in (3, 2, 1):
        name = 'faces-%dd' % nd
        kw = RANDOM[name]
        assert all(kw['box'][d] / grid[d] >= kw['edges'][-1] for d in range(nd))
        got = run_local(rbe, kw, grid_of(grid, kw['box']))
        assert tuple(got[0].shape) == (len(kw['centres']), 3, 1)
        check_profiles(got, reference(name), what=(name, grid))


def test_open_axes(rbe):
    """a grid that is open along two axes (a rank's block): the centres of the block against all rows"""
    kw = RANDOM['open']
    pos, b = kw['pos'], kw['edges'][-1]
    grid = cell_grid(len(pos), b, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    assert 100 < inside.sum() < 1000
    ref = ref_profiles(pos[inside], pos, UNIT, kw['edges'])
    assert ref['margin'] >= 1e-9 and ref['npairs'].sum() > 100
    check_profiles(run_local(rbe, kw, grid, centres=pos[inside], pos=pos), ref)


@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_row_forms_and_weights(rbe, dtype, form):
    """float64 and float32 rows, contiguous, strided and transposed, numpy arrays as well; weights on either side, on
    both and on neither; lattice rows with dyadic weights give exact sums; the inputs are left as they were"""
    pm = mesh(UNIT)
    c, p = lattice_rows(150, 3, 60).astype(dtype), lattice_rows(700, 3, 61).astype(dtype)
    w, m = dyadic_weights(150, 62), dyadic_weights(700, 63)
    edges = [0.0, 1 / 32., 1 / 16., 3 / 32., 1 / 8.]
    tc, tp = place(c, form, rbe.device), place(p, form, rbe.device)
    before = cpu(tp).copy()
    tw, tm = torch.from_numpy(w.astype(dtype)).to(rbe.device), torch.from_numpy(m.astype(dtype)).to(rbe.device)
    for kw in (dict(), dict(weight=w), dict(mass=m), dict(weight=w, mass=m)):
        dev_kw = {k: (tw if k == 'weight' else tm) for k in kw}
        ref = ref_profiles(c, p, UNIT, edges, **kw)
        check_profiles(radial_profiles(pm, tc, tp, edges, **dev_kw), ref, exact_w=True, what=sorted(kw))
        if form == 'C':
            check_profiles(radial_profiles(pm, c, p, edges, **kw), ref, exact_w=True, what=sorted(kw))
    assert numpy.array_equal(cpu(tp), before)
    ref = ref_profiles(c, p, UNIT, edges, mass=m, weight=w, mode='projected', sub=[0.0, 1 / 16., 1 / 8.], los=0)
    check_profiles(radial_profiles(pm, tc, tp, edges, mass=tm, weight=tw, mode='projected', piedges=[0.0, 1 / 16., 1 / 8.],
                                   los=0), ref, exact_w=True)


@pytest.mark.parametrize('nd', [2, 1])
def test_fewer_dimensions(rbe, nd):
    c, p = uniform(200, nd, 70), uniform(1500, nd, 71)
    m = numpy.random.RandomState(72).uniform(0.5, 1.5, 1500)
    edges = numpy.linspace(0.0, 0.05 if nd == 2 else 0.01, 10)
    ref = ref_profiles(c, p, UNIT[:nd], edges, mass=m)
    assert ref['margin'] >= 1e-9 and ref['npairs'].sum() > 1000
    check_profiles(radial_profiles(mesh(UNIT[:nd]), c, p, edges, mass=m), ref)


# ---- 4. identities with the kernels from before --------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['weights', 'projected', 'clustered'])
def test_rows_sum_to_pair_counts(rbe, name):
    """the sum over the centres of npart is the cross pair_counts of the centres with the sources, exactly, in the 1d
    and the projected mode: the kernels of csrc/pmx_pairs.hip"""
    kw = RANDOM[name]
    mode = kw.get('mode', '1d')
    res = run_case(rbe, name)
    pc = pair_counts(mesh(kw['box']), kw['centres'], kw['edges'], pos2=kw['pos'], mode=mode, piedges=kw.get('sub'),
                     los=kw.get('los', 2))
    assert torch.equal(res.npart.sum(dim=0), pc.npairs) and int(pc.npairs.sum()) > 1000


@pytest.mark.gpu
def test_counts_in_spheres_are_the_neighbours_of_the_short_range_force(hipbe):
    """npart with the edges [0, R], summed over its one bin, is the `neighbours` of short_range_force at r_cut = R
    (0 < r2 < R^2) plus the coincident sources (r2 == 0): the kernel of csrc/pmx_shortrange.hip"""
    from pmesh_amd.shortrange import short_range_force
    rows, blobs = clustered(3000, 31)
    centres = numpy.concatenate([blobs, rows[:500]])
    pm = mesh(UNIT)
    R = 0.04
    res = radial_profiles(pm, centres, rows, [0.0, R])
    _, nb = short_range_force(pm, centres, R / 4, r_cut=R, pos2=rows, neighbours=True)
    coincident = numpy.concatenate([numpy.zeros(len(blobs), dtype='i8'), numpy.ones(500, dtype='i8')])
    assert numpy.array_equal(cpu(res.npart)[:, 0], cpu(nb) + coincident) and int(cpu(nb).sum()) > 10000


# ---- 5. the methods of the result -----------------------------------------------------------------------------------------

def test_result_methods(rbe):
    kw = RANDOM['weights']
    res = run_case(rbe, 'weights')
    e = numpy.asarray(kw['edges'])
    mass = cpu(res.mass)
    assert numpy.array_equal(cpu(res.density()), mass / bin_volumes(e, 3))
    assert res.cumulative().dtype == torch.float64
    assert numpy.allclose(cpu(res.cumulative()), numpy.cumsum(mass, axis=1), rtol=8 * U, atol=0)
    with pytest.raises(ValueError, match='projected'):
        res.sigma()
    with pytest.raises(ValueError, match='projected'):
        res.delta_sigma()
    kw = RANDOM['projected']
    res = run_case(rbe, 'projected')
    e, s = numpy.asarray(kw['edges']), numpy.asarray(kw['sub'])
    mass = cpu(res.mass)
    assert res.piedges.tolist() == s.tolist() and res.los == 0 and res.mode == 'projected'
    assert numpy.array_equal(cpu(res.density()), mass / bin_volumes(e, 3, 'projected', s))
    area = numpy.pi * (e[1:] ** 2 - e[:-1] ** 2)
    sigma = mass.sum(axis=2) / area
    assert numpy.allclose(cpu(res.sigma()), sigma, rtol=8 * U, atol=0)
    inside = numpy.cumsum(mass.sum(axis=2), axis=1) / (numpy.pi * e[1:] ** 2)
    assert numpy.allclose(cpu(res.delta_sigma()), inside - sigma, rtol=0, atol=16 * U * numpy.abs(inside).max())
    assert (cpu(res.delta_sigma())[:, 0] == 0).all()            # the first annulus is the disc
    other = run_case(rbe, 'projected', edges=[0.01, 0.05, 0.08])
    with pytest.raises(ValueError, match='edges'):
        other.delta_sigma()


# ---- 6. spherical-overdensity masses ---------------------------------------------------------------------------------------

def ref_so(cum, edges, delta, rho_ref, nd):
    """the rule of so_masses on the cumulative masses `cum` (nc, nbins): (radius, mass, found, and per centre the
    crossing bin k and D_{k-1}, D_k, for the bound)"""
    R = edges[1:]
    D = cum / (rho_ref * ball_volume(R, nd))
    nc = len(cum)
    radius, mass = numpy.full(nc, numpy.nan), numpy.full(nc, numpy.nan)
    found, where = numpy.zeros(nc, dtype=bool), [None] * nc
    for i in range(nc):
        for k in range(1, len(R)):
            if D[i, k - 1] >= delta and D[i, k] < delta:
                t = (math.log(delta) - math.log(D[i, k - 1])) / (math.log(D[i, k]) - math.log(D[i, k - 1]))
                radius[i] = math.exp(math.log(R[k - 1]) + t * (math.log(R[k]) - math.log(R[k - 1])))
                mass[i] = delta * rho_ref * ball_volume(radius[i], nd)
                found[i], where[i] = True, (k, D[i, k - 1], D[i, k])
                break
    return radius, mass, found, where


def so_bound(where, edges, delta):
    """The relative bound on R_delta between two evaluations of the rule on the same D_{k-1}, D_k (unit masses: the
    cumulative masses are the same integers on both sides; the division by rho_ref V rounds the same way in numpy and
    torch up to 4 ulps of D).  Every log is good to 2 ulps of its value plus the 4 ulps of its argument: an absolute
    error of at most (2 |log x| + 4) U.  t = (log delta - log D0) / (log D1 - log D0) lies in [0, 1]; the errors of
    its numerator and denominator, each the sum of two such terms, divided by |log D1 - log D0|, plus 2 ulps for the
    subtraction and the division, bound its error.  log R = l0 + t (l1 - l0) carries that error times (l1 - l0), 3 ulps
    of |l0| + |l1| for its own operations and logs, and exp turns an absolute error of log R into a relative one of
    R, plus 2 ulps."""
    out = []
    for w in where:
        if w is None:
            out.append(0.0)
            continue
        k, d0, d1 = w
        l0, l1 = math.log(edges[k]), math.log(edges[k + 1])
        logs = 2 * (abs(math.log(d0)) + abs(math.log(d1)) + abs(math.log(delta))) + 12
        dt = 2 * logs * U / abs(math.log(d1) - math.log(d0)) + 2 * U
        out.append(dt * (l1 - l0) + 3 * U * (abs(l0) + abs(l1)) * 2 + 2 * U)
    return numpy.array(out)


@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_so_masses_against_the_restatement(rbe, dtype):
    """clustered rows about their blobs, about some of the rows and about uniform points (most of them in voids, with
    no crossing), unit masses, float64 and float32: found and npart
    exactly, radius and mass within so_bound; and with masses, where the cumulative masses are themselves sums: the
    same rule on the device's own cumulative masses"""
    rows, blobs = clustered(3000, 41)
    rows, centres = rows.astype(dtype), numpy.concatenate([blobs, rows[:200], uniform(50, 3, 45)]).astype(dtype)
    pm = mesh(UNIT)
    delta, rho = 50.0, 3000.0
    so = so_masses(pm, centres, rows, delta, rho, rmin=0.004, rmax=0.2, nbins=24)
    assert isinstance(so, SOResult) and so.radius.dtype == so.mass.dtype == torch.float64 and so.found.dtype == torch.bool
    edges = numpy.concatenate([[0.0], numpy.geomspace(0.004, 0.2, 24)])
    assert numpy.array_equal(so.profile.edges, edges)
    ref = ref_profiles(centres, rows, UNIT, edges)
    assert ref['margin'] >= 1e-9
    check_profiles(so.profile, ref)
    radius, mass, found, where = ref_so(numpy.cumsum(ref['wnpairs'], axis=1), edges, delta, rho, 3)
    assert 20 < found.sum() and (~found).sum() > 0
    assert numpy.array_equal(cpu(so.found), found)
    assert numpy.isnan(cpu(so.radius)[~found]).all() and numpy.isnan(cpu(so.mass)[~found]).all()
    bound = so_bound(where, edges, delta)
    assert (numpy.abs(cpu(so.radius)[found] / radius[found] - 1) <= bound[found]).all()
    assert (numpy.abs(cpu(so.mass)[found] / mass[found] - 1) <= 3 * bound[found] + 4 * U).all()
    assert (cpu(so.radius)[found] > 0.004).all() and (cpu(so.radius)[found] <= 0.2).all()
    # with masses: the rule applied to what the device summed
    m = numpy.random.RandomState(42).uniform(0.5, 1.5, 3000).astype(dtype)
    so = so_masses(pm, centres, rows, delta, rho, mass=m, rmin=0.004, rmax=0.2, nbins=24)
    check_profiles(so.profile, ref_profiles(centres, rows, UNIT, edges, mass=m))
    radius, mass, found, where = ref_so(cpu(so.profile.cumulative()), edges, delta, rho, 3)
    bound = so_bound(where, edges, delta)
    assert numpy.array_equal(cpu(so.found), found) and found.sum() > 20
    assert (numpy.abs(cpu(so.radius)[found] / radius[found] - 1) <= bound[found]).all()


def test_so_masses_by_hand(rbe):
    """one centre with eight sources in each of the four bins [0, .01), [.01, .02), [.02, .04), [.04, .08): M = 8, 16,
    24, 32 and, with rho_ref = 1, D_k = M_k / (4/3 pi R_k^3) = 1.9e6, 4.8e5, 9.0e4, 1.5e4.  delta = 2e5 is crossed
    between R_1 = .02 and R_2 = .04; delta = 1e3 lies below every D_k and delta = 1e7 above: no crossing, nan"""
    rng = numpy.random.RandomState(3)
    centre = numpy.array([[0.3, 0.6, 0.95]])
    v = rng.normal(size=(32, 3))
    v /= numpy.sqrt((v * v).sum(axis=1))[:, None]
    radii = numpy.repeat([0.005, 0.015, 0.03, 0.06], 8) * rng.uniform(0.8, 1.2, size=32)
    pos = (centre + v * radii[:, None]) % 1.0
    pm = mesh(UNIT)
    so = so_masses(pm, centre, pos, 2e5, 1.0, rmin=0.01, rmax=0.08, nbins=4)
    assert so.profile.edges.tolist() == [0.0] + numpy.geomspace(0.01, 0.08, 4).tolist()
    assert cpu(so.profile.npart).tolist() == [[8, 8, 8, 8]] and cpu(so.found).tolist() == [True]
    V = lambda r: 4.0 / 3.0 * numpy.pi * r ** 3
    R1, R2 = so.profile.edges[2], so.profile.edges[3]
    D1, D2 = 16 / V(R1), 24 / V(R2)
    assert abs(R1 - 0.02) < 1e-15 and abs(R2 - 0.04) < 1e-15 and D1 >= 2e5 > D2
    want = math.exp(math.log(R1) + (math.log(2e5) - math.log(D1)) / (math.log(D2) - math.log(D1)) * math.log(R2 / R1))
    assert 0.02 < want < 0.04
    assert abs(cpu(so.radius)[0] / want - 1) <= so_bound([(2, D1, D2)], so.profile.edges, 2e5)[0]
    assert abs(cpu(so.mass)[0] / (2e5 * V(want)) - 1) <= 1e-13
    for delta in (1e3, 1e7):
        so = so_masses(pm, centre, pos, delta, 1.0, rmin=0.01, rmax=0.08, nbins=4)
        assert cpu(so.found).tolist() == [False] and numpy.isnan(cpu(so.radius)).all() and numpy.isnan(cpu(so.mass)).all()
    # the defaults: rmax = L / 4, rmin = rmax / 1000, 64 bins
    so = so_masses(pm, centre, pos, 200.0, 32.0)
    assert len(so.profile.edges) == 65 and so.profile.edges[-1] == 0.25 and abs(so.profile.edges[1] - 0.25e-3) < 1e-18
    for kw in (dict(nbins=1), dict(nbins=257), dict(rmin=0.3), dict(rmax=0.6), dict(nbins=2.5)):
        with pytest.raises(ValueError):
            so_masses(pm, centre, pos, 200.0, 32.0, **kw)
    for delta, rho in ((0.0, 1.0), (200.0, -1.0), (numpy.nan, 1.0)):
        with pytest.raises(ValueError):
            so_masses(pm, centre, pos, delta, rho)


def test_halo_catalogue_centres(rbe):
    """the use the module is for: profiles and M_200 about the CMPosition of fof_catalog"""
    from pmesh_amd.fof import fof, fof_catalog
    rows, _ = clustered(3000, 43)
    m = numpy.random.RandomState(44).uniform(0.5, 1.5, 3000)
    pm = mesh(UNIT)
    cat = fof_catalog(pm, rows, fof(pm, rows, 0.01, nmin=20), mass=m)
    centres = cpu(cat.CMPosition)
    assert 4 <= len(centres) <= 20
    edges = numpy.geomspace(0.003, 0.1, 9)
    res = radial_profiles(pm, cat.CMPosition, rows, edges, mass=m)
    check_profiles(res, ref_profiles(centres, rows, UNIT, edges, mass=m))
    so = so_masses(pm, cat.CMPosition, rows, 200, m.sum(), mass=m)
    check_profiles(so.profile, ref_profiles(centres, rows, UNIT, so.profile.edges, mass=m))
    assert cpu(so.found)[1:].sum() >= 3 and tuple(so.radius.shape) == (len(centres),)


# ---- 7. arguments ----------------------------------------------------------------------------------------------------------

def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    c = pos[:10]
    for edges in ([0.1], [0.2, 0.1], [-0.1, 0.1], [0.0, numpy.nan], [[0.0, 0.1]]):
        with pytest.raises(ValueError, match='edges'):
            radial_profiles(pm, c, pos, edges)
    with pytest.raises(ValueError, match='separation'):
        radial_profiles(pm, c, pos, [0.0, 0.51])
    # the search radius of the projected mode is hypot(edges[-1], piedges[-1])
    with pytest.raises(ValueError, match='separation'):
        radial_profiles(pm, c, pos, [0.0, 0.4], mode='projected', piedges=[0.0, 0.4])
    assert tuple(radial_profiles(pm, c, pos, [0.0, 0.3], mode='projected', piedges=[0.0, 0.4]).npart.shape) == (10, 1, 1)
    with pytest.raises(ValueError, match='shape'):
        radial_profiles(pm, c[:, :2], pos, [0.0, 0.1])
    with pytest.raises(ValueError, match='shape'):
        radial_profiles(pm, c, pos.reshape(-1), [0.0, 0.1])
    with pytest.raises(TypeError):
        radial_profiles(pm, c, (pos * 100).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='weight'):
        radial_profiles(pm, c, pos, [0.0, 0.1], weight=numpy.ones(50))
    with pytest.raises(ValueError, match='mass'):
        radial_profiles(pm, c, pos, [0.0, 0.1], mass=numpy.ones(10))
    for mode in ('2d', 'angular'):
        with pytest.raises(ValueError, match='mode'):
            radial_profiles(pm, c, pos, [0.0, 0.1], mode=mode)
    with pytest.raises(ValueError, match='three dimensions'):
        radial_profiles(mesh(UNIT[:2]), c[:, :2], pos[:, :2], [0.0, 0.1], mode='projected', pimax=1)
    with pytest.raises(ValueError, match='los'):
        radial_profiles(pm, c, pos, [0.0, 0.1], mode='projected', piedges=[0.0, 0.1], los=3)
    with pytest.raises(ValueError, match='needs'):
        radial_profiles(pm, c, pos, [0.0, 0.1], mode='projected')
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    with pytest.raises(ValueError, match='2 rows'):
        radial_profiles(pm, bad[5:9], bad, [0.0, 0.1])
    with pytest.raises(NotImplementedError):
        radial_profiles(mesh([1.0] * 4), numpy.zeros((3, 4)), numpy.zeros((3, 4)), [0.0, 0.1])


# ---- 8. ranks --------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """radial_profiles on thread ranks holding centres and sources split unevenly (one rank holds none): what every
    rank got for its own centres"""
    kw = RANDOM[name]
    c, p, w, m = kw['centres'], kw['pos'], kw.get('weight'), kw.get('mass')
    s1, s2 = split(len(c), size), split(len(p), size)[::-1]

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a, b = s1[comm.rank], s2[comm.rank]
        res = radial_profiles(pm, c[a], p[b], kw['edges'], mass=None if m is None else m[b],
                              weight=None if w is None else w[a], mode=kw.get('mode', '1d'), piedges=kw.get('sub'))
        return cpu(res.npart), cpu(res.mass), cpu(res.rsum), len(c[a])
    return thread_ranks(size, body), s1


def check_ranks(name, size, np_):
    results, s1 = ranks_case(name, size, np_)
    ref = reference(name)
    assert ref['margin'] >= 1e-9
    sizes = [results[r][3] for r in range(size)]
    assert 0 in sizes and len(set(sizes)) > 1
    nbins = ref['npairs'].shape[1]
    for r in range(size):
        part = {k: ref[k][s1[r]] for k in ('npairs', 'wnpairs', 'rsum')}
        assert results[r][0].shape[0] == sizes[r] and int(numpy.prod(results[r][0].shape[1:])) == nbins
        check_profiles(results[r][:3], part, what=(name, size, r))


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_profiles(obe, size, np_):
    """weighted profiles at b = 0.1 in the unit box, and projected ones on the box [1, 0.5, 0.25]: every rank gets, for
    its own centres in its own order, the rows of the restatement of all rows; npart exactly"""
    for name in ('ranks', 'ranks-slab'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    for name in ('ranks', 'ranks-slab'):
        check_ranks(name, size, np_)


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank: a wrong shape, a wrong type, a coordinate that is not finite,
    2 b > L, a mass of the wrong length, too many bins, a bad overdensity"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        c = mine[:5]
        edges = [0.0, 0.05]
        with pytest.raises(ValueError):
            radial_profiles(pm, c[:, :2] if comm.rank == 1 else c, mine, edges)
        with pytest.raises(TypeError):
            radial_profiles(pm, c, (mine * 8).astype('i8') if comm.rank == 2 else mine, edges)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            radial_profiles(pm, c, bad, edges)
        with pytest.raises(ValueError):
            radial_profiles(pm, c, mine, [0.0, 0.6 if comm.rank == 1 else 0.05])
        with pytest.raises(ValueError):
            radial_profiles(pm, c, mine, edges, mass=numpy.ones(29 if comm.rank == 1 else 30))
        with pytest.raises(ValueError):
            radial_profiles(pm, c, mine, numpy.linspace(0, 0.05, MAX_BINS + (2 if comm.rank == 2 else 1)))
        with pytest.raises(ValueError):
            so_masses(pm, c, mine, -1.0 if comm.rank == 0 else 200.0, 90.0)
        got = cpu(radial_profiles(pm, c, mine, edges).npart)
        want = ref_profiles(c, pos, UNIT, edges)['npairs']
        assert numpy.array_equal(got, want)
        so = so_masses(pm, c, mine, 20.0, 90.0)
        assert tuple(so.radius.shape) == (5,)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 9. more secondaries than one launch takes -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_more_secondaries_than_one_launch_accumulates(hipbe):
    """2^23 + 5000 sources and 8 centres: the entry launches once per window of 2^23 slots of the sources and the second
    launch adds to what the first left.  Four of the centres sit in the cell that holds slot 2^23, which is split
    between the two launches.  No brute force at this size: the profiles against all sources equal, exactly, the sum of
    the profiles against their two halves (each within one launch), after tests.test_paircount's
    test_more_secondaries_than_one_launch_counts"""
    n2 = (1 << 23) + 5000
    dev = hipbe.device
    gen = torch.Generator(device=dev).manual_seed(5)
    p2 = torch.rand((n2, 3), generator=gen, device=dev, dtype=torch.float64)
    edges = numpy.linspace(0.0, 0.02, 5)
    # the grid radial_profiles lays, and in it the cell of slot 2^23
    grid = cell_grid(n2, 0.02, UNIT)
    _, _, cell_start, _, _, _ = cell_sort(hipbe, p2, grid, UNIT)
    cell = int(torch.searchsorted(cell_start.to(torch.int64), torch.tensor([1 << 23], device=dev), right=True)[0]) - 1
    lo, hi = int(cell_start[cell]), int(cell_start[cell + 1])
    assert lo < (1 << 23) < hi
    axes = numpy.array(numpy.unravel_index(cell, grid[0]), dtype='f8')
    middle = (axes + 0.5) / numpy.asarray(grid[2])
    offsets = numpy.array([[0, 0, 0], [0.2, -0.1, 0.3], [-0.3, 0.2, -0.2], [0.1, 0.3, 0.1]]) / numpy.asarray(grid[2])
    centres = torch.from_numpy(numpy.concatenate([middle + offsets, uniform(4, 3, 9)])).to(dev)
    pm = mesh(UNIT)
    whole = radial_profiles(pm, centres, p2, edges)
    half = n2 // 2
    parts = [radial_profiles(pm, centres, p2[:half], edges), radial_profiles(pm, centres, p2[half:], edges)]
    assert torch.equal(whole.npart, parts[0].npart + parts[1].npart)
    assert torch.equal(whole.mass, parts[0].mass + parts[1].mass)          # (unit masses: sums of integers)
    n = cpu(whole.npart)
    assert n.sum() > 1500 and (n.sum(axis=1) > 100).all()
    # and against the expectation of uniform rows, to a few standard deviations of the count
    want = 8 * n2 * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert (numpy.abs(n.sum(axis=0) - want) < 6 * numpy.sqrt(want)).all()


# ---- 10. streams -----------------------------------------------------------------------------------------------------------

def profiles_stream_case(be, mode):
    from tests import stream_cases as S

    class Profiles(S.Case):
        """pmx_pair_counts in the two row modes (profiles.local_profiles: the cell sorts and the kernel of
        pmx_pairs_rows.hip) with weights on both sides on lattice rows: npairs and wnpairs exact; rsum within the bound
        of tests/stream_cases.py's Pairs"""
        entries = ('pmx_fof_cells', 'pmx_fof_fill', 'pmx_pair_counts')
        name = 'profiles-' + mode

        def __init__(self):
            S.Case.__init__(self, be)
            edges = numpy.linspace(0.0, 0.1, 9)
            self.e2 = self.t(edges * edges)
            self.sub = self.t(numpy.linspace(0.0, 0.1, 5)) if mode == 'projected' else None
            b = float(numpy.hypot(0.1, 0.1)) * (1 + 1e-15) if mode == 'projected' else 0.1
            self.grid = cell_grid(S.NPART, b, S.UNIT_BOX)

        def make(self, seed):
            return [self.t(S.lattice_rows(seed, 50, 512)), self.t(S.dyadic(seed, 51, 512)),
                    self.t(S.lattice_rows(seed, 52)), self.t(S.dyadic(seed, 53))]

        def run(self, ins):
            return list(local_profiles(self.be, mode, 2, ins[0], ins[2], ins[1], ins[3], self.grid, S.UNIT_BOX,
                                       self.e2, self.sub))

        def bound(self):
            def f(want):
                M = S.host(want[0]).astype('f8')
                return [numpy.zeros(M.shape), numpy.zeros(M.shape), 2 * (M + 4) * U * numpy.abs(S.host(want[2]))]
            return f
    return Profiles()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['1d', 'projected'])
def test_delayed_producer(hipbe, mode):
    """the delayed producer of tests/test_streams.py on the new launch path, with its power conditions (after
    tests/test_surveypairs.py): the kernels of pmx_pairs_rows.hip run on the caller's stream, and the entry returns
    without waiting for it"""
    from tests import test_streams as T
    assert T.streams_are_unordered(), 'mechanism 1 has no power on this runtime (see tests/test_streams.py)'
    sleep = T.delay()
    case = profiles_stream_case(hipbe, mode)
    real, want, bounds = T.reference(case)
    inputs = case.make(2)
    decoy_out = T.keep(case.run(inputs))
    torch.cuda.synchronize()
    total, differ, _ = T.differences(decoy_out, want, bounds, factor=100.0)
    assert total > 0 and 2 * differ > total, \
        'power condition: the decoy inputs change only %d of %d output elements by more than 100 bounds' % (differ, total)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        sleep()
        case.load(inputs, real)
        e_fill = torch.cuda.Event()
        e_fill.record(s)
        early = e_fill.query()
        got = case.run(inputs)
        returned_early = e_fill.query()
        got = T.keep(got)
    s.synchronize()
    assert not early, 'power condition: the delay had run out before the operation was called'
    T.assert_same(case, got, want, bounds, 'behind a delayed copy on a side stream')
    assert case.host_async and not returned_early, \
        'pmx_pair_counts returned only after the delayed copy in front of it had completed: it waits for the stream'
    # and the profiles are those of the restatement
    c, w, p, m = [cpu(x) for x in real]
    ref = profile_core(c, p, numpy.ones(3), mode, 2, cpu(case.e2), None if case.sub is None else cpu(case.sub), w, m)
    check_profiles(want, ref, exact_w=True)


# ---- 11. the ABI and the resources ---------------------------------------------------------------------------------------

def test_the_modes_are_bound():
    assert (_abi.PMX_PAIRS_1D_ROWS, _abi.PMX_PAIRS_PROJECTED_ROWS, _abi.PMX_PAIRS_ROWS_MAX_BINS) == (5, 6, 256)
    assert ROW_MODES == {'1d': 5, 'projected': 6} and MAX_BINS == 256
    assert (_abi.PMX_PAIRS_1D, _abi.PMX_PAIRS_2D, _abi.PMX_PAIRS_PROJECTED) == (0, 1, 2)
    for name in ('radial_profiles', 'so_masses'):
        assert name in pmesh_amd.__doc__
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'pmesh_amd.h')).read()
    assert '(i * nr + rbin) * nsub + subbin' in header


def test_rows_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs_rows.hip')
    # rows_kernel<NDIM, MODE, WEIGHTED>: the mode 1d for 1 to 3 dimensions, the projected mode for 3; without and with
    # weights
    assert len(t) == 8 and all('rows_kernel' in k for k in t), sorted(t)
    for nd, mode in ((1, 5), (2, 5), (3, 5), (3, 6)):
        assert len([k for k in t if 'rows_kernelILi%dELi%dE' % (nd, mode) in k]) == 2, sorted(t)
    for name, r in t.items():
        weighted, projected = 'Lb1E' in name, 'Li6E' in name
        assert r['ScratchSize'] == 0, (name, r)
        # RWAVES histograms of 256 slots: a 32-bit count and a double (weighted: two doubles) per slot; the squared
        # edges of r and, in the projected mode, the edges of pi: 129 doubles each; and up to 16 bytes for the
        # placeholders of the arrays a variant does not use
        lds = RWAVES * 256 * (20 if weighted else 12) + 129 * 8 * (2 if projected else 1) + 16
        assert r['LDS'] <= lds <= 23 * 1024, (name, r, lds)
        # the full 8 waves per SIMD.  Measured at compile time: 38 to 42 VGPRs without weights, 56 with
        assert r['VGPRs'] <= 64, (name, r)
