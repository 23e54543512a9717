"""pmesh_amd.surveypairs (csrc/pmx_pairs_survey.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/surveypairs.py, include/pmesh_amd.h).  Everything of tests/test_paircount.py stays: double
arithmetic with every operation rounded once, squared edges e2[k] = edges[k] * edges[k], no square root choosing a bin,
exact npairs, double sums in no particular order.  The new parts.  The kernel knows one observer, the centre of the box,
o_d = L_d / 2.  For a pair of wrapped rows w_i, w_j: dx_d is the minimum image as before; l_d = (w_i,d + w_j,d) - L_d,
two roundings (twice the midpoint's offset from the observer); p = dx_0 l_0 + dx_1 l_1 + dx_2 l_2, l2 = l_0^2 + l_1^2 +
l_2^2, r2 = dx_0^2 + dx_1^2 + dx_2^2, each sum in that order; p2 = p * p.
PMX_PAIRS_2D_MIDPOINT (3), bins of (s, mu): the r-bin from q = r2; t = r2 * l2; the mu-bin is the number of k in
1 .. nsub - 1 with p2 >= sub[k] * t, sub[k] = muedges[k]^2; t == 0 goes to mu-bin 0.
PMX_PAIRS_PROJECTED_MIDPOINT (4), bins of (rp, pi): pi2 = p2 / l2, or 0 where l2 == 0; rp2 = r2 - pi2, or 0 where that
is negative; the r-bin from q = rp2 against e2; sub[k] = piedges[k]^2, squared on the host; the pi-bin is the number of
k in 1 .. nsub - 1 with pi2 >= sub[k]; pi2 >= sub[nsub] is not counted; rsum adds w sqrt(rp2).
Both ignore los, need three dimensions and are symmetric under exchanging the two rows.  The host layer requires every
row in [b / 2, L_d - b / 2) after the shift x' = (double)x + (L_d / 2 - observer_d): b = edges[-1], in the projected
mode hypot(edges[-1], piedges[-1]) rounded up; no counted pair is then a wrapped one.  The angular mode puts the rows
on a sphere of radius R = min_d L_d / (2 + 2 sin(theta_max / 2)) (1 - 2^-30) about the box centre, u = (x - observer) /
|x - observer|, and counts them in 1d with e2[k] = (2 R sin(theta_k / 2))^2; rsum is divided by R on the host.

The restatement is brute force, the same operations in the same order on the full (n1, n2) matrices; it extends
count_core of tests/test_paircount.py.  Under -m "not gpu" it serves the two new modes of pmx_pair_counts
(SurveyOracleBackend), so the host layer and the thread ranks run without a GPU; under -m gpu the kernel is compared
with it.

npairs is compared by exact equality everywhere; wnpairs and rsum by the bounds of tests/test_paircount.py (check):
|got - ref| <= (M + 4) 2^-52 S, exact wnpairs on lattice rows with dyadic weights.  No tolerance is introduced here.

The condition on random inputs (test_inputs_are_decided, no GPU): no pair with |q - e2[k]| < 1e-9 e2[k], |p2 - sub[k] t|
< 1e-9 t or |pi2 - sub[k]| < 1e-9 sub[k] (sub[k] > 0); the seeds are chosen so that it holds.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid
from pmesh_amd.paircount import local_counts, pair_counts
from pmesh_amd.surveypairs import (SurveyPairCounts, angular_radius, sky_to_cartesian, survey_correlation,
                                   survey_pair_counts, to_poles, to_wp)
from tests import stream_cases as S
from tests.test_fof import RANKS, ROW_FORMS, UNIT, WAVE_NS, mesh, place, split, thread_ranks, wrap
from tests.test_lpt import cpu
from tests.test_paircount import U, PairsOracleBackend, check, count_core, dyadic_weights

C2D, CPROJ = 3, 4
KERNEL = {'2d': '2d-midpoint', 'projected': 'projected-midpoint'}


# ---- the restatement -----------------------------------------------------------------------------------------------

def survey_core(w1, w2, box, mode, e2, sub, wt1=None, wt2=None, skip_diagonal=False):
    """The sums over the pairs of the wrapped rows w1 with w2 in the mode '2d-midpoint' or 'projected-midpoint'.  e2:
    the squared edges; sub: muedges^2 or piedges^2.  Returns a dict: npairs, wnpairs, rsum (flat), margin (the smallest
    relative distance of a pair from a deciding comparison, by the three measures of the module docstring)."""
    n1, n2 = len(w1), len(w2)
    nr, nsub = len(e2) - 1, len(sub) - 1
    nbins = nr * nsub
    out = dict(npairs=numpy.zeros(nbins, dtype='i8'), wnpairs=numpy.zeros(nbins), rsum=numpy.zeros(nbins),
               margin=numpy.inf)
    if n1 == 0 or n2 == 0:
        return out
    dx, l = [], []
    for d in range(3):
        x = w1[:, None, d] - w2[None, :, d]
        dx.append(x - box[d] * numpy.rint(x / box[d]))
        l.append((w1[:, None, d] + w2[None, :, d]) - box[d])
    r2 = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]
    p = dx[0] * l[0] + dx[1] * l[1] + dx[2] * l[2]
    l2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2]
    p2 = p * p
    sbin = numpy.zeros((n1, n2), dtype='i8')
    margin = numpy.inf
    if mode == '2d-midpoint':
        q = r2
        keep = (q >= e2[0]) & (q < e2[-1])
        t = r2 * l2
        some = keep & (t > 0)
        for k in range(1, nsub):
            st = sub[k] * t
            sbin += p2 >= st
            if some.any():
                margin = min(margin, float((numpy.abs(p2 - st)[some] / t[some]).min()))
        sbin[t == 0] = 0
    else:
        with numpy.errstate(invalid='ignore', divide='ignore'):
            pi2 = numpy.where(l2 == 0, 0.0, p2 / numpy.where(l2 == 0, 1.0, l2))
        q = r2 - pi2
        q = numpy.where(q < 0, 0.0, q)
        keep = (q >= e2[0]) & (q < e2[-1])
        for k in range(1, nsub + 1):
            if k < nsub:
                sbin += pi2 >= sub[k]
            if keep.any() and sub[k] > 0:
                margin = min(margin, float((numpy.abs(pi2 - sub[k])[keep] / sub[k]).min()))
        keep &= pi2 < sub[-1]
    if skip_diagonal:
        keep &= ~numpy.eye(n1, n2, dtype=bool)
    rbin = numpy.searchsorted(e2, q, side='right') - 1
    pe = e2[e2 > 0]
    for shift in (1, 0):
        near = pe[numpy.clip(numpy.searchsorted(pe, q) - shift, 0, len(pe) - 1)]
        margin = min(margin, float((numpy.abs(q - near) / near).min()))
    w = numpy.ones((n1, n2))
    if wt1 is not None:
        w = w * numpy.asarray(wt1).astype('f8').reshape(-1)[:, None]
    if wt2 is not None:
        w = w * numpy.asarray(wt2).astype('f8').reshape(-1)[None, :]
    flat = (rbin * nsub + sbin)[keep]
    out['npairs'] = numpy.bincount(flat, minlength=nbins).astype('i8')
    out['wnpairs'] = numpy.bincount(flat, weights=w[keep], minlength=nbins)
    out['rsum'] = numpy.bincount(flat, weights=(w * numpy.sqrt(q))[keep], minlength=nbins)
    out['margin'] = margin
    return out


def shifted(pos, box, observer):
    """the rows of the rule: x' = (double)x + (L / 2 - observer)"""
    x = numpy.asarray(pos).astype('f8')
    if observer is None:
        return x
    return x + (numpy.asarray(box, dtype='f8') / 2 - numpy.asarray(observer, dtype='f8'))


def ref_survey(pos1, box, edges, pos2=None, w1=None, w2=None, mode='1d', sub=None, observer=None):
    """the restatement of survey_pair_counts(mesh(box), pos1, edges, observer, pos2, w1, w2, mode, muedges / piedges =
    sub) in the modes 1d, 2d and projected"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    a = wrap(shifted(pos1, box, observer), box)
    auto = pos2 is None
    b = a if auto else wrap(shifted(pos2, box, observer), box)
    if mode == '1d':
        out = count_core(a, b, box, '1d', 2, e * e, None, w1, w1 if auto else w2, skip_diagonal=auto)
    else:
        s = numpy.asarray(sub, dtype='f8')
        out = survey_core(a, b, box, KERNEL[mode], e * e, s * s, w1, w1 if auto else w2, skip_diagonal=auto)
    out['nself'], out['wself'] = 0, 0.0
    if auto and e[0] == 0:
        out['nself'] = len(a)
        out['wself'] = float(len(a)) if w1 is None else float((numpy.asarray(w1).astype('f8') ** 2).sum())
    return out


def sphere_rows(pos, box, observer, R):
    x = numpy.asarray(pos).astype('f8')
    box = numpy.asarray(box, dtype='f8')
    d = x - (box / 2 if observer is None else numpy.asarray(observer, dtype='f8'))
    norm = numpy.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return box / 2 + R * (d / norm[:, None])


def ref_angular(pos1, box, thetaedges, pos2=None, w1=None, w2=None, observer=None):
    """the restatement of the chord rule of the angular mode"""
    box = numpy.asarray(box, dtype='f8')
    th = numpy.asarray(thetaedges, dtype='f8')
    R = angular_radius(list(box), th[-1])
    chord = 2 * R * numpy.sin(numpy.radians(th) / 2)
    a = wrap(sphere_rows(pos1, box, observer, R), box)
    auto = pos2 is None
    b = a if auto else wrap(sphere_rows(pos2, box, observer, R), box)
    out = count_core(a, b, box, '1d', 2, chord * chord, None, w1, w1 if auto else w2, skip_diagonal=auto)
    out['rsum'] = out['rsum'] / R
    out['nself'], out['wself'] = 0, 0.0
    if auto and th[0] == 0:
        out['nself'] = len(a)
        out['wself'] = float(len(a)) if w1 is None else float((numpy.asarray(w1).astype('f8') ** 2).sum())
    return out


class SurveyOracleBackend(PairsOracleBackend):
    """the CPU test double with the two midpoint modes of pmx_pair_counts served by the restatement"""
    name = 'oracle-surveypairs'

    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        if mode not in (C2D, CPROJ):
            return PairsOracleBackend.pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2,
                                                  cell_start2, weight2, ncell, periodic, boxsize, e2, sub, npairs,
                                                  wnpairs, rsum)
        n1, n2 = spos1.shape[0], spos2.shape[0]
        if n1 == 0 or n2 == 0:
            return
        assert spos1.shape[1] == 3 and cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        a, b = numpy.empty((n1, 3)), numpy.empty((n2, 3))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = survey_core(a, b, numpy.asarray(boxsize, dtype='f8'), '2d-midpoint' if mode == C2D else
                          'projected-midpoint', e2.numpy(), sub.numpy(), None if weight1 is None else weight1.numpy(),
                          None if weight2 is None else weight2.numpy())
        npairs += torch.from_numpy(got['npairs'])
        wnpairs += torch.from_numpy(got['wnpairs'])
        rsum += torch.from_numpy(got['rsum'])


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(SurveyOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def sbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(SurveyOracleBackend())
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

# seeds moved on where the first choice left a pair within 1e-9 of a deciding comparison (test_inputs_are_decided)
BUMP = {}


def interior(n, seed, b, box=UNIT, dtype='f8'):
    """n uniform rows of the padded interior [b / 2, L - b / 2) of the box (a hair inside it: float32 rows round)"""
    box = numpy.asarray(box, dtype='f8')
    u = numpy.random.RandomState(seed).uniform(size=(n, 3))
    return (b / 2 + (0.001 + 0.998 * u) * (box - b)).astype(dtype)


def wave_b(n1, n2):
    return min(0.45, 0.6 * max(n1, n2, 1) ** (-1 / 3.))


def wave_binning(n1, n2, mode):
    """(edges, sub edges, b)"""
    b = wave_b(n1, n2)
    if mode == '2d':
        return numpy.array([0.0, 0.4 * b, 0.8 * b, b]), numpy.array([0.0, 0.3, 0.7, 1.0]), b
    s = b / 1.5
    return numpy.array([0.0, 0.4 * s, 0.8 * s, s]), numpy.array([0.0, 0.5 * s, s]), float(numpy.hypot(s, s)) * (1 + 1e-15)


def wave_case(n1, n2, dtype, mode):
    edges, sub, b = wave_binning(n1, n2, mode)
    name = 'wave-%d-%d-%s-%s' % (n1, n2, dtype, mode)
    return (interior(n1, 300 + n1 + 5000 * BUMP.get(name, 0), b, dtype=dtype),
            interior(n2, 500 + n2 + 5000 * BUMP.get(name, 0), b, dtype=dtype), edges, sub)


BOUNDARY = {'8x128': (8, 128), '5x205': (5, 205), '7x129': (7, 129), '129x4': (129, 4), '40x100': (40, 100)}


def boundary_case(shape, mode):
    """400 rows, 300 more for the cross form, weights; the bins of BOUNDARY"""
    nr, nsub = BOUNDARY[shape]
    name = 'bins-%s-%s' % (shape, mode)
    bump = 5000 * BUMP.get(name, 0)
    if mode == '2d':
        edges, sub, b = numpy.linspace(0.0, 0.3, nr + 1), numpy.linspace(0.0, 1.0, nsub + 1), 0.3
    else:
        edges, sub = numpy.linspace(0.0, 0.2, nr + 1), numpy.linspace(0.0, 0.2, nsub + 1)
        b = float(numpy.hypot(0.2, 0.2)) * (1 + 1e-15)
    return dict(pos1=interior(400, 38 + bump, b), pos2=interior(300, 39 + bump, b), box=UNIT, edges=edges, sub=sub,
                mode=mode, w1=numpy.random.RandomState(3).uniform(0.5, 1.5, 400),
                w2=numpy.random.RandomState(4).uniform(0.5, 1.5, 300))


def random_cases():
    """name -> keyword arguments of ref_survey: every random input of the tests below"""
    cases = {}
    for mode in ('2d', 'projected'):
        for dtype in ('f8', 'f4'):
            for n1 in WAVE_NS:
                for n2 in WAVE_NS:
                    p1, p2, e, s = wave_case(n1, n2, dtype, mode)
                    cases['wave-%d-%d-%s-%s' % (n1, n2, dtype, mode)] = dict(pos1=p1, pos2=p2, box=UNIT, edges=e, sub=s,
                                                                             mode=mode)
                    if n1 == n2:
                        cases['wave-auto-%d-%s-%s' % (n1, dtype, mode)] = dict(pos1=p1, box=UNIT, edges=e, sub=s,
                                                                               mode=mode)
        for shape in BOUNDARY:
            kw = boundary_case(shape, mode)
            cases['bins-%s-%s' % (shape, mode)] = kw
            cases['bins-%s-%s-auto' % (shape, mode)] = dict(kw, pos2=None, w2=None, w1=None)
    b = 0.1
    rows = interior(900, 44, numpy.hypot(b, b) * 1.001)
    more = interior(700, 45, numpy.hypot(b, b) * 1.001)
    w1, w2 = numpy.random.RandomState(7).uniform(0.5, 1.5, 900), numpy.random.RandomState(8).uniform(0.5, 1.5, 700)
    cases['ranks-2d'] = dict(pos1=rows, pos2=more, box=UNIT, edges=numpy.linspace(0, b, 5), mode='2d',
                             sub=[0.0, 0.3, 0.8, 1.0], w1=w1, w2=w2)
    cases['ranks-projected'] = dict(pos1=rows, box=UNIT, edges=numpy.linspace(0, b, 4), mode='projected',
                                    sub=[0.0, 0.03, 0.06, 0.1], w1=w1)
    cases['ranks-1d'] = dict(pos1=rows - 0.02, box=UNIT, edges=numpy.linspace(0, b, 5), mode='1d',
                             observer=[0.48, 0.48, 0.48])
    cases['uniform'] = dict(pos1=interior(700, 31, 0.12), box=UNIT, edges=numpy.linspace(0, 0.12, 7), mode='2d',
                            sub=numpy.linspace(0, 1, 6))
    cases['uniform-1d'] = dict(cases['uniform'], mode='1d', sub=None)
    cases['cross'] = dict(pos1=interior(700, 32, 0.15), pos2=interior(500, 33, 0.15), box=UNIT,
                          edges=[0.01, 0.015, 0.04, 0.1], mode='projected', sub=[0.0, 0.02, 0.05, 0.1],
                          w1=dyadic_weights(700, 1), w2=dyadic_weights(500, 2))
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_survey(**RANDOM[name])
    return _REFERENCE[name]


def tensor(x, dev):
    return None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)


def run(be, kw, **over):
    """survey_pair_counts of the keyword arguments of ref_survey on one rank"""
    kw = dict(kw, **over)
    mode, sub = kw.get('mode', '1d'), kw.get('sub')
    return survey_pair_counts(mesh(kw['box']), tensor(kw['pos1'], be.device), kw['edges'],
                              observer=kw.get('observer'), pos2=tensor(kw.get('pos2'), be.device),
                              weight1=tensor(kw.get('w1'), be.device), weight2=tensor(kw.get('w2'), be.device),
                              mode=mode, muedges=sub if mode == '2d' else None,
                              piedges=sub if mode == 'projected' else None)


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_on_known_answers():
    """three pairs about the observer of the unit box, each counted twice: along a ray (mu = 1, pi = r), across it
    (mu = 0, pi = 0) and symmetric about the observer (l2 == 0: mu-bin 0, pi2 = 0, rp2 = r2)"""
    o = numpy.array([0.5, 0.5, 0.5])
    v = numpy.array([1.0, 2.0, 2.0]) / 64
    radial = numpy.stack([o + 4 * v, o + 6 * v])                                   # r = 6 / 64
    across = numpy.stack([o + [0.25, 1 / 32., 0], o + [0.25, -1 / 32., 0]])        # r = 1 / 16, p == 0
    mirror = numpy.stack([o + v, o - v])                                           # r = 6 / 64, l == 0
    edges, mu = [0.0, 0.05, 0.1], [0.0, 0.5, 1.0]
    for rows, want in ((radial, [0, 0, 0, 2]), (across, [0, 0, 2, 0]), (mirror, [0, 0, 2, 0])):
        assert ref_survey(rows, UNIT, edges, mode='2d', sub=mu)['npairs'].tolist() == want
    pi = [0.0, 0.05, 0.1]
    for rows, want in ((radial, [0, 2, 0, 0]), (across, [0, 0, 2, 0]), (mirror, [0, 0, 2, 0])):
        got = ref_survey(rows, UNIT, edges, mode='projected', sub=pi)
        assert got['npairs'].tolist() == want
    assert ref_survey(radial, UNIT, edges, mode='projected', sub=pi)['rsum'].tolist() == [0.0] * 4     # rp == 0 exactly
    assert ref_survey(mirror, UNIT, edges, mode='projected', sub=pi)['rsum'][2] == 2 * 6 / 64.
    # an observer elsewhere: the same rows moved with it
    moved = ref_survey(radial + 0.125, [2.0, 2.0, 2.0], edges, mode='2d', sub=mu, observer=o + 0.125)
    assert moved['npairs'].tolist() == [0, 0, 0, 2]


GROUPS = ['wave-f8-2d', 'wave-f4-2d', 'wave-f8-projected', 'wave-f4-projected', 'other']


@pytest.mark.parametrize('group', GROUPS)
def test_inputs_are_decided(group):
    if group == 'other':
        names = [n for n in sorted(RANDOM) if not n.startswith('wave')]
    else:
        names = [n for n in sorted(RANDOM) if n.startswith('wave') and n.endswith(group[4:])]
    assert len(names) >= 20
    for name in names:
        kw = RANDOM[name]
        ref = reference(name)
        assert ref['margin'] >= 1e-9, (name, ref['margin'])
        b = numpy.hypot(kw['edges'][-1], kw['sub'][-1]) if kw.get('mode') == 'projected' else kw['edges'][-1]
        assert 2 * b <= min(kw['box']) and len(kw['pos1']) <= 2500
        for p in (kw['pos1'], kw.get('pos2')):
            if p is not None and len(p):
                x = shifted(p, kw['box'], kw.get('observer'))
                assert x.min() >= b / 2 and x.max() < 1 - b / 2, name
        if name.startswith(('bins', 'ranks', 'uniform', 'cross')):
            assert (ref['npairs'] > 0).sum() >= min(len(ref['npairs']), 3), name


# ---- 2. the kernel's paths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['2d', 'projected'])
@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_wave_and_workgroup_edges(sbe, dtype, form, mode):
    """n1 and n2 independently from 0, 1, 2, 63, 64, 65, 257 and 1025 uniform rows of the padded interior, float64 and
    float32, contiguous, strided and transposed rows, cross and auto, without weights and with weights on one side"""
    pm = mesh(UNIT)
    for n1 in WAVE_NS:
        for n2 in WAVE_NS:
            p1, p2, e, s = wave_case(n1, n2, dtype, mode)
            t1, t2 = place(p1, form, sbe.device), place(p2, form, sbe.device)
            before = cpu(t1).copy()
            name = 'wave-%d-%d-%s-%s' % (n1, n2, dtype, mode)
            kw = dict(mode=mode, muedges=s if mode == '2d' else None, piedges=s if mode == 'projected' else None)
            check(survey_pair_counts(pm, t1, e, pos2=t2, **kw), reference(name), what=name)
            assert numpy.array_equal(cpu(t1), before)
            if n1 == n2:
                w = dyadic_weights(n1, 70 + n1)
                wt = torch.from_numpy(w.astype(dtype)).to(sbe.device)
                check(survey_pair_counts(pm, t1, e, pos2=t2, weight1=wt, **kw),
                      ref_survey(p1, UNIT, e, pos2=p2, w1=w, mode=mode, sub=s), what=name)
                check(survey_pair_counts(pm, t1, e, pos2=t2, weight2=wt, **kw),
                      ref_survey(p1, UNIT, e, pos2=p2, w2=w, mode=mode, sub=s), what=name)
                check(survey_pair_counts(pm, t1, e, **kw), reference('wave-auto-%d-%s-%s' % (n1, dtype, mode)),
                      what=name)


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('mode', ['2d', 'projected'])
@pytest.mark.parametrize('shape', sorted(BOUNDARY))
def test_histogram_and_edge_table_boundaries(sbe, shape, mode, weighted):
    """1024 bins (8 x 128) and 1025 (5 x 205): the small and the big histogram; nsub = 128 and 129: the sub edges in
    LDS and in global memory; nr = 129 with a small nsub; nbodykit's 40 x 100; cross with weights (the four weighted
    kernels) and auto without (the four others)"""
    name = 'bins-%s-%s' % (shape, mode) + ('' if weighted else '-auto')
    pc = run(sbe, RANDOM[name])
    assert tuple(pc.npairs.shape) == BOUNDARY[shape] and pc.mode == mode and pc.los == 'midpoint'
    assert pc.npairs.shape == pc.wnpairs.shape == pc.rsum.shape == pc.rmean.shape
    check(pc, reference(name), what=name)


def test_crowded(sbe):
    """600 rows in one cell: the histogram under contention; two launches give identical npairs"""
    pos = 0.5 + (numpy.random.RandomState(9).uniform(size=(600, 3)) - 0.5) * 0.04
    kw = dict(pos1=pos, box=UNIT, edges=numpy.linspace(0, 0.05, 6), mode='2d', sub=numpy.linspace(0, 1, 5))
    ref = ref_survey(**kw)
    assert ref['npairs'].sum() > 300000 and ref['margin'] >= 1e-9
    a, b = run(sbe, kw), run(sbe, kw)
    check(a, ref)
    check(b, ref)
    assert torch.equal(a.npairs, b.npairs)


# ---- 3. lattice cases, exact ----------------------------------------------------------------------------------------------

def both(be, rows, edges, mode, sub, pos2=None):
    """survey_pair_counts of a few lattice rows, checked against the restatement with exact weights: npairs"""
    kw = dict(pos1=numpy.asarray(rows, dtype='f8'), pos2=pos2, box=UNIT, edges=edges, mode=mode, sub=sub)
    pc = run(be, kw)
    check(pc, ref_survey(**kw), exact_w=True)
    return cpu(pc.npairs)


def test_lattice_pairs(sbe):
    """pairs on the 2^-12 lattice about the observer of the unit box, every quantity exact: a radial pair lands in the
    last mu-bin; a tangential pair (p == 0 exactly) in mu-bin 0 and pi-bin 0; a pair symmetric about the observer
    (l2 == 0) in mu-bin 0 with pi2 = 0 and rp2 = r2; pairs on an e2 edge and on a squared pi edge test <= and <;
    coincident rows and self pairs go to bin (0, 0)"""
    o = numpy.array([0.5, 0.5, 0.5])
    v = numpy.array([1.0, 2.0, 2.0]) / 64
    radial = [o + 4 * v, o + 6 * v]
    across = [o + [0.25, 1 / 32., 0], o + [0.25, -1 / 32., 0]]
    mirror = [o + v, o - v]
    edges, mu, pi = [0.0, 0.05, 0.1], [0.0, 0.25, 0.5, 1.0], [0.0, 0.05, 0.1]
    assert both(sbe, radial, edges, '2d', mu).tolist() == [[0, 0, 0], [0, 0, 2]]
    assert both(sbe, across, edges, '2d', mu).tolist() == [[0, 0, 0], [2, 0, 0]]
    assert both(sbe, mirror, edges, '2d', mu).tolist() == [[0, 0, 0], [2, 0, 0]]
    assert both(sbe, radial, edges, 'projected', pi).tolist() == [[0, 2], [0, 0]]            # rp = 0, pi = 6 / 64
    assert both(sbe, across, edges, 'projected', pi).tolist() == [[0, 0], [2, 0]]            # rp = 1 / 16, pi = 0
    assert both(sbe, mirror, edges, 'projected', pi).tolist() == [[0, 0], [2, 0]]            # rp = r = 6 / 64
    # on the edges.  The midpoint o + (1/4, 0, 0): l along x, so pi = |s_x| and rp^2 = s_y^2 + s_z^2, exactly
    m, g = o + [0.25, 0, 0], 1 / 256.

    def pair(s):
        return [m + numpy.asarray(s) * g / 2, m - numpy.asarray(s) * g / 2]
    # r = 5 g on an edge: e2[k] <= r2 puts it above, r2 < e2[k + 1] keeps it out below
    assert both(sbe, pair([0, 6, 8]), [0.0, 10 * g, 20 * g], '2d', mu).tolist() == [[0, 0, 0], [2, 0, 0]]
    assert both(sbe, pair([0, 6, 8]), [0.0, 5 * g, 10 * g], '2d', mu).tolist() == [[0, 0, 0], [0, 0, 0]]
    # pi = 6 g on a squared pi edge goes to the bin above; pi = pimax is not counted; rp = 10 g on an edge likewise
    assert both(sbe, pair([6, 6, 8]), [0.0, 10 * g, 20 * g], 'projected', [0.0, 6 * g, 12 * g]).tolist() == \
        [[0, 0], [0, 2]]
    assert both(sbe, pair([12, 6, 8]), [0.0, 10 * g, 20 * g], 'projected', [0.0, 6 * g, 12 * g]).tolist() == \
        [[0, 0], [0, 0]]
    assert both(sbe, pair([2, 6, 8]), [0.0, 5 * g, 10 * g], 'projected', [0.0, 6 * g, 12 * g]).tolist() == \
        [[0, 0], [0, 0]]
    # coincident rows: two rows at one place are a pair at r2 = 0 in bin (0, 0); a row is no pair with itself
    twice = numpy.array([o + v, o + v, o - 3 * v])
    for mode, sub in (('2d', mu), ('projected', pi)):
        n = both(sbe, twice, [0.0, 1 / 64., 0.2], mode, sub)
        assert n[0, 0] == 2 and n[0].sum() == 2
        n = both(sbe, twice, [0.0, 1 / 64., 0.2], mode, sub, pos2=twice.copy())
        assert n[0, 0] == 2 + 3                                                         # cross: the self pairs are pairs


def test_mu_comparison_at_equality(sbe):
    """p2 >= sub[k] * t at equality, one level down, where sub is passed as it is (no lattice pair sits on a dyadic mu
    other than 0 and 1: tests/test_paircount.py, test_mu_edges): the midpoint o + (1/4, 0, 0), s = (h, h, 0) has
    p2 = t / 2 exactly, so sub = 1/2 holds the pair and puts it in the bin above"""
    o = numpy.array([0.5, 0.5, 0.5])
    m, h = o + [0.25, 0, 0], 1 / 64.
    rows = numpy.stack([m + [h / 2, h / 2, 0], m - [h / 2, h / 2, 0]])
    e = numpy.array([0.0, 0.05])
    dev = sbe.device
    # (local_counts leaves the two self pairs to its caller: t == 0, mu-bin 0)
    for sub, want in (([0.0, 0.5, 1.0], [2, 2]), ([0.0, 0.5 + 2.0 ** -40, 1.0], [4, 0])):
        sub = numpy.asarray(sub)
        t = torch.from_numpy(rows).to(dev)
        got = local_counts(sbe, '2d-midpoint', 0, t, None, None, None, cell_grid(2, 0.05, UNIT), UNIT,
                           torch.from_numpy(e * e).to(dev), torch.from_numpy(sub).to(dev))
        ref = survey_core(rows, rows, numpy.asarray(UNIT), '2d-midpoint', e * e, sub)
        check(got, ref, exact_w=True)
        assert cpu(got[0]).tolist() == want


def lattice_interior(n, seed, b):
    """rows on the 2^-12 lattice of the unit box inside (b / 2, 1 - b / 2), the mirror image of each inside as well"""
    lo = int(numpy.ceil(b / 2 * 4096)) + 1
    return numpy.random.RandomState(seed).randint(lo, 4096 - lo, size=(n, 3)) / 4096.0


def test_identities(sbe):
    """exact in npairs: the (s, mu) counts summed over mu are the 1d counts of the same edges; swapping the two sets of
    a cross count, mirroring every row through the box centre (w -> L - w, exact on the lattice) and permuting the
    three axes change nothing"""
    two, one = run(sbe, RANDOM['uniform']), run(sbe, RANDOM['uniform-1d'])
    assert one.mode == '1d' and numpy.array_equal(cpu(two.npairs).sum(axis=1), cpu(one.npairs))
    check(one, reference('uniform-1d'))
    d = numpy.abs(cpu(two.rsum).sum(axis=1) - cpu(one.rsum))
    assert (d <= (cpu(one.npairs) + 4) * U * cpu(one.rsum)).all()
    b = 0.1
    p1, p2 = lattice_interior(800, 53, 0.15), lattice_interior(700, 54, 0.15)
    w1, w2 = dyadic_weights(800, 55), dyadic_weights(700, 56)
    for mode, sub in (('2d', [0.0, 0.3, 0.6, 1.0]), ('projected', [0.0, 1 / 32., 1 / 16., 0.1])):
        kw = dict(pos1=p1, pos2=p2, w1=w1, w2=w2, box=UNIT, edges=[0.0, 1 / 32., 1 / 16., b], mode=mode, sub=sub)
        ref = ref_survey(**kw)
        ab = run(sbe, kw)
        check(ab, ref, exact_w=True)
        ba = run(sbe, kw, pos1=p2, pos2=p1, w1=w2, w2=w1)
        assert torch.equal(ab.npairs, ba.npairs) and torch.equal(ab.wnpairs, ba.wnpairs)
        assert (ab.W1, ab.W2) == (ba.W2, ba.W1) == (w1.sum(), w2.sum())
        mirrored = run(sbe, kw, pos1=1.0 - p1, pos2=1.0 - p2)
        assert torch.equal(ab.npairs, mirrored.npairs) and torch.equal(ab.wnpairs, mirrored.wnpairs)
        for perm in ([1, 2, 0], [2, 1, 0]):
            turned = run(sbe, kw, pos1=p1[:, perm], pos2=p2[:, perm])
            assert torch.equal(ab.npairs, turned.npairs) and torch.equal(ab.wnpairs, turned.wnpairs)
        auto = run(sbe, kw, pos2=None, w2=None)
        check(auto, ref_survey(**dict(kw, pos2=None, w2=None)), exact_w=True)
        assert (cpu(auto.npairs) % 2 == 0).all()                # every unordered pair twice


# ---- 4. the host layer -----------------------------------------------------------------------------------------------------

def test_observer_shift(sbe):
    """an observer off the centre: the rows are shifted once in double, x' = (double)x + (L / 2 - observer); the counts
    are those of the rows shifted by hand about the centre, float32 rows included"""
    box = [1.0, 1.25, 1.5]
    obs = numpy.array([0.4, 0.7, 0.65])
    c = numpy.asarray(box) / 2 - obs
    for dtype in ('f8', 'f4'):
        pos = (interior(600, 60, 0.2, box) - c).astype(dtype)
        for mode, sub in (('2d', [0.0, 0.4, 1.0]), ('projected', [0.0, 0.05, 0.1]), ('1d', None)):
            kw = dict(pos1=pos, box=box, edges=[0.0, 0.05, 0.1], mode=mode, sub=sub, observer=obs)
            ref = ref_survey(**kw)
            assert ref['margin'] >= 1e-9 and ref['npairs'].sum() > 100
            pc = run(sbe, kw)
            assert isinstance(pc, SurveyPairCounts) and numpy.array_equal(pc.observer, obs) and pc.BoxSize == box
            check(pc, ref)
            by_hand = run(sbe, kw, pos1=pos.astype('f8') + c, observer=None)
            assert torch.equal(pc.npairs, by_hand.npairs) and numpy.array_equal(by_hand.observer, [0.5, 0.625, 0.75])
            check(by_hand, ref)


def test_padding(obe):
    """a row outside [b / 2, L - b / 2) raises, naming the axis and a BoxSize that would do, on every rank together"""
    pos = interior(90, 2, 0.1)
    pm = mesh(UNIT)
    bad = pos.copy()
    bad[7, 1] = 0.04
    with pytest.raises(ValueError, match='axis 1') as info:
        survey_pair_counts(pm, bad, [0.0, 0.1])
    assert 'BoxSize of more than %r' % (2 * (0.5 - 0.04) + 0.1) in str(info.value)
    bad = pos.copy()
    bad[3, 2] = 0.96
    with pytest.raises(ValueError, match='axis 2'):
        survey_pair_counts(pm, pos, [0.0, 0.1], pos2=bad)
    edge = pos.copy()
    edge[0] = [0.05, 0.05, 0.05]                                # b / 2 itself is inside
    assert int(cpu(survey_pair_counts(pm, edge, [0.0, 0.1]).npairs).sum()) >= 0
    with pytest.raises(ValueError, match='axis 0'):
        survey_pair_counts(pm, pos, [0.0, 0.1], observer=[0.1, 0.5, 0.5])
    # in the projected mode b is the hypotenuse: rows fine for b = 0.1 are not for hypot(0.1, 0.1)
    with pytest.raises(ValueError, match='axis'):
        survey_pair_counts(pm, edge, [0.0, 0.1], mode='projected', piedges=[0.0, 0.1])
    raised = []

    def body(comm):
        pmr = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30].copy()
        if comm.rank == 1:
            mine[4, 0] = 0.97
        with pytest.raises(ValueError, match='axis 0'):
            survey_pair_counts(pmr, mine, [0.0, 0.1], mode='2d', Nmu=3)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


def test_projected_search_radius(sbe):
    """b = hypot(edges[-1], piedges[-1]) in the projected mode: a pair with rp < rpmax and pi < pimax but r >
    max(rpmax, pimax), along a diagonal of the cylinder, is counted, among 1500 rows that set the cell size"""
    o = numpy.array([0.5, 0.5, 0.5])
    m = o + [0.3, 0, 0]
    pair = numpy.stack([m + [0.0225, 0.0225, 0], m - [0.0225, 0.0225, 0]])      # pi = rp = 0.045, r = 0.0636
    rows = interior(1500, 61, 0.08)
    rows = rows[numpy.sqrt(((rows - m) ** 2).sum(axis=1)) > 0.12]
    assert len(rows) > 1400
    kw = dict(pos1=numpy.concatenate([pair, rows]), box=UNIT, edges=[0.04, 0.05], mode='projected', sub=[0.0, 0.04, 0.05])
    ref = ref_survey(**kw)
    assert ref['margin'] >= 1e-9
    pc = run(sbe, kw)
    check(pc, ref)
    alone = run(sbe, kw, pos1=pair)
    assert cpu(alone.npairs).tolist() == [[0, 2]] and cpu(pc.npairs)[0, 1] >= 2
    with pytest.raises(ValueError, match='separation'):
        survey_pair_counts(mesh(UNIT), pair, [0.0, 0.4], mode='projected', piedges=[0.0, 0.4])


def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = interior(50, 1, 0.25)
    for edges in ([0.1], [0.2, 0.1], [-0.1, 0.1], [0.0, numpy.nan], [[0.0, 0.1]]):
        with pytest.raises(ValueError, match='edges'):
            survey_pair_counts(pm, pos, edges)
    with pytest.raises(ValueError, match='separation'):
        survey_pair_counts(pm, pos, [0.0, 0.51])
    with pytest.raises(ValueError, match='shape'):
        survey_pair_counts(pm, pos[:, :2], [0.0, 0.1])
    with pytest.raises(TypeError):
        survey_pair_counts(pm, (pos * 100).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='weight1'):
        survey_pair_counts(pm, pos, [0.0, 0.1], weight1=numpy.ones(49))
    with pytest.raises(ValueError, match='weight2'):
        survey_pair_counts(pm, pos, [0.0, 0.1], weight2=numpy.ones(50))
    with pytest.raises(ValueError, match='mode'):
        survey_pair_counts(pm, pos, [0.0, 0.1], mode='3d')
    with pytest.raises(ValueError, match='three dimensions'):
        survey_pair_counts(mesh(UNIT[:2]), pos[:, :2], [0.0, 0.1])
    for mode in ('2d', 'projected'):
        with pytest.raises(ValueError, match='needs'):
            survey_pair_counts(pm, pos, [0.0, 0.1], mode=mode)
    with pytest.raises(ValueError, match='muedges'):
        survey_pair_counts(pm, pos, [0.0, 0.1], mode='2d', muedges=[0.0, 0.9])
    with pytest.raises(ValueError, match='piedges'):
        survey_pair_counts(pm, pos, [0.0, 0.1], mode='projected', piedges=[0.01, 0.1])
    with pytest.raises(ValueError, match='bins'):
        survey_pair_counts(pm, pos, numpy.linspace(0, 0.2, 65), mode='2d', Nmu=65)
    for th in (None, [10.0], [0.0, 181.0], [20.0, 10.0], [-1.0, 10.0]):
        with pytest.raises(ValueError, match='thetaedges'):
            survey_pair_counts(pm, pos, None, mode='angular', thetaedges=th)
    for obs in ([0.5, 0.5], [0.5, 0.5, numpy.nan], 'here'):
        with pytest.raises(ValueError, match='observer'):
            survey_pair_counts(pm, pos, [0.0, 0.1], observer=obs)
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    with pytest.raises(ValueError, match='1 rows'):
        survey_pair_counts(pm, bad, [0.0, 0.1])
    at = pos.copy()
    at[3] = [0.25, 0.5, 0.5]
    with pytest.raises(ValueError, match='at the observer'):
        survey_pair_counts(pm, at, None, observer=[0.25, 0.5, 0.5], mode='angular', thetaedges=[0.0, 10.0])
    # no rows at all
    for mode, kw in (('1d', {}), ('2d', dict(Nmu=3)), ('projected', dict(piedges=[0.0, 0.05, 0.1]))):
        empty = survey_pair_counts(pm, numpy.zeros((0, 3)), [0.0, 0.1, 0.2], mode=mode, **kw)
        assert int(cpu(empty.npairs).sum()) == 0 and numpy.isnan(cpu(empty.rmean)).all() and empty.W1 == 0.0
        assert int(cpu(survey_pair_counts(pm, pos, [0.0, 0.1, 0.2], pos2=numpy.zeros((0, 3)), mode=mode,
                                          **kw).npairs).sum()) == 0
    # and the box counts keep their own refusals
    with pytest.raises(ValueError, match='mode'):
        pair_counts(pm, pos, [0.0, 0.1], mode='angular')
    with pytest.raises(ValueError, match='los'):
        pair_counts(pm, pos, [0.0, 0.1], mode='2d', los=3, Nmu=4)
    with pytest.raises(ValueError, match='mode'):
        pair_counts(pm, pos, [0.0, 0.1], mode='2d-midpoint', Nmu=4)


# ---- 5. angular ------------------------------------------------------------------------------------------------------------

def test_angular(sbe):
    """against the restatement of the chord rule; rows on the coordinate axes about the observer, 90 degrees apart,
    land in the bin that holds 90; theta, the angle of the mean chord, lies within its bin"""
    box = [1.0, 1.25, 1.5]
    obs = numpy.array([0.45, 0.6, 0.8])
    rs = numpy.random.RandomState(62)
    pos = obs + rs.normal(size=(700, 3)) * rs.uniform(0.05, 0.4, size=(700, 1))
    more = obs + rs.normal(size=(500, 3)) * 0.2
    th = [0.0, 5.0, 10.0, 20.0, 40.0]
    w1, w2 = rs.uniform(0.5, 1.5, 700), rs.uniform(0.5, 1.5, 500)
    pm = mesh(box)
    dev = sbe.device
    for kw in (dict(), dict(pos2=more), dict(pos2=more, w1=w1, w2=w2)):
        ref = ref_angular(pos, box, th, observer=obs, **kw)
        assert ref['margin'] >= 1e-9 and (ref['npairs'] > 100).all()
        pc = survey_pair_counts(pm, tensor(pos, dev), None, observer=obs, pos2=tensor(kw.get('pos2'), dev),
                                weight1=tensor(kw.get('w1'), dev), weight2=tensor(kw.get('w2'), dev), mode='angular',
                                thetaedges=th)
        check(pc, ref)
        assert pc.mode == 'angular' and pc.thetaedges.tolist() == th and tuple(pc.theta.shape) == (4,)
        assert numpy.allclose(pc.edges, 2 * numpy.sin(numpy.radians(th) / 2), rtol=1e-15)
        theta = cpu(pc.theta)
        assert ((theta > th[:-1]) & (theta < th[1:])).all()
    # the centre as the observer, float32 rows, and the axes
    axes = numpy.array([[0.9, 0.5, 0.5], [0.5, 0.6, 0.5], [0.5, 0.5, 0.2]], dtype='f4')
    pc = survey_pair_counts(mesh(UNIT), axes, None, mode='angular', thetaedges=[0.0, 60.0, 100.0, 180.0])
    assert cpu(pc.npairs).tolist() == [0, 6, 0] and numpy.array_equal(pc.observer, [0.5, 0.5, 0.5])
    assert abs(cpu(pc.theta)[1] - 90.0) < 1e-9 and numpy.isnan(cpu(pc.theta)[[0, 2]]).all()
    check(pc, ref_angular(axes, UNIT, [0.0, 60.0, 100.0, 180.0]))


def test_sky_to_cartesian(sbe):
    rs = numpy.random.RandomState(63)
    ra, dec, d = rs.uniform(0, 360, 100), rs.uniform(-90, 90, 100), rs.uniform(0.1, 2, 100)
    got = sky_to_cartesian(tensor(ra, sbe.device), dec, d.astype('f4'))
    assert got.dtype == torch.float64 and tuple(got.shape) == (100, 3) and got.device.type == sbe.device.type
    d = d.astype('f4').astype('f8')
    a, b = numpy.radians(ra), numpy.radians(dec)
    want = numpy.stack([d * numpy.cos(b) * numpy.cos(a), d * numpy.cos(b) * numpy.sin(a), d * numpy.sin(b)], axis=1)
    assert numpy.abs(cpu(got) - want).max() <= 16 * U * 2       # a few roundings of numbers below 2
    rad = sky_to_cartesian(a, b, d, degrees=False)
    assert numpy.abs(cpu(rad) - want).max() <= 16 * U * 2
    assert cpu(sky_to_cartesian([0.0, 90.0], [0.0, 0.0], [1.0, 2.0]))[0].tolist() == [1.0, 0.0, 0.0]


# ---- 6. the estimator -------------------------------------------------------------------------------------------------------

def landy_szalay(refs, sizes, shape):
    """the formula on the restated counts: refs and sizes of D1D2, D1R2, D2R1, R1R2 ((n_X, n_Y, X is Y)).  Returns
    (xi, bound).  Without weights wnpairs are exact integers on both sides, so the two differ by the roundings of the
    formula alone: each normalised count within 2 ulps (a division, or a reciprocal and a product, where the device
    library divides by a scalar so), three additions of numbers no larger than the sum S of the four, one division:
    |xi - want| <= 8 U S / nR1R2 + 4 U |want|"""
    n = []
    for ref, (nx, ny, same) in zip(refs, sizes):
        n.append(ref['wnpairs'].reshape(shape) / (float(nx) * float(ny) - (float(nx) if same else 0.0)))
    filled = refs[3]['npairs'].reshape(shape) > 0
    rr = numpy.where(filled, n[3], 1.0)
    xi = numpy.where(filled, (n[0] - n[1] - n[2] + n[3]) / rr, numpy.nan)
    bound = 8 * U * (n[0] + n[1] + n[2] + n[3]) / rr + 4 * U * numpy.abs(numpy.where(filled, xi, 0.0))
    return xi, bound


def same_xi(xi, want, bound):
    got = cpu(xi)
    filled = ~numpy.isnan(want)
    return numpy.array_equal(numpy.isnan(got), ~filled) and (numpy.abs(got - want)[filled] <= bound[filled]).all()


def test_survey_correlation(sbe):
    """Landy-Szalay on normalised counts against the formula applied to the restated counts, auto and cross, without
    weights: wnpairs are then exact integers and the two differ by the roundings of the formula alone (landy_szalay);
    R1R2 passed in equals R1R2 computed; to_poles and to_wp against their sums within the bound of a double
    sum of nsub terms"""
    b = 0.1
    d1, r1 = interior(500, 64, 0.15), interior(900, 65, 0.15)
    d2, r2 = interior(400, 66, 0.15), interior(800, 67, 0.15)
    pm = mesh(UNIT)
    edges = numpy.array([0.0, 0.001, 0.04, 0.07, b])               # the first bins are empty in R1R2: nan
    for mode, sub in (('2d', numpy.linspace(0, 1, 5)), ('projected', numpy.array([0.0, 0.03, 0.06, 0.1]))):
        kw = dict(mode=mode, muedges=sub if mode == '2d' else None, piedges=sub if mode == 'projected' else None)
        shape = (4, len(sub) - 1)
        ref = lambda a, c=None: ref_survey(a, UNIT, edges, pos2=c, mode=mode, sub=sub)
        # auto
        xi, counts = survey_correlation(pm, d1, r1, edges, **kw)
        refs = [ref(d1), ref(d1, r1), ref(d1, r1), ref(r1)]
        assert all(r['margin'] >= 1e-9 for r in refs)
        assert sorted(counts) == ['D1D2', 'D1R2', 'D2R1', 'R1R2'] and counts['D2R1'] is counts['D1R2']
        for k, r in zip(('D1D2', 'D1R2', 'D2R1', 'R1R2'), refs):
            check(counts[k], r, what=k)
        want, bound = landy_szalay(refs, [(500, 500, True), (500, 900, False), (500, 900, False), (900, 900, True)],
                                   shape)
        assert xi.dtype == torch.float64 and tuple(xi.shape) == shape
        assert numpy.isnan(want[0]).any() and not numpy.isnan(want[1:]).any()
        assert same_xi(xi, want, bound)
        again, c2 = survey_correlation(pm, d1, r1, edges, R1R2=counts['R1R2'], **kw)
        assert c2['R1R2'] is counts['R1R2'] and numpy.array_equal(cpu(again), cpu(xi), equal_nan=True)
        # cross
        xi, counts = survey_correlation(pm, d1, r1, edges, data2=d2, randoms2=r2, **kw)
        refs = [ref(d1, d2), ref(d1, r2), ref(d2, r1), ref(r1, r2)]
        for k, r in zip(('D1D2', 'D1R2', 'D2R1', 'R1R2'), refs):
            check(counts[k], r, what=k)
        want, bound = landy_szalay(refs, [(500, 400, False), (500, 800, False), (400, 900, False), (900, 800, False)],
                                   shape)
        assert same_xi(xi, want, bound)
        fin = numpy.where(numpy.isnan(want), 0.0, want)
        dsub = numpy.diff(sub)
        if mode == '2d':
            mid = (sub[1:] + sub[:-1]) / 2
            legendre = {0: numpy.ones_like(mid), 2: (3 * mid ** 2 - 1) / 2, 4: (35 * mid ** 4 - 30 * mid ** 2 + 3) / 8}
            poles = to_poles(torch.where(torch.isnan(xi), torch.zeros_like(xi), xi), sub, [0, 2, 4])
            assert tuple(poles.shape) == (4, 3) and isinstance(to_poles(fin, sub, [0]), numpy.ndarray)
            for i, l in enumerate((0, 2, 4)):
                terms = (2 * l + 1) * fin * legendre[l][None, :] * dsub[None, :]
                bound = (len(mid) + 4) * U * numpy.abs(terms).sum(axis=1) * 4   # (the polynomial itself: a few roundings)
                assert (numpy.abs(cpu(poles)[:, i] - terms.sum(axis=1)) <= bound).all()
            assert numpy.isnan(cpu(to_poles(xi, sub, [0]))[0, 0])
        else:
            wp = to_wp(torch.from_numpy(fin).to(xi.device), sub)
            terms = 2 * fin * dsub[None, :]
            assert tuple(wp.shape) == (4,)
            assert (numpy.abs(cpu(wp) - terms.sum(axis=1)) <= (len(dsub) + 4) * U * numpy.abs(terms).sum(axis=1)).all()
            assert numpy.array_equal(to_wp(fin, sub), 2 * (fin * dsub[None, :]).sum(axis=1))
    with pytest.raises(ValueError, match='randoms2'):
        survey_correlation(pm, d1, r1, edges, data2=d2)
    with pytest.raises(ValueError, match='data2'):
        survey_correlation(pm, d1, r1, edges, randoms2=r2)


# ---- 7. ranks --------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """survey_pair_counts on thread ranks holding both sets split unevenly (one rank holds no rows)"""
    kw = RANDOM[name]
    p1, p2, w1, w2 = kw['pos1'], kw.get('pos2'), kw.get('w1'), kw.get('w2')
    s1 = split(len(p1), size)
    s2 = split(len(p2), size)[::-1] if p2 is not None else None
    mode, sub = kw.get('mode', '1d'), kw.get('sub')

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a = s1[comm.rank]
        c = s2[comm.rank] if p2 is not None else None
        pc = survey_pair_counts(pm, p1[a], kw['edges'], observer=kw.get('observer'),
                                pos2=None if p2 is None else p2[c], weight1=None if w1 is None else w1[a],
                                weight2=None if w2 is None else w2[c], mode=mode,
                                muedges=sub if mode == '2d' else None, piedges=sub if mode == 'projected' else None)
        return cpu(pc.npairs), cpu(pc.wnpairs), cpu(pc.rsum), pc.W1, pc.W2, pc.W2sum, len(p1[a])
    return thread_ranks(size, body)


def check_ranks(size, np_):
    for name in ('ranks-2d', 'ranks-projected', 'ranks-1d'):
        results = ranks_case(name, size, np_)
        ref = reference(name)
        assert ref['margin'] >= 1e-9
        sizes = [results[r][6] for r in range(size)]
        assert 0 in sizes and len(set(sizes)) > 1
        for r in range(size):
            check(results[r][:3], ref, what=(name, size, r))
            for k in range(6):
                assert numpy.array_equal(results[r][k], results[0][k])      # identical on every rank


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_counts(obe, size, np_):
    """weighted cross in (s, mu), weighted auto in (rp, pi) and 1d about an observer off the centre: the arrays of
    every rank are identical and equal the restatement of all rows"""
    check_ranks(size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    check_ranks(size, np_)


# ---- 8. streams ------------------------------------------------------------------------------------------------------------

class SurveyPairs(S.Pairs):
    """pmx_pair_counts in the two midpoint modes (paircount.local_counts: the cell sort and the kernel of
    pmx_pairs_survey.hip), auto with weights on lattice rows: the bounds of tests/stream_cases.py's Pairs"""

    def __init__(self, be, mode):
        S.Pairs.__init__(self, be, mode)
        self.name = 'pairs-' + mode
        if mode == '2d-midpoint':
            self.sub = self.t(numpy.linspace(0.0, 1.0, 5) ** 2)
        else:
            self.sub = self.t(numpy.linspace(0.0, 0.1, 5) ** 2)
            self.grid = cell_grid(S.NPART, float(numpy.hypot(0.1, 0.1)) * (1 + 1e-15), S.UNIT_BOX)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['2d-midpoint', 'projected-midpoint'])
def test_delayed_producer(hipbe, mode):
    """the delayed producer of tests/test_streams.py on the new launch path, with its power conditions: the kernels of
    pmx_pairs_survey.hip run on the caller's stream, and the entry returns without waiting for it"""
    from tests import test_streams as T
    assert T.streams_are_unordered(), 'mechanism 1 has no power on this runtime (see tests/test_streams.py)'
    sleep = T.delay()
    case = SurveyPairs(hipbe, mode)
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
    # and the counts are those of the restatement
    rows, w = cpu(real[0]), cpu(real[1])
    ref = survey_core(rows, rows, numpy.ones(3), mode, cpu(case.e2), cpu(case.sub), w, w)
    check(want, ref, exact_w=True)


# ---- 9. the ABI and the resources ----------------------------------------------------------------------------------------

def test_the_modes_are_bound():
    assert _abi.PMX_PAIRS_2D_MIDPOINT == 3 == C2D and _abi.PMX_PAIRS_PROJECTED_MIDPOINT == 4 == CPROJ
    assert (_abi.PMX_PAIRS_1D, _abi.PMX_PAIRS_2D, _abi.PMX_PAIRS_PROJECTED) == (0, 1, 2)
    import pmesh_amd
    for name in ('survey_pair_counts', 'survey_correlation', 'to_poles', 'to_wp', 'sky_to_cartesian'):
        assert name in pmesh_amd.__doc__
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'pmesh_amd.h')).read()
    assert 'l_d = (w_i,d + w_j,d) - L_d' in header and 'p2 >= sub[k] * t' in header


def test_survey_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs_survey.hip')
    # survey_pairs_kernel<MODE, WEIGHTED, SLOTS>: the two midpoint modes; without and with weights; 1024 and 4096
    # histogram slots
    assert len(t) == 8 and all('survey_pairs_kernel' in k for k in t), sorted(t)
    for mode in (C2D, CPROJ):
        assert len([k for k in t if 'survey_pairs_kernelILi%dE' % mode in k]) == 4, sorted(t)
    for name, r in t.items():
        weighted, big = 'Lb1E' in name, 'Li4096E' in name
        assert r['ScratchSize'] == 0, (name, r)
        # the budgets of test_pairs_kernels_compile_within_their_budgets: two workgroups in the 160 KB of a CU at the least
        assert r['LDS'] <= 80 * 1024, (name, r)
        assert r['LDS'] <= ((80 if weighted else 52) if big else (24 if weighted else 16)) * 1024, (name, r)
        # the full 8 waves per SIMD.  Measured at compile time: 46 VGPRs without weights in both modes, with weights 48
        # and 50 (s, mu) and 50 and 52 (rp, pi) for 1024 and 4096 slots; LDS 14360 / 22552 / 51224 / 81920 bytes
        assert r['VGPRs'] <= 64, (name, r)
