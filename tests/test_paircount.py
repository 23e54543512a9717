"""pmesh_amd.paircount (csrc/pmx_pairs.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/paircount.py, include/pmesh_amd.h).  Rows are wrapped into [0, L_d) by FoF's rule; dx_d is the
minimum image of the wrapped rows; all arithmetic is double, every operation rounded once; r2 = sum_d dx_d^2 in the
order d = 0, 1, 2.  With e2[k] = edges[k] * edges[k] a pair is in r-bin k when e2[k] <= q < e2[k + 1]; q = r2 in the
modes 1d and 2d, q = rp2 (the two dx_d^2 with d != los, ascending d) in the projected mode.  2d: the mu-bin is the
number of k in 1 .. nmu - 1 with dx_los^2 >= muedges[k]^2 * r2, and 0 where r2 == 0.  Projected: the pi-bin is the
number of k in 1 .. npi - 1 with |dx_los| >= piedges[k]; |dx_los| >= piedges[-1] is not counted.  Cross: every (i, j);
auto: every ordered pair i != j by row index.  Per bin npairs (exact), wnpairs = sum w1 w2, rsum = sum w1 w2 sqrt(q).

The restatement is brute force: the full (n1, n2) matrices of r2, rp2 and dx_los, binned with the same comparisons.
Under -m "not gpu" it serves pmx_pair_counts (PairsOracleBackend), so the host layer and the thread ranks run without
a GPU; under -m gpu the kernel is compared with it.

npairs is compared by exact integer equality everywhere.  wnpairs is compared by exact equality where the weights are
multiples of 1/8 in [1/8, 2] and the positions lie on a 2^-12 lattice (every product and sum is then exact in any
order).  Otherwise wnpairs and rsum are compared within |got - ref| <= (M + 4) 2^-52 S: M the number of terms the
device may have added into the bin (its pairs, plus the csize self pairs of bin (0, 0) in the auto form), S the sum of
their absolute values: the worst case of a double sum in any order, plus one ulp for the square root.

The condition on random inputs: no pair with |q - e2[k]| < 1e-9 e2[k], |z2 - m2[k] r2| < 1e-9 r2 or |a - piedges[k]|
< 1e-9 (a contracted multiply-add could otherwise move a pair); test_inputs_are_decided asserts it without a GPU for
every random case.  The lattice cases are exact; their pairs sitting on edges test the <= and the < themselves.
"""
import os

import numpy
import pytest
import torch

from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid
from pmesh_amd.paircount import (MAX_BINS, MODES, PairCounts, bin_volumes, local_counts, pair_correlation,
                                 pair_counts)
from tests.test_fof import (GRIDS, PERIODIC, RANKS, ROW_FORMS, SLAB, UNIT, WAVE_NS, FofOracleBackend, crowded,
                            face_pairs, lattice, mesh, place, split, thread_ranks, uniform, wrap)
from tests.test_lpt import cpu

U = 2.0 ** -52


# ---- the restatement -----------------------------------------------------------------------------------------------

def count_core(w1, w2, box, mode, los, e2, sub, wt1=None, wt2=None, skip_diagonal=False):
    """The sums over the pairs of the wrapped rows w1 with w2.  e2: the squared edges; sub: m2 (2d) or piedges
    (projected).  Returns a dict: npairs, wnpairs, rsum (flat), margin (the smallest relative distance of a pair from
    an edge, by the three measures of the module docstring)."""
    n1, n2, nd = len(w1), len(w2), w1.shape[1]
    nr, nsub = len(e2) - 1, (1 if mode == '1d' else len(sub) - 1)
    nbins = nr * nsub
    out = dict(npairs=numpy.zeros(nbins, dtype='i8'), wnpairs=numpy.zeros(nbins), rsum=numpy.zeros(nbins),
               margin=numpy.inf)
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
    if skip_diagonal:
        keep &= ~numpy.eye(n1, n2, dtype=bool)
    rbin = numpy.searchsorted(e2, q, side='right') - 1          # the number of k with e2[k] <= q, less one
    margin = numpy.inf
    pe = e2[e2 > 0]
    for shift in (1, 0):                                        # the positive edge below (or the first) and the one above
        near = pe[numpy.clip(numpy.searchsorted(pe, q) - shift, 0, len(pe) - 1)]
        margin = min(margin, float((numpy.abs(q - near) / near).min()))
    sbin = numpy.zeros((n1, n2), dtype='i8')
    if mode == '2d':
        z2 = dx[los] * dx[los]
        some = keep & (q > 0)
        for k in range(1, nsub):
            t = sub[k] * q
            sbin += z2 >= t
            if some.any():
                margin = min(margin, float((numpy.abs(z2 - t)[some] / q[some]).min()))
        sbin[q == 0] = 0
    elif mode == 'projected':
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
    flat = (rbin * nsub + sbin)[keep]
    out['npairs'] = numpy.bincount(flat, minlength=nbins).astype('i8')
    out['wnpairs'] = numpy.bincount(flat, weights=w[keep], minlength=nbins)
    out['rsum'] = numpy.bincount(flat, weights=(w * numpy.sqrt(q))[keep], minlength=nbins)
    out['margin'] = margin
    return out


def ref_pairs(pos1, box, edges, pos2=None, w1=None, w2=None, mode='1d', sub=None, los=2):
    """the restatement of pair_counts(mesh(box), pos1, edges, pos2, w1, w2, mode, muedges / piedges = sub, los)"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    s = None if sub is None else numpy.asarray(sub, dtype='f8')
    a = wrap(pos1, box)
    auto = pos2 is None
    out = count_core(a, a if auto else wrap(pos2, box), box, mode, los, e * e, s * s if mode == '2d' else s,
                     w1, w1 if auto else w2, skip_diagonal=auto)
    # what the device may have added on top: the self pairs of the auto form, in bin (0, 0)
    out['nself'], out['wself'] = 0, 0.0
    if auto and e[0] == 0:
        out['nself'] = len(a)
        out['wself'] = float(len(a)) if w1 is None else float((numpy.asarray(w1).astype('f8') ** 2).sum())
    return out


class PairsOracleBackend(FofOracleBackend):
    """the CPU test double with pmx_pair_counts served by the restatement"""
    name = 'oracle-pairs'

    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        n1, n2, nd = spos1.shape[0], spos2.shape[0], spos1.shape[1]
        if n1 == 0 or n2 == 0:
            return
        name = {v: k for k, v in MODES.items()}[mode]
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell))
        # the rows back in row order: the weights come in row order
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = count_core(a, b, numpy.asarray(boxsize, dtype='f8'), name, los, e2.numpy(),
                         None if sub is None else sub.numpy(), None if weight1 is None else weight1.numpy(),
                         None if weight2 is None else weight2.numpy())
        npairs += torch.from_numpy(got['npairs'])
        wnpairs += torch.from_numpy(got['wnpairs'])
        rsum += torch.from_numpy(got['rsum'])


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(PairsOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def pbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(PairsOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def check(pc, ref, exact_w=False, what=''):
    """a PairCounts (or a triple of flat arrays) against the restatement's dict"""
    got = (pc.npairs, pc.wnpairs, pc.rsum) if isinstance(pc, PairCounts) else pc
    got = [(x if isinstance(x, numpy.ndarray) else cpu(x)).reshape(-1) for x in got]
    assert got[0].dtype == numpy.int64 and got[1].dtype == got[2].dtype == numpy.float64
    assert numpy.array_equal(got[0], ref['npairs']), (what, got[0][:8], ref['npairs'][:8])
    M = ref['npairs'].astype('f8')
    Sw, Sr = numpy.abs(ref['wnpairs']).copy(), numpy.abs(ref['rsum'])
    M[0] += ref.get('nself', 0)
    Sw[0] += ref.get('wself', 0.0)
    dw, dr = numpy.abs(got[1] - ref['wnpairs']), numpy.abs(got[2] - ref['rsum'])
    if exact_w:
        assert numpy.array_equal(got[1], ref['wnpairs']), what
    else:
        assert (dw <= (M + 4) * U * Sw).all(), (what, dw.max())
    assert (dr <= (M + 4) * U * Sr).all(), (what, dr.max())


def dyadic_weights(n, seed):
    return numpy.random.RandomState(seed).randint(1, 17, size=n) / 8.0


def lattice_rows(n, nd, seed, box=None):
    """rows on the 2^-12 lattice of the box: differences, squares and their sums are exact"""
    box = numpy.ones(nd) if box is None else numpy.asarray(box)
    return numpy.random.RandomState(seed).randint(0, 4096, size=(n, nd)) / 4096.0 * box


# ---- the inputs ----------------------------------------------------------------------------------------------------

def wave_b(n1, n2):
    return min(0.45, 0.6 * max(n1, n2, 1) ** (-1 / 3.))


def wave_case(n1, n2, dtype):
    b = wave_b(n1, n2)
    return (uniform(n1, 3, 300 + n1).astype(dtype), uniform(n2, 3, 500 + n2).astype(dtype),
            numpy.array([0.0, 0.4 * b, 0.8 * b, b]))


def random_cases():
    """name -> keyword arguments of ref_pairs: every random input of the tests below"""
    cases = {}
    for dtype in ('f8', 'f4'):
        for n1 in WAVE_NS:
            for n2 in WAVE_NS:
                p1, p2, e = wave_case(n1, n2, dtype)
                cases['wave-%d-%d-%s' % (n1, n2, dtype)] = dict(pos1=p1, pos2=p2, box=UNIT, edges=e)
            cases['wave-auto-%d-%s' % (n1, dtype)] = dict(pos1=wave_case(n1, n1, dtype)[0], box=UNIT,
                                                          edges=wave_case(n1, n1, dtype)[2])
    cases['crowded'] = dict(pos1=crowded(), box=UNIT, edges=numpy.linspace(0, 0.05, 6))
    for nd in (3, 2, 1):
        rows = numpy.concatenate([face_pairs(SLAB[:nd], 0.05), uniform(300, nd, 61, SLAB[:nd])])
        cases['faces-%dd' % nd] = dict(pos1=rows, box=SLAB[:nd], edges=[0.0, 0.02, 0.04, 0.05])
    cases['open'] = dict(pos1=uniform(2000, 3, 12), box=UNIT, edges=[0.01, 0.03, 0.05])
    cases['uniform'] = dict(pos1=uniform(700, 3, 31), box=UNIT, edges=numpy.linspace(0, 0.12, 7))
    cases['uniform-2d'] = dict(pos1=uniform(700, 3, 31), box=UNIT, edges=numpy.linspace(0, 0.12, 7), mode='2d',
                               sub=numpy.linspace(0, 1, 6))
    cases['nonuniform'] = dict(pos1=uniform(700, 3, 32), pos2=uniform(500, 3, 33), box=UNIT,
                               edges=[0.01, 0.015, 0.04, 0.1, 0.11])
    cases['one-bin'] = dict(pos1=uniform(700, 3, 32), box=UNIT, edges=[0.02, 0.1])
    cases['bins-200'] = dict(pos1=uniform(700, 3, 34), box=UNIT, edges=numpy.linspace(0, 0.15, 201))
    cases['bins-max-1d'] = dict(pos1=uniform(700, 3, 35), box=UNIT, edges=numpy.linspace(0, 0.15, MAX_BINS + 1))
    cases['bins-max-2d'] = dict(pos1=uniform(400, 3, 36), pos2=uniform(300, 3, 37), box=UNIT,
                                edges=numpy.linspace(0, 0.3, 65), mode='2d', sub=numpy.linspace(0, 1, 65))
    cases['bins-max-2d-weighted'] = dict(cases['bins-max-2d'], w1=numpy.random.RandomState(3).uniform(0.5, 1.5, 400),
                                         w2=numpy.random.RandomState(4).uniform(0.5, 1.5, 300))
    cases['bins-40x100'] = dict(pos1=uniform(400, 3, 38), box=UNIT, edges=numpy.linspace(0, 0.3, 41), mode='2d',
                                sub=numpy.linspace(0, 1, 101), los=1)
    cases['projected'] = dict(pos1=uniform(700, 3, 39, SLAB), pos2=uniform(600, 3, 40, SLAB), box=SLAB,
                              edges=[0.0, 0.02, 0.05, 0.08], mode='projected', sub=[0.0, 0.03, 0.06, 0.12], los=0)
    cases['weights-uniform'] = dict(pos1=uniform(600, 3, 41), pos2=uniform(500, 3, 42), box=UNIT,
                                    edges=numpy.linspace(0, 0.15, 6),
                                    w1=numpy.random.RandomState(5).uniform(0.5, 1.5, 600),
                                    w2=numpy.random.RandomState(6).uniform(0.5, 1.5, 500).astype('f4'))
    cases['weights-auto'] = dict(pos1=uniform(600, 3, 41), box=UNIT, edges=numpy.linspace(0, 0.15, 6),
                                 w1=numpy.random.RandomState(5).uniform(0.5, 1.5, 600))
    cases['xi'] = dict(pos1=uniform(2000, 3, 43), box=UNIT, edges=numpy.linspace(0.0, 0.1, 6))
    cases['ranks'] = dict(pos1=uniform(900, 3, 44), pos2=uniform(700, 3, 45), box=UNIT,
                          edges=numpy.linspace(0, 0.1, 5), w1=numpy.random.RandomState(7).uniform(0.5, 1.5, 900),
                          w2=numpy.random.RandomState(8).uniform(0.5, 1.5, 700))
    cases['ranks-auto'] = dict(pos1=uniform(900, 3, 44), box=UNIT, edges=numpy.linspace(0, 0.1, 5))
    cases['ranks-slab'] = dict(pos1=uniform(900, 3, 46, SLAB), box=SLAB, edges=[0.0, 0.05, 0.1, 0.125], mode='2d',
                               sub=[0.0, 0.3, 0.8, 1.0], w1=numpy.random.RandomState(9).uniform(0.5, 1.5, 900))
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_pairs(**RANDOM[name])
    return _REFERENCE[name]


def run_case(be, name, **over):
    """pair_counts of a random case on one rank"""
    kw = dict(RANDOM[name], **over)
    dev = be.device
    t = lambda x: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)
    mode = kw.get('mode', '1d')
    sub = kw.get('sub')
    return pair_counts(mesh(kw['box']), t(kw['pos1']), kw['edges'], pos2=t(kw.get('pos2')), weight1=t(kw.get('w1')),
                       weight2=t(kw.get('w2')), mode=mode, muedges=sub if mode == '2d' else None,
                       piedges=sub if mode == 'projected' else None, los=kw.get('los', 2))


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_on_known_answers():
    """the 8^3 lattice of spacing 1/8: r3(1..3) = 6 + 12 + 8 and r3(4..8) = 6 + 24 + 24 + 0 + 12 neighbours per row;
    pairs at exactly 3/8 are excluded, pairs at exactly 1/8 included; and five rows on a line"""
    pos = lattice(3)
    assert ref_pairs(pos, UNIT, [1 / 8., 2 / 8., 3 / 8.])['npairs'].tolist() == [13312, 33792] == [512 * 26, 512 * 66]
    assert ref_pairs(pos, UNIT, [0, 1 / 8., 2 / 8., 3 / 8., 1 / 2.])['npairs'].tolist() == [0, 13312, 33792, 80896]
    line = numpy.array([[0.95], [0.5], [0.02], [0.09], [0.41]])
    got = ref_pairs(line, [1.0], [0.0, 0.08, 0.1])
    assert got['npairs'].tolist() == [4, 2] and got['nself'] == 5     # 0.95-0.02, 0.02-0.09 | 0.5-0.41, each twice
    assert abs(got['rsum'][0] - 2 * (0.07 + 0.07)) < 1e-15
    cross = ref_pairs(line, [1.0], [0.0, 0.08, 0.1], pos2=line.copy())
    assert cross['npairs'].tolist() == [9, 2]
    # mu: (0, 1, 1) / 8 has mu^2 = 1/2, on the line of sight mu = 1 lands in the last bin; pi: |dz| = 1/8 on an edge
    two = numpy.array([[0, 0, 0], [0, 1 / 8., 1 / 8.], [0, 0, 3 / 8.]])
    got = ref_pairs(two, UNIT, [0.0, 0.5], mode='2d', sub=[0.0, 0.5, 1.0])
    assert got['npairs'].tolist() == [0, 6]
    got = ref_pairs(two, UNIT, [0.0, 0.5], mode='2d', sub=[0.0, 0.75, 1.0])
    assert got['npairs'].tolist() == [2, 4]
    got = ref_pairs(two, UNIT, [0.0, 0.2], mode='projected', sub=[0.0, 1 / 8., 2 / 8., 3 / 8.])
    assert got['npairs'].tolist() == [0, 2, 2]                       # |dz| = 1/8 and 2/8 on their edges; 3/8 = pimax is out


@pytest.mark.parametrize('group', ['wave-f8', 'wave-f4', 'other'])
def test_inputs_are_decided(group):
    names = [n for n in sorted(RANDOM) if (n.startswith('wave') and n.endswith(group[-2:])) or
             (group == 'other' and not n.startswith('wave'))]
    assert len(names) >= 20
    for name in names:
        kw = RANDOM[name]
        ref = reference(name)
        assert ref['margin'] >= 1e-9, (name, ref['margin'])
        b = max(kw['edges'][-1], kw['sub'][-1]) if kw.get('mode') == 'projected' else kw['edges'][-1]
        assert 2 * b <= min(kw['box']) and len(kw['pos1']) <= 2500
        if not name.startswith('wave') and name != 'crowded':
            assert (ref['npairs'] > 0).sum() >= min(len(ref['npairs']), 3), name


def test_lattice_rows_are_exact():
    """1500 rows on the 2^-12 lattice: r2 equals the exact rational value (integer arithmetic on the numerators)"""
    pos = lattice_rows(1500, 3, 50)
    k = numpy.rint(pos * 4096).astype('i8')
    assert numpy.array_equal(k / 4096.0, pos)
    d = k[:, None, :] - k[None, :, :]
    d = d - 4096 * numpy.rint(d / 4096.0).astype('i8')
    exact = (d * d).sum(axis=2)
    w = wrap(pos, UNIT)
    r2 = numpy.zeros((1500, 1500))
    for a in range(3):
        dx = w[:, None, a] - w[None, :, a]
        dx = dx - numpy.rint(dx)
        r2 = r2 + dx * dx
    assert numpy.array_equal(r2 * 4096.0 ** 2, exact.astype('f8'))


def test_bin_volumes():
    """every V_bin formula against a midpoint-rule integral of the shell's measure"""
    e = numpy.array([0.0, 0.3, 0.5, 1.25])
    r = (numpy.arange(200000) + 0.5) * (1.25 / 200000)
    dr = 1.25 / 200000
    which = numpy.searchsorted(e, r, side='right') - 1
    for nd, measure in ((3, 4 * numpy.pi * r * r), (2, 2 * numpy.pi * r), (1, 2 * numpy.ones_like(r))):
        want = numpy.bincount(which, weights=measure * dr, minlength=3)
        assert numpy.allclose(bin_volumes(e, nd), want, rtol=1e-9, atol=0)
    mu = numpy.array([0.0, 0.25, 0.5, 1.0])
    v3 = bin_volumes(e, 3)
    # the shell between two cones |cos theta| in [mu_lo, mu_hi): 2 * 2 pi r^2 dr (mu_hi - mu_lo)
    got = bin_volumes(e, 3, '2d', mu)
    assert got.shape == (3, 3) and numpy.allclose(got, v3[:, None] * numpy.diff(mu)[None, :], rtol=1e-15)
    assert numpy.allclose(got.sum(axis=1), v3, rtol=1e-15)
    # a direct integral of one (r, mu) bin in cylinder coordinates: rp^2 + z^2 in [e_lo^2, e_hi^2), |z| / r in [mu_lo, mu_hi)
    g = (numpy.arange(1500) + 0.5) * (1.25 / 1500)
    rp, z = numpy.meshgrid(g, g, indexing='ij')
    rr = numpy.sqrt(rp * rp + z * z)
    inside = (rr >= 0.3) & (rr < 0.5) & (z / rr >= 0.25) & (z / rr < 0.5)
    assert abs((2 * numpy.pi * rp * inside).sum() * 2 * (1.25 / 1500) ** 2 / got[1, 1] - 1) < 2e-3
    pi = numpy.array([0.0, 1.0, 2.0, 4.0])
    got = bin_volumes(e, 3, 'projected', pi)
    want = numpy.bincount(which, weights=2 * numpy.pi * r * dr, minlength=3)[:, None] * (2 * numpy.diff(pi))[None, :]
    assert numpy.allclose(got, want, rtol=1e-9)


# ---- 2. known answers and the kernel's paths -----------------------------------------------------------------------------

def test_known_answer(pbe):
    """the 8^3 lattice of the unit box, auto: npairs [13312, 33792] and [0, 13312, 33792, 80896]; without weights
    wnpairs = npairs; rmean of the first bin is the mean over its three shells; the 2-d and 1-d lattices"""
    pm = mesh(UNIT)
    pos = torch.from_numpy(lattice(3)).to(pbe.device)
    pc = pair_counts(pm, pos, [1 / 8., 2 / 8., 3 / 8.])
    assert isinstance(pc, PairCounts) and pc.mode == '1d' and pc.auto and pc.npairs.dtype == torch.int64
    assert cpu(pc.npairs).tolist() == [13312, 33792]
    assert cpu(pc.wnpairs).tolist() == [13312.0, 33792.0]
    assert (pc.W1, pc.W2, pc.W2sum) == (512.0, 512.0, 512.0)
    check(pc, ref_pairs(lattice(3), UNIT, [1 / 8., 2 / 8., 3 / 8.]))
    assert abs(cpu(pc.rmean)[0] - (6 + 12 * 2 ** 0.5 + 8 * 3 ** 0.5) / 26 / 8) <= 1e-14
    edges = [0, 1 / 8., 2 / 8., 3 / 8., 1 / 2.]
    pc = pair_counts(pm, pos, edges)
    assert cpu(pc.npairs).tolist() == [0, 13312, 33792, 80896]
    check(pc, ref_pairs(lattice(3), UNIT, edges))
    assert numpy.isnan(cpu(pc.rmean)[0]) and not numpy.isnan(cpu(pc.rmean)[1:]).any()
    for nd in (2, 1):
        ref = ref_pairs(lattice(nd), UNIT[:nd], edges)
        assert ref['npairs'].tolist() == ([0, 64 * 8, 64 * 16, 64 * 20] if nd == 2 else [0, 16, 16, 16])
        check(pair_counts(mesh(UNIT[:nd]), lattice(nd), edges), ref)


def grid_of(ncell, box):
    nd = len(box)
    return (list(ncell[:nd]), [0.0] * nd, [ncell[d] / box[d] for d in range(nd)], PERIODIC[nd])


def run_local(be, kw, grid, pos1=None, pos2=None):
    """local_counts on a forced grid: the flat triple"""
    dev = be.device
    e = numpy.asarray(kw['edges'], dtype='f8')
    p1 = torch.from_numpy(kw['pos1'] if pos1 is None else pos1).to(dev)
    p2 = None if pos2 is None else torch.from_numpy(pos2).to(dev)
    return local_counts(be, kw.get('mode', '1d'), kw.get('los', 2), p1, None, p2, None, grid, kw['box'],
                        torch.from_numpy(e * e).to(dev), None)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(pbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes (in 3-d, 2-d and 1-d): no pair is visited twice, none is missed"""
    for nd in (3, 2, 1):
        name = 'faces-%dd' % nd
        kw = RANDOM[name]
        assert all(kw['box'][d] / grid[d] >= kw['edges'][-1] for d in range(nd))
        got = [cpu(x) for x in run_local(pbe, kw, grid_of(grid, kw['box']))]
        ref = reference(name)
        got[0][0] -= ref['nself']                               # (local_counts leaves the self pairs to its caller)
        got[1][0] -= ref['wself']
        check(got, ref, what=(name, grid))
    # and the grid the host layer lays through the cell cap: few rows and a large b
    pos = face_pairs(SLAB, 0.05)
    assert cell_grid(len(pos), 0.05, SLAB)[0] == [6, 3, 1]
    check(pair_counts(mesh(SLAB), pos, [0.0, 0.02, 0.04, 0.05]), ref_pairs(pos, SLAB, [0.0, 0.02, 0.04, 0.05]))


def test_open_axes(pbe):
    """a grid that is open along two axes (a rank's block): the rows of the block against all rows, nothing wraps on
    the open axes, rows outside the extent sit in the end cells and pair with nothing"""
    kw = RANDOM['open']
    pos, b = kw['pos1'], kw['edges'][-1]
    grid = cell_grid(len(pos), b, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2 and grid[1][0] == 0.25 - b
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    assert 100 < inside.sum() < 1000
    got = run_local(pbe, kw, grid, pos1=pos[inside], pos2=pos)
    ref = ref_pairs(pos[inside], UNIT, kw['edges'], pos2=pos)
    assert ref['margin'] >= 1e-9 and ref['npairs'].min() > 10
    check(got, ref)


def wave_check(be, dtype, form, pairs, auto):
    pm = mesh(UNIT)
    for n1, n2 in pairs:
        p1, p2, e = wave_case(n1, n2, dtype)
        t1, t2 = place(p1, form, be.device), place(p2, form, be.device)
        before = cpu(t1).copy()
        name = 'wave-%d-%d-%s' % (n1, n2, dtype)
        check(pair_counts(pm, t1, e, pos2=t2), reference(name), what=name)
        assert numpy.array_equal(cpu(t1), before)
        if n1 == n2:
            # dyadic weights on one side, None on the other: float32 positions are dyadic as well, but not these sums
            w = dyadic_weights(n1, 70 + n1)
            wt = torch.from_numpy(w.astype(dtype)).to(be.device)
            check(pair_counts(pm, t1, e, pos2=t2, weight1=wt), ref_pairs(p1, UNIT, e, pos2=p2, w1=w), what=name)
            check(pair_counts(pm, t1, e, pos2=t2, weight2=wt), ref_pairs(p1, UNIT, e, pos2=p2, w2=w), what=name)
            if auto:
                check(pair_counts(pm, t1, e), reference('wave-auto-%d-%s' % (n1, dtype)), what=name)
                if form == 'C' and n1 in (0, 65):
                    check(pair_counts(pm, p1, e), reference('wave-auto-%d-%s' % (n1, dtype)), what=name)


@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_wave_and_workgroup_edges(pbe, dtype, form):
    """n1 and n2 independently from 0, 1, 2, 63, 64, 65, 257 and 1025 uniform rows, float64 and float32, contiguous,
    strided and transposed rows, cross and auto, and weights on one side only"""
    wave_check(pbe, dtype, form, [(a, b) for a in WAVE_NS for b in WAVE_NS], auto=True)


def test_crowded(pbe):
    """600 rows in one cell: the histogram under contention; two launches give identical npairs"""
    ref = reference('crowded')
    assert ref['npairs'].sum() > 300000
    a, b = run_case(pbe, 'crowded'), run_case(pbe, 'crowded')
    check(a, ref)
    check(b, ref)
    assert torch.equal(a.npairs, b.npairs)
    # and with lattice rows and dyadic weights: every sum of wnpairs is exact
    pos = 0.5 + (lattice_rows(600, 3, 51) - 0.5) * 2.0 ** -5
    w = dyadic_weights(600, 52)
    e = numpy.array([0.0, 1 / 128., 1 / 64., 1 / 32.])
    check(pair_counts(mesh(UNIT), pos, e, weight1=w), ref_pairs(pos, UNIT, e, w1=w), exact_w=True)


@pytest.mark.parametrize('name', ['one-bin', 'nonuniform', 'bins-200', 'bins-max-1d', 'bins-max-2d',
                                  'bins-max-2d-weighted', 'bins-40x100', 'uniform', 'uniform-2d', 'projected',
                                  'weights-uniform', 'weights-auto'])
def test_random_cases(pbe, name):
    """one bin; PMX_PAIRS_MAX_BINS bins in 1d and as 64 x 64 in 2d, without and with weights; nbodykit's 40 x 100;
    non-uniform edges with edges[0] > 0; more edges than the kernel holds in LDS; the three modes; weights within the
    bound of a double sum in any order"""
    pc = run_case(pbe, name)
    kw = RANDOM[name]
    nr, nsub = len(kw['edges']) - 1, len(kw.get('sub', [0, 1])) - 1
    assert tuple(pc.npairs.shape) == ((nr,) if kw.get('mode', '1d') == '1d' else (nr, nsub))
    assert pc.npairs.shape == pc.wnpairs.shape == pc.rsum.shape == pc.rmean.shape
    if name.startswith('bins-max'):
        assert nr * nsub == MAX_BINS >= 4096
    check(pc, reference(name), what=name)


def test_too_many_bins(obe):
    pm, pos = mesh(UNIT), uniform(50, 3, 1)
    with pytest.raises(ValueError, match='bins'):
        pair_counts(pm, pos, numpy.linspace(0, 0.2, MAX_BINS + 2))
    with pytest.raises(ValueError, match='bins'):
        pair_counts(pm, pos, numpy.linspace(0, 0.2, 65), mode='2d', Nmu=65)
    with pytest.raises(ValueError, match='bins'):
        pair_counts(pm, pos, numpy.linspace(0, 0.2, 1026), mode='projected', pimax=4)
    assert tuple(pair_counts(pm, pos, numpy.linspace(0, 0.2, 65), mode='2d', Nmu=64).npairs.shape) == (64, 64)


def test_coincident_rows(pbe):
    """two distinct rows at one position are a pair at r2 = 0: counted in the auto form when edges[0] == 0, in mu-bin
    0 and pi-bin 0; a row is no pair with itself; with edges[0] > 0 neither is counted"""
    pos = numpy.concatenate([uniform(100, 3, 2), uniform(100, 3, 2)[:7], [[1.0, 1.0, 1.0], [0.0, 0.0, 0.0]]])
    pm = mesh(UNIT)
    pc = pair_counts(pm, pos, [0.0, 1e-3])
    assert cpu(pc.npairs).tolist() == [16] and cpu(pc.wnpairs).tolist() == [16.0] and cpu(pc.rsum).tolist() == [0.0]
    pc = pair_counts(pm, pos, [0.0, 1e-3, 0.1], mode='2d', Nmu=4)
    assert cpu(pc.npairs)[0].tolist() == [16, 0, 0, 0]
    check(pc, ref_pairs(pos, UNIT, [0.0, 1e-3, 0.1], mode='2d', sub=numpy.linspace(0, 1, 5)))
    pc = pair_counts(pm, pos, [0.0, 1e-3], mode='projected', piedges=[0.0, 0.1, 0.25], los=1)
    assert cpu(pc.npairs)[0, 0] >= 16
    check(pc, ref_pairs(pos, UNIT, [0.0, 1e-3], mode='projected', sub=[0.0, 0.1, 0.25], los=1))
    assert cpu(pair_counts(pm, pos, [1e-6, 1e-3]).npairs).tolist() == [0]
    # cross with a copy: the self pairs are pairs
    assert cpu(pair_counts(pm, pos, [0.0, 1e-3], pos2=pos.copy()).npairs).tolist() == [16 + 109]


def test_mu_edges(pbe):
    """2d on the lattice with dyadic muedges: pairs along the line of sight (mu = 1) land in the last bin, pairs across
    it (mu = 0) in the first.  A lattice pair cannot sit on a dyadic mu other than 0 and 1 (x^2 + y^2 = (4^k - a^2) /
    a^2 z^2 has no solution for odd a: the factor is 3 mod 4), so the comparison z2 >= m2[k] * r2 at equality is tested
    one level down, where m2 is passed as it is: m2 = 1/2 holds the pairs (0, 1, 1) / 8, m2 = 1/4 none, and both give
    what the restatement gives"""
    pos = lattice(3)
    edges = [1 / 8., 5 / 32., 3 / 16., 3 / 8.]
    for los in (0, 1, 2):
        mu = [0.0, 0.25, 0.5, 0.75, 1.0]
        ref = ref_pairs(pos, UNIT, edges, mode='2d', sub=mu, los=los)
        pc = pair_counts(mesh(UNIT), pos, edges, mode='2d', muedges=mu, los=los)
        check(pc, ref, exact_w=True)
        first = cpu(pc.npairs)[0]                                # the shell r = 1/8: four across, two along
        assert first.tolist() == [512 * 4, 0, 0, 512 * 2] and pc.los == los and pc.muedges.tolist() == mu
    dev = pbe.device
    e = numpy.asarray(edges)
    for m2 in ([0.0, 0.5, 1.0], [0.0, 0.25, 0.5, 1.0]):
        m2 = numpy.asarray(m2)
        t = torch.from_numpy(pos).to(dev)
        got = local_counts(pbe, '2d', 2, t, None, None, None, cell_grid(512, 3 / 8., UNIT), UNIT,
                           torch.from_numpy(e * e).to(dev), torch.from_numpy(m2).to(dev))
        ref = count_core(pos, pos, numpy.asarray(UNIT), '2d', 2, e * e, m2)
        check(got, ref, exact_w=True)
        # the shell r^2 = 2/64, bin 1: four of its twelve pairs lie across, the eight with z2 = r2 / 2 sit on m2 = 1/2
        shell = cpu(got[0]).reshape(3, -1)[1]
        assert shell.tolist() == ([512 * 4, 512 * 8] if len(m2) == 3 else [512 * 4, 0, 512 * 8])


def test_projected(pbe):
    """bins of (rp, pi) on the lattice of spacing 1 in the box of side 8, every line of sight, pimax = 3 (unit bins):
    pairs at exactly piedges[k] go to bin k, pairs at exactly pimax are not counted, rp at exactly an edge likewise"""
    pos, box = lattice(3) * 8, [8.0] * 3
    edges = [0.0, 1.0, 2.0, 3.5]
    for los in (0, 1, 2):
        pc = pair_counts(mesh(box), pos, edges, mode='projected', pimax=3, los=los)
        assert pc.piedges.tolist() == [0.0, 1.0, 2.0, 3.0] and pc.muedges is None and pc.mode == 'projected'
        ref = ref_pairs(pos, box, edges, mode='projected', sub=[0.0, 1.0, 2.0, 3.0], los=los)
        check(pc, ref, exact_w=True)
        n = cpu(pc.npairs)
        # rp = 0: the row itself is no pair; |pi| = 1 and 2 once on either side, |pi| = 3 is pimax
        assert n[0].tolist() == [0, 512 * 2, 512 * 2]
        # rp^2 in [1, 4): (1, 0), (0, 1) and (1, 1): eight columns, pi = 0 once, |pi| = 1, 2 twice
        assert n[1].tolist() == [512 * 8, 512 * 16, 512 * 16]
    # pi further than rp: the search radius is max(edges[-1], piedges[-1])
    with pytest.raises(ValueError, match='separation'):
        pair_counts(mesh(box), pos, [0.0, 1.0], mode='projected', pimax=5)
    pc = pair_counts(mesh(box), pos, [0.0, 1.0], mode='projected', pimax=4)
    check(pc, ref_pairs(pos, box, [0.0, 1.0], mode='projected', sub=numpy.arange(5.0)))


def test_identities(pbe):
    kw = RANDOM['uniform']
    pos, edges = kw['pos1'], kw['edges']
    pm = mesh(UNIT)
    b = edges[-1]
    w = wrap(pos, UNIT)
    # the count inside b
    within = count_core(w, w, numpy.asarray(UNIT), '1d', 2, numpy.array([0.0, b * b]), None, skip_diagonal=True)
    one = pair_counts(pm, pos, edges)
    assert int(cpu(one.npairs).sum()) == int(within['npairs'][0]) == int(cpu(pair_counts(pm, pos, [0, b]).npairs)[0])
    # auto = cross with a copy, less the n self pairs in bin (0, 0)
    t = torch.from_numpy(pos).to(pbe.device)
    cross = pair_counts(pm, t, edges, pos2=t.clone())
    want = cpu(cross.npairs).copy()
    want[0] -= len(pos)
    assert numpy.array_equal(cpu(one.npairs), want) and not cross.auto and cross.W2sum == 0.0
    # cross is symmetric under swapping the sets and the weights
    other = uniform(500, 3, 33)
    w1, w2 = dyadic_weights(700, 1), dyadic_weights(500, 2)
    ab = pair_counts(pm, pos, edges, pos2=other, weight1=w1, weight2=w2)
    ba = pair_counts(pm, other, edges, pos2=pos, weight1=w2, weight2=w1)
    assert torch.equal(ab.npairs, ba.npairs) and (ab.W1, ab.W2) == (ba.W2, ba.W1) == (w1.sum(), w2.sum())
    ref = ref_pairs(pos, UNIT, edges, pos2=other, w1=w1, w2=w2)
    check(ab, ref)
    check(ba, ref)
    # a 2d result summed over mu is the 1d result
    two = run_case(pbe, 'uniform-2d')
    assert numpy.array_equal(cpu(two.npairs).sum(axis=1), cpu(one.npairs))
    d = numpy.abs(cpu(two.rsum).sum(axis=1) - cpu(one.rsum))
    assert (d <= (cpu(one.npairs) + 4) * U * cpu(one.rsum)).all()


def test_weighted_exactly(pbe):
    """weights that are multiples of 1/8 in [1/8, 2] on rows of the 2^-12 lattice: wnpairs exactly, cross and auto, in
    float64 and float32 storage, in all three modes"""
    p1, p2 = lattice_rows(900, 3, 53), lattice_rows(800, 3, 54)
    w1, w2 = dyadic_weights(900, 55), dyadic_weights(800, 56)
    pm = mesh(UNIT)
    edges = [0.0, 1 / 32., 1 / 16., 3 / 32., 1 / 8.]
    for dtype in ('f8', 'f4'):
        a, b, u, v = p1.astype(dtype), p2.astype(dtype), w1.astype(dtype), w2.astype(dtype)
        assert numpy.array_equal(a.astype('f8'), p1) and numpy.array_equal(u.astype('f8'), w1)
        check(pair_counts(pm, a, edges, pos2=b, weight1=u, weight2=v), ref_pairs(p1, UNIT, edges, p2, w1, w2), True)
        check(pair_counts(pm, a, edges, weight1=u), ref_pairs(p1, UNIT, edges, w1=w1), True)
    check(pair_counts(pm, p1, edges, pos2=p2, weight1=w1, weight2=w2, mode='2d', muedges=[0, 0.5, 1]),
          ref_pairs(p1, UNIT, edges, p2, w1, w2, mode='2d', sub=[0, 0.5, 1]), True)
    check(pair_counts(pm, p1, edges, weight1=w1, mode='projected', piedges=[0, 1 / 16., 1 / 8.], los=0),
          ref_pairs(p1, UNIT, edges, w1=w1, mode='projected', sub=[0, 1 / 16., 1 / 8.], los=0), True)


def test_pair_correlation(pbe):
    """xi = wnpairs / RR - 1 on 2000 uniform rows, RR = (W1 W2 - sum w^2) V_bin / V_box formed here from the
    restatement's counts: within the bound of the sums carried through the division (and four ulps for the division
    and the subtraction)"""
    kw = RANDOM['xi']
    pos, edges = kw['pos1'], numpy.asarray(kw['edges'])
    ref = reference('xi')
    xi, pc = pair_correlation(mesh(UNIT), pos, edges)
    check(pc, ref)
    rr = (2000.0 * 2000.0 - 2000.0) * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    want = ref['wnpairs'] / rr - 1
    M, S = ref['npairs'].astype('f8'), ref['wnpairs'].copy()
    M[0] += 2000
    S[0] += 2000
    bound = (M + 4) * U * S / rr + 4 * U * (numpy.abs(ref['wnpairs'] / rr) + 1)
    assert xi.dtype == torch.float64 and (numpy.abs(cpu(xi) - want) <= bound).all()
    assert (numpy.abs(want) < 0.5).all()                        # uniform rows: no clustering beyond the shot noise
    # weighted cross counts in 2d: RR has no self term
    kw = RANDOM['weights-uniform']
    mu = numpy.linspace(0, 1, 4)
    xi, pc = pair_correlation(mesh(UNIT), kw['pos1'], kw['edges'], pos2=kw['pos2'], weight1=kw['w1'],
                              weight2=kw['w2'], mode='2d', muedges=mu)
    ref = ref_pairs(kw['pos1'], UNIT, kw['edges'], kw['pos2'], kw['w1'], kw['w2'], mode='2d', sub=mu)
    check(pc, ref)
    W1, W2 = kw['w1'].sum(), kw['w2'].astype('f8').sum()
    assert abs(pc.W1 - W1) <= 600 * U * W1 and abs(pc.W2 - W2) <= 500 * U * W2 and pc.W2sum == 0.0
    e = numpy.asarray(kw['edges'])
    rr = (pc.W1 * pc.W2 * 4 * numpy.pi / 3 * (e[1:] ** 3 - e[:-1] ** 3))[:, None] * numpy.diff(mu)[None, :]
    want = ref['wnpairs'].reshape(5, 3) / rr - 1
    bound = ((ref['npairs'] + 4) * U * ref['wnpairs']).reshape(5, 3) / rr + 8 * U * (numpy.abs(want) + 2)
    assert tuple(xi.shape) == (5, 3) and (numpy.abs(cpu(xi) - want) <= bound).all()


def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    for edges in ([0.1], [0.2, 0.1], [-0.1, 0.1], [0.0, numpy.nan], [0.0, numpy.inf], [[0.0, 0.1]], [0.1, 0.1]):
        with pytest.raises(ValueError, match='edges'):
            pair_counts(pm, pos, edges)
    with pytest.raises(ValueError, match='separation'):
        pair_counts(pm, pos, [0.0, 0.51])
    with pytest.raises(ValueError, match='separation'):
        pair_counts(mesh(SLAB), pos, [0.0, 0.13])              # 2 b > the shortest side
    assert tuple(pair_counts(mesh(SLAB), pos, [0.0, 0.125]).npairs.shape) == (1,)
    with pytest.raises(ValueError, match='shape'):
        pair_counts(pm, pos[:, :2], [0.0, 0.1])
    with pytest.raises(ValueError, match='shape'):
        pair_counts(pm, pos, [0.0, 0.1], pos2=pos.reshape(-1))
    with pytest.raises(TypeError):
        pair_counts(pm, (pos * 100).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='weight1'):
        pair_counts(pm, pos, [0.0, 0.1], weight1=numpy.ones(49))
    with pytest.raises(ValueError, match='weight2'):
        pair_counts(pm, pos, [0.0, 0.1], pos2=pos[:40], weight2=numpy.ones(50))
    with pytest.raises(ValueError, match='weight2'):
        pair_counts(pm, pos, [0.0, 0.1], weight2=numpy.ones(50))
    with pytest.raises(TypeError):
        pair_counts(pm, pos, [0.0, 0.1], weight1=numpy.ones(50, dtype='i4'))
    with pytest.raises(ValueError, match='mode'):
        pair_counts(pm, pos, [0.0, 0.1], mode='angular')
    for mode, kw in (('2d', dict(Nmu=4)), ('projected', dict(pimax=1))):
        with pytest.raises(ValueError, match='three dimensions'):
            pair_counts(mesh(UNIT[:2]), pos[:, :2], [0.0, 0.1], mode=mode, **kw)
        with pytest.raises(ValueError, match='los'):
            pair_counts(pm, pos, [0.0, 0.1], mode=mode, los=3, **kw)
        with pytest.raises(ValueError, match='needs'):
            pair_counts(pm, pos, [0.0, 0.1], mode=mode)
    for mu in ([0.1, 1.0], [0.0, 0.9], [0.0, 0.6, 0.5, 1.0]):
        with pytest.raises(ValueError, match='muedges'):
            pair_counts(pm, pos, [0.0, 0.1], mode='2d', muedges=mu)
    with pytest.raises(ValueError, match='piedges'):
        pair_counts(pm, pos, [0.0, 0.1], mode='projected', piedges=[0.01, 0.1])
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows'):
        pair_counts(pm, bad, [0.0, 0.1])
    with pytest.raises(ValueError, match='3 rows'):
        pair_counts(pm, bad, [0.0, 0.1], pos2=bad[5:8])
    with pytest.raises(NotImplementedError):
        pair_counts(mesh([1.0] * 4), numpy.zeros((3, 4)), [0.0, 0.1])
    # no rows at all
    empty = pair_counts(pm, numpy.zeros((0, 3)), [0.0, 0.1, 0.2])
    assert cpu(empty.npairs).tolist() == [0, 0] and numpy.isnan(cpu(empty.rmean)).all() and empty.W1 == 0.0
    assert cpu(pair_counts(pm, pos, [0.0, 0.1], pos2=numpy.zeros((0, 3))).npairs).tolist() == [0]


# ---- 3. ranks ------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """pair_counts on thread ranks holding both sets split unevenly (one rank holds no rows): what every rank got"""
    kw = RANDOM[name]
    p1, p2, w1, w2 = kw['pos1'], kw.get('pos2'), kw.get('w1'), kw.get('w2')
    s1 = split(len(p1), size)
    s2 = split(len(p2), size)[::-1] if p2 is not None else None
    mode, sub = kw.get('mode', '1d'), kw.get('sub')

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a = s1[comm.rank]
        c = s2[comm.rank] if p2 is not None else None
        pc = pair_counts(pm, p1[a], kw['edges'], pos2=None if p2 is None else p2[c],
                         weight1=None if w1 is None else w1[a], weight2=None if w2 is None else w2[c], mode=mode,
                         muedges=sub if mode == '2d' else None, piedges=sub if mode == 'projected' else None)
        return cpu(pc.npairs), cpu(pc.wnpairs), cpu(pc.rsum), pc.W1, pc.W2, pc.W2sum, len(p1[a])
    return thread_ranks(size, body)


def check_ranks(name, size, np_):
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
    """weighted cross, auto, and weighted 2d auto at b = 1/8 on the box [1, 0.5, 0.25] (with np = [2, 2] the block plus
    2 b covers the box along y and z): the arrays of every rank are identical and equal the restatement of all rows"""
    for name in ('ranks', 'ranks-auto', 'ranks-slab'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    for name in ('ranks', 'ranks-auto', 'ranks-slab'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
def test_more_secondaries_than_one_launch_counts(hipbe):
    """2^23 + 5000 secondaries: the entry launches once per window of 2^23 slots of the secondaries, and the cell that
    holds slot 2^23 is split between two launches.  No brute force at this size: the counts against all secondaries
    equal, exactly, the sum of the counts against their two halves (each within one launch), whatever the grids"""
    n2 = (1 << 23) + 5000
    dev = hipbe.device
    gen = torch.Generator(device=dev).manual_seed(5)
    p2 = torch.rand((n2, 3), generator=gen, device=dev, dtype=torch.float64)
    # a quarter of a primary per cell of side b: seven around every cell, the one that holds slot 2^23 among them
    p1 = torch.rand((1 << 15, 3), generator=gen, device=dev, dtype=torch.float64)
    pm = mesh(UNIT)
    edges = numpy.linspace(0.0, 0.02, 5)
    whole = pair_counts(pm, p1, edges, pos2=p2)
    half = n2 // 2
    parts = [pair_counts(pm, p1, edges, pos2=p2[:half]), pair_counts(pm, p1, edges, pos2=p2[half:])]
    assert int(cpu(whole.npairs).sum()) > 5000000
    assert torch.equal(whole.npairs, parts[0].npairs + parts[1].npairs)
    # and against the expectation of uniform rows, to a few standard deviations of the count
    want = len(p1) * n2 * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert (numpy.abs(cpu(whole.npairs) - want) < 6 * numpy.sqrt(want)).all()


@pytest.mark.parametrize('box', [UNIT, SLAB], ids=['unit', 'slab'])
@pytest.mark.parametrize('size,np_', RANKS)
def test_no_rank_receives_a_row_twice(obe, size, np_, box):
    """what the count over the ranks rests on: without ghosts every row goes to exactly one owner; with ghosts within
    b (up to L / 8) no rank receives a global index twice"""
    pos = uniform(900, 3, 47, box)
    parts = split(len(pos), size)
    b = min(box) / 2 if box is SLAB else 1 / 8.

    def body(comm):
        pm = mesh(box, comm, np_)
        dev = backend.get().device
        sl = parts[comm.rank]
        t = torch.from_numpy(pos[sl]).to(dev)
        gid = torch.arange(sl.start, sl.stop, dtype=torch.int64, device=dev)
        own = cpu(pm.decompose(t, smoothing=0).exchange(gid))
        smoothing = b * numpy.asarray(pm.Nmesh, dtype='f8') / numpy.asarray(box) * (1 + 1e-9)
        seen = cpu(pm.decompose(t, smoothing=smoothing).exchange(gid))
        assert len(numpy.unique(seen)) == len(seen)
        assert numpy.isin(own, seen).all()
        return own
    results = thread_ranks(size, body)
    owners = numpy.concatenate([results[r] for r in range(size)])
    assert numpy.array_equal(numpy.sort(owners), numpy.arange(len(pos)))


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank: a wrong shape, a wrong type, a coordinate that is not finite,
    2 b > L, a weight of the wrong length, too many bins"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        edges = [0.0, 0.05]
        with pytest.raises(ValueError):
            pair_counts(pm, mine[:, :2] if comm.rank == 1 else mine, edges)
        with pytest.raises(TypeError):
            pair_counts(pm, (mine * 8).astype('i8') if comm.rank == 2 else mine, edges)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            pair_counts(pm, bad, edges)
        with pytest.raises(ValueError, match='separation'):
            pair_counts(pm, mine, [0.0, 0.6])
        with pytest.raises(ValueError):
            pair_counts(pm, mine, edges, weight1=numpy.ones(29 if comm.rank == 1 else 30))
        with pytest.raises(ValueError):
            pair_counts(pm, mine, numpy.linspace(0, 0.05, MAX_BINS + (2 if comm.rank == 2 else 1)))
        assert int(cpu(pair_counts(pm, mine, edges).npairs)[0]) == int(ref_pairs(pos, UNIT, edges)['npairs'][0])
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 4. the ABI and the resources ----------------------------------------------------------------------------------------

def test_the_entry_is_bound():
    assert 'pair_counts' in _abi.DEVICE_ONLY and _abi.PMX_PAIRS_MAX_BINS >= 4096
    assert (_abi.PMX_PAIRS_1D, _abi.PMX_PAIRS_2D, _abi.PMX_PAIRS_PROJECTED) == (0, 1, 2)
    lib = backend.load_library()
    assert hasattr(lib, 'pmx_pair_counts')
    import pmesh_amd
    assert 'pair_counts' in pmesh_amd.__doc__


def test_pairs_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs.hip')
    # pairs_kernel<NDIM, MODE, WEIGHTED, SLOTS>: 1d for 1 to 3 dimensions, 2d and projected for 3; without and with
    # weights; 1024 and 4096 histogram slots
    assert len(t) == 20 and all('pairs_kernel' in k for k in t), sorted(t)
    for nd, mode in ((1, 0), (2, 0), (3, 0), (3, 1), (3, 2)):
        assert len([k for k in t if 'pairs_kernelILi%dELi%dE' % (nd, mode) in k]) == 4, sorted(t)
    for name, r in t.items():
        weighted, big = 'Lb1E' in name, 'Li4096E' in name
        assert r['ScratchSize'] == 0, (name, r)
        # two workgroups in the 160 KB of a CU at the least
        assert r['LDS'] <= 80 * 1024, (name, r)
        assert r['LDS'] <= ((80 if weighted else 52) if big else (24 if weighted else 16)) * 1024, (name, r)
        # measured at compile time: without weights 25 (1-d rows) to 40 (2d), with weights 30 to 44
        assert r['VGPRs'] <= (48 if weighted else 40), (name, r)
    # and moving the cell helpers into pmx_cells_dev.h left the FoF kernels where they were
    link = [r for k, r in resources('pmx_fof.hip').items() if 'link_kernel' in k]
    assert len(link) == 3 and all(r['VGPRs'] <= 48 and r['LDS'] == 0 and r['ScratchSize'] == 0 for r in link)
