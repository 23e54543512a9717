"""pmesh_amd.pairvel (csrc/pmx_pairs_vel.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/pairvel.py, include/pmesh_amd.h).  The modes 7 (PMX_PAIRS_1D_VELOCITY), 8
(PMX_PAIRS_PROJECTED_VELOCITY) and 9 (PMX_PAIRS_1D_LOS) of pmx_pair_counts share rows, wrapping, the minimum image
dx_d (primary minus secondary), r2, q, the squared edges, the r-bin, the pi-bin and the pimax cut with the modes 1d,
projected and 1d of pmesh_amd.paircount.  Both sets bring a block of columns, (w, v_0 .. v_{ndim-1}) or (w, s).  Per
counted pair, w = w1_i * w2_j:
  7  dv_d = v_i,d - v_j,d; h = sum_d dx_d dv_d and dv2 = sum_d dv_d^2 in the order d = 0, 1, 2; r = sqrt(r2); u = h / r
     where r2 > 0, else 0; S1 += (w u), S2 += (w u) u, S3 += w dv2
  8  u = dx_los < 0 ? -dv_los : dv_los; S1, S2, S3 as above, dv2 over all three axes; the m = 0 sum adds w sqrt(rp2)
  9  o_d = 0.5 L_d; a_d = w_i,d - o_d, b_d = w_j,d - o_d; a2, b2, pa = dx.a, pb = dx.b summed over d = 0, 1, 2 in order;
     ta = a2 > 0 ? pa / sqrt(a2) : 0, tb likewise; c = r2 > 0 ? 0.5 * ((ta + tb) / r) : 0; ds = s_i - s_j;
     S1 += (w c) ds, S2 += (w c) c, S3 += (w ds) ds
rsum[m * nbins + b]: m = 0 the sum of w sqrt(q), m = 1, 2, 3 the sums S1, S2, S3.

The restatement (vel_core) is brute force over the full (n1, n2) matrix: exactly these operations, in this order, in
float64.  npairs, wnpairs, the m = 0 sum and the margin are those of tests.test_paircount.count_core itself, called on
the same rows with the base mode; the bin of every pair is formed with count_core's comparisons and is held to
count_core's npairs bin by bin before anything is summed into it.  Under -m "not gpu" the restatement serves the three
modes of pmx_pair_counts (VelOracleBackend; the other modes go to its parents), so the host layer and the thread ranks
run without a GPU; under -m gpu the kernel is compared with it.

No tolerance is new.  npairs is compared by equality, with the restatement and with pair_counts of the same arguments
in the base mode.  Each of the five double sums is compared per bin within the bound of tests.test_paircount.check,
|got - ref| <= (M + 4) 2^-52 S: M the pairs of the bin, S the sum of the absolute values of that sum's terms; the terms
are the rule's, only the order of addition differs.  wnpairs and S3 are compared by equality where the rows lie on a
2^-12 lattice, the weights are multiples of 1/8 in [1/8, 2] and the velocities multiples of 1/8 below 16 in magnitude:
every term and every partial sum is then exact.  Random inputs keep every pair at least 1e-9 (relative) from an edge
by the margin count_core reports; test_inputs_are_decided asserts it without a GPU for every random input.
"""
import os

import numpy
import pytest
import torch

import pmesh_amd
from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid, cell_sort
from pmesh_amd.paircount import VELOCITY_MODES, PairCounts, local_counts, pair_counts
from pmesh_amd.pairvel import MAX_BINS, PairwiseLOS, PairwiseVelocities, pairwise_los, pairwise_velocities
from tests.test_fof import GRIDS, RANKS, SLAB, UNIT, crowded, face_pairs, mesh, split, thread_ranks, uniform, wrap
from tests.test_lpt import cpu
from tests.test_paircount import U, PairsOracleBackend, count_core, dyadic_weights, grid_of, lattice_rows

BASE = {'1d-velocity': '1d', 'projected-velocity': 'projected', '1d-los': '1d'}
CODES = {v: k for k, v in VELOCITY_MODES.items()}
WAVE_NS = [1, 63, 64, 65, 255, 256, 257, 513]


# ---- the restatement -----------------------------------------------------------------------------------------------

def vel_core(w1, w2, box, kernel, los, e2, sub, blk1, blk2, skip_diagonal=False):
    """The sums over the pairs of the wrapped rows w1 with w2 and their blocks of columns blk1, blk2 (float64).  kernel:
    a key of VELOCITY_MODES.  Returns a dict: npairs (flat), sums (5, nbins): w, w sqrt(q), S1, S2, S3; abs (5, nbins):
    the sums of the absolute values of their terms; margin (count_core's)."""
    base = BASE[kernel]
    blk1, blk2 = numpy.asarray(blk1, dtype='f8'), numpy.asarray(blk2, dtype='f8')
    n1, n2, nd = len(w1), len(w2), w1.shape[1]
    assert blk1.shape == (n1, 2 if kernel == '1d-los' else 1 + nd) and blk2.shape == (n2, blk1.shape[1])
    core = count_core(w1, w2, box, base, los, e2, sub, blk1[:, 0], blk2[:, 0], skip_diagonal=skip_diagonal)
    nr, nsub = len(e2) - 1, (1 if base == '1d' else len(sub) - 1)
    nbins = nr * nsub
    out = dict(npairs=core['npairs'], margin=core['margin'], sums=numpy.zeros((5, nbins)), abs=numpy.zeros((5, nbins)))
    if n1 == 0 or n2 == 0:
        return out
    dx = []
    for d in range(nd):
        x = w1[:, None, d] - w2[None, :, d]
        dx.append(x - box[d] * numpy.rint(x / box[d]))
    q = numpy.zeros((n1, n2))
    for d in range(nd):
        if base != 'projected' or d != los:
            q = q + dx[d] * dx[d]
    keep = (q >= e2[0]) & (q < e2[-1])
    if skip_diagonal:
        keep &= ~numpy.eye(n1, n2, dtype=bool)
    rbin = numpy.searchsorted(e2, q, side='right') - 1
    sbin = numpy.zeros((n1, n2), dtype='i8')
    if base == 'projected':
        a = numpy.abs(dx[los])
        for k in range(1, nsub):
            sbin += a >= sub[k]
        keep &= a < sub[-1]
    flat = (rbin * nsub + sbin)[keep]
    # the decisions are count_core's
    assert numpy.array_equal(numpy.bincount(flat, minlength=nbins), core['npairs'])
    w = blk1[:, 0][:, None] * blk2[:, 0][None, :]
    r = numpy.sqrt(q)
    with numpy.errstate(divide='ignore', invalid='ignore'):
        if kernel == '1d-los':
            o = 0.5 * numpy.asarray(box, dtype='f8')
            av, bv = w1 - o[None, :], w2 - o[None, :]
            a2, b2 = numpy.zeros(n1), numpy.zeros(n2)
            pa, pb = numpy.zeros((n1, n2)), numpy.zeros((n1, n2))
            for d in range(3):
                a2 = a2 + av[:, d] * av[:, d]
                b2 = b2 + bv[:, d] * bv[:, d]
                pa = pa + dx[d] * av[:, None, d]
                pb = pb + dx[d] * bv[None, :, d]
            ta = numpy.where((a2 > 0)[:, None], pa / numpy.sqrt(a2)[:, None], 0.0)
            tb = numpy.where((b2 > 0)[None, :], pb / numpy.sqrt(b2)[None, :], 0.0)
            c = numpy.where(q > 0, 0.5 * ((ta + tb) / r), 0.0)
            ds = blk1[:, 1][:, None] - blk2[:, 1][None, :]
            terms = [w, w * r, (w * c) * ds, (w * c) * c, (w * ds) * ds]
        else:
            dv = [blk1[:, 1 + d][:, None] - blk2[:, 1 + d][None, :] for d in range(nd)]
            h, dv2 = numpy.zeros((n1, n2)), numpy.zeros((n1, n2))
            for d in range(nd):
                h = h + dx[d] * dv[d]
                dv2 = dv2 + dv[d] * dv[d]
            if base == 'projected':
                u = numpy.where(dx[los] < 0, -dv[los], dv[los])
            else:
                u = numpy.where(q > 0, h / r, 0.0)
            terms = [w, w * r, w * u, (w * u) * u, w * dv2]
    for m, t in enumerate(terms):
        out['sums'][m] = numpy.bincount(flat, weights=t[keep], minlength=nbins)
        out['abs'][m] = numpy.bincount(flat, weights=numpy.abs(t)[keep], minlength=nbins)
    assert numpy.array_equal(out['sums'][0], core['wnpairs']) and numpy.array_equal(out['sums'][1], core['rsum'])
    return out


def block(n, cols, w=None):
    """the (n, 1 + ncol) float64 block (w, columns) of one set"""
    cols = numpy.asarray(cols).astype('f8').reshape(n, -1)
    w = numpy.ones(n) if w is None else numpy.asarray(w).astype('f8')
    return numpy.concatenate([w.reshape(n, 1), cols], axis=1)


def ref_vel(kernel, pos1, box, edges, cols1, pos2=None, cols2=None, w1=None, w2=None, sub=None, los=2):
    """the restatement of pairwise_velocities / pairwise_los(mesh(box), pos1, cols1, edges, pos2, cols2, w1, w2, ...)
    about an observer at the box centre"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    s = None if sub is None else numpy.asarray(sub, dtype='f8')
    a = wrap(numpy.asarray(pos1).astype('f8'), box)
    auto = pos2 is None
    b1 = block(len(a), cols1, w1)
    out = vel_core(a, a if auto else wrap(numpy.asarray(pos2).astype('f8'), box), box, kernel, los, e * e, s, b1,
                   b1 if auto else block(len(pos2), cols2, w2), skip_diagonal=auto)
    # what the device may have added on top: the self pairs of the auto form, in bin (0, 0) of npairs and wnpairs
    out['nself'], out['wself'] = 0, 0.0
    if auto and e[0] == 0:
        out['nself'], out['wself'] = len(a), float((b1[:, 0] ** 2).sum())
    return out


class VelOracleBackend(PairsOracleBackend):
    """the CPU test double with the three velocity modes of pmx_pair_counts served by the restatement"""
    name = 'oracle-pairvel'

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
        assert nbins <= MAX_BINS and npairs.numel() == wnpairs.numel() == nbins and rsum.numel() == 4 * nbins
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell))
        ncol = 2 if CODES[mode] == '1d-los' else 1 + nd
        for w, n in ((weight1, n1), (weight2, n2)):
            assert tuple(w.shape) == (n, ncol) and w.is_contiguous() and w.dtype in (torch.float32, torch.float64)
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = vel_core(a, b, numpy.asarray(boxsize, dtype='f8'), CODES[mode], los, e2.numpy(),
                       None if sub is None else sub.numpy(), weight1.numpy(), weight2.numpy())
        npairs += torch.from_numpy(got['npairs'])
        wnpairs += torch.from_numpy(got['sums'][0])
        rsum += torch.from_numpy(got['sums'][1:].reshape(-1))


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(VelOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def vbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(VelOracleBackend())
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


def arrays(got):
    """(npairs, the five sums as a (5, nbins) array) of a result of pairvel, or of the flat triple of local_counts"""
    if isinstance(got, PairwiseVelocities):
        got = (got.npairs, got.wnpairs, torch.stack([got.rsum, got.vsum, got.v2sum, got.dv2sum]))
    elif isinstance(got, PairwiseLOS):
        got = (got.npairs, got.wnpairs, torch.stack([got.rsum, got.num, got.den, got.ds2sum]))
    n, wn, rs = [(x if isinstance(x, numpy.ndarray) else cpu(x)) for x in got]
    assert n.dtype == numpy.int64 and wn.dtype == rs.dtype == numpy.float64
    n, wn = n.reshape(-1), wn.reshape(-1)
    return n, numpy.concatenate([wn[None, :], rs.reshape(4, len(n))])


def check_vel(got, ref, exact=False, factor=1, what=''):
    """a result against the restatement's dict: npairs by equality; every sum per bin within `factor` times the bound
    of tests.test_paircount.check; exact: wnpairs and S3 by equality"""
    n, sums = arrays(got)
    assert numpy.array_equal(n, ref['npairs']), (what, n[:8], ref['npairs'][:8])
    M = ref['npairs'].astype('f8')
    S = ref['abs'].copy()
    M[0] += ref.get('nself', 0)
    S[0, 0] += ref.get('wself', 0.0)
    for m in range(5):
        if exact and m in (0, 4):
            assert numpy.array_equal(sums[m], ref['sums'][m]), (what, m)
        else:
            d = numpy.abs(sums[m] - ref['sums'][m])
            assert (d <= factor * (M + 4) * U * S[m]).all(), (what, m, d.max())


def dyadic_vel(n, ncol, seed):
    """multiples of 1/8 below 16 in magnitude"""
    return numpy.random.RandomState(seed).randint(-127, 128, size=(n, ncol)) / 8.0


def normal_vel(n, ncol, seed):
    return numpy.random.RandomState(seed).normal(size=(n, ncol))


def padded(n, seed, b, box=UNIT):
    """uniform rows in the interior [b / 2, L - b / 2) that the mode 9 asks for"""
    box = numpy.asarray(box, dtype='f8')
    return b / 2 + uniform(n, 3, seed) * (box - b) * (1 - 2.0 ** -20)


def dev_t(be, x):
    return None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(be.device)


# ---- the inputs ----------------------------------------------------------------------------------------------------

def wave_b(n1, n2):
    return min(0.45, 0.6 * max(n1, n2, 1) ** (-1 / 3.))


def wave_case(kernel, n1, n2, form):
    """rows, columns, edges and their storage: form 'f8' (all float64), 'f4' (all float32), 'mixed' (float32 rows with
    float64 columns in the first set, float64 rows with float32 columns in the second)"""
    b = wave_b(n1, n2)
    ncol = 1 if kernel == '1d-los' else 3
    types = {'f8': ('f8',) * 4, 'f4': ('f4',) * 4, 'mixed': ('f4', 'f8', 'f8', 'f4')}[form]
    kw = dict(pos1=padded(n1, 300 + n1, b).astype(types[0]), cols1=normal_vel(n1, ncol, 310 + n1).astype(types[1]),
              pos2=padded(n2, 500 + n2, b).astype(types[2]), cols2=normal_vel(n2, ncol, 510 + n2).astype(types[3]),
              w1=numpy.random.RandomState(320 + n1).uniform(0.5, 1.5, n1).astype(types[1]),
              w2=numpy.random.RandomState(520 + n2).uniform(0.5, 1.5, n2).astype(types[3]), box=UNIT,
              edges=numpy.array([0.0, 0.4 * b, 0.8 * b, b]))
    if kernel == 'projected-velocity':
        kw.update(sub=[0.0, 0.3 * b, 0.9 * b], los=1)
    return kw


def wave_pairs(kernel):
    """mode 7: n1 and n2 independently; modes 8 and 9: n1 == n2 and the pairs of neighbouring sizes"""
    if kernel == '1d-velocity':
        return [(a, b) for a in WAVE_NS for b in WAVE_NS]
    return [(a, a) for a in WAVE_NS] + [(WAVE_NS[k], WAVE_NS[k + 1]) for k in range(len(WAVE_NS) - 1)]


def bins_case(nr, seed):
    return dict(pos1=uniform(700, 3, seed), cols1=normal_vel(700, 3, seed + 1), box=UNIT,
                edges=numpy.linspace(0.0, 0.15, nr + 1))


def hubble_case():
    """rows inside a quarter of the box with v = H x"""
    pos = 0.3 + 0.25 * uniform(600, 3, 81)
    return dict(pos1=pos, cols1=0.7 * pos, box=UNIT, edges=numpy.linspace(0.0, 0.1, 6))


def random_cases():
    """name -> (kernel, keyword arguments of ref_vel): every random input of the tests below"""
    cases = {}
    for kernel in sorted(VELOCITY_MODES):
        for form in ('f8', 'f4', 'mixed'):
            for n1, n2 in wave_pairs(kernel):
                cases['wave-%s-%d-%d-%s' % (kernel, n1, n2, form)] = (kernel, wave_case(kernel, n1, n2, form))
            for n in WAVE_NS:
                kw = wave_case(kernel, n, n, form)
                cases['wave-auto-%s-%d-%s' % (kernel, n, form)] = (kernel, dict(kw, pos2=None, cols2=None, w2=None))
    for nd in (3, 2, 1):
        rows = numpy.concatenate([face_pairs(SLAB[:nd], 0.05), uniform(300, nd, 61, SLAB[:nd])])
        cases['faces-%dd' % nd] = ('1d-velocity', dict(pos1=rows, cols1=normal_vel(len(rows), nd, 62), box=SLAB[:nd],
                                                       edges=[0.0, 0.02, 0.04, 0.05]))
    rows = numpy.concatenate([face_pairs(SLAB, 0.05), uniform(300, 3, 61, SLAB)])
    cases['faces-projected'] = ('projected-velocity', dict(pos1=rows, cols1=normal_vel(len(rows), 3, 63), box=SLAB,
                                                           edges=[0.0, 0.02, 0.04, 0.05], sub=[0.0, 0.01, 0.05], los=0))
    cases['faces-los'] = ('1d-los', dict(pos1=rows, cols1=normal_vel(len(rows), 1, 64), box=SLAB,
                                         edges=[0.0, 0.02, 0.04, 0.05]))
    cases['open'] = ('1d-velocity', dict(pos1=uniform(2000, 3, 12), cols1=normal_vel(2000, 3, 13), box=UNIT,
                                         edges=[0.01, 0.03, 0.05]))
    for nd in (2, 1):
        cases['dim-%d' % nd] = ('1d-velocity', dict(pos1=uniform(1500, nd, 70), cols1=normal_vel(1500, nd, 71),
                                                    pos2=uniform(1200, nd, 72), cols2=normal_vel(1200, nd, 73),
                                                    w1=numpy.random.RandomState(74).uniform(0.5, 1.5, 1500),
                                                    box=UNIT[:nd], edges=numpy.linspace(0.0, 0.05 if nd == 2 else 0.01, 10)))
    for nr in (1, 128, 129, 1024):
        cases['bins-%d' % nr] = ('1d-velocity', bins_case(nr, 200 + nr))
    for los in (0, 1, 2):
        cases['bins-32x32-los%d' % los] = ('projected-velocity', dict(
            pos1=uniform(700, 3, 240 + los), cols1=normal_vel(700, 3, 250 + los), box=UNIT,
            edges=numpy.linspace(0.0, 0.15, 33), sub=numpy.linspace(0.0, 0.15, 33), los=los))
    cases['bins-1024-los'] = ('1d-los', dict(pos1=padded(700, 260, 0.15), cols1=normal_vel(700, 1, 261), box=UNIT,
                                             edges=numpy.linspace(0.0, 0.15, 1025)))
    cases['crowded'] = ('1d-velocity', dict(pos1=crowded(), cols1=normal_vel(len(crowded()), 3, 90), box=UNIT,
                                            edges=numpy.linspace(0.0, 0.05, 5)))
    cases['crowded-los'] = ('1d-los', dict(pos1=crowded(), cols1=normal_vel(len(crowded()), 1, 91), box=UNIT,
                                           edges=numpy.linspace(0.0, 0.05, 5)))
    cases['hubble'] = ('1d-velocity', hubble_case())
    rng = numpy.random.RandomState(95)
    cases['independent'] = ('1d-velocity', dict(pos1=uniform(800, 3, 94), cols1=1.5 * rng.normal(size=(800, 3)),
                                                box=UNIT, edges=numpy.linspace(0.08, 0.2, 5)))
    cases['ranks'] = ('1d-velocity', dict(pos1=uniform(900, 3, 44), cols1=normal_vel(900, 3, 46), pos2=uniform(700, 3, 45),
                                          cols2=normal_vel(700, 3, 47), box=UNIT, edges=numpy.linspace(0, 0.1, 5),
                                          w1=numpy.random.RandomState(7).uniform(0.5, 1.5, 900),
                                          w2=numpy.random.RandomState(8).uniform(0.5, 1.5, 700)))
    cases['ranks-slab'] = ('projected-velocity', dict(pos1=uniform(900, 3, 46, SLAB), cols1=normal_vel(900, 3, 48),
                                                      box=SLAB, edges=[0.0, 0.05, 0.1, 0.125], sub=[0.0, 0.03, 0.1],
                                                      w1=numpy.random.RandomState(9).uniform(0.5, 1.5, 900)))
    cases['ranks-los'] = ('1d-los', dict(pos1=padded(900, 49, 0.1), cols1=normal_vel(900, 1, 50), box=UNIT,
                                         edges=numpy.linspace(0, 0.1, 5)))
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        kernel, kw = RANDOM[name]
        _REFERENCE[name] = ref_vel(kernel, **kw)
    return _REFERENCE[name]


def run(be, kernel, kw):
    """pairwise_velocities or pairwise_los of the keyword arguments of ref_vel, on one rank or on the rank of `pm`"""
    kw = dict(kw)
    pm = kw.pop('pm', None) or mesh(kw['box'])
    t = lambda x: dev_t(be, x)
    if kernel == '1d-los':
        return pairwise_los(pm, t(kw['pos1']), t(kw['cols1']), kw['edges'], pos2=t(kw.get('pos2')),
                            s2=t(kw.get('cols2')), weight1=t(kw.get('w1')), weight2=t(kw.get('w2')))
    return pairwise_velocities(pm, t(kw['pos1']), t(kw['cols1']), kw['edges'], pos2=t(kw.get('pos2')),
                               vel2=t(kw.get('cols2')), weight1=t(kw.get('w1')), weight2=t(kw.get('w2')),
                               mode=BASE[kernel], piedges=kw.get('sub'), los=kw.get('los', 2))


def base_counts(kernel, kw):
    """pair_counts of the same arguments in the base mode"""
    return pair_counts(mesh(kw['box']), kw['pos1'], kw['edges'], pos2=kw.get('pos2'), weight1=kw.get('w1'),
                       weight2=kw.get('w2'), mode=BASE[kernel], piedges=kw.get('sub'), los=kw.get('los', 2))


def run_local(be, kernel, kw, grid, pos1=None, cols1=None, pos2=None, cols2=None):
    """local_counts on a forced grid with unit weights: the flat triple"""
    dev = be.device
    e = numpy.asarray(kw['edges'], dtype='f8')
    p1 = kw['pos1'] if pos1 is None else pos1
    c1 = kw['cols1'] if cols1 is None else cols1
    sub = None if kw.get('sub') is None else torch.from_numpy(numpy.asarray(kw['sub'], dtype='f8')).to(dev)
    return local_counts(be, kernel, kw.get('los', 2), torch.from_numpy(p1).to(dev),
                        torch.from_numpy(block(len(p1), c1)).to(dev),
                        None if pos2 is None else torch.from_numpy(pos2).to(dev),
                        None if pos2 is None else torch.from_numpy(block(len(pos2), cols2)).to(dev), grid, kw['box'],
                        torch.from_numpy(e * e).to(dev), sub)


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_on_known_answers():
    """two rows at distance 0.3 along x, moving apart at 2 and sideways at 1: u = 2, dv2 = 5; along the line of sight x
    u = 2 as well, along y the pair has dx_los == 0 and u = dv_y = +1 for one order and -1 for the other"""
    pos = numpy.array([[0.2, 0.5, 0.5], [0.5, 0.5, 0.5]])
    vel = numpy.array([[-1.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
    got = ref_vel('1d-velocity', pos, UNIT, [0.0, 0.4], vel)
    assert got['npairs'].tolist() == [2] and got['nself'] == 2
    assert numpy.abs(got['sums'][:, 0] - [2, 0.6, 4, 8, 10]).max() < 1e-15
    got = ref_vel('projected-velocity', pos, UNIT, [0.0, 0.1], vel, sub=[0.0, 0.4], los=0)
    assert got['npairs'].tolist() == [2] and numpy.abs(got['sums'][:, 0] - [2, 0, 4, 8, 10]).max() < 1e-15
    got = ref_vel('projected-velocity', pos, UNIT, [0.0, 0.4], vel, sub=[0.0, 0.1], los=1)
    assert got['npairs'].tolist() == [2] and got['sums'][2:, 0].tolist() == [0.0, 2.0, 10.0]


def decided(names):
    for name in names:
        kernel, kw = RANDOM[name]
        ref = reference(name)
        assert ref['margin'] >= 1e-9, (name, ref['margin'])
        b = max(kw['edges'][-1], kw['sub'][-1]) if kernel == 'projected-velocity' else kw['edges'][-1]
        assert 2 * b <= min(kw['box']) and len(kw['pos1']) <= 2500
        if kernel == '1d-los' and not name.startswith('faces'):
            box = numpy.asarray(kw['box'])
            for p in (kw['pos1'], kw.get('pos2')):
                assert p is None or ((p >= b / 2) & (p < box - b / 2)).all(), name


@pytest.mark.parametrize('kernel', sorted(VELOCITY_MODES))
@pytest.mark.parametrize('form', ['f8', 'f4', 'mixed'])
def test_wave_inputs_are_decided(kernel, form):
    names = [n for n in sorted(RANDOM) if n.startswith('wave') and '-%s-' % kernel in n and n.endswith('-' + form)]
    assert len(names) >= 23
    decided(names)


def test_inputs_are_decided():
    names = [n for n in sorted(RANDOM) if not n.startswith('wave')]
    assert len(names) >= 20
    decided(names)
    for name in names:
        if not name.startswith('crowded'):
            assert (reference(name)['npairs'] > 0).sum() >= min(len(reference(name)['npairs']), 3), name


# ---- 2. known answers ----------------------------------------------------------------------------------------------------

def test_known_answers(vbe):
    pm = mesh(UNIT)
    # two rows approaching head-on along x across the periodic face: the minimum image is used, dx = -+0.1, and u = -3
    pos = numpy.array([[0.95, 0.5, 0.5], [0.05, 0.5, 0.5]])
    vel = numpy.array([[1.0, 0.0, 0.0], [-2.0, 0.0, 0.0]])
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.2])
    assert isinstance(pv, PairwiseVelocities) and isinstance(pv, PairCounts) and pv.auto and pv.mode == '1d'
    assert cpu(pv.npairs).tolist() == [2] and cpu(pv.wnpairs).tolist() == [2.0]
    check_vel(pv, ref_vel('1d-velocity', pos, UNIT, [0.0, 0.2], vel))
    # (dx = 0.95 - 0.05 - 1 is not exactly -0.1: a few roundings on u = 3 dx / |dx|, their square root on the dispersions)
    assert abs(cpu(pv.v12)[0] + 3) <= 12 * U and abs(cpu(pv.rmean)[0] - 0.1) <= 4 * U
    assert cpu(pv.sigma_par)[0] <= 3 * numpy.sqrt(8 * U) and cpu(pv.sigma_perp)[0] <= 3 * numpy.sqrt(8 * U)
    # a pair at right angles to its velocity difference: u == 0, dv2sum > 0
    vel = numpy.array([[0.0, 1.0, 0.0], [0.0, -1.0, 2.0]])
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.2])
    assert cpu(pv.vsum).tolist() == [0.0] and cpu(pv.v2sum).tolist() == [0.0] and cpu(pv.dv2sum).tolist() == [16.0]
    assert cpu(pv.v12).tolist() == [0.0] and cpu(pv.sigma_perp).tolist() == [2.0]
    # two distinct coincident rows: counted in bin 0 when edges[0] == 0, u == 0 by the rule; not with edges[0] > 0
    pos = numpy.array([[0.3, 0.4, 0.5], [0.3, 0.4, 0.5], [0.9, 0.9, 0.9]])
    vel = numpy.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [5.0, 5.0, 5.0]])
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.1, 0.2])
    assert cpu(pv.npairs).tolist() == [2, 0] and cpu(pv.wnpairs).tolist() == [2.0, 0.0]
    assert cpu(pv.vsum).tolist() == [0.0, 0.0] and cpu(pv.dv2sum).tolist() == [10.0, 0.0]
    assert numpy.isnan(cpu(pv.v12)[1]) and numpy.isnan(cpu(pv.sigma_par)[1]) and numpy.isnan(cpu(pv.sigma_perp)[1])
    assert cpu(pairwise_velocities(pm, pos, vel, [1e-6, 0.1]).npairs).tolist() == [0]
    # the same in the cross form with a copy: the three self pairs are pairs, and add nothing to S1 .. S3
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.1], pos2=pos.copy(), vel2=vel.copy())
    assert cpu(pv.npairs).tolist() == [5] and cpu(pv.dv2sum).tolist() == [10.0] and not pv.auto
    # a pair with dx_los == 0 in the projected mode: u = +dv_los for both orders, so the two cancel
    pos = numpy.array([[0.2, 0.5, 0.5], [0.5, 0.5, 0.5]])
    vel = numpy.array([[-1.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.4], mode='projected', piedges=[0.0, 0.1], los=1)
    assert pv.mode == 'projected' and pv.los == 1 and tuple(pv.npairs.shape) == (1, 1) and pv.piedges.tolist() == [0, 0.1]
    assert cpu(pv.npairs).tolist() == [[2]] and cpu(pv.vsum).tolist() == [[0.0]] and cpu(pv.v2sum).tolist() == [[2.0]]
    assert cpu(pv.dv2sum).tolist() == [[10.0]] and cpu(pv.sigma_par).tolist() == [[1.0]]
    # along x: both orders have u = +2 (the pair recedes); rmean is that of rp = 0
    pv = pairwise_velocities(pm, pos, vel, [0.0, 0.1], mode='projected', piedges=[0.0, 0.4], los=0)
    assert cpu(pv.v12).tolist() == [[2.0]] and cpu(pv.rmean).tolist() == [[0.0]]
    check_vel(pv, ref_vel('projected-velocity', pos, UNIT, [0.0, 0.1], vel, sub=[0.0, 0.4], los=0))


def test_known_answers_of_the_line_of_sight_estimator(vbe):
    """two rows on one ray from the observer: c = +-1 and v12 = ds / c, the scalar difference signed by the order along
    the ray; two rows symmetric about the observer's direction: c == 0, nothing in num and den, v12 nan; an observer off
    the centre"""
    pm = mesh(UNIT)
    pos = numpy.array([[0.5, 0.5, 0.625], [0.5, 0.5, 0.75]])
    s = numpy.array([1.0, 4.0])
    ks = pairwise_los(pm, pos, s, [0.0, 0.25])
    assert isinstance(ks, PairwiseLOS) and ks.los == 'observer' and ks.observer.tolist() == [0.5, 0.5, 0.5] and ks.auto
    assert cpu(ks.npairs).tolist() == [2] and cpu(ks.num).tolist() == [6.0] and cpu(ks.den).tolist() == [2.0]
    assert cpu(ks.ds2sum).tolist() == [18.0] and cpu(ks.v12).tolist() == [3.0] and cpu(ks.rmean).tolist() == [0.125]
    # symmetric about the ray along z: a = (-d, 0, h), b = (d, 0, h): dx.a / |a| + dx.b / |b| = 0
    pos = numpy.array([[0.375, 0.5, 0.75], [0.625, 0.5, 0.75]])
    ks = pairwise_los(pm, pos, s, [0.0, 0.3])
    assert cpu(ks.npairs).tolist() == [2] and cpu(ks.num).tolist() == [0.0] and cpu(ks.den).tolist() == [0.0]
    assert cpu(ks.ds2sum).tolist() == [18.0] and numpy.isnan(cpu(ks.v12)[0])
    check_vel(ks, ref_vel('1d-los', pos, UNIT, [0.0, 0.3], s))
    # the observer elsewhere: the rows are shifted so that it sits at the centre
    obs = numpy.array([0.25, 0.5, 0.5])
    pos = numpy.array([[0.375, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 0.375, 0.5]])
    s3 = numpy.array([1.0, 4.0, 2.0])
    ks = pairwise_los(pm, pos, s3, [0.0, 0.15], observer=obs, weight1=numpy.array([2.0, 0.5, 1.0]))
    assert ks.observer.tolist() == obs.tolist() and cpu(ks.npairs).tolist() == [2]
    check_vel(ks, ref_vel('1d-los', pos + (0.5 - obs), UNIT, [0.0, 0.15], s3, w1=[2.0, 0.5, 1.0]))
    assert cpu(ks.v12).tolist() == [3.0] and cpu(ks.wnpairs).tolist() == [2.0]
    # a row outside the padded interior is refused, as by survey_pair_counts
    with pytest.raises(ValueError, match='outside'):
        pairwise_los(pm, numpy.array([[0.5, 0.5, 0.99], [0.5, 0.5, 0.9]]), s, [0.0, 0.25])


# ---- 3. the kernel's paths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', ['f8', 'f4', 'mixed'])
@pytest.mark.parametrize('kernel', sorted(VELOCITY_MODES))
def test_wave_and_workgroup_edges(vbe, kernel, form):
    """n1 and n2 from 1, 63, 64, 65, 255, 256, 257 and 513 rows, cross and auto, float64 and float32 rows and columns and
    a mixture of them, weights on both sides; npairs is that of pair_counts in the base mode"""
    for n1, n2 in wave_pairs(kernel):
        name = 'wave-%s-%d-%d-%s' % (kernel, n1, n2, form)
        got = run(vbe, kernel, RANDOM[name][1])
        check_vel(got, reference(name), what=name)
        if n1 == n2:
            assert torch.equal(got.npairs, base_counts(kernel, RANDOM[name][1]).npairs)
            name = 'wave-auto-%s-%d-%s' % (kernel, n1, form)
            check_vel(run(vbe, kernel, RANDOM[name][1]), reference(name), what=name)


@pytest.mark.parametrize('name', ['dim-2', 'dim-1', 'bins-1', 'bins-128', 'bins-129', 'bins-1024', 'bins-32x32-los0',
                                  'bins-32x32-los1', 'bins-32x32-los2', 'bins-1024-los', 'hubble', 'independent'])
def test_random_cases(vbe, name):
    """mode 7 in two and one dimensions (cross, weights on one side); 1 bin, 128 and 129 (edges in LDS and in global
    memory) and 1024 = PMX_PAIRS_VELOCITY_MAX_BINS bins in mode 7 and mode 9; 32 x 32 in mode 8 for every line of sight;
    npairs is that of pair_counts in the base mode"""
    kernel, kw = RANDOM[name]
    got = run(vbe, kernel, kw)
    nr = len(kw['edges']) - 1
    assert tuple(got.npairs.shape) == ((nr,) if kw.get('sub') is None else (nr, len(kw['sub']) - 1))
    assert got.npairs.shape == got.wnpairs.shape == got.rsum.shape == got.rmean.shape == got.v12.shape
    if '1024' in name or '32x32' in name:
        assert got.npairs.numel() == MAX_BINS == 1024
    check_vel(got, reference(name), what=name)
    assert torch.equal(got.npairs, base_counts(kernel, kw).npairs)


def test_too_many_bins(obe):
    pm, pos = mesh(UNIT), uniform(50, 3, 1)
    with pytest.raises(ValueError, match='bins'):
        pairwise_velocities(pm, pos, pos, numpy.linspace(0, 0.2, MAX_BINS + 2))
    with pytest.raises(ValueError, match='bins'):
        pairwise_velocities(pm, pos, pos, numpy.linspace(0, 0.2, 42), mode='projected', piedges=numpy.linspace(0, 0.2, 26))
    with pytest.raises(ValueError, match='bins'):
        pairwise_los(pm, pos * 0.5 + 0.25, pos[:, 0], numpy.linspace(0, 0.2, MAX_BINS + 2))
    assert tuple(pairwise_velocities(pm, pos, pos, numpy.linspace(0, 0.2, MAX_BINS + 1)).npairs.shape) == (1024,)


@pytest.mark.gpu
def test_the_entry_refuses_more_than_1024_bins_and_wrong_columns(hipbe):
    """1025 bins: PMX_EINVAL from the entry itself, in all three modes; a block of the wrong number of columns, or none,
    likewise; 1024 bins are taken"""
    from pmesh_amd.backend import PmxError
    dev = hipbe.device
    pos = torch.from_numpy(uniform(50, 3, 1) * 0.5 + 0.25).to(dev)
    blk = {n: torch.ones((50, n), dtype=torch.float64, device=dev) for n in (1, 2, 3, 4, 5)}
    grid = cell_grid(50, 0.2, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(hipbe, pos, grid, UNIT)
    e = lambda n, top: torch.from_numpy(numpy.linspace(0, top, n + 1) ** 2).to(dev)

    def call(mode, w1, w2, e2, sub, nout=4 * 1025):
        out = (torch.zeros(1025, dtype=torch.int64, device=dev), torch.zeros(1025, dtype=torch.float64, device=dev),
               torch.zeros(nout, dtype=torch.float64, device=dev))
        wv1, wv2 = backend._arrays.vec(w1), backend._arrays.vec(w2)
        import ctypes as C
        hipbe.call('pair_counts', 3, int(mode), 2, 50, spos.data_ptr(), order.data_ptr(), cell_of.data_ptr(),
                   C.byref(wv1) if w1 is not None else None, 50, spos.data_ptr(), order.data_ptr(),
                   cell_start.data_ptr(), C.byref(wv2) if w2 is not None else None, _abi.i64arr(grid[0], 3),
                   int(grid[3]), _abi.f64arr(UNIT, 3), e2.numel() - 1, e2.data_ptr(),
                   sub.numel() - 1 if sub is not None else 1, sub.data_ptr() if sub is not None else None,
                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), hipbe.stream())
        return out
    pie = torch.sqrt(e(25, 0.2))
    for mode, ncol, sub in ((7, 4, None), (9, 2, None)):
        with pytest.raises(PmxError, match='BINS'):
            call(mode, blk[ncol], blk[ncol], e(1025, 0.2), sub)
        assert int(call(mode, blk[ncol], blk[ncol], e(1024, 0.2), sub)[0].sum()) >= 50
    with pytest.raises(PmxError, match='BINS'):
        call(8, blk[4], blk[4], e(41, 0.2), pie)                   # 41 x 25 = 1025
    assert int(call(8, blk[4], blk[4], e(40, 0.2), pie)[0].sum()) >= 50
    for mode, sub, good in ((7, None, 4), (8, pie, 4), (9, None, 2)):
        for w1, w2 in ((blk[good], blk[good + 1]), (blk[good - 1], blk[good]), (None, blk[good]), (blk[good], None)):
            with pytest.raises(PmxError, match='columns'):
                call(mode, w1, w2, e(4, 0.2), sub)
    # and the guard of Backend.pair_counts in front of it: an rsum of nbins entries would be overrun
    with pytest.raises(ValueError, match='rsum'):
        hipbe.pair_counts(7, 2, spos, order, cell_of, blk[4], spos, order, cell_start, blk[4], grid[0], grid[3], UNIT,
                          e(4, 0.2), None, torch.zeros(4, dtype=torch.int64, device=dev),
                          torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev))


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(vbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes: mode 7 in 3-d, 2-d and 1-d, modes 8 and 9 in 3-d (at this level nothing keeps the rows
    of mode 9 from the faces: the rule is defined there as well)"""
    for name in ('faces-3d', 'faces-2d', 'faces-1d', 'faces-projected', 'faces-los'):
        kernel, kw = RANDOM[name]
        nd = len(kw['box'])
        assert all(kw['box'][d] / grid[d] >= kw['edges'][-1] for d in range(nd))
        got = [cpu(x) for x in run_local(vbe, kernel, kw, grid_of(grid, kw['box']))]
        ref = reference(name)
        got[0][0] -= ref['nself']                               # (local_counts leaves the self pairs to its caller)
        got[1][0] -= ref['wself']
        check_vel(got, ref, what=(name, grid))


def test_open_axes(vbe):
    """a grid that is open along two axes (a rank's block): the rows of the block against all rows"""
    kernel, kw = RANDOM['open']
    pos, vel, b = kw['pos1'], kw['cols1'], kw['edges'][-1]
    grid = cell_grid(len(pos), b, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    assert 100 < inside.sum() < 1000
    got = run_local(vbe, kernel, kw, grid, pos1=pos[inside], cols1=vel[inside], pos2=pos, cols2=vel)
    ref = ref_vel(kernel, pos[inside], UNIT, kw['edges'], vel[inside], pos2=pos, cols2=vel)
    assert ref['margin'] >= 1e-9 and ref['npairs'].min() > 10
    check_vel(got, ref)


def test_crowded(vbe):
    """600 rows in one cell (and 50 isolated ones) with 4 bins: many lanes meet on one LDS address; two launches give identical npairs; with
    lattice rows, dyadic weights and dyadic velocities wnpairs and S3 are exact"""
    for name in ('crowded', 'crowded-los'):
        kernel, kw = RANDOM[name]
        ref = reference(name)
        assert len(kw['pos1']) == 650 and len(ref['npairs']) == 4 and ref['npairs'].sum() > 300000
        a, b = run(vbe, kernel, kw), run(vbe, kernel, kw)
        check_vel(a, ref, what=name)
        check_vel(b, ref, what=name)
        assert torch.equal(a.npairs, b.npairs)
    pos = 0.5 + (lattice_rows(600, 3, 51) - 0.5) * 2.0 ** -5
    w = dyadic_weights(600, 52)
    e = numpy.array([0.0, 1 / 128., 1 / 64., 1 / 32.])
    for kernel, ncol in (('1d-velocity', 3), ('1d-los', 1)):
        kw = dict(pos1=pos, cols1=dyadic_vel(600, ncol, 53), w1=w, box=UNIT, edges=e)
        check_vel(run(vbe, kernel, kw), ref_vel(kernel, **kw), exact=True, what=kernel)


def test_exact_sums(vbe):
    """rows on the 2^-12 lattice, weights that are multiples of 1/8, velocities that are multiples of 1/8 below 16:
    wnpairs and dv2sum / ds2sum exactly, cross and auto, in float64 and float32 storage, in all three modes"""
    p1, p2 = lattice_rows(900, 3, 53), lattice_rows(800, 3, 54)
    w1, w2 = dyadic_weights(900, 55), dyadic_weights(800, 56)
    edges = [0.0, 1 / 32., 1 / 16., 3 / 32., 1 / 8.]
    for kernel, ncol in (('1d-velocity', 3), ('projected-velocity', 3), ('1d-los', 1)):
        v1, v2 = dyadic_vel(900, ncol, 57), dyadic_vel(800, ncol, 58)
        a, b = (p1, p2) if kernel != '1d-los' else (0.0625 + p1 * 0.875, 0.0625 + p2 * 0.875)
        extra = dict(sub=[0.0, 1 / 16., 1 / 8.], los=0) if kernel == 'projected-velocity' else {}
        for dtype in ('f8', 'f4'):
            kw = dict(pos1=a.astype(dtype), cols1=v1.astype(dtype), pos2=b.astype(dtype), cols2=v2.astype(dtype),
                      w1=w1.astype(dtype), w2=w2.astype(dtype), box=UNIT, edges=edges, **extra)
            assert numpy.array_equal(kw['pos1'].astype('f8'), a) and numpy.array_equal(kw['cols1'].astype('f8'), v1)
            check_vel(run(vbe, kernel, kw), ref_vel(kernel, **kw), exact=True, what=(kernel, dtype))
            kw.update(pos2=None, cols2=None, w2=None)
            check_vel(run(vbe, kernel, kw), ref_vel(kernel, **kw), exact=True, what=(kernel, dtype, 'auto'))


@pytest.mark.gpu
def test_more_secondaries_than_one_launch(hipbe):
    """300 primaries against 2^23 + 1000 secondaries: the entry launches once per window of 2^23 slots of the
    secondaries, and the cell that holds slot 2^23 is split between two launches; eight of the primaries sit in it.  No
    brute force at this size (after tests.test_paircount's test_more_secondaries_than_one_launch_counts): the sums
    against all secondaries equal the sums against their two halves, each within one launch.  Rows on the lattice,
    dyadic velocities: npairs, wnpairs and dv2sum exactly.  rsum, S1 and S2 within twice the bound, with S bounded from
    the outputs: the terms of rsum and S2 are not negative, so S is the sum itself, and S of S1 is at most sqrt(wnpairs
    S2) by the Cauchy-Schwarz inequality"""
    n2 = (1 << 23) + 1000
    dev = hipbe.device
    gen = torch.Generator(device=dev).manual_seed(5)
    p2 = torch.randint(0, 4096, (n2, 3), generator=gen, device=dev).to(torch.float64) / 4096
    v2 = torch.randint(-127, 128, (n2, 3), generator=gen, device=dev).to(torch.float64) / 8
    edges = numpy.linspace(0.0, 0.02, 5)
    grid = cell_grid(n2, 0.02, UNIT)
    _, _, cell_start, _, _, _ = cell_sort(hipbe, p2, grid, UNIT)
    cell = int(torch.searchsorted(cell_start.to(torch.int64), torch.tensor([1 << 23], device=dev), right=True)[0]) - 1
    assert int(cell_start[cell]) < (1 << 23) < int(cell_start[cell + 1])
    axes = numpy.array(numpy.unravel_index(cell, grid[0]), dtype='f8')
    near = (axes + numpy.random.RandomState(3).randint(1, 8, size=(8, 3)) / 8.0) / numpy.asarray(grid[2])
    p1 = torch.from_numpy(numpy.concatenate([near, lattice_rows(292, 3, 9)])).to(dev)
    v1 = torch.from_numpy(dyadic_vel(300, 3, 10)).to(dev)
    pm = mesh(UNIT)
    whole = pairwise_velocities(pm, p1, v1, edges, pos2=p2, vel2=v2)
    half = n2 // 2
    parts = [pairwise_velocities(pm, p1, v1, edges, pos2=p2[:half], vel2=v2[:half]),
             pairwise_velocities(pm, p1, v1, edges, pos2=p2[half:], vel2=v2[half:])]
    n = cpu(whole.npairs)
    assert n.sum() > 50000 and torch.equal(whole.npairs, parts[0].npairs + parts[1].npairs)
    assert torch.equal(whole.wnpairs, parts[0].wnpairs + parts[1].wnpairs)
    assert torch.equal(whole.dv2sum, parts[0].dv2sum + parts[1].dv2sum)
    wn, s2 = cpu(whole.wnpairs), cpu(whole.v2sum)
    for field, S in (('rsum', cpu(whole.rsum)), ('v2sum', s2), ('vsum', numpy.sqrt(wn * s2))):
        d = numpy.abs(cpu(getattr(whole, field)) - cpu(getattr(parts[0], field)) - cpu(getattr(parts[1], field)))
        assert (d <= 2 * (n + 4) * U * S * (1 + 1e-9)).all(), (field, d.max())
    # and against the expectation of uniform rows, to a few standard deviations of the count
    want = 300 * n2 * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert (numpy.abs(n - want) < 6 * numpy.sqrt(want)).all()


# ---- 4. physics checks of the derived fields --------------------------------------------------------------------------------

def ratio_bound(ref, m, den=0, factor=1):
    """the bound on sums[m] / sums[den] per bin that the bounds of the two sums give, the quotient carried through to
    first order (the factor 1 + 1e-9 covers the rest) plus two ulps for the division itself"""
    M = ref['npairs'] + 4.0
    num, d = ref['sums'][m], ref['sums'][den]
    return factor * (M * U * ref['abs'][m] + numpy.abs(num / d) * M * U * ref['abs'][den]) / numpy.abs(d) * (1 + 1e-9) \
        + 2 * U * numpy.abs(num / d)


def test_hubble_flow(vbe):
    """v = H x on rows inside a quarter of the box: dv = H dx for every pair (none is a wrapped one: the rows span
    0.25 < 1 / 2), so u = H r up to two roundings and v12 == H rmean within the bounds of the sums; the transverse
    dispersion vanishes within 1e-6 H b, b the largest edge"""
    H = 0.7
    kernel, kw = RANDOM['hubble']
    ref = reference('hubble')
    assert ref['npairs'].min() > 50
    pv = run(vbe, kernel, kw)
    check_vel(pv, ref)
    v12, rmean = cpu(pv.v12), cpu(pv.rmean)
    # two ulps for the product H x of the input, three for dx.dv / r against H r: term by term, hence on the mean
    bound = ratio_bound(ref, 2) + H * ratio_bound(ref, 1) + 8 * U * H * rmean
    assert (numpy.abs(v12 - H * rmean) <= bound).all(), numpy.abs(v12 - H * rmean).max()
    assert (cpu(pv.sigma_perp) <= 1e-6 * H * kw['edges'][-1]).all()
    assert (cpu(pv.sigma_par) > 0.1 * H * numpy.diff(kw['edges'])).all()     # (the spread of r within a bin)


def test_independent_velocities(vbe):
    """velocities drawn independently of position, n = 800 rows, sigma = 1.5 per axis: u is the difference of two
    independent projections, normal with the variance 2 sigma^2, so v2sum / wnpairs estimates 2 sigma^2 and lies within 5
    standard errors of it.  The standard error, from the restatement's pair count: the N = npairs / 2 unordered pairs of
    a bin (the ordered count holds each twice) have Var(u^2) = 2 (2 sigma^2)^2 = 8 sigma^4 each.  Two pairs that share a
    row, their directions at the cosine rho, have Cov(u_ij, u_ik) = rho sigma^2 and Cov(u_ij^2, u_ik^2) = 2 rho^2
    sigma^4, on average over isotropic directions 2/3 sigma^4; a pair shares a row with about 2 k others, k = 2 N / n the
    pairs of one row in the bin.  Var(sum u^2) = N sigma^4 (8 + 2 k 2/3), and the standard error of the mean is
    2 sigma^2 sqrt(2 / N) sqrt(1 + k / 6).  The mean of rho itself vanishes, so v12 = mean u has the standard error
    sigma sqrt(2 / N) and lies within 5 of them of zero"""
    sigma = 1.5
    kernel, kw = RANDOM['independent']
    ref = reference('independent')
    pv = run(vbe, kernel, kw)
    check_vel(pv, ref)
    N = ref['npairs'] / 2.0
    assert N.min() > 300
    err = 2 * sigma ** 2 * numpy.sqrt(2 / N) * numpy.sqrt(1 + (2 * N / 800) / 6)
    got = cpu(pv.v2sum) / cpu(pv.wnpairs)
    assert (numpy.abs(got - 2 * sigma ** 2) <= 5 * err).all(), (got, err)
    assert (5 * err < sigma ** 2).all()                                      # (the check has power: half the expectation)
    assert (numpy.abs(cpu(pv.v12)) <= 5 * sigma * numpy.sqrt(2 / N)).all()


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_line_of_sight_of_a_hubble_flow(vbe, axis):
    """mode 9 with s_i = v_i . n_i from the Hubble flow v = H x returns the v12 of mode 7.  The estimator weighs a pair
    by c = (1 + cos theta) / 2 times the cosine of the pair to the line of sight, theta the angle between the two rows
    at the observer, so the two agree to rounding only where theta = 0: the rows lie on one ray from the observer, here
    along a box axis, on the 2^-12 lattice, with H = 1/2 and dyadic weights.  Then n = e_axis for every row, s = H x_axis,
    ds = H dx, c = +-1, and every term of num, den and of mode 7's vsum and wnpairs is exact and the same number: only
    the order of the additions differs, and v12 of both lies within the bounds of the sums of H rmean"""
    H = 0.5
    t = numpy.unique(numpy.random.RandomState(97 + axis).randint(1, 1000, size=400)) / 4096.0      # 0 < t < 1 / 4
    pos = numpy.full((len(t), 3), 0.5)
    pos[:, axis] = 0.5 + t
    vel = H * pos
    w = dyadic_weights(len(t), 98)
    edges = [0.0, 1 / 64., 1 / 32., 1 / 16.]
    s = vel[:, axis]                                                         # v . n with n = e_axis
    r7 = ref_vel('1d-velocity', pos, UNIT, edges, vel, w1=w)
    r9 = ref_vel('1d-los', pos, UNIT, edges, s, w1=w)
    assert r7['npairs'].min() > 1000 and numpy.array_equal(r7['npairs'], r9['npairs'])
    assert numpy.array_equal(r9['abs'][2], r7['abs'][2]) and numpy.array_equal(r9['abs'][3], r7['abs'][0])
    pm = mesh(UNIT)
    pv = pairwise_velocities(pm, pos, vel, edges, weight1=w)
    ks = pairwise_los(pm, pos, s, edges, weight1=w)
    check_vel(pv, r7, exact=True)
    check_vel(ks, r9, exact=True)
    assert torch.equal(pv.npairs, ks.npairs)
    bound = ratio_bound(r7, 2) + ratio_bound(r9, 2, den=3)
    assert (numpy.abs(cpu(ks.v12) - cpu(pv.v12)) <= bound).all()
    assert (numpy.abs(cpu(ks.v12) - H * cpu(pv.rmean)) <= ratio_bound(r9, 2, den=3) + H * ratio_bound(r7, 1)).all()
    assert (cpu(ks.v12) > 0).all()


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------

def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1) * 0.5 + 0.25
    vel = normal_vel(50, 3, 2)
    with pytest.raises(ValueError, match='edges'):
        pairwise_velocities(pm, pos, vel, [0.2, 0.1])
    with pytest.raises(ValueError, match='separation'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.51])
    with pytest.raises(ValueError, match='mode'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], mode='2d')
    with pytest.raises(ValueError, match='vel1'):
        pairwise_velocities(pm, pos, vel[:, :2], [0.0, 0.1])
    with pytest.raises(ValueError, match='vel1'):
        pairwise_velocities(pm, pos, vel[:49], [0.0, 0.1])
    with pytest.raises(ValueError, match='vel1'):
        pairwise_velocities(pm, pos, None, [0.0, 0.1])
    with pytest.raises(ValueError, match='vel2 needs pos2'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], vel2=vel)
    with pytest.raises(ValueError, match='pos2 needs vel2'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], pos2=pos)
    with pytest.raises(ValueError, match='vel2'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], pos2=pos[:40], vel2=vel)
    with pytest.raises(TypeError):
        pairwise_velocities(pm, pos, (vel * 8).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='weight1'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], weight1=numpy.ones(49))
    with pytest.raises(ValueError, match='weight2'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], weight2=numpy.ones(50))
    bad = vel.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows of vel1'):
        pairwise_velocities(pm, pos, bad, [0.0, 0.1])
    with pytest.raises(ValueError, match='three dimensions'):
        pairwise_velocities(mesh(UNIT[:2]), pos[:, :2], vel[:, :2], [0.0, 0.1], mode='projected', pimax=1)
    with pytest.raises(ValueError, match='los'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], mode='projected', piedges=[0.0, 0.1], los=3)
    with pytest.raises(ValueError, match='needs'):
        pairwise_velocities(pm, pos, vel, [0.0, 0.1], mode='projected')
    with pytest.raises(NotImplementedError):
        pairwise_velocities(mesh([1.0] * 4), numpy.zeros((3, 4)), numpy.zeros((3, 4)), [0.0, 0.1])
    with pytest.raises(ValueError, match='three dimensions'):
        pairwise_los(mesh(UNIT[:2]), pos[:, :2], vel[:, 0], [0.0, 0.1])
    with pytest.raises(ValueError, match='s1'):
        pairwise_los(pm, pos, vel, [0.0, 0.1])
    with pytest.raises(ValueError, match='observer'):
        pairwise_los(pm, pos, vel[:, 0], [0.0, 0.1], observer=[0.5, 0.5])
    with pytest.raises(ValueError, match='1 rows of s1'):
        pairwise_los(pm, pos, bad[:, 1], [0.0, 0.1])
    # no rows at all
    empty = pairwise_velocities(pm, numpy.zeros((0, 3)), numpy.zeros((0, 3)), [0.0, 0.1, 0.2])
    assert cpu(empty.npairs).tolist() == [0, 0] and numpy.isnan(cpu(empty.v12)).all() and empty.W1 == 0.0
    assert cpu(pairwise_los(pm, pos, vel[:, 0], [0.0, 0.1], pos2=numpy.zeros((0, 3)), s2=numpy.zeros(0)).npairs).tolist() == [0]
    # one dimension has no transverse axis
    one = pairwise_velocities(mesh(UNIT[:1]), pos[:, :1], vel[:, :1], [0.0, 0.1])
    assert one.sigma_perp is None and one.ndim == 1 and int(one.npairs[0]) > 0


# ---- 6. ranks --------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """the call on thread ranks holding both sets split unevenly (one rank holds no rows): what every rank got"""
    kernel, kw = RANDOM[name]
    p2 = kw.get('pos2')
    s1 = split(len(kw['pos1']), size)
    s2 = split(len(p2), size)[::-1] if p2 is not None else None

    def body(comm):
        mine = dict(kw, pm=mesh(kw['box'], comm, np_))
        for key, sl in (('pos1', s1), ('cols1', s1), ('w1', s1), ('pos2', s2), ('cols2', s2), ('w2', s2)):
            if kw.get(key) is not None:
                mine[key] = kw[key][sl[comm.rank]]
        got = run(backend.get(), kernel, mine)
        n, sums = arrays(got)
        return n, sums, got.W1, got.W2, got.W2sum, len(mine['pos1'])
    return thread_ranks(size, body)


def check_ranks(name, size, np_):
    results = ranks_case(name, size, np_)
    ref = reference(name)
    assert ref['margin'] >= 1e-9
    sizes = [results[r][5] for r in range(size)]
    assert 0 in sizes and len(set(sizes)) > 1
    nbins = len(ref['npairs'])
    for r in range(size):
        n, sums = results[r][:2]
        check_vel((n, sums[0], sums[1:].reshape(4 * nbins)), ref, factor=2, what=(name, size, r))
        for k in range(5):
            assert numpy.array_equal(results[r][k], results[0][k])      # identical on every rank


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_sums(obe, size, np_):
    """weighted cross in mode 7, weighted auto in mode 8 on the box [1, 0.5, 0.25], auto in mode 9: the arrays of every
    rank are identical; npairs is that of the restatement of all rows exactly, the sums within twice the bound"""
    for name in ('ranks', 'ranks-slab', 'ranks-los'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_on_the_device(hipbe, size, np_):
    for name in ('ranks', 'ranks-slab', 'ranks-los'):
        check_ranks(name, size, np_)


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank: velocities of a wrong shape, of a wrong type, of a wrong length,
    not finite; too many bins; a row of mode 9 outside the padded interior"""
    pos = uniform(90, 3, 2) * 0.5 + 0.25
    vel = normal_vel(90, 3, 3)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        sl = slice(30 * comm.rank, 30 * comm.rank + 30)
        mine, v = pos[sl], vel[sl]
        edges = [0.0, 0.05]
        with pytest.raises(ValueError):
            pairwise_velocities(pm, mine, v[:, :2] if comm.rank == 1 else v, edges)
        with pytest.raises(TypeError):
            pairwise_velocities(pm, mine, (v * 8).astype('i8') if comm.rank == 2 else v, edges)
        with pytest.raises(ValueError):
            pairwise_velocities(pm, mine, v[:29] if comm.rank == 0 else v, edges)
        bad = v.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows of vel1'):
            pairwise_velocities(pm, mine, bad, edges)
        with pytest.raises(ValueError):
            pairwise_velocities(pm, mine, v, numpy.linspace(0, 0.05, MAX_BINS + (2 if comm.rank == 2 else 1)))
        with pytest.raises(ValueError):
            pairwise_velocities(pm, mine, v, edges, vel2=v if comm.rank == 1 else None)
        out = mine.copy()
        if comm.rank == 1:
            out[0, 0] = 0.99
        with pytest.raises(ValueError, match='outside'):
            pairwise_los(pm, out, v[:, 0], edges)
        with pytest.raises(ValueError, match='1 rows of s1'):
            pairwise_los(pm, mine, bad[:, 2], edges)
        want = ref_vel('1d-velocity', pos, UNIT, edges, vel)
        check_vel(pairwise_velocities(pm, mine, v, edges), want, factor=2)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 7. streams ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('kernel', sorted(VELOCITY_MODES))
def test_capture_on_a_side_stream(hipbe, kernel):
    """Backend.pair_counts in every new mode with the inputs sorted and the outputs allocated beforehand: the zeroing and
    the call captured into a graph on a side stream leave the poisoned outputs as they were (nothing ran eagerly or on
    another stream); the replay gives npairs of the null-stream call exactly and its sums within twice the bound"""
    from tests import test_streams as T
    dev = hipbe.device
    n = 3000
    ncol = 1 if kernel == '1d-los' else 3
    pos = 0.05 + 0.9 * lattice_rows(n, 3, 30)
    cols, w = dyadic_vel(n, ncol, 31), dyadic_weights(n, 32)
    e = numpy.linspace(0.0, 0.1, 9)
    sub = numpy.linspace(0.0, 0.1, 5) if kernel == 'projected-velocity' else None
    ref = vel_core(pos, pos, numpy.ones(3), kernel, 2, e * e, sub, block(n, cols, w), block(n, cols, w))
    grid = cell_grid(n, 0.1, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(hipbe, torch.from_numpy(pos).to(dev), grid, UNIT)
    blk = torch.from_numpy(block(n, cols, w)).to(dev)
    e2 = torch.from_numpy(e * e).to(dev)
    subt = None if sub is None else torch.from_numpy(sub).to(dev)
    nbins = len(ref['npairs'])
    outs = [torch.zeros(nbins, dtype=torch.int64, device=dev), torch.zeros(nbins, dtype=torch.float64, device=dev),
            torch.zeros(4 * nbins, dtype=torch.float64, device=dev)]

    def work():
        for t in outs:
            t.zero_()
        hipbe.pair_counts(VELOCITY_MODES[kernel], 2, spos, order, cell_of, blk, spos, order, cell_start, blk, grid[0],
                          grid[3], UNIT, e2, subt, *outs)
    work()
    torch.cuda.synchronize()
    want = [cpu(t).copy() for t in outs]
    check_vel(want, ref, exact=True)
    T.poison(outs)
    torch.cuda.synchronize()
    assert all(T.poisoned(outs))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        work()
    torch.cuda.synchronize()
    assert all(T.poisoned(outs)), 'a captured zeroing or kernel ran eagerly, or on another stream'
    g.replay()
    torch.cuda.synchronize()
    got = [cpu(t) for t in outs]
    assert numpy.array_equal(got[0], want[0])
    check_vel(got, ref, exact=True, factor=2)


# ---- 8. the ABI and the resources ------------------------------------------------------------------------------------------

def test_the_modes_are_bound():
    assert (_abi.PMX_PAIRS_1D_VELOCITY, _abi.PMX_PAIRS_PROJECTED_VELOCITY, _abi.PMX_PAIRS_1D_LOS) == (7, 8, 9)
    assert _abi.PMX_PAIRS_VELOCITY_MAX_BINS == MAX_BINS == 1024
    assert VELOCITY_MODES == {'1d-velocity': 7, 'projected-velocity': 8, '1d-los': 9}
    for name in ('pairwise_velocities', 'pairwise_los'):
        assert name in pmesh_amd.__doc__ and callable(getattr(pmesh_amd.pairvel, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pmesh_amd.h')).read()
    for text in ('S1 += (w u), S2 += (w u) u, S3 += w dv2', 'S1 += (w c) ds, S2 += (w c) c, S3 += (w ds) ds',
                 'rsum[m * nbins + b]'):
        assert text in header and text in ' '.join(pmesh_amd.pairvel.__doc__.replace('``', '').split()), text
    assert 'pmx_pairs_vel.hip' in open(os.path.join(root, 'pmesh_amd', 'csrc', 'Makefile')).read()


def test_the_entry_accepts_the_modes():
    """pmx_pair_counts with no rows returns before it touches the device: PMX_OK in the modes 7 to 9 (and 0 to 6),
    PMX_EINVAL in mode 10, with more than 1024 bins in the modes 7 to 9, and in mode 9 in two dimensions"""
    import ctypes as C
    lib = backend.load_library()

    def rc(ndim, mode, nr, nsub=1):
        return lib.pmx_pair_counts(ndim, mode, 2, 0, None, None, None, None, 0, None, None, None, None,
                                   _abi.i64arr([1, 1, 1], 3), 7, _abi.f64arr(UNIT, 3), nr, None, nsub, None, None, None,
                                   None, C.c_void_p(0))
    assert [rc(3, mode, 4, 1 if mode in (0, 5, 7, 9) else 2) for mode in range(11)] == [0] * 10 + [_abi.PMX_EINVAL]
    assert [rc(3, mode, 1025) for mode in (0, 7, 9)] == [0, _abi.PMX_EINVAL, _abi.PMX_EINVAL]
    assert [rc(3, 8, 41, 25), rc(3, 8, 32, 32), rc(3, 7, 4, 2), rc(2, 7, 4), rc(2, 9, 4), rc(2, 8, 4, 2)] == \
        [_abi.PMX_EINVAL, 0, _abi.PMX_EINVAL, 0, _abi.PMX_EINVAL, _abi.PMX_EINVAL]


def test_vel_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs_vel.hip')
    # vel_kernel<NDIM, MODE>: mode 7 for 1 to 3 dimensions, modes 8 and 9 for 3
    assert len(t) == 5 and all('vel_kernel' in k for k in t), sorted(t)
    # measured at compile time: 40, 48 and 58 VGPRs in mode 7 for 1, 2 and 3 dimensions, 60 in mode 8, 76 in mode 9
    measured = {'ILi1ELi7E': 40, 'ILi2ELi7E': 48, 'ILi3ELi7E': 58, 'ILi3ELi8E': 60, 'ILi3ELi9E': 76}
    for name, r in t.items():
        key = [k for k in measured if 'vel_kernel' + k in name]
        assert len(key) == 1, name
        assert r['ScratchSize'] == 0, (name, r)
        # 1024 bins of a 32-bit count and five doubles, the 129 squared edges of r and, in mode 8, the 129 edges of pi:
        # three workgroups in the 160 KB of a CU
        assert r['LDS'] <= 1024 * 44 + 129 * 8 * (2 if 'Li8E' in name else 1) + 16 <= 48 * 1024, (name, r)
        assert r['VGPRs'] <= measured[key[0]] + 4, (name, r)
