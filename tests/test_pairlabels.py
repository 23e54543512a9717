"""pmesh_amd.pairlabels (csrc/pmx_pairs_labels.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/pairlabels.py, include/pmesh_amd.h).  The modes 16 | m (PMX_PAIRS_SPLIT) and 32 | m
(PMX_PAIRS_JACKKNIFE) of pmx_pair_counts, m a base mode 0 .. 4, share rows, wrapping, the minimum image, r2, q, the
squared edges, the r-, mu- and pi-bin and the pimax cut with the base mode.  Both sets bring the block (w, label).  Per
counted pair of bin b with the labels a (primary) and c (secondary), w = w1_i * w2_j:
  split      kind = (a == c and a is a label) ? 1 : 0; npairs[kind * nbins + b] += 1, wnpairs[...] += w,
             rsum[...] += w sqrt(q); 2 * nbins entries each
  jackknife  K = (4096 / nbins - 2) / 2; a label is in range when it is below K; all[b] gets (1, w, w sqrt(q)); if a is
             in range side[a][b] gets (1, w); if c is in range side[c][b] gets (1, w); if a == c and in range same[a][b]
             gets (1, w); blocks of nbins: 0 all, 1 + k side[k], 1 + K + k same[k]; rsum: all only
A label that is negative, not finite or out of range is no label.

The restatement (label_core) is brute force over the full (n1, n2) matrix.  It forms the bin of every pair with its own
comparisons (pair_bins: the five base modes in one function) and holds them to npairs of tests.test_paircount.count_core
/ tests.test_surveypairs.survey_core bin by bin before anything is summed; the label logic is written with masks over
the matrix, one label at a time.  Under -m "not gpu" it serves the new modes of pmx_pair_counts (LabelOracleBackend; the
other modes go to its parents); under -m gpu the kernel is compared with it.

No tolerance is new.  Counts are compared with array_equal.  Weighted sums use dyadic weights (dyadic_weights:
multiples of 1/8 in [1/8, 2]): every product and every partial sum is exact in any order, so they are compared by
equality too.  rsum, and the sums on thread ranks, are compared within the bound of tests.test_paircount.check,
|got - ref| <= (M + 4) 2^-52 S (twice that on ranks).  Random inputs keep every pair at least 1e-9 (relative) from an
edge by the margin the cores report; test_inputs_are_decided asserts it without a GPU.
"""
import os

import numpy
import pytest
import torch

import pmesh_amd
from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid, cell_sort, fof
from pmesh_amd.paircount import (LABEL_BASES, LABEL_MODES, PairCounts, label_lengths, label_slots, local_counts,
                                 pair_correlation, pair_counts)
from pmesh_amd.pairlabels import (MAX_BINS, JackknifeCorrelation, JackknifeCounts, SplitCounts, box_regions,
                                  pair_correlation_jackknife, pair_correlation_split, pair_counts_jackknife,
                                  pair_counts_split, survey_correlation_jackknife, survey_pair_counts_jackknife)
from pmesh_amd.surveypairs import SurveyPairCounts, survey_correlation, survey_pair_counts, to_poles
from tests.test_fof import GRIDS, RANKS, SLAB, UNIT, face_pairs, mesh, split, thread_ranks, uniform, wrap
from tests.test_lpt import cpu
from tests.test_paircount import U, check, count_core, dyadic_weights, grid_of, lattice_rows
from tests.test_surveypairs import SurveyOracleBackend, survey_core

CODES = {v: k for k, v in LABEL_MODES.items()}
BOX_MODES = ('1d', '2d', 'projected')


# ---- the restatement -----------------------------------------------------------------------------------------------

def pair_bins(w1, w2, box, base, los, e2, sub):
    """(keep, bin, q) over the (n1, n2) matrix of the wrapped rows in the base mode `base` of LABEL_BASES: the counted
    pairs, their flat bin, and q.  sub: what the entry is given (m2, piedges or piedges^2)."""
    nd = w1.shape[1]
    dx = []
    for d in range(nd):
        x = w1[:, None, d] - w2[None, :, d]
        dx.append(x - box[d] * numpy.rint(x / box[d]))
    nsub = 1 if base == '1d' else len(sub) - 1
    sbin = numpy.zeros((len(w1), len(w2)), dtype='i8')
    extra = True
    if base in ('1d', '2d', 'projected'):
        q = numpy.zeros((len(w1), len(w2)))
        for d in range(nd):
            if base != 'projected' or d != los:
                q = q + dx[d] * dx[d]
        if base == '2d':
            z2 = dx[los] * dx[los]
            for k in range(1, nsub):
                sbin += (z2 >= sub[k] * q) & (q > 0)
        elif base == 'projected':
            az = numpy.abs(dx[los])
            for k in range(1, nsub):
                sbin += az >= sub[k]
            extra = az < sub[-1]
    else:
        l = [(w1[:, None, d] + w2[None, :, d]) - box[d] for d in range(3)]
        r2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]
        p = (dx[0] * l[0] + dx[1] * l[1]) + dx[2] * l[2]
        l2 = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]
        p2 = p * p
        if base == '2d-midpoint':
            q = r2
            t = r2 * l2
            for k in range(1, nsub):
                sbin += (p2 >= sub[k] * t) & (t != 0)
        else:
            with numpy.errstate(invalid='ignore', divide='ignore'):
                pi2 = numpy.where(l2 == 0, 0.0, p2 / numpy.where(l2 == 0, 1.0, l2))
            q = numpy.maximum(r2 - pi2, 0.0)
            for k in range(1, nsub):
                sbin += pi2 >= sub[k]
            extra = pi2 < sub[-1]
    keep = (q >= e2[0]) & (q < e2[-1]) & extra
    rbin = numpy.zeros_like(sbin)
    for k in range(1, len(e2) - 1):
        rbin += q >= e2[k]
    return keep, rbin * nsub + sbin, q


def label_core(w1, w2, box, kernel, los, e2, sub, blk1, blk2, skip_diagonal=False):
    """The arrays of the entry in the mode `kernel` of LABEL_MODES over the pairs of the wrapped rows w1 with w2 and
    their blocks (w, label).  Returns a dict: npairs, wnpairs, rsum in the layout of the header; margin; nbins, K."""
    family, base = kernel.split('-', 1)
    blk1, blk2 = numpy.asarray(blk1, dtype='f8'), numpy.asarray(blk2, dtype='f8')
    n1, n2 = len(w1), len(w2)
    assert blk1.shape == (n1, 2) and blk2.shape == (n2, 2)
    nbins = (len(e2) - 1) * (1 if base == '1d' else len(sub) - 1)
    K = label_slots(nbins)
    assert K >= 1
    ncount, nrsum = (2 * nbins, 2 * nbins) if family == 'split' else ((1 + 2 * K) * nbins, nbins)
    out = dict(npairs=numpy.zeros(ncount, dtype='i8'), wnpairs=numpy.zeros(ncount), rsum=numpy.zeros(nrsum),
               margin=numpy.inf, nbins=nbins, K=K)
    if n1 == 0 or n2 == 0:
        return out
    if base in BOX_MODES:
        core = count_core(w1, w2, box, base, los, e2, sub, skip_diagonal=skip_diagonal)
    else:
        core = survey_core(w1, w2, box, base, e2, sub, skip_diagonal=skip_diagonal)
    keep, bins, q = pair_bins(w1, w2, box, base, los, e2, sub)
    if skip_diagonal:
        keep = keep & ~numpy.eye(n1, n2, dtype=bool)
    # the decisions are those of the base mode's restatement
    assert numpy.array_equal(numpy.bincount(bins[keep], minlength=nbins), core['npairs'])
    out['margin'] = core['margin']
    w = blk1[:, 0][:, None] * blk2[:, 0][None, :]
    wr = w * numpy.sqrt(q)
    la, lc = blk1[:, 1], blk2[:, 1]

    def add(block, mask, times=1, r=False):
        m = keep & mask
        sl = slice(block * nbins, (block + 1) * nbins)
        out['npairs'][sl] += times * numpy.bincount(bins[m], minlength=nbins)
        out['wnpairs'][sl] += times * numpy.bincount(bins[m], weights=w[m], minlength=nbins)
        if r:
            out['rsum'][sl] += numpy.bincount(bins[m], weights=wr[m], minlength=nbins)
    everything = numpy.ones((n1, n2), dtype=bool)
    if family == 'split':
        with numpy.errstate(invalid='ignore'):
            is_label = numpy.isfinite(la) & (la >= 0)
            same = is_label[:, None] & (la[:, None] == lc[None, :])
        add(1, same, r=True)
        add(0, ~same, r=True)
    else:
        add(0, everything, r=True)
        with numpy.errstate(invalid='ignore'):
            labels = sorted(set(int(x) for x in numpy.concatenate([la, lc]) if 0 <= x < K))
        for k in labels:
            ina, inc = (la >= 0) & (la < K) & (numpy.floor(la) == k), (lc >= 0) & (lc < K) & (numpy.floor(lc) == k)
            add(1 + k, ina[:, None] & everything)
            add(1 + k, inc[None, :] & everything)
            add(1 + K + k, ina[:, None] & inc[None, :])
    return out


def blk(n, label, w=None, dtype='f8'):
    """the (n, 2) block (w, label) of one set"""
    w = numpy.ones(n) if w is None else numpy.asarray(w)
    return numpy.stack([w.astype('f8'), numpy.asarray(label).astype('f8')], axis=1).astype(dtype)


def given_sub(base, sub):
    """what the entry gets as `sub` of the public sub edges"""
    if sub is None:
        return None
    s = numpy.asarray(sub, dtype='f8')
    return s if base == 'projected' else s * s


class LabelOracleBackend(SurveyOracleBackend):
    """the CPU test double with the modes by row labels of pmx_pair_counts served by the restatement"""
    name = 'oracle-pairlabels'

    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        if mode not in CODES:
            return SurveyOracleBackend.pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2,
                                                   cell_start2, weight2, ncell, periodic, boxsize, e2, sub, npairs,
                                                   wnpairs, rsum)
        n1, n2, nd = spos1.shape[0], spos2.shape[0], spos1.shape[1]
        if n1 == 0 or n2 == 0:
            return
        nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
        ncount, nrsum = label_lengths(CODES[mode], nbins)
        assert npairs.numel() == wnpairs.numel() == ncount and rsum.numel() == nrsum
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        for w, n in ((weight1, n1), (weight2, n2)):
            assert tuple(w.shape) == (n, 2) and w.is_contiguous() and w.dtype in (torch.float32, torch.float64)
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = label_core(a, b, numpy.asarray(boxsize, dtype='f8'), CODES[mode], los, e2.numpy(),
                         None if sub is None else sub.numpy(), weight1.numpy(), weight2.numpy())
        npairs += torch.from_numpy(got['npairs'])
        wnpairs += torch.from_numpy(got['wnpairs'])
        rsum += torch.from_numpy(got['rsum'])


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(LabelOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def lbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(LabelOracleBackend())
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


def check_arrays(got, ref, exact_w=True, factor=1, what=''):
    """the flat triple of local_counts against the restatement's dict: npairs by equality; wnpairs by equality (dyadic
    weights) or within the bound; rsum within `factor` times the bound of tests.test_paircount.check.  The terms are not
    negative: S is the sum itself."""
    n, wn, rs = [(x if isinstance(x, numpy.ndarray) else cpu(x)).reshape(-1) for x in got]
    assert n.dtype == numpy.int64 and wn.dtype == rs.dtype == numpy.float64
    assert numpy.array_equal(n, ref['npairs']), (what, numpy.nonzero(n != ref['npairs'])[0][:8])
    M = ref['npairs'].astype('f8')
    if exact_w:
        assert numpy.array_equal(wn, ref['wnpairs']), what
    else:
        assert (numpy.abs(wn - ref['wnpairs']) <= factor * (M + 4) * U * numpy.abs(ref['wnpairs'])).all(), what
    Mr = M[:len(rs)]                                            # (jackknife: rsum covers the block `all`, the first)
    assert (numpy.abs(rs - ref['rsum']) <= factor * (Mr + 4) * U * numpy.abs(ref['rsum'])).all(), what


def same_counts(a, b, factor=2, what=''):
    """two PairCounts of one set of pairs: npairs and (dyadic) wnpairs by equality; rsum within twice the bound of
    check, once for each of the two (the terms are not negative: S is the sum itself)"""
    assert torch.equal(a.npairs, b.npairs), what
    assert torch.equal(a.wnpairs, b.wnpairs), what
    d, M, S = cpu(torch.abs(a.rsum - b.rsum)), cpu(b.npairs).astype('f8'), cpu(torch.abs(b.rsum))
    assert (d <= factor * (M + 4) * U * S).all(), (what, d.max())


def dev_t(be, x):
    return None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(be.device)


def run_local(be, kernel, box, edges, pos1, blk1, pos2=None, blk2=None, sub=None, los=2, grid=None):
    """local_counts of the blocks on the cell grid of one rank (or a forced one): the flat triple"""
    e = numpy.asarray(edges, dtype='f8')
    base = kernel.split('-', 1)[1]
    b = float(e[-1])
    if base == 'projected':
        b = float(max(e[-1], sub[-1]))
    elif base == 'projected-midpoint':
        b = float(numpy.nextafter(numpy.hypot(e[-1], sub[-1]), numpy.inf))
    if grid is None:
        grid = cell_grid(max(len(pos1), 0 if pos2 is None else len(pos2)), b, box)
    return local_counts(be, kernel, los, dev_t(be, pos1), dev_t(be, blk1), dev_t(be, pos2), dev_t(be, blk2), grid,
                        list(box), dev_t(be, e * e), dev_t(be, given_sub(base, sub)))


def ref_local(kernel, box, edges, pos1, blk1, pos2=None, blk2=None, sub=None, los=2):
    """the restatement of run_local (the self pairs of one set passed as both are pairs)"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    a = wrap(numpy.asarray(pos1).astype('f8'), box)
    b = a if pos2 is None else wrap(numpy.asarray(pos2).astype('f8'), box)
    return label_core(a, b, box, kernel, los, e * e, given_sub(kernel.split('-', 1)[1], sub), blk1,
                      blk1 if blk2 is None else blk2)


def interior(n, seed, b, dtype='f8'):
    """uniform rows in [b / 2, 1 - b / 2): what the midpoint modes ask of the public calls"""
    return (b / 2 + uniform(n, 3, seed) * (1 - b) * (1 - 2.0 ** -20)).astype(dtype)


def random_labels(n, nlab, seed, unlabelled=0.0):
    rng = numpy.random.RandomState(seed)
    lab = rng.randint(0, nlab, size=n)
    return numpy.where(rng.uniform(size=n) < unlabelled, -1, lab).astype('i8')


SUBS = {'1d': None, '2d': [0.0, 0.3, 0.7, 1.0], 'projected': [0.0, 0.04, 0.1], '2d-midpoint': [0.0, 0.3, 0.7, 1.0],
        'projected-midpoint': [0.0, 0.04, 0.1]}
EDGES = numpy.array([0.0, 0.05, 0.09, 0.12])


def base_case(base, form, dtype):
    """320 and 280 rows with dyadic weights and six labels, a tenth of the rows in nothing"""
    b = float(numpy.hypot(0.12, 0.1)) + 0.01                     # (room for an observer a little off the centre)
    kw = dict(pos1=interior(320, 11, b, dtype), w1=dyadic_weights(320, 12).astype(dtype), l1=random_labels(320, 6, 13, 0.1),
              sub=SUBS[base], los=1)
    if form == 'cross':
        kw.update(pos2=interior(280, 14, b, dtype), w2=dyadic_weights(280, 15).astype(dtype),
                  l2=random_labels(280, 6, 16, 0.1))
    return kw


def local_ref_of_case(kernel, kw):
    n1 = len(kw['pos1'])
    b2 = None if kw.get('pos2') is None else blk(len(kw['pos2']), kw['l2'], kw['w2'])
    return ref_local(kernel, UNIT, EDGES, kw['pos1'], blk(n1, kw['l1'], kw['w1']), kw.get('pos2'), b2, kw['sub'], kw['los'])


# ---- 1. the restatement on hand-computed answers, and the inputs (no GPU) --------------------------------------------------

LINE = dict(pos=numpy.array([[1 / 8.], [2 / 8.], [2 / 8.], [5 / 8.], [11 / 16.]]), lab=numpy.array([0, 0, 1, -1, 1]),
            w=numpy.array([1.0, 2.0, 0.5, 4.0, 1.0]))
# rows on a line, unordered pairs inside [0, 7/16): 0-1 at 1/8 (labels 0, 0: a == c), 0-2 at 1/8 (0, 1: a != c), 1-2
# coincident (0, 1), 1-3 and 2-3 at 3/8 (a row in nothing), 3-4 at 1/16 (nothing, 1); 0-3 at 1/2 and 0-4, 1-4, 2-4 at
# 7/16 are outside.  Every ordered pair counts: twice the unordered ones.
LINE_ANSWER = {
    0.0: dict(total=([8, 4], [15.0, 20.0]), same=([2, 0], [4.0, 0.0]), side0=([8, 2], [11.0, 16.0]),
              side1=([6, 2], [11.0, 4.0]), same0=([2, 0], [4.0, 0.0]), same1=([0, 0], [0.0, 0.0])),
    # with edges[0] = 1/16 the coincident pair 1-2 is in no bin
    1 / 16.: dict(total=([6, 4], [13.0, 20.0]), same=([2, 0], [4.0, 0.0]), side0=([6, 2], [9.0, 16.0]),
                  side1=([4, 2], [9.0, 4.0]), same0=([2, 0], [4.0, 0.0]), same1=([0, 0], [0.0, 0.0]))}
PLANE = dict(pos1=numpy.array([[1 / 4., 1 / 4.], [1 / 2., 1 / 4.]]), lab1=numpy.array([0, 1]),
             pos2=numpy.array([[1 / 4., 1 / 2.], [1 / 2., 1 / 2.], [1 / 4., 1 / 4.]]), lab2=numpy.array([0, 0, -1]))
# in a plane, cross, one bin [0, 3/8): all six pairs are inside (1/4, sqrt(1/8) and one coincident pair); the first
# primary (label 0) meets two rows of label 0 (same) and a row in nothing; the second (label 1) meets label 0 twice and
# the row in nothing
PLANE_ANSWER = dict(total=6, same=2, side0=7, side1=3, same0=2, same1=0)


def test_restatement_on_hand_computed_answers():
    for first, want in LINE_ANSWER.items():
        e = numpy.array([first, 3 / 16., 7 / 16.])
        b = blk(5, LINE['lab'], LINE['w'])
        sp = label_core(LINE['pos'], LINE['pos'], [1.0], 'split-1d', 2, e * e, None, b, b, skip_diagonal=True)
        jk = label_core(LINE['pos'], LINE['pos'], [1.0], 'jackknife-1d', 2, e * e, None, b, b, skip_diagonal=True)
        K = jk['K']
        assert K == 1023 and len(jk['npairs']) == (1 + 2 * K) * 2 and len(jk['rsum']) == 2 and len(sp['npairs']) == 4
        for arr, col in (('npairs', 0), ('wnpairs', 1)):
            assert sp[arr][2:].tolist() == want['same'][col]
            assert (sp[arr][:2] + sp[arr][2:]).tolist() == want['total'][col]
            assert jk[arr][:2].tolist() == want['total'][col]
            assert jk[arr][2:4].tolist() == want['side0'][col] and jk[arr][4:6].tolist() == want['side1'][col]
            s0 = 2 * (1 + K)
            assert jk[arr][s0:s0 + 2].tolist() == want['same0'][col] and jk[arr][s0 + 2:s0 + 4].tolist() == want['same1'][col]
            assert jk[arr][6:s0].sum() == 0 and jk[arr][s0 + 4:].sum() == 0
    e2 = numpy.array([0.0, 9 / 64.])
    b1, b2 = blk(2, PLANE['lab1']), blk(3, PLANE['lab2'])
    sp = label_core(PLANE['pos1'], PLANE['pos2'], [1.0, 1.0], 'split-1d', 2, e2, None, b1, b2)
    jk = label_core(PLANE['pos1'], PLANE['pos2'], [1.0, 1.0], 'jackknife-1d', 2, e2, None, b1, b2)
    K = jk['K']
    assert K == 2047 and sp['npairs'].tolist() == [4, 2]
    assert [int(jk['npairs'][k]) for k in (0, 1, 2, 1 + K, 2 + K)] == [6, 7, 3, 2, 0] and jk['npairs'].sum() == 18
    # a NaN, an infinite and a negative label are no label, and the same as nothing; so is one at or above K
    odd = blk(3, [numpy.nan, numpy.inf, -2.0])
    sp = label_core(PLANE['pos2'], PLANE['pos2'], [1.0, 1.0], 'split-1d', 2, e2, None, odd, odd)
    assert sp['npairs'].tolist() == [9, 0]
    jk = label_core(PLANE['pos2'], PLANE['pos2'], [1.0, 1.0], 'jackknife-1d', 2, e2, None, odd, blk(3, [K, K + 1, 2.0 ** 40]))
    assert jk['npairs'][0] == 9 and jk['npairs'][1:].sum() == 0


def test_inputs_are_decided():
    for base in LABEL_BASES:
        for form in ('auto', 'cross'):
            ref = local_ref_of_case('split-' + base, base_case(base, form, 'f8'))
            assert ref['margin'] >= 1e-9, (base, form, ref['margin'])
            assert ref['npairs'][:ref['nbins']].sum() > 200 and ref['npairs'][ref['nbins']:].sum() > 50


# ---- 2. hand-computed answers through the public calls -----------------------------------------------------------------------

def test_hand_computed_answers(lbe):
    pm = mesh([1.0])
    for first, want in LINE_ANSWER.items():
        e = [first, 3 / 16., 7 / 16.]
        sc = pair_counts_split(pm, LINE['pos'], LINE['lab'], e, weight1=LINE['w'])
        assert isinstance(sc, SplitCounts) and isinstance(sc.same, PairCounts) and sc.same.auto and sc.same.mode == '1d'
        assert cpu(sc.same.npairs).tolist() == want['same'][0] and cpu(sc.same.wnpairs).tolist() == want['same'][1]
        assert cpu(sc.total.npairs).tolist() == want['total'][0] and cpu(sc.total.wnpairs).tolist() == want['total'][1]
        assert torch.equal(sc.same.npairs + sc.different.npairs, sc.total.npairs)
        jk = pair_counts_jackknife(pm, LINE['pos'], LINE['lab'], e, 2, weight1=LINE['w'])
        assert isinstance(jk, JackknifeCounts) and jk.ncalls == 1 and jk.nlab == 2
        assert cpu(jk.total.npairs).tolist() == want['total'][0] and cpu(jk.total.wnpairs).tolist() == want['total'][1]
        for arr, col in ((jk.side_npairs, 0), (jk.side_wnpairs, 1)):
            assert cpu(arr).tolist() == [want['side0'][col], want['side1'][col]]
        for arr, col in ((jk.same_npairs, 0), (jk.same_wnpairs, 1)):
            assert cpu(arr).tolist() == [want['same0'][col], want['same1'][col]]
        assert jk.W1_k.tolist() == [3.0, 1.5] and jk.W2sum_k.tolist() == [5.0, 1.25] and jk.total.W1 == 8.5
    pm = mesh([1.0, 1.0])
    sc = pair_counts_split(pm, PLANE['pos1'], PLANE['lab1'], [0.0, 3 / 8.], pos2=PLANE['pos2'], label2=PLANE['lab2'])
    assert cpu(sc.same.npairs).tolist() == [2] and cpu(sc.different.npairs).tolist() == [4] and not sc.total.auto
    jk = pair_counts_jackknife(pm, PLANE['pos1'], PLANE['lab1'], [0.0, 3 / 8.], 2, pos2=PLANE['pos2'], label2=PLANE['lab2'])
    assert cpu(jk.side_npairs).tolist() == [[7], [3]] and cpu(jk.same_npairs).tolist() == [[2], [0]]
    assert cpu(jk.total.npairs).tolist() == [6] and jk.W2_k.tolist() == [2.0, 0.0] and jk.W2sum_k.tolist() == [0.0, 0.0]
    # without region 0 the second primary and the row in nothing are left: one pair; without region 1 three
    assert cpu(jk.realization_counts(0).npairs).tolist() == [1] and cpu(jk.realization_counts(1).npairs).tolist() == [3]


# ---- 3. the defining equalities ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('form', ['auto', 'cross'])
@pytest.mark.parametrize('base', LABEL_BASES)
def test_the_entry_against_the_restatement(lbe, base, form, dtype):
    """both families in every base mode, at the level of local_counts: every slot of the three arrays"""
    kw = base_case(base, form, dtype)
    n1 = len(kw['pos1'])
    b1 = blk(n1, kw['l1'], kw['w1'], dtype)
    b2 = None if form == 'auto' else blk(len(kw['pos2']), kw['l2'], kw['w2'], dtype)
    for family in ('split', 'jackknife'):
        kernel = '%s-%s' % (family, base)
        got = run_local(lbe, kernel, UNIT, EDGES, kw['pos1'], b1, kw.get('pos2'), b2, kw['sub'], kw['los'])
        check_arrays(got, ref_local(kernel, UNIT, EDGES, kw['pos1'], b1, kw.get('pos2'), b2, kw['sub'], kw['los']),
                     what=(kernel, form, dtype))


def public_kw(base, kw):
    out = dict(pos2=kw.get('pos2'), weight1=kw['w1'], weight2=kw.get('w2'), mode=base)
    if base == '2d':
        out.update(muedges=kw['sub'], los=kw['los'])
    elif base == 'projected':
        out.update(piedges=kw['sub'], los=kw['los'])
    return out


@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('form', ['auto', 'cross'])
@pytest.mark.parametrize('base', BOX_MODES)
def test_defining_equalities(lbe, base, form, dtype):
    """same + different == pair_counts, JackknifeCounts.total == pair_counts, sum_k side_k == 2 total when every row
    has a label, sum_k same_k == SplitCounts.same"""
    kw = base_case(base, form, dtype)
    pm = mesh(UNIT)
    pk = public_kw(base, kw)
    pc = pair_counts(pm, kw['pos1'], EDGES, **pk)
    sc = pair_counts_split(pm, kw['pos1'], kw['l1'], EDGES, label2=kw.get('l2'), **pk)
    assert torch.equal(sc.same.npairs + sc.different.npairs, pc.npairs) and int(sc.same.npairs.sum()) > 0
    assert torch.equal(sc.same.wnpairs + sc.different.wnpairs, pc.wnpairs)
    same_counts(sc.total, pc, what=(base, form, 'split'))
    assert (sc.total.W1, sc.total.W2, sc.total.W2sum) == (pc.W1, pc.W2, pc.W2sum) and sc.same.npairs.shape == pc.npairs.shape
    jk = pair_counts_jackknife(pm, kw['pos1'], kw['l1'], EDGES, 6, label2=kw.get('l2'), **pk)
    same_counts(jk.total, pc, what=(base, form, 'jackknife'))
    assert jk.side_npairs.shape == (6,) + tuple(pc.npairs.shape) == tuple(jk.same_wnpairs.shape)
    assert torch.equal(jk.same_npairs.sum(dim=0), sc.same.npairs) and torch.equal(jk.same_wnpairs.sum(dim=0), sc.same.wnpairs)
    # every row in a region
    l1 = numpy.where(kw['l1'] < 0, 5, kw['l1'])
    l2 = None if form == 'auto' else numpy.where(kw['l2'] < 0, 0, kw['l2'])
    jk = pair_counts_jackknife(pm, kw['pos1'], l1, EDGES, 6, label2=l2, **pk)
    assert torch.equal(jk.side_npairs.sum(dim=0), 2 * pc.npairs) and torch.equal(jk.side_wnpairs.sum(dim=0), 2 * pc.wnpairs)
    assert abs(jk.W1_k.sum() - pc.W1) == 0 and abs(jk.W2_k.sum() - pc.W2) == 0


@pytest.mark.parametrize('form', ['auto', 'cross'])
@pytest.mark.parametrize('mode', ['1d', '2d', 'projected', 'angular'])
def test_survey_forms(lbe, mode, form):
    kw = base_case({'1d': '1d', 'angular': '1d'}.get(mode, mode + '-midpoint'), form, 'f8')
    pm = mesh(UNIT)
    obs = [0.5, 0.5, 0.5 + 2.0 ** -9]
    pk = dict(observer=obs, pos2=kw.get('pos2'), weight1=kw['w1'], weight2=kw.get('w2'), mode=mode)
    if mode == '2d':
        pk.update(muedges=kw['sub'])
    elif mode == 'projected':
        pk.update(piedges=kw['sub'])
    elif mode == 'angular':
        pk.update(thetaedges=[0.0, 4.0, 9.0, 15.0])
    pc = survey_pair_counts(pm, kw['pos1'], EDGES, **pk)
    l1 = numpy.where(kw['l1'] < 0, 5, kw['l1'])
    l2 = None if form == 'auto' else numpy.where(kw['l2'] < 0, 0, kw['l2'])
    jk = survey_pair_counts_jackknife(pm, kw['pos1'], l1, EDGES, 6, label2=l2, **pk)
    assert isinstance(jk.total, SurveyPairCounts) and jk.total.los == 'midpoint' and jk.total.observer.tolist() == obs
    same_counts(jk.total, pc, what=(mode, form))
    assert int(pc.npairs.sum()) > 100 and torch.equal(jk.side_npairs.sum(dim=0), 2 * pc.npairs)
    assert (jk.total.theta is None) == (mode != 'angular')
    k = 2
    keep1 = l1 != k
    sub = dict(pk, weight1=kw['w1'][keep1])
    if form == 'cross':
        sub.update(pos2=kw['pos2'][l2 != k], weight2=kw['w2'][l2 != k])
    less = survey_pair_counts(pm, kw['pos1'][keep1], EDGES, **sub)
    got = jk.realization_counts(k)
    assert torch.equal(got.npairs, less.npairs) and torch.equal(got.wnpairs, less.wnpairs)


# ---- 4. delete-one and the split for real -----------------------------------------------------------------------------------

@pytest.mark.parametrize('base,form', [('1d', 'auto'), ('1d', 'cross'), ('2d', 'auto'), ('projected', 'cross')])
def test_delete_one_for_real(lbe, base, form):
    """600 rows in the 8 octants of box_regions: for every k, realization_counts(k) is pair_counts of the rows whose
    label is not k, and norm_k that call's W1 W2 - W2sum (dyadic weights: exact)"""
    pm = mesh(UNIT)
    p1, w1 = uniform(600, 3, 21), dyadic_weights(600, 22)
    l1 = cpu(box_regions(pm, p1, 2))
    assert sorted(set(l1.tolist())) == list(range(8))
    pk = dict(weight1=w1, mode=base)
    if base == '2d':
        pk.update(Nmu=3, los=0)
    elif base == 'projected':
        pk.update(piedges=[0.0, 0.05, 0.1], los=1)
    p2 = w2 = l2 = None
    if form == 'cross':
        p2, w2 = uniform(500, 3, 23), dyadic_weights(500, 24)
        l2 = cpu(box_regions(pm, p2, [2, 2, 2]))
        pk.update(pos2=p2, weight2=w2)
    edges = [0.0, 0.06, 0.1, 0.13]
    jk = pair_counts_jackknife(pm, p1, l1, edges, 8, label2=l2, **pk)
    assert jk.ncalls == 1
    for k in range(8):
        keep = l1 != k
        sub = dict(pk, weight1=w1[keep])
        if form == 'cross':
            sub.update(pos2=p2[l2 != k], weight2=w2[l2 != k])
        less = pair_counts(pm, p1[keep], edges, **sub)
        got = jk.realization_counts(k)
        assert torch.equal(got.npairs, less.npairs) and torch.equal(got.wnpairs, less.wnpairs), k
        assert (got.W1, got.W2, got.W2sum) == (less.W1, less.W2, less.W2sum)
        wn, norm = jk.realization(k)
        assert torch.equal(wn, less.wnpairs) and norm == less.W1 * less.W2 - less.W2sum
        assert norm == jk.norms()[k] and int(less.npairs.sum()) > 500


def test_box_regions(lbe):
    pm = mesh(SLAB)
    pos = numpy.array([[0.0, 0.0, 0.0], [0.49, 0.24, 0.12], [0.5, 0.25, 0.125], [1.5, -0.01, 0.3], [numpy.nan, 0.1, 0.1]])
    # the fourth row wraps to (0.5, 0.49, 0.05): the cells (1, 1, 0) of 2 x 2 x 2 and (0, 2, 0) of 1 x 3 x 2
    assert cpu(box_regions(pm, pos, 2)).tolist() == [0, 0, 7, 6, -1]
    assert cpu(box_regions(pm, pos, [1, 3, 2])).tolist() == [0, 2, 3, 4, -1]
    assert box_regions(pm, pos.astype('f4'), 2).dtype == torch.int64
    with pytest.raises(ValueError, match='nsub'):
        box_regions(pm, pos, 0)
    with pytest.raises(ValueError, match='nsub'):
        box_regions(pm, pos, [2, 2])


def test_split_for_real(lbe):
    """.same is the sum over the labels of pair_counts of that label's rows alone; one label is 2^40, which only a
    float64 block holds"""
    pm = mesh(UNIT)
    pos, w = 0.3 + 0.2 * uniform(400, 3, 31), dyadic_weights(400, 32)
    names = numpy.array([-1, 0, 3, 70000, 2 ** 40])
    lab = names[numpy.random.RandomState(33).randint(0, 5, size=400)]
    edges = [0.0, 0.05, 0.1]
    sc = pair_counts_split(pm, pos.astype('f4'), lab, edges, weight1=w.astype('f4'))
    n, wn = torch.zeros_like(sc.same.npairs), torch.zeros_like(sc.same.wnpairs)
    for name in names[1:]:
        pc = pair_counts(pm, pos.astype('f4')[lab == name], edges, weight1=w[lab == name])
        n, wn = n + pc.npairs, wn + pc.wnpairs
    assert torch.equal(sc.same.npairs, n) and torch.equal(sc.same.wnpairs, wn) and int(n.sum()) > 1000
    # 2^40 + 1 is another host: in a float32 block the two would be one
    lab2 = numpy.where(numpy.arange(400) % 2 == 0, 2 ** 40, 2 ** 40 + 1)
    sc = pair_counts_split(pm, pos, lab2, edges)
    even, odd = pair_counts(pm, pos[::2], edges), pair_counts(pm, pos[1::2], edges)
    assert torch.equal(sc.same.npairs, even.npairs + odd.npairs)
    with pytest.raises(ValueError, match='labels'):
        pair_counts_split(pm, pos, numpy.full(400, 2 ** 53), edges)
    xi1, xi2, sc = pair_correlation_split(pm, pos, lab, edges, weight1=w)
    xi, pc = pair_correlation(pm, pos, edges, weight1=w)
    assert torch.equal(sc.total.wnpairs, pc.wnpairs)
    # same + different == total exactly (dyadic weights); each of the three xi carries the rounding of its division and
    # of its "- 1", each at most U max(1, 1 + xi), and the four additions here as much again
    d = cpu(torch.abs((1 + xi) - ((1 + xi1) + (1 + xi2))))
    assert (d <= 10 * U * numpy.maximum(1, cpu(1 + xi))).all()


def test_friends_lie_in_the_one_halo_term(lbe):
    """minid of fof as the label: two rows closer than the linking length are friends, hence in one group: no pair
    below b is in .different"""
    pm = mesh(UNIT)
    rng = numpy.random.RandomState(41)
    centres = uniform(12, 3, 42)
    pos = wrap((centres[:, None, :] + 0.01 * rng.normal(size=(12, 25, 3))).reshape(-1, 3), UNIT)
    b = 0.012
    res = fof(pm, pos, b, nmin=1)
    sc = pair_counts_split(pm, pos, res.minid, [0.0, b / 2, b, 3 * b])
    assert cpu(sc.different.npairs)[:2].tolist() == [0, 0] and cpu(sc.same.npairs)[:2].min() > 50
    assert int(sc.different.npairs[2]) > 0
    # labels > 0 alone: the rows of groups below nmin are in nothing
    res = fof(pm, pos, b, nmin=5)
    lab = torch.where(res.labels > 0, res.labels, torch.full_like(res.labels, -1))
    sc2 = pair_counts_split(pm, pos, lab, [0.0, b / 2, b, 3 * b])
    assert torch.equal(sc2.total.npairs, sc.total.npairs) and int(sc2.same.npairs.sum()) <= int(sc.same.npairs.sum())


# ---- 5. wave, workgroup and slot edges ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('n1', [63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(lbe, n1):
    b = 0.2
    p1, p2 = uniform(n1, 3, 300 + n1), uniform(300, 3, 51)
    b1 = blk(n1, random_labels(n1, 4, 310 + n1, 0.1), dyadic_weights(n1, 320 + n1))
    b2 = blk(300, random_labels(300, 4, 52, 0.1), dyadic_weights(300, 53))
    for kernel in ('split-1d', 'jackknife-1d'):
        ref = ref_local(kernel, UNIT, [0.0, 0.4 * b, b], p1, b1, p2, b2)
        assert ref['margin'] >= 1e-9 and ref['npairs'].sum() > 100
        check_arrays(run_local(lbe, kernel, UNIT, [0.0, 0.4 * b, b], p1, b1, p2, b2), ref, what=(kernel, n1))


def delete_check(pm, jk, pos, lab, w, edges, ks, **kw):
    for k in ks:
        keep = lab != k
        less = pair_counts(pm, pos[keep], edges, weight1=w[keep], **kw)
        got = jk.realization_counts(k)
        assert torch.equal(got.npairs, less.npairs) and torch.equal(got.wnpairs, less.wnpairs), k


@pytest.mark.parametrize('nlab,ncalls', [(50, 1), (51, 2), (101, 3)])
def test_more_labels_than_one_call(lbe, nlab, ncalls):
    """40 bins: K = 50; 51 labels take two calls and 101 three, the last with one label"""
    pm = mesh(UNIT)
    assert label_slots(40) == 50
    pos, w = uniform(500, 3, 61), dyadic_weights(500, 62)
    lab = random_labels(500, nlab, 63, 0.05)
    lab[:nlab] = numpy.arange(nlab)
    edges = numpy.linspace(0.0, 0.2, 41)
    jk = pair_counts_jackknife(pm, pos, lab, edges, nlab, weight1=w)
    assert jk.ncalls == ncalls and tuple(jk.side_npairs.shape) == (nlab, 40)
    pc = pair_counts(pm, pos, edges, weight1=w)
    same_counts(jk.total, pc)
    sc = pair_counts_split(pm, pos, lab, edges, weight1=w)
    assert torch.equal(jk.same_npairs.sum(dim=0), sc.same.npairs) and torch.equal(jk.same_wnpairs.sum(dim=0), sc.same.wnpairs)
    delete_check(pm, jk, pos, lab, w, edges, [0, 49, nlab - 1])


def test_the_most_bins(lbe):
    """1024 bins: K = 1 and three labels take three calls, as 1d and as 32 x 32"""
    pm = mesh(UNIT)
    assert label_slots(1024) == 1 and MAX_BINS == 1024
    pos, w = uniform(500, 3, 64), dyadic_weights(500, 65)
    lab = random_labels(500, 3, 66, 0.05)
    for edges, kw in ((numpy.linspace(0.0, 0.2, 1025), {}),
                      (numpy.linspace(0.0, 0.2, 33), dict(mode='projected', piedges=numpy.linspace(0.0, 0.2, 33), los=0))):
        jk = pair_counts_jackknife(pm, pos, lab, edges, 3, weight1=w, **kw)
        assert jk.ncalls == 3 and jk.side_npairs.numel() == 3 * 1024
        same_counts(jk.total, pair_counts(pm, pos, edges, weight1=w, **kw))
        delete_check(pm, jk, pos, lab, w, edges, [0, 1, 2], **kw)
        sc = pair_counts_split(pm, pos, lab, edges, weight1=w, **kw)
        assert torch.equal(jk.same_npairs.sum(dim=0), sc.same.npairs)


def test_too_many_bins(obe):
    pm, pos, lab = mesh(UNIT), uniform(50, 3, 1), numpy.zeros(50, dtype='i8')
    for call in (lambda e, **kw: pair_counts_jackknife(pm, pos, lab, e, 1, **kw),
                 lambda e, **kw: pair_counts_split(pm, pos, lab, e, **kw)):
        with pytest.raises(ValueError, match='bins'):
            call(numpy.linspace(0, 0.2, 1026))
        with pytest.raises(ValueError, match='bins'):
            call(numpy.linspace(0, 0.2, 42), mode='2d', Nmu=25)
    with pytest.raises(ValueError, match='bins'):
        run_local(obe, 'jackknife-1d', UNIT, numpy.linspace(0, 0.2, 1026), pos, blk(50, lab))


def entry_rc(ndim, mode, nr, nsub=1):
    """pmx_pair_counts with no rows: it returns before it touches the device"""
    import ctypes as C
    lib = backend.load_library()
    return lib.pmx_pair_counts(ndim, mode, 2, 0, None, None, None, None, 0, None, None, None, None,
                               _abi.i64arr([1, 1, 1], 3), 7, _abi.f64arr(UNIT, 3), nr, None, nsub, None, None, None,
                               None, C.c_void_p(0))


def test_the_entry_accepts_the_modes():
    """16 .. 20 and 32 .. 36 are taken; 10 .. 15, 21 .. 31 and 37 (and 48, both flags) are PMX_EINVAL; so are 1025
    bins, the 2d and projected forms in two dimensions, and two sub-bins in a 1d form"""
    nsub = lambda mode: 1 if mode & 7 == 0 else 2
    for mode in list(range(16, 21)) + list(range(32, 37)):
        assert entry_rc(3, mode, 4, nsub(mode)) == _abi.PMX_OK, mode
    for mode in list(range(10, 16)) + list(range(21, 32)) + [37, 38, 39, 40, 48, 52, 64, -16]:
        assert entry_rc(3, mode, 4, nsub(mode)) == _abi.PMX_EINVAL, mode
    for flag in (16, 32):
        assert [entry_rc(3, flag, 1024), entry_rc(3, flag, 1025), entry_rc(3, flag | 2, 32, 32), entry_rc(3, flag | 2, 41, 25),
                entry_rc(3, flag | 3, 41, 25)] == [0, _abi.PMX_EINVAL, 0, _abi.PMX_EINVAL, _abi.PMX_EINVAL]
        assert [entry_rc(2, flag, 4), entry_rc(1, flag, 4), entry_rc(3, flag, 4, 2)] == [0, 0, _abi.PMX_EINVAL]
        assert [entry_rc(2, flag | m, 4, 2) for m in (1, 2, 3, 4)] == [_abi.PMX_EINVAL] * 4


@pytest.mark.gpu
def test_the_entry_refuses_wrong_columns(hipbe):
    """a block of one or three columns, or none, on either side: PMX_EINVAL from the entry itself, in both families;
    and the guards of Backend.pair_counts in front of it: arrays that the kernel would overrun"""
    import ctypes as C
    from pmesh_amd.backend import PmxError
    dev = hipbe.device
    pos = torch.from_numpy(uniform(50, 3, 1)).to(dev)
    blocks = {n: torch.ones((50, n), dtype=torch.float64, device=dev) for n in (1, 2, 3)}
    grid = cell_grid(50, 0.2, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(hipbe, pos, grid, UNIT)
    e2 = torch.from_numpy(numpy.linspace(0, 0.2, 5) ** 2).to(dev)
    outs = lambda n: (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
                      torch.zeros(n, dtype=torch.float64, device=dev))

    def call(mode, w1, w2):
        out = outs(4096)
        wv1, wv2 = backend._arrays.vec(w1), backend._arrays.vec(w2)
        hipbe.call('pair_counts', 3, int(mode), 2, 50, spos.data_ptr(), order.data_ptr(), cell_of.data_ptr(),
                   C.byref(wv1) if w1 is not None else None, 50, spos.data_ptr(), order.data_ptr(),
                   cell_start.data_ptr(), C.byref(wv2) if w2 is not None else None, _abi.i64arr(grid[0], 3),
                   int(grid[3]), _abi.f64arr(UNIT, 3), 4, e2.data_ptr(), 1, None, out[0].data_ptr(), out[1].data_ptr(),
                   out[2].data_ptr(), hipbe.stream())
        return out
    for mode in (16, 32):
        for w1, w2 in ((blocks[2], blocks[3]), (blocks[1], blocks[2]), (None, blocks[2]), (blocks[2], None)):
            with pytest.raises(PmxError, match='columns'):
                call(mode, w1, w2)
        # every row has the label 1: the 50 self pairs alone are 50 pairs of the kind 1, or of all, side[1] and same[1]
        taken = call(mode, blocks[2], blocks[2])[0]
        assert int((taken[4:8] if mode == 16 else taken[:4]).sum()) >= 50 and (mode == 32 or int(taken[:4].sum()) == 0)
        for w1, n in ((blocks[2], 4), (blocks[3], 4096), (None, 4096)):
            with pytest.raises(ValueError, match='label'):
                hipbe.pair_counts(mode, 2, spos, order, cell_of, w1, spos, order, cell_start, blocks[2], grid[0], grid[3],
                                  UNIT, e2, None, *outs(n))


# ---- 6. contention, labels out of range, grids ---------------------------------------------------------------------------------

def test_contention(lbe):
    """300 rows in one cell: alternating labels, all rows in one label, every row its own label"""
    pm = mesh(UNIT)
    pos = 0.5 + (lattice_rows(300, 3, 71) - 0.5) * 2.0 ** -5
    w = dyadic_weights(300, 72)
    edges = [0.0, 1 / 128., 1 / 64., 1 / 32.]
    pc = pair_counts(pm, pos, edges, weight1=w)
    assert int(pc.npairs.sum()) > 50000
    for name, lab in (('alternating', numpy.arange(300) % 2), ('one', numpy.zeros(300, dtype='i8')),
                      ('own', numpy.arange(300))):
        for kernel in ('split-1d', 'jackknife-1d'):
            b1 = blk(300, lab, w)
            check_arrays(run_local(lbe, kernel, UNIT, edges, pos, b1), ref_local(kernel, UNIT, edges, pos, b1),
                         what=(name, kernel))
        sc = pair_counts_split(pm, pos, lab, edges, weight1=w)
        assert torch.equal(sc.same.npairs + sc.different.npairs, pc.npairs)
        if name == 'one':
            assert torch.equal(sc.same.npairs, pc.npairs) and torch.equal(sc.same.wnpairs, pc.wnpairs)
        if name == 'own':
            assert int(sc.same.npairs.sum()) == 0 and float(sc.same.wnpairs.abs().sum()) == 0
        jk = pair_counts_jackknife(pm, pos, lab, edges, int(lab.max()) + 1, weight1=w)
        assert torch.equal(jk.side_npairs.sum(dim=0), 2 * pc.npairs) and torch.equal(jk.total.npairs, pc.npairs)
        assert torch.equal(jk.same_npairs.sum(dim=0), sc.same.npairs)


def test_labels_out_of_range_add_to_all_only(lbe):
    """8 bins: K = 255; rows with the labels 255, 256, 2^30, NaN, inf and -1 in a direct call touch no side and no same"""
    assert label_slots(8) == 255
    pos = uniform(400, 3, 73)
    odd = numpy.array([255.0, 256.0, 2.0 ** 30, numpy.nan, numpy.inf, -1.0, 254.0, 0.0])
    lab = odd[numpy.arange(400) % 8]
    edges = numpy.linspace(0.0, 0.2, 9)
    b1 = blk(400, lab, dyadic_weights(400, 74))
    got = [cpu(x) for x in run_local(lbe, 'jackknife-1d', UNIT, edges, pos, b1)]
    check_arrays(got, ref_local('jackknife-1d', UNIT, edges, pos, b1))
    n = got[0].reshape(511, 8)
    inside = [0, 1, 255, 256, 510]                               # all, side[0], side[254], same[0], same[254]
    assert n[inside].min(axis=1).min() >= 0 and n[[0, 1, 255]].sum(axis=1).min() > 0
    assert n[[k for k in range(511) if k not in inside]].sum() == 0
    # the split: none of them is the same as anything but 254 and 0, and inf is not the same as inf
    got = [cpu(x) for x in run_local(lbe, 'split-1d', UNIT, edges, pos, b1)]
    check_arrays(got, ref_local('split-1d', UNIT, edges, pos, b1))
    only = blk(400, numpy.where(lab == numpy.inf, numpy.inf, -1.0))
    assert cpu(run_local(lbe, 'split-1d', UNIT, edges, pos, only)[0])[8:].sum() == 0


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(lbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along periodic axes: both families in 3-d, 2-d and 1-d, and the projected and a midpoint form in 3-d"""
    for nd, base, sub in ((3, '1d', None), (2, '1d', None), (1, '1d', None), (3, 'projected', [0.0, 0.01, 0.05]),
                          (3, '2d-midpoint', [0.0, 0.5, 1.0])):
        box = SLAB[:nd]
        rows = numpy.concatenate([face_pairs(box, 0.05), uniform(300, nd, 61, box)])
        b1 = blk(len(rows), random_labels(len(rows), 3, 75, 0.1), dyadic_weights(len(rows), 76))
        edges = [0.0, 0.02, 0.04, 0.05]
        for family in ('split', 'jackknife'):
            kernel = '%s-%s' % (family, base)
            ref = ref_local(kernel, box, edges, rows, b1, sub=sub, los=0)
            assert ref['margin'] >= 1e-9
            got = run_local(lbe, kernel, box, edges, rows, b1, sub=sub, los=0, grid=grid_of(grid[:nd], box))
            check_arrays(got, ref, what=(kernel, nd, grid))


def test_open_axes(lbe):
    """a grid that is open along two axes (a rank's block): the rows of the block against all rows"""
    pos = uniform(2000, 3, 12)
    lab = random_labels(2000, 5, 77, 0.1)
    grid = cell_grid(len(pos), 0.05, UNIT, lo=[0.25, 0.0, 0.5], hi=[0.75, 1.0, 0.75])
    assert grid[3] == 2
    inside = ((pos[:, 0] >= 0.25) & (pos[:, 0] < 0.75) & (pos[:, 2] >= 0.5) & (pos[:, 2] < 0.75))
    edges = [0.01, 0.03, 0.05]
    for kernel in ('split-1d', 'jackknife-1d'):
        b1, b2 = blk(int(inside.sum()), lab[inside]), blk(2000, lab)
        ref = ref_local(kernel, UNIT, edges, pos[inside], b1, pos, b2)
        assert ref['margin'] >= 1e-9 and ref['npairs'][:2].min() > 10
        check_arrays(run_local(lbe, kernel, UNIT, edges, pos[inside], b1, pos, b2, grid=grid), ref)


@pytest.mark.gpu
def test_more_secondaries_than_one_launch(hipbe):
    """300 primaries against 2^23 + 1000 secondaries: the entry launches once per window of 2^23 slots of the
    secondaries, and the cell that holds slot 2^23 is split between two launches; eight of the primaries sit in it.  No
    brute force at this size: the sums against all secondaries equal the sums against their two halves, each within one
    launch.  Unit weights: npairs and wnpairs exactly"""
    n2 = (1 << 23) + 1000
    dev = hipbe.device
    gen = torch.Generator(device=dev).manual_seed(5)
    p2 = torch.randint(0, 4096, (n2, 3), generator=gen, device=dev).to(torch.float64) / 4096
    pm = mesh(UNIT)
    l2 = box_regions(pm, p2, 2)
    edges = numpy.linspace(0.0, 0.02, 5)
    grid = cell_grid(n2, 0.02, UNIT)
    _, _, cell_start, _, _, _ = cell_sort(hipbe, p2, grid, UNIT)
    cell = int(torch.searchsorted(cell_start.to(torch.int64), torch.tensor([1 << 23], device=dev), right=True)[0]) - 1
    assert int(cell_start[cell]) < (1 << 23) < int(cell_start[cell + 1])
    axes = numpy.array(numpy.unravel_index(cell, grid[0]), dtype='f8')
    near = (axes + numpy.random.RandomState(3).randint(1, 8, size=(8, 3)) / 8.0) / numpy.asarray(grid[2])
    p1 = torch.from_numpy(numpy.concatenate([near, lattice_rows(292, 3, 9)])).to(dev)
    l1 = box_regions(pm, p1, 2)
    whole = pair_counts_jackknife(pm, p1, l1, edges, 8, pos2=p2, label2=l2)
    half = n2 // 2
    parts = [pair_counts_jackknife(pm, p1, l1, edges, 8, pos2=p2[:half], label2=l2[:half]),
             pair_counts_jackknife(pm, p1, l1, edges, 8, pos2=p2[half:], label2=l2[half:])]
    assert int(whole.total.npairs.sum()) > 50000
    for name in ('side_npairs', 'side_wnpairs', 'same_npairs', 'same_wnpairs'):
        assert torch.equal(getattr(whole, name), getattr(parts[0], name) + getattr(parts[1], name)), name
    assert torch.equal(whole.total.npairs, parts[0].total.npairs + parts[1].total.npairs)
    assert torch.equal(whole.side_npairs.sum(dim=0), 2 * whole.total.npairs)
    n = cpu(whole.total.npairs)
    want = 300 * n2 * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert (numpy.abs(n - want) < 6 * numpy.sqrt(want)).all()


# ---- 7. the estimator ------------------------------------------------------------------------------------------------------

def numpy_cov(x):
    x = x.reshape(len(x), -1)
    d = x - x.mean(axis=0)[None]
    return (len(x) - 1.0) / len(x) * (d.T @ d)


def ls_bound(dd, dr, rr):
    """how far two evaluations of (dd - dr - dr + rr) / rr may lie apart when the sums and the norms behind the three
    normalised counts are the same exact numbers: each count carries up to two roundings on either side (a division, or
    a reciprocal and a product), 4 U of it between the two; the three additions and the division five more of
    quantities no larger than S = |dd| + 2 |dr| + |rr|: 9 U S / |rr|"""
    return 9 * U * (numpy.abs(dd) + 2 * numpy.abs(dr) + numpy.abs(rr)) / numpy.abs(rr)


def test_estimator_on_a_lattice(lbe):
    """rows on a full 8^3 lattice and the 8 octants as regions, translates of one another: the sums of every region
    are the same numbers, so all realisations are one double, their mean (eight equal terms, a division by eight) is
    that double and cov is 0, for alpha = 1/2 without randoms; the identities of the sums"""
    pm = mesh(UNIT)
    g = (numpy.arange(8) + 0.5) / 8
    pos = numpy.stack([a.reshape(-1) for a in numpy.meshgrid(g, g, g, indexing='ij')], axis=1)
    lab = box_regions(pm, pos, 2)
    edges = [0.0, 0.13, 0.18, 0.23]                              # the neighbours at 1/8, sqrt(2)/8 and sqrt(3)/8
    jc = pair_correlation_jackknife(pm, pos, lab, edges, 8)
    assert isinstance(jc, JackknifeCorrelation) and jc.alpha == 0.5 and tuple(jc.realizations.shape) == (8, 3)
    assert cpu(jc.counts.total.npairs).tolist() == [512 * 6, 512 * 12, 512 * 8]
    real = cpu(jc.realizations)
    assert numpy.array_equal(real, real[[0] * 8])
    assert numpy.abs(cpu(jc.cov)).max() == 0 and tuple(jc.cov.shape) == (3, 3) and cpu(jc.error).tolist() == [0, 0, 0]
    xi, pc = pair_correlation(pm, pos, edges)
    # wnpairs_k / RR_k = (7/8 total) / (7/8 RR): the same number with three roundings more, each of 1 + xi
    assert torch.equal(jc.xi, xi) and (numpy.abs(real[0] - cpu(xi)) <= 8 * U * numpy.abs(1 + cpu(xi))).all()
    jk = jc.counts
    wn, norm = jk.realizations(0.5)
    assert torch.equal(wn.sum(dim=0), 7 * jk.total.wnpairs)
    assert float(norm.sum()) == 7 * (jk.total.W1 * jk.total.W2 - jk.total.W2sum)
    assert torch.equal(wn[3], jk.realization(3, 0.5)[0]) and float(norm[3]) == jk.realization(3, 0.5)[1]
    assert torch.equal(wn[3], jk.total.wnpairs - jk.side_wnpairs[3] / 2)


def test_estimator(lbe):
    """the identities and the covariance formula on random rows with dyadic weights; the rules about alpha"""
    pm = mesh(UNIT)
    pos, w = uniform(700, 3, 81), dyadic_weights(700, 82)
    lab = cpu(box_regions(pm, pos, [3, 2, 1]))
    edges = [0.0, 0.05, 0.1]
    jc = pair_correlation_jackknife(pm, pos, lab, edges, 6, weight1=w, mode='2d', Nmu=2)
    jk = jc.counts
    wn, norm = jk.realizations(0.5)
    assert torch.equal(wn.sum(dim=0), 5 * jk.total.wnpairs)
    assert float(norm.sum()) == 5 * (jk.total.W1 * jk.total.W2 - jk.total.W2sum)
    real = cpu(jc.realizations)
    assert real.shape == (6, 2, 2) and tuple(jc.cov.shape) == (4, 4) and tuple(jc.error.shape) == (2, 2)
    # the formula in numpy on the same realisations.  Sums of 6 terms in another order: the bound of check, (M + 4) U S.
    # The mean has S <= 6 max|x| / 6; the deviations d inherit its error e; an entry of cov is a sum of 6 products
    # (d_i + e)(d_j + e)
    want = numpy_cov(real)
    x = real.reshape(6, -1)
    e = 10 * U * numpy.abs(x).max()
    assert numpy.abs(cpu(jc.mean) - real.mean(axis=0)).max() <= e
    d = numpy.abs(x - x.mean(axis=0)[None]) + e
    S = 5 / 6. * (d.T @ d)
    assert (numpy.abs(cpu(jc.cov) - want) <= 10 * U * S + 5 / 6. * e * (d.sum(axis=0)[:, None] + d.sum(axis=0)[None, :])).all()
    assert torch.equal(jc.error, torch.sqrt(torch.diagonal(jc.cov)).reshape(2, 2)) and cpu(jc.error).min() > 0
    for alpha in (1.0, 0.0, 0.25):
        with pytest.raises(ValueError, match='alpha'):
            pair_correlation_jackknife(pm, pos, lab, edges, 6, alpha=alpha)
    # with randoms: Landy-Szalay of the totals is survey_correlation's formula on pair_counts; alpha defaults to 1 and the
    # realisation k is the estimator of the rows outside region k
    ran = uniform(900, 3, 83)
    rlab = cpu(box_regions(pm, ran, [3, 2, 1]))
    jr = pair_correlation_jackknife(pm, pos, lab, edges, 6, weight1=w, randoms1=ran, rlabel1=rlab)
    assert jr.alpha == 1.0 and sorted(jr.counts) == ['D1D2', 'D1R2', 'D2R1', 'R1R2'] and jr.counts['D2R1'] is jr.counts['D1R2']

    def ls(p, pw, r):
        dd, dr, rr = pair_counts(pm, p, edges, weight1=pw), pair_counts(pm, p, edges, pos2=r, weight1=pw), pair_counts(pm, r, edges)
        n = [cpu(c.wnpairs) / (c.W1 * c.W2 - c.W2sum) for c in (dd, dr, rr)]
        return (n[0] - n[1] - n[1] + n[2]) / n[2], ls_bound(*n)
    # dyadic weights: the sums and the norms are exact on both sides; the host arithmetic on them is not the same
    want, bound = ls(pos, w, ran)
    assert (numpy.abs(cpu(jr.xi) - want) <= bound).all()
    k = 4
    want, bound = ls(pos[lab != k], w[lab != k], ran[rlab != k])
    assert (numpy.abs(cpu(jr.realizations[k]) - want) <= bound).all()
    again = pair_correlation_jackknife(pm, pos, lab, edges, 6, weight1=w, randoms1=ran, rlabel1=rlab,
                                       R1R2=jr.counts['R1R2'])
    assert torch.equal(again.realizations, jr.realizations) and again.counts['R1R2'] is jr.counts['R1R2']


def test_survey_correlation_jackknife(lbe):
    pm = mesh(UNIT)
    b = 0.1
    data, ran = interior(500, 84, b), interior(800, 85, b)
    dl, rl = cpu(box_regions(pm, data, 2)), cpu(box_regions(pm, ran, 2))
    edges = [0.0, 0.05, 0.1]
    jc = survey_correlation_jackknife(pm, data, dl, ran, rl, edges, 8, mode='2d', Nmu=4)
    xi, counts = survey_correlation(pm, data, ran, edges, mode='2d', Nmu=4)
    assert tuple(jc.realizations.shape) == (8, 2, 4)
    # unit weights: the sums and the norms are exact on both sides, and the expression is survey_correlation's
    assert numpy.array_equal(cpu(jc.xi), cpu(xi), equal_nan=True) and jc.alpha == 1.0
    for key in counts:
        assert torch.equal(jc.counts[key].total.npairs, counts[key].npairs), key
    k = 5
    one, less = survey_correlation(pm, data[dl != k], ran[rl != k], edges, mode='2d', Nmu=4)
    n = [cpu(c.wnpairs) / (c.W1 * c.W2 - c.W2sum) for c in (less['D1D2'], less['D1R2'], less['R1R2'])]
    assert (numpy.abs(cpu(jc.realizations[k]) - cpu(one)) <= ls_bound(*n)).all() and numpy.isfinite(cpu(one)).all()
    poles = to_poles(jc.realizations[k], counts['D1D2'].muedges, [0, 2])
    assert tuple(poles.shape) == (2, 2)


# ---- 8. arguments, ranks -------------------------------------------------------------------------------------------------

def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos, lab = uniform(50, 3, 1), random_labels(50, 4, 2)
    e = [0.0, 0.1]
    with pytest.raises(ValueError, match='edges'):
        pair_counts_jackknife(pm, pos, lab, [0.2, 0.1], 4)
    with pytest.raises(ValueError, match='labels'):
        pair_counts_jackknife(pm, pos, lab, e, 3)
    with pytest.raises(ValueError, match='nlab'):
        pair_counts_jackknife(pm, pos, lab, e, 0)
    with pytest.raises(TypeError, match='label1'):
        pair_counts_jackknife(pm, pos, lab.astype('f8'), e, 4)
    with pytest.raises(ValueError, match='label1'):
        pair_counts_jackknife(pm, pos, lab[:49], e, 4)
    with pytest.raises(ValueError, match='label1'):
        pair_counts_split(pm, pos, None, e)
    with pytest.raises(ValueError, match='label2 needs pos2'):
        pair_counts_split(pm, pos, lab, e, label2=lab)
    with pytest.raises(ValueError, match='pos2 needs label2'):
        pair_counts_split(pm, pos, lab, e, pos2=pos)
    with pytest.raises(ValueError, match='weight1'):
        pair_counts_split(pm, pos, lab, e, weight1=numpy.ones(49))
    with pytest.raises(ValueError, match='mode'):
        pair_counts_split(pm, pos, lab, e, mode='angular')
    with pytest.raises(ValueError, match='three dimensions'):
        pair_counts_jackknife(mesh(UNIT[:2]), pos[:, :2], lab, e, 4, mode='2d', Nmu=2)
    with pytest.raises(ValueError, match='outside'):
        survey_pair_counts_jackknife(pm, pos, lab, e, 4)
    empty = pair_counts_jackknife(pm, numpy.zeros((0, 3)), numpy.zeros(0, dtype='i8'), e, 4)
    assert cpu(empty.total.npairs).tolist() == [0] and cpu(empty.side_npairs).tolist() == [[0]] * 4 and empty.W1_k.tolist() == [0] * 4
    one = pair_counts_jackknife(mesh(UNIT[:1]), pos[:, :1], lab, [0.0, 0.01], 4)
    assert int(one.total.npairs[0]) > 0 and torch.equal(one.side_npairs.sum(dim=0), 2 * one.total.npairs)


RANK_CASE = dict(pos1=uniform(900, 3, 44), pos2=uniform(700, 3, 45), w1=dyadic_weights(900, 46), w2=dyadic_weights(700, 47),
                 l1=random_labels(900, 7, 48, 0.1), l2=random_labels(700, 7, 49, 0.1), edges=numpy.linspace(0, 0.1, 5))


def ranks_arrays(size, np_, form):
    kw = RANK_CASE
    cross = form == 'cross'
    s1, s2 = split(900, size), split(700, size)[::-1]

    def body(comm):
        pm = mesh(UNIT, comm, np_)
        a, b = s1[comm.rank], s2[comm.rank]
        more = dict(pos2=kw['pos2'][b], label2=kw['l2'][b], weight2=kw['w2'][b]) if cross else {}
        jk = pair_counts_jackknife(pm, kw['pos1'][a], kw['l1'][a], kw['edges'], 7, weight1=kw['w1'][a], **more)
        sc = pair_counts_split(pm, kw['pos1'][a], kw['l1'][a], kw['edges'], weight1=kw['w1'][a], **more)
        return [cpu(x) for x in (jk.total.npairs, jk.total.wnpairs, jk.total.rsum, jk.side_npairs, jk.side_wnpairs,
                                 jk.same_npairs, jk.same_wnpairs, sc.same.npairs, sc.same.wnpairs, sc.same.rsum,
                                 sc.different.npairs, sc.different.rsum)] + [jk.W1_k, jk.W2_k, jk.W2sum_k]
    return thread_ranks(size, body)


def check_ranks(size, np_):
    for form in ('auto', 'cross'):
        results = ranks_arrays(size, np_, form)
        one = ranks_arrays_one(form)
        for r in range(size):
            for k, (got, want) in enumerate(zip(results[r], one)):
                if k in (2, 9, 11):
                    # rsum: twice the bound, M from the counts next to it
                    M = one[k - 2 if k != 11 else 10].astype('f8')
                    assert (numpy.abs(got - want) <= 2 * (M + 4) * U * numpy.abs(want)).all(), (form, r, k)
                else:
                    assert numpy.array_equal(got, want), (form, r, k)
                assert numpy.array_equal(got, results[0][k])


_ONE = {}


def ranks_arrays_one(form):
    if form not in _ONE:
        _ONE[form] = ranks_arrays_single(form)
    return _ONE[form]


def ranks_arrays_single(form):
    kw = RANK_CASE
    pm = mesh(UNIT)
    more = dict(pos2=kw['pos2'], label2=kw['l2'], weight2=kw['w2']) if form == 'cross' else {}
    jk = pair_counts_jackknife(pm, kw['pos1'], kw['l1'], kw['edges'], 7, weight1=kw['w1'], **more)
    sc = pair_counts_split(pm, kw['pos1'], kw['l1'], kw['edges'], weight1=kw['w1'], **more)
    return [cpu(x) for x in (jk.total.npairs, jk.total.wnpairs, jk.total.rsum, jk.side_npairs, jk.side_wnpairs,
                             jk.same_npairs, jk.same_wnpairs, sc.same.npairs, sc.same.wnpairs, sc.same.rsum,
                             sc.different.npairs, sc.different.rsum)] + [jk.W1_k, jk.W2_k, jk.W2sum_k]


@pytest.mark.parametrize('size,np_', RANKS[:2])
def test_ranks_give_the_one_rank_arrays(obe, size, np_):
    """2 and 3 thread ranks holding both sets split unevenly (one rank holds no rows): counts and the dyadic sums
    exactly, rsum within twice the bound, identical on every rank"""
    check_ranks(size, np_)


@pytest.mark.gpu
@pytest.mark.parametrize('size,np_', RANKS[:2])
def test_ranks_on_the_device(hipbe, size, np_):
    _ONE.clear()
    check_ranks(size, np_)
    _ONE.clear()


def test_ranks_raise_together(obe):
    pos, lab = uniform(90, 3, 2), random_labels(90, 4, 3)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        sl = slice(30 * comm.rank, 30 * comm.rank + 30)
        mine, l = pos[sl], lab[sl]
        edges = [0.0, 0.05]
        bad = l.copy()
        if comm.rank == 1:
            bad[3] = 4
        with pytest.raises(ValueError):
            pair_counts_jackknife(pm, mine, bad, edges, 4)
        with pytest.raises(TypeError):
            pair_counts_jackknife(pm, mine, l.astype('f4') if comm.rank == 2 else l, edges, 4)
        with pytest.raises(ValueError):
            pair_counts_split(pm, mine, l[:29] if comm.rank == 0 else l, edges)
        with pytest.raises(ValueError):
            pair_counts_split(pm, mine, l, numpy.linspace(0, 0.05, 1026 if comm.rank == 2 else 1025))
        with pytest.raises(ValueError):
            pair_counts_split(pm, mine, l, edges, label2=l if comm.rank == 1 else None)
        with pytest.raises(ValueError):
            pair_correlation_jackknife(pm, mine, l, edges, 4, alpha=1.0)
        jk = pair_counts_jackknife(pm, mine, l, edges, 4)
        assert torch.equal(jk.total.npairs, pair_counts(pm, mine, edges).npairs)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 9. streams ------------------------------------------------------------------------------------------------------------

STREAMS_PER_POOL = 32


@pytest.fixture(scope='module')
def side_streams():
    """The side streams of this module: one full round of torch's pool of 32 streams, drawn once and handed out in
    turn.  torch.cuda.Stream() walks that pool round robin, and the runtime maps its streams onto a few hardware queues,
    one of which the null stream uses: which pool stream a later module draws decides whether its side stream can
    overtake the null stream at all, the power condition of the delayed-producer tests (tests/test_streams.py:
    streams_are_unordered, checked once per session by whichever module comes first).  A full round leaves the pool
    where this module found it, so those modules draw the streams they drew before this module existed"""
    pool = [torch.cuda.Stream() for _ in range(STREAMS_PER_POOL)]
    taken = [0]

    def draw():
        taken[0] += 1
        return pool[(taken[0] - 1) % STREAMS_PER_POOL]
    return draw


@pytest.mark.gpu
@pytest.mark.parametrize('kernel', sorted(LABEL_MODES))
def test_capture_on_a_side_stream(hipbe, side_streams, kernel):
    """Backend.pair_counts in every new mode with the inputs sorted and the outputs allocated beforehand: the zeroing and
    the call captured into a graph on a side stream leave the poisoned outputs as they were (nothing ran eagerly or on
    another stream); the replay gives npairs of the null-stream call exactly"""
    from tests import test_streams as T
    dev = hipbe.device
    n = 1500
    base = kernel.split('-', 1)[1]
    pos = 0.05 + 0.9 * lattice_rows(n, 3, 30)
    b1 = blk(n, random_labels(n, 5, 31, 0.1), dyadic_weights(n, 32))
    e = numpy.linspace(0.0, 0.1, 9)
    sub = None if base == '1d' else (numpy.linspace(0.0, 1.0, 5) if base.startswith('2d') else numpy.linspace(0.0, 0.1, 5))
    given = given_sub(base, sub)
    ref = label_core(pos, pos, numpy.ones(3), kernel, 2, e * e, given, b1, b1)
    grid = cell_grid(n, float(numpy.hypot(0.1, 0.1)) * 1.0001, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(hipbe, torch.from_numpy(pos).to(dev), grid, UNIT)
    bt = torch.from_numpy(b1).to(dev)
    e2, subt = torch.from_numpy(e * e).to(dev), dev_t(hipbe, given)
    ncount, nrsum = label_lengths(kernel, ref['nbins'])
    outs = [torch.zeros(ncount, dtype=torch.int64, device=dev), torch.zeros(ncount, dtype=torch.float64, device=dev),
            torch.zeros(nrsum, dtype=torch.float64, device=dev)]

    def work():
        for t in outs:
            t.zero_()
        hipbe.pair_counts(LABEL_MODES[kernel], 2, spos, order, cell_of, bt, spos, order, cell_start, bt, grid[0],
                          grid[3], UNIT, e2, subt, *outs)
    work()
    torch.cuda.synchronize()
    want = [cpu(t).copy() for t in outs]
    check_arrays(want, ref, what=kernel)
    T.poison(outs)
    torch.cuda.synchronize()
    assert all(T.poisoned(outs))
    s = side_streams()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        work()
    torch.cuda.synchronize()
    assert all(T.poisoned(outs)), 'a captured zeroing or kernel ran eagerly, or on another stream'
    g.replay()
    torch.cuda.synchronize()
    got = [cpu(t) for t in outs]
    assert numpy.array_equal(got[0], want[0])
    check_arrays(got, ref, what=kernel)


# ---- 10. the ABI and the resources -----------------------------------------------------------------------------------------

def test_the_modes_are_bound():
    assert (_abi.PMX_PAIRS_SPLIT, _abi.PMX_PAIRS_JACKKNIFE, _abi.PMX_PAIRS_LABEL_SLOTS) == (16, 32, 4096)
    assert sorted(LABEL_MODES.values()) == list(range(16, 21)) + list(range(32, 37))
    assert LABEL_MODES['split-projected-midpoint'] == 20 and LABEL_MODES['jackknife-2d'] == 33
    assert [label_slots(n) for n in (1, 40, 1024, 1025)] == [2047, 50, 1, 0]
    for name in ('pair_counts_jackknife', 'pair_correlation_jackknife', 'survey_pair_counts_jackknife',
                 'survey_correlation_jackknife', 'pair_counts_split', 'pair_correlation_split', 'box_regions'):
        assert name in pmesh_amd.__doc__ and callable(getattr(pmesh_amd.pairlabels, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = ' '.join(open(os.path.join(root, 'include', 'pmesh_amd.h')).read().replace('\n *', '\n').split())
    doc = ' '.join(pmesh_amd.pairlabels.__doc__.replace('``', '').split())
    for text in ('all[b] gets (1, w, w sqrt(q)); if a is in range, side[a][b] gets (1, w); if c is in range, side[c][b] '
                 'gets (1, w), so a pair with a == c adds 2 and 2w (w + w, exact); if a == c and in range, same[a][b] '
                 'gets (1, w)', 'kind = (a == c and a is a label) ? 1 : 0', 'npairs[kind * nbins + b] += 1'):
        assert text in header and text in doc, text
    assert 'pmx_pairs_labels.hip' in open(os.path.join(root, 'pmesh_amd', 'csrc', 'Makefile')).read()


def test_labels_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs_labels.hip')
    # labels_kernel<NDIM, BASE, JACK>: the base mode 1d for 1 to 3 dimensions, the four others for 3, in both families
    assert len(t) == 14 and all('labels_kernel' in k for k in t), sorted(t)
    # measured at compile time, split (Lb0E) and jackknife (Lb1E)
    measured = {'ILi1ELi0ELb0E': 36, 'ILi2ELi0ELb0E': 40, 'ILi3ELi0ELb0E': 46, 'ILi3ELi1ELb0E': 46, 'ILi3ELi2ELb0E': 47,
                'ILi3ELi3ELb0E': 50, 'ILi3ELi4ELb0E': 52, 'ILi1ELi0ELb1E': 40, 'ILi2ELi0ELb1E': 46, 'ILi3ELi0ELb1E': 50,
                'ILi3ELi1ELb1E': 52, 'ILi3ELi2ELb1E': 52, 'ILi3ELi3ELb1E': 56, 'ILi3ELi4ELb1E': 58}
    seen = set()
    for name, r in t.items():
        key = [k for k in measured if 'labels_kernel' + k in name]
        assert len(key) == 1, name
        seen.add(key[0])
        assert r['ScratchSize'] == 0, (name, r)
        # 4096 slots of a 32-bit count and a double, the 129 squared edges of r and the 129 of the sub axis: three
        # workgroups in the 160 KB of a CU
        assert r['LDS'] <= 4096 * 12 + 2 * 129 * 8 + 16 <= 53 * 1024, (name, r)
        assert r['VGPRs'] <= measured[key[0]] + 4, (name, r)
    assert len(seen) == 14
