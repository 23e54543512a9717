"""pmesh_amd.threept (csrc/pmx_threept.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/threept.py, include/pmesh_amd.h).  Rows of three columns are wrapped into [0, L_d) by FoF's rule;
dx_d is the minimum image of the wrapped rows; all arithmetic is double; r2 = dx_0^2 + dx_1^2 + dx_2^2 in that order.
With e2[k] = edges[k] * edges[k] row j is a neighbour of i in bin b when e2[b] <= r2 < e2[b + 1]; a pair with r2 == 0 is
never a neighbour.  u = dx / sqrt(r2).  With N_i(b) the neighbours of primary i in bin b (from the secondaries)

    zeta_l[b1, b2] = sum_i w_i sum_{j in N_i(b1)} sum_{k in N_i(b2)} w_j w_k P_l(u_ij . u_ik)      (j == k included)
    diag[b] = sum_i w_i sum_j w_j^2,  wpairs[b] = sum_i w_i sum_j w_j,  npairs[b] = sum_i |N_i(b)|

The restatement is brute force: per primary the matrix of u_ij . u_ik over its neighbours, numpy.polynomial.legendre.
legval of it, binned with the rule's comparisons.  Under -m "not gpu" it serves pmx_threept_multipoles
(ThreeptOracleBackend), so the host layer and the thread ranks run without a GPU; under -m gpu the kernel, which sums
spherical harmonics per primary instead (rule 5), is compared with it.

Tolerances.  npairs is exact everywhere.  zeta_0 is exact wherever the weights are 1; zeta_0, diag and wpairs are exact
where the weights are multiples of 1/8.  Otherwise

    |got - ref| <= (K(b1) + K(b2) + n_nz + 4 C_l) 2^-52 S[b1, b2]
    S[b1, b2] = sum_i |w_i| (sum_{N_i(b1)} |w_j|) (sum_{N_i(b2)} |w_k|)

K(b) the largest |N_i(b)| (the sums A of the two bins), n_nz the number of primaries with a neighbour in both bins
(the sum over the primaries, in any order), and C_l the error of the harmonics themselves: the largest |factorised -
brute force| / (2^-52 S) between two numpy computations (`factorised` below restates rule 5) over the cases of this
file, measured on the CPU and never from the device code; 4 x that is the margin for fused multiply-adds and another
order inside the recurrences.  Measured (test_the_measured_constants_hold recomputes them on the smaller cases):

    l      0     1     2     3     4      5     6     7     8     9     10
    C_l    0.99  1.39  4.5   5.0   30.75  2.4   5.6   29.0  7.2   8.0   12.0     (MEASURED below: rounded up)

(the largest on the weighted ranks case, the crowded cell, centre-2 twice, the lattice — whose zeta_4 is the sum of 512
equal terms —, the 32 narrow bins at l = 7, and the 700 uniform rows for the rest.)

diag and wpairs otherwise: |got - ref| <= (K(b) + n_nz(b) + 4) 2^-52 S: an inner sum of K terms, a product or two, and
the sum over the primaries.

The condition on random inputs: no pair within 1e-9 relative of a squared edge (a contracted multiply-add could
otherwise move a pair).  The wave cases are those of tests/test_paircount.py (its test_inputs_are_decided shows them
decided); test_inputs_are_decided here asserts it for every other random case, without a GPU.
"""
import os

import numpy
import pytest
import torch
from numpy.polynomial import legendre

from pmesh_amd import _abi, backend
from pmesh_amd.fof import cell_grid
from pmesh_amd.paircount import bin_volumes, pair_counts
from pmesh_amd.threept import (MAX_BINS, MAX_ELL, ThreePoint, local_multipoles, threept_correlation,
                               threept_multipoles, triplet_weight)
from tests.test_fof import (GRIDS, RANKS, ROW_FORMS, SLAB, UNIT, WAVE_NS, crowded, face_pairs, lattice, mesh, place,
                            split, thread_ranks, uniform, wrap)
from tests.test_lpt import cpu
from tests.test_paircount import (RANDOM, PairsOracleBackend, count_core, dyadic_weights, grid_of, lattice_rows,
                                  wave_case)

U = 2.0 ** -52
# C_l as measured on the CPU between the two numpy computations, rounded up (the module docstring)
MEASURED = [1, 2, 5, 5, 31, 3, 6, 29, 8, 8, 12]
ALL = tuple(range(MAX_ELL + 1))


# ---- the restatement -----------------------------------------------------------------------------------------------

def neighbours(a, b, box, e2):
    """(dx of the shape (n1, n2, 3), r2, keep, bin) of the wrapped rows a with b"""
    dx = numpy.empty((len(a), len(b), 3))
    for d in range(3):
        x = a[:, None, d] - b[None, :, d]
        dx[:, :, d] = x - box[d] * numpy.rint(x / box[d])
    r2 = dx[:, :, 0] * dx[:, :, 0]
    r2 = r2 + dx[:, :, 1] * dx[:, :, 1]
    r2 = r2 + dx[:, :, 2] * dx[:, :, 2]
    keep = (r2 >= e2[0]) & (r2 < e2[-1]) & (r2 > 0)
    rbin = numpy.searchsorted(e2, r2, side='right') - 1
    return dx, r2, keep, rbin


def harmonics(u, lmax):
    """the (n, (lmax + 1)^2) real components Y of rule 5 at the unit rows u: component l^2 for m = 0, l^2 + 2 m - 1 and
    l^2 + 2 m for the real and imaginary parts of m > 0"""
    n = len(u)
    out = numpy.zeros((n, (lmax + 1) ** 2))
    z = u[:, 2]
    xy = u[:, 0] + 1j * u[:, 1]
    p = numpy.ones(n, dtype=complex)
    for m in range(lmax + 1):
        if m:
            p = p * xy
        qmm = float(numpy.prod(numpy.arange(1.0, 2 * m, 2.0)))
        q2, q1 = None, numpy.full(n, qmm)
        for l in range(m, lmax + 1):
            if l == m + 1:
                q2, q1 = q1, (2 * m + 1) * z * q1
            elif l > m + 1:
                q2, q1 = q1, ((2 * l - 1) * z * q1 - (l + m - 1) * q2) / (l - m)
            norm = numpy.sqrt((1.0 if m == 0 else 2.0) / float(numpy.prod(numpy.arange(l - m + 1.0, l + m + 1.0))))
            if m == 0:
                out[:, l * l] = norm * q1 * p.real
            else:
                out[:, l * l + 2 * m - 1] = norm * q1 * p.real
                out[:, l * l + 2 * m] = norm * q1 * p.imag
    return out


def mirrored(m):
    """the lower triangle of m on both sides: zeta is symmetric exactly (b1 >= b2 is summed, b2 > b1 is its copy)"""
    low = numpy.tril(m)
    return low + numpy.tril(m, -1).T


def threept_core(a, b, box, e2, poles, w1=None, w2=None, factorised=False):
    """The sums of the rule over the wrapped rows a (primaries) and b (secondaries).  Returns a dict: zeta {l: (nr, nr)},
    diag, wpairs, npairs, and for the bounds S (nr, nr), Sd, Sw, K (nr,), nnz (nr, nr), counts (n1, nr).  factorised:
    zeta by rule 5 instead of the brute-force Legendre sum."""
    n1, n2, nr = len(a), len(b), len(e2) - 1
    box = numpy.asarray(box, dtype='f8')
    poles = tuple(poles)
    out = dict(zeta={l: numpy.zeros((nr, nr)) for l in poles}, diag=numpy.zeros(nr), wpairs=numpy.zeros(nr),
               npairs=numpy.zeros(nr, dtype='i8'), S=numpy.zeros((nr, nr)), Sd=numpy.zeros(nr), Sw=numpy.zeros(nr),
               K=numpy.zeros(nr), nnz=numpy.zeros((nr, nr)), counts=numpy.zeros((n1, nr), dtype='i8'))
    if n1 == 0 or n2 == 0:
        return out
    w1 = numpy.ones(n1) if w1 is None else numpy.asarray(w1).astype('f8').reshape(-1)
    w2 = numpy.ones(n2) if w2 is None else numpy.asarray(w2).astype('f8').reshape(-1)
    dx, r2, keep, rbin = neighbours(a, b, box, e2)
    lmax = max(poles)
    for i in range(n1):
        k = numpy.nonzero(keep[i])[0]
        if len(k) == 0:
            continue
        u = dx[i, k] / numpy.sqrt(r2[i, k])[:, None]
        onehot = numpy.zeros((len(k), nr))
        onehot[numpy.arange(len(k)), rbin[i, k]] = 1.0
        bw = onehot * w2[k][:, None]
        cnt = onehot.sum(axis=0)
        sw = bw.sum(axis=0)
        sa = numpy.abs(bw).sum(axis=0)
        out['counts'][i] = cnt
        out['npairs'] += cnt.astype('i8')
        out['wpairs'] += w1[i] * sw
        out['diag'] += w1[i] * (bw * bw).sum(axis=0)
        out['S'] += abs(w1[i]) * sa[:, None] * sa[None, :]
        out['Sw'] += abs(w1[i]) * sa
        out['Sd'] += abs(w1[i]) * (bw * bw).sum(axis=0)
        out['K'] = numpy.maximum(out['K'], cnt)
        out['nnz'] += (cnt[:, None] > 0) & (cnt[None, :] > 0)
        if factorised:
            A = bw.T.dot(harmonics(u, lmax))                    # (nr, ncomp)
            for l in poles:
                c = slice(l * l, (l + 1) * (l + 1))
                out['zeta'][l] += w1[i] * mirrored(A[:, c].dot(A[:, c].T))
        else:
            cosine = u.dot(u.T)
            for l in poles:
                P = legendre.legval(cosine, [0.0] * l + [1.0])
                out['zeta'][l] += w1[i] * mirrored(bw.T.dot(P).dot(bw))
    return out


def ref_threept(pos, box, edges, poles=(0, 1, 2), pos2=None, w=None, w2=None, factorised=False):
    """the restatement of threept_multipoles(mesh(box), pos, edges, poles, pos2, w, w2)"""
    e = numpy.asarray(edges, dtype='f8')
    a = wrap(pos, box)
    auto = pos2 is None
    return threept_core(a, a if auto else wrap(pos2, box), box, e * e, poles, w, w if auto else w2, factorised)


class ThreeptOracleBackend(PairsOracleBackend):
    """the CPU test double with pmx_threept_multipoles served by the restatement"""
    name = 'oracle-threept'

    def threept_multipoles(self, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                           periodic, boxsize, e2, lmax, zeta, diag, wpairs, npairs):
        n1, n2 = spos1.shape[0], spos2.shape[0]
        if n1 == 0 or n2 == 0:
            return
        assert spos1.shape[1] == 3 and tuple(zeta.shape) == (lmax + 1, e2.numel() - 1, e2.numel() - 1)
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        a, b = numpy.empty((n1, 3)), numpy.empty((n2, 3))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = threept_core(a, b, boxsize, e2.numpy(), range(lmax + 1), None if weight1 is None else weight1.numpy(),
                           None if weight2 is None else weight2.numpy())
        zeta += torch.from_numpy(numpy.stack([got['zeta'][l] for l in range(lmax + 1)]))
        diag += torch.from_numpy(got['diag'])
        wpairs += torch.from_numpy(got['wpairs'])
        npairs += torch.from_numpy(got['npairs'])


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(ThreeptOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def pbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(ThreeptOracleBackend())
    yield b
    backend.reset()


@pytest.fixture
def hipbe():
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


def check(tp, ref, poles=None, unit=False, dyadic=False, what=''):
    """a ThreePoint (or the four arrays and the poles) against the restatement's dict"""
    if isinstance(tp, ThreePoint):
        got, poles = (tp.zeta, tp.diag, tp.wpairs, tp.npairs), tp.poles
    else:
        got = tp
    zeta, diag, wpairs, npairs = [(x if isinstance(x, numpy.ndarray) else cpu(x)) for x in got]
    nr = len(ref['npairs'])
    assert npairs.dtype == numpy.int64 and zeta.dtype == diag.dtype == wpairs.dtype == numpy.float64
    assert zeta.shape == (len(poles), nr, nr) and diag.shape == wpairs.shape == npairs.shape == (nr,)
    assert numpy.array_equal(npairs, ref['npairs']), (what, npairs, ref['npairs'])
    K = ref['K'][:, None] + ref['K'][None, :] + ref['nnz']
    nnz = numpy.diag(ref['nnz'])
    for n, l in enumerate(poles):
        assert numpy.array_equal(zeta[n], zeta[n].T), (what, l)
        want = ref['zeta'][l]
        d = numpy.abs(zeta[n] - want)
        if l == 0 and (unit or dyadic):
            assert numpy.array_equal(zeta[n], want), (what, d.max())
        else:
            bound = (K + 4 * MEASURED[l]) * U * ref['S']
            assert (d <= bound).all(), (what, l, (d / numpy.maximum(U * ref['S'], 1e-300)).max(), K.max())
    if unit or dyadic:
        assert numpy.array_equal(diag, ref['diag']) and numpy.array_equal(wpairs, ref['wpairs']), what
    else:
        assert (numpy.abs(diag - ref['diag']) <= (ref['K'] + nnz + 4) * U * ref['Sd']).all(), what
        assert (numpy.abs(wpairs - ref['wpairs']) <= (ref['K'] + nnz + 4) * U * ref['Sw']).all(), what
    if unit:
        assert numpy.array_equal(diag, npairs.astype('f8')) and numpy.array_equal(wpairs, npairs.astype('f8'))


# ---- the inputs ----------------------------------------------------------------------------------------------------

CENTRE_KS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
CENTRE_EDGES = [0.05, 0.1, 0.15, 0.2]


def centre_case(K):
    """a row at the centre of K rows at random directions, their radii inside the bins"""
    rng = numpy.random.RandomState(900 + K)
    v = rng.normal(size=(K, 3))
    v *= (rng.uniform(0.051, 0.199, size=K) / numpy.sqrt((v * v).sum(axis=1)))[:, None]
    return numpy.concatenate([[[0.5, 0.5, 0.5]], 0.5 + v])


def own_cases():
    """name -> keyword arguments of ref_threept: the random inputs of this file that are not test_paircount's"""
    cases = {}
    for K in CENTRE_KS:
        cases['centre-%d' % K] = dict(pos=centre_case(K), box=UNIT, edges=CENTRE_EDGES, poles=(0, 1, 2, 3, 4))
        if K in (31, 32, 33, 65, 129):
            cases['centre-%d-high' % K] = dict(pos=centre_case(K), box=UNIT, edges=CENTRE_EDGES, poles=(0, 5, 10))
    cases['bins-32'] = dict(pos=uniform(700, 3, 31), box=UNIT, edges=numpy.linspace(0.0, 0.16, 33), poles=(0, 1, 2))
    cases['bins-32-high'] = dict(cases['bins-32'], poles=(0, 7))
    return cases


def shared_case(name, poles=(0, 1, 2)):
    """a 3-d '1d' case of test_paircount.RANDOM as keyword arguments of ref_threept"""
    kw = RANDOM[name]
    assert kw.get('mode', '1d') == '1d' and len(kw['box']) == 3 and len(kw['edges']) - 1 <= MAX_BINS
    return dict(pos=kw['pos1'], box=kw['box'], edges=kw['edges'], poles=poles, pos2=kw.get('pos2'), w=kw.get('w1'),
                w2=kw.get('w2'))


def all_cases():
    cases = own_cases()
    cases['crowded'] = shared_case('crowded')
    cases['faces'] = shared_case('faces-3d')
    cases['nonuniform'] = shared_case('nonuniform', (0, 1, 2, 3))
    cases['one-bin'] = shared_case('one-bin', (0, 2, 9))
    cases['uniform'] = shared_case('uniform', ALL)
    cases['weights-uniform'] = shared_case('weights-uniform', (0, 1, 2, 3, 4))
    cases['weights-auto'] = shared_case('weights-auto', (0, 2, 6))
    cases['xi'] = shared_case('xi')
    cases['ranks'] = shared_case('ranks')
    cases['ranks-auto'] = shared_case('ranks-auto', (0, 3, 5))
    return cases


CASES = all_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_threept(**CASES[name])
    return _REFERENCE[name]


def wave_reference(n1, n2, dtype):
    key = ('wave', n1, n2, dtype)
    if key not in _REFERENCE:
        p1, p2, e = wave_case(n1, n2, dtype)
        _REFERENCE[key] = ref_threept(p1, UNIT, e, pos2=p2)
        _REFERENCE[key + ('auto',)] = ref_threept(p1, UNIT, e) if n1 == n2 else None
    return _REFERENCE[key], _REFERENCE[key + ('auto',)]


def run_case(be, name, **over):
    kw = dict(CASES[name], **over)
    dev = be.device
    t = lambda x: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)
    return threept_multipoles(mesh(kw['box']), t(kw['pos']), kw['edges'], kw['poles'], pos2=t(kw.get('pos2')),
                              weight=t(kw.get('w')), weight2=t(kw.get('w2')))


def is_unit(name):
    return CASES[name].get('w') is None and CASES[name].get('w2') is None


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

LATTICE_EDGES = [0.1, 0.15, 0.2, 0.23]


def test_restatement_on_known_answers():
    """the 8^3 lattice: shells of 6, 12 and 8 neighbours at 1/8, sqrt(2)/8 and sqrt(3)/8; the pairs at exactly 2/8 are
    outside the last edge.  zeta_0 = 512 n(b1) n(b2); the odd multipoles and l = 2 vanish by the cube's symmetry"""
    ref = ref_threept(lattice(3), UNIT, LATTICE_EDGES, poles=range(7))
    n = numpy.array([6.0, 12.0, 8.0])
    assert ref['npairs'].tolist() == [512 * 6, 512 * 12, 512 * 8]
    assert numpy.array_equal(ref['zeta'][0], 512 * n[:, None] * n[None, :])
    for l in (1, 2, 3, 5):
        assert (numpy.abs(ref['zeta'][l]) <= 64 * U * ref['S']).all()
    want4 = 512 * numpy.array([[21, -10.5, -56 / 3.], [-10.5, 5.25, 28 / 3.], [-56 / 3., 28 / 3., 448 / 27.]])
    assert (numpy.abs(ref['zeta'][4] - want4) <= 64 * U * ref['S']).all()
    assert abs(ref['zeta'][6][0, 0] - 512 * 4.5) <= 64 * U * ref['S'][0, 0]
    assert numpy.array_equal(ref['diag'], ref['npairs'].astype('f8'))
    # and two rows: a primary with one neighbour has zeta_l = 1 for every l (P_l(1) = 1; u . u is 1 to a few ulps and
    # P_l'(1) = l (l + 1) / 2)
    two = ref_threept(numpy.array([[0.1, 0.1, 0.1], [0.13, 0.14, 0.22]]), UNIT, [0.0, 0.2], poles=ALL)
    for l in ALL:
        assert abs(two['zeta'][l][0, 0] - 2.0) <= 4 * (l * (l + 1) + 4) * U
    f = ref_threept(numpy.array([[0.1, 0.1, 0.1], [0.13, 0.14, 0.22]]), UNIT, [0.0, 0.2], poles=ALL, factorised=True)
    for l in ALL:
        assert abs(f['zeta'][l][0, 0] - 2.0) <= 4 * (l * (l + 1) + 4) * U


def test_inputs_are_decided():
    names = [n for n in sorted(CASES) if n.startswith('centre') or n.startswith('bins-32')]
    assert len(names) >= 15
    for name in names:
        kw = CASES[name]
        e = numpy.asarray(kw['edges'], dtype='f8')
        w = wrap(kw['pos'], kw['box'])
        got = count_core(w, w, numpy.asarray(kw['box']), '1d', 2, e * e, None, skip_diagonal=True)
        assert got['margin'] >= 1e-9, (name, got['margin'])
        assert numpy.array_equal(got['npairs'][1:], reference(name)['npairs'][1:])
        assert 2 * e[-1] <= min(kw['box'])
    for K in CENTRE_KS:
        assert reference('centre-%d' % K)['counts'][0].sum() == K      # every row is a neighbour of the centre
    assert (reference('bins-32')['npairs'] > 0).sum() >= 30


SMALL = ['centre-2', 'centre-33', 'centre-65-high', 'centre-129', 'bins-32-high', 'nonuniform', 'one-bin', 'uniform',
         'weights-uniform', 'weights-auto', 'ranks-auto', 'faces']


def test_the_measured_constants_hold():
    """C_l: |factorised - brute force| <= MEASURED[l] 2^-52 S between the two numpy computations, and the lattice"""
    worst = numpy.zeros(MAX_ELL + 1)
    runs = [(CASES[name], reference(name)) for name in SMALL]
    lat = dict(pos=lattice(3), box=UNIT, edges=LATTICE_EDGES, poles=ALL)
    runs.append((lat, ref_threept(**lat)))
    for kw, ref in runs:
        f = ref_threept(factorised=True, **kw)
        assert numpy.array_equal(f['npairs'], ref['npairs'])
        for l in kw['poles']:
            ok = ref['S'] > 0
            assert numpy.array_equal(f['zeta'][l][~ok], ref['zeta'][l][~ok])
            if ok.any():
                worst[l] = max(worst[l], (numpy.abs(f['zeta'][l] - ref['zeta'][l])[ok] / (U * ref['S'][ok])).max())
    assert (worst <= numpy.array(MEASURED)).all(), worst


# ---- 2. known answers and the kernel's paths -----------------------------------------------------------------------------

def test_known_answer(pbe):
    """the 8^3 lattice with edges [0.1, 0.15, 0.2, 0.23]: zeta_0 = 512 [[36, 72, 48], [72, 144, 96], [48, 96, 64]]
    exactly; zeta_1 = zeta_2 = zeta_3 = zeta_5 = 0, zeta_4 = 512 [[21, -10.5, -56/3], [., 5.25, 28/3], [., ., 448/27]]
    and zeta_6[0, 0] = 512 * 4.5 within the bound"""
    pos = torch.from_numpy(lattice(3)).to(pbe.device)
    tp = threept_multipoles(mesh(UNIT), pos, LATTICE_EDGES, poles=range(7))
    assert isinstance(tp, ThreePoint) and tp.auto and tp.poles == tuple(range(7)) and tp.npairs.dtype == torch.int64
    assert (tp.W1, tp.W2, tp.W2sq, tp.W3) == (512.0,) * 4 and tp.BoxSize == UNIT
    ref = ref_threept(lattice(3), UNIT, LATTICE_EDGES, poles=range(7))
    check(tp, ref, unit=True)
    z = cpu(tp.zeta)
    assert z[0].tolist() == (512 * numpy.array([[36, 72, 48], [72, 144, 96], [48, 96, 64.]])).tolist()
    K = 2 * 12 + 512
    for l in (1, 2, 3, 5):
        assert (numpy.abs(z[l]) <= (K + 4 * MEASURED[l]) * U * ref['S']).all(), l
    want4 = 512 * numpy.array([[21, -10.5, -56 / 3.], [-10.5, 5.25, 28 / 3.], [-56 / 3., 28 / 3., 448 / 27.]])
    assert (numpy.abs(z[4] - want4) <= (K + 4 * MEASURED[4] + 2) * U * ref['S']).all()
    assert abs(z[6][0, 0] - 512 * 4.5) <= (K + 4 * MEASURED[6] + 2) * U * ref['S'][0, 0]
    assert cpu(tp.npairs).tolist() == [3072, 6144, 4096] and cpu(tp.diag).tolist() == [3072.0, 6144.0, 4096.0]


@pytest.mark.parametrize('K', CENTRE_KS)
def test_chunk_edges(pbe, K):
    """a row at the centre of K rows, auto: 0, 1, 2 neighbours and every count around the chunks of 32 and 64 entries
    and around one stride of 256 slots, in the low class of multipoles and (for some K) the high one"""
    check(run_case(pbe, 'centre-%d' % K), reference('centre-%d' % K), unit=True, what=K)
    if 'centre-%d-high' % K in CASES:
        check(run_case(pbe, 'centre-%d-high' % K), reference('centre-%d-high' % K), unit=True, what=K)


@pytest.mark.parametrize('form', ROW_FORMS)
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_wave_and_workgroup_edges(pbe, dtype, form):
    """n1 and n2 independently from 0, 1, 2, 63, 64, 65, 257 and 1025 uniform rows, float64 and float32, contiguous,
    strided and transposed rows, cross and auto; dyadic weights on either side where n1 == n2"""
    pm = mesh(UNIT)
    for n1 in WAVE_NS:
        for n2 in WAVE_NS:
            p1, p2, e = wave_case(n1, n2, dtype)
            cross, auto = wave_reference(n1, n2, dtype)
            t1, t2 = place(p1, form, pbe.device), place(p2, form, pbe.device)
            before = cpu(t1).copy()
            check(threept_multipoles(pm, t1, e, pos2=t2), cross, unit=True, what=(n1, n2))
            assert numpy.array_equal(cpu(t1), before)
            if n1 == n2:
                check(threept_multipoles(pm, t1, e), auto, unit=True, what=(n1, 'auto'))
                if form == 'C' and n1 in (65, 257):
                    w = dyadic_weights(n1, 70 + n1)
                    wt = torch.from_numpy(w.astype(dtype)).to(pbe.device)
                    check(threept_multipoles(pm, t1, e, pos2=t2, weight=wt), ref_threept(p1, UNIT, e, pos2=p2, w=w),
                          dyadic=True, what=(n1, 'w'))
                    check(threept_multipoles(pm, t1, e, pos2=t2, weight2=wt), ref_threept(p1, UNIT, e, pos2=p2, w2=w),
                          dyadic=True, what=(n1, 'w2'))


def test_crowded(pbe):
    """600 rows in one cell: many chunks per primary; two launches give identical npairs and zeta_0"""
    ref = reference('crowded')
    assert ref['npairs'].sum() > 300000 and ref['K'].max() > 200
    a, b = run_case(pbe, 'crowded'), run_case(pbe, 'crowded')
    check(a, ref, unit=True)
    check(b, ref, unit=True)
    assert torch.equal(a.npairs, b.npairs) and torch.equal(a.zeta[0], b.zeta[0])


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: 'x'.join(str(c) for c in g))
def test_grid_edge_shapes(pbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along the periodic axes: no neighbour is visited twice, none is missed"""
    kw = CASES['faces']
    assert all(kw['box'][d] / grid[d] >= kw['edges'][-1] for d in range(3))
    dev = pbe.device
    e = numpy.asarray(kw['edges'], dtype='f8')
    got = local_multipoles(pbe, torch.from_numpy(kw['pos']).to(dev), None, None, None, grid_of(grid, kw['box']),
                           kw['box'], torch.from_numpy(e * e).to(dev), 2)
    check(got, reference('faces'), poles=(0, 1, 2), unit=True, what=grid)


def test_the_grid_of_the_host_layer(pbe):
    pos = face_pairs(SLAB, 0.05)
    edges = [0.0, 0.02, 0.04, 0.05]
    assert cell_grid(len(pos), 0.05, SLAB)[0] == [6, 3, 1]
    ref = ref_threept(pos, SLAB, edges)
    assert ref['npairs'].sum() == len(pos)
    check(threept_multipoles(mesh(SLAB), pos, edges), ref, unit=True)


@pytest.mark.parametrize('name', ['nonuniform', 'one-bin', 'bins-32', 'bins-32-high', 'uniform', 'weights-uniform',
                                  'weights-auto'])
def test_random_cases(pbe, name):
    """edges[0] > 0 in the cross form; one bin; PMX_THREEPT_MAX_BINS bins in both classes; every multipole 0 .. 10;
    weights on both sides (float32 on one) in the cross and the auto form"""
    tp = run_case(pbe, name)
    kw = CASES[name]
    nr = len(kw['edges']) - 1
    assert tuple(tp.zeta.shape) == (len(kw['poles']), nr, nr) and tp.auto == (kw.get('pos2') is None)
    if name.startswith('bins-32'):
        assert nr == MAX_BINS == 32
    check(tp, reference(name), unit=is_unit(name), what=name)


def test_poles_subset_and_order(pbe):
    """poles=(0,), poles=(4, 1) and poles=range(11) of one input: the same matrices, in the order asked for"""
    full = run_case(pbe, 'uniform')
    ref = reference('uniform')
    assert full.poles == ALL
    one = run_case(pbe, 'uniform', poles=(0,))
    check(one, ref, unit=True)
    assert torch.equal(one.zeta[0], full.zeta[0])
    two = run_case(pbe, 'uniform', poles=(4, 1))
    assert two.poles == (4, 1) and tuple(two.zeta.shape) == (2, 6, 6)
    check(two, ref, unit=True)
    check(run_case(pbe, 'uniform', poles=[10]), ref, unit=True)


def test_weighted_exactly(pbe):
    """weights that are multiples of 1/8 in [1/8, 2]: zeta_0, diag and wpairs exactly, cross and auto, in float64 and
    float32 storage; the other multipoles within the bound"""
    p1, p2 = lattice_rows(900, 3, 53), lattice_rows(800, 3, 54)
    w1, w2 = dyadic_weights(900, 55), dyadic_weights(800, 56)
    pm = mesh(UNIT)
    edges = [0.0, 1 / 32., 1 / 16., 3 / 32., 1 / 8.]
    cross, auto = ref_threept(p1, UNIT, edges, pos2=p2, w=w1, w2=w2), ref_threept(p1, UNIT, edges, w=w1)
    for dtype in ('f8', 'f4'):
        a, b, u, v = p1.astype(dtype), p2.astype(dtype), w1.astype(dtype), w2.astype(dtype)
        check(threept_multipoles(pm, a, edges, pos2=b, weight=u, weight2=v), cross, dyadic=True)
        check(threept_multipoles(pm, a, edges, weight=u), auto, dyadic=True)
    tp = threept_multipoles(pm, p1, edges, pos2=p2, weight2=w2.astype('f4'))
    check(tp, ref_threept(p1, UNIT, edges, pos2=p2, w2=w2), dyadic=True)
    assert (tp.W1, tp.W2, tp.W2sq, tp.W3) == (900.0, w2.sum(), (w2 * w2).sum(), 0.0)


def test_identities(pbe):
    """npairs is that of pair_counts where edges[0] > 0; zeta is symmetric (check); zeta_0 with unit weights is sum_i
    n_i(b1) n_i(b2).  Also with a coincident pair of rows (never neighbours) and rows at exactly an edge, on the
    lattice: 1/8 = edges[0] is inside, 3/8 = edges[-1] outside"""
    pm = mesh(UNIT)
    kw = CASES['nonuniform']
    tp = run_case(pbe, 'nonuniform')
    pc = pair_counts(pm, kw['pos'], kw['edges'], pos2=kw['pos2'])
    assert torch.equal(tp.npairs, pc.npairs)
    n = reference('nonuniform')['counts'].astype('f8')
    assert numpy.array_equal(cpu(tp.zeta[0]), n.T.dot(n))
    pos = numpy.concatenate([lattice(3), lattice(3)[:5], [[1.0, 1.0, 1.0]]])
    edges = [1 / 8., 2 / 8., 3 / 8.]
    tp = threept_multipoles(pm, pos, edges, poles=(0, 2, 4))
    ref = ref_threept(pos, UNIT, edges, poles=(0, 2, 4))
    check(tp, ref, unit=True)
    assert torch.equal(tp.npairs, pair_counts(pm, pos, edges).npairs)
    n = ref['counts'].astype('f8')
    assert numpy.array_equal(cpu(tp.zeta[0]), n.T.dot(n))
    # far from the copies the shells hold 26 and 66 rows; row 0 also sees the copies of rows 1 and 2, not its own two
    assert n[100].tolist() == [26.0, 66.0] and n[0].tolist() == [27.0, 67.0]
    # with edges[0] == 0 the coincident rows are still no neighbours
    tp = threept_multipoles(pm, pos, [0.0, 1 / 16.], poles=(0,))
    assert cpu(tp.npairs).tolist() == [0] and cpu(tp.zeta).tolist() == [[[0.0]]]


def test_threept_correlation(pbe):
    """zeta_hat = (2 l + 1) (zeta - [b1 == b2] diag) / RRR - [l == 0], RRR = T V_b1 V_b2 / V_box^2, formed here from
    the restatement's sums; normalized(); T of the auto and the cross form"""
    kw = CASES['xi']
    edges = numpy.asarray(kw['edges'])
    ref = reference('xi')
    zh, tp = threept_correlation(mesh(UNIT), kw['pos'], edges)
    check(tp, ref, unit=True)
    n = 2000.0
    assert triplet_weight(tp) == n ** 3 - 3 * n * n + 2 * n == n * (n - 1) * (n - 2)
    v = 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    rrr = n * (n - 1) * (n - 2) * v[:, None] * v[None, :]
    assert numpy.allclose(bin_volumes(edges, 3), v, rtol=1e-15)
    K = ref['K'][:, None] + ref['K'][None, :] + ref['nnz']
    for k, l in enumerate(tp.poles):
        want = (2 * l + 1) * (ref['zeta'][l] - numpy.diag(ref['diag'])) / rrr - (l == 0)
        bound = (2 * l + 1) * (K + 4 * MEASURED[l] + 8) * U * ref['S'] / rrr + 8 * U * (numpy.abs(want) + 2)
        assert (numpy.abs(cpu(zh[k]) - want) <= bound).all(), l
        f = (2 * l + 1) / (4 * numpy.pi) ** 2
        assert numpy.allclose(cpu(tp.normalized()[k]), f * cpu(tp.zeta[k]), rtol=4 * U, atol=0)
    assert zh.dtype == torch.float64 and tuple(zh.shape) == (3, 5, 5)
    assert (numpy.abs(cpu(zh[0])[2:, 2:]) < 0.5).all()          # uniform rows: no clustering beyond the shot noise
    # the cross form with weights: T = W1 (W2^2 - W2sq)
    kw = CASES['weights-uniform']
    zh, tp = threept_correlation(mesh(UNIT), kw['pos'], kw['edges'], (0, 2), kw['pos2'], kw['w'], kw['w2'])
    w1, w2 = kw['w'], kw['w2'].astype('f8')
    T = w1.sum() * (w2.sum() ** 2 - (w2 * w2).sum())
    assert not tp.auto and tp.W3 == 0.0 and abs(triplet_weight(tp) - T) <= 2000 * U * T
    e = numpy.asarray(kw['edges'])
    v = 4 * numpy.pi / 3 * (e[1:] ** 3 - e[:-1] ** 3)
    rrr = triplet_weight(tp) * v[:, None] * v[None, :]
    want = 5 * (cpu(tp.zeta[1]) - numpy.diag(cpu(tp.diag))) / rrr
    assert numpy.allclose(cpu(zh[1]), want, rtol=16 * U, atol=16 * U)
    # the auto form with weights: T = W1^3 - 3 W1 W2sq + 2 W3 is the sum over distinct triplets
    w = numpy.array([0.5, 2.0, 3.0, 1.25])
    tp = threept_multipoles(mesh(UNIT), uniform(4, 3, 3), [0.0, 0.1], weight=w)
    direct = sum(w[i] * w[j] * w[k] for i in range(4) for j in range(4) for k in range(4) if len({i, j, k}) == 3)
    assert abs(triplet_weight(tp) - direct) <= 64 * U * direct


def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    for edges in ([0.1], [0.2, 0.1], [-0.1, 0.1], [0.0, numpy.nan], [[0.0, 0.1]]):
        with pytest.raises(ValueError, match='edges'):
            threept_multipoles(pm, pos, edges)
    with pytest.raises(ValueError, match='separation'):
        threept_multipoles(pm, pos, [0.0, 0.51])
    with pytest.raises(ValueError, match='bins'):
        threept_multipoles(pm, pos, numpy.linspace(0, 0.2, MAX_BINS + 2))
    assert tuple(threept_multipoles(pm, pos, numpy.linspace(0, 0.2, MAX_BINS + 1), (0,)).zeta.shape) == (1, 32, 32)
    for poles in ((), (0, 0), (11,), (-1,), (0.5,), (1, 2, 1), 3, ('a',)):
        with pytest.raises(ValueError, match='poles'):
            threept_multipoles(pm, pos, [0.0, 0.1], poles=poles)
    with pytest.raises(ValueError, match='shape'):
        threept_multipoles(pm, pos[:, :2], [0.0, 0.1])
    with pytest.raises(TypeError):
        threept_multipoles(pm, (pos * 100).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='weight'):
        threept_multipoles(pm, pos, [0.0, 0.1], weight=numpy.ones(49))
    with pytest.raises(ValueError, match='weight2'):
        threept_multipoles(pm, pos, [0.0, 0.1], weight2=numpy.ones(50))
    with pytest.raises(ValueError, match='weight2'):
        threept_multipoles(pm, pos, [0.0, 0.1], pos2=pos[:40], weight2=numpy.ones(50))
    bad = pos.copy()
    bad[7, 1] = numpy.nan
    bad[9, 0] = numpy.inf
    with pytest.raises(ValueError, match='2 rows'):
        threept_multipoles(pm, bad, [0.0, 0.1])
    with pytest.raises(ValueError, match='3 rows'):
        threept_multipoles(pm, bad, [0.0, 0.1], pos2=bad[5:8])
    for nd in (2, 1):
        with pytest.raises(NotImplementedError):
            threept_multipoles(mesh(UNIT[:nd]), pos[:, :nd], [0.0, 0.1])
    empty = threept_multipoles(pm, numpy.zeros((0, 3)), [0.0, 0.1, 0.2])
    assert cpu(empty.npairs).tolist() == [0, 0] and not cpu(empty.zeta).any() and empty.W1 == 0.0
    assert cpu(threept_multipoles(pm, pos, [0.0, 0.1], pos2=numpy.zeros((0, 3))).npairs).tolist() == [0]


# ---- 3. ranks ------------------------------------------------------------------------------------------------------------

def check_ranks(name, size, np_):
    kw = CASES[name]
    p1, p2, w1, w2 = kw['pos'], kw.get('pos2'), kw.get('w'), kw.get('w2')
    s1 = split(len(p1), size)
    s2 = split(len(p2), size)[::-1] if p2 is not None else None

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a = s1[comm.rank]
        c = s2[comm.rank] if p2 is not None else None
        tp = threept_multipoles(pm, p1[a], kw['edges'], kw['poles'], pos2=None if p2 is None else p2[c],
                                weight=None if w1 is None else w1[a], weight2=None if w2 is None else w2[c])
        return cpu(tp.zeta), cpu(tp.diag), cpu(tp.wpairs), cpu(tp.npairs), (tp.W1, tp.W2, tp.W2sq, tp.W3)
    results = thread_ranks(size, body)
    ref = reference(name)
    for r in range(size):
        check(results[r][:4], ref, poles=kw['poles'], unit=is_unit(name), what=(name, size, r))
        for k in range(5):
            assert numpy.array_equal(results[r][k], results[0][k])      # identical on every rank
    W = results[0][4]
    if w1 is None:
        assert W == (float(len(p1)),) * 4
    else:
        assert abs(W[0] - w1.sum()) <= len(w1) * U * w1.sum() and W[3] == 0.0


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_sums(obe, size, np_):
    """weighted cross and auto at b = 0.1 over thread ranks holding the rows split unevenly (one rank holds none): the
    arrays of every rank are identical and equal the restatement of all rows"""
    for name in ('ranks', 'ranks-auto'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
def test_ranks_on_the_device(hipbe):
    size, np_ = RANKS[-1]
    for name in ('ranks', 'ranks-auto'):
        check_ranks(name, size, np_)


def test_ranks_raise_together(obe):
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        edges = [0.0, 0.05]
        with pytest.raises(ValueError):
            threept_multipoles(pm, mine[:, :2] if comm.rank == 1 else mine, edges)
        with pytest.raises(TypeError):
            threept_multipoles(pm, (mine * 8).astype('i8') if comm.rank == 2 else mine, edges)
        bad = mine.copy()
        if comm.rank == 0:
            bad[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            threept_multipoles(pm, bad, edges)
        with pytest.raises(ValueError):
            threept_multipoles(pm, mine, edges, poles=(0, 11) if comm.rank == 1 else (0, 1))
        with pytest.raises(ValueError):
            threept_multipoles(pm, mine, numpy.linspace(0, 0.05, MAX_BINS + (2 if comm.rank == 2 else 1)))
        got = threept_multipoles(pm, mine, edges, poles=(0,))
        assert int(cpu(got.npairs)[0]) == int(ref_threept(pos, UNIT, edges, poles=(0,))['npairs'][0])
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 4. the ABI and the resources ----------------------------------------------------------------------------------------

def test_the_entry_is_bound():
    assert 'threept_multipoles' in _abi.DEVICE_ONLY
    assert (_abi.PMX_THREEPT_MAX_ELL, _abi.PMX_THREEPT_MAX_BINS) == (10, 32) == (MAX_ELL, MAX_BINS)
    lib = backend.load_library()
    assert hasattr(lib, 'pmx_threept_multipoles')
    import pmesh_amd
    assert 'threept_multipoles' in pmesh_amd.__doc__ and 'threept_correlation' in pmesh_amd.__doc__


def test_threept_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_threept.hip')
    # threept_kernel<WEIGHTED, LMAX>: without and with weights; the classes of multipoles up to 4 and up to 10
    mirror = [r for k, r in t.items() if 'threept_mirror_kernel' in k]
    assert len(mirror) == 1 and mirror[0]['ScratchSize'] == 0 and mirror[0]['LDS'] == 0 and len(t) == 5, sorted(t)
    t = {k: r for k, r in t.items() if 'threept_kernel' in k}
    assert sorted(k.split('threept_kernel')[1][:12] for k in t) == ['ILb0ELi10EEE', 'ILb0ELi4EEEv', 'ILb1ELi10EEE',
                                                                    'ILb1ELi4EEEv'], sorted(t)
    for name, r in t.items():
        high = 'Li10E' in name
        assert r['ScratchSize'] == 0, (name, r)
        # two workgroups in the 160 KB of a CU at the least
        assert r['LDS'] <= 80 * 1024, (name, r)
        # measured at compile time: 166 (three waves per SIMD) in the low class, 252 (two) in the high one; plus 8
        assert r['VGPRs'] <= (260 if high else 174), (name, r)
    # sharing pair_image and pair_bin through pmx_cells_dev.h left the pair-count and FoF kernels where they were
    pairs = resources('pmx_pairs.hip')
    assert len(pairs) == 20
    for name, r in pairs.items():
        weighted, big = 'Lb1E' in name, 'Li4096E' in name
        assert r['ScratchSize'] == 0 and r['VGPRs'] <= (48 if weighted else 40), (name, r)
        assert r['LDS'] <= ((80 if weighted else 52) if big else (24 if weighted else 16)) * 1024, (name, r)
    link = [r for k, r in resources('pmx_fof.hip').items() if 'link_kernel' in k]
    assert len(link) == 3 and all(r['VGPRs'] <= 48 and r['LDS'] == 0 and r['ScratchSize'] == 0 for r in link)
