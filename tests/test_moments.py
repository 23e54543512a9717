"""pmesh_amd.moments (csrc/pmx_pairs_moments.hip) against a numpy restatement of its rule.

The rule (pmesh_amd/moments.py, include/pmesh_amd.h) is that of the mode 1d of pmesh_amd.profiles with the edges of
every centre scaled by the square of its own scale, E_k = e2[k] * s2_i, and with NS sums per (centre, bin) behind the
count and the mass: m sqrt(q), m s, m s (x) s, the same over q, and with velocities m v, m v^2 and m s x v.

The restatement is brute force over the full (n1, n2) matrix in float64 (moments_core); it also returns, per sum, the
sum of the absolute values of its elementary products, and the smallest relative distance of any q from any scaled
edge.  Under -m "not gpu" it serves the mode 517 of pmx_pair_counts (MomentsOracleBackend; the other modes go to its
parents), so the host layer and the thread ranks run without a GPU; under -m gpu the kernel is compared with it.

npart is compared by exact equality everywhere.  Every double sum is held per (centre, bin, component) within the bound
of tests.test_paircount.check: |got - ref| <= (M + 4) 2^-52 S, M the pairs of that bin of that centre, S the sum of the
absolute values of its elementary products (for the angular momentum the sum of |m s_a v_b| + |m s_b v_a|): a term
carries at most four roundings and the sum M - 1.  On dyadic inputs (rows on the 2^-12 lattice, masses and weights in
eighths, velocities in eighths below 16, scales that are powers of two) every term and partial sum of every sum but rsum
and the reduced tensor is exact in double, and those are compared by equality.  Random inputs keep every pair at least
1e-9 (relative) from every scaled edge (test_inputs_are_decided).
"""
import ctypes as C
import os
import re

import numpy
import pytest
import torch

import pmesh_amd
from pmesh_amd import _abi, backend, moments
from pmesh_amd._cells import cell_grid, cell_sort
from pmesh_amd.alignments import alignment_counts
from pmesh_amd.moments import (MAX_BINS, MOMENTS_MODE, MomentsResult, ShapeResult, ellipticity_from_shapes, halo_shapes,
                               local_moments, moment_sums, radial_moments, tensor_pairs)
from pmesh_amd.paircount import pair_counts
from pmesh_amd.profiles import radial_profiles
from tests.test_alignments import AlignOracleBackend
from tests.test_alignments import CODES as ALIGN_CODES
from tests.test_fof import RANKS, SLAB, UNIT, face_pairs, mesh, split, thread_ranks, uniform, wrap
from tests.test_lpt import cpu
from tests.test_paircount import U, dyadic_weights, grid_of, lattice_rows
from tests.test_profiles import ProfilesOracleBackend, neighbourhood, profile_core

RWAVES = 4               # centres per workgroup of moments_kernel (csrc/pmx_pairs_moments.hip)


# ---- the restatement -----------------------------------------------------------------------------------------------

def moments_core(w1, w2, box, e2, c1, c2):
    """The sums over the pairs of every wrapped row of w1 with the wrapped rows w2 by the rule of pmesh_amd.moments.  c1:
    the (n1, 2) columns (w, s2); c2: the (n2, 1) columns (m) or the (n2, 1 + nd) columns (m, v).  A dict of npairs,
    wnpairs (n1, nr), sums (n1, nr, NS), wabs and abs (the sums of the absolute values of the elementary products, of
    the same shapes) and margin (the smallest relative distance of any q from any scaled edge above 0)"""
    n1, n2, nd = len(w1), len(w2), w1.shape[1]
    nr = len(e2) - 1
    c1, c2 = numpy.asarray(c1).astype('f8'), numpy.asarray(c2).astype('f8')
    assert c1.shape == (n1, 2) and c2.shape in ((n2, 1), (n2, 1 + nd))
    vel = c2.shape[1] > 1
    ns = moment_sums(nd, vel)
    out = dict(npairs=numpy.zeros((n1, nr), dtype='i8'), wnpairs=numpy.zeros((n1, nr)), sums=numpy.zeros((n1, nr, ns)),
               wabs=numpy.zeros((n1, nr)), abs=numpy.zeros((n1, nr, ns)), margin=numpy.inf)
    if n1 == 0 or n2 == 0:
        return out
    dx = []
    for d in range(nd):
        x = w1[:, None, d] - w2[None, :, d]
        dx.append(x - box[d] * numpy.rint(x / box[d]))
    q = numpy.zeros((n1, n2))
    for d in range(nd):
        q = q + dx[d] * dx[d]
    E = e2[None, :] * c1[:, 1][:, None]                          # the scaled edges of every centre: one rounding
    keep = (q >= E[:, :1]) & (q < E[:, -1:])
    rbin = numpy.zeros((n1, n2), dtype='i8')
    margin = numpy.inf
    for k in range(nr + 1):
        Ek = E[:, k][:, None]
        if 1 <= k < nr:
            rbin += q >= Ek
        some = Ek[:, 0] > 0
        if some.any():
            margin = min(margin, float((numpy.abs(q[some] - Ek[some]) / Ek[some]).min()))
    out['margin'] = margin
    flat = (numpy.arange(n1)[:, None] * nr + rbin)[keep]

    def binned(t):
        return numpy.bincount(flat, weights=t[keep], minlength=n1 * nr).reshape(n1, nr)
    out['npairs'] = numpy.bincount(flat, minlength=n1 * nr).astype('i8').reshape(n1, nr)
    m = c1[:, 0][:, None] * c2[:, 0][None, :]
    s = [-x for x in dx]
    out['wnpairs'], out['wabs'] = binned(m), binned(numpy.abs(m))
    safe = numpy.where(q > 0, q, 1.0)

    def terms():
        t = m * numpy.sqrt(q)
        yield t, numpy.abs(t)
        for d in range(nd):
            t = m * s[d]
            yield t, numpy.abs(t)
        for a, b in tensor_pairs(nd):
            t = m * s[a] * s[b]
            yield t, numpy.abs(t)
        for a, b in tensor_pairs(nd):
            t = numpy.where(q > 0, (m * s[a] * s[b]) / safe, 0.0)
            yield t, numpy.abs(t)
        if vel:
            v = [c2[:, 1 + d][None, :] for d in range(nd)]
            v2 = numpy.zeros((1, n2))
            for d in range(nd):
                t = m * v[d]
                v2 = v2 + v[d] * v[d]
                yield t, numpy.abs(t)
            yield m * v2, numpy.abs(m) * v2
            for a, b in (((1, 2), (2, 0), (0, 1)) if nd == 3 else ((0, 1),)):
                yield m * (s[a] * v[b] - s[b] * v[a]), numpy.abs(m * s[a] * v[b]) + numpy.abs(m * s[b] * v[a])
    for k, (t, mag) in enumerate(terms()):
        out['sums'][:, :, k], out['abs'][:, :, k] = binned(t), binned(mag)
    assert k == ns - 1
    return out


def columns(n, nd, first=None, second=None, rest=None):
    """the block (first or 1, second or 1) or (first or 1, rest) of n rows"""
    one = numpy.ones(n)
    cols = [one if first is None else numpy.asarray(first).astype('f8').reshape(-1)]
    if rest is not None:
        cols += list(numpy.asarray(rest).astype('f8').reshape(n, nd).T)
    elif second is not False:
        cols += [one if second is None else numpy.asarray(second).astype('f8').reshape(-1) ** 2]
    return numpy.stack(cols, axis=1)


def ref_moments(centres, pos, box, edges, mass=None, vel=None, weight=None, scale=None):
    """the restatement of radial_moments(mesh(box), centres, pos, edges, mass, vel, weight, scale)"""
    box = numpy.asarray(box, dtype='f8')
    e = numpy.asarray(edges, dtype='f8')
    nd = len(box)
    return moments_core(wrap(centres, box), wrap(pos, box), box, e * e, columns(len(centres), nd, weight, scale),
                        columns(len(pos), nd, mass, False, vel))


def packed(res):
    """a MomentsResult as the triple (npairs, wnpairs, the (nc, nr, NS) array of the kernel), the symmetric tensors
    checked to be symmetric"""
    nd = res.ndim
    parts = [cpu(res.rsum)[..., None], cpu(res.first)]
    for t in (cpu(res.second), cpu(res.reduced)):
        assert t.shape[-2:] == (nd, nd) and numpy.array_equal(t, numpy.swapaxes(t, -1, -2))
        parts.append(numpy.stack([t[..., a, b] for a, b in tensor_pairs(nd)], axis=-1))
    if res.momentum is not None:
        parts += [cpu(res.momentum), cpu(res.kinetic)[..., None], cpu(res.angular)]
    return cpu(res.npart), cpu(res.mass), numpy.concatenate(parts, axis=-1)


def exact_components(nd, ns):
    """the components of the NS sums that are exact on dyadic inputs: all but rsum and the reduced tensor"""
    nt = nd * (nd + 1) // 2
    ok = numpy.ones(ns, dtype=bool)
    ok[0] = False
    ok[1 + nd + nt:1 + nd + 2 * nt] = False
    return ok


def check_moments(got, ref, exact=False, what=''):
    """a MomentsResult (or the triple of arrays of local_moments) against the restatement's dict: npairs exactly, every
    sum within (M + 4) U S; with `exact`, every sum but rsum and the reduced tensor by equality"""
    if isinstance(got, MomentsResult):
        n1, nr = ref['npairs'].shape
        assert got.npart.dtype == torch.int64 and tuple(got.npart.shape) == (n1, nr) == tuple(got.rmean.shape)
        got = packed(got)
    n, w, s = [x if isinstance(x, numpy.ndarray) else cpu(x) for x in got]
    n, w, s = n.reshape(ref['npairs'].shape), w.reshape(ref['npairs'].shape), s.reshape(ref['sums'].shape)
    assert n.dtype == numpy.int64 and w.dtype == s.dtype == numpy.float64
    assert numpy.array_equal(n, ref['npairs']), (what, n.reshape(-1)[:8], ref['npairs'].reshape(-1)[:8])
    M = ref['npairs'].astype('f8')
    assert numpy.isfinite(w).all() and numpy.isfinite(s).all(), what
    dw, ds = numpy.abs(w - ref['wnpairs']), numpy.abs(s - ref['sums'])
    assert (dw <= (M + 4) * U * ref['wabs']).all(), (what, dw.max())
    over = ds > (M[..., None] + 4) * U * ref['abs']
    assert not over.any(), (what, numpy.argwhere(over)[:4], ds[over][:4], ((M[..., None] + 4) * U * ref['abs'])[over][:4])
    if exact:
        ns = ref['sums'].shape[2]
        ok = exact_components({9: 2, 13: 2, 16: 3, 23: 3}[ns], ns)
        assert numpy.array_equal(w, ref['wnpairs']), what
        assert numpy.array_equal(s[..., ok], ref['sums'][..., ok]), (what, numpy.argwhere(s[..., ok] != ref['sums'][..., ok])[:4])


class MomentsOracleBackend(ProfilesOracleBackend):
    """the CPU test double with the mode 517 of pmx_pair_counts served by the restatement; the alignment modes go to
    tests.test_alignments' double, everything else to the parent"""
    name = 'oracle-moments'

    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        args = (mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell, periodic,
                boxsize, e2, sub, npairs, wnpairs, rsum)
        if mode in ALIGN_CODES:
            return AlignOracleBackend.pair_counts(self, *args)
        if mode != MOMENTS_MODE:
            return ProfilesOracleBackend.pair_counts(self, *args)
        n1, n2, nd = spos1.shape[0], spos2.shape[0], spos1.shape[1]
        if n1 == 0 or n2 == 0:
            return
        nr = e2.numel() - 1
        assert sub is None and nd in (2, 3) and 1 <= nr <= MAX_BINS
        assert tuple(weight1.shape) == (n1, 2) and weight2.shape[0] == n2 and weight2.shape[1] in (1, 1 + nd)
        ns = moment_sums(nd, weight2.shape[1] > 1)
        assert npairs.numel() == wnpairs.numel() == n1 * nr and rsum.numel() == n1 * nr * ns
        assert cell_start2.numel() == int(numpy.prod(ncell)) + 1 and int(cell_start2[-1]) == n2
        assert int(cell_of1.max()) < int(numpy.prod(ncell))
        a, b = numpy.empty((n1, nd)), numpy.empty((n2, nd))
        a[order1.numpy()] = spos1.numpy()
        b[order2.numpy()] = spos2.numpy()
        got = moments_core(a, b, numpy.asarray(boxsize, dtype='f8'), e2.numpy(), weight1.numpy(), weight2.numpy())
        npairs += torch.from_numpy(got['npairs']).reshape(npairs.shape)
        wnpairs += torch.from_numpy(got['wnpairs']).reshape(wnpairs.shape)
        rsum += torch.from_numpy(got['sums']).reshape(rsum.shape)


@pytest.fixture
def obe():
    backend.reset()
    b = backend.use(MomentsOracleBackend())
    yield b
    backend.reset()


@pytest.fixture(params=['oracle', pytest.param('hip', marks=pytest.mark.gpu)])
def fbe(request):
    backend.reset()
    if request.param == 'hip':
        b = backend.get()
        assert b.name == 'hip'
    else:
        b = backend.use(MomentsOracleBackend())
    yield b
    if request.param == 'hip':
        torch.cuda.synchronize()
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

def eighths(n, nd, seed):
    """velocities in eighths below 16, of either sign"""
    return numpy.random.RandomState(seed).randint(-127, 128, size=(n, nd)) / 8.0


def normal(n, nd, seed):
    return numpy.random.RandomState(seed).normal(size=(n, nd))


def positive(n, seed):
    return numpy.random.RandomState(seed).uniform(0.5, 1.5, n)


def bins_case(nr, nd=3):
    pos = uniform(2000, nd, 200 + nr)
    return dict(centres=numpy.concatenate([pos[:40], uniform(40, nd, 300 + nr)]), pos=pos, box=UNIT[:nd],
                edges=numpy.linspace(0.0, 0.12, nr + 1), mass=positive(2000, 400 + nr), vel=normal(2000, nd, 500 + nr),
                weight=positive(80, 600 + nr))


def random_cases():
    """name -> keyword arguments of ref_moments: every random input of the tests below"""
    cases = {}
    for nr in (1, 2, 33, 64):
        cases['bins-%d' % nr] = bins_case(nr)
    cases['no-vel'] = dict(bins_case(3), vel=None)
    cases['plain'] = dict(bins_case(4), vel=None, mass=None, weight=None)
    cases['2d'] = dict(bins_case(5, 2), edges=[0.0, 0.03, 0.06, 0.1])
    cases['2d-no-vel'] = dict(bins_case(6, 2), edges=[0.0, 0.03, 0.06, 0.1], vel=None)
    kw = bins_case(7)
    cases['f4'] = dict(kw, centres=kw['centres'].astype('f4'), pos=kw['pos'].astype('f4'), mass=kw['mass'].astype('f4'),
                       vel=kw['vel'].astype('f4'), weight=kw['weight'].astype('f4'))
    cases['edges-above-0'] = dict(bins_case(8), edges=[0.01, 0.015, 0.04, 0.1, 0.11])
    cases['scales'] = dict(bins_case(9), edges=[0.0, 0.01, 0.02, 0.025],
                           scale=2.0 ** numpy.random.RandomState(9).randint(-1, 3, 80))
    for nd in (3, 2):
        rows = numpy.concatenate([face_pairs(SLAB[:nd], 0.05), uniform(300, nd, 61, SLAB[:nd])])
        cases['faces-%dd' % nd] = dict(centres=rows[::2].copy(), pos=rows, box=SLAB[:nd], edges=[0.0, 0.02, 0.04, 0.05],
                                       mass=positive(len(rows), 62), vel=normal(len(rows), nd, 63))
    cases['ranks'] = dict(centres=uniform(300, 3, 44), pos=uniform(700, 3, 45), box=UNIT, edges=[0.0, 0.02, 0.04, 0.05],
                          weight=positive(300, 46), mass=positive(700, 47), vel=normal(700, 3, 48),
                          scale=2.0 ** numpy.random.RandomState(49).randint(-1, 2, 300))
    cases['ranks-slab'] = dict(centres=uniform(200, 3, 50, SLAB), pos=uniform(600, 3, 51, SLAB), box=SLAB,
                               edges=[0.0, 0.04, 0.08, 0.1], mass=positive(600, 52))
    return cases


RANDOM = random_cases()
_REFERENCE = {}


def reference(name):
    """the restatement of a random case, computed once"""
    if name not in _REFERENCE:
        _REFERENCE[name] = ref_moments(**RANDOM[name])
    return _REFERENCE[name]


def run(be, kw, **over):
    """radial_moments of the keyword arguments of ref_moments on one rank"""
    kw = dict(kw, **over)
    t = lambda x: None if x is None else torch.from_numpy(numpy.ascontiguousarray(x)).to(be.device)
    return radial_moments(mesh(kw['box']), t(kw['centres']), t(kw['pos']), kw['edges'], mass=t(kw.get('mass')),
                          vel=t(kw.get('vel')), weight=t(kw.get('weight')), scale=t(kw.get('scale')))


def dyadic_case(nd, seed, nc=60, n=1500, scale=True):
    """rows on the 2^-12 lattice crowded into a box of side 1/4 about the middle, masses and weights in eighths,
    velocities in eighths below 16, scales 1/2 .. 4, dyadic edges out to 3/128 (times 4: 3/32)"""
    pos = 0.5 + (lattice_rows(n, nd, seed) - 0.5) * 0.25
    centres = numpy.concatenate([pos[:nc // 2], 0.5 + (lattice_rows(nc - nc // 2, nd, seed + 1) - 0.5) * 0.25])
    kw = dict(centres=centres, pos=pos, box=UNIT[:nd], edges=numpy.array([0.0, 1 / 128., 1 / 64., 3 / 128.]),
              mass=dyadic_weights(n, seed + 2), vel=eighths(n, nd, seed + 3), weight=dyadic_weights(nc, seed + 4))
    if scale:
        kw['scale'] = 2.0 ** numpy.random.RandomState(seed + 5).randint(-1, 3, nc)
    return kw


# ---- 1. the restatement and the inputs (no GPU) ------------------------------------------------------------------------

def test_restatement_with_unit_scales_is_profile_core():
    """with s2 == 1 the decisions and the first two sums are those of tests.test_profiles.profile_core, to the bit; the
    tensors are symmetric sums of the vectors: their traces give back m q and m"""
    for name in ('bins-2', '2d', 'edges-above-0'):
        kw = RANDOM[name]
        box = numpy.asarray(kw['box'], dtype='f8')
        e = numpy.asarray(kw['edges'], dtype='f8')
        ref = reference(name)
        old = profile_core(wrap(kw['centres'], box), wrap(kw['pos'], box), box, '1d', 2, e * e, None, kw['weight'],
                           kw['mass'])
        assert numpy.array_equal(ref['npairs'], old['npairs']) and ref['npairs'].sum() > 300
        assert numpy.array_equal(ref['wnpairs'], old['wnpairs']) and numpy.array_equal(ref['sums'][..., 0], old['rsum'])
        nd = len(box)
        nt = nd * (nd + 1) // 2
        diag = [k for k, (a, b) in enumerate(tensor_pairs(nd)) if a == b]
        trace = ref['sums'][..., 1 + nd + nt:1 + nd + 2 * nt][..., diag].sum(axis=-1)
        inside = ref['npairs'] > 0
        inside[:40] = False                                     # (those centres are sources: a pair at q == 0 adds no trace)
        assert numpy.allclose(trace[inside], ref['wnpairs'][inside], rtol=1e-12)
        assert ref['sums'].shape[2] == moment_sums(nd, True) == (23 if nd == 3 else 13)


def test_restatement_on_known_answers():
    """the 8^3 lattice about one of its points in units of a scale of 1/8: the point itself in [0, 1), then 6 + 12 + 8
    neighbours in [1, 2); their first moments vanish, their second moments are (2 + 8 + 8) / 64 on the diagonal and 0
    off it; with v = (1, 2, 3) for every source the momentum is 26 v and the angular momentum vanishes"""
    from tests.test_fof import lattice
    pos = lattice(3)
    v = numpy.tile([1.0, 2.0, 3.0], (512, 1))
    ref = ref_moments(pos[[77]], pos, UNIT, [0.0, 1.0, 2.0], vel=v, scale=[1 / 8.])
    assert ref['npairs'].tolist() == [[1, 26]]                 # (pairs at exactly an edge go to the bin above)
    s = ref['sums'][0, 1]
    assert (s[1:4] == 0).all() and s[4:10].tolist() == [18 / 64., 0, 0, 18 / 64., 0, 18 / 64.]
    assert abs(s[10:16].sum() - 26) < 1e-13 and s[16:19].tolist() == [26.0, 52.0, 78.0] and s[19] == 26 * 14.0
    assert (s[20:23] == 0).all() and (ref['sums'][0, 0] == [0] * 16 + [1, 2, 3, 14, 0, 0, 0]).all()
    # a source at s = (1/8, 0, 0) with v = (0, 1, 0): L_z = +1/8; in two dimensions the scalar
    one = ref_moments(numpy.array([[0.5, 0.5, 0.5]]), numpy.array([[0.625, 0.5, 0.5]]), UNIT, [0.0, 0.2],
                      vel=numpy.array([[0.0, 1.0, 0.0]]))
    assert one['sums'][0, 0, 1:4].tolist() == [0.125, 0, 0] and one['sums'][0, 0, 20:23].tolist() == [0, 0, 0.125]
    two = ref_moments(numpy.array([[0.5, 0.5]]), numpy.array([[0.625, 0.5]]), UNIT[:2], [0.0, 0.2],
                      vel=numpy.array([[0.0, 1.0]]))
    assert two['sums'].shape == (1, 1, 13) and two['sums'][0, 0, 12] == 0.125


@pytest.mark.parametrize('name', sorted(RANDOM))
def test_inputs_are_decided(name):
    kw = RANDOM[name]
    ref = reference(name)
    assert ref['margin'] >= 1e-9, (name, ref['margin'])
    b = kw['edges'][-1] * (1.0 if kw.get('scale') is None else max(kw['scale']))
    assert 2 * b <= min(kw['box']) and len(kw['pos']) <= 2000 and len(kw['centres']) <= 400
    assert (ref['npairs'].sum(axis=0) > 0).sum() >= min(ref['npairs'].shape[1], 3), name


def test_dyadic_inputs_are_exact_in_any_order():
    """the claim behind the comparisons by equality: summed in reversed order of the sources, every sum of the dyadic
    case but rsum and the reduced tensor is the same to the bit"""
    for nd in (3, 2):
        kw = dyadic_case(nd, 70 + nd)
        a = ref_moments(**kw)
        back = {k: (v[::-1].copy() if k in ('pos', 'mass', 'vel') else v) for k, v in kw.items()}
        b = ref_moments(**back)
        ok = exact_components(nd, a['sums'].shape[2])
        assert a['npairs'].sum() > 2000 and numpy.array_equal(a['npairs'], b['npairs'])
        assert numpy.array_equal(a['wnpairs'], b['wnpairs'])
        assert numpy.array_equal(a['sums'][..., ok], b['sums'][..., ok])
        assert a['margin'] > 0 and len(set(kw['scale'])) == 4 and max(kw['scale']) / min(kw['scale']) == 8


# ---- 2. the kernel's paths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['bins-1', 'bins-2', 'bins-33', 'bins-64', 'no-vel', 'plain', '2d', '2d-no-vel', 'f4',
                                  'edges-above-0', 'scales', 'faces-3d', 'faces-2d'])
def test_random_cases(fbe, name):
    """1, 2, 33 and 64 bins (16 and 1 copies of the histogram, and the limit); with and without velocities in three and
    two dimensions; no columns at all; float rows and columns; edges[0] > 0; scales 1/2 .. 4 on random rows; rows across
    every face of the box [1, 0.5, 0.25]"""
    res = run(fbe, RANDOM[name])
    kw = RANDOM[name]
    nc, nr, nd = len(kw['centres']), len(kw['edges']) - 1, len(kw['box'])
    assert tuple(res.first.shape) == (nc, nr, nd) and tuple(res.second.shape) == tuple(res.reduced.shape) == (nc, nr, nd, nd)
    if kw.get('vel') is None:
        assert res.momentum is None and res.kinetic is None and res.angular is None
    else:
        assert tuple(res.angular.shape) == (nc, nr, 3 if nd == 3 else 1) and tuple(res.kinetic.shape) == (nc, nr)
    check_moments(res, reference(name), what=name)


@pytest.mark.parametrize('nc', [1, RWAVES, RWAVES + 1, 2 * RWAVES + 1])
def test_wave_and_workgroup_edges(fbe, nc):
    """1, 4, 5 and 9 centres, the first of them far from the others in cell order; 0, 1, 63, 64, 65 and 64 * 5 + 1
    sources in the 27 cells of the first centre: the strides of the wave over the ranges laid end to end"""
    edges = [0.0, 0.03, 0.06, 0.1]
    for m in (0, 1, 63, 64, 65, 64 * 5 + 1):
        centres, pos = neighbourhood(nc, m, 400 + m)
        kw = dict(centres=centres, pos=pos, box=UNIT, edges=edges, mass=positive(len(pos), m), vel=normal(len(pos), 3, m))
        ref = ref_moments(**kw)
        assert ref['margin'] >= 1e-9 and ref['npairs'][0].sum() == m
        res = run(fbe, kw)
        check_moments(res, ref, what=(nc, m))
        assert int(cpu(res.npart)[0].sum()) == m


@pytest.mark.parametrize('nd', [3, 2])
def test_dyadic_rows_are_exact(fbe, nd):
    """rows on the lattice, masses, weights and velocities in eighths, scales 1/2, 1, 2 and 4: every sum but rsum and
    the reduced tensor equals the restatement's to the bit; and the results are linear in the centres' weights"""
    kw = dyadic_case(nd, 70 + nd)
    ref = ref_moments(**kw)
    res = run(fbe, kw)
    check_moments(res, ref, exact=True, what=nd)
    plain = packed(run(fbe, kw, weight=None))
    w = kw['weight']
    ok = exact_components(nd, ref['sums'].shape[2])
    got = packed(res)
    assert numpy.array_equal(got[0], plain[0]) and numpy.array_equal(got[1], plain[1] * w[:, None])
    assert numpy.array_equal(got[2][..., ok], (plain[2] * w[:, None, None])[..., ok])
    assert numpy.allclose(got[2], plain[2] * w[:, None, None], rtol=1e-12, atol=1e-15)
    # float rows and columns are widened exactly: the same numbers as floats give the same bits
    f4 = {k: (v.astype('f4') if k in ('centres', 'pos', 'mass', 'vel', 'weight') else v) for k, v in kw.items()}
    check_moments(run(fbe, f4), ref, exact=True, what=(nd, 'f4'))


def test_the_sign_through_every_face(fbe):
    """the box [1, 0.5, 0.25]; per axis and side one centre 2^-6 inside the face and one source of mass m at centre +
    delta e_d, delta = +-2^-5, wrapped over the face: first_d == m delta exactly, the other components 0, and with v =
    e_(d+1) the angular momentum is m delta e_(d+2)"""
    centres, pos, vel, delta = [], [], [], []
    for d in range(3):
        for sign in (1.0, -1.0):
            k = len(centres)
            c = numpy.array([(2 + k) / 8., (1 + k) / 16., 0.125])
            c[d] = SLAB[d] - 2.0 ** -6 if sign > 0 else 2.0 ** -6
            p = c.copy()
            p[d] += sign * 2.0 ** -5
            centres.append(c)
            pos.append(p % SLAB)
            vel.append(numpy.eye(3)[(d + 1) % 3])
            delta.append(sign * 2.0 ** -5)
    centres, pos, vel = numpy.array(centres), numpy.array(pos), numpy.array(vel)
    assert (numpy.abs(pos - centres).max(axis=1) > 0.2).all()      # every source sits across the box from its centre
    mass = numpy.array([1.0, 2.0, 0.5, 4.0, 0.25, 8.0])
    kw = dict(centres=centres, pos=pos, box=SLAB, edges=[0.0, 0.05], mass=mass, vel=vel)
    ref = ref_moments(**kw)
    assert ref['npairs'].tolist() == [[1]] * 6
    res = run(fbe, kw)
    check_moments(res, ref, exact=True)
    first, ang = cpu(res.first)[:, 0], cpu(res.angular)[:, 0]
    for k in range(6):
        d = k // 2
        want = numpy.zeros(3)
        want[d] = mass[k] * delta[k]
        assert first[k].tolist() == want.tolist(), (k, first[k])
        assert ang[k].tolist() == numpy.roll(want, 2).tolist(), (k, ang[k])
    assert first[0, 0] == +2.0 ** -5 and first[1, 0] == -2.0 ** -4


@pytest.mark.parametrize('grid', [[1, 1, 1], [2, 2, 2], [3, 3, 3], [3, 2, 1]], ids=lambda g: 'x'.join(map(str, g)))
def test_grid_edge_shapes(fbe, grid):
    """pairs across every face, edge and corner of the box [1, 0.5, 0.25] and 300 uniform rows on grids of 1, 2 and 3
    cells along the periodic axes, in three and two dimensions: no pair is visited twice, none is missed"""
    for nd in (3, 2):
        name = 'faces-%dd' % nd
        kw = RANDOM[name]
        assert all(kw['box'][d] / grid[d] >= kw['edges'][-1] for d in range(nd))
        t = lambda x: torch.from_numpy(numpy.ascontiguousarray(x)).to(fbe.device)
        e = numpy.asarray(kw['edges'])
        got = local_moments(fbe, t(kw['centres']), t(kw['pos']), t(columns(len(kw['centres']), nd)),
                            t(columns(len(kw['pos']), nd, kw['mass'], False, kw['vel'])), grid_of(grid, kw['box']),
                            kw['box'], t(e * e))
        check_moments(got, reference(name), what=(name, grid))


def test_coincident_and_empty(fbe):
    """a source that coincides with its centre is counted when edges[0] == 0, with a reduced term of 0: nothing is nan
    or inf; it is not counted when edges[0] > 0; a centre with nothing around it has zeros and rmean nan; no centres,
    no sources"""
    pos = numpy.concatenate([uniform(300, 3, 2) * 0.4, [[0.25, 0.25, 0.25]] * 3])
    centres = numpy.array([[0.25, 0.25, 0.25], [0.8, 0.8, 0.8], [1.25, 0.25, 0.25]])
    kw = dict(centres=centres, pos=pos, box=UNIT, edges=[0.0, 1e-4, 0.05], vel=normal(303, 3, 3))
    ref = ref_moments(**kw)
    assert ref['npairs'][:, 0].tolist() == [3, 0, 3] and ref['npairs'][1].sum() == 0 and ref['npairs'][0, 1] > 0
    res = run(fbe, kw)
    check_moments(res, ref)
    for t in (res.rsum, res.first, res.second, res.reduced, res.momentum, res.kinetic, res.angular):
        assert bool(torch.isfinite(t).all())
    assert cpu(res.reduced)[[0, 2], 0].tolist() == [numpy.zeros((3, 3)).tolist()] * 2
    assert numpy.isnan(cpu(res.rmean)[1]).all() and not numpy.isnan(cpu(res.rmean)[0]).any()
    res = run(fbe, kw, edges=[1e-6, 1e-4, 0.05])
    assert cpu(res.npart)[:, 0].tolist() == [0, 0, 0]
    check_moments(res, ref_moments(**dict(kw, edges=[1e-6, 1e-4, 0.05])))
    none = run(fbe, kw, centres=numpy.zeros((0, 3)))
    assert tuple(none.npart.shape) == (0, 2) and tuple(none.second.shape) == (0, 2, 3, 3)
    none = run(fbe, kw, pos=numpy.zeros((0, 3)), vel=numpy.zeros((0, 3)))
    assert cpu(none.npart).tolist() == [[0, 0]] * 3 and numpy.isnan(cpu(none.rmean)).all()
    assert tuple(none.angular.shape) == (3, 2, 3) and not cpu(none.angular).any()


def test_without_scale_the_counts_are_the_profiles(fbe):
    """scale=None: npart equals radial_profiles(...).npart exactly; mass and rsum agree within the bound; within() is
    the cumulative sum along r"""
    kw = RANDOM['bins-33']
    res = run(fbe, kw)
    t = lambda x: torch.from_numpy(numpy.ascontiguousarray(x)).to(fbe.device)
    prof = radial_profiles(mesh(UNIT), t(kw['centres']), t(kw['pos']), kw['edges'], mass=t(kw['mass']),
                           weight=t(kw['weight']))
    assert torch.equal(res.npart, prof.npart) and int(res.npart.sum()) > 1000
    M = cpu(res.npart).astype('f8')
    ref = reference('bins-33')
    assert (numpy.abs(cpu(res.mass) - cpu(prof.mass)) <= 2 * (M + 4) * U * ref['wabs']).all()
    assert (numpy.abs(cpu(res.rsum) - cpu(prof.rsum)) <= 2 * (M + 4) * U * ref['abs'][..., 0]).all()
    cum = res.within()
    assert torch.equal(cum.npart, torch.cumsum(res.npart, 1)) and torch.equal(cum.second, torch.cumsum(res.second, 1))
    one = res.within(4)
    assert tuple(one.npart.shape) == (80, 1) and torch.equal(one.npart[:, 0], cum.npart[:, 4])
    assert torch.equal(one.angular[:, 0], cum.angular[:, 4]) and one.edges.tolist() == [0.0, kw['edges'][5]]
    with pytest.raises(ValueError):
        res.within(33)


# ---- 3. more secondaries than one launch takes -----------------------------------------------------------------------------

@pytest.mark.gpu
def test_more_secondaries_than_one_launch_accumulates(hipbe):
    """2^23 + 1000 sources and 8 centres: the entry launches once per window of 2^23 slots of the sources and the second
    launch adds to what the first left.  Four of the centres sit in the cell that holds slot 2^23, which is split between
    the two launches.  No brute force at this size: the sums against all sources equal the sums against their two halves
    (each within one launch): npart and mass (unit masses) exactly, the others within the bound of a double sum"""
    n2 = (1 << 23) + 1000
    dev = hipbe.device
    gen = torch.Generator(device=dev).manual_seed(5)
    p2 = torch.rand((n2, 3), generator=gen, device=dev, dtype=torch.float64)
    vel = torch.rand((n2, 3), generator=gen, device=dev, dtype=torch.float32)
    edges = numpy.linspace(0.0, 0.02, 3)
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
    whole = radial_moments(pm, centres, p2, edges, vel=vel)
    half = n2 // 2
    parts = [radial_moments(pm, centres, p2[:half], edges, vel=vel[:half]),
             radial_moments(pm, centres, p2[half:], edges, vel=vel[half:])]
    assert torch.equal(whole.npart, parts[0].npart + parts[1].npart)
    assert torch.equal(whole.mass, parts[0].mass + parts[1].mass)          # (unit masses: sums of integers)
    n = cpu(whole.npart)
    assert n.sum() > 1500 and (n.sum(axis=1) > 100).all()
    a, b, c = packed(whole), packed(parts[0]), packed(parts[1])
    # |s| < 0.02 and |v| < 1: every elementary product is below 1 in absolute value, S <= 2 M
    assert (numpy.abs(a[2] - (b[2] + c[2])) <= 2 * (n[..., None] + 4) * U * 2 * n[..., None]).all()
    want = 8 * n2 * 4 * numpy.pi / 3 * (edges[1:] ** 3 - edges[:-1] ** 3)
    assert (numpy.abs(n.sum(axis=0) - want) < 6 * numpy.sqrt(want)).all()


# ---- 4. the entry --------------------------------------------------------------------------------------------------------

def test_the_mode_is_bound():
    assert (_abi.PMX_PAIRS_MOMENTS, _abi.PMX_PAIRS_MOMENTS_MAX_BINS, MOMENTS_MODE, MAX_BINS) == (512, 64, 517, 64)
    for name in ('radial_moments', 'halo_shapes', 'ellipticity_from_shapes'):
        assert name in pmesh_amd.__doc__ and callable(getattr(moments, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pmesh_amd.h')).read()
    doc = ' '.join(moments.__doc__.replace('``', '').split())
    for text in ('E_k = e2[k] * s2_i', '00, 01, 02, 11, 12, 22', '(m * s_a * s_b) / q',
                 '(s_1 v_2 - s_2 v_1, s_2 v_0 - s_0 v_2, s_0 v_1 - s_1 v_0)'):
        assert text in ' '.join(re.sub(r'\n \*', '\n', header).split()) and text in doc, text
    assert 'pmx_pairs_moments.hip' in open(os.path.join(root, 'pmesh_amd', 'csrc', 'Makefile')).read()
    assert (moment_sums(3, False), moment_sums(3, True), moment_sums(2, False), moment_sums(2, True)) == (16, 23, 9, 13)


def test_the_entry_accepts_the_mode():
    """pmx_pair_counts with no rows returns before it touches the device: PMX_OK in the mode 517 in two and three
    dimensions with up to 64 bins; PMX_EINVAL in 512 alone, 512 | m for every other m below 8, 512 combined with 16, 32
    or 128, in one dimension, with nsub = 2 and with 65 bins"""
    lib = backend.load_library()
    bad = _abi.PMX_EINVAL

    def rc(ndim, mode, nr, nsub=1):
        return lib.pmx_pair_counts(ndim, mode, 2, 0, None, None, None, None, 0, None, None, None, None,
                                   _abi.i64arr([1, 1, 1], 3), 7, _abi.f64arr(UNIT, 3), nr, None, nsub, None, None, None,
                                   None, C.c_void_p(0))
    assert [rc(3, 517, 4), rc(2, 517, 4), rc(3, 517, 64), rc(3, 517, 1)] == [0] * 4
    assert [rc(3, 512 | m, 4) for m in (0, 1, 2, 3, 4, 6, 7)] == [bad] * 7
    assert [rc(3, 517 | f, 4) for f in (16, 32, 128, 8, 64, 256, 1024)] == [bad] * 7
    assert [rc(1, 517, 4), rc(3, 517, 4, 2), rc(3, 517, 65), rc(2, 517, 65), rc(3, -517, 4)] == [bad] * 5


@pytest.mark.gpu
def test_the_entry_refuses_bad_arguments_and_writes_nothing(hipbe):
    """sub != NULL, nsub != 1, weight1 of 1 column, weight2 of 2 columns in three dimensions, a missing block, one
    dimension, the modes 512 and 518 and 65 bins: PMX_EINVAL from the entry itself, and the outputs stay as they were;
    the guards of Backend.pair_counts in front of it"""
    from pmesh_amd.backend import PmxError
    dev = hipbe.device
    pos = torch.from_numpy(uniform(50, 3, 1) * 0.5 + 0.25).to(dev)
    blk = {n: torch.ones((50, n), dtype=torch.float64, device=dev) for n in (1, 2, 3, 4)}
    grid = cell_grid(50, 0.2, UNIT)
    _, cell_of, cell_start, order, spos, _ = cell_sort(hipbe, pos, grid, UNIT)
    e = lambda n: torch.from_numpy(numpy.linspace(0, 0.2, n + 1) ** 2).to(dev)
    outs = [torch.zeros(50 * 65, dtype=torch.int64, device=dev), torch.zeros(50 * 65, dtype=torch.float64, device=dev),
            torch.zeros(50 * 65 * 23, dtype=torch.float64, device=dev)]

    def call(mode, w1, w2, e2, sub=None, nsub=1, ndim=3):
        wv1, wv2 = backend._arrays.vec(w1), backend._arrays.vec(w2)
        hipbe.call('pair_counts', ndim, int(mode), 2, 50, spos.data_ptr(), order.data_ptr(), cell_of.data_ptr(),
                   C.byref(wv1) if w1 is not None else None, 50, spos.data_ptr(), order.data_ptr(),
                   cell_start.data_ptr(), C.byref(wv2) if w2 is not None else None, _abi.i64arr(grid[0], 3),
                   int(grid[3]), _abi.f64arr(UNIT, 3), e2.numel() - 1, e2.data_ptr(), nsub,
                   sub.data_ptr() if sub is not None else None, outs[0].data_ptr(), outs[1].data_ptr(),
                   outs[2].data_ptr(), hipbe.stream())
    sub = torch.tensor([0.0, 0.1, 0.2], dtype=torch.float64, device=dev)
    refused = [dict(mode=517, w1=blk[2], w2=blk[1], e2=e(4), sub=sub), dict(mode=517, w1=blk[2], w2=blk[1], e2=e(4), sub=sub, nsub=2),
               dict(mode=517, w1=blk[2], w2=blk[1], e2=e(4), nsub=2), dict(mode=517, w1=blk[1], w2=blk[1], e2=e(4)),
               dict(mode=517, w1=blk[3], w2=blk[4], e2=e(4)), dict(mode=517, w1=blk[2], w2=blk[2], e2=e(4)),
               dict(mode=517, w1=blk[2], w2=blk[3], e2=e(4)), dict(mode=517, w1=None, w2=blk[1], e2=e(4)),
               dict(mode=517, w1=blk[2], w2=None, e2=e(4)), dict(mode=517, w1=blk[2], w2=blk[1], e2=e(4), ndim=1),
               dict(mode=512, w1=blk[2], w2=blk[1], e2=e(4)), dict(mode=518, w1=blk[2], w2=blk[1], e2=e(4)),
               dict(mode=517, w1=blk[2], w2=blk[4], e2=e(65))]
    for kw in refused:
        with pytest.raises(PmxError) as err:
            call(**kw)
        assert err.value.code == _abi.PMX_EINVAL, kw
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in outs)
    with pytest.raises(PmxError, match='columns'):
        call(517, blk[2], blk[2], e(4))
    with pytest.raises(PmxError, match='BINS'):
        call(517, blk[2], blk[4], e(65))
    call(517, blk[2], blk[4], e(64))
    call(517, blk[2], blk[1], e(1))
    torch.cuda.synchronize()
    assert int(outs[0].sum()) >= 100
    args = (spos, order, cell_of, blk[2], spos, order, cell_start)
    tail = (grid[0], grid[3], UNIT)
    small = [torch.zeros(200, dtype=torch.int64, device=dev), torch.zeros(200, dtype=torch.float64, device=dev)]
    with pytest.raises(ValueError, match='rsum'):
        hipbe.pair_counts(517, 2, *args, blk[4], *tail, e(4), None, *small, torch.zeros(200 * 16, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match='sub'):
        hipbe.pair_counts(517, 2, *args, blk[1], *tail, e(4), sub, *outs)
    with pytest.raises(ValueError, match='bins'):
        hipbe.pair_counts(517, 2, *args, blk[1], *tail, e(65), None, *outs)
    with pytest.raises(ValueError, match='weight1'):
        hipbe.pair_counts(517, 2, spos, order, cell_of, blk[3], spos, order, cell_start, blk[1], *tail, e(4), None, *outs)
    with pytest.raises(ValueError, match='weight2'):
        hipbe.pair_counts(517, 2, *args, blk[2], *tail, e(4), None, *outs)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
def test_float_and_double_blocks_at_the_entry(hipbe, dtype):
    """Backend.pair_counts in the mode 517 with both blocks of columns as doubles and as floats, on dyadic values: a
    float is widened exactly, so both give the restatement's sums to the bit"""
    kw = dyadic_case(3, 90)
    dev = hipbe.device
    t = lambda x, dt='f8': torch.from_numpy(numpy.ascontiguousarray(x).astype(dt)).to(dev)
    e = kw['edges']
    c1 = columns(60, 3, kw['weight'], kw['scale'])
    c2 = columns(1500, 3, kw['mass'], False, kw['vel'])
    ref = moments_core(kw['centres'], kw['pos'], numpy.ones(3), e * e, c1, c2)
    got = local_moments(hipbe, t(kw['centres']), t(kw['pos']), t(c1, dtype), t(c2, dtype), cell_grid(1500, 3 / 32., UNIT),
                        UNIT, t(e * e))
    check_moments(got, ref, exact=True, what=dtype)


def test_bad_arguments(obe):
    pm = mesh(UNIT)
    pos = uniform(50, 3, 1)
    c = pos[:10]
    for edges in ([0.1], [0.2, 0.1], [-0.1, 0.1], [0.0, numpy.nan]):
        with pytest.raises(ValueError, match='edges'):
            radial_moments(pm, c, pos, edges)
    with pytest.raises(ValueError, match='bins'):
        radial_moments(pm, c, pos, numpy.linspace(0, 0.2, MAX_BINS + 2))
    assert tuple(radial_moments(pm, c, pos, numpy.linspace(0, 0.2, MAX_BINS + 1)).npart.shape) == (10, 64)
    with pytest.raises(ValueError, match='separation'):
        radial_moments(pm, c, pos, [0.0, 0.51])
    with pytest.raises(ValueError, match='separation'):
        radial_moments(pm, c, pos, [0.0, 0.3], scale=numpy.full(10, 2.0))
    for bad in (0.0, -1.0, numpy.nan, numpy.inf):
        s = numpy.ones(10)
        s[3] = bad
        with pytest.raises(ValueError, match='scale'):
            radial_moments(pm, c, pos, [0.0, 0.1], scale=s)
    with pytest.raises(ValueError, match='scale'):
        radial_moments(pm, c, pos, [0.0, 0.1], scale=numpy.ones(9))
    with pytest.raises(ValueError, match='shape'):
        radial_moments(pm, c[:, :2], pos, [0.0, 0.1])
    with pytest.raises(ValueError, match='vel'):
        radial_moments(pm, c, pos, [0.0, 0.1], vel=numpy.ones((50, 2)))
    with pytest.raises(ValueError, match='mass'):
        radial_moments(pm, c, pos, [0.0, 0.1], mass=numpy.ones(10))
    with pytest.raises(TypeError):
        radial_moments(pm, c, (pos * 100).astype('i8'), [0.0, 0.1])
    with pytest.raises(ValueError, match='two or three'):
        radial_moments(mesh(UNIT[:1]), c[:, :1], pos[:, :1], [0.0, 0.1])
    nanpos = pos.copy()
    nanpos[7, 1] = numpy.nan
    with pytest.raises(ValueError, match='2 rows'):
        radial_moments(pm, nanpos[5:9], nanpos, [0.0, 0.1])
    v = numpy.ones((50, 3))
    v[4, 0] = numpy.inf
    with pytest.raises(ValueError, match='1 rows'):
        radial_moments(pm, c, pos, [0.0, 0.1], vel=v)
    with pytest.raises(ValueError, match='radius'):
        halo_shapes(pm, c, pos, numpy.ones(9) * 0.1)
    with pytest.raises(ValueError, match='scale'):
        halo_shapes(pm, c, pos, -0.1)
    with pytest.raises(ValueError, match='centre_vel'):
        halo_shapes(pm, c, pos, 0.1, centre_vel=numpy.zeros((10, 3)))


# ---- 5. halo_shapes --------------------------------------------------------------------------------------------------------

def rotation(seed):
    q, r = numpy.linalg.qr(numpy.random.RandomState(seed).normal(size=(3, 3)))
    q = q * numpy.sign(numpy.diag(r))
    return q if numpy.linalg.det(q) > 0 else q[:, ::-1]


def signed(v):
    """unit vectors with their component of largest magnitude positive"""
    v = numpy.asarray(v, dtype='f8')
    k = numpy.abs(v).argmax(axis=-1)
    return v * numpy.sign(numpy.take_along_axis(v, k[..., None], axis=-1))


# the deviation of torch.linalg.eigh on symmetric 3 x 3 tensors from numpy.linalg.eigh of the same tensors, relative
# to the Frobenius norm: measured in test_shapes_of_random_clumps (its docstring), times 8; above 1e-12 is a defect
EIGEN_BOUND = 8 * 9.42e-16
# the same for the unit eigenvectors of tensors whose eigenvalues are 10 % of the largest apart or more
AXIS_BOUND = 8 * 9.99e-16


def test_six_sources_on_the_axes(fbe):
    """six sources of equal mass at centre +- a e_x, +- b e_y, +- c e_z, a > b > c dyadic, radius 2 a: the tensor is
    diag(a^2, b^2, c^2) / 3 exactly, the major axis e_x and the ratios b / a and c / a to the solver's rounding; the same
    six turned by a fixed rotation give the same eigenvalues and the turned axis"""
    a, b, c = 0.125, 0.0625, 0.03125
    centre = numpy.array([[0.5, 0.25, 0.75]])
    arms = numpy.concatenate([numpy.diag([a, b, c]), -numpy.diag([a, b, c])])
    pm = mesh(UNIT)
    sh = halo_shapes(pm, centre, centre + arms, 2 * a)
    assert isinstance(sh, ShapeResult) and cpu(sh.npart).tolist() == [6] and cpu(sh.mass).tolist() == [6.0]
    assert cpu(sh.offset).tolist() == [[0.0, 0.0, 0.0]]
    assert numpy.array_equal(cpu(sh.tensor)[0], numpy.diag([a * a / 3, b * b / 3, c * c / 3]))
    norm = numpy.sqrt(a ** 4 + b ** 4 + c ** 4) / 3
    want = numpy.array([a * a, b * b, c * c]) / 3
    assert (numpy.abs(cpu(sh.eigenvalues)[0] - want) <= EIGEN_BOUND * norm).all()
    assert (numpy.abs(cpu(sh.axes)[0] - numpy.eye(3)) <= AXIS_BOUND).all() and cpu(sh.major).shape == (1, 3)
    # sqrt(l1 / l0): two relative errors of EIGEN_BOUND norm / l, halved by the root, and two roundings
    ratio_bound = lambda l: EIGEN_BOUND * norm * (1 / l + 1 / want[0]) / 2 + 2 * U
    assert abs(cpu(sh.b_over_a)[0] - b / a) <= ratio_bound(want[1]) * b / a
    assert abs(cpu(sh.c_over_a)[0] - c / a) <= ratio_bound(want[2]) * c / a
    T = (a * a - b * b) / (a * a - c * c)
    assert abs(cpu(sh.triaxiality)[0] - T) <= 1e-12
    Q = rotation(4)
    turned = halo_shapes(pm, centre, centre + arms.dot(Q.T), 2 * a)
    assert cpu(turned.npart).tolist() == [6]
    # the tensor itself now carries the roundings of the rows: |s| <= a (1 + U), six terms
    slack = 16 * U * a * a
    assert (numpy.abs(cpu(turned.eigenvalues)[0] - want) <= EIGEN_BOUND * norm + slack).all()
    gap = (b * b - c * c) / 3
    assert (numpy.abs(cpu(turned.axes)[0] - signed(Q.T)) <= AXIS_BOUND + slack / gap).all()
    red = halo_shapes(pm, centre, centre + arms, 2 * a, reduced=True)
    assert numpy.array_equal(cpu(red.tensor)[0], numpy.eye(3) / 3)   # (every term is m / q * s * s = 1 or 0: exact)
    # in two dimensions: four sources, one ratio
    sh2 = halo_shapes(mesh(UNIT[:2]), centre[:, :2], centre[:, :2] + arms[[0, 1, 3, 4], :2], 2 * a)
    assert numpy.array_equal(cpu(sh2.tensor)[0], numpy.diag([a * a / 2, b * b / 2])) and sh2.c_over_a is None
    assert abs(cpu(sh2.b_over_a)[0] - b / a) <= 1e-14 and sh2.spin is None and sh2.triaxiality is None


def test_rigid_rotation(fbe):
    """sixteen sources of mass m on a ring s of radius rho about the z axis of the centre with v = Omega x s + V0: J = 16
    m rho^2 omega e_z, the mean velocity is V0, and sigma = omega rho / sqrt(3); about a second centre the same sixteen
    velocities on a ring of half the radius: half of J.  With and without centre_vel = V0.  Then velocity, sigma, the
    angular momentum and the spin by the formulas of halo_shapes on the device's own sums, and the sums themselves
    against the restatement"""
    rho, omega, m = 0.0625, 3.0, 0.5
    phi = 2 * numpy.pi * numpy.arange(16) / 16
    s = rho * numpy.stack([numpy.cos(phi), numpy.sin(phi), 0 * phi], axis=1)
    V0 = numpy.array([0.25, -0.5, 1.0])
    v = numpy.cross([0.0, 0.0, omega], s) + V0
    centre = numpy.array([[0.5, 0.5, 0.5], [0.2, 0.2, 0.2]])
    pos = numpy.concatenate([centre[0] + s, centre[1] + 0.5 * s])
    vel = numpy.concatenate([v, v])
    mass = numpy.full(32, m)
    pm = mesh(UNIT)
    R = 0.1
    for cv in (None, numpy.tile(V0, (2, 1))):
        sh = halo_shapes(pm, centre, pos, R, mass=mass, vel=vel, centre_vel=cv, G=2.0)
        check_moments(sh.moments, ref_moments(centre, pos, UNIT, [0.0, 1.0], mass=mass, vel=vel, scale=[R, R]))
        assert cpu(sh.npart).tolist() == [16, 16] and cpu(sh.mass).tolist() == [8.0, 8.0]
        scale = numpy.array([1.0, 0.5])
        J = cpu(sh.angular_momentum)
        assert numpy.allclose(J[:, 2], 16 * m * rho * rho * scale * omega, rtol=1e-13)
        assert (numpy.abs(J[:, :2]) <= 1e-15).all()
        want_v = numpy.tile(V0 if cv is None else 0 * V0, (2, 1))
        assert numpy.allclose(cpu(sh.velocity), want_v, rtol=0, atol=1e-14)
        assert numpy.allclose(cpu(sh.sigma), omega * rho / numpy.sqrt(3.0), rtol=1e-12)
        M = 16 * m
        V = numpy.sqrt(2.0 * M / R)
        assert numpy.allclose(cpu(sh.spin), J[:, 2] / (numpy.sqrt(2.0) * M * V * R), rtol=1e-13)
        # the formulas on the device's own sums
        mom = sh.moments
        first, mo, ke, an = cpu(mom.first)[:, 0], cpu(mom.momentum)[:, 0], cpu(mom.kinetic)[:, 0], cpu(mom.angular)[:, 0]
        mean = mo / M
        vref = mean if cv is None else cv
        assert numpy.allclose(J, an - numpy.cross(first, vref), rtol=0, atol=8 * U * numpy.abs(an).max())
        assert numpy.allclose(cpu(sh.sigma), numpy.sqrt(numpy.maximum(ke / M - (mean * mean).sum(axis=1), 0) / 3),
                              rtol=0, atol=64 * U * (ke / M) / cpu(sh.sigma))


def clumps(seed=5, nclump=12, per=160):
    """`nclump` triaxial Gaussian clumps of `per` sources in random orientations about centres 0.2 apart or more, with
    unequal masses: (centres, pos, mass)"""
    rng = numpy.random.RandomState(seed)
    cells = rng.permutation(64)[:nclump]
    centres = (numpy.stack(numpy.unravel_index(cells, (4, 4, 4)), axis=1) + 0.5) / 4.0
    rows = []
    for k in range(nclump):
        sig = numpy.array([0.02, 0.012, 0.007]) * rng.uniform(0.9, 1.1)
        rows.append(centres[k] + (rng.normal(size=(per, 3)) * sig).dot(rotation(seed + k).T))
    return centres + rng.normal(size=centres.shape) * 0.002, numpy.concatenate(rows) % 1.0, rng.uniform(0.5, 1.5, nclump * per)


def ref_tensor(ref):
    """(tensor, its elementwise bound, offset) of halo_shapes' rule on the restatement's sums of one bin.  second / M, M
    and first / M each carry (n + 4) U S of their sum and one rounding of the division, the product of the offsets
    twice that, the subtraction one more: (4 n + 20) U (S2_ab / M + S1_a S1_b / M^2) bounds the difference of two
    evaluations"""
    n, M = ref['npairs'][:, 0].astype('f8'), ref['wnpairs'][:, 0]
    nd = 3
    pairs = tensor_pairs(nd)
    first, S1 = ref['sums'][:, 0, 1:1 + nd] / M[:, None], ref['abs'][:, 0, 1:1 + nd] / M[:, None]
    T, B = numpy.zeros((len(M), nd, nd)), numpy.zeros((len(M), nd, nd))
    for k, (a, b) in enumerate(pairs):
        T[:, a, b] = T[:, b, a] = ref['sums'][:, 0, 1 + nd + k] / M - first[:, a] * first[:, b]
        B[:, a, b] = B[:, b, a] = (4 * n + 20) * U * (ref['abs'][:, 0, 1 + nd + k] / M + S1[:, a] * S1[:, b])
    return T, B, first


def test_shapes_of_random_clumps(fbe):
    """Twelve triaxial clumps in random orientations: tensor against the restatement within ref_tensor's bound;
    eigenvalues and axes against numpy.linalg.eigh of the restatement's tensor within the solver's bound plus the
    perturbation the difference of the two tensors allows (Weyl: its Frobenius norm for the eigenvalues, over the gap for
    the axes).
    The solver's bound.  Measured here, against numpy.linalg.eigh of the device's own tensor copied to the host, relative
    to the Frobenius norm: eigenvalues 5.1e-16 on the CPU double and 9.42e-16 on the MI355X, axes 7.77e-16 and 9.99e-16;
    EIGEN_BOUND and AXIS_BOUND are 8 times the larger.  The figures are printed before they are asserted."""
    centres, pos, mass = clumps()
    radius = numpy.full(len(centres), 0.06)
    sh = halo_shapes(mesh(UNIT), centres, pos, radius, mass=mass)
    ref = ref_moments(centres, pos, UNIT, [0.0, 1.0], mass=mass, scale=radius)
    assert ref['margin'] >= 1e-9 and (ref['npairs'][:, 0] >= 150).all()
    check_moments(sh.moments, ref)
    T, B, first = ref_tensor(ref)
    got = cpu(sh.tensor)
    assert (numpy.abs(got - T) <= B).all(), (numpy.abs(got - T) / B).max()
    assert (numpy.abs(cpu(sh.offset) - first) <= (2 * ref['npairs'][:, :1] + 9) * U * ref['abs'][:, 0, 1:4] / ref['wnpairs'][:, :1]).all()
    norm = numpy.sqrt((T * T).sum(axis=(1, 2)))
    lam, vec = numpy.linalg.eigh(T)
    lam, vec = lam[:, ::-1], signed(numpy.swapaxes(vec[:, :, ::-1], 1, 2))
    gaps = numpy.minimum(lam[:, 0] - lam[:, 1], lam[:, 1] - lam[:, 2])
    assert (gaps >= 0.1 * lam[:, 0]).all(), (gaps / lam[:, 0]).min()      # well separated: the axes are well conditioned
    # the solver alone: the device's tensor through numpy
    lam_d, vec_d = numpy.linalg.eigh(got)
    lam_d, vec_d = lam_d[:, ::-1], signed(numpy.swapaxes(vec_d[:, :, ::-1], 1, 2))
    dev_l = (numpy.abs(cpu(sh.eigenvalues) - lam_d) / norm[:, None]).max()
    dev_v = numpy.abs(cpu(sh.axes) - vec_d).max()
    print('eigh deviation on %s: eigenvalues %.3g of the norm, axes %.3g' % (fbe.name, dev_l, dev_v))
    assert EIGEN_BOUND <= 1e-12 and dev_l <= EIGEN_BOUND and dev_v <= AXIS_BOUND
    # against the restatement
    diff = numpy.sqrt(((got - T) ** 2).sum(axis=(1, 2)))
    assert (numpy.abs(cpu(sh.eigenvalues) - lam) <= (EIGEN_BOUND * norm + diff)[:, None]).all()
    assert (numpy.abs(cpu(sh.axes) - vec) <= (AXIS_BOUND + 2 * diff / gaps)[:, None, None]).all()
    assert numpy.array_equal(cpu(sh.major), cpu(sh.axes)[:, 0]) and (cpu(sh.axes).max(axis=2) == numpy.abs(cpu(sh.axes)).max(axis=2)).all()
    assert numpy.allclose(cpu(sh.b_over_a), numpy.sqrt(lam[:, 1] / lam[:, 0]), rtol=1e-12)
    assert numpy.allclose(cpu(sh.c_over_a), numpy.sqrt(lam[:, 2] / lam[:, 0]), rtol=1e-12)
    assert (cpu(sh.c_over_a) < cpu(sh.b_over_a)).all() and (cpu(sh.b_over_a) < 1).all()
    g = cpu(ellipticity_from_shapes(sh, los=2))
    assert g.shape == (12, 2) and numpy.allclose((g * g).sum(axis=1), 1.0)


def test_centres_without_a_radius_or_sources(fbe):
    """a centre whose radius is nan and a centre with three sources have nan rows; their neighbours are what they are
    without them"""
    centres, pos, mass = clumps(seed=6, nclump=5)
    lonely = numpy.array([[0.01, 0.01, 0.01]])
    few = lonely + numpy.array([[0.001, 0, 0], [0, 0.001, 0], [0, 0, 0.001]])
    c = numpy.concatenate([centres[:2], lonely, centres[2:]])
    p, m = numpy.concatenate([pos, few]), numpy.concatenate([mass, numpy.ones(3)])
    radius = numpy.full(6, 0.06)
    radius[4] = numpy.nan
    pm = mesh(UNIT)
    vel = normal(len(p), 3, 8)
    sh = halo_shapes(pm, c, p, radius, mass=m, vel=vel)
    base = halo_shapes(pm, c[[0, 1, 3, 5]], p, 0.06, mass=m, vel=vel)
    assert cpu(sh.npart)[2] == 3 and numpy.isnan(cpu(sh.radius)[4])
    for name in ('offset', 'tensor', 'eigenvalues', 'axes', 'major', 'b_over_a', 'c_over_a', 'triaxiality', 'velocity',
                 'sigma', 'angular_momentum', 'spin'):
        t, b = cpu(getattr(sh, name)), cpu(getattr(base, name))
        assert numpy.isnan(t[[2, 4]]).all(), name
        assert numpy.isfinite(t[[0, 1, 3, 5]]).all(), name
        assert numpy.allclose(t[[0, 1, 3, 5]], b, rtol=1e-9, atol=1e-12), name
    assert numpy.array_equal(cpu(sh.npart)[[0, 1, 3, 5]], cpu(base.npart))
    # every radius nan: nothing is searched, everything is nan
    none = halo_shapes(pm, c, p, numpy.full(6, numpy.nan), mass=m)
    assert numpy.isnan(cpu(none.tensor)).all() and numpy.isnan(cpu(none.radius)).all()


def test_from_particles_to_alignments(fbe):
    """the chain the module closes: planted clumps -> fof -> fof_catalog -> halo_shapes -> alignment_counts on the major
    axes; its npairs equals that of pair_counts on the same centres; the ellipticities go through
    projected_alignment_counts"""
    from pmesh_amd.alignments import projected_alignment_counts
    from pmesh_amd.fof import fof, fof_catalog
    _, pos, mass = clumps(seed=7, nclump=10)
    pm = mesh(UNIT)
    vel = normal(len(pos), 3, 9)
    cat = fof_catalog(pm, pos, fof(pm, pos, 0.012, nmin=20), mass=mass, vel=vel)
    nh = cat.CMPosition.shape[0] - 1
    assert 8 <= nh <= 14
    sh = halo_shapes(pm, cat.CMPosition, pos, 0.05, mass=mass, vel=vel, centre_vel=cat.CMVelocity)
    major = sh.major[1:]
    assert bool(torch.isfinite(major).all()) and bool(torch.isfinite(sh.spin[1:]).all())
    assert numpy.allclose(cpu((major * major).sum(dim=1)), 1.0, rtol=1e-14)
    edges = numpy.array([0.0, 0.3, 0.45])
    ac = alignment_counts(pm, cat.CMPosition[1:], major, edges)
    pc = pair_counts(pm, cat.CMPosition[1:], edges)
    assert numpy.array_equal(cpu(ac.npairs), cpu(pc.npairs)) and int(cpu(ac.npairs).sum()) > 10
    pa = projected_alignment_counts(pm, cat.CMPosition[1:], ellipticity_from_shapes(sh)[1:], [0.0, 0.2, 0.4],
                                    piedges=[0.0, 0.2])
    assert int(cpu(pa.npairs).sum()) > 0


# ---- 6. ranks --------------------------------------------------------------------------------------------------------------

def ranks_case(name, size, np_):
    """radial_moments on thread ranks holding centres and sources split unevenly (one rank holds none of either): what
    every rank got for its own centres"""
    kw = RANDOM[name]
    c, p = kw['centres'], kw['pos']
    s1, s2 = split(len(c), size), split(len(p), size)[::-1]
    cut = lambda x, s: None if x is None else x[s]

    def body(comm):
        pm = mesh(kw['box'], comm, np_)
        a, b = s1[comm.rank], s2[comm.rank]
        res = radial_moments(pm, c[a], p[b], kw['edges'], mass=cut(kw.get('mass'), b), vel=cut(kw.get('vel'), b),
                             weight=cut(kw.get('weight'), a), scale=cut(kw.get('scale'), a))
        return packed(res) + (len(c[a]), len(p[b]))
    return thread_ranks(size, body), s1


def check_ranks(name, size, np_):
    results, s1 = ranks_case(name, size, np_)
    ref = reference(name)
    assert ref['margin'] >= 1e-9
    assert 0 in [results[r][3] for r in range(size)] and 0 in [results[r][4] for r in range(size)]
    for r in range(size):
        part = {k: ref[k][s1[r]] for k in ('npairs', 'wnpairs', 'sums', 'wabs', 'abs')}
        assert results[r][0].shape[0] == results[r][3]
        if results[r][3]:
            check_moments(results[r][:3], part, what=(name, size, r))


@pytest.mark.parametrize('size,np_', RANKS)
def test_ranks_give_the_one_rank_moments(obe, size, np_):
    """weighted moments with velocities and per-centre scales in the unit box, and ones without velocities on the box [1,
    0.5, 0.25]: every rank gets, for its own centres in its own order, the rows of the restatement of all rows"""
    for name in ('ranks', 'ranks-slab'):
        check_ranks(name, size, np_)


@pytest.mark.gpu
def test_ranks_on_the_device(hipbe):
    size, np_ = RANKS[-1]
    for name in ('ranks', 'ranks-slab'):
        check_ranks(name, size, np_)


def test_ranks_raise_together(obe):
    """bad arguments on one rank raise on every rank: a scale that is not positive or not finite, 2 b > L through one
    rank's scale, a coordinate that is not finite, too many bins"""
    pos = uniform(90, 3, 2)
    raised = []

    def body(comm):
        pm = mesh(UNIT, comm, [3])
        mine = pos[30 * comm.rank:30 * comm.rank + 30]
        c = mine[:5]
        edges = [0.0, 0.05]
        for bad in (0.0, -2.0, numpy.nan, numpy.inf):
            s = numpy.ones(5)
            if comm.rank == 1:
                s[2] = bad
            with pytest.raises(ValueError):
                radial_moments(pm, c, mine, edges, scale=s)
        with pytest.raises(ValueError, match='separation'):
            radial_moments(pm, c, mine, edges, scale=numpy.full(5, 11.0 if comm.rank == 2 else 1.0))
        nan = mine.copy()
        if comm.rank == 0:
            nan[3, 2] = numpy.nan
        with pytest.raises(ValueError, match='1 rows'):
            radial_moments(pm, c, nan, edges)
        with pytest.raises(ValueError):
            radial_moments(pm, c, mine, numpy.linspace(0, 0.05, MAX_BINS + (2 if comm.rank == 2 else 1)))
        with pytest.raises(ValueError):
            halo_shapes(pm, c, mine, -1.0 if comm.rank == 0 else 0.05)
        got = cpu(radial_moments(pm, c, mine, edges, scale=numpy.full(5, 1.0 + comm.rank)).npart)
        want = ref_moments(c, pos, UNIT, edges, scale=numpy.full(5, 1.0 + comm.rank))['npairs']
        assert numpy.array_equal(got, want)
        raised.append(comm.rank)
        return True
    thread_ranks(3, body)
    assert sorted(raised) == [0, 1, 2]


# ---- 7. streams ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('vel', [False, True])
def test_capture_poison_replay(hipbe, vel):
    """Backend.pair_counts in the mode 517 with the inputs sorted and the outputs allocated beforehand, after
    tests/test_streams.py's test_capture_poison_replay: the zeroing and the call captured into a graph on a side stream
    leave the poisoned outputs as they were (nothing ran eagerly or on another stream); the replay gives the eager
    call's npairs and exact sums to the bit and the others within twice the bound"""
    from tests import test_streams as T
    dev = hipbe.device
    kw = dyadic_case(3, 95, nc=200, n=3000)
    e = kw['edges']
    c1 = columns(200, 3, kw['weight'], kw['scale'])
    c2 = columns(3000, 3, kw['mass'], False, kw['vel'] if vel else None)
    ref = moments_core(kw['centres'], kw['pos'], numpy.ones(3), e * e, c1, c2)
    t = lambda x: torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)
    grid = cell_grid(3000, 3 / 32., UNIT)
    _, cell_of1, _, order1, spos1, _ = cell_sort(hipbe, t(kw['centres']), grid, UNIT)
    _, _, cell_start2, order2, spos2, _ = cell_sort(hipbe, t(kw['pos']), grid, UNIT)
    w1, w2, e2 = t(c1), t(c2), t(e * e)
    ns = moment_sums(3, vel)
    outs = [torch.zeros((200, 3), dtype=torch.int64, device=dev), torch.zeros((200, 3), dtype=torch.float64, device=dev),
            torch.zeros((200, 3, ns), dtype=torch.float64, device=dev)]

    def work():
        for x in outs:
            x.zero_()
        hipbe.pair_counts(MOMENTS_MODE, 0, spos1, order1, cell_of1, w1, spos2, order2, cell_start2, w2, grid[0], grid[3],
                          UNIT, e2, None, *outs)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            work()
    s.synchronize()
    want = [cpu(x).copy() for x in outs]
    check_moments(want, ref, exact=True)
    T.poison(outs)
    torch.cuda.synchronize()
    assert all(T.poisoned(outs))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        work()
    torch.cuda.synchronize()
    assert all(T.poisoned(outs)), 'a captured zeroing or kernel ran eagerly, or on another stream'
    g.replay()
    torch.cuda.synchronize()
    got = [cpu(x) for x in outs]
    check_moments(got, ref, exact=True)
    ok = exact_components(3, ns)
    assert numpy.array_equal(got[0], want[0]) and numpy.array_equal(got[1], want[1])
    assert numpy.array_equal(got[2][..., ok], want[2][..., ok])


# ---- 8. the resources ------------------------------------------------------------------------------------------------------

def test_moments_kernels_compile_within_their_budgets():
    from tests.test_kernel_resources import HIPCC, resources
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    t = resources('pmx_pairs_moments.hip')
    # moments_kernel<NDIM, VEL>: two and three dimensions, without and with velocities
    assert len(t) == 4 and all('moments_kernel' in k for k in t), sorted(t)
    for nd in (2, 3):
        for vel in (0, 1):
            name = [k for k in t if 'moments_kernelILi%dELb%dE' % (nd, vel) in k]
            assert len(name) == 1, sorted(t)
            r = t[name[0]]
            assert r['ScratchSize'] == 0, (name, r)
            # per wave: 64 slots of a 32-bit count and 1 + NS doubles, and the 65 scaled edges; two workgroups and more
            # in the 160 KB of a CU
            assert r['LDS'] <= RWAVES * (64 * (4 + 8 * (1 + moment_sums(nd, bool(vel)))) + 65 * 8) <= 65536, (name, r)
