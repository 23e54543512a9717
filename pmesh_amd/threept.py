"""Multipoles of the isotropic three-point correlation function of particles, made on the device.

What nbodykit's ``SimulationBox3PCF`` does on the host (a kd-tree over the rows copied over PCIe) as one entry of the C
ABI (csrc/pmx_threept.hip, include/pmesh_amd.h: pmx_threept_multipoles) behind the cell grid of pmesh_amd.fof: the
Slepian & Eisenstein (2015) spherical-harmonic factorisation, O(N neighbours) instead of O(N neighbours^2), over the
rows of ``lognormal_catalog``, of an N-body run or of ``fof_catalog`` without leaving HBM.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Rows.  ``pos`` and ``pos2`` are ``(n, 3)`` rows, float64 or float32 (widened exactly), wrapped and differenced by
   rules 1-2 of pmesh_amd.paircount: FoF's wrap, then the minimum image of the wrapped rows.  All arithmetic is double.
   ``r2 = dx_0^2 + dx_1^2 + dx_2^2``, summed in that order.  Only meshes of three dimensions are accepted; others raise
   NotImplementedError.
2. Bins.  ``edges`` follows rule 3 of paircount; the host squares the edges once.  Row j is a neighbour of i in bin b
   when ``e2[b] <= r2 < e2[b + 1]``.  A pair with ``r2 == 0`` is never a neighbour (the row itself, a coincident row): it
   has no direction.  The search radius is ``b = edges[-1]`` with ``2 b <= min_d L_d``.  At most PMX_THREEPT_MAX_BINS
   (32) radial bins.
3. Direction.  ``r = sqrt(r2)`` and ``u_d = dx_d / r``.
4. Sums.  With N_i(b) the neighbours of primary i in bin b, taken from the secondaries, for every requested ``l`` in
   0 .. PMX_THREEPT_MAX_ELL (10):

       zeta_l[b1, b2] = sum_i w_i  sum_{j in N_i(b1)} sum_{k in N_i(b2)} w_j w_k P_l(u_ij . u_ik)

   The term j == k (b1 == b2) is included.  So that a caller can remove it: ``diag[b] = sum_i w_i sum_{j in N_i(b)}
   w_j^2`` (P_l(1) = 1: the same for every l), ``npairs[b] = sum_i |N_i(b)|`` (int64, exact), ``wpairs[b] = sum_i w_i
   sum_{j in N_i(b)} w_j``.
5. How.  Per primary the kernel forms ``A_{l,c}(b) = sum_j w_j Y_{l,c}(u_ij)`` over the 2 l + 1 real components, for m =
   0 .. l: ``Y = N_lm Q_l^m(u_z) Re / Im (u_x + i u_y)^m``, ``N_lm = sqrt(eps_m (l - m)! / (l + m)!)`` with eps_0 = 1 and
   eps_m = 2 otherwise; ``Q_l^m = P_l^m / sin^m`` is a polynomial in u_z from ``Q_m^m = (2 m - 1)!!``, ``Q_{m+1}^m =
   (2 m + 1) z Q_m^m`` and ``(l - m) Q_l^m = (2 l - 1) z Q_{l-1}^m - (l + m - 1) Q_{l-2}^m``; ``(u_x + i u_y)^m`` by
   repeated complex multiplication.  By the addition theorem ``sum_c A_{l,c}(b1) A_{l,c}(b2)`` is the double sum of
   P_l, and ``zeta_l += w_i`` times it.  N_00 Q_0^0 = 1 exactly: with unit weights zeta_0 is a sum of integers, exact
   below 2^53.
6. Forms.  Auto (``pos2 is None``): the secondaries are the primaries.  Cross: the primaries are ``pos``, both
   neighbours come from ``pos2``.  The order of the double sums is unspecified; npairs, and zeta_0 with unit weights,
   never vary.

    from pmesh_amd.threept import threept_multipoles, threept_correlation
    tp = threept_multipoles(pm, pos, edges, poles=(0, 1, 2))
    tp.zeta, tp.diag, tp.npairs, tp.wpairs, tp.normalized()
    zeta_hat, tp = threept_correlation(pm, pos, edges, poles=(0, 2))

``normalized()`` is ``zeta_l (2 l + 1) / (4 pi)^2``, the ``sum_m a_lm a*_lm / (4 pi)`` normalisation of Slepian &
Eisenstein's eq. 15.  nbodykit is not a dependency and no test pins agreement with it beyond this formula.

Host: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) with the radius b and one kernel per rank.  Every
primary sees its whole neighbourhood on its owner, so one allreduce of the three float arrays, packed, and one of
npairs finish it, and nothing is subtracted afterwards.
"""
import numpy
import torch

from . import _abi, backend
from ._cells import Neighbourhood, allsum, box_of, read_rows, refuse_not_finite, sorted_sets, together, within_reach
from .paircount import _edges, bin_volumes, too_many

MAX_ELL = _abi.PMX_THREEPT_MAX_ELL
MAX_BINS = _abi.PMX_THREEPT_MAX_BINS


class ThreePoint(object):
    """The sums of rule 4, identical on every rank: ``zeta`` (len(poles), nr, nr), ``diag`` and ``wpairs`` (nr,)
    (float64) and ``npairs`` (nr,) (int64), device tensors; zeta is symmetric in its last two axes.  ``poles`` (a
    tuple), ``edges`` (a numpy array), ``auto``, ``BoxSize``; the power sums of the weights over all ranks (row counts
    without weights): ``W1`` (sum of w over the primaries), ``W2``, ``W2sq`` (sum of w and of w^2 over the secondaries)
    and ``W3`` (auto: the sum of w^3; cross: 0)."""

    def __init__(self, zeta, diag, wpairs, npairs, poles, edges, auto, BoxSize, W1, W2, W2sq, W3):
        self.zeta, self.diag, self.wpairs, self.npairs = zeta, diag, wpairs, npairs
        self.poles, self.edges, self.auto, self.BoxSize = poles, edges, auto, BoxSize
        self.W1, self.W2, self.W2sq, self.W3 = W1, W2, W2sq, W3

    def normalized(self):
        """zeta_l (2 l + 1) / (4 pi)^2 (Slepian & Eisenstein 2015, eq. 15)"""
        f = numpy.array([(2 * l + 1) / (4 * numpy.pi) ** 2 for l in self.poles])
        return self.zeta * torch.from_numpy(f).to(self.zeta.device)[:, None, None]


def _poles(poles):
    """(the poles as a tuple of ints, error)"""
    try:
        p = [x for x in poles]
        ok = len(p) > 0 and all(int(x) == x for x in p)
    except (TypeError, ValueError):
        ok = False
    if not ok or len(set(int(x) for x in p)) != len(p) or min(p) < 0 or max(p) > MAX_ELL:
        return None, ValueError('poles must be distinct integers in 0 .. %d (PMX_THREEPT_MAX_ELL), at least one' % MAX_ELL)
    return tuple(int(x) for x in p), None


def local_multipoles(be, pos1, w1, pos2, w2, grid, box, e2, lmax):
    """The four arrays of the rows of one rank on the cell grid `grid` (of _cells.cell_grid): the primaries `pos1` with
    the secondaries `pos2` (None: pos1 itself).  e2: a device tensor.  Returns (zeta of the shape (lmax + 1, nr, nr),
    diag, wpairs, npairs)."""
    dev = pos1.device
    nr = e2.numel() - 1
    zeta = torch.zeros((lmax + 1, nr, nr), dtype=torch.float64, device=dev)
    diag = torch.zeros(nr, dtype=torch.float64, device=dev)
    wpairs = torch.zeros(nr, dtype=torch.float64, device=dev)
    npairs = torch.zeros(nr, dtype=torch.int64, device=dev)
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, pos1, pos2, grid, box)
    if pos2 is None:
        w2 = w1
    be.threept_multipoles(spos1, order1, cell_of1, w1, spos2, order2, cell_start2, w2, grid[0], grid[3], box, e2,
                          lmax, zeta, diag, wpairs, npairs)
    return zeta, diag, wpairs, npairs


def _power_sums(comm, w, n):
    """(sum of w, of w^2, of w^3) over all ranks, as floats; the row count three times without weights"""
    if w is None:
        total = float(comm.allreduce(n)) if comm.size > 1 else float(n)
        return total, total, total
    w = w.to(torch.float64)
    s = allsum(comm, torch.stack([w.sum(), (w * w).sum(), (w * w * w).sum()])).cpu()
    return float(s[0]), float(s[1]), float(s[2])


def threept_multipoles(pm, pos, edges, poles=(0, 1, 2), pos2=None, weight=None, weight2=None):
    """The three-point multipole sums of the rows by the rule of the module docstring: a ThreePoint.

    pm : ParticleMesh of three dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos : (n, 3) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    edges : the nr + 1 edges of the radial bins, in box units; nr <= 32.
    poles : distinct integers in 0 .. 10, in the order the first axis of ``zeta`` takes.
    pos2 : the rows both neighbours are taken from, or None: from pos.
    weight, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd != 3:
        raise NotImplementedError('three-point multipoles need a mesh of three dimensions, not %d' % nd)
    box = box_of(pm)
    auto = pos2 is None
    e, error = _edges(edges, 'edges')
    b = None
    if error is None:
        error = too_many(e, None, MAX_BINS, '(PMX_THREEPT_MAX_BINS)')
    if error is None:
        b = float(e[-1])
        if not within_reach(b, box):
            error = ValueError('the largest separation must be finite, positive and at most half the shortest box '
                               'side: %r' % b)
    if error is None:
        poles, error = _poles(poles)
    if error is None and auto and weight2 is not None:
        error = ValueError('weight2 needs pos2')
    wanted = (('pos', pos, nd, None), ('pos2', pos2, nd, None), ('weight', weight, 1, 0), ('weight2', weight2, 1, 1))
    (pos, pos2, weight, weight2), error = read_rows(pm, be, wanted, error)
    together(comm, error)
    if weight is not None:
        weight = weight.reshape(-1)
    if weight2 is not None:
        weight2 = weight2.reshape(-1)
    refuse_not_finite(comm, 'pos and pos2', pos, pos2)
    n1 = pos.shape[0]
    sums1 = _power_sums(comm, weight, n1)
    W1 = sums1[0]
    if auto:
        W2, W2sq, W3 = sums1
    else:
        W2, W2sq, _ = _power_sums(comm, weight2, pos2.shape[0])
        W3 = 0.0
    lmax = max(poles)
    dev = be.device
    e2 = torch.from_numpy(e * e).to(dev)
    hood = Neighbourhood(pm, b, pos, pos2)
    p1, q1 = hood.to_owners(pos), hood.to_owners(weight)
    p2, q2 = hood.to_sources(pos if auto else pos2), hood.to_sources(weight if auto else weight2)
    sums = local_multipoles(be, p1, q1, None if hood.same else p2, q2, hood.grid, box, e2, lmax)
    if comm.size > 1:
        # the three float arrays travel as one
        nr = len(e) - 1
        flat = hood.allsum(torch.cat([sums[0].reshape(-1), sums[1], sums[2]]))
        nz = (lmax + 1) * nr * nr
        sums = (flat[:nz].reshape(lmax + 1, nr, nr), flat[nz:nz + nr], flat[nz + nr:], hood.allsum(sums[3]))
    zeta, diag, wpairs, npairs = sums
    zeta = zeta[list(poles)].contiguous()
    return ThreePoint(zeta, diag, wpairs, npairs, poles, e, auto, box, W1, W2, W2sq, W3)


def triplet_weight(tp):
    """T: the sum of w_i w_j w_k over the triplets of distinct rows a ThreePoint was summed over.  Auto: W1^3 - 3 W1
    W2sq + 2 W3; cross (i from the primaries, j != k from the secondaries): W1 (W2^2 - W2sq)."""
    if tp.auto:
        return tp.W1 ** 3 - 3 * tp.W1 * tp.W2sq + 2 * tp.W3
    return tp.W1 * (tp.W2 ** 2 - tp.W2sq)


def threept_correlation(pm, pos, edges, poles=(0, 1, 2), pos2=None, weight=None, weight2=None):
    """(zeta_hat, ThreePoint): the natural estimator with analytic randoms of the multipoles of the FULL three-point
    function (the connected part needs the caller's xi(r): it is not subtracted here),

        zeta_hat_l[b1, b2] = (2 l + 1) (zeta_l[b1, b2] - [b1 == b2] diag[b1]) / RRR[b1, b2] - [l == 0]
        RRR = T V_b1 V_b2 / V_box^2

    with V_b of paircount.bin_volumes and T of triplet_weight: a float64 device tensor of the shape of ``zeta``.  The
    arguments are those of threept_multipoles.  Host arithmetic on the returned numbers."""
    tp = threept_multipoles(pm, pos, edges, poles, pos2, weight, weight2)
    v = bin_volumes(tp.edges, 3) / float(numpy.prod(tp.BoxSize))
    rrr = triplet_weight(tp) * v[:, None] * v[None, :]
    dev = tp.zeta.device
    f = torch.tensor([2.0 * l + 1 for l in tp.poles], dtype=torch.float64, device=dev)[:, None, None]
    mono = torch.tensor([1.0 if l == 0 else 0.0 for l in tp.poles], dtype=torch.float64, device=dev)[:, None, None]
    zeta_hat = f * (tp.zeta - torch.diag(tp.diag)[None]) / torch.from_numpy(numpy.ascontiguousarray(rrr)).to(dev) - mono
    return zeta_hat, tp
