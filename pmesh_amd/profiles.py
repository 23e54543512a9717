"""Radial profiles about centres and spherical-overdensity masses, made on the device.

What a user of ``fof_catalog`` asks for next: the density profile and the enclosed mass of every halo about its
``CMPosition``, the radius and mass at a given overdensity (R_200, M_200), void and stacked profiles about arbitrary
centres, counts in spheres, and the surface density Sigma(R) and Delta Sigma(R) about lenses.  The other particle
modules sum over all primaries; this one keeps the histogram of every centre apart, in one launch for all of them,
where a loop of ``pair_counts`` over the centres costs one launch and one host synchronisation each.  No entry of the
C ABI is added: ``pmx_pair_counts`` (include/pmesh_amd.h) has two more modes, PMX_PAIRS_1D_ROWS (5) and
PMX_PAIRS_PROJECTED_ROWS (6), whose kernels (csrc/pmx_pairs_rows.hip) give one wave to every centre.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Shared with pmesh_amd.paircount.  Rows, wrapping, minimum image, ``r2``, ``q``, the squared edges, the r-bin, the
   pi-bin and the ``pimax`` cut are exactly those of its modes ``'1d'`` and ``'projected'`` (rules 1, 3 and 5 there).
   All arithmetic is in double, every operation rounded once, with no contraction and no square root to choose a bin.
   ``'projected'`` needs ndim == 3 and ``los`` in {0, 1, 2}; ``'1d'`` takes ndim 1 to 3.
2. Bin index.  The bin of a pair (centre i, source j) is ``(i * nr + rbin) * nsub + subbin``, i the row of the centre
   in the caller's order; ``nsub`` is 1 in the mode 1d and the number of pi bins in the projected mode.
3. Sums, per centre and bin.  ``npart`` is int64 and exact and depends on no decomposition or launch; ``mass = sum
   weight_i mass_j`` and ``rsum = sum weight_i mass_j sqrt(q)`` are double sums in no particular order: their last
   bits may vary from run to run.  Without ``mass`` and ``weight``, ``mass`` is ``npart`` as a double.
4. No row identity.  A centre that coincides with a source has ``r2 == 0``: it is counted in bin 0 when ``edges[0] ==
   0`` and nowhere otherwise.  A profile of rows about themselves holds every row in its own first bin.
5. Search radius.  ``b = edges[-1]``, in the projected mode ``hypot(edges[-1], piedges[-1])``; b is finite, positive
   and ``2 b <= min_d L_d``, otherwise ValueError on every rank.  Rows with a coordinate that is not finite raise
   ValueError with their number, on every rank.
6. Bin limit.  ``nr * nsub`` is at most PMX_PAIRS_ROWS_MAX_BINS (256); more raise ValueError.

    from pmesh_amd.profiles import radial_profiles, so_masses
    prof = radial_profiles(pm, cat.CMPosition, pos, edges, mass=m)     # prof.npart, prof.mass, prof.rmean: (nc, nr)
    prof.density(), prof.cumulative()                                  # rho(r) and M(< r) of every centre
    so = so_masses(pm, cat.CMPosition, pos, 200, rho_mean, mass=m)     # so.radius, so.mass, so.found

Host: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) with the centres as primaries and the radius b; one
kernel per rank fills all histograms, and they return to the caller's rows with the mode 'min'.  Every centre has one
owner: there is no allreduce.  With fewer centres
than the device has wave slots (a few thousand) the device is under-filled; a row is not split over several waves.
"""
import numpy
import torch

from . import _abi, backend
from ._cells import Neighbourhood, box_of, read_rows, refuse_not_finite, sorted_sets, together, within_reach
from .knn import ball_volume
from .paircount import _binning, bin_volumes

MAX_BINS = _abi.PMX_PAIRS_ROWS_MAX_BINS
ROW_MODES = {'1d': _abi.PMX_PAIRS_1D_ROWS, 'projected': _abi.PMX_PAIRS_PROJECTED_ROWS}


class ProfileResult(object):
    """The histograms of one rank's centres, device tensors in the caller's row order, of the shape (nc, nr) or, in the
    projected mode, (nc, nr, npi): ``npart`` (int64), ``mass`` (the weighted count), ``rsum`` and ``rmean = rsum /
    mass`` (float64; nan where the bin holds no pair); and ``edges``, ``piedges`` (numpy arrays; None in the mode 1d),
    ``mode``, ``los``, ``ndim``."""

    def __init__(self, npart, mass, rsum, edges, piedges, mode, los, ndim):
        self.npart, self.mass, self.rsum = npart, mass, rsum
        nan = torch.full_like(rsum, float('nan'))
        self.rmean = torch.where(npart > 0, rsum / torch.where(npart > 0, mass, torch.ones_like(mass)), nan)
        self.edges, self.piedges, self.mode, self.los, self.ndim = edges, piedges, mode, los, ndim

    def _host(self, a):
        return torch.from_numpy(numpy.ascontiguousarray(a, dtype='f8')).to(self.mass.device)

    def density(self):
        """mass over the volume of the bin (paircount.bin_volumes): rho(r), or in the projected mode rho(rp, pi)"""
        return self.mass / self._host(bin_volumes(self.edges, self.ndim, self.mode, self.piedges))

    def cumulative(self):
        """the mass through every bin of r (of rp): the cumulative sum along r in float64, M(< edges[k + 1]) where
        edges[0] == 0"""
        return torch.cumsum(self.mass, dim=1)

    def sigma(self):
        """(projected) Sigma(R): the mass of every annulus, summed over the pi bins, over its area: (nc, nr)"""
        if self.mode != 'projected':
            raise ValueError("sigma needs mode='projected'")
        e = self.edges
        return self.mass.sum(dim=2) / self._host(numpy.pi * (e[1:] ** 2 - e[:-1] ** 2))

    def delta_sigma(self):
        """(projected, edges[0] == 0) Delta Sigma of every annulus: the mean surface density inside its outer edge,
        ``M(< edges[k + 1]) / (pi edges[k + 1]^2)``, less its own Sigma: (nc, nr)"""
        if self.mode != 'projected':
            raise ValueError("delta_sigma needs mode='projected'")
        if self.edges[0] != 0:
            raise ValueError('delta_sigma needs edges[0] == 0: the mass inside the first edge is not known')
        inside = torch.cumsum(self.mass.sum(dim=2), dim=1) / self._host(numpy.pi * self.edges[1:] ** 2)
        return inside - self.sigma()


class SOResult(object):
    """``radius`` and ``mass`` (float64 (nc,) device tensors; nan where no crossing was found), ``found`` (bool (nc,))
    and ``profile``, the ProfileResult they were read from."""

    def __init__(self, radius, mass, found, profile):
        self.radius, self.mass, self.found, self.profile = radius, mass, found, profile


def local_profiles(be, mode, los, centres, pos, weight1, weight2, grid, box, e2, sub):
    """The histograms of the rows of one rank on the cell grid `grid` (of _cells.cell_grid): every row of `centres` with
    every row of `pos`.  e2 and sub: device tensors.  mode: a key of ROW_MODES.  Returns (npairs, wnpairs, rsum) of the
    shape (n1, nr, nsub) in the row order of `centres`."""
    dev = centres.device
    n1 = centres.shape[0]
    shape = (n1, e2.numel() - 1, sub.numel() - 1 if sub is not None else 1)
    npairs = torch.zeros(shape, dtype=torch.int64, device=dev)
    wnpairs = torch.zeros(shape, dtype=torch.float64, device=dev)
    rsum = torch.zeros(shape, dtype=torch.float64, device=dev)
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, centres, pos, grid, box)
    be.pair_counts(ROW_MODES[mode], los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2,
                   grid[0], grid[3], box, e2, sub, npairs, wnpairs, rsum)
    return npairs, wnpairs, rsum


def radial_profiles(pm, centres, pos, edges, mass=None, weight=None, mode='1d', piedges=None, pimax=None, los=2):
    """The histograms of the rows `pos` about every row of `centres` by the rule of the module docstring: a
    ProfileResult.

    pm : ParticleMesh of 1, 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    centres : (nc, ndim), pos : (n, ndim), float64 or float32, device tensors or numpy arrays, this rank's rows (any
        number, none included).
    edges : the nr + 1 edges of the bins of r (of rp in the projected mode), in box units.
    mass : (n,) float rows, one per source, or None for 1.  weight : (nc,) float rows, one per centre, or None for 1.
    mode : '1d' or 'projected'.  piedges, or pimax for bins of unit width in [0, pimax]; los : the axis of the line of
        sight (the conventions of pair_counts).

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('profiles on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    box = box_of(pm)
    e = sub = b = None
    if mode not in ROW_MODES:
        error = ValueError("mode must be '1d' or 'projected', not %r" % (mode,))
    else:
        e, sub, error = _binning(nd, edges, mode, None, None, piedges, pimax, los)
    if error is None:
        nbins = (len(e) - 1) * (len(sub) - 1 if sub is not None else 1)
        if nbins > MAX_BINS:
            error = ValueError('%d bins per centre: at most %d (PMX_PAIRS_ROWS_MAX_BINS)' % (nbins, MAX_BINS))
    if error is None:
        b = float(numpy.hypot(e[-1], sub[-1])) if mode == 'projected' else float(e[-1])
        if not within_reach(b, box):
            error = ValueError('the largest separation must be finite, positive and at most half the shortest box '
                               'side: %r' % b)
    wanted = (('centres', centres, nd, None), ('pos', pos, nd, None), ('weight', weight, 1, 0), ('mass', mass, 1, 1))
    (centres, pos, weight, mass), error = read_rows(pm, be, wanted, error)
    together(comm, error)
    if weight is not None:
        weight = weight.reshape(-1)
    if mass is not None:
        mass = mass.reshape(-1)
    refuse_not_finite(comm, 'centres and pos', centres, pos)
    dev = be.device
    e2 = torch.from_numpy(numpy.ascontiguousarray(e * e)).to(dev)
    subt = None if sub is None else torch.from_numpy(numpy.ascontiguousarray(sub)).to(dev)
    nc = centres.shape[0]
    hood = Neighbourhood(pm, b, centres, pos)
    p1, q1 = hood.to_owners(centres), hood.to_owners(weight)
    p2, q2 = hood.to_sources(pos), hood.to_sources(mass)
    sums = local_profiles(be, mode, los, p1, p2, q1, q2, hood.grid, box, e2, subt)
    sums = [hood.to_callers(x.flatten(1), 'min') for x in sums]
    shape = (nc, len(e) - 1) if sub is None else (nc, len(e) - 1, len(sub) - 1)
    npart, wsum, rsum = [s.reshape(shape) for s in sums]
    return ProfileResult(npart, wsum, rsum, e, sub, mode, los, nd)


def so_masses(pm, centres, pos, delta, rho_ref, mass=None, rmin=None, rmax=None, nbins=64):
    """The spherical-overdensity radius and mass of every centre: an SOResult.

    The rule.  ``edges = [0] + geomspace(rmin, rmax, nbins)``: nbins bins, bin 0 = [0, rmin).  With ``M_k`` the
    cumulative mass through bin k of radial_profiles(pm, centres, pos, edges, mass=mass), ``R_k = edges[k + 1]`` and
    ``D_k = M_k / (rho_ref V_ndim(R_k))`` (knn.ball_volume), the crossing is the smallest k >= 1 with ``D_{k-1} >=
    delta`` and ``D_k < delta``; ``found`` says whether there is one.  There ``log R_delta`` interpolates linearly in
    ``log D`` between (R_{k-1}, D_{k-1}) and (R_k, D_k), and ``M_delta = delta rho_ref V_ndim(R_delta)``.  Without a
    crossing radius and mass are nan.  The result depends on no schedule beyond the last bits of the mass sums (none
    at all without `mass`).

    delta, rho_ref : positive numbers (200 and the mean density for M_200m).  rmin, rmax : 0 < rmin < rmax, 2 rmax <=
    min(BoxSize); the defaults are min(BoxSize) / 4 and rmax / 1000.  nbins : 2 .. 256.  All of it is torch on the device
    on top of one radial_profiles call: there is no host loop over the centres.
    """
    nd = len(pm.Nmesh)
    box = box_of(pm)
    error = edges = None
    try:
        delta, rho_ref = float(delta), float(rho_ref)
        rmax = float(min(box)) / 4 if rmax is None else float(rmax)
        rmin = rmax / 1000 if rmin is None else float(rmin)
        if int(nbins) != nbins:
            raise ValueError
        nbins = int(nbins)
    except (TypeError, ValueError):
        error = ValueError('delta, rho_ref, rmin and rmax must be numbers and nbins an integer')
    if error is None and not (delta > 0 and rho_ref > 0 and numpy.isfinite(delta) and numpy.isfinite(rho_ref)):
        error = ValueError('delta and rho_ref must be finite and positive')
    if error is None and not (0 < rmin < rmax and numpy.isfinite(rmax)):
        error = ValueError('rmin and rmax must be finite with 0 < rmin < rmax')
    if error is None and not 2 <= nbins <= MAX_BINS:
        error = ValueError('nbins must be in 2 .. %d (PMX_PAIRS_ROWS_MAX_BINS)' % MAX_BINS)
    if error is None:
        edges = numpy.concatenate([[0.0], numpy.geomspace(rmin, rmax, nbins)])
    together(pm.comm, error)
    prof = radial_profiles(pm, centres, pos, edges, mass=mass)
    dev = prof.mass.device
    nc = prof.mass.shape[0]
    R = torch.from_numpy(edges[1:].copy()).to(dev)
    D = prof.cumulative() / (rho_ref * ball_volume(R, nd))
    cross = (D[:, :-1] >= delta) & (D[:, 1:] < delta)
    found = cross.any(dim=1)
    k = cross.to(torch.int8).argmax(dim=1) + 1                     # (the first crossing; 1 where there is none)
    rows = torch.arange(nc, device=dev)
    d0, d1 = D[rows, k - 1], D[rows, k]
    l0, l1 = torch.log(R[k - 1]), torch.log(R[k])
    g0, g1 = torch.log(d0), torch.log(d1)
    logr = l0 + (numpy.log(delta) - g0) / (g1 - g0) * (l1 - l0)
    nan = torch.full_like(logr, float('nan'))
    radius = torch.where(found, torch.exp(logr), nan)
    return SOResult(radius, torch.where(found, delta * rho_ref * ball_volume(radius, nd), nan), found, prof)
