"""Moment sums of the sources about centres, made on the device: halo shapes, spins and velocity dispersions.

What a user of ``fof_catalog`` and ``so_masses`` asks for next: the inertia tensor, the axis ratios and the major axis of
every halo, its centre-of-mass offset, its velocity dispersion, its angular momentum and its spin.  All of them are sums
over the sources inside spheres about a centre: the walk of pmesh_amd.profiles, with a payload per pair and with bins in
units of every centre's own radius, so that "inside R_200 of every halo" is one call.  No entry of the C ABI is added:
``pmx_pair_counts`` (include/pmesh_amd.h) has one more mode, PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS (517), whose kernel
(csrc/pmx_pairs_moments.hip) gives one wave to every centre.  It closes the chain

    fof -> fof_catalog -> so_masses -> halo_shapes -> alignment_counts

The rule (normative; include/pmesh_amd.h restates it next to the flag).  ndim is 2 or 3.

1. Rows, wrap and minimum image are those of pmesh_amd.profiles in the mode 1d (rule 1 there).  For centre i and source
   j: ``dx_d`` is what the row mode forms, centre minus source, minimum image; ``q = sum_d dx_d^2`` from 0 in ascending
   d, in double, every operation rounded once, no contraction; ``s_d = -dx_d`` (exact) is the source as seen from the
   centre.
2. Columns.  The centre brings ``(w_i, s2_i)``: its weight (1 without `weight`) and the square of its scale (1.0
   without `scale`), finite and positive.  The source brings ``(m_j)`` or ``(m_j, v_0 .. v_{ndim-1})`` (m_j = 1 without
   `mass`).  Float or double; a float is widened exactly.
3. Bins.  The edges of centre i are ``E_k = e2[k] * s2_i``, ``e2[k] = edges[k] * edges[k]``, one rounding each.  The
   pair is in bin k when ``E_k <= q < E_{k+1}`` and is not counted when ``q < E_0`` or ``q >= E_nr``: the comparisons
   of the profiles on E in place of e2; no square root chooses a bin.  With ``s2_i == 1.0`` the bins are bit for bit
   those of ``radial_profiles``.  At most PMX_PAIRS_MOMENTS_MAX_BINS (64) bins; more raise ValueError.
4. Sums, per centre i and bin b, with ``m = w_i * m_j`` (one rounding): ``npart += 1`` (int64, exact, independent of
   any decomposition or launch); ``mass += m``; and, in this order in the kernel's array of NS sums per (centre, bin),
   ``rsum += m * sqrt(q)``; ``first_d += m * s_d``; ``second_ab += m * s_a * s_b`` for a <= b in the order 00, 01, 02,
   11, 12, 22; ``reduced_ab += (m * s_a * s_b) / q``, the term 0 where ``q == 0``; and with velocities ``momentum_d +=
   m * v_d``; ``kinetic += m * (sum_d v_d^2)``; ``angular += m * (s x v)``: ``(s_1 v_2 - s_2 v_1, s_2 v_0 - s_0 v_2,
   s_0 v_1 - s_1 v_0)`` in three dimensions, ``s_0 v_1 - s_1 v_0`` in two.  NS = 16 or 23 in three dimensions, 9 or 13
   in two.  These are double sums in no fixed order: their last bits may vary from run to run; within a term the
   operations may be contracted or regrouped, at most four roundings per term.
5. No row identity.  A source that coincides with a centre is a pair at ``q == 0``, as in pmesh_amd.profiles rule 4:
   counted in bin 0 when ``edges[0] == 0``, with ``s == 0`` and its reduced term 0.
6. Search radius.  ``b = edges[-1] * max(scale)``, the maximum over the centres of all ranks (1 without `scale`); b is
   finite, positive and ``2 b <= min_d L_d``, otherwise ValueError on every rank.  A scale that is not finite and
   positive, and rows with a coordinate (or a mass, a velocity, a weight) that is not finite, raise ValueError on
   every rank.

    from pmesh_amd.moments import radial_moments, halo_shapes, ellipticity_from_shapes
    so = so_masses(pm, cat.CMPosition, pos, 200, rho_mean, mass=m)
    shapes = halo_shapes(pm, cat.CMPosition, pos, so.radius, mass=m, vel=vel, centre_vel=cat.CMVelocity)
    shapes.b_over_a, shapes.c_over_a, shapes.sigma, shapes.spin        # (nc,) each; nan where R_200 was not found
    ac = alignment_counts(pm, cat.CMPosition[1:], shapes.major[1:], edges)   # omega(r), eta(r) of the halo axes
    g = ellipticity_from_shapes(shapes)                                # (g1, g2) rows for projected_alignment_counts
    mom = radial_moments(pm, centres, pos, [0, 0.5, 1, 2], mass=m, scale=so.radius)   # shells in units of R_200
    mom.within(1).second                                               # the moments inside R_200: (nc, 1, 3, 3)

Host: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) with the centres as primaries and the radius b, exactly
as ``radial_profiles`` does it; one kernel per rank fills all sums, and they return to the caller's rows with the mode
'min'.  Every centre has one owner: there is no allreduce of sums.  ``halo_shapes`` is torch on the device on top of
one ``radial_moments`` call, with no host loop over the centres.

Out of scope: iterative reduced or ellipsoidal-aperture tensors, shapes from the FoF membership, projected moment sums,
jackknife combinations, gradients.
"""
import numpy
import torch

from . import _abi, backend
from ._cells import Neighbourhood, box_of, read_rows, refuse_not_finite, sorted_sets, together, within_reach
from .alignments import ellipticity_from_orientation
from .paircount import _binning

MAX_BINS = _abi.PMX_PAIRS_MOMENTS_MAX_BINS
MOMENTS_MODE = _abi.PMX_PAIRS_MOMENTS | _abi.PMX_PAIRS_1D_ROWS


def tensor_pairs(ndim):
    """the (a, b), a <= b, of the NT = ndim (ndim + 1) / 2 components of a symmetric tensor in the order of rule 4"""
    return [(a, b) for a in range(ndim) for b in range(a, ndim)]


def moment_sums(ndim, vel):
    """NS of rule 4: the doubles per (centre, bin) of the kernel's rsum"""
    return 1 + ndim + ndim * (ndim + 1) + ((ndim + 1 + (3 if ndim == 3 else 1)) if vel else 0)


def _symmetric(t, ndim):
    """(..., NT) components in the order of tensor_pairs -> (..., ndim, ndim), symmetric"""
    out = t.new_zeros(t.shape[:-1] + (ndim, ndim))
    for k, (a, b) in enumerate(tensor_pairs(ndim)):
        out[..., a, b] = t[..., k]
        out[..., b, a] = t[..., k]
    return out


class MomentsResult(object):
    """The moment sums of one rank's centres, float64 device tensors in the caller's row order (``npart``: int64):
    ``npart``, ``mass``, ``rsum`` and ``rmean = rsum / mass`` (nc, nr; nan where the bin holds no pair); ``first`` (nc,
    nr, ndim); ``second`` and ``reduced`` (nc, nr, ndim, ndim), symmetric; with velocities ``momentum`` (nc, nr, ndim),
    ``kinetic`` (nc, nr) and ``angular`` (nc, nr, NL; NL = 3 in three dimensions, 1 in two), otherwise None; and
    ``edges`` (numpy), ``scale`` ((nc,) device tensor, or None: the edges are in box units) and ``ndim``."""

    def __init__(self, npart, mass, rsum, first, second, reduced, momentum, kinetic, angular, edges, scale, ndim):
        self.npart, self.mass, self.rsum = npart, mass, rsum
        self.first, self.second, self.reduced = first, second, reduced
        self.momentum, self.kinetic, self.angular = momentum, kinetic, angular
        self.edges, self.scale, self.ndim = edges, scale, ndim
        nan = torch.full_like(rsum, float('nan'))
        self.rmean = torch.where(npart > 0, rsum / torch.where(npart > 0, mass, torch.ones_like(mass)), nan)

    def within(self, k=None):
        """The cumulative sums along r: a MomentsResult whose bin j holds the sums of the bins 0 .. j, the aperture
        ``edges[0] * scale <= r < edges[j + 1] * scale`` (the ball ``r < edges[j + 1] * scale`` where edges[0] == 0).
        With k, only the aperture through bin k: one bin, of the edges ``[edges[0], edges[k + 1]]``."""
        def cum(t):
            if t is None:
                return None
            c = torch.cumsum(t, dim=1)
            return c if k is None else c[:, k:k + 1]
        nr = len(self.edges) - 1
        if k is not None and not 0 <= k < nr:
            raise ValueError('k must be in 0 .. %d, not %r' % (nr - 1, k))
        edges = self.edges if k is None else numpy.array([self.edges[0], self.edges[k + 1]])
        return MomentsResult(cum(self.npart), cum(self.mass), cum(self.rsum), cum(self.first), cum(self.second),
                             cum(self.reduced), cum(self.momentum), cum(self.kinetic), cum(self.angular), edges,
                             self.scale, self.ndim)


class ShapeResult(object):
    """What halo_shapes returns, float64 device tensors with one row per centre in the caller's order (``npart``:
    int64): ``npart``, ``mass``, ``offset`` (nc, ndim), ``tensor`` (nc, ndim, ndim), ``eigenvalues`` (nc, ndim;
    descending), ``axes`` (nc, ndim, ndim; axes[:, k] the unit eigenvector of eigenvalues[:, k], its largest component
    positive), ``major`` = axes[:, 0], ``b_over_a``, ``c_over_a`` and ``triaxiality`` (nc; the last two None in two
    dimensions); with velocities ``velocity`` (nc, ndim), ``sigma`` (nc), ``angular_momentum`` (nc, NL) and ``spin``
    (nc; None in two dimensions), otherwise None; ``radius`` (nc), ``moments`` (the MomentsResult they were read from)
    and ``ndim``.  Rows of centres without a radius or with fewer than ndim + 1 sources are nan."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def local_moments(be, centres, pos, weight1, weight2, grid, box, e2):
    """The sums of the rows of one rank on the cell grid `grid` (of _cells.cell_grid): every row of `centres` with every
    row of `pos`.  weight1: the (n1, 2) block (w, s2); weight2: the (n2, 1) block (m) or the (n2, 1 + ndim) block (m, v);
    e2: a device tensor.  Returns (npairs, wnpairs, rsum) of the shapes (n1, nr), (n1, nr) and (n1, nr, NS) in the row
    order of `centres`."""
    dev = centres.device
    n1, nd, nr = centres.shape[0], centres.shape[1], e2.numel() - 1
    ns = moment_sums(nd, weight2.shape[1] > 1)
    npairs = torch.zeros((n1, nr), dtype=torch.int64, device=dev)
    wnpairs = torch.zeros((n1, nr), dtype=torch.float64, device=dev)
    rsum = torch.zeros((n1, nr, ns), dtype=torch.float64, device=dev)
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, centres, pos, grid, box)
    be.pair_counts(MOMENTS_MODE, 0, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, grid[0],
                   grid[3], box, e2, None, npairs, wnpairs, rsum)
    return npairs, wnpairs, rsum


def radial_moments(pm, centres, pos, edges, mass=None, vel=None, weight=None, scale=None):
    """The moment sums of the rows `pos` about every row of `centres` by the rule of the module docstring: a
    MomentsResult.

    pm : ParticleMesh of 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    centres : (nc, ndim), pos : (n, ndim), float64 or float32, device tensors or numpy arrays, this rank's rows (any
        number, none included).
    edges : the nr + 1 edges of the bins of r: in box units, or with `scale` in units of every centre's scale.
    mass : (n,) float rows, one per source, or None for 1.  vel : (n, ndim) float rows, or None: no velocity sums.
    weight : (nc,) float rows, one per centre, or None for 1.  scale : (nc,) positive float rows, or None.

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('moments on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    box = box_of(pm)
    e = None
    if nd < 2:
        error = ValueError('moments need a mesh of two or three dimensions, not %d' % nd)
    else:
        e, _, error = _binning(nd, edges, '1d', None, None, None, None, 2)
    if error is None and len(e) - 1 > MAX_BINS:
        error = ValueError('%d bins per centre: at most %d (PMX_PAIRS_MOMENTS_MAX_BINS)' % (len(e) - 1, MAX_BINS))
    wanted = (('centres', centres, nd, None), ('pos', pos, nd, None), ('weight', weight, 1, 0), ('scale', scale, 1, 0),
              ('mass', mass, 1, 1), ('vel', vel, nd, 1))
    (centres, pos, weight, scale, mass, vel), error = read_rows(pm, be, wanted, error)
    together(comm, error)
    f8 = torch.float64
    nc, n = centres.shape[0], pos.shape[0]
    dev = be.device
    smax = 1.0
    if scale is not None:
        scale = scale.reshape(-1).to(f8)
        good = bool((torch.isfinite(scale) & (scale > 0)).all())
        together(comm, None if good else ValueError('scale must be finite and positive for every centre'))
        smax = float(scale.max()) if nc else 0.0
        if comm.size > 1:
            smax = float(comm.allreduce(smax, op='max'))
        if smax == 0.0:                                            # (no centre on any rank)
            smax = 1.0
    b = float(e[-1]) * smax
    if not within_reach(b, box):
        raise ValueError('the largest separation, edges[-1] * max(scale), must be finite, positive and at most half '
                         'the shortest box side: %r' % b)            # (b is the same on every rank)
    refuse_not_finite(comm, 'centres and pos', centres, pos)
    refuse_not_finite(comm, 'weight, mass and vel', weight, mass, vel, entry='an entry')
    # the columns: (w, s2) of the centres in double; (m) or (m, v) of the sources, in float where all given are
    ones = lambda k, dt: torch.ones((k, 1), dtype=dt, device=dev)
    w1 = torch.cat([ones(nc, f8) if weight is None else weight.reshape(-1, 1).to(f8),
                    ones(nc, f8) if scale is None else (scale * scale).reshape(-1, 1)], dim=1)
    given = [t for t in (mass, vel) if t is not None]
    dt = torch.float32 if all(t.dtype == torch.float32 for t in given) else f8
    w2 = torch.cat([ones(n, dt) if mass is None else mass.reshape(-1, 1).to(dt)] +
                   ([] if vel is None else [vel.to(dt)]), dim=1)
    e2 = torch.from_numpy(numpy.ascontiguousarray(e * e)).to(dev)
    hood = Neighbourhood(pm, b, centres, pos)
    p1, q1 = hood.to_owners(centres), hood.to_owners(w1)
    p2, q2 = hood.to_sources(pos), hood.to_sources(w2)
    sums = local_moments(be, p1, p2, q1, q2, hood.grid, box, e2)
    npart, wsum, rs = [hood.to_callers(x.flatten(1), 'min') for x in sums]
    nr = len(e) - 1
    nt = nd * (nd + 1) // 2
    rs = rs.reshape(nc, nr, moment_sums(nd, vel is not None))
    o = 1 + nd
    first, second, reduced = rs[..., 1:o], _symmetric(rs[..., o:o + nt], nd), _symmetric(rs[..., o + nt:o + 2 * nt], nd)
    momentum = kinetic = angular = None
    if vel is not None:
        o += 2 * nt
        momentum, kinetic, angular = rs[..., o:o + nd], rs[..., o + nd], rs[..., o + nd + 1:]
    return MomentsResult(npart.reshape(nc, nr), wsum.reshape(nc, nr), rs[..., 0], first, second, reduced, momentum,
                         kinetic, angular, e, scale, nd)


def _cross(a, b):
    """a x b of (n, ndim) rows: (n, 3) in three dimensions, the (n, 1) scalar a_0 b_1 - a_1 b_0 in two"""
    if a.shape[1] == 3:
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)
    return (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).reshape(-1, 1)


def halo_shapes(pm, centres, pos, radius, mass=None, vel=None, centre_vel=None, reduced=False, G=1.0):
    """The shape, the velocity dispersion and the spin of the sources inside the sphere of `radius` about every centre: a
    ShapeResult.

    One ``radial_moments(pm, centres, pos, [0, 1], mass=mass, vel=vel, scale=radius)`` call; with M, first, second,
    reduced, momentum, kinetic and angular its sums of the one bin ``r < radius`` of a centre:
      offset            first / M: the centre of mass relative to the centre
      tensor            second / M - offset (x) offset: the second-moment tensor about the centre of mass; with
                        ``reduced=True`` reduced / M: the reduced tensor (every source weighted by 1 / r^2) about the
                        centre
      eigenvalues, axes those of ``torch.linalg.eigh`` on the device, descending; every axis has its component of
                        largest magnitude positive.  major = axes[:, 0]: the rows alignment_counts takes
      b_over_a, c_over_a   sqrt(eigenvalues[:, 1] / eigenvalues[:, 0]), sqrt(eigenvalues[:, 2] / eigenvalues[:, 0])
      triaxiality       (l_0 - l_1) / (l_0 - l_2), l the eigenvalues: 0 oblate, 1 prolate
      velocity          momentum / M less `centre_vel` ((nc, ndim) rows, e.g. CMVelocity; None: 0)
      sigma             sqrt(max(kinetic / M - |momentum / M|^2, 0) / ndim): the 1-d dispersion about the mean
      angular_momentum  angular - first x v_ref: the angular momentum about the centre of the motion relative to
                        v_ref.  The reference velocity v_ref is `centre_vel` where it is given and the mean velocity
                        momentum / M of the sources of the sphere otherwise
      spin              |J| / (sqrt(2) M V R), V = sqrt(G M / R), R the radius: the parameter of Bullock et al. 2001
                        (three dimensions)
    radius : a positive number, or (nc,) of them, e.g. ``so_masses(...).radius``.  A centre whose radius is nan (no
    crossing was found) has nan rows and costs nothing; any other radius that is not positive and finite raises
    ValueError.  A centre with fewer than ndim + 1 sources has nan rows as well (npart and mass are kept).
    """
    be = backend.get()
    nd = len(pm.Nmesh)
    dev = be.device
    f8 = torch.float64
    (c, cv), error = read_rows(pm, be, (('centres', centres, nd, None), ('centre_vel', centre_vel, nd, 0)))
    if error is None and cv is not None and vel is None:
        error = ValueError('centre_vel needs vel')
    nc = 0 if c is None else c.shape[0]
    R = None
    if error is None:
        try:
            if not isinstance(radius, torch.Tensor):
                radius = torch.from_numpy(numpy.array(radius, dtype='f8'))   # (not as_tensor: a Python float is a float32)
            R = radius.to(device=dev, dtype=f8).reshape(-1)
            R = R.expand(nc).clone() if R.numel() == 1 else R
            if R.numel() != nc:
                raise ValueError
        except (TypeError, ValueError, RuntimeError):
            error = ValueError('radius must be a number or one per centre')
    together(pm.comm, error)
    known = ~torch.isnan(R)
    # a centre without a radius takes the smallest of the others (it widens no search) and is masked afterwards
    fill = R[known].min() if bool(known.any()) else torch.tensor(2.0 ** -20 * min(box_of(pm)), dtype=f8, device=dev)
    mom = radial_moments(pm, c, pos, [0.0, 1.0], mass=mass, vel=vel, scale=torch.where(known, R, fill))
    npart, M = mom.npart[:, 0], mom.mass[:, 0]
    ok = known & (npart >= nd + 1) & (M != 0)
    nan = float('nan')
    safe = torch.where(ok, M, torch.ones_like(M))
    mask = lambda t: torch.where(ok.reshape((-1,) + (1,) * (t.dim() - 1)), t, torch.full_like(t, nan))
    offset = mom.first[:, 0] / safe[:, None]
    if reduced:
        tensor = mom.reduced[:, 0] / safe[:, None, None]
    else:
        tensor = mom.second[:, 0] / safe[:, None, None] - offset[:, :, None] * offset[:, None, :]
    eye = torch.eye(nd, dtype=f8, device=dev).expand(nc, nd, nd)
    vals, vecs = torch.linalg.eigh(torch.where(ok[:, None, None], tensor, eye))
    vals, axes = vals.flip(1), vecs.flip(2).transpose(1, 2)        # descending; axes[:, k] the k-th eigenvector
    big = axes.gather(2, axes.abs().argmax(dim=2, keepdim=True))
    axes = axes * torch.where(big < 0, -torch.ones_like(big), torch.ones_like(big))
    lead = torch.where(ok & (vals[:, 0] > 0), vals[:, 0], torch.ones_like(M))
    ratio = lambda k: torch.sqrt(torch.clamp(vals[:, k], min=0) / lead)
    out = dict(npart=npart, mass=M, offset=mask(offset), tensor=mask(tensor), eigenvalues=mask(vals), axes=mask(axes),
               major=mask(axes[:, 0]), b_over_a=mask(ratio(1)), c_over_a=None, triaxiality=None, velocity=None,
               sigma=None, angular_momentum=None, spin=None, radius=torch.where(known, R, torch.full_like(R, nan)),
               moments=mom, ndim=nd, reduced=bool(reduced))
    if nd == 3:
        out['c_over_a'] = mask(ratio(2))
        out['triaxiality'] = mask((vals[:, 0] - vals[:, 1]) / (vals[:, 0] - vals[:, 2]))
    if vel is not None:
        mean = mom.momentum[:, 0] / safe[:, None]
        vref = mean if cv is None else cv.to(f8)
        out['velocity'] = mask(mean if cv is None else mean - vref)
        out['sigma'] = mask(torch.sqrt(torch.clamp(mom.kinetic[:, 0] / safe - (mean * mean).sum(dim=1), min=0) / nd))
        J = mom.angular[:, 0] - _cross(mom.first[:, 0], vref)
        out['angular_momentum'] = mask(J)
        if nd == 3:
            Rs = torch.where(known, R, torch.ones_like(R))
            V = torch.sqrt(float(G) * safe.abs() / Rs)
            out['spin'] = mask(torch.sqrt((J * J).sum(dim=1)) / (numpy.sqrt(2.0) * safe * V * Rs))
    return ShapeResult(**out)


def ellipticity_from_shapes(shapes, los=2):
    """the (g1, g2) rows projected_alignment_counts takes, of the major axes of a three-dimensional ShapeResult"""
    return ellipticity_from_orientation(torch.nan_to_num(shapes.major), los=los)
