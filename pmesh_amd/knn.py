"""The k nearest neighbours of particles, their distances and the densities made of them, on the device.

What callers do today with a kd-tree on the host: nbodykit's ``KDDensity`` (a density proxy from the distance to a
neighbour of fixed rank), MP-Gadget's density loop (the smoothing length that encloses a fixed number of neighbours:
the per-particle ``hsml`` of ``pm.paint``), and the nearest-neighbour distribution statistics (kNN-CDF) of a catalogue
against query points.  The other particle modules answer "what lies within a radius known in advance"; this one answers
"how far is the k-th nearest row": a selection, as one entry of the C ABI (csrc/pmx_knn.hip, include/pmesh_amd.h:
pmx_knn) on the cell grid of pmesh_amd.fof.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Rows.  ``pos`` (primaries) and ``pos2`` (sources; None: the primaries themselves) are ``(n, ndim)`` rows, ``ndim =
   len(pm.Nmesh)`` = 1, 2 or 3, float64 or float32 (widened exactly).  Rows are wrapped by rule 2 of pmesh_amd.fof;
   ``dx_d = x_i,d - x_j,d`` is the minimum image of the wrapped rows; ``r2 = sum_d dx_d^2``, accumulated in the order
   d = 0, 1, 2.  All arithmetic is in double and every operation is rounded once.
2. Candidates.  Source j is a candidate of primary i when ``r2 < rmax2``, ``rmax2 = rmax * rmax`` formed once on the
   host.  ``rmax`` is finite and positive with ``2 rmax <= min_d L_d``; its default is ``min_d L_d / 2``.  No square
   root decides anything.
3. Result, cross form.  ``dist2[i, :]`` holds the k smallest candidate ``r2`` of row i, ascending, as float64; columns
   with no candidate hold ``+inf``.  The multiset of the k smallest values is unique, so ``dist2`` is defined bit for
   bit and depends on no decomposition, launch or search schedule.  ``index[i, c]`` (int64) is the global row index of
   a source whose ``r2`` to row i equals ``dist2[i, c]``, or ``-1`` where ``dist2`` is inf.  The indices of one row are
   distinct.  Among sources tied in ``r2``, which one is named is unspecified: the indices are witnesses, not a
   canonical order.  The global index of a row is its local index plus the number of rows on the lower ranks (fof rule
   5).  ``found[i]`` is the number of finite columns.
4. Result, auto form (``pos2 is None``).  The cross form of ``pos`` against itself with ``k + 1``, with one column
   removed per row: the column whose index is the row's own global index if it is present, otherwise the last column.
   The row itself has ``r2 == 0`` exactly, so the values are those of "every other row, coincident ones included at
   r2 = 0".  Identity is the global index, not the position.
5. Limits.  ``1 <= k <= PMX_KNN_MAX_K`` (64) in the cross form, ``k <= 63`` in the auto form.  Rows that are not finite
   raise ValueError with their number, and so does a rank past the row limit of DESIGN.md §5.7.0.  Every argument
   error is raised on all ranks together.

    from pmesh_amd.knn import knn, knn_density, knn_cdf
    res = knn(pm, pos, 32)                        # res.dist2, res.dist, res.index, res.found, res.rounds
    rho = knn_density(pm, pos, k=32)              # k / V_ndim(d_k)
    N, nquery = knn_cdf(pm, data, query, [1, 2, 4, 8], redges)

The search is by growing radius.  One launch of the entry is a fixed-radius top-k over the 3^ndim neighbouring cells
of a grid of side >= R; it also counts the sources inside R exactly.  Round t uses ``R_t = min(R_0 2^t, rmax)``, ``R_0
= first_radius(...)`` the radius of the ball that holds ``2 (k + 1)`` sources at the mean density over all ranks.  A row
whose count reaches k' (k, or k + 1 in the auto form) is resolved: its k' nearest all lie inside ``R_t``.  Resolved rows
are not searched again; the others go to the next round on a new grid; the round with ``R_t == rmax`` is the last, and
its rows keep what they have, inf-padded.  One host synchronisation per round counts the unresolved rows (with ranks,
one allreduce).  By rule 3 the result depends neither on ``R_0`` nor on the schedule.

Host, per round: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) of the unresolved primaries and all sources
with the radius ``R_t``.  On several ranks an int64 column of the sources' global indices travels with them; the
kernel's local indices are mapped through that column on the device, and the rows return to their callers with the mode
'min' (every primary has one owner).
"""
import numpy
import torch

from . import _abi, backend
from ._cells import Neighbourhood, box_of, read_rows, refuse_not_finite, rows, sorted_sets, together, within_reach

MAX_K = _abi.PMX_KNN_MAX_K


class KNNResult(object):
    """The neighbours of one rank's rows, device tensors in the caller's row order: ``dist2`` (float64, (n, k)), ``dist``
    (its square root), ``index`` (int64 (n, k), global source rows; None with ``index=False``), ``found`` (int64 (n,),
    the finite columns); and ``k``, ``rmax``, ``rounds`` (the search rounds this call took, the same on every rank)."""

    def __init__(self, dist2, index, found, k, rmax, rounds):
        self.dist2, self.index, self.found, self.k, self.rmax, self.rounds = dist2, index, found, k, rmax, rounds

    @property
    def dist(self):
        return torch.sqrt(self.dist2)


def ball_volume(r, ndim):
    """V_ndim(r): 2 r, pi r^2 or 4/3 pi r^3 (r a number, an array or a tensor)"""
    if ndim == 1:
        return 2.0 * r
    if ndim == 2:
        return numpy.pi * (r * r)
    return 4.0 / 3.0 * numpy.pi * (r * r * r)


def first_radius(n2_total, k, box):
    """R_0: the radius of the ndim-ball that holds 2 (k + 1) sources at the mean density of `n2_total` sources in the
    box (inf without sources)"""
    nd = len(box)
    if n2_total <= 0:
        return numpy.inf
    vol = 2.0 * (k + 1) * float(numpy.prod(numpy.asarray(box, dtype='f8'))) / float(n2_total)
    if nd == 1:
        return vol / 2.0
    if nd == 2:
        return float(numpy.sqrt(vol / numpy.pi))
    return float((3.0 * vol / (4.0 * numpy.pi)) ** (1.0 / 3.0))


def local_knn(be, pos1, pos2, grid, box, r2max, k, index=True):
    """One launch on the rows of one rank on the cell grid `grid` (of _cells.cell_grid, its cells of a side >= the
    radius): the k smallest r2 < r2max of every row of `pos1` among the rows of `pos2` (None: pos1 itself, the row
    included).  Returns (dist2 (n1, k) float64, index (n1, k) int32 local rows of pos2 or None, count (n1,) int64: the
    sources with r2 < r2max, not capped) in the row order of pos1."""
    dev = pos1.device
    n1 = pos1.shape[0]
    dist2 = torch.empty((n1, k), dtype=torch.float64, device=dev)
    idx = torch.empty((n1, k), dtype=torch.int32, device=dev) if index else None
    count = torch.empty(n1, dtype=torch.int64, device=dev)
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, pos1, pos2, grid, box)
    be.knn(spos1, order1, cell_of1, spos2, order2, cell_start2, grid[0], grid[3], box, r2max, k, dist2, idx, count)
    return dist2, idx, count


def _count(comm, n):
    return int(comm.allreduce(int(n))) if comm.size > 1 else int(n)


def _arguments(pm, be, pos, pos2, k, rmax):
    """(box, pos, pos2, k, rmax, error) of knn()"""
    nd = len(pm.Nmesh)
    box = box_of(pm)
    error = None
    auto = pos2 is None
    try:
        kk = int(k)
        if kk != k:
            raise ValueError
    except (TypeError, ValueError):
        kk, error = None, ValueError('k must be an integer, not %r' % (k,))
    most = MAX_K - 1 if auto else MAX_K
    if error is None and not 1 <= kk <= most:
        error = ValueError('k must be in 1 .. %d (PMX_KNN_MAX_K%s), not %d' % (most, ' - 1: the auto form' if auto else '',
                                                                               kk))
    rm = None
    if error is None:
        try:
            rm = min(box) / 2 if rmax is None else float(rmax)
        except (TypeError, ValueError):
            rm = numpy.nan
        if not within_reach(rm, box):
            error = ValueError('rmax must be finite, positive and at most half the shortest box side: %r' % (rmax,))
    (pos, pos2), error = read_rows(pm, be, (('pos', pos, nd, None), ('pos2', pos2, nd, None)), error)
    return box, pos, pos2, kk, rm, error


def knn(pm, pos, k, pos2=None, rmax=None, index=True):
    """The k nearest sources of every row of `pos` within `rmax` by the rule of the module docstring: a KNNResult.

    pm : ParticleMesh of 1, 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos : (n, ndim) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    k : the number of neighbours, 1 .. 64 (63 in the auto form).
    pos2 : the rows of the sources, or None: `pos` itself, every row without itself (rule 4).
    rmax : sources at rmax and beyond are no neighbours; the default is half the shortest box side.
    index : False leaves ``index`` None (the auto form still forms it: identity is the index).

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('nearest neighbours on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    box, pos, pos2, k, rmax, error = _arguments(pm, be, pos, pos2, k, rmax)
    together(comm, error)
    auto = pos2 is None
    src = pos if auto else pos2
    refuse_not_finite(comm, 'pos and pos2', pos, pos2)
    dev = be.device
    n1, n2 = pos.shape[0], src.shape[0]
    kk = k + 1 if auto else k
    want_index = bool(index) or auto
    if comm.size > 1:
        sizes = [int(s) for s in comm.allgather(n2)]
        n2_total, offset2 = sum(sizes), sum(sizes[:comm.rank])
    else:
        n2_total, offset2 = n2, 0
    gid2 = torch.arange(offset2, offset2 + n2, dtype=torch.int64, device=dev)
    rmax2 = rmax * rmax
    r0 = first_radius(n2_total, k, box)
    dist2 = torch.full((n1, kk), float('inf'), dtype=torch.float64, device=dev)
    idx = torch.full((n1, kk), -1, dtype=torch.int64, device=dev) if want_index else None
    todo = None                                  # the local rows still to search: None for all of them
    rounds = 0
    while True:
        radius = r0 * 2.0 ** rounds
        last = not radius < rmax
        radius, r2 = (rmax, rmax2) if last else (radius, radius * radius)
        p1 = pos if todo is None else pos[todo]
        hood = Neighbourhood(pm, radius, p1, None if auto and todo is None else src)
        q1 = hood.to_owners(p1)
        q2, g2 = hood.to_sources(src, gid2)
        d, ix, cnt = local_knn(be, q1, None if hood.same else q2, hood.grid, box, r2, kk, want_index)
        d, cnt = hood.to_callers(d, 'min'), hood.to_callers(cnt, 'min')
        if want_index:
            ix = ix.to(torch.int64)
            if comm.size > 1:
                # the kernel's rows of q2 are not the sources' global rows
                ix = torch.where(ix >= 0, g2[ix.clamp(min=0)] if g2.numel() else ix, torch.full_like(ix, -1))
            ix = hood.to_callers(ix, 'min')
        # (the rows that are not resolved are written again in a later round)
        if todo is None:
            dist2 = d
            idx = ix if want_index else None
            left = torch.nonzero(cnt < kk).reshape(-1)
        else:
            dist2[todo] = d
            if want_index:
                idx[todo] = ix
            left = todo[cnt < kk]
        rounds += 1
        if last or _count(comm, left.numel()) == 0:
            break
        todo = left
    if auto:
        # rule 4: drop the column that names the row itself, or the last one
        offset1 = offset2
        me = torch.arange(offset1, offset1 + n1, dtype=torch.int64, device=dev).reshape(-1, 1)
        own_col = idx == me
        drop = torch.where(own_col.any(dim=1), own_col.to(torch.int8).argmax(dim=1),
                           torch.full((n1,), k, dtype=torch.int64, device=dev))
        keep = torch.arange(kk, device=dev).reshape(1, -1) != drop.reshape(-1, 1)
        dist2 = dist2[keep].reshape(n1, k)
        idx = idx[keep].reshape(n1, k)
    found = torch.isfinite(dist2).sum(dim=1)
    return KNNResult(dist2, idx if index else None, found, k, rmax, rounds)


def knn_density(pm, pos, k=32, pos2=None, mass2=None, rmax=None):
    """The density estimate ``rho_i = M_i / V_ndim(d_k)`` of every row of `pos`: an (n,) float64 device tensor.

    ``d_k = sqrt(dist2[:, k - 1])`` is the distance to the k-th nearest source of knn(pm, pos, k, pos2, rmax);
    ``V_ndim(r)`` is 2 r, pi r^2 or 4/3 pi r^3; ``M_i`` is k, or with `mass2` the sum of the masses of the k sources
    that ``index`` names.  mass2 : (n2,) float rows, the masses of the sources in this rank's row order (of `pos2`, or
    of `pos` where pos2 is None); on several ranks they are gathered to every rank once.  ``rho_i`` is 0 where fewer
    than k sources lie within rmax, and inf where the k nearest coincide with the row (d_k = 0).

    nbodykit's ``KDDensity`` reports a proxy proportional to ``d^-ndim`` of a neighbour of fixed rank, with an
    unspecified scale; without masses ``rho`` is ``k / V_ndim(1)`` times ``d_k^-ndim``: the same proxy with the scale
    of a number density and the rank a parameter.

    As a smoothing length for ``pm.paint(pos, hsml=...)``: hsml is dimensionless and multiplies the support of the
    window, its full width in cells (window.py; csrc/pmx_window.hip: ``support * hsml``).  A window that reaches d_k on
    either side of the particle along axis d has ``hsml = 2 d_k Nmesh_d / (BoxSize_d support)``; there is one hsml per
    particle, so on a mesh whose cells are not cubes one axis has to be chosen.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('nearest neighbours on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    error = m = None
    if mass2 is not None:
        src, error = rows(pm, be, pos if pos2 is None else pos2, 'pos' if pos2 is None else 'pos2', nd)
        if error is None:
            m, error = rows(pm, be, mass2, 'mass2', 1, src.shape[0])
    together(comm, error)
    res = knn(pm, pos, k, pos2=pos2, rmax=rmax, index=mass2 is not None)
    if m is None:
        total = float(res.k)
    else:
        m = m.reshape(-1).to(torch.float64)
        if comm.size > 1:
            parts = comm.allgather(m.cpu().numpy())
            m = torch.from_numpy(numpy.concatenate(parts)).to(be.device)
        if m.numel():
            total = torch.where(res.index >= 0, m[res.index.clamp(min=0)], torch.zeros_like(res.dist2)).sum(dim=1)
        else:
            total = torch.zeros(res.dist2.shape[0], dtype=torch.float64, device=be.device)
    dk = torch.sqrt(res.dist2[:, res.k - 1])
    rho = total / ball_volume(dk, nd)
    return torch.where(res.found >= res.k, rho, torch.zeros_like(rho))


def knn_cdf(pm, data, query, ks, redges, rmax=None):
    """The cumulative nearest-neighbour counts of the rows `query` against the rows `data`: ``(N, nquery)``, N an int64
    numpy array of the shape (len(ks), len(redges)) with ``N[a, b]`` the number of query rows whose ks[a]-th nearest
    data row has ``dist2 < redges[b]^2``, summed over the ranks, and nquery the number of query rows of all ranks: N /
    nquery is the kNN-CDF.  The counts are exact: the squared edges are formed on the host, and no square root is taken.

    ks : integers in 1 .. 64.  redges : finite, not negative, not decreasing, in box units.  rmax : the radius of the
    search, at least redges[-1], which is its default.  One cross knn with k = max(ks) serves all of it."""
    comm = pm.comm
    error = None
    e = numpy.atleast_1d(numpy.asarray(redges, dtype='f8'))
    try:
        kl = [int(a) for a in ks]
        if len(kl) == 0 or any(a != b for a, b in zip(kl, ks)) or min(kl) < 1 or max(kl) > MAX_K:
            raise ValueError
    except (TypeError, ValueError):
        error = ValueError('ks must be integers in 1 .. %d, at least one' % MAX_K)
    if error is None and (e.ndim != 1 or len(e) == 0 or not numpy.isfinite(e).all() or (e < 0).any()
                          or (numpy.diff(e) < 0).any() or not e[-1] > 0):
        error = ValueError('redges must be finite, not negative and not decreasing, the last one positive')
    if error is None and rmax is not None and not float(rmax) >= e[-1]:
        error = ValueError('rmax must be at least redges[-1]')
    together(comm, error)
    res = knn(pm, query, max(kl), pos2=data, rmax=float(e[-1]) if rmax is None else rmax, index=False)
    e2 = torch.from_numpy(e * e).to(res.dist2.device)
    cols = res.dist2[:, torch.tensor([a - 1 for a in kl], dtype=torch.int64, device=res.dist2.device)]
    counts = (cols.unsqueeze(2) < e2.reshape(1, 1, -1)).sum(dim=0).cpu().numpy().astype('i8')
    nquery = res.dist2.shape[0]
    if comm.size > 1:
        counts = numpy.asarray(comm.allreduce(counts))
        nquery = int(comm.allreduce(nquery))
    return counts, nquery
