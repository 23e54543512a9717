"""Friends-of-friends groups of particles and a halo catalogue, made on the device.

What nbodykit's ``FOF`` and ``FOF.find_features`` do on the host (a kd-tree over the rows, a merge loop over the
ranks, numpy bincounts for the centres) as six entries of the C ABI (csrc/pmx_fof.hip, include/pmesh_amd.h): the rows
of ``examples/nbody.py`` or ``lognormal_catalog`` become halos without leaving HBM.

The rule (normative; include/pmesh_amd.h restates it next to the entry points).

1. Positions are ``(n, ndim)`` rows, ``ndim = len(pm.Nmesh)`` = 1, 2 or 3, float64 or float32 (widened exactly); all
   arithmetic is in double.
2. Rows are first wrapped into ``[0, L_d)``: ``w = x - L * floor(x / L)``, plus L where that is negative, 0 where it
   is not below L.
3. Two rows are friends when ``sum_d dx_d^2 <= b^2``, ``dx_d`` the minimum-image difference ``dx_d -= L_d * rint(dx_d
   / L_d)`` of the wrapped rows, the sum accumulated in the order d = 0, 1, 2.
4. ``b``, the linking length in box units, is finite, positive and ``2 b <= min_d L_d``; otherwise ValueError on
   every rank.
5. A group is a connected component of the friendship graph over the rows of all ranks.  The canonical label of a row
   is ``minid``, the smallest global row index of its group; the global index of a row is its local index plus the
   number of rows on the lower ranks.  ``minid`` depends on no decomposition and on no order in which lanes run: two
   calls give identical arrays.

    from pmesh_amd.fof import fof, fof_catalog
    res = fof(pm, pos, 0.2, nmin=20, absolute=False)
    res.minid, res.labels, res.ngroups, res.length, res.iterations
    cat = fof_catalog(pm, pos, res, mass=None, vel=vel)
    cat.Length, cat.Mass, cat.CMPosition, cat.CMVelocity

On several ranks (nbodykit's merge loop): the ghost layout of DESIGN.md §5.7.0 (``_cells.ghost_layout``) delivers every
row to the ranks whose block it lies within b of; every rank groups its own rows and ghosts; then the labels are
gathered back to the owners with a minimum over the copies (``Layout.gather(mode='min')``), exchanged out again and
minimised over the local components, until no label changes on any rank.  Labels only decrease, so this ends.
"""
import numpy
import torch

from . import _abi, backend
from ._cells import (allsum, block, box_of, cell_grid, cell_sort, ghost_layout, row_limit, rows, together,
                     within_reach)


class FOFResult(object):
    """The groups of one rank's rows: ``minid`` (int64 device tensor, one per local row), ``labels`` (int64; 0 for rows
    whose group has fewer than nmin members, otherwise 1 .. ngroups by group length descending, ties by ascending
    minid), ``ngroups`` (over all ranks), ``length`` (int64 device tensor of ngroups + 1 entries, entry 0 the number of
    unlabelled rows), ``iterations`` (the merge rounds over the ranks), ``linking_length`` (in box units), ``csize``
    and ``offset`` (the global index of this rank's first row)."""

    def __init__(self, minid, labels, ngroups, length, iterations, linking_length, csize, offset):
        self.minid, self.labels, self.ngroups, self.length = minid, labels, ngroups, length
        self.iterations, self.linking_length, self.csize, self.offset = iterations, linking_length, csize, offset


class FOFCatalog(object):
    """The halos, identical on every rank, row 0 unused: ``Length`` (int64), ``Mass``, ``CMPosition`` and
    ``CMVelocity`` (float64 device tensors of ngroups + 1 rows)."""

    def __init__(self, Length, Mass, CMPosition, CMVelocity):
        self.Length, self.Mass, self.CMPosition, self.CMVelocity = Length, Mass, CMPosition, CMVelocity


def local_groups(be, pos, b, box, grid):
    """passes 1 to 3 on the rows of one rank: (root of every row: int32, rows that are not finite: device int64)"""
    wpos, cell_of, cell_start, order, spos, flagged = cell_sort(be, pos, grid, box)
    del wpos
    parent = torch.empty(pos.shape[0], dtype=torch.int32, device=pos.device)
    be.fof_link(spos, order, cell_of, cell_start, grid[0], grid[3], box, b * b, parent)
    be.fof_flatten(parent)
    return parent, flagged


def fof(pm, pos, linking_length, nmin=20, absolute=True):
    """The friends-of-friends groups of the rows `pos` by the rule of the module docstring: an FOFResult.

    pm : ParticleMesh of 1, 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos : (n, ndim) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    linking_length : in box units; with ``absolute=False`` in units of the mean separation ``(V / csize)^(1 / ndim)``,
        as in nbodykit.
    nmin : groups of fewer rows get the label 0.

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them: parents are
    32-bit.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('friends-of-friends on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    box = box_of(pm)
    pos, error = rows(pm, be, pos)
    if error is None and not (int(nmin) == nmin and nmin >= 1):
        error = ValueError('nmin must be a positive integer')
    together(comm, error)
    n = pos.shape[0]
    sizes = [int(s) for s in comm.allgather(n)] if comm.size > 1 else [n]
    csize, offset = sum(sizes), sum(sizes[:comm.rank])
    b = float(linking_length)
    if not absolute and csize > 0:
        b *= (float(numpy.prod(box)) / csize) ** (1.0 / nd)
    if not within_reach(b, box):
        raise ValueError('the linking length must be finite, positive and at most half the shortest box side: %r' % b)
    dev = be.device
    gid = torch.arange(offset, offset + n, dtype=torch.int64, device=dev)
    iterations = 0
    if comm.size == 1:
        row_limit(comm, n, ghosts=False)
        root, flagged = local_groups(be, pos, b, box, cell_grid(n, b, box))
        minid = gid
        be.fof_minlabel(root, minid, torch.empty_like(minid), torch.zeros(1, dtype=torch.int64, device=dev))
        nbad = int(flagged.cpu()[0])
    else:
        layout = ghost_layout(pm, pos, b)
        row_limit(comm, layout.recvlength, ghosts=True)
        rpos, val = layout.exchange(pos, gid)
        lo, hi = block(pm)
        root, flagged = local_groups(be, rpos, b, box, cell_grid(rpos.shape[0], b, box, lo, hi))
        work = torch.empty_like(val)
        changed = torch.zeros(1, dtype=torch.int64, device=dev)
        be.fof_minlabel(root, val, work, changed)
        nbad = int(comm.allreduce(int(flagged.cpu()[0])))
        while not nbad:
            iterations += 1
            layout.forget()
            val = layout.exchange(layout.gather(val, mode='min')).clone()
            changed.zero_()
            be.fof_minlabel(root, val, work, changed)
            if int(comm.allreduce(int(changed.cpu()[0]))) == 0:
                break
        minid = layout.gather(val, mode='min')
    if nbad:
        raise ValueError('%d rows of pos have a coordinate that is not finite' % nbad)
    labels, ngroups, length = _number(comm, minid, int(nmin), csize)
    return FOFResult(minid, labels, ngroups, length, iterations, b, csize, offset)


def _number(comm, minid, nmin, csize):
    """labels of the local rows, ngroups and length from the minid of the owners' rows: the groups of at least nmin
    rows by length descending, ties by ascending minid (host-side plumbing: one unique, one allgather, one sort)"""
    dev = minid.device
    ids, counts = torch.unique(minid, return_counts=True)
    ids, counts = ids.cpu().numpy(), counts.cpu().numpy()
    if comm.size > 1:
        parts = comm.allgather((ids, counts))
        allids = numpy.concatenate([p[0] for p in parts])
        ids, inverse = numpy.unique(allids, return_inverse=True)
        counts = numpy.bincount(inverse, weights=numpy.concatenate([p[1] for p in parts]),
                                minlength=len(ids)).astype('i8')
    keep = counts >= nmin
    order = numpy.lexsort((ids[keep], -counts[keep]))
    ngroups = int(keep.sum())
    label_of = numpy.zeros(len(ids) + 1, dtype='i8')
    label_of[numpy.flatnonzero(keep)[order]] = numpy.arange(1, ngroups + 1)
    length = numpy.empty(ngroups + 1, dtype='i8')
    length[1:] = counts[keep][order]
    length[0] = csize - length[1:].sum()
    if len(ids):
        where = torch.searchsorted(torch.from_numpy(ids).to(dev), minid)
        labels = torch.from_numpy(label_of).to(dev)[where]
    else:
        labels = torch.zeros_like(minid)
    return labels, ngroups, torch.from_numpy(length).to(dev)


def _wrapped(x, box):
    """rule 2 on the columns of x"""
    w = x - box * torch.floor(x / box)
    w = torch.where(w < 0, w + box, w)
    return torch.where(w < box, w, torch.zeros_like(w))


def fof_catalog(pm, pos, result, mass=None, vel=None):
    """The halo catalogue of the FOFResult `result` of the same `pos`: an FOFCatalog.

    mass : (n,) float rows, or None for unit masses.  vel : (n, ndim) float rows, or None (CMVelocity is then zero).

    CMPosition follows nbodykit's periodic rule: the displacements from a reference member — the row whose global index
    is the group's minid — are wrapped to the minimum image, mass-weighted and averaged; the result is added to the
    reference and wrapped into the box.  CMVelocity is the mass-weighted mean of vel, Mass the sum of mass, Length
    ``result.length``.  The sums are double sums in an order that depends on the atomics: the last bits may differ from
    run to run.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('friends-of-friends on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    error = None if isinstance(result, FOFResult) else TypeError('result must be the FOFResult of fof(pm, pos, ...)')
    n = result.labels.shape[0] if error is None else None
    cols = []
    for what, x, ncol in (('pos', pos, nd), ('mass', mass, 1), ('vel', vel, nd)):
        t = None
        if x is not None and error is None:
            t, error = rows(pm, be, x, what, ncol, n)
        cols.append(t)
    together(comm, error)
    pos, mass, vel = cols
    dev = be.device
    box = box_of(pm)
    boxt = torch.tensor(box, dtype=torch.float64, device=dev)
    ng = result.ngroups
    # the reference member of every group: the row whose global index is the group's minid, on the rank that owns it
    ref = torch.zeros((ng + 1, nd), dtype=torch.float64, device=dev)
    gid = torch.arange(result.offset, result.offset + n, dtype=torch.int64, device=dev)
    sel = torch.nonzero((result.labels > 0) & (gid == result.minid)).reshape(-1)
    ref[result.labels[sel]] = pos[sel].to(torch.float64)
    ref = allsum(comm, ref)
    out = torch.zeros((ng + 1, 1 + 2 * nd), dtype=torch.float64, device=dev)
    be.fof_group_sums(pos, result.labels, mass, vel, ref, box, out)
    out = allsum(comm, out)
    total = out[:, 0:1].clone()
    total[0] = 1.0
    cm = _wrapped(_wrapped(ref, boxt) + out[:, 1:1 + nd] / total, boxt)
    cv = out[:, 1 + nd:] / total
    cm[0] = 0
    cv[0] = 0
    Mass = out[:, 0].clone()
    Mass[0] = 0
    return FOFCatalog(result.length, Mass, cm, cv)
