"""The host layer that the cell-grid statistics share: fof, paircount and the modules behind its
``_count``, threept, shortrange, knn and profiles.

Reading the arguments (``rows``, ``read_rows``, ``together``, ``refuse_not_finite``, ``within_reach``, ``box_of``), the
cell grid and the sort of one or two sets into it (``cell_grid``, ``cell_sort``, ``sorted_sets``), and the routing of
two sets of rows over the ranks (``Neighbourhood``; ``ghost_layout`` and ``row_limit`` for fof, which keeps a layout of
its own).  Nothing here launches a kernel of a statistic; this module imports none of theirs.
"""
import numpy
import torch

from . import _abi
from ._arrays import to_device

MAX_ROWS = _abi.PMX_FOF_MAX_ROWS
CELLS_PER_ROW = _abi.PMX_FOF_CELLS_PER_ROW
# ghosts travel a hair further than the search radius: a pair at exactly the radius across a block face must not depend
# on the rounding of the routing
HAIR = 1e-9


def together(comm, error):
    """raise `error` (None, or an exception) on every rank when any rank has one"""
    code = 0 if error is None else (1 if isinstance(error, TypeError) else 2)
    worst = int(comm.allreduce(code, op='max')) if comm.size > 1 else code
    if error is not None:
        raise error
    if worst:
        raise (TypeError if worst == 1 else ValueError)('another rank refused its arguments')


def allsum(comm, t):
    return t if comm.size == 1 else comm.allreduce(t)


def box_of(pm):
    """the sides of the periodic box, one float per axis of the mesh"""
    return [float(x) for x in numpy.broadcast_to(numpy.asarray(pm.BoxSize, dtype='f8'), (len(pm.Nmesh),))]


def within_reach(b, box):
    """whether the search radius `b` is finite, positive and at most half the shortest side: a row then has one image
    of every other within b"""
    return bool(numpy.isfinite(b) and b > 0 and 2 * b <= min(box))


def rows(pm, be, pos, what='pos', ncol=None, n=None):
    """(tensor or None, error or None): `pos` as an (n, ncol) float tensor on the device"""
    ncol = len(pm.Nmesh) if ncol is None else ncol
    try:
        t, _ = to_device(pos, be.device, what)
    except TypeError as e:
        return None, e
    if ncol == 1 and t.dim() == 1:
        t = t.reshape(-1, 1)
    if t.dim() != 2 or t.shape[1] != ncol:
        return None, ValueError('%s must have the shape (n, %d), not %s' % (what, ncol, tuple(t.shape)))
    if n is not None and t.shape[0] != n:
        return None, ValueError('%s must have %d rows, not %d' % (what, n, t.shape[0]))
    return t, None


def read_rows(pm, be, wanted, error=None):
    """(tensors, error) of the entries (name, value, columns, the earlier entry whose row count it must have or None) of
    `wanted`: ``rows`` of every value that is not None, up to the first error, `error` itself if there is one already"""
    got = []
    for what, x, ncol, of in wanted:
        t = None
        if x is not None and error is None:
            t, error = rows(pm, be, x, what, ncol, None if of is None else got[of].shape[0])
        got.append(t)
    return got, error


def refuse_not_finite(comm, what, *tensors, entry='a coordinate'):
    """ValueError on every rank, with their number over all ranks, when rows of the `tensors` (None: no rows) are not
    finite; `what` names the sets in the message"""
    nbad = sum(int((~torch.isfinite(t)).any(dim=1).sum()) for t in tensors if t is not None)
    if comm.size > 1:
        nbad = int(comm.allreduce(nbad))
    if nbad:
        raise ValueError('%d rows of %s have %s that is not finite' % (nbad, what, entry))


def cell_grid(n, b, box, lo=None, hi=None):
    """The cell grid of `n` rows for the linking length `b`: (ncell, origin, inv_side, periodic mask), per axis.

    Without a block (one rank) every axis is periodic: origin 0, extent L_d.  With the block [lo, hi) of a rank, an axis
    where the block plus 2 b covers the box is periodic as well; otherwise it is open, from lo_d - b over hi_d - lo_d +
    2 b.  The cells have a side >= b on every axis, and there are at most max(1, PMX_FOF_CELLS_PER_ROW * n) of them:
    the side grows to about the mean separation when b is smaller."""
    nd = len(box)
    box = numpy.asarray(box, dtype='f8')
    origin, extent, mask = numpy.zeros(nd), box.copy(), 0
    for d in range(nd):
        if lo is not None and (hi[d] - lo[d]) + 2 * b < box[d]:
            origin[d] = (lo[d] - b) % box[d]
            extent[d] = (hi[d] - lo[d]) + 2 * b
        else:
            mask |= _abi.PMX_FOF_PERIODIC_X << d
    most = numpy.maximum(numpy.floor(extent / b), 1)
    most = numpy.where((extent / most < b) & (most > 1), most - 1, most)
    cap = min(max(1, CELLS_PER_ROW * int(n)), MAX_ROWS)
    ncell = most.copy()
    side = (numpy.prod(extent) / cap) ** (1.0 / nd)
    while numpy.prod(ncell) > cap:
        ncell = numpy.clip(numpy.floor(extent / side), 1, most)
        side *= 1.05
    ncell = [int(c) for c in ncell]
    return ncell, [float(o) for o in origin], [c / float(e) for c, e in zip(ncell, extent)], mask


def cell_sort(be, pos, grid, box):
    """pass 1 on the (n, ndim) rows: (wpos, cell_of, cell_start, order, spos, rows that are not finite)"""
    ncell, origin, inv_side, mask = grid
    n, nd = pos.shape
    dev = pos.device
    ncells = int(numpy.prod(ncell))
    wpos = torch.empty((n, nd), dtype=torch.float64, device=dev)
    spos = torch.empty((n, nd), dtype=torch.float64, device=dev)
    cell_of = torch.empty(n, dtype=torch.int32, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(ncells, dtype=torch.int32, device=dev)
    flagged = torch.zeros(1, dtype=torch.int64, device=dev)
    be.fof_cells(pos, box, origin, inv_side, ncell, mask, wpos, cell_of, counts, flagged)
    cell_start = torch.zeros(ncells + 1, dtype=torch.int32, device=dev)
    cell_start[1:] = torch.cumsum(counts, 0)
    counts.zero_()
    be.fof_fill(wpos, cell_of, cell_start, counts, order, spos)
    return wpos, cell_of, cell_start, order, spos, flagged


def sorted_sets(be, pos1, pos2, grid, box):
    """The primaries `pos1` and the secondaries `pos2` sorted into the cells of `grid`, as the entries take them:
    (spos1, order1, cell_of1, spos2, order2, cell_start2).  pos2 None: the secondaries are the primaries, one sort
    serves both and spos2 and order2 are spos1 and order1 themselves."""
    _, cell_of1, cell_start1, order1, spos1, _ = cell_sort(be, pos1, grid, box)
    if pos2 is None:
        return spos1, order1, cell_of1, spos1, order1, cell_start1
    _, _, cell_start2, order2, spos2, _ = cell_sort(be, pos2, grid, box)
    return spos1, order1, cell_of1, spos2, order2, cell_start2


def block(pm):
    """the low and high corners of this rank's real-field block in box units, or (None, None): one periodic grid"""
    region = pm.domain.primary_region
    if pm.comm.size == 1 or region is None or len(region['start']) != 1:
        return None, None
    h = numpy.asarray(pm.BoxSize, dtype='f8') / numpy.asarray(pm.Nmesh, dtype='f8')
    return region['start'][0] * h, region['end'][0] * h


def ghost_layout(pm, pos, radius):
    """the layout that delivers every row of `pos` to every rank whose block it lies within `radius` (and HAIR) of"""
    smoothing = radius * numpy.asarray(pm.Nmesh, dtype='f8') / numpy.asarray(box_of(pm)) * (1 + HAIR)
    return pm.decompose(pos, smoothing=smoothing)


def row_limit(comm, most, ghosts):
    """ValueError on every rank when a rank would sort more than MAX_ROWS rows: slots and parents are 32-bit"""
    text = 'more than 2^31 - 1 rows%s on one rank' % (' and ghosts' if ghosts else '')
    together(comm, ValueError(text) if most > MAX_ROWS else None)


class Neighbourhood(object):
    """Where the rows of one collective call meet: every primary (a row of `pos1`) on one rank, its owner, together
    with every source (a row of `pos2`; None: of pos1) within `radius` of it.  Made once per call, by all ranks.

    One rank is the owner of everything, and nothing travels.  On several, the primaries go to the rank whose block
    holds them (``pm.decompose`` without ghosts) and the sources to every rank whose block they lie within the radius
    of (``ghost_layout``); every ordered pair within the radius is then seen on exactly one rank.  ``grid`` is the cell
    grid of the rows a rank then holds, over its block where there are several, ``box`` the sides of the box, and
    ``same`` says that the sources are the primaries' own rows in their own order (the auto form on one rank): one sort
    serves both sets.  More than MAX_ROWS rows on a rank raise ValueError on all of them.

    Every exchange drops the layout's memo afterwards: a layout remembers its last exchange by the address, version,
    shape, stride and dtype of the tensor, and the tensors of a rank that holds no rows can share all five."""

    def __init__(self, pm, radius, pos1, pos2=None):
        self.comm = pm.comm
        self.box = box_of(pm)
        src = pos1 if pos2 is None else pos2
        self.same = pos2 is None and self.comm.size == 1
        if self.comm.size == 1:
            self.own = self.ghosts = None
            most = max(pos1.shape[0], src.shape[0])
            lo = hi = None
        else:
            self.own = pm.decompose(pos1, smoothing=0)
            self.ghosts = ghost_layout(pm, src, radius)
            most = max(self.own.recvlength, self.ghosts.recvlength)
            lo, hi = block(pm)
        row_limit(self.comm, most, ghosts=self.own is not None)
        self.grid = cell_grid(most, radius, self.box, lo, hi)

    @staticmethod
    def _bring(layout, tensors):
        if len(tensors) == 1 and (layout is None or tensors[0] is None):
            return tensors[0]
        if layout is None:
            return tensors
        out = layout.exchange(*tensors)
        layout.forget()
        return out

    def to_owners(self, *tensors):
        """per-primary tensors on the owners of the primaries; one tensor: it (None stays None); several: a tuple, and
        they travel in one exchange"""
        return self._bring(self.own, tensors)

    def to_sources(self, *tensors):
        """the same for per-source tensors: on every rank that holds a copy of the source"""
        return self._bring(self.ghosts, tensors)

    def to_callers(self, t, mode):
        """a per-primary result of the owners (None stays None) back in the callers' rows; every primary has exactly one
        owner, so `mode` ('sum', 'min') only says how the one copy is combined with the identity"""
        return t if t is None or self.own is None else self.own.gather(t, mode=mode)

    def allsum(self, t):
        return allsum(self.comm, t)
