"""Binned pair counts of particles and the two-point function from them, made on the device.

What nbodykit's ``SimulationBoxPairCount`` and ``SimulationBox2PCF`` do on the host (Corrfunc over the rows copied over
PCIe) as one entry of the C ABI (csrc/pmx_pairs.hip, include/pmesh_amd.h: pmx_pair_counts) behind the cell grid of
pmesh_amd.fof: the rows of ``lognormal_catalog``, of an N-body run or of ``fof_catalog`` are counted without leaving
HBM, down to separations far below the cell size of any mesh.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Rows.  ``pos1`` and ``pos2`` are ``(n, ndim)`` rows, ``ndim = len(pm.Nmesh)`` in 1 .. 3, float64 or float32 (widened
   exactly).  All arithmetic is in double, every operation rounded once.  Rows are wrapped by rule 2 of pmesh_amd.fof;
   ``dx_d`` is its minimum image of the wrapped rows; ``r2 = sum_d dx_d^2`` is accumulated in the order d = 0, 1, 2.
2. Modes.  ``'1d'`` bins by r, ``'2d'`` by (r, mu), ``'projected'`` by (rp, pi).  The last two need ndim == 3 and a
   line-of-sight axis ``los`` in {0, 1, 2}, default 2.
3. Edges.  ``edges`` (for r or rp) is increasing and finite with ``edges[0] >= 0``.  The host forms ``e2[k] = edges[k] *
   edges[k]`` once, in double; no square root chooses a bin.  A pair is in r-bin k when ``e2[k] <= q < e2[k + 1]``,
   ``q = r2`` in the modes 1d and 2d; in the projected mode ``q = rp2``, the sum of the two ``dx_d^2`` with d != los in
   ascending d.  Pairs outside ``[e2[0], e2[-1])`` are not counted.
4. mu bins (2d).  ``muedges`` is increasing from 0 to 1; ``m2[k] = muedges[k]^2`` is formed on the host.  With ``z2 =
   dx_los^2`` the mu-bin is the number of k in 1 .. nmu - 1 with ``z2 >= m2[k] * r2``: no division, no square root;
   mu = 1 lands in the last bin.  A pair with ``r2 == 0`` goes to mu-bin 0.
5. pi bins (projected).  ``piedges`` is increasing from 0.  With ``a = |dx_los|`` the pi-bin is the number of k in
   1 .. npi - 1 with ``a >= piedges[k]``; pairs with ``a >= piedges[-1]`` are not counted.
6. Pairs.  Cross (``pos2`` given): every (i in pos1, j in pos2), coincident rows included.  Auto (``pos2 is None``):
   every ordered pair i != j of pos1, so each unordered pair counts twice, as Corrfunc and nbodykit report it; self
   pairs are excluded.  The identity of a row is its global index, not its position: two different rows at one
   position are a pair at r2 = 0.
7. Sums, per bin.  ``npairs`` is int64 and exact; ``wnpairs = sum w1_i w2_j`` and ``rsum = sum w1_i w2_j r`` are double
   sums, ``r = sqrt(q)``.  Weights are ``(n,)`` float rows, or None for 1.  The order of the double sums is unspecified:
   their last bits may vary from run to run.  npairs never varies.
8. Search radius.  ``b = edges[-1]``, in the projected mode ``max(edges[-1], piedges[-1])``; b is finite, positive and
   ``2 b <= min_d L_d``, otherwise ValueError on every rank.  Rows with a coordinate that is not finite raise
   ValueError with their number, on every rank.
9. Bin limit.  ``nr``, ``nr * nmu`` or ``nrp * npi`` is at most PMX_PAIRS_MAX_BINS (4096); more raise ValueError.

    from pmesh_amd.paircount import pair_counts, pair_correlation
    pc = pair_counts(pm, pos, edges)                               # auto, bins of r
    pc.npairs, pc.wnpairs, pc.rsum, pc.rmean
    xi, pc = pair_correlation(pm, pos, edges, mode='2d', Nmu=100)  # xi(r, mu), natural estimator, analytic randoms

Host: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) with the radius b; each rank counts its primaries
against its secondaries with one kernel, and one allreduce per array sums the three.  In the auto form the self pairs
are subtracted on the host: they have r2 == 0 exactly, so they sit in bin (0, 0) when edges[0] == 0 and nowhere
otherwise.
"""
import numpy
import torch

from . import _abi, backend
from ._cells import Neighbourhood, allsum, box_of, read_rows, refuse_not_finite, sorted_sets, together, within_reach

MAX_BINS = _abi.PMX_PAIRS_MAX_BINS
MODES = {'1d': _abi.PMX_PAIRS_1D, '2d': _abi.PMX_PAIRS_2D, 'projected': _abi.PMX_PAIRS_PROJECTED}
# the modes of local_counts: those of pair_counts, and the two of pmesh_amd.surveypairs whose line of sight is the pair's
KERNEL_MODES = dict(MODES, **{'2d-midpoint': _abi.PMX_PAIRS_2D_MIDPOINT,
                              'projected-midpoint': _abi.PMX_PAIRS_PROJECTED_MIDPOINT})
# and the three of pmesh_amd.pairvel, whose sets bring a block of columns (w, v_0 .. v_{ndim-1}) or (w, s) in place of the
# one-column weight and whose rsum holds four sums per bin
VELOCITY_MODES = {'1d-velocity': _abi.PMX_PAIRS_1D_VELOCITY, 'projected-velocity': _abi.PMX_PAIRS_PROJECTED_VELOCITY,
                  '1d-los': _abi.PMX_PAIRS_1D_LOS}
KERNEL_MODES.update(VELOCITY_MODES)
# and those of pmesh_amd.pairlabels, a flag above one of the five base modes: the sets bring the block (w, label), and
# the three arrays hold 2 (split) or 1 + 2 K (jackknife; rsum: 1) blocks of nbins entries
LABEL_SLOTS = _abi.PMX_PAIRS_LABEL_SLOTS
LABEL_BASES = ('1d', '2d', 'projected', '2d-midpoint', 'projected-midpoint')
LABEL_MODES = {}
for _family, _flag in (('split', _abi.PMX_PAIRS_SPLIT), ('jackknife', _abi.PMX_PAIRS_JACKKNIFE)):
    for _base in LABEL_BASES:
        LABEL_MODES['%s-%s' % (_family, _base)] = _flag | KERNEL_MODES[_base]
KERNEL_MODES.update(LABEL_MODES)
# and the two of pmesh_amd.alignments, the flag PMX_PAIRS_ALIGN above the base modes 1d and projected: the sets bring the
# block (w, a_0 .. a_{ndim-1}) or (w, g1, g2), and rsum holds 1 + NS sums per bin, NS = 3 or 6
ALIGN_MODES = {'1d-align': _abi.PMX_PAIRS_ALIGN | _abi.PMX_PAIRS_1D,
               'projected-align': _abi.PMX_PAIRS_ALIGN | _abi.PMX_PAIRS_PROJECTED}
ALIGN_SUMS = {'1d-align': 3, 'projected-align': 6}
KERNEL_MODES.update(ALIGN_MODES)


def label_slots(nbins):
    """K of the jackknife modes: the labels one call takes, ``(PMX_PAIRS_LABEL_SLOTS / nbins - 2) / 2``; below 1: too
    many bins"""
    return (LABEL_SLOTS // nbins - 2) // 2


def label_lengths(mode, nbins):
    """the lengths of (npairs and wnpairs, rsum) in a mode of LABEL_MODES"""
    if mode.startswith('split'):
        return 2 * nbins, 2 * nbins
    return (1 + 2 * label_slots(nbins)) * nbins, nbins


# every mode of local_counts: (the blocks of nbins entries in npairs and wnpairs, None: the 1 + 2 K of the jackknife;
# the blocks in rsum; the most bins that local_counts itself checks, None where the callers' check is the only one;
# what its error calls the modes)
_BLOCKS = {_mode: (1, 1, None, None) for _mode in KERNEL_MODES}
_BLOCKS.update({_mode: (1, 4, None, None) for _mode in VELOCITY_MODES})
_BLOCKS.update({_mode: (2 if _mode.startswith('split') else None, 2 if _mode.startswith('split') else 1,
                        LABEL_SLOTS // 4, 'the modes by row labels') for _mode in LABEL_MODES})
_BLOCKS.update({_mode: (1, 1 + ALIGN_SUMS[_mode], _abi.PMX_PAIRS_ALIGN_MAX_BINS, 'the alignment modes')
                for _mode in ALIGN_MODES})


class PairCounts(object):
    """The binned sums over the pairs, identical on every rank: ``npairs`` (int64), ``wnpairs``, ``rsum`` and ``rmean =
    rsum / wnpairs`` (float64; nan where the bin holds no pair), device tensors of the shape (nr,), (nr, nmu) or (nrp,
    npi); ``edges`` and ``muedges`` / ``piedges`` (numpy arrays, None where the mode has none), ``mode``, ``los``,
    ``auto``; ``W1`` and ``W2`` (the sums of the weights of the two sets over all ranks; the row counts without
    weights), ``W2sum`` (auto: the sum of w^2; cross: 0), ``BoxSize``."""

    def __init__(self, npairs, wnpairs, rsum, edges, muedges, piedges, mode, los, auto, W1, W2, W2sum, BoxSize):
        self.npairs, self.wnpairs, self.rsum = npairs, wnpairs, rsum
        nan = torch.full_like(rsum, float('nan'))
        self.rmean = torch.where(npairs > 0, rsum / torch.where(npairs > 0, wnpairs, torch.ones_like(wnpairs)), nan)
        self.edges, self.muedges, self.piedges = edges, muedges, piedges
        self.mode, self.los, self.auto = mode, los, auto
        self.W1, self.W2, self.W2sum, self.BoxSize = W1, W2, W2sum, BoxSize


def bin_volumes(edges, ndim, mode='1d', sub=None):
    """V_bin of every bin: the volume in which the second row of a pair of that bin lies around the first.

    1d: 4 pi / 3 (e_hi^3 - e_lo^3) for ndim 3, pi (e_hi^2 - e_lo^2) for ndim 2, 2 (e_hi - e_lo) for ndim 1.  2d: the 3-d
    value times (mu_hi - mu_lo).  projected: pi (rp_hi^2 - rp_lo^2) * 2 (pi_hi - pi_lo)."""
    e = numpy.asarray(edges, dtype='f8')
    if mode == 'projected':
        s = numpy.asarray(sub, dtype='f8')
        return (numpy.pi * (e[1:] ** 2 - e[:-1] ** 2))[:, None] * (2 * (s[1:] - s[:-1]))[None, :]
    if ndim == 3:
        v = 4 * numpy.pi / 3 * (e[1:] ** 3 - e[:-1] ** 3)
    elif ndim == 2:
        v = numpy.pi * (e[1:] ** 2 - e[:-1] ** 2)
    else:
        v = 2 * (e[1:] - e[:-1])
    if mode == '2d':
        s = numpy.asarray(sub, dtype='f8')
        return v[:, None] * (s[1:] - s[:-1])[None, :]
    return v


def _edges(x, what, first=None, last=None):
    """(the edges as a float64 numpy array, error)"""
    try:
        e = numpy.array(x, dtype='f8')
    except (TypeError, ValueError):
        return None, ValueError('%s must be a sequence of numbers' % what)
    if e.ndim != 1 or len(e) < 2 or not numpy.isfinite(e).all() or not (numpy.diff(e) > 0).all() or e[0] < 0:
        return None, ValueError('%s must be increasing and finite, at least two of them, the first >= 0' % what)
    if first is not None and e[0] != first:
        return None, ValueError('%s must start at %g' % (what, first))
    if last is not None and e[-1] != last:
        return None, ValueError('%s must end at %g' % (what, last))
    return e, None


def too_many(e, sub, limit, what):
    """None, or the error of more than `limit` bins of the edges `e` and the sub edges `sub` (None: one sub bin); `what`
    ends the message: the name of the limit"""
    nbins = (len(e) - 1) * (len(sub) - 1 if sub is not None else 1)
    if nbins > limit:
        return ValueError('%d bins: at most %d %s' % (nbins, limit, what))
    return None


def _binning(nd, edges, mode, muedges, Nmu, piedges, pimax, los):
    """(edges, sub edges or None, error) of the arguments that say how to bin"""
    if mode not in MODES:
        return None, None, ValueError("mode must be '1d', '2d' or 'projected', not %r" % (mode,))
    e, error = _edges(edges, 'edges')
    if error is not None:
        return None, None, error
    sub = None
    if mode != '1d':
        if nd != 3:
            return None, None, ValueError("mode=%r needs a mesh of three dimensions, not %d" % (mode, nd))
        if los not in (0, 1, 2):
            return None, None, ValueError('los must be 0, 1 or 2, not %r' % (los,))
        if mode == '2d':
            if muedges is None and Nmu is not None and int(Nmu) == Nmu and Nmu >= 1:
                muedges = numpy.linspace(0.0, 1.0, int(Nmu) + 1)
            if muedges is None:
                return None, None, ValueError("mode='2d' needs muedges, or Nmu: a positive integer")
            sub, error = _edges(muedges, 'muedges', first=0.0, last=1.0)
        else:
            if piedges is None and pimax is not None and int(pimax) == pimax and pimax >= 1:
                piedges = numpy.arange(0.0, int(pimax) + 1)
            if piedges is None:
                return None, None, ValueError("mode='projected' needs piedges, or pimax: a positive integer")
            sub, error = _edges(piedges, 'piedges', first=0.0)
        if error is not None:
            return None, None, error
    error = too_many(e, sub, MAX_BINS, '(PMX_PAIRS_MAX_BINS)')
    return (e, sub, None) if error is None else (None, None, error)


def local_counts(be, mode, los, pos1, weight1, pos2, weight2, grid, box, e2, sub):
    """The three arrays of the rows of one rank on the cell grid `grid` (of _cells.cell_grid): every row of `pos1` with
    every row of `pos2` (None: with every row of pos1, itself included: the caller subtracts the self pairs).  e2 and
    sub: device tensors.  mode: a key of KERNEL_MODES.  Returns (npairs, wnpairs, rsum), flat.  In the modes of
    VELOCITY_MODES weight1 and weight2 are the (n, ncol) blocks of columns of the two sets and rsum has 4 * nbins
    entries, rsum[m * nbins + b].  In the modes of LABEL_MODES they are the (n, 2) blocks (w, label) and the arrays have
    the lengths of label_lengths: the blocks of the header, each of nbins entries.  In the modes of ALIGN_MODES they are
    the (n, 1 + ndim) blocks (w, a) or the (n, 3) blocks (w, g1, g2), and rsum has (1 + NS) * nbins entries, NS of
    ALIGN_SUMS."""
    dev = pos1.device
    nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
    counts, sums, limit, what = _BLOCKS[mode]
    if limit is not None and nbins > limit:
        raise ValueError('%d bins: at most %d in %s' % (nbins, limit, what))
    if counts is None:
        counts = 1 + 2 * label_slots(nbins)
    ncount, nrsum = counts * nbins, sums * nbins
    npairs = torch.zeros(ncount, dtype=torch.int64, device=dev)
    wnpairs = torch.zeros(ncount, dtype=torch.float64, device=dev)
    rsum = torch.zeros(nrsum, dtype=torch.float64, device=dev)
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, pos1, pos2, grid, box)
    if pos2 is None:
        weight2 = weight1
    be.pair_counts(KERNEL_MODES[mode], los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2,
                   grid[0], grid[3], box, e2, sub, npairs, wnpairs, rsum)
    return npairs, wnpairs, rsum


def _weight_sums(comm, w, n):
    """(sum of w, sum of w^2) over all ranks, as floats; the row count twice without weights"""
    if w is None:
        total = float(comm.allreduce(n)) if comm.size > 1 else float(n)
        return total, total
    w = w.to(torch.float64)
    s = torch.stack([w.sum(), (w * w).sum()])
    s = allsum(comm, s).cpu()
    return float(s[0]), float(s[1])


def _block_of(weight, cols):
    """the contiguous (n, 1 + ncol) block (w, columns) of one set: w = 1 without a weight; float32 where the columns
    and the weight are, else float64"""
    dtype = cols.dtype if weight is None or weight.dtype == cols.dtype else torch.float64
    w = torch.ones(cols.shape[0], dtype=dtype, device=cols.device) if weight is None else weight.to(dtype)
    return torch.cat([w.reshape(-1, 1), cols.to(dtype)], dim=1).contiguous()


def _count(pm, pos1, pos2, weight1, weight2, kernel, los, e2, sub, b, error, prepare=None, columns=None,
           self_pairs=True):
    """What the public counting calls share behind their own reading of the binning: the argument checks of the rows
    and the weights, the weight sums, the routing, the allreduce and the self pairs.

    kernel : the mode of local_counts.  e2, sub : float64 numpy arrays, what the kernel is given (sub None in 1d).
    b : the search radius, or None with `error`.  error : what the caller found wrong already, or None.
    prepare : None, or a function (pos1, pos2) -> (pos1, pos2) applied to the device rows once they are known to be
        finite, before anything is counted; it raises on every rank together.
    columns : None, or (name, x1, x2, ncol) for the modes of VELOCITY_MODES: the further columns of the rows of the two
        sets, (n, ncol) float rows called `name`1 and `name`2 in messages; x2 is given exactly when pos2 is.  They must
        be finite.  Each set then travels as one contiguous (n, 1 + ncol) block (w, columns), w = 1 without a weight,
        float32 where all of its parts are, through the exchanges of the weights, and rsum has 4 * nbins entries.
        The modes of LABEL_MODES bring ('label', l1, l2, 1) in the same way: the labels as floats, which hold them
        exactly.  The modes of ALIGN_MODES bring ('shape', s1, s2, ndim) or ('ellipticity', g1, g2, 2), and rsum has
        (1 + NS) * nbins entries.  A fifth member, (bool, bool), says of which of the two sets a row whose columns are
        all zero is refused (an orientation of no direction): ValueError with their number, on every rank.
    self_pairs : False leaves the self pairs of the auto form in the arrays: the caller of a mode of LABEL_MODES, whose
        arrays hold several blocks, removes them from the blocks they sit in.
    Returns (npairs, wnpairs, rsum: flat device tensors, identical on every rank; W1, W2, W2sum; box)."""
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    box = box_of(pm)
    auto = pos2 is None
    if error is None and not within_reach(b, box):
        error = ValueError('the largest separation must be finite, positive and at most half the shortest box '
                           'side: %r' % b)
    if error is None and auto and weight2 is not None:
        error = ValueError('weight2 needs pos2')
    wanted = [('pos1', pos1, nd, None), ('pos2', pos2, nd, None), ('weight1', weight1, 1, 0), ('weight2', weight2, 1, 1)]
    if columns is not None:
        name, x1, x2, ncol = columns[:4]
        if error is None and x1 is None:
            error = ValueError('%s1 is needed' % name)
        if error is None and (x2 is None) != auto:
            error = ValueError('%s2 needs pos2' % name if auto else 'pos2 needs %s2' % name)
        wanted += [(name + '1', x1, ncol, 0), (name + '2', x2, ncol, 1)]
    rows, error = read_rows(pm, be, wanted, error)
    together(comm, error)
    pos1, pos2, weight1, weight2 = rows[:4]
    if weight1 is not None:
        weight1 = weight1.reshape(-1)
    if weight2 is not None:
        weight2 = weight2.reshape(-1)
    refuse_not_finite(comm, 'pos1 and pos2', pos1, pos2)
    if columns is not None:
        refuse_not_finite(comm, '%s1 and %s2' % (columns[0], columns[0]), *rows[4:], entry='an entry')
        if len(columns) > 4:
            nbad = sum(int((x == 0).all(dim=1).sum()) for x, on in zip(rows[4:], columns[4]) if x is not None and on)
            if comm.size > 1:
                nbad = int(comm.allreduce(nbad))
            if nbad:
                raise ValueError('%d rows of %s1 and %s2 are zero vectors' % (nbad, columns[0], columns[0]))
    if prepare is not None:
        pos1, pos2 = prepare(pos1, pos2)
    n1 = pos1.shape[0]
    W1, W1sq = _weight_sums(comm, weight1, n1)
    W2, W2sum = (W1, W1sq) if auto else (_weight_sums(comm, weight2, pos2.shape[0])[0], 0.0)
    csize1 = int(comm.allreduce(n1)) if comm.size > 1 else n1
    if columns is not None:
        # from here on the weight of a set is its block of columns
        weight1 = _block_of(weight1, rows[4])
        weight2 = None if auto else _block_of(weight2, rows[5])
    dev = be.device
    first = e2[0]
    e2 = torch.from_numpy(numpy.ascontiguousarray(e2, dtype='f8')).to(dev)
    subt = None if sub is None else torch.from_numpy(numpy.ascontiguousarray(sub, dtype='f8')).to(dev)
    hood = Neighbourhood(pm, b, pos1, pos2)
    p1, q1 = hood.to_owners(pos1), hood.to_owners(weight1)
    p2, q2 = hood.to_sources(pos1 if auto else pos2), hood.to_sources(weight1 if auto else weight2)
    sums = local_counts(be, kernel, los, p1, q1, None if hood.same else p2, q2, hood.grid, box, e2, subt)
    sums = [hood.allsum(x) for x in sums]
    npairs, wnpairs, rsum = sums
    if self_pairs and auto and first == 0:
        # the self pairs: r2 == 0 exactly, bin (0, 0)
        npairs[0] -= csize1
        wnpairs[0] -= W2sum
    return npairs, wnpairs, rsum, W1, W2, W2sum, box


def pair_counts(pm, pos1, edges, pos2=None, weight1=None, weight2=None, mode='1d', muedges=None, Nmu=None,
                piedges=None, pimax=None, los=2):
    """The binned pair counts of the rows by the rule of the module docstring: a PairCounts.

    pm : ParticleMesh of 1, 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos1 : (n, ndim) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    edges : the nr + 1 edges of the bins of r (of rp in the projected mode), in box units.
    pos2 : the rows of a second set for the cross counts, or None: the ordered pairs i != j of pos1.
    weight1, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.
    mode : '1d', '2d' or 'projected'.  muedges, or Nmu for Nmu uniform bins of mu in [0, 1]; piedges, or pimax for bins
        of unit width in [0, pimax]: nbodykit's conventions.  los : the axis of the line of sight.

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('pair counts on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    e, sub, error = _binning(nd, edges, mode, muedges, Nmu, piedges, pimax, los)
    b = e2 = given = None
    if error is None:
        b = float(max(e[-1], sub[-1])) if mode == 'projected' else float(e[-1])
        e2 = e * e
        given = sub * sub if mode == '2d' else sub
    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, mode, los, e2, given, b, error)
    shape = (len(e) - 1,) if sub is None else (len(e) - 1, len(sub) - 1)
    return PairCounts(npairs.reshape(shape), wnpairs.reshape(shape), rsum.reshape(shape), e,
                      sub if mode == '2d' else None, sub if mode == 'projected' else None, mode, los, pos2 is None, W1,
                      W2, W2sum, box)


def pair_correlation(pm, pos1, edges, pos2=None, weight1=None, weight2=None, mode='1d', muedges=None, Nmu=None,
                     piedges=None, pimax=None, los=2):
    """(xi, PairCounts): the natural estimator with analytic randoms, ``xi = wnpairs / RR - 1`` with ``RR = (W1 W2 -
    [auto] sum w^2) V_bin / V_box`` (bin_volumes), a float64 device tensor of the shape of the counts.  The arguments
    are those of pair_counts.  RR is host arithmetic on nbins numbers."""
    pc = pair_counts(pm, pos1, edges, pos2, weight1, weight2, mode, muedges, Nmu, piedges, pimax, los)
    sub = pc.muedges if mode == '2d' else pc.piedges
    rr = (pc.W1 * pc.W2 - pc.W2sum) * bin_volumes(pc.edges, len(pc.BoxSize), mode, sub) / float(numpy.prod(pc.BoxSize))
    xi = pc.wnpairs / torch.from_numpy(numpy.ascontiguousarray(rr)).to(pc.wnpairs.device) - 1
    return xi, pc
