"""The short-range pair force of particles, summed on the device: the other half of a TreePM / P3M force.

A mesh force is smoothed below about two cells.  MP-Gadget splits Newton's force into a long-range part, solved on
the mesh with the Gaussian filter ``exp(-k^2 r_split^2)``, and a short-range part summed over near pairs (by its tree).
This module sums the short-range part over the pairs of the cell grid of pmesh_amd.fof (the P3M form) as one entry of
the C ABI (csrc/pmx_shortrange.hip, include/pmesh_amd.h: pmx_short_range); ``Transfer.long_range(d, r_split)`` is the
mesh partner, and the sum of the two is Newton's force.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Rows.  ``pos`` (primaries) and ``pos2`` (sources; None: the primaries themselves) are ``(n, 3)`` rows, float64 or
   float32 (widened exactly).  Three dimensions only; anything else raises NotImplementedError.  Rows are wrapped by
   rule 2 of pmesh_amd.fof; ``dx_d = x_i,d - x_j,d`` is its minimum image of the wrapped rows; ``r2 = dx_0^2 + dx_1^2
   + dx_2^2``, summed in that order.  All arithmetic is in double.
2. Cut.  Source j is a neighbour of primary i when ``0 < r2 < rc2``, ``rc2 = r_cut * r_cut`` formed once on the host;
   no square root decides this.  Pairs with ``r2 == 0`` (a row with itself, coincident rows) contribute nothing: the
   entry needs no row identity and the auto form no correction.
3. Force.  ``r = sqrt(r2)``, ``u = r / (2 r_split)``, ``s2 = r2 + softening^2``;

       fac = erfc(u) + (2 / sqrt(pi)) u exp(-u^2)
       acc_i,d = -G sum_j m_j dx_d fac / (s2 sqrt(s2))
       pot_i   = -G sum_j m_j erfc(u) / sqrt(s2)
       neighbours_i = the number of neighbours (int64, exact)

   Masses are one column in row order, float32 or float64; None means 1.  ``fac`` and ``erfc`` are evaluated in closed
   form with the device's double ``erfc`` and ``exp``.  The order of the double sums is unspecified: the last bits may
   vary; ``neighbours`` never varies.
4. Arguments.  ``r_split > 0`` and finite; ``r_cut`` finite, positive, ``2 r_cut <= min_d L_d``, default ``4.5 *
   r_split`` (Gadget's RCUT); ``softening >= 0`` (Plummer).  Rows that are not finite raise ValueError with their
   number.  Every argument error is raised on all ranks together.

Units.  ``examples/nbody.py`` solves ``laplace(phi) = rho`` with mean density 1: its force is this one with ``G = 1 /
(4 pi)`` and ``mass = V / N`` per particle, and its long-range partner is ``i D(k_d) / k^2 exp(-k^2 r_split^2)``,
``gauss_r = sqrt(2) r_split``:

    from pmesh_amd.shortrange import short_range_force
    from pmesh_amd.transfer import Transfer
    acc = short_range_force(pm, pos, r_split, mass=m, G=1 / (4 * numpy.pi))       # + the readout of
    mesh = [rho_k.apply(Transfer.long_range(d, r_split)).c2r() for d in range(3)]  # these at pos

On one rank the rows are sorted into one periodic cell grid of side >= r_cut (``fof.cell_grid`` / ``fof.cell_sort``;
the auto form sorts once) and one kernel sums.  On several ranks the routing is that of pair_counts: the primaries go to
their owners (``pm.decompose`` without ghosts), the sources and their masses to every rank whose block they lie within
r_cut of; each rank sums the force on its primaries, and ``Layout.gather(mode='sum')`` returns the rows to their
callers: every primary has one owner, so nothing is added twice.
"""
import numpy
import torch

from . import backend
from .fof import MAX_ROWS, _block, _rows, _together, cell_grid, cell_sort

RCUT = 4.5                               # the default r_cut in units of r_split (Gadget's RCUT)


def local_force(be, pos1, pos2, mass2, grid, box, G, r_split, rc2, eps2, potential=False, neighbours=False):
    """The sums of the rows of one rank on the cell grid `grid` (of fof.cell_grid): the force on every row of `pos1`
    from the rows of `pos2` with the masses `mass2` (pos2 None: from pos1 itself, mass2 then its masses).  Returns (acc
    (n1, 3), pot (n1,) or None, neighbours (n1,) or None) in the row order of pos1."""
    dev = pos1.device
    n1 = pos1.shape[0]
    acc = torch.empty((n1, 3), dtype=torch.float64, device=dev)
    pot = torch.empty(n1, dtype=torch.float64, device=dev) if potential else None
    nb = torch.empty(n1, dtype=torch.int64, device=dev) if neighbours else None
    _, cell_of1, cell_start1, order1, spos1, _ = cell_sort(be, pos1, grid, box)
    if pos2 is None:
        order2, cell_start2, spos2 = order1, cell_start1, spos1
    else:
        _, _, cell_start2, order2, spos2, _ = cell_sort(be, pos2, grid, box)
    be.short_range(spos1, order1, cell_of1, spos2, order2, cell_start2, mass2, grid[0], grid[3], box, G, r_split, rc2,
                   eps2, acc, pot, nb)
    return acc, pot, nb


def _positive(x, what, zero=False):
    """(x as a float, error): finite and positive (zero: or zero)"""
    try:
        v = float(x)
    except (TypeError, ValueError):
        return None, ValueError('%s must be a number, not %r' % (what, x))
    if not (numpy.isfinite(v) and (v >= 0 if zero else v > 0)):
        return None, ValueError('%s must be finite and %s: %r' % (what, 'not negative' if zero else 'positive', x))
    return v, None


def short_range_force(pm, pos, r_split, r_cut=None, mass=None, pos2=None, mass2=None, softening=0.0, G=1.0,
                      potential=False, neighbours=False):
    """The short-range acceleration of the rows `pos` by the rule of the module docstring: ``acc``, an (n, 3) float64
    device tensor in the caller's row order; with ``potential`` and ``neighbours`` a tuple ``(acc[, pot][,
    neighbours])``, pot (n,) float64 and neighbours (n,) int64.

    pm : ParticleMesh of three dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos : (n, 3) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    r_split : the scale of the split, in box units; the mesh partner is ``Transfer.long_range(d, r_split)``.
    r_cut : pairs at r_cut and beyond are not summed (erfc(2.25) = 1.5e-3 at the default 4.5 r_split).
    mass : (n,) float rows, the masses of `pos`, or None for 1: the sources' masses when pos2 is None.  With pos2 the
        acceleration does not depend on them.
    pos2, mass2 : the rows and masses of the sources, or None: `pos` and `mass`.  mass2 needs pos2.
    softening : the Plummer softening length.  G : the constant of gravity.

    Argument errors are raised on every rank together.  More than 2^31 - 1 rows, ghosts included, on one rank raise
    ValueError: slots are 32-bit.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd != 3:
        raise NotImplementedError('the short-range force needs a mesh of three dimensions, not %d' % nd)
    box = [float(x) for x in numpy.broadcast_to(numpy.asarray(pm.BoxSize, dtype='f8'), (nd,))]
    auto = pos2 is None
    rs, error = _positive(r_split, 'r_split')
    rc = eps = g = None
    if error is None:
        rc, error = _positive(RCUT * rs if r_cut is None else r_cut, 'r_cut')
    if error is None and not 2 * rc <= min(box):
        error = ValueError('r_cut must be at most half the shortest box side: %r' % rc)
    if error is None:
        eps, error = _positive(softening, 'softening', zero=True)
    if error is None:
        try:
            g = float(G)
        except (TypeError, ValueError):
            g = numpy.nan
        if not numpy.isfinite(g):
            error = ValueError('G must be a finite number, not %r' % (G,))
    if error is None and auto and mass2 is not None:
        error = ValueError('mass2 needs pos2')
    rows = []
    for what, x, ncol, of in (('pos', pos, nd, None), ('pos2', pos2, nd, None), ('mass', mass, 1, 0),
                              ('mass2', mass2, 1, 1)):
        t = None
        if x is not None and error is None:
            t, error = _rows(pm, be, x, what, ncol, None if of is None else rows[of].shape[0])
        rows.append(t)
    _together(comm, error)
    pos, pos2, mass, mass2 = rows
    if mass is not None:
        mass = mass.reshape(-1)
    if mass2 is not None:
        mass2 = mass2.reshape(-1)
    nbad = int((~torch.isfinite(pos)).any(dim=1).sum()) + (0 if auto else int((~torch.isfinite(pos2)).any(dim=1).sum()))
    if comm.size > 1:
        nbad = int(comm.allreduce(nbad))
    if nbad:
        raise ValueError('%d rows of pos and pos2 have a coordinate that is not finite' % nbad)
    n1 = pos.shape[0]
    src, msrc = (pos, mass) if auto else (pos2, mass2)
    rc2, eps2 = rc * rc, eps * eps
    if comm.size == 1:
        most = max(n1, src.shape[0])
        _together(comm, ValueError('more than 2^31 - 1 rows on one rank') if most > MAX_ROWS else None)
        acc, pot, nb = local_force(be, pos, None if auto else src, msrc, cell_grid(most, rc, box), box, g, rs, rc2,
                                   eps2, potential, neighbours)
    else:
        # the routing of pair_counts: the primaries to their owners, the sources to every rank whose block they lie
        # within r_cut of (a hair more: a pair just inside r_cut across a block face must not depend on the rounding
        # of the routing)
        own = pm.decompose(pos, smoothing=0)
        smoothing = rc * numpy.asarray(pm.Nmesh, dtype='f8') / numpy.asarray(box) * (1 + 1e-9)
        ghosts = pm.decompose(src, smoothing=smoothing)
        most = max(own.recvlength, ghosts.recvlength)
        _together(comm, ValueError('more than 2^31 - 1 rows and ghosts on one rank') if most > MAX_ROWS else None)
        p1 = own.exchange(pos)
        p2 = ghosts.exchange(src)
        q2 = ghosts.exchange(msrc) if msrc is not None else None
        lo, hi = _block(pm)
        acc, pot, nb = local_force(be, p1, p2, q2, cell_grid(most, rc, box, lo, hi), box, g, rs, rc2, eps2, potential,
                                   neighbours)
        # every primary has exactly one owner: the sum over its copies is its value
        acc = own.gather(acc, mode='sum')
        pot = own.gather(pot, mode='sum') if potential else None
        nb = own.gather(nb, mode='sum') if neighbours else None
    out = (acc,) + ((pot,) if potential else ()) + ((nb,) if neighbours else ())
    return out[0] if len(out) == 1 else out
