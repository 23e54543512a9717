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

Host: the routing of DESIGN.md §5.7.0 (``_cells.Neighbourhood``) with the radius r_cut; the sources' masses travel with
them, each rank sums the force on its primaries with one kernel, and the rows return to their callers with the mode
'sum': every primary has one owner, so nothing is added twice.
"""
import numpy
import torch

from . import backend
from ._cells import Neighbourhood, box_of, read_rows, refuse_not_finite, sorted_sets, together, within_reach

RCUT = 4.5                               # the default r_cut in units of r_split (Gadget's RCUT)


def local_force(be, pos1, pos2, mass2, grid, box, G, r_split, rc2, eps2, potential=False, neighbours=False):
    """The sums of the rows of one rank on the cell grid `grid` (of _cells.cell_grid): the force on every row of `pos1`
    from the rows of `pos2` with the masses `mass2` (pos2 None: from pos1 itself, mass2 then its masses).  Returns (acc
    (n1, 3), pot (n1,) or None, neighbours (n1,) or None) in the row order of pos1."""
    dev = pos1.device
    n1 = pos1.shape[0]
    acc = torch.empty((n1, 3), dtype=torch.float64, device=dev)
    pot = torch.empty(n1, dtype=torch.float64, device=dev) if potential else None
    nb = torch.empty(n1, dtype=torch.int64, device=dev) if neighbours else None
    spos1, order1, cell_of1, spos2, order2, cell_start2 = sorted_sets(be, pos1, pos2, grid, box)
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

    Argument errors are raised on every rank together, the row limit of DESIGN.md §5.7.0 among them.
    """
    be = backend.get()
    comm = pm.comm
    nd = len(pm.Nmesh)
    if nd != 3:
        raise NotImplementedError('the short-range force needs a mesh of three dimensions, not %d' % nd)
    box = box_of(pm)
    auto = pos2 is None
    rs, error = _positive(r_split, 'r_split')
    rc = eps = g = None
    if error is None:
        rc, error = _positive(RCUT * rs if r_cut is None else r_cut, 'r_cut')
    if error is None and not within_reach(rc, box):
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
    wanted = (('pos', pos, nd, None), ('pos2', pos2, nd, None), ('mass', mass, 1, 0), ('mass2', mass2, 1, 1))
    (pos, pos2, mass, mass2), error = read_rows(pm, be, wanted, error)
    together(comm, error)
    if mass is not None:
        mass = mass.reshape(-1)
    if mass2 is not None:
        mass2 = mass2.reshape(-1)
    refuse_not_finite(comm, 'pos and pos2', pos, pos2)
    src, msrc = (pos, mass) if auto else (pos2, mass2)
    rc2, eps2 = rc * rc, eps * eps
    hood = Neighbourhood(pm, rc, pos, pos2)
    p1, p2, q2 = hood.to_owners(pos), hood.to_sources(src), hood.to_sources(msrc)
    acc, pot, nb = local_force(be, p1, None if hood.same else p2, q2, hood.grid, box, g, rs, rc2, eps2, potential,
                               neighbours)
    acc, pot, nb = [hood.to_callers(x, 'sum') for x in (acc, pot, nb)]
    out = (acc,) + ((pot,) if potential else ()) + ((nb,) if neighbours else ())
    return out[0] if len(out) == 1 else out
