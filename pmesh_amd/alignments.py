"""Intrinsic-alignment pair statistics of particles, made on the device.

What halotools-ia does on the host as ``ed_3d``, ``ee_3d``, ``gi_plus_projected``, ``ii_plus_projected`` and their
``minus`` partners: the position-shape and shape-shape correlations omega(r) and eta(r) of orientation vectors, and
the projected w_g+(rp), w_++(rp) and w_xx(rp) of spin-2 ellipticities, measured on halo catalogues to calibrate the
alignment models of weak-lensing surveys, for the rows of ``fof_catalog`` or ``so_masses`` without leaving HBM.  None of
them is a weighted ``pair_counts``: the quantity summed depends on the geometry of the pair relative to a per-row
vector or spin-2 quantity.  No entry of the C ABI is added: ``pmx_pair_counts`` (include/pmesh_amd.h) has the flag
PMX_PAIRS_ALIGN = 128 above two of its base modes, PMX_PAIRS_ALIGN | PMX_PAIRS_1D (128) and PMX_PAIRS_ALIGN |
PMX_PAIRS_PROJECTED (130), whose kernels are in csrc/pmx_pairs_align.hip.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

Shared with the base modes, unchanged.  Mode 128 shares everything below with PMX_PAIRS_1D (``'1d'`` of
pmesh_amd.paircount), mode 130 with PMX_PAIRS_PROJECTED (``'projected'``): rows, wrapping, the minimum image ``dx_d``
(primary minus secondary), ``r2``, ``q``, the squared edges, the r-bin, the pi-bin, the pimax cut and the loop over
windows of 2^23 secondaries; all arithmetic in double; every operation rounded once, no contraction; no square root
chooses a bin.  ``npairs`` in these modes equals ``npairs`` of the base mode on the same arguments, to the last count.

Per-row columns.  ``weight1`` and ``weight2`` of the entry are both required: contiguous blocks in row order, float or
double.  The host packs them as one ``(n, ncol)`` tensor (w = 1 without a weight).  A set without shapes brings zeros.

Outputs.  ``npairs`` and ``wnpairs`` have ``nbins = nr * nsub`` entries.  ``rsum`` has ``(1 + NS) * nbins`` entries,
``rsum[m * nbins + b]``: m = 0 is ``sum w sqrt(q)``, as in the base mode; m = 1 .. NS are the sums below.  ``nbins`` is
at most PMX_PAIRS_ALIGN_MAX_BINS (1024); more raise ValueError before any launch.  The order of the double sums is
unspecified; ``npairs`` is exact.

Per counted pair, with ``w = w1_i * w2_j``:

Mode 128 (``alignment_counts``), ndim 2 or 3, NS = 3.  The columns are ``(w, a_0 .. a_{ndim-1})``: an orientation
vector, not necessarily a unit vector.  With ``a`` the primary's vector and ``c`` the secondary's, each sum over
``d < ndim`` in ascending d: ``a2 = sum a_d a_d``, ``c2 = sum c_d c_d``, ``pa = sum dx_d a_d``, ``pc = sum dx_d c_d``,
``ac = sum a_d c_d``.  ``t1 = (r2 > 0 && a2 > 0) ? (pa * pa) / (a2 * r2) : 0``, the cos^2 between the primary's axis
and the separation.  ``t2 = (r2 > 0 && c2 > 0) ? (pc * pc) / (c2 * r2) : 0``.  ``t3 = (r2 > 0 && a2 > 0 && c2 > 0) ?
(ac * ac) / (a2 * c2) : 0``, the cos^2 between the two axes.  ``S1 += w * t1, S2 += w * t2, S3 += w * t3``

Mode 130 (``projected_alignment_counts``), ndim 3, ``los`` in {0, 1, 2}, NS = 6.  The columns are ``(w, g1, g2)``: the
spin-2 ellipticity in the plane normal to ``los``, referred to the axes ``A < B``, the two axes other than ``los`` in
ascending order.  ``g1 > 0`` is elongation along A, ``g2 > 0`` along the diagonal A = B.  With ``rp2 = q``: ``cc = dx_A
* dx_A - dx_B * dx_B`` and ``ss = 2.0 * (dx_A * dx_B)``.  For the primary ``p1 = rp2 > 0 ? (g1_i * cc + g2_i * ss) /
rp2 : 0`` and ``x1 = rp2 > 0 ? (g1_i * ss - g2_i * cc) / rp2 : 0``; ``p2`` and ``x2`` are the same with the secondary's
columns.  The direction is spin-2, so the reversed separation gives the same ``cc`` and ``ss``.
``S1 += w * p1, S2 += w * p2, S3 += (w * p1) * p2, S4 += (w * x1) * x2, S5 += w * x1, S6 += w * x2``
``p > 0`` means the shape points along the projected separation (radial alignment); ``x`` is the 45 degree component,
whose means vanish by parity.  No trigonometric call and no square root beyond the base mode's.

Consequences.  A pair with ``r2 == 0`` (``rp2 == 0``) adds nothing to ``S1 .. S_NS``, so a self pair of the auto form is
inert there; the host subtracts the self pairs from ``npairs[0]`` and ``wnpairs[0]`` exactly as pmesh_amd.paircount
does.  Scaling a vector by a power of two changes no bit of any sum of mode 128, and neither does ``a -> -a``.  The
products ``a2 * r2`` and ``a2 * c2`` must neither overflow nor underflow: finite, sanely scaled columns are the
caller's business; the host checks that they are finite.  The search radius, the finiteness of the rows and the ranks
are those of pmesh_amd.paircount (rule 8 and the routing there).

    from pmesh_amd.alignments import alignment_counts, projected_alignment_counts, ellipticity_from_orientation
    ac = alignment_counts(pm, pos, axis, edges)                    # auto, bins of r
    ac.omega, ac.eta                                               # <cos^2> - 1/ndim of axis-separation and axis-axis
    g = ellipticity_from_orientation(axis, los=2, magnitude=0.2)
    pa = projected_alignment_counts(pm, pos, g, rpedges, pos2=galaxies, pimax=40)
    pa.w('plus1')                                                  # w_g+(rp): shapes in set 1, positions in set 2
    pa.w('plusplus'), pa.w('crosscross'), pa.w('cross1')           # w_++, w_xx and the null test w_gx (ellip2 given)

Out of scope: the survey forms, whose line of sight is the observer's; jackknife combinations of these sums.  The
caller brings the orientations: pmesh_amd.moments.halo_shapes measures them about the centres of a halo catalogue.
"""
import numpy
import torch

from . import _abi, backend
from .paircount import PairCounts, _binning, _count, bin_volumes, too_many
from .pairvel import _ratio
from .surveypairs import to_wp

MAX_BINS = _abi.PMX_PAIRS_ALIGN_MAX_BINS
PROJECTED_SUMS = ('plus1', 'plus2', 'plusplus', 'crosscross', 'cross1', 'cross2')


class AlignmentCounts(PairCounts):
    """A PairCounts with the sums of the rule, device tensors of the shape (nr,), identical on every rank: ``ed_sum``
    (S1), ``de_sum`` (S2), ``ee_sum`` (S3); and derived from them, nan where a bin holds no pair: ``omega = ed_sum /
    wnpairs - 1 / ndim``, the alignment of the axes of set 1 with the directions to set 2; ``omega_de = de_sum / wnpairs
    - 1 / ndim``, that of the axes of set 2 with the directions to set 1; ``eta = ee_sum / wnpairs - 1 / ndim``, that of
    the axes of the two sets with each other.  ``omega_de`` and ``eta`` are None where the second set brought no shapes.
    ``ndim``."""

    def __init__(self, npairs, wnpairs, sums, *args, **kw):
        self.ndim = kw.pop('ndim')
        both = kw.pop('both')
        PairCounts.__init__(self, npairs, wnpairs, sums[0], *args, **kw)
        self.ed_sum, self.de_sum, self.ee_sum = sums[1], sums[2], sums[3]
        filled = npairs > 0
        self.omega = _ratio(self.ed_sum, wnpairs, filled) - 1.0 / self.ndim
        self.omega_de = _ratio(self.de_sum, wnpairs, filled) - 1.0 / self.ndim if both else None
        self.eta = _ratio(self.ee_sum, wnpairs, filled) - 1.0 / self.ndim if both else None


class ProjectedAlignments(PairCounts):
    """A PairCounts of the shape (nrp, npi) with the sums of the rule, device tensors of that shape, identical on every
    rank: ``plus1`` (S1), ``plus2`` (S2), ``plusplus`` (S3), ``crosscross`` (S4), ``cross1`` (S5), ``cross2`` (S6).
    ``xi(which)`` and ``w(which)`` turn one of them into a correlation function."""

    def __init__(self, npairs, wnpairs, sums, *args, **kw):
        PairCounts.__init__(self, npairs, wnpairs, sums[0], *args, **kw)
        for name, s in zip(PROJECTED_SUMS, sums[1:]):
            setattr(self, name, s)

    def rr(self):
        """the analytic ``RR = (W1 W2 - [auto] sum w^2) V_bin / V_box`` of pair_correlation: (nrp, npi), float64, numpy"""
        return (self.W1 * self.W2 - self.W2sum) * bin_volumes(self.edges, 3, 'projected', self.piedges) \
            / float(numpy.prod(self.BoxSize))

    def xi(self, which):
        """``S / RR`` for the sum called `which` (a name of PROJECTED_SUMS): (nrp, npi), a device tensor"""
        if which not in PROJECTED_SUMS:
            raise ValueError('which must be one of %s, not %r' % (', '.join(PROJECTED_SUMS), which))
        s = getattr(self, which)
        return s / torch.from_numpy(numpy.ascontiguousarray(self.rr())).to(s.device)

    def w(self, which):
        """the projected function ``2 sum_pi xi(which) dpi`` (to_wp): (nrp,).  w_g+ is ``w('plus1')`` with the shapes in
        set 1 and the positions in set 2, w_++ ``w('plusplus')``, w_xx ``w('crosscross')``, the null test w_gx
        ``w('cross1')``"""
        return to_wp(self.xi(which), self.piedges)


def _no_shapes(pos2, ncol):
    """zeros for the columns of a second set that has none; None where pos2 has no length (_count says what is wrong)"""
    try:
        return numpy.zeros((len(pos2), ncol), dtype='f4')
    except TypeError:
        return None


def alignment_counts(pm, pos1, shape1, edges, pos2=None, shape2=None, weight1=None, weight2=None):
    """The position-shape and shape-shape sums of the rows in bins of r by the rule of the module docstring (mode 128):
    an AlignmentCounts.

    pm : ParticleMesh of 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos1, shape1 : (n, ndim) float64 or float32, device tensors or numpy arrays, this rank's rows and their orientation
        vectors (any number, none included), of any length but zero: a set declared with shapes whose rows include a
        zero or non-finite vector raises ValueError.
    edges : the nr + 1 edges of the bins of r, in box units.
    pos2, shape2 : the rows of a second set for the cross form, or None: the ordered pairs i != j of pos1, and shape2
        must then be None.  pos2 without shape2 is a set of positions only: it brings zeros, and ``omega_de`` and ``eta``
        are None.
    weight1, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.

    Argument errors are raised on every rank together.
    """
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('alignment counts on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    e = b = e2 = None
    if nd < 2:
        error = ValueError('alignment_counts needs a mesh of two or three dimensions, not %d' % nd)
    else:
        e, _, error = _binning(nd, edges, '1d', None, None, None, None, 2)
    if error is None:
        error = too_many(e, None, MAX_BINS, '(PMX_PAIRS_ALIGN_MAX_BINS)')
    if error is None:
        b = float(e[-1])
        e2 = e * e
    auto = pos2 is None
    both = auto or shape2 is not None
    cols2 = shape2 if both else _no_shapes(pos2, nd)
    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, '1d-align', 2, e2, None, b, error,
                                                       columns=('shape', shape1, cols2, nd, (True, both)))
    return AlignmentCounts(npairs, wnpairs, list(rsum.reshape(4, -1)), e, None, None, '1d', 2, auto, W1, W2, W2sum, box,
                           ndim=nd, both=both)


def projected_alignment_counts(pm, pos1, ellip1, edges, pos2=None, ellip2=None, weight1=None, weight2=None,
                               piedges=None, pimax=None, los=2):
    """The sums of the projected ellipticity components in bins of (rp, pi) by the rule of the module docstring (mode
    130): a ProjectedAlignments.

    pm : ParticleMesh of three dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos1 : (n, 3), ellip1 : (n, 2) float64 or float32, device tensors or numpy arrays, this rank's rows and their
        ellipticities (g1, g2) in the plane normal to `los` (ellipticity_from_orientation makes them from 3-d axes).
        They must be finite; zero is a round shape.
    edges : the nrp + 1 edges of the bins of rp, in box units.
    pos2, ellip2 : the rows of a second set for the cross form, or None: the ordered pairs i != j of pos1, and ellip2
        must then be None.  pos2 without ellip2 is a set of positions only: it brings zeros.
    weight1, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.
    piedges, or pimax for bins of unit width in [0, pimax]; los : the axis of the line of sight (the conventions of
        pair_counts).

    Argument errors are raised on every rank together.
    """
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('alignment counts on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    b = e2 = None
    e, sub, error = _binning(nd, edges, 'projected', None, None, piedges, pimax, los)
    if error is None:
        error = too_many(e, sub, MAX_BINS, '(PMX_PAIRS_ALIGN_MAX_BINS)')
    if error is None:
        b = float(max(e[-1], sub[-1]))
        e2 = e * e
    auto = pos2 is None
    cols2 = ellip2 if auto or ellip2 is not None else _no_shapes(pos2, 2)
    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, 'projected-align', los, e2, sub,
                                                       b, error, columns=('ellipticity', ellip1, cols2, 2))
    shape = (len(e) - 1, len(sub) - 1)
    sums = [x.reshape(shape) for x in rsum.reshape(7, -1)]
    return ProjectedAlignments(npairs.reshape(shape), wnpairs.reshape(shape), sums, e, None, sub, 'projected', los, auto,
                               W1, W2, W2sum, box)


def ellipticity_from_orientation(vec, los=2, magnitude=1.0):
    """The spin-2 ellipticity of 3-d axes projected along the box axis `los`: an (n, 2) float64 device tensor ``(g1, g2)
    = |e| ((u_A^2 - u_B^2), 2 u_A u_B) / (u_A^2 + u_B^2)``, A < B the two axes other than `los`, u the rows of `vec`
    ((n, 3), device tensor or numpy array, of any length), ``|e|`` = `magnitude`, a number or (n,) of them.  Zeros where
    the projection vanishes: an axis along the line of sight looks round.  Torch arithmetic on the device."""
    if los not in (0, 1, 2):
        raise ValueError('los must be 0, 1 or 2, not %r' % (los,))
    dev = backend.get().device
    u = torch.as_tensor(vec).to(device=dev, dtype=torch.float64)
    if u.dim() != 2 or u.shape[1] != 3:
        raise ValueError('vec must have the shape (n, 3), not %s' % (tuple(u.shape),))
    A, B = [d for d in range(3) if d != los]
    ua, ub = u[:, A], u[:, B]
    norm = ua * ua + ub * ub
    if not isinstance(magnitude, torch.Tensor):
        magnitude = torch.from_numpy(numpy.asarray(magnitude, dtype='f8'))
    mag = magnitude.to(device=dev, dtype=torch.float64)
    some = norm > 0
    safe = torch.where(some, norm, torch.ones_like(norm))
    g = torch.stack([(ua * ua - ub * ub) / safe, 2 * (ua * ub) / safe], dim=1) * mag.reshape(-1, 1)
    return torch.where(some[:, None], g, torch.zeros_like(g))
