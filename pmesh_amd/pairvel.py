"""Pairwise velocity statistics of particles, made on the device.

What halotools does on the host as ``mean_radial_velocity_vs_r``, ``radial_pvd_vs_r``, ``mean_los_velocity_vs_rp`` and
``los_pvd_vs_rp``, and the pairwise estimator of Ferreira et al. (1999) that Hand et al. (2012) used for the kSZ
signal: the mean pairwise (infall) velocity v12(r), the pairwise dispersions parallel and transverse to the pair, the
line-of-sight pairwise velocity and its dispersion in bins of (rp, pi) — the input of the streaming model of
redshift-space distortions — for the rows and velocities of ``lognormal_catalog(displacement=True)``, of an N-body run
or of ``fof_catalog`` (``CMVelocity``), without leaving HBM.  None of them is a weighted ``pair_counts``: the quantity
summed depends on the pair, not on a product of per-row weights.  No entry of the C ABI is added: ``pmx_pair_counts``
(include/pmesh_amd.h) has three more modes, PMX_PAIRS_1D_VELOCITY (7), PMX_PAIRS_PROJECTED_VELOCITY (8) and
PMX_PAIRS_1D_LOS (9), whose kernels are in csrc/pmx_pairs_vel.hip.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

Shared with the base modes, unchanged.  Mode 7 shares everything below with PMX_PAIRS_1D (``'1d'`` of
pmesh_amd.paircount), mode 8 with PMX_PAIRS_PROJECTED (``'projected'``), mode 9 with PMX_PAIRS_1D: rows, wrapping, the
minimum image ``dx_d`` (primary minus secondary), ``r2``, ``q``, the squared edges, the r-bin, the pi-bin and the pimax
cut; all arithmetic in double; every operation rounded once, no contraction; no square root chooses a bin.  ``npairs``
in these modes equals ``npairs`` of the corresponding base mode on the same arguments, to the last count.

Per-row columns.  Both sets bring a block of columns in row order, float or double: ``(w, v_0 .. v_{ndim-1})`` in the
modes 7 and 8, ``(w, s)`` in the mode 9.  The host packs them as one contiguous ``(n, ncol)`` tensor (w = 1 without a
weight), so a pair's read of a secondary row is one 16- or 32-byte piece.

Outputs.  ``npairs`` and ``wnpairs`` have ``nr * nsub`` entries, as in the base modes.  ``rsum`` has ``4 * nr * nsub``
entries, ``rsum[m * nbins + b]``: m = 0 is ``sum w sqrt(q)``, as in the base modes; m = 1, 2, 3 are the three sums
``S1``, ``S2``, ``S3`` below.  The order of the double sums is unspecified; ``npairs`` is exact.

Per counted pair, with ``w = w1_i * w2_j``:

Mode 7 (``pairwise_velocities(mode='1d')``), ndim 1 to 3.  ``dv_d = v_i,d - v_j,d``.  ``h = dx_0 dv_0 + dx_1 dv_1 +
dx_2 dv_2`` and ``dv2 = dv_0^2 + dv_1^2 + dv_2^2``, each summed in that order over ``d < ndim``.  ``r = sqrt(r2)``.
``u = h / r`` where ``r2 > 0``, else 0.  ``S1 += (w u)``, ``S2 += (w u) u``, ``S3 += w dv2``.  u is the radial pairwise
velocity.  Negative means the pair approaches.

Mode 8 (``pairwise_velocities(mode='projected')``), ndim 3, ``los`` in {0, 1, 2}.  ``u = dx_los < 0 ? -dv_los :
dv_los``.  ``S1``, ``S2``, ``S3`` as above, with ``dv2`` over all three axes.  The m = 0 sum adds ``w sqrt(rp2)``, as
PMX_PAIRS_PROJECTED does.

Mode 9 (``pairwise_los``), ndim 3.  ``los`` is ignored.  The observer is at ``o_d = 0.5 * L_d``, as in the midpoint
modes of pmesh_amd.surveypairs, and the rows are kept in ``[b/2, L_d - b/2)`` as for them.  ``a_d = w_i,d - o_d`` and
``b_d = w_j,d - o_d``, where ``w_i``, ``w_j`` are the wrapped rows.  ``a2``, ``b2``, ``pa = dx·a`` and ``pb = dx·b`` are
each summed over d = 0, 1, 2 in order.  ``ta = a2 > 0 ? pa / sqrt(a2) : 0``; ``tb`` likewise.  ``c = r2 > 0 ? 0.5 * ((ta
+ tb) / r) : 0``.  ``ds = s_i - s_j``.  ``S1 += (w c) ds``, ``S2 += (w c) c``, ``S3 += (w ds) ds``.

Consequences.  A self pair (one set passed as both) has ``r2 == 0``, ``dv == 0`` and ``ds == 0``, so it adds nothing to
``S1 .. S3``; the host subtracts the self pairs from ``npairs[0]`` and ``wnpairs[0]`` exactly as pmesh_amd.paircount
does.  Each statistic is even under exchanging the two rows, so the auto form counts every unordered pair twice,
consistently in the numerator and the denominator.  ``nr * nsub`` is at most PMX_PAIRS_VELOCITY_MAX_BINS (1024); more
raise ValueError.  The search radius, the finiteness of the rows and the ranks are those of pmesh_amd.paircount (rules
8 and the routing there); velocity rows and scalars must be finite as well.

    from pmesh_amd.pairvel import pairwise_velocities, pairwise_los
    pv = pairwise_velocities(pm, pos, vel, edges)                  # auto, bins of r
    pv.v12, pv.sigma_par, pv.sigma_perp, pv.rmean
    pv = pairwise_velocities(pm, pos, vel, edges, mode='projected', pimax=40)   # (rp, pi): pv.v12 is v_los(rp, pi)
    ks = pairwise_los(pm, pos, T, edges, observer=obs)             # ks.v12 = num / den; the kSZ momentum is -ks.v12
"""
import torch

from . import _abi
from ._cells import box_of
from .paircount import PairCounts, _binning, _count, too_many
from .surveypairs import _observer, _preparation

MAX_BINS = _abi.PMX_PAIRS_VELOCITY_MAX_BINS
KERNELS = {'1d': '1d-velocity', 'projected': 'projected-velocity'}


def _ratio(num, den, filled):
    """num / den where `filled`, nan elsewhere"""
    return torch.where(filled, num / torch.where(filled, den, torch.ones_like(den)), torch.full_like(num, float('nan')))


class PairwiseVelocities(PairCounts):
    """A PairCounts with the sums of the rule, device tensors of the shape of the counts, identical on every rank:
    ``vsum`` (S1), ``v2sum`` (S2), ``dv2sum`` (S3); and derived from them, nan where a bin holds no pair: ``v12 = vsum
    / wnpairs``, the mean pairwise velocity (radial in the mode 1d, along the line of sight in the projected mode);
    ``sigma_par = sqrt(v2sum / wnpairs - v12^2)``, its dispersion; ``sigma_perp = sqrt((dv2sum - v2sum) / ((ndim - 1)
    wnpairs))``, the dispersion per transverse axis (None for ndim 1).  A variance that the roundings of the sums left
    below zero counts as zero.  ``ndim``."""

    def __init__(self, npairs, wnpairs, sums, *args, **kw):
        self.ndim = kw.pop('ndim')
        PairCounts.__init__(self, npairs, wnpairs, sums[0], *args, **kw)
        self.vsum, self.v2sum, self.dv2sum = sums[1], sums[2], sums[3]
        filled = npairs > 0
        self.v12 = _ratio(self.vsum, wnpairs, filled)
        self.sigma_par = torch.sqrt(torch.clamp(_ratio(self.v2sum, wnpairs, filled) - self.v12 * self.v12, min=0))
        self.sigma_perp = None
        if self.ndim > 1:
            self.sigma_perp = torch.sqrt(torch.clamp(_ratio(self.dv2sum - self.v2sum, (self.ndim - 1) * wnpairs,
                                                            filled), min=0))


class PairwiseLOS(PairCounts):
    """A PairCounts with ``los = 'observer'``, ``observer`` (box coordinates, a float64 numpy array) and the sums of
    the rule, device tensors of the shape (nr,), identical on every rank: ``num`` (S1), ``den`` (S2), ``ds2sum`` (S3);
    and ``v12 = num / den``, nan where the bin holds no pair or ``den == 0``."""

    def __init__(self, npairs, wnpairs, sums, *args, **kw):
        self.observer = kw.pop('observer')
        PairCounts.__init__(self, npairs, wnpairs, sums[0], *args, **kw)
        self.num, self.den, self.ds2sum = sums[1], sums[2], sums[3]
        self.v12 = _ratio(self.num, self.den, (npairs > 0) & (self.den != 0))


def pairwise_velocities(pm, pos1, vel1, edges, pos2=None, vel2=None, weight1=None, weight2=None, mode='1d',
                        piedges=None, pimax=None, los=2):
    """The pairwise velocity sums of the rows by the rule of the module docstring: a PairwiseVelocities.

    pm : ParticleMesh of 1, 2 or 3 dimensions; its BoxSize is the periodic box, its communicator the ranks.
    pos1, vel1 : (n, ndim) float64 or float32, device tensors or numpy arrays, this rank's rows and their velocities
        (any number, none included).  Velocity rows must be finite and of the length of their positions.
    edges : the nr + 1 edges of the bins of r (of rp in the projected mode), in box units.
    pos2, vel2 : the rows of a second set for the cross form, or None: the ordered pairs i != j of pos1.  vel2 needs
        pos2, and pos2 vel2.
    weight1, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.
    mode : '1d' (the radial pairwise velocity in bins of r) or 'projected' (the pairwise velocity along the axis `los`
        in bins of (rp, pi)).  piedges, or pimax for bins of unit width in [0, pimax]; los : the axis of the line of
        sight (the conventions of pair_counts).

    Argument errors are raised on every rank together.
    """
    nd = len(pm.Nmesh)
    if nd > _abi.PMX_MAXDIM:
        raise NotImplementedError('pairwise velocities on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    e = sub = b = e2 = None
    if mode not in KERNELS:
        error = ValueError("mode must be '1d' or 'projected', not %r" % (mode,))
    else:
        e, sub, error = _binning(nd, edges, mode, None, None, piedges, pimax, los)
    if error is None:
        error = too_many(e, sub, MAX_BINS, '(PMX_PAIRS_VELOCITY_MAX_BINS)')
    if error is None:
        b = float(max(e[-1], sub[-1])) if mode == 'projected' else float(e[-1])
        e2 = e * e
    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, KERNELS.get(mode), los, e2, sub,
                                                       b, error, columns=('vel', vel1, vel2, nd))
    shape = (len(e) - 1,) if sub is None else (len(e) - 1, len(sub) - 1)
    sums = [x.reshape(shape) for x in rsum.reshape(4, -1)]
    return PairwiseVelocities(npairs.reshape(shape), wnpairs.reshape(shape), sums, e, None, sub, mode, los,
                              pos2 is None, W1, W2, W2sum, box, ndim=nd)


def pairwise_los(pm, pos1, s1, edges, observer=None, pos2=None, s2=None, weight1=None, weight2=None):
    """The pairwise estimator of Ferreira et al. (1999) for one line-of-sight scalar per row, by the rule of the module
    docstring (mode 9): a PairwiseLOS with ``v12 = num / den``, ``num = sum w c_ij (s_i - s_j)``, ``den = sum w
    c_ij^2`` and ``c_ij = r_ij . (n_i + n_j) / (2 r_ij)``, n the unit vector from the observer to a row.

    With ``s`` the line-of-sight peculiar velocity of every row, positive away from the observer, ``v12`` estimates the
    mean pairwise velocity v12(r), negative for infall.  With ``s = T``, the kSZ temperature of every row, the pairwise
    momentum of Hand et al. (2012) is ``-v12``: their estimator carries the opposite sign.

    pm : ParticleMesh of three dimensions; its BoxSize is the volume that holds the survey, its communicator the ranks.
    pos1 : (n, 3), s1 : (n,), float64 or float32, device tensors or numpy arrays, this rank's rows (any number, none
        included).  The scalars must be finite.
    edges : the nr + 1 edges of the bins of r, in box units.
    observer : three numbers in box coordinates, or None: the centre of the box.  The rows are shifted and checked as
        survey_pair_counts does: after the shift every row must lie in ``[b / 2, L_d - b / 2)``, ``b = edges[-1]``.
    pos2, s2 : the rows of a second set for the cross form, or None.  weight1, weight2 : (n,) float rows, or None.

    Argument errors and a row outside ``[b / 2, L_d - b / 2)`` raise on every rank together.
    """
    nd = len(pm.Nmesh)
    box = box_of(pm)
    e = b = e2 = obs = None
    if nd != 3:
        error = ValueError('pairwise_los needs a mesh of three dimensions, not %d' % nd)
    else:
        e, _, error = _binning(nd, edges, '1d', None, None, None, None, 2)
    if error is None:
        error = too_many(e, None, MAX_BINS, '(PMX_PAIRS_VELOCITY_MAX_BINS)')
    if error is None:
        obs, error = _observer(observer, box)
    if error is None:
        b = float(e[-1])
        e2 = e * e
    prepare = _preparation(pm.comm, box, b, observer, obs)
    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, '1d-los', 2, e2, None, b, error,
                                                       prepare, columns=('s', s1, s2, 1))
    return PairwiseLOS(npairs, wnpairs, list(rsum.reshape(4, -1)), e, None, None, '1d', 'observer', pos2 is None, W1,
                       W2, W2sum, box, observer=obs)
