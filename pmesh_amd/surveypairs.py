"""Pair counts of a survey catalogue with the line of sight of the pair itself, and the Landy-Szalay two-point
function from them, made on the device.

What nbodykit's ``SurveyDataPairCount``, ``SurveyData2PCF`` and ``AngularPairCount`` do on the host (Corrfunc's
``DDsmu_mocks``, ``DDrppi_mocks`` and ``DDtheta_mocks`` over the rows copied over PCIe): the partner in configuration
space of ``survey_multipoles``, for a cut-sky mock, a light cone, data plus randoms.  The counting is that of
pmesh_amd.paircount — the same entry of the C ABI (include/pmesh_amd.h: pmx_pair_counts), the same cell grid, the same
histogram — with two more modes whose kernels (csrc/pmx_pairs_survey.hip) choose the mu or pi bin of a pair from the
direction from the observer to the pair's midpoint instead of from a box axis.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).  Rules 1, 3, 6, 7 and 9 of
pmesh_amd.paircount stay: double arithmetic with every operation rounded once, squared edges, no square root choosing
a bin, exact ``npairs``, double sums in an unspecified order.  The new parts:

Observer.  The kernel knows one observer: the centre of the box, ``o_d = L_d / 2``.  For a pair of wrapped rows
``w_i``, ``w_j``: ``dx_d`` is as in pmesh_amd.paircount; ``l_d = (w_i,d + w_j,d) - L_d``, two roundings: twice the
midpoint's offset from the observer, of which only the direction matters.  ``p = dx_0 l_0 + dx_1 l_1 + dx_2 l_2``,
``l2 = l_0^2 + l_1^2 + l_2^2``, ``r2 = dx_0^2 + dx_1^2 + dx_2^2``, each sum taken in that order; ``p2 = p * p``.

``mode='2d'`` (PMX_PAIRS_2D_MIDPOINT, 3), bins of (s, mu).  The r-bin comes from ``q = r2`` as in the mode 2d of the
box.  ``t = r2 * l2``; the mu-bin is the number of k in 1 .. nsub - 1 with ``p2 >= sub[k] * t``, ``sub[k] =
muedges[k]^2``: no division.  A pair with ``t == 0`` goes to mu-bin 0: that covers ``r2 == 0``, and a pair symmetric
about the observer.  This is Corrfunc's ``DDsmu_mocks`` convention: ``mu^2 = (s.l)^2 / (s^2 l^2)``, ``l = (x1 + x2) /
2``.

``mode='projected'`` (PMX_PAIRS_PROJECTED_MIDPOINT, 4), bins of (rp, pi).  ``pi2 = p2 / l2``, or 0 where ``l2 == 0``;
``rp2 = r2 - pi2``, or 0 where that is negative.  The r-bin comes from ``q = rp2`` against ``e2``.  ``sub[k] =
piedges[k]^2``, squared on the host (the axis mode of the box passes ``piedges`` themselves); the pi-bin is the number
of k in 1 .. nsub - 1 with ``pi2 >= sub[k]``; a pair with ``pi2 >= sub[nsub]`` is not counted.  ``rsum`` adds ``w
sqrt(rp2)``.  This is Corrfunc's ``DDrppi_mocks``: ``pi = |s.l| / |l|``, ``rp^2 = s^2 - pi^2``.

Both modes need three dimensions and are symmetric under exchanging the two rows, so the auto form still counts every
unordered pair twice.

No wrap-around.  A survey is not periodic, but the grid, the routing and the minimum image are.  Every row must
therefore lie in ``[b / 2, L_d - b / 2)`` on every axis, after the shift below; ``b`` is the search radius.  Two rows
are then never closer through the boundary than ``b``, and no counted pair is a wrapped one.  ``b = edges[-1]`` in the
modes 1d, 2d and angular; in the projected mode ``b = hypot(edges[-1], piedges[-1])`` rounded up: the cylinder is not
aligned with the cells, so the walk over the cube of cells must cover its bounding sphere.  ``2 b <= min_d L_d``.

Observer elsewhere.  ``observer`` is in box coordinates, default the box centre.  Otherwise the rows are shifted once,
in double on the device: ``x' = (double)x + c_d`` with ``c_d = L_d / 2 - observer_d`` formed on the host; the shifted
rows are the rows of the rule.

``mode='1d'`` bins by s: the 1d kernel of the box after the shift and the padding check.

``mode='angular'`` bins by the angle between two rows as seen from the observer, through chords, as nbodykit's
``AngularPairCount`` does: ``u = (x - observer) / |x - observer|`` in double on the device (a row at the observer
raises ValueError), the rows become ``L / 2 + R u`` with ``R = min_d L_d / (2 + 2 sin(theta_max / 2)) * (1 - 2^-30)``,
and the 1d kernel counts them with ``e2[k] = (2 R sin(theta_k / 2))^2`` formed on the host: the bin is decided by
``r2`` against ``e2``.  ``thetaedges`` are in degrees, increasing, ``0 <= theta <= 180``.  ``rsum`` is divided by ``R``
on the host, ``edges`` are the chords ``2 sin(theta_k / 2)`` of the unit sphere, and ``theta = 2 asin(rmean / 2)`` in
degrees is the angle of the mean chord of a bin, not the mean angle.

    from pmesh_amd.surveypairs import survey_pair_counts, survey_correlation, to_poles, to_wp, sky_to_cartesian
    pos = sky_to_cartesian(ra, dec, distance) + observer           # a catalogue around an observer in the box
    pc = survey_pair_counts(pm, pos, edges, observer=observer, mode='2d', Nmu=100)
    xi, counts = survey_correlation(pm, data, randoms, edges, observer=observer, mode='2d', Nmu=100)
    xi_l = to_poles(xi, counts['D1D2'].muedges, [0, 2, 4])
"""
import math

import numpy
import torch

from . import backend
from ._cells import box_of
from .paircount import MAX_BINS, PairCounts, _binning, _count, _edges

MODES = ('1d', '2d', 'projected', 'angular')
KERNELS = {'1d': '1d', '2d': '2d-midpoint', 'projected': 'projected-midpoint', 'angular': '1d'}


class SurveyPairCounts(PairCounts):
    """A PairCounts with ``los = 'midpoint'`` and ``observer`` (box coordinates, a float64 numpy array); in the angular
    mode ``thetaedges`` (degrees), ``edges`` and ``rmean`` in chords of the unit sphere and ``theta``, the angle of the
    mean chord of every bin in degrees (nan where the bin holds no pair); None in the other modes."""

    def __init__(self, *args, **kw):
        self.observer = kw.pop('observer')
        self.thetaedges = kw.pop('thetaedges', None)
        PairCounts.__init__(self, *args, **kw)
        self.theta = None
        if self.thetaedges is not None:
            self.theta = torch.rad2deg(2 * torch.asin(torch.clamp(self.rmean / 2, max=1.0)))


def angular_radius(box, theta_max):
    """R of the angular mode: the radius of the sphere about the box centre on which the rows are put, such that the
    sphere and half the largest chord fit into the box"""
    return min(box) / (2 + 2 * math.sin(math.radians(theta_max) / 2)) * (1 - 2.0 ** -30)


def _survey_binning(nd, edges, mode, muedges, Nmu, piedges, pimax, thetaedges, box):
    """(edges, sub edges or None, e2, what the kernel gets as sub, b, R or None, error)"""
    none = (None,) * 6
    if nd != 3:
        return none + (ValueError('survey pair counts need a mesh of three dimensions, not %d' % nd),)
    if mode not in MODES:
        return none + (ValueError("mode must be '1d', '2d', 'projected' or 'angular', not %r" % (mode,)),)
    if mode == 'angular':
        th, error = _edges(thetaedges, 'thetaedges')
        if error is None and th[-1] > 180:
            error = ValueError('thetaedges must be increasing and finite, at least two of them, within 0 .. 180 degrees')
        if error is None and len(th) - 1 > MAX_BINS:
            error = ValueError('%d bins: at most %d (PMX_PAIRS_MAX_BINS)' % (len(th) - 1, MAX_BINS))
        if error is not None:
            return none + (error,)
        R = angular_radius(box, th[-1])
        half = numpy.sin(numpy.radians(th) / 2)
        chord = 2 * R * half
        e2 = chord * chord
        if not (numpy.diff(e2) > 0).all():
            return none + (ValueError('thetaedges are too close: their chords do not increase'),)
        return 2 * half, None, e2, None, float(chord[-1]), R, None
    e, sub, error = _binning(nd, edges, mode, muedges, Nmu, piedges, pimax, 2)
    if error is not None:
        return none + (error,)
    b = float(e[-1])
    if mode == 'projected':
        b = float(numpy.nextafter(numpy.hypot(e[-1], sub[-1]), numpy.inf))
    return e, sub, e * e, None if sub is None else sub * sub, b, None, None


def _observer(observer, box):
    """(the observer as a float64 array, error)"""
    if observer is None:
        return numpy.asarray(box, dtype='f8') / 2, None
    try:
        o = numpy.array(observer, dtype='f8')
    except (TypeError, ValueError):
        return None, ValueError('observer must be three numbers')
    if o.shape != (3,) or not numpy.isfinite(o).all():
        return None, ValueError('observer must be three finite numbers, in box coordinates')
    return o, None


def _preparation(comm, box, b, observer, obs, mode='1d', R=None):
    """The `prepare` step of paircount._count for rows about an observer: the shift of the rows that puts `obs` (the
    observer as an array; `observer`: what the caller passed, None for the box centre) at the box centre, in the angular
    mode the rows on the sphere of radius R, and the check that every row lies in [b / 2, L_d - b / 2); it raises on
    every rank together."""

    def _prepare(p1, p2):
        L = torch.tensor(box, dtype=torch.float64, device=p1.device)
        centre = L / 2
        shift = None
        if observer is not None:
            shift = torch.from_numpy(numpy.asarray(box, dtype='f8') / 2 - obs).to(p1.device)
        out, at_observer = [], 0
        lo, hi = numpy.full(3, numpy.inf), numpy.full(3, -numpy.inf)
        for p in (p1, p2):
            if p is None:
                out.append(None)
                continue
            x = p
            if mode == 'angular':
                d = p.to(torch.float64) - (centre if observer is None else torch.from_numpy(obs).to(p1.device))
                norm = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
                at_observer += int((norm == 0).sum())
                x = centre + R * (d / norm[:, None])
            elif shift is not None:
                x = p.to(torch.float64) + shift
            if x.shape[0]:
                lo = numpy.minimum(lo, x.min(dim=0)[0].cpu().numpy())
                hi = numpy.maximum(hi, x.max(dim=0)[0].cpu().numpy())
            out.append(x)
        if comm.size > 1:
            at_observer = int(comm.allreduce(at_observer))
            lo, hi = comm.allreduce(lo, op='min'), comm.allreduce(hi, op='max')
        if at_observer:
            raise ValueError('%d rows lie at the observer: they have no direction' % at_observer)
        for d in range(3):
            if lo[d] <= hi[d] and not (lo[d] >= b / 2 and hi[d] < box[d] - b / 2):
                need = 2 * max(box[d] / 2 - lo[d], hi[d] - box[d] / 2) + b
                raise ValueError('rows lie outside [b / 2, L - b / 2) = [%r, %r) along axis %d, %r .. %r about an '
                                 'observer at the centre: pairs would be counted through the periodic boundary.  A '
                                 'BoxSize of more than %r along axis %d holds them'
                                 % (b / 2, box[d] - b / 2, d, float(lo[d]), float(hi[d]), float(need), d))
        return out[0], out[1]
    return _prepare


def survey_pair_counts(pm, pos1, edges, observer=None, pos2=None, weight1=None, weight2=None, mode='1d', muedges=None,
                       Nmu=None, piedges=None, pimax=None, thetaedges=None):
    """The binned pair counts of the rows by the rule of the module docstring: a SurveyPairCounts.

    pm : ParticleMesh of three dimensions; its BoxSize is the volume that holds the survey, its communicator the ranks.
    pos1 : (n, 3) float64 or float32, device tensor or numpy array, this rank's rows (any number, none included).
    edges : the nr + 1 edges of the bins of s (of rp in the projected mode), in box units; ignored in the angular mode.
    observer : three numbers in box coordinates, or None: the centre of the box.
    pos2 : the rows of a second set for the cross counts, or None: the ordered pairs i != j of pos1.
    weight1, weight2 : (n,) float rows, or None for 1.  weight2 needs pos2.
    mode : '1d', '2d', 'projected' or 'angular'.  muedges, or Nmu for Nmu uniform bins of mu in [0, 1]; piedges, or
        pimax for bins of unit width in [0, pimax]; thetaedges in degrees: nbodykit's conventions.

    Argument errors, a row outside ``[b / 2, L_d - b / 2)`` and a row at the observer (angular) raise on every rank
    together.
    """
    nd = len(pm.Nmesh)
    box = box_of(pm)
    e, sub, e2, given, b, R, error = _survey_binning(nd, edges, mode, muedges, Nmu, piedges, pimax, thetaedges, box)
    obs = None
    if error is None:
        obs, error = _observer(observer, box)
    prepare = _preparation(pm.comm, box, b, observer, obs, mode, R)

    npairs, wnpairs, rsum, W1, W2, W2sum, box = _count(pm, pos1, pos2, weight1, weight2, KERNELS.get(mode), 2, e2,
                                                       given, b, error, prepare)
    if mode == 'angular':
        rsum = rsum / R
    shape = (len(e) - 1,) if sub is None else (len(e) - 1, len(sub) - 1)
    return SurveyPairCounts(npairs.reshape(shape), wnpairs.reshape(shape), rsum.reshape(shape), e,
                            sub if mode == '2d' else None, sub if mode == 'projected' else None, mode, 'midpoint',
                            pos2 is None, W1, W2, W2sum, box, observer=obs,
                            thetaedges=numpy.array(thetaedges, dtype='f8') if mode == 'angular' else None)


def _normalised(pc):
    """wnpairs over the weighted number of pairs of the two sets: W_X W_Y, less sum w^2 where X is Y"""
    return pc.wnpairs / (pc.W1 * pc.W2 - pc.W2sum)


def survey_correlation(pm, data1, randoms1, edges, observer=None, data2=None, randoms2=None, data_weight1=None,
                       randoms_weight1=None, data_weight2=None, randoms_weight2=None, R1R2=None, mode='1d',
                       muedges=None, Nmu=None, piedges=None, pimax=None, thetaedges=None):
    """(xi, counts): the Landy-Szalay estimator on normalised counts, nbodykit's ``SurveyData2PCF``:

        xi = (nD1D2 - nD1R2 - nD2R1 + nR1R2) / nR1R2,    nXY = wnpairs_XY / (W_X W_Y - [X is Y] sum w^2)

    a float64 device tensor of the shape of the counts, nan where the R1R2 bin is empty, and ``counts``, a dict of the
    SurveyPairCounts 'D1D2', 'D1R2', 'D2R1' and 'R1R2'.  Without ``data2`` it is the auto form: the second sets are the
    first ones, and D2R1 is D1R2, counted once.  With ``data2``, ``randoms2`` is needed.  ``R1R2`` may be passed in: the
    SurveyPairCounts of an earlier call on the same randoms and bins.  The other arguments are those of
    survey_pair_counts.  The estimator is host arithmetic on nbins numbers."""
    cross = data2 is not None
    if cross and randoms2 is None:
        raise ValueError('data2 needs randoms2')
    if not cross and (randoms2 is not None or data_weight2 is not None or randoms_weight2 is not None):
        raise ValueError('randoms2 and the weights of the second sets need data2')
    if R1R2 is not None and not isinstance(R1R2, PairCounts):
        raise TypeError('R1R2 must be the SurveyPairCounts of survey_pair_counts')
    kw = dict(observer=observer, mode=mode, muedges=muedges, Nmu=Nmu, piedges=piedges, pimax=pimax,
              thetaedges=thetaedges)
    counts = {}
    counts['D1D2'] = survey_pair_counts(pm, data1, edges, pos2=data2, weight1=data_weight1, weight2=data_weight2, **kw)
    counts['D1R2'] = survey_pair_counts(pm, data1, edges, pos2=randoms2 if cross else randoms1, weight1=data_weight1,
                                        weight2=randoms_weight2 if cross else randoms_weight1, **kw)
    if cross:
        counts['D2R1'] = survey_pair_counts(pm, data2, edges, pos2=randoms1, weight1=data_weight2,
                                            weight2=randoms_weight1, **kw)
    else:
        counts['D2R1'] = counts['D1R2']
    if R1R2 is None:
        R1R2 = survey_pair_counts(pm, randoms1, edges, pos2=randoms2, weight1=randoms_weight1,
                                  weight2=randoms_weight2, **kw)
    elif tuple(R1R2.npairs.shape) != tuple(counts['D1D2'].npairs.shape):
        raise ValueError('R1R2 has the bins %s, the counts %s' % (tuple(R1R2.npairs.shape),
                                                                   tuple(counts['D1D2'].npairs.shape)))
    counts['R1R2'] = R1R2
    dd, dr, rd, rr = (_normalised(counts[k]) for k in ('D1D2', 'D1R2', 'D2R1', 'R1R2'))
    filled = R1R2.npairs > 0
    xi = (dd - dr - rd + rr) / torch.where(filled, rr, torch.ones_like(rr))
    return torch.where(filled, xi, torch.full_like(xi, float('nan'))), counts


def _legendre(l, x):
    c = numpy.zeros(l + 1)
    c[l] = 1.0
    return numpy.polynomial.legendre.legval(x, c)


def to_poles(xi, muedges, poles):
    """The multipoles of xi(s, mu): ``(2 l + 1) sum_mu xi P_l(mu_mid) dmu`` for every l of `poles`, mu_mid the middle
    of a mu bin: (nr, len(poles)), a tensor where xi is one, else a numpy array.  mu runs over [0, 1]: odd l are not
    zero here and mean nothing for a pair-symmetric xi."""
    mu = numpy.asarray(muedges, dtype='f8')
    mid, dmu = (mu[1:] + mu[:-1]) / 2, numpy.diff(mu)
    m = numpy.stack([(2 * l + 1) * _legendre(int(l), mid) * dmu for l in poles], axis=1)      # (nmu, npoles)
    if isinstance(xi, torch.Tensor):
        return (xi[:, :, None] * torch.from_numpy(m).to(xi.device)[None, :, :]).sum(dim=1)
    return (numpy.asarray(xi)[:, :, None] * m[None, :, :]).sum(axis=1)


def to_wp(xi, piedges):
    """The projected function of xi(rp, pi): ``2 sum_pi xi dpi``: (nrp,), a tensor where xi is one"""
    dpi = numpy.diff(numpy.asarray(piedges, dtype='f8'))
    if isinstance(xi, torch.Tensor):
        return 2 * (xi * torch.from_numpy(dpi).to(xi.device)[None, :]).sum(dim=1)
    return 2 * (numpy.asarray(xi) * dpi[None, :]).sum(axis=1)


def sky_to_cartesian(ra, dec, distance, degrees=True):
    """(n, 3) float64 rows on the device about an observer at the origin: ``x = d cos(dec) cos(ra)``, ``y = d cos(dec)
    sin(ra)``, ``z = d sin(dec)``.  ra, dec, distance: (n,) device tensors or numpy arrays; angles in degrees unless
    ``degrees=False``.  Add the observer's box coordinates to place the rows in a box."""
    dev = backend.get().device
    cols = []
    for what, x in (('ra', ra), ('dec', dec), ('distance', distance)):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(numpy.ascontiguousarray(x, dtype='f8'))
        t = t.to(dev).to(torch.float64).reshape(-1)
        cols.append(t)
    ra, dec, d = cols
    if not (ra.shape == dec.shape == d.shape):
        raise ValueError('ra, dec and distance must have one length')
    if degrees:
        ra, dec = torch.deg2rad(ra), torch.deg2rad(dec)
    c = d * torch.cos(dec)
    return torch.stack([c * torch.cos(ra), c * torch.sin(ra), d * torch.sin(dec)], dim=1)
