"""Pair counts by row labels, made on the device: the delete-one jackknife of the two-point function and its covariance
in one walk over the pairs, and the one-halo / two-halo split.

What halotools does on the host as ``tpcf_jackknife`` and ``tpcf_one_two_halo_decomp``, and pycorr's jackknife
estimators.  A delete-one jackknife over K regions otherwise takes K + 1 weighted ``pair_counts`` calls with 0 / 1
weights, K + 1 walks over the same pairs; and "the two rows carry the same host id" is not a product of per-row
weights, so no weighted call counts it at all.  Both are one capability of the kernel: the bin of a pair depends on an
integer label of each of its two rows.  No entry of the C ABI is added: ``pmx_pair_counts`` (include/pmesh_amd.h) has
two flags above its base modes, PMX_PAIRS_SPLIT (16) and PMX_PAIRS_JACKKNIFE (32), whose kernels are in
csrc/pmx_pairs_labels.hip.

The rule (normative; include/pmesh_amd.h restates it next to the entry point).

1. Modes.  The valid modes are ``16 | m`` and ``32 | m``, m one of the base modes 0 to 4: ``'1d'``, ``'2d'`` and
   ``'projected'`` of pmesh_amd.paircount, ``'2d'`` and ``'projected'`` of pmesh_amd.surveypairs (the line of sight of
   the pair itself).  Rows, wrapping, the minimum image, ``r2``, ``q``, the squared edges, the r-, mu- and pi-bin and the
   pimax cut are exactly those of the base mode, ndim 1 to 3 for 1d and three dimensions otherwise.  Summed over its
   label classes, ``npairs`` of a label mode equals ``npairs`` of the base mode on the same arguments, to the last count.
2. Columns.  Both sets bring the block ``(w, label)`` in row order, float or double: the host packs it as one contiguous
   ``(n, 2)`` tensor, w = 1 without a weight, float64 whenever a label exceeds 2^24 or the weight is float64.  A label
   is a non-negative integer value held exactly in the column's type.  A label that is negative, not finite, or out of
   range for the call is "no label": the kernel tests it with a comparison that is false for NaN; such a row never
   indexes anything and is never "the same" as any row.
3. Split (16 | m), ``nbins = nr * nsub <= 1024``.  With ``kind = (a == c and a is a label) ? 1 : 0``, per counted pair of
   weight ``w = w1_i * w2_j`` in bin b: ``npairs[kind * nbins + b] += 1``, ``wnpairs[...] += w``, ``rsum[...] += w *
   sqrt(q)``.  All three arrays have ``2 * nbins`` entries.
4. Jackknife (32 | m).  ``K = (PMX_PAIRS_LABEL_SLOTS / nbins - 2) / 2`` in integer division, PMX_PAIRS_LABEL_SLOTS =
   4096; K >= 1, that is ``nbins <= 1024``.  A label is in range when it is below K.  ``npairs`` and ``wnpairs`` have
   ``(1 + 2 K) * nbins`` entries, in blocks of nbins: block 0 is ``all``, block 1 + k is ``side[k]``, block 1 + K + k is
   ``same[k]``; ``rsum`` has nbins entries and covers ``all`` only.  Per counted pair in bin b, with labels a (primary)
   and c (secondary): all[b] gets (1, w, w sqrt(q)); if a is in range, side[a][b] gets (1, w); if c is in range,
   side[c][b] gets (1, w), so a pair with a == c adds 2 and 2w (w + w, exact); if a == c and in range, same[a][b] gets
   (1, w).
5. Sums.  ``npairs`` is exact and depends on no decomposition or launch; the order of the double sums is unspecified, as
   in the base modes.
6. Self pairs.  The entry knows no row identity.  A self pair has ``r2 == 0`` and a == c; in the auto form with
   ``edges[0] == 0`` the host removes it from bin (0, 0): from ``same`` of the split (``different`` for a row without a
   label); from ``all``, twice from ``side[a]`` and once from ``same[a]`` of the jackknife.
7. More labels than K.  ``nlab > K`` takes ``ceil(nlab / K)`` calls, each with the labels of its chunk shifted to
   ``[0, K)`` and the rest set to -1; ``all`` is taken from the first call.  The search radius, the finiteness of the
   rows and the ranks are those of pmesh_amd.paircount (rule 8 and the routing there).

From the three sums every delete-one realisation follows, in any cross-pair weighting: with ``cross_k = side_k - 2
same_k``, the pairs with exactly one end in region k, ``wnpairs_k = total - same_k - alpha * cross_k``; ``alpha = 1`` is
the standard delete-one, any other alpha (Mohammad & Percival 2021) is arithmetic on the same arrays.

    from pmesh_amd.pairlabels import box_regions, pair_correlation_jackknife, pair_counts_split
    lab = box_regions(pm, pos, 4)                                  # 64 cuboid regions
    jk = pair_correlation_jackknife(pm, pos, lab, edges, 64)       # jk.xi, jk.cov, jk.error
    sc = pair_counts_split(pm, pos, fof(pm, pos, 0.2, absolute=False).minid, edges)   # sc.same, sc.different, sc.total
"""
import numpy
import torch

from . import _abi, backend
from ._arrays import to_device
from ._cells import allsum, box_of, rows, together
from .paircount import LABEL_SLOTS, PairCounts, _binning, _count, bin_volumes, label_slots, too_many
from .surveypairs import KERNELS as SURVEY_KERNELS
from .surveypairs import SurveyPairCounts, _observer, _preparation, _survey_binning

MAX_BINS = LABEL_SLOTS // 4
EXACT = 2 ** 53                                  # the largest label a float64 column holds with all below it
EXACT32 = 2 ** 24                                # and a float32 column


class SplitCounts(object):
    """``same`` (pairs of two rows of one label: the one-halo term), ``different`` (all others: the two-halo term) and
    ``total``, their sum: PairCounts of the base mode, identical on every rank."""

    def __init__(self, same, different, total):
        self.same, self.different, self.total = same, different, total


class JackknifeCounts(object):
    """The sums of a delete-one jackknife over ``nlab`` labels, identical on every rank.

    ``total``: the PairCounts (SurveyPairCounts about an observer) that the unlabelled call returns.  ``side_npairs``
    (int64), ``side_wnpairs``: per label the pairs with an end in it, a pair with both ends in it twice; ``same_npairs``,
    ``same_wnpairs``: per label the pairs with both ends in it; device tensors of the shape (nlab, *bins).  ``W1_k``,
    ``W2_k``, ``W2sum_k``: the sums of the weights of the rows of every label in the two sets and (auto; cross: 0) of
    their squares, float64 numpy arrays of nlab entries.  ``ncalls``: the calls of the kernel it took."""

    def __init__(self, total, side_npairs, side_wnpairs, same_npairs, same_wnpairs, W1_k, W2_k, W2sum_k, ncalls):
        self.total = total
        self.side_npairs, self.side_wnpairs = side_npairs, side_wnpairs
        self.same_npairs, self.same_wnpairs = same_npairs, same_wnpairs
        self.W1_k, self.W2_k, self.W2sum_k = W1_k, W2_k, W2sum_k
        self.nlab, self.ncalls = len(W1_k), ncalls

    def norms(self, alpha=1.0):
        """norm_k of every label, a float64 numpy array: the expression of `realization` on the all-separation sums
        ``Nall = W1 W2 - [auto] W2sum``, ``Nsame_k = W1_k W2_k - [auto] W2sum_k`` and ``Nside_k = W1_k W2 + W1 W2_k -
        [auto] 2 W2sum_k``"""
        t = self.total
        n_all = t.W1 * t.W2 - t.W2sum
        n_same = self.W1_k * self.W2_k - self.W2sum_k
        n_side = self.W1_k * t.W2 + t.W1 * self.W2_k - 2 * self.W2sum_k
        return n_all - n_same - alpha * (n_side - 2 * n_same)

    def realizations(self, alpha=1.0):
        """(wnpairs_k of the shape (nlab, *bins), norm_k of nlab entries, both device tensors) of every label"""
        cross = self.side_wnpairs - 2 * self.same_wnpairs
        wn = self.total.wnpairs[None] - self.same_wnpairs - alpha * cross
        return wn, torch.from_numpy(self.norms(alpha)).to(wn.device)

    def realization(self, k, alpha=1.0):
        """(wnpairs_k, norm_k) of the sample without region k: ``cross_k = side_k - 2 same_k``, the pairs with exactly
        one end in k; ``wnpairs_k = total - same_k - alpha * cross_k``; norm_k the same expression on the
        all-separation sums (a float).  alpha = 1 is the standard delete-one."""
        cross = self.side_wnpairs[k] - 2 * self.same_wnpairs[k]
        return self.total.wnpairs - self.same_wnpairs[k] - alpha * cross, float(self.norms(alpha)[k])

    def realization_counts(self, k):
        """The PairCounts of the rows whose label is not k (alpha = 1), with exact integer ``npairs``.  ``rsum`` and
        ``rmean`` are those of all rows: the sums of r are not kept per label."""
        t = self.total
        npairs = t.npairs - self.side_npairs[k] + self.same_npairs[k]
        wnpairs = t.wnpairs - self.side_wnpairs[k] + self.same_wnpairs[k]
        return PairCounts(npairs, wnpairs, t.rsum, t.edges, t.muedges, t.piedges, t.mode, t.los, t.auto,
                          t.W1 - self.W1_k[k], t.W2 - self.W2_k[k], t.W2sum - self.W2sum_k[k], t.BoxSize)


class JackknifeCorrelation(object):
    """``xi`` of the full sample; ``realizations`` of the shape (nlab, *bins); ``mean``, their mean; ``cov``, over the
    flattened bins: ``(nlab - 1) / nlab * sum_k (x_k - mean)(x_k - mean)^T``; ``error``, the square root of its
    diagonal in the shape of the bins: float64 device tensors.  ``counts``: the JackknifeCounts they come from (a dict
    'D1D2', 'D1R2', 'D2R1', 'R1R2' of them with randoms).  ``alpha``."""

    def __init__(self, xi, realizations, counts, alpha):
        self.xi, self.realizations, self.counts, self.alpha = xi, realizations, counts, alpha
        nlab = realizations.shape[0]
        self.mean = realizations.mean(dim=0)
        d = (realizations - self.mean[None]).reshape(nlab, -1)
        self.cov = (nlab - 1) / float(nlab) * (d.t() @ d)
        self.error = torch.sqrt(torch.diagonal(self.cov)).reshape(self.mean.shape)


def box_regions(pm, pos, nsub):
    """int64 labels of the ``prod(nsub)`` cuboid sub-boxes of the wrapped rows, a device tensor of n entries.

    nsub: one integer for every axis, or one per axis.  The rule: the row is widened to double and wrapped into
    ``[0, L_d)`` as ``w = x - L_d floor(x / L_d)``; ``c_d = min(floor(w * nsub_d / L_d), nsub_d - 1)``, clamped at 0; the
    label is ``(c_0 * nsub_1 + c_1) * nsub_2 + c_2``: the last axis runs fastest.  A row with a coordinate that is not
    finite gets -1."""
    be = backend.get()
    nd = len(pm.Nmesh)
    pos, error = rows(pm, be, pos)
    ns = None
    if error is None:
        try:
            ns = numpy.broadcast_to(numpy.asarray(nsub, dtype='f8'), (nd,))
        except (TypeError, ValueError):
            pass
        if ns is None or not ((ns == numpy.floor(ns)) & (ns >= 1)).all():
            error = ValueError('nsub must be positive integers, one or one per axis')
    together(pm.comm, error)
    box = numpy.asarray(box_of(pm))
    x = pos.to(torch.float64)
    label = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    for d in range(nd):
        L, n = float(box[d]), int(ns[d])
        w = x[:, d] - L * torch.floor(x[:, d] / L)
        c = torch.clamp(torch.floor(torch.nan_to_num(w, nan=0.0, posinf=0.0, neginf=0.0) * n / L), 0, n - 1)
        label = label * n + c.to(torch.int64)
    return torch.where(torch.isfinite(x).all(dim=1), label, torch.full_like(label, -1))


# ---- the labels and their blocks ---------------------------------------------------------------------------------------

def _labels(be, x, what, n=None):
    """(the labels as an (n,) int64 tensor on the device, error)"""
    if x is None:
        return None, ValueError('%s is needed' % what)
    try:
        t, _ = to_device(x, be.device, what, allow_int=True)
    except TypeError as e:
        return None, e
    if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        return None, TypeError('%s must be integers, got %s' % (what, t.dtype))
    if t.dim() != 1:
        return None, ValueError('%s must have the shape (n,), not %s' % (what, tuple(t.shape)))
    if n is not None and t.shape[0] != n:
        return None, ValueError('%s must have %d rows, not %d' % (what, n, t.shape[0]))
    return t.to(be.device).to(torch.int64), None


def _read(pm, pos1, label1, pos2, label2, nlab, error):
    """(label1, label2 as int64 device tensors, the dtype of their columns, error) of the arguments of a public call:
    label2 is needed exactly with pos2; nlab None: any label (split), else labels must lie below it; negative: in
    nothing.  The largest label of all ranks decides the dtype, so that every rank packs the same block."""
    be = backend.get()
    comm = pm.comm
    l1 = l2 = None
    if error is None and nlab is not None and not (int(nlab) == nlab and 1 <= nlab < EXACT32):
        error = ValueError('nlab must be a positive integer below 2^24, not %r' % (nlab,))
    if error is None:
        l1, error = _labels(be, label1, 'label1', None if not hasattr(pos1, 'shape') else pos1.shape[0])
    if error is None and (label2 is None) != (pos2 is None):
        error = ValueError('label2 needs pos2' if pos2 is None else 'pos2 needs label2')
    if error is None and label2 is not None:
        l2, error = _labels(be, label2, 'label2', None if not hasattr(pos2, 'shape') else pos2.shape[0])
    top = -1
    if error is None:
        top = max([int(t.max()) for t in (l1, l2) if t is not None and t.numel()] + [-1])
        if top >= (EXACT if nlab is None else nlab):
            error = ValueError('labels must lie in [0, %s), or be negative for a row that is in nothing: found %d'
                               % ('2^53' if nlab is None else '%d' % nlab, top))
    # every rank learns of an error of any rank here, and of the largest label
    together(comm, error)
    if comm.size > 1:
        top = int(comm.allreduce(top, op='max'))
    return l1, l2, (torch.float32 if top <= EXACT32 else torch.float64), None


def _column(label, dtype, lo=None, hi=None):
    """the (n, 1) column of the labels: negative ones -1; with a chunk [lo, hi) those within it shifted to [0, hi - lo)
    and the rest -1"""
    if label is None:
        return None
    keep = label >= 0 if lo is None else (label >= lo) & (label < hi)
    shifted = label if lo is None else label - lo
    return torch.where(keep, shifted, torch.full_like(label, -1)).to(dtype).reshape(-1, 1)


def _weights(pm, weight, n, dev):
    """the weights of one set as an (n,) float64 device tensor (after _count has accepted them)"""
    if weight is None:
        return torch.ones(n, dtype=torch.float64, device=dev)
    t, _ = rows(pm, backend.get(), weight, 'weight', 1, n)
    return t.reshape(-1).to(torch.float64)


def _per_label(comm, label, w, nlab):
    """(the rows, the sum of w, the sum of w^2) of every label in [0, nlab) over all ranks: float64 numpy arrays (the
    rows counted in double: exact below 2^53)"""
    keep = (label >= 0) & (label < nlab)
    lab, w = label[keep], w[keep]
    out = torch.zeros((3, nlab), dtype=torch.float64, device=label.device)
    out[0].index_add_(0, lab, torch.ones_like(w))
    out[1].index_add_(0, lab, w)
    out[2].index_add_(0, lab, w * w)
    out = allsum(comm, out).cpu().numpy()
    return out[0], out[1], out[2]


class _Binning(object):
    """How one public call bins: what _count is given, and how a PairCounts of the base mode is made of three flat
    arrays"""

    def __init__(self, pm, edges, mode, muedges, Nmu, piedges, pimax, los, survey=False, observer=None,
                 thetaedges=None):
        nd = len(pm.Nmesh)
        if nd > _abi.PMX_MAXDIM:
            raise NotImplementedError('pair counts on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
        self.pm, self.mode, self.survey, self.nd = pm, mode, survey, nd
        self.box = box_of(pm)
        self.prepare = self.R = self.obs = self.thetaedges = None
        self.e = self.sub = self.e2 = self.given = self.b = None
        if survey:
            self.los = 2
            self.e, self.sub, self.e2, self.given, self.b, self.R, self.error = _survey_binning(
                nd, edges, mode, muedges, Nmu, piedges, pimax, thetaedges, self.box)
            if self.error is None:
                self.obs, self.error = _observer(observer, self.box)
            self.prepare = _preparation(pm.comm, self.box, self.b, observer, self.obs, mode, self.R)
            self.base = SURVEY_KERNELS.get(mode)
            if mode == 'angular' and self.error is None:
                self.thetaedges = numpy.array(thetaedges, dtype='f8')
        else:
            self.los = los
            self.e, self.sub, self.error = _binning(nd, edges, mode, muedges, Nmu, piedges, pimax, los)
            self.base = mode
            if self.error is None:
                self.b = float(max(self.e[-1], self.sub[-1])) if mode == 'projected' else float(self.e[-1])
                self.e2 = self.e * self.e
                self.given = self.sub * self.sub if mode == '2d' else self.sub
        if self.error is None:
            self.error = too_many(self.e, self.sub, MAX_BINS, 'in the modes by row labels (PMX_PAIRS_LABEL_SLOTS / 4)')
        if self.error is None:
            self.shape = (len(self.e) - 1,) if self.sub is None else (len(self.e) - 1, len(self.sub) - 1)
            self.nbins = int(numpy.prod(self.shape))

    def count(self, family, pos1, col1, pos2, col2, weight1, weight2, error=None):
        """_count in the label mode of this binning with the columns of the labels: the flat arrays with the self
        pairs left in, and the weight sums"""
        key = None if self.base is None else '%s-%s' % (family, self.base)
        return _count(self.pm, pos1, pos2, weight1, weight2, key, self.los, self.e2, self.given, self.b,
                      self.error if error is None else error, self.prepare, columns=('label', col1, col2, 1),
                      self_pairs=False)

    def counts(self, npairs, wnpairs, rsum, auto, W1, W2, W2sum):
        """the PairCounts of the base mode of three flat arrays of nbins entries"""
        if self.R is not None:
            rsum = rsum / self.R
        args = (npairs.reshape(self.shape), wnpairs.reshape(self.shape), rsum.reshape(self.shape), self.e,
                self.sub if self.mode == '2d' else None, self.sub if self.mode == 'projected' else None, self.mode)
        if self.survey:
            return SurveyPairCounts(*(args + ('midpoint', auto, W1, W2, W2sum, self.box)), observer=self.obs,
                                    thetaedges=self.thetaedges)
        return PairCounts(*(args + (self.los, auto, W1, W2, W2sum, self.box)))


# ---- the split ---------------------------------------------------------------------------------------------------------

def pair_counts_split(pm, pos1, label1, edges, pos2=None, label2=None, weight1=None, weight2=None, mode='1d',
                      muedges=None, Nmu=None, piedges=None, pimax=None, los=2):
    """The pair counts of the rows apart by "the two rows carry the same label" (rule 3 of the module docstring): a
    SplitCounts with ``same`` (the one-halo term), ``different`` (the two-halo term) and ``total``.

    label1, label2 : (n,) integers, device tensors or numpy arrays: the host id of every row.  A negative label means
        "in nothing": such a row is in the same host as no row, itself included.  Pass ``fof(...).minid`` (the smallest
        global row index of the group of every row), or ``where(labels > 0, labels, -1)`` of its ``labels`` to leave
        the rows of groups below nmin in nothing.  Labels lie below 2^53.  label2 is needed exactly with pos2.
    The other arguments are those of pair_counts.  At most 1024 bins.

    In the auto form the self pairs are removed from ``same``, or from ``different`` for the rows without a label, as
    pair_counts removes them.  Argument errors are raised on every rank together.
    """
    bn = _Binning(pm, edges, mode, muedges, Nmu, piedges, pimax, los)
    return _split(bn, pos1, label1, pos2, label2, weight1, weight2)


def _split(bn, pos1, label1, pos2, label2, weight1, weight2):
    pm = bn.pm
    auto = pos2 is None
    l1, l2, dtype, _ = _read(pm, pos1, label1, pos2, label2, None, bn.error)
    npairs, wnpairs, rsum, W1, W2, W2sum, _ = bn.count('split', pos1, _column(l1, dtype), pos2, _column(l2, dtype),
                                                       weight1, weight2)
    nb = bn.nbins
    if auto and bn.e2[0] == 0:
        # the self pairs: r2 == 0 exactly, bin (0, 0), of the kind 1 where the row has a label
        w = _weights(pm, weight1, l1.shape[0], l1.device)
        has = l1 >= 0
        s = torch.stack([has.sum().to(torch.float64), (~has).sum().to(torch.float64), (w * w)[has].sum()])
        s = allsum(pm.comm, s).cpu().numpy()
        npairs[nb] -= int(s[0])
        wnpairs[nb] -= float(s[2])
        npairs[0] -= int(s[1])
        wnpairs[0] -= W2sum - float(s[2])
    parts = [bn.counts(npairs[k * nb:(k + 1) * nb], wnpairs[k * nb:(k + 1) * nb], rsum[k * nb:(k + 1) * nb], auto, W1,
                       W2, W2sum) for k in (1, 0)]
    total = bn.counts(npairs[:nb] + npairs[nb:], wnpairs[:nb] + wnpairs[nb:], rsum[:nb] + rsum[nb:], auto, W1, W2,
                      W2sum)
    return SplitCounts(parts[0], parts[1], total)


def _analytic_rr(pc, norm):
    """norm V_bin / V_box of the natural estimator in the periodic box, on the device, in the arithmetic of
    pair_correlation; norm: a float, or a numpy array of one norm per realisation (the leading axis of the result)"""
    sub = pc.muedges if pc.mode == '2d' else pc.piedges
    vol = bin_volumes(pc.edges, len(pc.BoxSize), pc.mode, sub)
    if isinstance(norm, numpy.ndarray):
        norm = norm.reshape((-1,) + (1,) * vol.ndim)
    rr = norm * vol / float(numpy.prod(pc.BoxSize))
    return torch.from_numpy(numpy.ascontiguousarray(rr)).to(pc.wnpairs.device)


def pair_correlation_split(pm, pos1, label1, edges, pos2=None, label2=None, weight1=None, weight2=None, mode='1d',
                           muedges=None, Nmu=None, piedges=None, pimax=None, los=2):
    """(xi_1h, xi_2h, SplitCounts): the one-halo and the two-halo term by the natural estimator with the analytic ``RR``
    of pair_correlation, ``xi_1h = same.wnpairs / RR - 1`` and ``xi_2h = different.wnpairs / RR - 1`` (halotools'
    convention), so that ``1 + xi == (1 + xi_1h) + (1 + xi_2h)``.  The arguments are those of pair_counts_split."""
    sc = pair_counts_split(pm, pos1, label1, edges, pos2, label2, weight1, weight2, mode, muedges, Nmu, piedges, pimax,
                           los)
    rr = _analytic_rr(sc.total, sc.total.W1 * sc.total.W2 - sc.total.W2sum)
    return sc.same.wnpairs / rr - 1, sc.different.wnpairs / rr - 1, sc


# ---- the jackknife -----------------------------------------------------------------------------------------------------

def _jackknife(bn, pos1, label1, nlab, pos2, label2, weight1, weight2):
    pm = bn.pm
    auto = pos2 is None
    l1, l2, dtype, _ = _read(pm, pos1, label1, pos2, label2, nlab, bn.error)
    nlab = int(nlab)
    nb = bn.nbins
    K = label_slots(nb)
    ncalls = -(-nlab // K)
    dev = l1.device
    side_n = torch.zeros((nlab, nb), dtype=torch.int64, device=dev)
    same_n = torch.zeros((nlab, nb), dtype=torch.int64, device=dev)
    side_w = torch.zeros((nlab, nb), dtype=torch.float64, device=dev)
    same_w = torch.zeros((nlab, nb), dtype=torch.float64, device=dev)
    first = None
    for c in range(ncalls):
        lo = c * K
        hi = min(lo + K, nlab)
        npairs, wnpairs, rsum, W1, W2, W2sum, _ = bn.count('jackknife', pos1, _column(l1, dtype, lo, hi), pos2,
                                                           _column(l2, dtype, lo, hi), weight1, weight2)
        if c == 0:
            first = (npairs[:nb].clone(), wnpairs[:nb].clone(), rsum, W1, W2, W2sum)
        for out, arr, block in ((side_n, npairs, 1), (side_w, wnpairs, 1), (same_n, npairs, 1 + K),
                                (same_w, wnpairs, 1 + K)):
            out[lo:hi] = arr[block * nb:(block + hi - lo) * nb].reshape(hi - lo, nb)
    all_n, all_w, rsum, W1, W2, W2sum = first
    n1k, W1_k, Wsq_k = _per_label(pm.comm, l1, _weights(pm, weight1, l1.shape[0], dev), nlab)
    if auto:
        W2_k, W2sum_k = W1_k, Wsq_k
        if bn.e2[0] == 0:
            # the self pairs: r2 == 0 exactly, bin (0, 0): one in all, two in side[a], one in same[a]
            csize = l1.shape[0] if pm.comm.size == 1 else int(pm.comm.allreduce(l1.shape[0]))
            all_n[0] -= csize
            all_w[0] -= W2sum
            nk = torch.from_numpy(n1k.astype('i8')).to(dev)
            wk = torch.from_numpy(Wsq_k).to(dev)
            side_n[:, 0] -= 2 * nk
            side_w[:, 0] -= 2 * wk
            same_n[:, 0] -= nk
            same_w[:, 0] -= wk
    else:
        _, W2_k, _ = _per_label(pm.comm, l2, _weights(pm, weight2, l2.shape[0], dev), nlab)
        W2sum_k = numpy.zeros(nlab)
    total = bn.counts(all_n, all_w, rsum, auto, W1, W2, W2sum)
    shape = (nlab,) + bn.shape
    return JackknifeCounts(total, side_n.reshape(shape), side_w.reshape(shape), same_n.reshape(shape),
                           same_w.reshape(shape), W1_k, W2_k, W2sum_k, ncalls)


def pair_counts_jackknife(pm, pos1, label1, edges, nlab, pos2=None, label2=None, weight1=None, weight2=None,
                          mode='1d', muedges=None, Nmu=None, piedges=None, pimax=None, los=2):
    """The sums of a delete-one jackknife over the labels 0 .. nlab - 1 (rule 4 of the module docstring): a
    JackknifeCounts, whose ``total`` equals what pair_counts returns and whose ``realization_counts(k)`` equals
    pair_counts of the rows whose label is not k.

    label1, label2 : (n,) integers, device tensors or numpy arrays: the region of every row, of ``box_regions`` for
        example.  Labels must lie in ``[0, nlab)``, or be negative for a row that is in no region (it is in every
        realisation); anything else raises ValueError on every rank together.  label2 is needed exactly with pos2.
    nlab : the number of regions.  One call of the kernel takes ``K = (4096 / nbins - 2) / 2`` labels (50 at 40 bins);
        more take ``ceil(nlab / K)`` calls (``ncalls``).
    The other arguments are those of pair_counts.  At most 1024 bins.
    """
    bn = _Binning(pm, edges, mode, muedges, Nmu, piedges, pimax, los)
    return _jackknife(bn, pos1, label1, nlab, pos2, label2, weight1, weight2)


def survey_pair_counts_jackknife(pm, pos1, label1, edges, nlab, observer=None, pos2=None, label2=None, weight1=None,
                                 weight2=None, mode='1d', muedges=None, Nmu=None, piedges=None, pimax=None,
                                 thetaedges=None):
    """pair_counts_jackknife about an observer: the modes '1d', '2d', 'projected' and 'angular' of survey_pair_counts,
    with its shift of the rows and its check of the padding; ``total`` is a SurveyPairCounts equal to what
    survey_pair_counts returns."""
    bn = _Binning(pm, edges, mode, muedges, Nmu, piedges, pimax, 2, survey=True, observer=observer,
                  thetaedges=thetaedges)
    return _jackknife(bn, pos1, label1, nlab, pos2, label2, weight1, weight2)


def _normalised(jk, alpha):
    """(wnpairs / norm of the full sample, of every realisation) of a JackknifeCounts"""
    t = jk.total
    wn, norm = jk.realizations(alpha)
    return t.wnpairs / (t.W1 * t.W2 - t.W2sum), wn / norm.reshape((-1,) + (1,) * t.wnpairs.dim())


def _landy_szalay(counts, alpha):
    """(xi, realizations) of the dict of the four JackknifeCounts, nan where the R1R2 bin is empty"""
    full, real = zip(*[_normalised(counts[k], alpha) for k in ('D1D2', 'D1R2', 'D2R1', 'R1R2')])
    out = []
    for dd, dr, rd, rr in (full, real):
        filled = rr > 0
        xi = (dd - dr - rd + rr) / torch.where(filled, rr, torch.ones_like(rr))
        out.append(torch.where(filled, xi, torch.full_like(xi, float('nan'))))
    return out[0], out[1]


def _correlation_with_randoms(count, data1, dlabel1, randoms1, rlabel1, data2, dlabel2, randoms2, rlabel2, dw1, rw1,
                              dw2, rw2, R1R2, alpha):
    cross = data2 is not None
    if cross and randoms2 is None:
        raise ValueError('data2 needs randoms2')
    if not cross and (randoms2 is not None or dw2 is not None or rw2 is not None):
        raise ValueError('randoms2 and the weights of the second sets need data2')
    if R1R2 is not None and not isinstance(R1R2, JackknifeCounts):
        raise TypeError('R1R2 must be the JackknifeCounts of an earlier call')
    counts = {}
    counts['D1D2'] = count(data1, dlabel1, data2, dlabel2, dw1, dw2)
    if cross:
        counts['D1R2'] = count(data1, dlabel1, randoms2, rlabel2, dw1, rw2)
        counts['D2R1'] = count(data2, dlabel2, randoms1, rlabel1, dw2, rw1)
    else:
        counts['D1R2'] = counts['D2R1'] = count(data1, dlabel1, randoms1, rlabel1, dw1, rw1)
    if R1R2 is None:
        R1R2 = count(randoms1, rlabel1, randoms2, rlabel2, rw1, rw2)
    elif tuple(R1R2.side_npairs.shape) != tuple(counts['D1D2'].side_npairs.shape):
        raise ValueError('R1R2 has the labels and bins %s, the counts %s' % (tuple(R1R2.side_npairs.shape),
                                                                             tuple(counts['D1D2'].side_npairs.shape)))
    counts['R1R2'] = R1R2
    xi, real = _landy_szalay(counts, alpha)
    return JackknifeCorrelation(xi, real, counts, alpha)


def pair_correlation_jackknife(pm, pos1, label1, edges, nlab, pos2=None, label2=None, weight1=None, weight2=None,
                               randoms1=None, rlabel1=None, randoms2=None, rlabel2=None, randoms_weight1=None,
                               randoms_weight2=None, R1R2=None, alpha=None, mode='1d', muedges=None, Nmu=None,
                               piedges=None, pimax=None, los=2):
    """The two-point function with its delete-one jackknife realisations and covariance: a JackknifeCorrelation.

    Without randoms: the natural estimator with analytic randoms in the periodic box, ``x_k = wnpairs_k / (norm_k V_bin
    / V_box) - 1``.  Only ``alpha = 1/2`` is allowed, and it is the default there: then ``wnpairs_k = total - side_k /
    2``, every pair with one end in region k counted half.  Its expectation for uniform rows is ``norm_k V_bin / V_box``
    exactly, for regions of any shape: every row of region k sees its full shell, which no analytic RR of the sample
    with a hole cut out (alpha = 1) can say without knowing the shape of the hole.  That is why the weighting is fixed;
    any other alpha without randoms raises ValueError.

    With ``randoms1`` and ``rlabel1`` (and ``randoms2``, ``rlabel2`` with pos2): Landy-Szalay on the normalised
    realisations, ``nXY_k = wnpairs_XY,k / norm_XY,k``, as survey_correlation does on totals; ``alpha`` defaults to 1.
    R1R2 is counted once: the JackknifeCounts ``counts['R1R2']`` of an earlier call on the same randoms, labels and bins
    may be passed back in.  The other arguments are those of pair_counts_jackknife.
    """
    def count(p1, l1, p2, l2, w1, w2):
        return pair_counts_jackknife(pm, p1, l1, edges, nlab, p2, l2, w1, w2, mode, muedges, Nmu, piedges, pimax, los)
    if randoms1 is None:
        if alpha is not None and alpha != 0.5:
            raise ValueError('without randoms only alpha = 1/2 has an analytic RR: pass randoms1 and rlabel1 for '
                             'alpha = %r' % (alpha,))
        if randoms2 is not None or R1R2 is not None:
            raise ValueError('randoms2 and R1R2 need randoms1')
        jk = count(pos1, label1, pos2, label2, weight1, weight2)
        t = jk.total
        xi = t.wnpairs / _analytic_rr(t, t.W1 * t.W2 - t.W2sum) - 1
        wn, _ = jk.realizations(0.5)
        real = wn / _analytic_rr(t, jk.norms(0.5)) - 1
        return JackknifeCorrelation(xi, real, jk, 0.5)
    return _correlation_with_randoms(count, pos1, label1, randoms1, rlabel1, pos2, label2, randoms2, rlabel2, weight1,
                                     randoms_weight1, weight2, randoms_weight2, R1R2, 1.0 if alpha is None else alpha)


def survey_correlation_jackknife(pm, data1, dlabel1, randoms1, rlabel1, edges, nlab, observer=None, data2=None,
                                 dlabel2=None, randoms2=None, rlabel2=None, data_weight1=None, randoms_weight1=None,
                                 data_weight2=None, randoms_weight2=None, R1R2=None, alpha=1.0, mode='1d',
                                 muedges=None, Nmu=None, piedges=None, pimax=None, thetaedges=None):
    """survey_correlation with its delete-one jackknife realisations and covariance: a JackknifeCorrelation by
    Landy-Szalay on the normalised realisations of survey_pair_counts_jackknife.  ``to_poles`` and ``to_wp`` of
    pmesh_amd.surveypairs apply to ``realizations`` along their leading axis, one realisation at a time.  The arguments
    are those of survey_correlation, with the labels of the four sets, nlab and alpha."""
    def count(p1, l1, p2, l2, w1, w2):
        return survey_pair_counts_jackknife(pm, p1, l1, edges, nlab, observer, p2, l2, w1, w2, mode, muedges, Nmu,
                                            piedges, pimax, thetaedges)
    return _correlation_with_randoms(count, data1, dlabel1, randoms1, rlabel1, data2, dlabel2, randoms2, rlabel2,
                                     data_weight1, randoms_weight1, data_weight2, randoms_weight2, R1R2, alpha)
