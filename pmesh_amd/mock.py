"""Poisson-sampled particles from a density field, and lognormal mock catalogues, made on the device.

What nbodykit's LogNormalCatalog does on the host (numpy Poisson counts of the mesh, numpy.repeat of the cell
coordinates, uniform offsets, and the positions over PCIe) as four kernels (csrc/pmx_poisson.hip,
include/pmesh_amd.h): the loop white noise -> Tabulated -> c2r -> sample -> paint_interlaced -> power_spectrum /
correlation_function / bispectrum stays in HBM.  The result is reproducible bit for bit from a seed and does not
depend on how the mesh is split over ranks.

The sampling rule (normative; include/pmesh_amd.h restates it next to the entry points).  Every random number is one
call of Philox4x32-10 with ``key = (seed & 0xffffffff, seed >> 32)`` and ``counter = (g & 0xffffffff, g >> 32, j,
stream)``, g the GLOBAL C-order index of the cell over Nmesh.

1. The rate of a cell, in double: ``lam = scale * x`` (mode 'linear') or ``lam = scale * exp(bias * x)`` (mode 'exp').
   A rate that is NaN, negative, infinite or above ``PMX_POISSON_MAX_RATE`` (2^20) is refused: ValueError.
2. Its count (stream 0): ``n = max(1, ceil(lam / 16))`` chunks of rate ``lam / n``; chunk j is drawn by inversion of
   ``u = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53`` with a sequential search of at most 128 steps.
3. Its particles (stream 1): particle p (j = p) lies at ``x_d = ((i_d - 0.5) + (w_d + 0.5) * 2^-32) * (L_d / N_d)``,
   wrapped into [0, L_d): uniform in the cell CENTRED on the grid point i_d, the convention of the windows of this
   package, so that a nearest-grid-point paint of the particles returns the counts.
4. Cells come in the C order of the local block, the particles of a cell in the order of p.

    from pmesh_amd.mock import poisson_sample, lognormal_catalog
    s = poisson_sample(one_plus_delta, nbar=3e-4, seed=42)
    s.pos, s.counts, s.size, s.csize, s.expected
    cat = lognormal_catalog(pm, transfer, nbar=3e-4, seed=42, bias=2.0, displacement=True)
    cat.pos, cat.displacement, cat.delta_k
"""
import numpy
import torch

from . import _abi, backend

_MODES = {'linear': _abi.PMX_POISSON_LINEAR, 'exp': _abi.PMX_POISSON_EXP}
SEGMENT = _abi.PMX_POISSON_SEGMENT
#: the stream word of the Philox call that derives the Poisson seed of a lognormal catalogue from its seed
SEED_STREAM = 2


def philox4x32(counter, key):
    """Philox4x32-10 of four counter words under two key words (python ints): the four output words"""
    c0, c1, c2, c3 = (int(c) & 0xffffffff for c in counter)
    k0, k1 = (int(k) & 0xffffffff for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c3 ^ k1, p0 & 0xffffffff
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def poisson_seed(seed):
    """The seed of the Poisson sampling of ``lognormal_catalog(..., seed)``: ``w0 | w1 << 32`` of the Philox call with
    counter (0, 0, 0, SEED_STREAM) under the key of `seed`, so that the white noise (which takes `seed` itself) and the
    sampling draw from different streams."""
    seed = _seed(seed)
    w = philox4x32((0, 0, 0, SEED_STREAM), (seed & 0xffffffff, seed >> 32))
    return w[0] | (w[1] << 32)


def _seed(seed):
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError('seed must be an integer in [0, 2^64)')
    return int(seed)


class PoissonSample(object):
    """The particles of one rank: ``pos`` ((size, ndim) float64 device tensor), ``counts`` (uint32 device tensor of the
    shape of the local block), ``size`` (local number of particles), ``csize`` (summed over the ranks), ``expected``
    (the sum of the rates over all ranks) and ``cells`` (int64 global C-order cell index per particle, or None)."""

    def __init__(self, pos, counts, size, csize, expected, cells):
        self.pos, self.counts, self.size, self.csize, self.expected, self.cells = pos, counts, size, csize, expected, cells


class LognormalCatalog(PoissonSample):
    """A PoissonSample with ``delta_k`` (the Gaussian field's spectrum, a ComplexField), ``mean`` (the mean of
    exp(bias delta_G) over the mesh), ``poisson_seed`` and ``displacement`` ((size, ndim) float64, or None)."""


def _sample(field, mode, scale, bias, seed, return_cells, rate_sum=None):
    """the kernels on the local block of `field`: (pos, counts, size, flagged, rate sum, cells), this rank's; the rate
    sum is computed unless the caller has it"""
    be = backend.get()
    pm = field.pm
    x = field.value
    ndim = x.dim()
    ncells = x.numel()
    nseg = (ncells + SEGMENT - 1) // SEGMENT
    dev = x.device
    counts = torch.empty(tuple(x.shape), dtype=torch.uint32, device=dev)
    # [total, flagged, rate sum as a double]: what the host needs to go on, in one copy
    head = torch.zeros(3, dtype=torch.int64, device=dev)
    seg = torch.empty(nseg, dtype=torch.int64, device=dev)
    if rate_sum is None:
        be.poisson_rate_sum(x, mode, scale, bias, head[2:3].view(torch.float64))
    be.poisson_count(x, field.start, pm.Nmesh, mode, scale, bias, seed, counts, seg, head[1:2])
    be.poisson_scan(seg, head[0:1])
    host = head.cpu().numpy()                    # the one synchronisation: the output has to be allocated
    total, flagged = int(host[0]), int(host[1])
    rsum = float(host[2:3].view('f8')[0]) if rate_sum is None else float(rate_sum)
    pos = torch.empty((total, ndim), dtype=torch.float64, device=dev)
    cells = torch.empty(total, dtype=torch.int64, device=dev) if return_cells else None
    if not flagged:
        be.poisson_emit(tuple(x.shape), field.start, pm.Nmesh, pm.BoxSize, seed, counts, seg, pos, cells)
    return pos, counts, total, flagged, rsum, cells


def _finish(cls, field, out):
    """the sums over the ranks, and the error every rank raises together when any cell was refused"""
    pos, counts, total, flagged, rsum, cells = out
    sums = numpy.array([total, flagged, rsum], dtype='f8')
    if field.pm.comm.size > 1:
        sums = numpy.asarray(field.pm.comm.allreduce(sums))
    if sums[1] > 0:
        raise ValueError('%d cells have a rate that is NaN, negative, infinite or above PMX_POISSON_MAX_RATE = %d'
                         % (int(sums[1]), _abi.PMX_POISSON_MAX_RATE))
    return cls(pos, counts, total, int(sums[0]), float(sums[2]), cells)


def _checked(field):
    from .pm import RealField
    if not isinstance(field, RealField):
        raise TypeError('poisson_sample samples RealField objects, not %s' % type(field).__name__)
    if len(field.pm.Nmesh) > _abi.PMX_MAXDIM:
        raise NotImplementedError('Poisson sampling of meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    if field.value.dtype not in (torch.float32, torch.float64):
        raise ValueError('poisson_sample samples float32 or float64 meshes (complex-to-complex meshes are not '
                         'supported)')
    return field


def _cell_volume(pm):
    return float(numpy.prod(numpy.asarray(pm.BoxSize, dtype='f8') / numpy.asarray(pm.Nmesh, dtype='f8')))


def poisson_sample(field, nbar=None, seed=0, mode='linear', bias=1.0, scale=None, return_cells=False):
    """Particles Poisson-sampled from the RealField `field` by the rule of the module docstring: a PoissonSample.

    field : RealField of 1, 2 or 3 dimensions, f4 or f8, on one or several ranks; left as it is.
    nbar : the mean number density in box units: the rate of a cell is ``nbar * V_cell * field`` (mode 'linear'; with
        mode 'exp' ``nbar * V_cell * exp(bias * field)``), so a ``1 + delta`` field has the mean rate ``nbar * V_cell``.
    scale : the factor in front of the field given directly instead; exactly one of `nbar` and `scale`.
    seed : integer in [0, 2^64).  The same seed gives the same particles, whatever the decomposition.
    return_cells : also return the global C-order cell index of every particle.

    An all-zero field gives ``pos`` of shape (0, ndim).  A rate that is NaN, negative, infinite or above
    PMX_POISSON_MAX_RATE raises ValueError on every rank.

    The particles of a rank lie within half a cell of its block: a nearest-grid-point paint of them needs no exchange,
    but ``pm.decompose`` is still needed before painting with a wider window on several ranks.
    """
    field = _checked(field)
    if mode not in _MODES:
        raise ValueError("mode must be 'linear' or 'exp'")
    if (nbar is None) == (scale is None):
        raise ValueError('exactly one of nbar and scale must be given')
    if scale is None:
        scale = float(nbar) * _cell_volume(field.pm)
    scale, bias = float(scale), float(bias)
    if not (numpy.isfinite(scale) and numpy.isfinite(bias)):
        raise ValueError('nbar, scale and bias must be finite')
    return _finish(PoissonSample, field, _sample(field, _MODES[mode], scale, bias, _seed(seed), return_cells))


def lognormal_catalog(pm, transfer, nbar, seed, bias=1.0, unitary=False, displacement=False, resampler=None,
                      return_cells=False):
    """A lognormal mock catalogue on the ParticleMesh `pm` (1 to 3 dimensions): a LognormalCatalog.

    1. ``delta_k = pm.generate_whitenoise(seed, unitary=unitary)`` with `transfer` applied.  `transfer` is a
       :class:`pmesh_amd.transfer.Tabulated` (or any Transfer) of ``sqrt(P(k) / V)``, V the volume of the box; from a
       table ``k, P`` of the linear power spectrum::

           V = numpy.prod(pm.BoxSize)
           transfer = Tabulated(k, numpy.sqrt(P / V), loglog=True)
           cat = lognormal_catalog(pm, transfer, nbar, seed)

    2. ``delta_G = c2r(delta_k)`` (delta_k is kept, for the displacement and for the caller).
    3. ``m = sum exp(bias delta_G) / Ncells`` over the whole mesh (pmx_poisson_rate_sum and one allreduce).
    4. Counts and positions from mode 'exp' with ``scale = nbar V_cell / m``: the mean density is `nbar` exactly in
       expectation — the normalisation of nbodykit's lognormal_transform, which fixes the mean of the transformed field
       instead of subtracting sigma^2 / 2.
    5. The Poisson seed is ``poisson_seed(seed)``: one Philox call under the key of `seed`, so the stream of the field
       and the stream of the sampling differ.
    6. With ``displacement=True`` the result holds ``lpt1(delta_k, pos, resampler=resampler)``: the linear displacement
       psi at the particles, from which a caller forms velocities and the redshift-space positions
       ``x + f (psi . los) los``.  Growth factors and redshift-space distortions remain the caller's.

    seed : integer in [0, 2^32) (the range of the white noise).  bias : the Lagrangian bias in the exponent.
    return_cells : as for poisson_sample (the rows of several ranks, sorted by it, are the one-rank rows).
    """
    from .lpt import lpt1
    from .transfer import Transfer
    if len(pm.Nmesh) > _abi.PMX_MAXDIM:
        raise NotImplementedError('lognormal catalogues of meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
    if not isinstance(transfer, Transfer):
        raise TypeError('transfer must be a pmesh_amd.transfer.Transfer (a Tabulated of sqrt(P(k) / V))')
    if _seed(seed) >= 2 ** 32:
        raise ValueError('seed must be below 2^32: it also seeds the white noise')
    nbar, bias = float(nbar), float(bias)
    if not (numpy.isfinite(nbar) and nbar >= 0 and numpy.isfinite(bias)):
        raise ValueError('nbar must be finite and not negative, bias finite')
    delta_k = pm.generate_whitenoise(int(seed), unitary=unitary)
    delta_k.apply(transfer, out=Ellipsis)
    delta_g = _checked(delta_k.c2r())
    be = backend.get()
    msum = torch.zeros(1, dtype=torch.float64, device=delta_g.value.device)
    be.poisson_rate_sum(delta_g.value, _abi.PMX_POISSON_EXP, 1.0, bias, msum)
    local = float(msum.cpu()[0])
    msum = numpy.array([local])
    if pm.comm.size > 1:
        msum = numpy.asarray(pm.comm.allreduce(msum))
    mean = float(msum[0]) / float(numpy.prod(numpy.asarray(pm.Nmesh, dtype='f8')))
    if not (numpy.isfinite(mean) and mean > 0):
        raise ValueError('the mean of exp(bias delta_G) is %r: the field or the bias is too large' % mean)
    pseed = poisson_seed(seed)
    scale = nbar * _cell_volume(pm) / mean
    cat = _finish(LognormalCatalog, delta_g,
                  _sample(delta_g, _abi.PMX_POISSON_EXP, scale, bias, pseed, return_cells, rate_sum=scale * local))
    cat.delta_k, cat.mean, cat.poisson_seed = delta_k, mean, pseed
    cat.displacement = lpt1(delta_k, cat.pos, resampler=resampler) if displacement else None
    return cat
