"""pmx_apply_transfer (csrc/pmx_transfer.hip) at kernel level, against a numpy restatement of the reference's filters.

The restatement is written from the callables a caller of the reference passes to Field.apply: dx1_transfer,
force_transfer, pot_transfer and lowpass_transfer of examples/nbody.py:154-181 and the window compensation of
pmesh/window.py:65-80 (v / prod_d sinc(w_d / 2)^p), with the coordinates of pm.py:1200-1226 from the integer mode
number i - N [i >= N // 2]: w = 2 pi i / N, k = 2 pi i / L.  It is compared element by element, never through a norm:

    |got - want| <= tol (1 + k^2 r^2 / 2) S(k) |v|

with S the magnitude of the factor (`restate`), tol = 1e-14 for complex128 and 2^-22 for complex64 (the kernel
computes in double and rounds each component once: 2^-24 sqrt(2) S |v|).  The Gaussian's exponent scales the bound
because the rounding of k^2 enters the result multiplied by it.  Under -m "not gpu" the entry is served by the CPU
oracle (oracle/pmesh_oracle.c: pmo_apply_transfer), which checks the restatement; under -m gpu by the kernel.
"""
import ctypes as C

import numpy
import pytest
import torch

from pmesh_amd import _abi
from pmesh_amd.backend import PmxError
from pmesh_amd.pm import ParticleMesh, TransposedComplexField, UntransposedComplexField
from pmesh_amd.transfer import Transfer
from tests.test_lpt import FORMS, TALL, TALL_1D, WRAP, _block, cpu

BOX = [100., 80., 120.]
GEOMS = [([16, 16, 9], [0, 0, 0], [16, 16, 16]),          # an r2c half spectrum: k = 0 and all three Nyquist indices
         ([45, 15, 45], [0, 0, 0], [45, 45, 45]),         # odd, a block of a c2c spectrum
         ([12, 48, 25], [36, 0, 0], [48, 48, 48]),        # 3 * 2^k, a slab at 36: the negative half of axis 0 only
         ([1, 48, 25], [24, 0, 0], [48, 48, 48]),         # a one-plane slab that is the Nyquist plane
         ([24, 17], [0, 0], [24, 32]),                    # 2-d
         ([300], [0], [598])] + TALL + TALL_1D            # 1-d; then a slowest axis longer than the launch grid
TOL = {'c16': 1e-14, 'c8': 2.0 ** -22}


# ---- the restatement -----------------------------------------------------------------------------------------------

def mode_numbers(shape, start, nmesh):
    """per axis the signed integer mode number of the block's indices, shaped to broadcast along its own axis"""
    nd = len(shape)
    out = []
    for d in range(nd):
        i = numpy.arange(shape[d], dtype='i8') + int(start[d])
        i = i - int(nmesh[d]) * (i >= int(nmesh[d]) // 2)
        out.append(i.astype('f8').reshape([-1 if e == d else 1 for e in range(nd)]))
    return out


def k_squared(shape, start, nmesh, box):
    k2 = numpy.zeros(tuple(shape))
    for i, L in zip(mode_numbers(shape, start, nmesh), box):
        k2 = k2 + (2 * numpy.pi * i / L) ** 2
    return k2


def restate(t, shape, start, nmesh, box):
    """(f, gradient, bound): the factor of Transfer t on the block is f (real), times 1j when `gradient`; bound is
    (1 + k^2 r^2 / 2) S(k) of the module docstring.  S = r0 = |amplitude| q^laplace_pow exp(-k^2 r^2 / 2) /
    prod_d |sinc(w_d / 2)|^p without a gradient, r0 |k_d| with the spectral one (modes with k_d = 0 must come out
    exactly 0) and r0 max(|D4(k_d)|, 1 / C) with the finite difference: at the Nyquist index 8 sin w - sin 2w is
    pure cancellation of the rounding of w = k C, where two correct double evaluations differ by about 4 eps / C."""
    i = mode_numbers(shape, start, nmesh)
    w = [2 * numpy.pi * i_d / N for i_d, N in zip(i, nmesh)]
    k = [2 * numpy.pi * i_d / L for i_d, L in zip(i, box)]
    k2 = numpy.zeros(tuple(shape))
    for kd in k:
        k2 = k2 + kd ** 2
    f = numpy.full(tuple(shape), t.amplitude)
    if t.laplace_pow:
        q = k2.copy()
        q[q == 0] = 1.0                                      # nbody.py:157
        f = f * q ** t.laplace_pow
    exponent = 0.5 * k2 * t.gauss_r ** 2
    if t.gauss_r:
        f = f * numpy.exp(-exponent)                         # nbody.py:180
    if t.deconv_pow:
        for wd in w:                                         # window.py:74-78, fwindow = sinc(w / 2)^p
            half = 0.5 * wd
            s = numpy.where(half == 0, 1.0, numpy.sin(half) / numpy.where(half == 0, 1.0, half))
            f = f / s ** t.deconv_pow
    S = numpy.abs(f)
    gradient = t.grad_dir >= 0
    if gradient:
        d = t.grad_dir
        if t.grad_kind == 'spectral':
            D = k[d]                                         # nbody.py:158
            S = S * numpy.abs(D)
        else:
            Cc = box[d] / nmesh[d]                           # nbody.py:166-168
            wc = k[d] * Cc
            D = 1.0 / Cc * 1 / 6.0 * (8 * numpy.sin(wc) - numpy.sin(2 * wc))
            S = S * numpy.maximum(numpy.abs(D), 1.0 / Cc)
        f = f * D
    return f, gradient, (1.0 + exponent) * S


def transfers(ndim, r):
    """(name, Transfer): the closed forms by name, every power and deconvolution, and two combinations that only the
    general instantiation of the kernel serves"""
    out = []
    for d in range(ndim):
        out += [('dx1(%d)' % d, Transfer.dx1(d)), ('force(%d)' % d, Transfer.force(d))]
    out += [('potential', Transfer.potential()), ('amplitude', Transfer(amplitude=2.5))]
    out += [('laplace_pow=%d' % p, Transfer(laplace_pow=p)) for p in (-2, -1, 1, 2)]
    out += [('lowpass', Transfer.lowpass(r))]
    out += [('deconv_pow=%d' % p, Transfer(deconv_pow=p)) for p in (1, 2, 3, 4)]
    out += [('all', Transfer(amplitude=-0.5, laplace_pow=-1, grad_dir=ndim - 1, grad_kind='finite4', deconv_pow=3,
                             gauss_r=r)),
            ('laplace2 grad0 gauss', Transfer(laplace_pow=2, grad_dir=0, gauss_r=r))]
    return out


def smoothing(shape, start, nmesh, box):
    """r = 6 / k_max of the block: the Gaussian's exponent stays below 18 and no mode underflows to 0"""
    return 6.0 / numpy.sqrt(k_squared(shape, start, nmesh, box).max())


_restated = {}      # geometry -> [(name, Transfer, f, gradient, bound)]: one geometry at a time, shared by its cases


def restated(gi):
    if gi not in _restated:
        _restated.clear()
        shape, start, nmesh = GEOMS[gi]
        box = BOX[:len(shape)]
        r = smoothing(shape, start, nmesh, box)
        _restated[gi] = [(name, t) + restate(t, shape, start, nmesh, box) for name, t in transfers(len(shape), r)]
    return _restated[gi]


def apply_transfer(be, t, v, out, start, nmesh, box):
    """the entry itself on the blocks v and out (out may be v), Transfer t"""
    es = v.element_size()
    c = t._cstruct()
    be.call('apply_transfer', C.byref(c), v.dim(), es // 2, v.data_ptr(), _abi.i64arr([s * es for s in v.stride()], 3),
            out.data_ptr(), _abi.i64arr([s * es for s in out.stride()], 3), _abi.i64arr(v.shape, 3),
            _abi.i64arr(start, 3), _abi.i64arr(nmesh, 3), _abi.f64arr(box, 3), be.stream())


def times(f, gradient, v):
    """(1j f if gradient else f) * v, component by component"""
    return -f * v.imag + 1j * (f * v.real) if gradient else f * v.real + 1j * (f * v.imag)


def assert_each(got, want, bound, v, tol, what):
    """element by element: |got - want| <= tol bound |v|; NaN (an element never written) fails"""
    err = numpy.abs(numpy.asarray(got).astype('c16') - want)
    lim = tol * bound * numpy.abs(v)
    bad = ~(err <= lim)
    if bad.any():
        at = numpy.unravel_index(numpy.argmax(bad), bad.shape)
        with numpy.errstate(divide='ignore', invalid='ignore'):
            worst = numpy.nanmax(numpy.where(lim > 0, err / lim, numpy.where(err > 0, numpy.inf, 0.0)))
        raise AssertionError('%s: %d of %d elements off, first at %s (got %r, want %r, allowed %.3g); the worst is '
                             '%.3g of its bound' % (what, bad.sum(), bad.size, at, got[at], want[at], lim[at], worst))
    # the rows a workgroup reaches on its second trip over the slowest axis, on their own
    for d, n in enumerate(err.shape):
        if n > WRAP:
            sel = (slice(None),) * d + (slice(WRAP, None),)
            assert numpy.isfinite(numpy.asarray(got)[sel]).all() and (err[sel] <= lim[sel]).all(), what


# ---- the kernel against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('cdt', ['c16', 'c8'])
@pytest.mark.parametrize('gi', range(len(GEOMS)), ids=['x'.join(map(str, g[0])) for g in GEOMS])
def test_transfer_kernel(be, gi, cdt, form):
    shape, start, nmesh = GEOMS[gi]
    box = BOX[:len(shape)]
    rng = numpy.random.RandomState(40 + gi)
    v = _block(shape, cdt, form, rng)
    out = _block(shape, cdt, 'pad' if form != 'pad' else 'C', rng)
    assert v.stride() != out.stride() or len(shape) == 1
    held = v.clone()
    vals = cpu(v).astype('c16')
    nan = complex(float('nan'), float('nan'))
    for name, t, f, gradient, bound in restated(gi):
        want = times(f, gradient, vals)
        what = '%s %s %s %s' % (shape, cdt, form, name)
        out.fill_(nan)
        apply_transfer(be, t, v, out, start, nmesh, box)
        assert_each(cpu(out), want, bound, vals, TOL[cdt], what)
        assert torch.equal(v, held), what + ': the input changed'
        apply_transfer(be, t, v, v, start, nmesh, box)       # in place
        assert_each(cpu(v), want, bound, vals, TOL[cdt], what + ' in place')
        v.copy_(held)


# ---- the array-operator form against the kernel --------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['T', 'U'])
@pytest.mark.parametrize('Nmesh,BoxSize,dtype', [([16, 12, 10], [100., 80., 120.], 'f8'), ([24, 20], [100., 80.], 'f4'),
                                                 ([64], [100.], 'f8')])
def test_call_equals_apply(be, Nmesh, BoxSize, dtype, kind):
    """field.apply(lambda k, v: T(k, v)), the same formula written with array operators, and field.apply(T)"""
    pm = ParticleMesh(Nmesh, BoxSize=BoxSize, dtype=dtype)
    c = pm.create(type=UntransposedComplexField if kind == 'U' else TransposedComplexField)
    rng = numpy.random.RandomState(7)
    shape = tuple(c.value.shape)
    c.value[...] = torch.from_numpy(rng.normal(size=shape) + 1j * rng.normal(size=shape)).to(c.value.device)
    vals = cpu(c.value).astype('c16')
    start = [int(s) for s in c.start]
    r = smoothing(shape, start, Nmesh, BoxSize)
    for name, t in transfers(len(Nmesh), r):
        f, gradient, bound = restate(t, shape, start, Nmesh, BoxSize)
        fused = cpu(c.apply(t).value)
        called = cpu(c.apply(lambda k, v: t(k, v)).value)
        what = '%s %s %s %s' % (Nmesh, dtype, kind, name)
        assert_each(fused, times(f, gradient, vals), bound, vals, TOL['c16' if dtype == 'f8' else 'c8'], what)
        assert_each(called, fused.astype('c16'), bound, vals, TOL['c16' if dtype == 'f8' else 'c8'], what + ' called')


# ---- arguments -----------------------------------------------------------------------------------------------------

def test_bad_arguments(be):
    v = torch.zeros((4, 4, 4), dtype=torch.complex128, device=be.device)
    strides = _abi.i64arr([s * 16 for s in v.stride()], 3)

    def call(t, ndim, elsize):
        be.call('apply_transfer', C.byref(t), ndim, elsize, v.data_ptr(), strides, v.data_ptr(), strides,
                _abi.i64arr([4, 4, 4], 3), _abi.i64arr([0, 0, 0], 3), _abi.i64arr([4, 4, 4], 3),
                _abi.f64arr([1., 1., 1.], 3), be.stream())
    call(Transfer.dx1(2)._cstruct(), 3, 8)
    with pytest.raises(PmxError):
        call(Transfer.dx1(2)._cstruct(), 2, 8)             # grad_dir >= ndim
    with pytest.raises(PmxError):
        apply_transfer(be, Transfer.force(1), v[0, 0], v[0, 0], [0], [4], [1.])
    for ndim in (0, 4):
        with pytest.raises(PmxError):
            call(Transfer.potential()._cstruct(), ndim, 8)
    with pytest.raises(PmxError):
        call(Transfer.potential()._cstruct(), 3, 2)
