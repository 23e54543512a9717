"""Fused transfer functions for ``ComplexField.apply``.

The reference applies arbitrary Python callables slab by slab
(pmesh/pm.py:617-648); the PM cycle only ever uses a few closed forms
(examples/nbody.py:154-181; pmesh/transfer.py:69-112, 232-240; window
compensation pmesh/window.py:65-80).  A :class:`Transfer` describes such a form
and runs as ONE kernel over the complex field (csrc/pmx_transfer.hip, one
complex read + one write per mode, wavenumbers recomputed from the index):

    T(k) = amplitude * (k^2)^laplace_pow * exp(-k^2 r^2 / 2) / prod_d sinc(w_d/2)^deconv_pow
           * [ i * D(k_dir) ]            k^2(0) := 1 as in nbody.py:156-157

with D(k) = k ("dx1_transfer") or the 4-point finite difference
(8 sin w - sin 2w) / (6 C), w = k C, C = L/N ("force_transfer").

A Transfer is also an ordinary ``func(k, v)`` callable (same formula written
with array operators), so it can be passed anywhere the reference takes a
filter, and the two evaluations are tested against each other.
"""
import ctypes as C

import numpy
import torch

from . import _abi, backend


class Transfer(object):
    def __init__(self, amplitude=1.0, laplace_pow=0, grad_dir=None, grad_kind='spectral',
                 deconv_pow=0, gauss_r=0.0):
        self.amplitude = float(amplitude)
        self.laplace_pow = int(laplace_pow)
        self.grad_dir = -1 if grad_dir is None else int(grad_dir)
        if grad_kind not in ('spectral', 'finite4'):
            raise ValueError("grad_kind must be 'spectral' or 'finite4'")
        self.grad_kind = grad_kind
        self.deconv_pow = int(deconv_pow)
        self.gauss_r = float(gauss_r)

    # the closed forms of the reference, by name
    @classmethod
    def dx1(cls, direction):
        """ 1j * k_d / k^2  (examples/nbody.py:154-160) """
        return cls(laplace_pow=-1, grad_dir=direction, grad_kind='spectral')

    @classmethod
    def force(cls, direction):
        """ 1j * D4(k_d) / k^2  (examples/nbody.py:162-171) """
        return cls(laplace_pow=-1, grad_dir=direction, grad_kind='finite4')

    @classmethod
    def long_range(cls, direction, r_split, grad_kind='finite4'):
        """ 1j * D(k_d) / k^2 * exp(-k^2 r_split^2): the mesh partner of shortrange.short_range_force(r_split) """
        return cls(laplace_pow=-1, grad_dir=direction, grad_kind=grad_kind, gauss_r=numpy.sqrt(2.0) * r_split)

    @classmethod
    def potential(cls):
        """ -1 / k^2  (examples/nbody.py:173-176; transfer.py:232-240) """
        return cls(amplitude=-1.0, laplace_pow=-1)

    @classmethod
    def lowpass(cls, r):
        """ exp(-k^2 r^2 / 2)  (examples/nbody.py:177-181; transfer.py:97-112) """
        return cls(gauss_r=r)

    @classmethod
    def compensation(cls, resampler):
        """ 1 / prod_d sinc(w_d/2)^p, p the native support of the window
            (ResampleWindow.get_compensation, window.py:65-80) """
        from .window import FindResampler
        return cls(deconv_pow=FindResampler(resampler).nativesupport)

    def fusable(self):
        """closed forms without per-element transcendentals can ride on the first pass of c2r ([r4] the
        finite-difference gradient along axes 1 and 2 too: its factor belongs to the column and comes from a table;
        along axis 0 it would cost the fused kernels a load per element and stays a kernel of its own)"""
        return (self.gauss_r == 0.0 and self.deconv_pow == 0 and -1 <= self.laplace_pow <= 1 and
                (self.grad_dir < 0 or self.grad_kind == 'spectral' or self.grad_dir > 0))

    def _cstruct(self):
        t = _abi.Transfer()
        t.amplitude = self.amplitude
        t.laplace_pow = self.laplace_pow
        t.grad_dir = self.grad_dir
        t.grad_kind = 0 if self.grad_kind == 'spectral' else 1
        t.deconv_pow = self.deconv_pow
        t.gauss_r = self.gauss_r
        return t

    def _launch(self, field, outv):
        be = backend.get()
        v = field.value
        es = v.element_size()
        nd = v.dim()
        t = self._cstruct()
        be.call('apply_transfer', C.byref(t), nd, es // 2, v.data_ptr(),
                _abi.i64arr([s * es for s in v.stride()], 3), outv.data_ptr(),
                _abi.i64arr([s * es for s in outv.stride()], 3), _abi.i64arr(v.shape, 3),
                _abi.i64arr(field.start, 3), _abi.i64arr(field.Nmesh, 3),
                _abi.f64arr(field.BoxSize, 3), be.stream())

    @staticmethod
    def _double_wavenumbers(k, v):
        """The kernel evaluates T in double from the mode's index whatever the precision of the mesh, and so does this
        form: the wavenumbers Field.apply hands out on an f4 mesh are rounded to float32 (as the reference casts
        them), so they are recomputed from the mode numbers the slab carries (v.i, v.BoxSize, v.Nmesh; the roundings
        of pm._block_coords in float64), or widened where it carries none.  float64 wavenumbers pass through."""
        if all(str(ki.dtype).endswith('float64') for ki in k):
            return k

        def f8(a):
            return a.to(torch.float64) if isinstance(a, torch.Tensor) else a.astype('f8')
        i = getattr(v, 'i', None)
        if i is None or not hasattr(v, 'BoxSize') or not hasattr(v, 'Nmesh'):
            return [f8(ki) for ki in k]
        out = []
        for ii, L, N in zip(i, v.BoxSize, v.Nmesh):
            N = int(N)
            out.append(f8(ii - N * (ii >= N // 2)) * (2 * numpy.pi / N) * N / float(L))
        return out

    def __call__(self, k, v):
        """ the same transfer as a reference-style filter func(k, v), kind='wavenumber' """
        xp_sin, xp_exp = (torch.sin, torch.exp) if isinstance(v, torch.Tensor) else (numpy.sin, numpy.exp)
        k = self._double_wavenumbers(k, v)
        k2 = sum(ki ** 2 for ki in k)
        r = self.amplitude
        if self.laplace_pow:
            q = k2 + (k2 == 0) * 1.0
            r = r * q ** self.laplace_pow
        if self.gauss_r:
            r = r * xp_exp(-0.5 * k2 * self.gauss_r ** 2)
        if self.deconv_pow:
            BoxSize, Nmesh = v.BoxSize, v.Nmesh
            for ki, L, N in zip(k, BoxSize, Nmesh):
                w = ki * (float(L) / float(N))
                half = 0.5 * w
                s = xp_sin(half) / (half + (half == 0) * 1.0) + (half == 0) * 1.0
                r = r / s ** self.deconv_pow
        if self.grad_dir >= 0:
            d = self.grad_dir
            if self.grad_kind == 'spectral':
                D = k[d]
            else:
                Cc = float(v.BoxSize[d]) / float(v.Nmesh[d])
                w = k[d] * Cc
                D = 1.0 / Cc * 1 / 6.0 * (8 * xp_sin(w) - xp_sin(2 * w))
            r = 1j * (r * D)
        return r * v


class Tabulated(Transfer):
    """A transfer function tabulated in |k| (an extension; the reference's callers evaluate one with numpy.interp
    inside Field.apply, examples/nbody.py:245-282):

        T(|k|) = amplitude * interp(|k|),    |k| = sqrt((k_0^2 + k_1^2) + k_2^2)

    loglog=False: interp is ``numpy.interp(|k|, k, t, left, right)``.  loglog=True: it is
    ``exp(numpy.interp(log|k|, log k, log t))`` for k[0] <= |k| <= k[-1], `left` below and `right` above (|k| = 0
    gives `left`).  k: 2 .. PMX_KTABLE_MAX strictly increasing finite values (positive when loglog), t: as many finite
    values (positive when loglog).

    One kernel over the complex field (csrc/pmx_lpt.hip: ktable_kernel, a binary search of the table in device
    memory, started from a closed-form guess when the table is uniform in k, or in log k for loglog); it is not fused into c2r, so ``c2r(transfer=Tabulated(...))`` applies it as a kernel of its own.  Like
    every Transfer it is also a ``func(k, v)`` callable evaluated with array operators on the host or device.

        delta_k = pm.generate_whitenoise(seed, unitary=True).apply(Tabulated(k, (P / V) ** 0.5, loglog=True))

    ``apply_vjp`` and ``apply_jvp`` are its gradients with respect to the field and to the values t (band powers,
    transfer-function nodes); the abscissae k have none.
    """

    def __init__(self, k, t, loglog=False, amplitude=1.0, left=0.0, right=0.0):
        Transfer.__init__(self, amplitude=amplitude)
        k = numpy.array(k, dtype='f8')
        t = numpy.array(t, dtype='f8')
        if k.ndim != 1 or t.ndim != 1 or len(k) != len(t):
            raise ValueError('k and t must be 1-d arrays of the same length')
        if len(k) < 2 or len(k) > _abi.PMX_KTABLE_MAX:
            raise ValueError('a table of 2 .. PMX_KTABLE_MAX = %d entries, not %d' % (_abi.PMX_KTABLE_MAX, len(k)))
        if not (numpy.isfinite(k).all() and numpy.isfinite(t).all()):
            raise ValueError('k and t must be finite')
        if not (numpy.diff(k) > 0).all():
            raise ValueError('k must be strictly increasing')
        self.loglog = bool(loglog)
        if self.loglog and not ((k > 0).all() and (t > 0).all()):
            raise ValueError('loglog tables need positive k and t')
        self.left, self.right = float(left), float(right)
        if not (numpy.isfinite(self.amplitude) and numpy.isfinite(self.left) and numpy.isfinite(self.right)):
            raise ValueError('amplitude, left and right must be finite')
        self.k, self.t = k, t
        self._x, self._y = (numpy.log(k), numpy.log(t)) if self.loglog else (k, t)
        self._dev = {}

    def fusable(self):
        return False

    def _table(self, device):
        """the device copy of the table (x, y as float64) and its pmx_ktable"""
        got = self._dev.get(device)
        if got is None:
            x = torch.from_numpy(self._x).to(device)
            y = torch.from_numpy(self._y).to(device)
            s = _abi.KTable()
            s.n, s.loglog, s.amplitude = len(self._x), int(self.loglog), self.amplitude
            s.left, s.right, s.kmin, s.kmax = self.left, self.right, float(self.k[0]), float(self.k[-1])
            # a table uniform in x (k, or log k): the kernel's search starts from a closed-form guess
            step = numpy.diff(self._x)
            if numpy.abs(step - step.mean()).max() <= 1e-6 * step.mean():
                s.inv_step = 1.0 / step.mean()
            s.x, s.y = x.data_ptr(), y.data_ptr()
            got = self._dev[device] = (x, y, s)
        return got

    def _launch(self, field, outv):
        be = backend.get()
        v = field.value
        if v.numel() == 0:
            return
        x, y, s = self._table(be.device)
        be.apply_ktable(s, v, outv, field.start, field.Nmesh, field.BoxSize)

    # ---- gradients with respect to the field and the table values --------------------------------------------------

    def _check(self, name, f, like=None):
        from .pm import BaseComplexField
        if not isinstance(f, BaseComplexField):
            raise TypeError('%s must be a ComplexField, not %s' % (name, type(f).__name__))
        if f.value.dim() > _abi.PMX_MAXDIM:
            raise NotImplementedError('tabulated transfers on meshes of more than %d dimensions' % _abi.PMX_MAXDIM)
        if like is not None and (type(f) is not type(like) or tuple(f.value.shape) != tuple(like.value.shape)
                                 or tuple(f.start) != tuple(like.start) or f.value.dtype != like.value.dtype):
            raise ValueError('%s must have the layout and dtype of the field' % name)
        return f

    def apply_vjp(self, field, v, out_t=True):
        """The gradients of ``field.apply(self)`` for the cotangent v (a ComplexField of field's layout):
        (grad_field, grad_t).  grad_field = v.apply(self) (T is real: its own adjoint).  grad_t (out_t) is a numpy
        array of len(t), summed over pm.comm: the derivative of Re(v.cdot(field.apply(self))) with respect to t,

            grad_t[i] = amplitude * sum_m w_m Re(conj(v_m) field_m) dinterp(|k_m|) / dt_i

        by one reduction kernel (csrc/pmx_ktable_grad.hip, include/pmesh_amd.h: pmx_ktable_vjp).  Between two entries
        a linear table weighs them 1 - f and f; a log-log table the same times interp(|k|) / t_i; outside the table
        `left` and `right` are constants and the weight is 0."""
        self._check('field', field)
        self._check('v', v, field)
        grad_field = v.apply(self)
        if not out_t:
            return grad_field, None
        be = backend.get()
        n = len(self.t)
        g = torch.zeros(n, dtype=torch.float64, device=be.device)
        if field.value.numel():
            x, y, s = self._table(be.device)
            be.ktable_vjp(s, field.compressed, field.value, v.value, field.start, field.Nmesh, field.BoxSize, g)
        comm = field.pm.comm
        if comm.size > 1:
            g = comm.allreduce(g)
        g = g.cpu().numpy() * self.amplitude
        if self.loglog:
            g = g / self.t
        return grad_field, g

    def apply_jvp(self, field, v_field=None, v_t=None):
        """The tangent of ``field.apply(self)`` along v_field (a ComplexField of field's layout) and v_t (len(t)
        values): a ComplexField.  The field part is v_field.apply(self); the table part of a linear table is the
        table of v_t applied to the field, that of a log-log table T(|k|) times the interpolation in ln k of v_t / t
        (the kernel pmx_apply_ktable_jvp)."""
        self._check('field', field)
        out = None
        if v_field is not None:
            out = self._check('v_field', v_field, field).apply(self)
        if v_t is not None:
            v_t = numpy.array(v_t, dtype='f8')
            if v_t.shape != self.t.shape or not numpy.isfinite(v_t).all():
                raise ValueError('v_t must hold %d finite values' % len(self.t))
            if not self.loglog:
                part = field.apply(Tabulated(self.k, v_t, amplitude=self.amplitude, left=0.0, right=0.0))
            else:
                be = backend.get()
                from .pm import _blank
                hip = be.name == 'hip' and field.value.numel()
                part = _blank(type(field), field.pm) if hip else field.pm.create(type=type(field))
                if field.value.numel():
                    x, y, s = self._table(be.device)
                    dy = torch.from_numpy(v_t / self.t).to(be.device)
                    be.apply_ktable_jvp(s, dy, field.value, part.value, field.start, field.Nmesh, field.BoxSize)
            if out is None:
                out = part
            else:
                out.value[...] += part.value
        if out is None:
            out = field.pm.create(type=type(field))
            out.value[...] = 0
        return out

    def interp(self, kmag):
        """interp(|k|) of the class docstring on a numpy array"""
        kmag = numpy.asarray(kmag, dtype='f8')
        if not self.loglog:
            return numpy.interp(kmag, self.k, self.t, left=self.left, right=self.right)
        inside = (kmag >= self.k[0]) & (kmag <= self.k[-1])
        with numpy.errstate(divide='ignore', invalid='ignore'):
            u = numpy.log(numpy.where(inside, kmag, self.k[0]))
        return numpy.where(inside, numpy.exp(numpy.interp(u, self._x, self._y)),
                           numpy.where(kmag < self.k[0], self.left, self.right))

    def __call__(self, k, v):
        """ the same transfer as a reference-style filter func(k, v), kind='wavenumber' (evaluated on the host) """
        from ._devarr import DevArr
        k2 = 0
        for ki in k:
            ki = ki.cpu().numpy() if isinstance(ki, (torch.Tensor, DevArr)) else numpy.asarray(ki)
            k2 = k2 + ki * ki
        f = self.amplitude * self.interp(numpy.sqrt(k2))
        if isinstance(v, DevArr):
            return DevArr(v.t * torch.from_numpy(numpy.ascontiguousarray(f)).to(v.t.device))
        if isinstance(v, torch.Tensor):
            return v * torch.from_numpy(numpy.ascontiguousarray(f)).to(v.device)
        return f * v
