"""ParticleMesh / RealField / ComplexField: the host-side mirror of ``pmesh/pm.py``.

The operator surface of the PM cycle keeps the reference's names, arguments,
defaults and semantics (file:line cited per method, relative to the reference
tree):

    ParticleMesh(Nmesh, BoxSize, comm, np, dtype, plan_method, resampler)   pm.py:1295
    pm.create / decompose / paint / generate_uniform_particle_grid ...      pm.py:1602, 1754, 1795, 1705
    RealField.r2c / readout / apply / csum / cmean / cdot / cnorm           pm.py:655, 745, 881, 725
    ComplexField.c2r / apply / cdot / cnorm                                 pm.py:987, 1047, 935, 911

What is different is where the data lives and who computes: field values are
device tensors (``field.value`` is a torch view of HBM; ``numpy.asarray(field)``
copies to the host), particles may be device tensors too, and every per-element
operation is a HIP kernel or rocFFT behind include/pmesh_amd.h — this module is
orchestration only.  Objects of the reference that were PFFT's are in
``pmesh_amd.fft``.
"""
import functools
import numbers
import operator
import os
import warnings
import weakref
from collections import OrderedDict

import numpy
import torch
from numpy.lib.mixins import NDArrayOperatorsMixin as NDArrayLike

from . import _abi, backend, domain
from . import fft as _fft
from ._arrays import to_device, is_tensor, torch_dtype, numpy_dtype, to_numpy, vec
from ._devarr import DevArr, unwrap as _dev_unwrap
from .comm import default_comm
from .transfer import Transfer
from .window import FindResampler, Affine

_gettype = type


def is_inplace(out):
    return out is Ellipsis


class _BlockGeometry(object):
    """shape / strides / element size of a rank's real block as ResampleWindow._painter reads them off a tensor (the
    geometry of a bin plan without a field to go with it: ParticleMesh.tile_order)"""
    def __init__(self, shape, strides, elsize):
        self.shape, self._strides, self._elsize = tuple(shape), tuple(strides), elsize

    def dim(self):
        return len(self.shape)

    def element_size(self):
        return self._elsize

    def stride(self, d=None):
        return self._strides if d is None else self._strides[d]


def _deprecated(message, replacement, *args):
    warnings.warn(message, DeprecationWarning, stacklevel=3)
    return replacement(*args)


def _position_gradient_target(out_pos, pos, gradient):
    """where readout_vjp / paint_vjp put the gradient with respect to the positions (pm.py:820-826, 1908-1914): a new
    array, or — out_pos=Ellipsis or the position array itself — over the positions, which are then read from a
    copy.  Returns (out_pos, pos to read)."""
    if gradient is not None:
        raise ValueError("gradient of gradient is not yet supported")
    if out_pos is None:
        return _zeros_like(pos), pos
    if is_inplace(out_pos) or out_pos is pos:
        return pos, _copy(pos)
    return out_pos, pos


# numpy ufunc -> torch function, so that `rho1[...] *= fac`, `field + 1`, abs(field) ...
# stay on the device (Field.__array_ufunc__, pm.py:169-208)
_UFUNCS = {
    numpy.add: torch.add, numpy.subtract: torch.sub, numpy.multiply: torch.mul,
    numpy.true_divide: torch.true_divide, numpy.negative: torch.neg, numpy.absolute: torch.abs,
    numpy.power: torch.pow, numpy.conjugate: torch.conj, numpy.exp: torch.exp, numpy.log: torch.log,
    numpy.sqrt: torch.sqrt, numpy.square: torch.square, numpy.sin: torch.sin, numpy.cos: torch.cos,
    numpy.equal: torch.eq, numpy.not_equal: torch.ne, numpy.less: torch.lt, numpy.greater: torch.gt,
    numpy.less_equal: torch.le, numpy.greater_equal: torch.ge, numpy.maximum: torch.maximum,
    numpy.minimum: torch.minimum,
}


class xslab(list):
    """the broadcastable coordinate arrays of one slab; normp() is their p-norm (pm.py:122-136)."""
    def normp(self, p=2, zeromode=None):
        total = None
        for coord in self:
            term = abs(coord) ** p
            total = term if total is None else total + term
        if zeromode is not None:
            total[total == 0] = zeromode
        return total


def _slab_cut(field):
    """how a slab iteration cuts `field`: (axis iterated over, number of slabs, function that brings that axis to
    the front of an array with the field's dimensions).  The axis is the one with the largest stride — slabs are
    then contiguous pieces of the buffer; a 2-d field is one slab (pm.py:90-104)."""
    if field.ndim == 2:
        return 2, 1, (lambda t: t[None, ...])
    strides = field.value.stride()
    order = sorted(range(field.ndim), key=lambda d: (strides[d], d), reverse=True)
    return order[0], int(field.shape[order[0]]), (lambda t: t.permute(order))


class slabiter(object):
    """ iterate over the slowest-varying axis of a field to gain locality, yielding the
        slab values with their sparse coordinates attached (pm.py:87-120). """
    def __init__(self, field, value):
        self.axis, self.nslabs, front = _slab_cut(field)
        self._values = front(value)
        self._coords = {'x': [front(c) for c in field.x], 'i': [front(c) for c in field.i]}
        self.Nmesh, self.BoxSize = field.Nmesh, field.BoxSize
        self.x = xslabiter(self, 'x')
        self.i = xslabiter(self, 'i')

    def _coords_of(self, which, irow):
        # every axis but the iterated one keeps its single broadcast entry
        return [DevArr(c[irow if d == self.axis else 0]) for d, c in enumerate(self._coords[which])]

    def __iter__(self):
        # (the slabs are numpy-flavoured handles on views of the field, _devarr.DevArr, as the arguments of an apply
        # callable are: `numpy.abs(slab) ** 2`, `slab[...] *= w` work on the device and write through to the field;
        # `slab.t` is the tensor)
        for irow in range(self.nslabs):
            s = DevArr(self._values[irow])
            s.x, s.i = self._coords_of('x', irow), self._coords_of('i', irow)
            s.Nmesh, s.BoxSize = self.Nmesh, self.BoxSize
            yield s


class xslabiter(object):
    """ the coordinate side of a slab iteration: per slab, the broadcastable coordinate arrays
    with the iteration axis cut down to that slab (pm.py:138-153) """
    def __init__(self, slabs, which):
        self._slabs, self._which = slabs, which
        self.axis, self.nslabs = slabs.axis, slabs.nslabs
        self.BoxSize, self.Nmesh = slabs.BoxSize, slabs.Nmesh

    def __iter__(self):
        for irow in range(self.nslabs):
            slab = xslab(self._slabs._coords_of(self._which, irow))
            slab.BoxSize, slab.Nmesh = self.BoxSize, self.Nmesh
            yield slab


class Field(NDArrayLike):
    """ Base class for RealField and ComplexField (pm.py:156-648). """
    __array_priority__ = 20.0
    _HANDLED_TYPES = (numpy.ndarray, numbers.Number, torch.Tensor)

    def __repr__(self):
        if hasattr(self, 'value'):
            return '%s:' % self.__class__.__name__ + repr(self.value)
        return '%s:' % self.__class__.__name__

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        out = kwargs.get('out', ())
        known = self._HANDLED_TYPES + (Field,)
        if not all(isinstance(x, known) for x in tuple(inputs) + tuple(out)):
            return NotImplemented
        dev = self.value.device

        def unwrap(x):
            if isinstance(x, Field):
                return x.value
            if isinstance(x, numpy.ndarray):
                return torch.from_numpy(numpy.ascontiguousarray(x)).to(dev)
            return x

        tf = _UFUNCS.get(ufunc) if method == '__call__' else None
        if tf is not None:
            args = tuple(unwrap(x) for x in inputs)
            if not any(isinstance(a, torch.Tensor) for a in args):
                args = (torch.as_tensor(args[0], device=dev),) + args[1:]
            result = tf(*args)
            if out:
                o = unwrap(out[0])
                o.copy_(result)
                result = o
        else:
            # host round trip for anything torch has no direct equivalent of
            hin = tuple(x.value.cpu().numpy() if isinstance(x, Field) else
                        (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in inputs)
            kw = dict(kwargs)
            kw.pop('out', None)
            r = getattr(ufunc, method)(*hin, **kw)
            if method == 'at':
                return None
            if type(r) is tuple:
                return tuple(self._cast_result(torch.from_numpy(numpy.asarray(x)).to(dev)) for x in r)
            result = torch.from_numpy(numpy.ascontiguousarray(r)).to(dev)
            if out:
                o = unwrap(out[0])
                o.copy_(result)
                result = o
        return self._cast_result(result)

    def _cast_result(self, result):
        # booleans and different shapes cannot be reasonable Field objects (pm.py:189-199)
        if result.dtype == torch.bool:
            return result
        if tuple(result.shape) != tuple(self.shape):
            return result
        if out_is_view_of(result, self.value):
            return self
        return self.pm.create(_gettype(self), value=result)

    def copy(self):
        return self.pm.create(_gettype(self), value=self.value)

    def _check_compatible(self, other):
        # two fields must be of one kind; anything else only has to have this field's local shape (pm.py:210-216)
        if not isinstance(other, Field):
            assert tuple(numpy.shape(other)) == tuple(int(n) for n in self.shape)
        elif not isinstance(other, _gettype(self)):
            raise TypeError("type of two operands of cdot must be the same type")

    def __init__(self, pm, base=None):
        """ bind a local buffer of `pm`'s partition and mirror the attributes callers read off a
        field (pm.py:220-265): value / start / cshape / shape / size / dtype / slices / csize """
        if not isinstance(self, (RealField, TransposedComplexField, UntransposedComplexField)):
            raise TypeError("Only RealField and ComplexField. No more subclassing")
        self.pm = pm
        self.BoxSize, self.Nmesh, self.ndim = pm.BoxSize, pm.Nmesh, len(pm.Nmesh)
        # what depends only on the mesh and the kind of field is worked out once per ParticleMesh (a time-stepping
        # caller makes two or three field objects per step)
        meta = pm._field_meta.get(type(self))
        if meta is None:
            meta = pm._field_meta[type(self)] = self._describe(pm)
        (self._partition, real, self.start, self.cshape, self.csize, self.shape, self.size, self.dtype, self.slices) = meta
        buf = self._base = _fft.LocalBuffer(self._partition, pm._rdtype, base=base)
        self._value = buf.view_input() if real else buf.view_output()

    @classmethod
    def _describe(cls, pm):
        """(partition, real?, start, cshape, csize, shape, size, dtype, slices) of this kind of field on `pm`"""
        part = pm._get_partition(cls)
        real = issubclass(cls, RealField)
        start, edges, shape = ((part.local_i_start, part.i_edges, part.local_i_shape) if real else
                               (part.local_o_start, part.o_edges, part.local_o_shape))
        shape = tuple(int(n) for n in shape)
        cshape = numpy.array([e[-1] for e in edges], dtype='intp')       # the collective shape
        if real and not getattr(part, 'is_c2c', False):
            dtype = numpy.dtype(pm._rdtype)
        else:
            dtype = numpy.dtype('c16' if numpy.dtype(pm._rdtype).itemsize == 8 else 'c8')
        # where the local block sits in the collective array
        slices = tuple(slice(int(a), int(a) + int(n)) for a, n in zip(start, shape))
        return (part, real, start, cshape, int(numpy.prod(cshape, dtype='i8')), shape,
                int(numpy.prod(shape, dtype='i8')), dtype, slices)

    # `value` is the view of the local block (pm.py:234-242).  A forward transform on one rank may have left its
    # last pass for the inverse transform that usually follows at once (fft.DEFER_LAST_PASS): whoever looks at
    # the values first makes it happen.
    @property
    def value(self):
        _fft.settle(self._base.storage)
        return self._value

    @value.setter
    def value(self, v):
        self._value = v

    # views of the same memory: the components and the (..., 2) real layout of a complex field
    @property
    def real(self):
        return self.value.real

    @property
    def imag(self):
        return self.value.imag

    @property
    def plain(self):
        return torch.view_as_real(self.value)

    # coordinates are built lazily: the fused kernels never read them
    @property
    def x(self):
        return self.pm.create_coords(type(self), return_indices=False)

    @property
    def i(self):
        return self.pm.create_coords(type(self), return_indices=True)

    @property
    def slabs(self):
        return slabiter(self, self.value)

    @property
    def flat(self):
        return numpy.asarray(self).flat

    @property
    def compressed(self):
        return self.cshape[-1] != self.Nmesh[-1]

    def __array__(self, dtype=None, copy=None):
        a = self.value.cpu().numpy()
        if dtype is not None:
            a = a.astype(dtype)
        return a

    def __getitem__(self, index):
        return self.value.__getitem__(index)

    def __setitem__(self, index, y):
        if isinstance(y, Field):
            y = y.value
        if isinstance(y, DevArr):           # (what a slab loop or an apply callable computed)
            y = y.t
        if isinstance(y, torch.Tensor):
            if y.data_ptr() == self.value.data_ptr() and tuple(y.shape) == tuple(self.value.shape) \
                    and y.stride() == self.value.stride() and index is Ellipsis:
                return  # `field[...] *= a`: the in-place result is being stored onto itself
            self.value[index] = y.to(self.value.device)
        elif isinstance(y, numbers.Number):
            self.value[index] = y
        else:
            a = numpy.asarray(y)
            t = torch.from_numpy(numpy.ascontiguousarray(a)).to(self.value.device)
            if not self.value.is_complex() and t.is_complex():
                raise TypeError('cannot assign complex values to a real field')
            self.value[index] = t.to(self.value.dtype) if t.dtype != self.value.dtype else t

    def _ctol(self, index):
        """ collective index -> (array it addresses, local index or None if another rank owns it);
        a complex field takes one extra entry, 0 / 1, for the real / imaginary part """
        index = [int(i) for i in index]
        nd = self.ndim
        if len(index) not in (nd, nd + 1):
            raise IndexError("Only vector index in global indexing is supported. for complex append 0 or 1 for real and imag")
        target = self.plain if len(index) == nd + 1 else self.value
        local = []
        for d in range(nd):
            g = index[d] + int(self.Nmesh[d]) if index[d] < 0 else index[d]      # negative: from the end
            l = g - int(self.start[d])
            if not 0 <= l < self.shape[d]:
                return target, None
            local.append(l)
        return target, tuple(local + index[nd:])

    def cgetitem(self, index):
        """ get a value from absolute index collectively (pm.py:287-296). """
        value, localindex = self._ctol(index)
        if localindex is not None:
            ret = value[tuple(int(i) for i in localindex)].item()
        else:
            ret = 0
        # every rank must bring the same kind of number to the collective
        return self.pm.comm.allreduce(complex(ret) if value.is_complex() else float(ret))

    def csetitem(self, index, y):
        """ set a value at an absolute index collectively; maintains Hermitian conjugation
            (pm.py:298-345).  Returns the value that was actually set.

            A complex field stores one of every conjugate pair (k, -k); setting mode k also sets
            its partner -k (if this rank holds it) to conj(y).  A mode that is its own partner
            keeps only the real part.  With a trailing 0 / 1 the index addresses the real /
            imaginary component alone (the partner's imaginary part gets the opposite sign, and
            the imaginary part of a self-conjugate mode cannot be set: 0 is returned). """
        index = numpy.array(index, copy=True)
        component = len(index) == self.ndim + 1            # (..., 0 | 1): one component
        value, here = self._ctol(index)
        there = None
        if isinstance(self, BaseComplexField):
            partner = index.copy()
            partner[:self.ndim] = (self.Nmesh - index[:self.ndim]) % self.Nmesh
            there = self._ctol(partner)[1]
        mine = y if here is not None else 0
        theirs = y if there is not None else 0
        selfconj = here is not None and here == there
        if component:
            if index[-1] == 1:
                theirs = -theirs
                if selfconj:
                    mine = theirs = 0
        elif len(index) == self.ndim:
            theirs = numpy.conjugate(theirs)
            if selfconj:
                mine = numpy.real(mine)
                theirs = numpy.real(theirs)
        if here is not None:
            value[tuple(int(i) for i in here)] = mine
        if there is not None:
            value[tuple(int(i) for i in there)] = theirs
        # every rank brings the same kind of number to the collective
        r = self.pm.comm.allreduce(complex(mine) if value.is_complex() else float(numpy.real(mine)))
        if isinstance(r, complex) and r.imag == 0 and not isinstance(mine, complex):
            r = r.real
        return r

    # ---- C-order redistribution (pm.py:384-448; the reference uses mpsort) --------------
    def _cindex(self):
        """ position of every local element in the C-ordered global array (int64 tensor) """
        dev = self.value.device
        g = torch.zeros([int(n) for n in self.shape], dtype=torch.int64, device=dev)
        for d in range(self.ndim):
            idx = torch.arange(int(self.start[d]), int(self.start[d]) + int(self.shape[d]), device=dev)
            g = g * int(self.cshape[d]) + idx.reshape([-1 if dd == d else 1 for dd in range(self.ndim)])
        return g

    # the deprecated spellings of ravel / unravel (pm.py:381-387)
    def sort(self, out=None):
        return _deprecated("Use ravel instead of sort", self.ravel, out)

    def unsort(self, flatiter):
        return _deprecated("Use pm.unravel instead of unsort", self.unravel, flatiter)

    def ravel(self, out=None):
        """ Ravel the field to 'C'-order, partitioned by ranks: rank r receives the next
            `self.size` items of the global C-ordered sequence (pm.py:389-424).

            out : None (a new 1-d device tensor is returned), Ellipsis (in place: the local
            buffer is overwritten), a device tensor, or a numpy array / flatiter (filled on
            the host).  Returns what was filled. """
        n = int(self.size)
        if self.pm.comm.size > 1:
            offs = _flat_offsets(self.pm.comm, n)
            res = torch.empty(n, dtype=self.value.dtype, device=self.value.device)
            _cpush(self.pm.comm, self.value.reshape(-1), self._cindex().reshape(-1), res, offs)
        else:
            res = self.value.reshape(-1)          # a single rank is already in C order
        if out is None:
            return res.clone() if self.pm.comm.size == 1 else res
        if is_inplace(out):
            self.value[...] = res.reshape(self.value.shape)
            return self.value
        if is_tensor(out):
            out.reshape(-1).copy_(res)
            return out
        flat = out if isinstance(out, numpy.flatiter) else out.flat
        assert len(flat) == n
        flat[...] = res.cpu().numpy()
        return flat

    def unravel(self, flatiter):
        """ Fill the field from C-ordered values partitioned over the ranks in any way
            (pm.py:426-448): `flatiter` is this rank's consecutive piece (numpy array, flatiter or
            device tensor); the pieces of all ranks, in rank order, are the global array. """
        if is_tensor(flatiter):
            flat = flatiter.reshape(-1)
        else:
            if not isinstance(flatiter, numpy.flatiter):
                flatiter = numpy.asarray(flatiter).flat
            a = numpy.array(flatiter, copy=True)
            a.setflags(write=True)
            flat = torch.from_numpy(a).to(self.value.device)
        if flat.dtype != self.value.dtype:
            flat = flat.to(self.value.dtype)
        comm = self.pm.comm
        assert comm.allreduce(int(flat.numel())) == self.csize
        if comm.size > 1:
            offs = _flat_offsets(comm, int(flat.numel()))
            vals = _ctake(comm, flat, offs, self._cindex().reshape(-1))
            self.value[...] = vals.reshape(self.value.shape)
        else:
            self.value[...] = flat.reshape(self.value.shape)

    def resample(self, out):
        """ Resample the Field by filling 0 or truncating modes.  Convert from and between
            Real/Complex automatically (pm.py:479-547).

            out : Field of another ParticleMesh (RealField or a complex field). """
        assert isinstance(out, Field)
        if all(out.Nmesh == self.Nmesh):
            # no resampling needed, just the Fourier transforms (the reference then still runs
            # the mode loop below, which removes the Nyquist planes; kept)
            self.cast(type=_gettype(out), out=out)
        src = self.cast(type=TransposedComplexField)
        complex = out.pm.create(type=TransposedComplexField, base=out._base, value=0)
        tmp = src.ravel()
        dev = tmp.device
        # indtable stores the index in the source for the mode in the destination
        indtable = [reindex(int(src.Nmesh[d]), int(out.Nmesh[d])) for d in range(src.ndim)]
        ind = build_index([t[numpy.r_[sl]] for t, sl in zip(indtable, complex.slices)], src.cshape)
        ind = torch.from_numpy(ind).to(dev)
        mask = ind >= 0
        argind = ind[mask]
        if src.pm.comm.size > 1:
            data = _ctake(src.pm.comm, tmp, _flat_offsets(src.pm.comm, int(tmp.numel())), argind)
        else:
            data = tmp[argind]
        complex.value[mask] = data.to(complex.value.dtype)
        # ensure the down sample is real; remove the Nyquist planes of the output and of the input
        ii = [torch.arange(int(st), int(st) + int(n), device=dev).reshape([-1 if dd == d else 1 for dd in range(src.ndim)])
              for d, (st, n) in enumerate(zip(complex.start, complex.shape))]
        selfconj = functools.reduce(operator.and_, [(int(n) - i) % int(n) == i for i, n in zip(ii, complex.Nmesh)])
        selfconj = selfconj.expand(complex.value.shape)
        complex.value.imag[selfconj] = 0
        for Nm in (complex.Nmesh, src.Nmesh):
            nyq = functools.reduce(operator.or_, [i == int(n) // 2 for i, n in zip(ii, Nm)])
            complex.value[nyq.expand(complex.value.shape)] = 0
        if isinstance(out, RealField):
            complex.c2r(out)
        elif complex._base is not out._base or _gettype(out) is not TransposedComplexField:
            complex.cast(type=_gettype(out), out=out)
        return out

    def preview(self, Nmesh=None, axes=None, resampler=None, method=None):
        """ gathers the mesh into a numpy array (with reduced resolution), projected onto
            `axes`, broadcast to all ranks (pm.py:549-615).

            Nmesh : desired Nmesh of the result or None; axes : axes to preserve;
            method : "upsample" | "downsample" | None (by the direction of the change). """
        keep = list(range(self.ndim)) if axes is None else (list(axes) if hasattr(axes, '__iter__') else [axes])
        field = self.c2r() if isinstance(self, BaseComplexField) else self
        if Nmesh is not None:
            want = numpy.ones(self.ndim, dtype='intp') * numpy.asarray(Nmesh)
            if not all(want == field.Nmesh):
                if method is None:
                    method = 'downsample' if any(want < field.Nmesh) else 'upsample'
                if method not in ('downsample', 'upsample'):
                    raise ValueError("method can only be downsample or upsample")
                field = getattr(field.pm.reshape(want), method)(field, resampler=resampler, keep_mean=True)
        # project on the device (sum over the axes that go), then every rank adds its block into the global image
        gone = [d for d in range(self.ndim) if d not in keep]
        image = field.value.permute(keep + gone)
        if gone:
            image = image.sum(dim=tuple(range(len(keep), self.ndim)))
        result = numpy.zeros([field.cshape[d] for d in keep], dtype=field.dtype)
        result[tuple(field.slices[d] for d in keep)] += image.cpu().numpy()
        return numpy.asarray(self.pm.comm.allreduce(result))

    def cast(self, type=None, out=None):
        """ cast the field object to the given type, maintaining the meaning of the field
            (pm.py:450-477). """
        if type is None and out is None:
            raise ValueError('either type or out must be given')
        if out is None:
            out = self.pm.create(type=_typestr_to_type(type))
        elif type is not None and not isinstance(out, _typestr_to_type(type)):
            raise TypeError('out is not of the requested type')
        if isinstance(self, RealField) and isinstance(out, RealField):
            if out is not self:
                out.value[...] = self.value
            return out
        if isinstance(self, RealField) and isinstance(out, BaseComplexField):
            return self.r2c(out=out)
        if isinstance(self, BaseComplexField) and isinstance(out, RealField):
            return self.c2r(out=out)
        if isinstance(self, BaseComplexField) and isinstance(out, BaseComplexField):
            if _gettype(self) is _gettype(out):
                if out is not self:
                    out.value[...] = self.value
                return out
            if self.pm.comm.size == 1:
                out.value[...] = self.value
                return out
            if out._base in self._base:
                raise ValueError('the layouts differ: this cast cannot be done in place')
            to_u = isinstance(out, UntransposedComplexField)
            self.pm.plans['forwardU'].retranspose(self._base, out._base, to_u)
            return out
        raise TypeError('unsupported cast')

    def apply(self, func, kind, out):
        """ implements all kinds of apply operations (pm.py:617-648).

        `func` is either a :class:`pmesh_amd.transfer.Transfer` (the fused transfer-function
        kernel: one launch, no coordinate arrays are read) or a callable ``func(x, v)`` as in
        the reference.  A callable is first tried on device tensors (coordinates and values
        stay in HBM; works for lambdas built from operators and broadcasting); if it only
        understands numpy it is evaluated on the host, slab by slab as the reference does.
        """
        if out is None:
            # (every value of the new field is written below; only the GPU backend hands out raw memory)
            out = _blank(_gettype(self), self.pm) if backend.get().name == 'hip' else self.pm.create(type=_gettype(self))
        if is_inplace(out):
            out = self
        if isinstance(out, Field):
            assert isinstance(out, _gettype(self))
            outv = out.value
        else:
            outv = out
        assert tuple(outv.shape) == tuple(self.value.shape)

        if isinstance(func, Transfer):
            if not isinstance(self, BaseComplexField):
                raise TypeError('fused transfer functions apply to complex fields')
            if kind not in ('wavenumber', 'circular'):
                raise ValueError('fused transfer functions need kind wavenumber or circular')
            func._launch(self, outv)
            return out

        x, i = self.x, self.i
        if kind in ('relative', 'absolute', 'wavenumber'):
            coords = xslab(x)
        elif kind == 'index':
            coords = xslab(i)
        elif kind == 'circular':
            coords = xslab([ki * float(L) / float(N) for ki, L, N in zip(x, self.BoxSize, self.Nmesh)])
        else:
            raise ValueError("unknown kind of apply function.")
        coords.BoxSize = self.BoxSize
        coords.Nmesh = self.Nmesh
        # The callable sees numpy-flavoured handles on the device tensors (_devarr.DevArr): numpy ufuncs and the
        # functions transfer functions use run as torch operations in HBM, masks and nonzero() follow numpy's
        # conventions.  Whatever it cannot express (TypeError and friends) sends the callable to the host.
        v = self.value[...]
        version = v._version
        try:
            dcoords = xslab([DevArr(c) for c in coords])
            dcoords.BoxSize, dcoords.Nmesh = self.BoxSize, self.Nmesh
            dv = DevArr(v)
            dv.x, dv.i = xslab([DevArr(c) for c in x]), xslab([DevArr(c) for c in i])
            dv.BoxSize, dv.Nmesh = self.BoxSize, self.Nmesh
            r = _dev_unwrap(func(dcoords, dv), v.device)
            if not isinstance(r, torch.Tensor):
                r = torch.as_tensor(r, device=v.device)
            outv[...] = r
            return out
        except (TypeError, RuntimeError, ValueError, AttributeError, NotImplementedError) as ex:
            failure = ex
        if v._version != version:
            # (the host evaluation would start from values the failed attempt has already changed)
            raise RuntimeError('Field.apply: the callable modified its input in place and then failed on device arrays '
                               '(%s: %s); return a new array instead, or use operations numpy and torch share'
                               % (type(failure).__name__, failure))
        self._apply_host(func, kind, outv)
        return out

    def _apply_host(self, func, kind, outv):
        """The reference's slab loop on numpy arrays (pm.py:87-120, 633-647)."""
        host = self.value.cpu().numpy()
        res = numpy.empty_like(host)
        xs = [a.cpu().numpy() for a in self.x]
        is_ = [a.cpu().numpy() for a in self.i]
        for irow in range(host.shape[0]):
            def row(arrs):
                return [a[irow:irow + 1] if a.shape[0] != 1 else a for a in arrs]
            kx = xslab(row(xs))
            ki = xslab(row(is_))
            islab = host[irow:irow + 1].view(type=_hslab)
            islab.x, islab.i, islab.BoxSize, islab.Nmesh = kx, ki, self.BoxSize, self.Nmesh
            if kind in ('relative', 'absolute', 'wavenumber'):
                arg = kx
            elif kind == 'index':
                arg = ki
            else:
                arg = xslab([k * L / N for k, L, N in zip(kx, self.BoxSize, self.Nmesh)])
            arg.BoxSize, arg.Nmesh = self.BoxSize, self.Nmesh
            res[irow:irow + 1] = func(arg, islab)
        outv[...] = torch.from_numpy(res).to(outv.device)


class _hslab(numpy.ndarray):
    pass


slab = _hslab          # (the reference's name for the array type its slab iterators hand out, pm.py:84)


def out_is_view_of(a, b):
    return a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape) and a.stride() == b.stride()


class RealField(Field):
    def __init__(self, pm, base=None):
        Field.__init__(self, pm, base)

    def r2c(self, out=None):
        """ Perform real to complex transformation (pm.py:655-694); normalised by
            1/prod(Nmesh) on the forward transform (pm.py:692). """
        # a field object of the caller's: views of its value taken BEFORE this call must hold the finished spectrum
        # afterwards (in the reference `value` is a plain array, pm.py:234-242), so nothing is left deferred on it
        callers = out is not None and not is_inplace(out) and out is not self
        if out is None:
            # (one rank, LDS kernels: the first pass of the out-of-place transform writes the whole result)
            out = (_blank(TransposedComplexField, self.pm) if self.pm.plans['forwardT'].fills_output()
                   else TransposedComplexField(self.pm))
        elif is_inplace(out) or out is self:
            out = TransposedComplexField(self.pm, base=self._base)         # the spectrum over this field's own buffer
        assert isinstance(out, (BaseComplexField,))
        inplace = self._base in out._base and out._base in self._base
        T = 'U' if isinstance(out, UntransposedComplexField) else 'T'
        plan = self.pm.plans[('ipforward' if inplace else 'forward') + T]
        plan.execute(self._base, out._base)
        if callers:
            _fft.settle(out._base.storage)
        return out

    def ctranspose(self, axes):
        """ Collectively transpose a RealField: the coordinates are replaced according to the
            new set of axes (pm.py:696-723; as in the reference, through a nearest-neighbour
            readout and paint of one particle per mesh point). """
        assert len(numpy.unique(axes)) == self.ndim
        assert numpy.max(axes) == self.ndim - 1
        axes = numpy.array(axes, dtype='intp')
        pm = self.pm.reshape(BoxSize=self.BoxSize[axes], Nmesh=self.Nmesh[axes])
        q = self.pm.generate_uniform_particle_grid(shift=0)
        v = self.readout(q, resampler='nnb')
        q = q[..., torch.as_tensor(axes, device=q.device)].contiguous()
        layout = pm.decompose(q, smoothing='nnb')
        return pm.paint(q, mass=v, resampler='nnb', layout=layout)

    def csum(self, dtype=None):
        """ Collective sum of the entire mesh (pm.py:725-739). """
        s = self.value.sum(dtype=torch_dtype(dtype) if dtype is not None else None)
        return self.pm.comm.allreduce(s.item())

    def cmean(self, dtype=None):
        """ Collective mean of the entire mesh (pm.py:741-743). """
        return self.csum(dtype=dtype) / self.csize

    def readout(self, pos, hsml=None, out=None, resampler=None, transform=None, gradient=None, layout=None):
        """
        Read out from real field at positions (pm.py:745-791).

        pos : (, ndim) positions in simulation units; hsml : window scaling per particle;
        gradient : None or the direction of the window derivative; resampler : window name,
        default pm.resampler; layout : domain decomposition — positions are first routed to
        the ranks that hold the cells and the partial results are summed on the way back.
        """
        transform = transform or self.pm.affine
        resampler = FindResampler(self.pm.resampler if resampler is None else resampler)
        if layout is None:
            return resampler.readout(self.value, pos, hsml=hsml, out=out, transform=transform, diffdir=gradient)
        if _ghosts_only(layout, resampler, transform, hsml):
            # partial sums of the caller's own particles straight from the local block, plus
            # the partial sums of their ghosts on other ranks added on the way back
            be = backend.get()
            dpos, host = to_device(pos, be.device, 'pos')
            # a caller's device buffer takes the result directly (no fresh tensor per call)
            direct = (is_tensor(out) and out.device == be.device and out.dtype in (torch.float64, torch.float32) and
                      out.dim() == 1 and out.shape[0] == dpos.shape[0])      # (any stride: a column of an (n, 3) force array)
            pending = None
            if layout.comm.size > 1:
                # the ghosts first: their partial sums travel back to their owners (on RCCL's stream) while the
                # caller's own particles — almost all of the work — are read out
                rpos = layout.exchange_remote(dpos)
                rres = resampler.readout(self.value, rpos, transform=transform, diffdir=gradient)
                pending = layout.gather_remote_add(rres, None, async_op=True)
            res = resampler.readout(self.value, dpos, out=out if direct else None, transform=transform,
                                    diffdir=gradient)
            if pending is not None:
                pending.wait(res)
            if direct:
                return out
            if out is not None:
                if is_tensor(out):
                    out.copy_(res)
                else:
                    to_numpy(res, out=out)
                return out
            return to_numpy(res) if host else res
        localpos = layout.exchange(pos)
        localhsml = exchange(layout, hsml)
        localresult = self.readout(localpos, hsml=localhsml, resampler=resampler, transform=transform,
                                   gradient=gradient, out=None, layout=None)
        return layout.gather(localresult, out=out)

    def readout_vjp(self, pos, v, resampler=None, transform=None, gradient=None,
                    out_self=None, out_pos=None, layout=None):
        """ back-propagate the gradient of readout (pm.py:793-846). """
        if out_pos is not False:
            out_pos, pos = _position_gradient_target(out_pos, pos, gradient)
            for d in range(pos.shape[1]):
                r = self.readout(pos, resampler=resampler, transform=transform, gradient=d, layout=layout)
                out_pos[:, d] = _mul(r, v)
        if out_self is not False:
            out_self = RealField(self.pm) if out_self is None else (self if is_inplace(out_self) else out_self)
            self.pm.paint(pos, mass=v, resampler=resampler, transform=transform, gradient=gradient,
                          hold=False, layout=layout, out=out_self)
        return out_self, out_pos

    def readout_jvp(self, pos, v_self=None, v_pos=None, resampler=None, transform=None, gradient=None, layout=None):
        """ f_i = W_qi A_q (pm.py:848-859) """
        jvp = 0
        if v_pos is not None:
            for d in range(self.ndim):
                jvp = jvp + _mul(self.readout(pos, resampler=resampler, transform=transform, gradient=d,
                                              layout=layout), v_pos[..., d])
        if v_self is not None:
            jvp = jvp + v_self.readout(pos, resampler=resampler, transform=transform, gradient=None, layout=layout)
        return jvp

    def paint(self, pos, mass=1.0, resampler=None, transform=None, hold=False, gradient=None, layout=None):
        warnings.warn("Use ParticleMesh.paint instead", DeprecationWarning, stacklevel=2)
        self.pm.paint(pos, mass=mass, resampler=resampler, transform=transform, hold=hold,
                      gradient=gradient, layout=layout, out=self)

    def c2r_vjp(v, out=None):
        """ Back-propagate the gradient of c2r from self to out (pm.py:865-870) """
        out = v.r2c(out)
        out.value[...] *= float(numpy.prod(out.pm.Nmesh ** 1.0))
        return out

    def apply(self, func, kind="relative", out=None):
        """ apply a function func(r, y) to the field (pm.py:872-895); kind is 'relative'
            (distance from [-0.5 Boxsize, 0.5 BoxSize)), 'index' or 'absolute'. """
        assert kind in ['relative', 'index', 'absolute']
        return Field.apply(self, func, kind, out)

    def cdot(self, other):
        self._check_compatible(other)
        o = other.value if isinstance(other, Field) else torch.as_tensor(numpy.asarray(other), device=self.value.device)
        return self.pm.comm.allreduce(torch.sum(self.value * o).item())

    def cnorm(self):
        return self.cdot(self)


class BaseComplexField(Field):

    def _hermitian_weight(self):
        """ 2 for modes whose conjugate is not stored, 1 otherwise (pm.py:908-918). """
        if not self.compressed:
            return None
        il = self.i[-1]
        return 1 + ((il != 0) & (il != int(self.Nmesh[-1]) // 2)).to(self.value.real.dtype)

    def cnorm(self, metric=None, norm=None):
        r""" collective norm; the conjugates are added too (pm.py:920-945). """
        y = self.value.real ** 2 + self.value.imag ** 2 if norm is None else norm(self.value)
        if metric is not None:
            k = xslab(self.x).normp(p=2) ** 0.5
            y = y * metric(k)
        w = self._hermitian_weight()
        if w is not None:
            y = y * w
        return self.pm.comm.allreduce(y.sum().item())

    def cdot(self, other, metric=None):
        r""" Collective inner product between the independent modes of two Complex Fields
            (pm.py:947-975). """
        if isinstance(other, Field):
            if not isinstance(other, _gettype(self)):
                raise TypeError("type of two operands of cdot must be the same type")
            o = other.value
        else:
            o = torch.as_tensor(numpy.asarray(other), device=self.value.device)
        r = torch.conj(o) * self.value
        w = self._hermitian_weight()
        if w is not None:
            r = r * w
        if metric is not None:
            r = r * metric(xslab(self.x).normp() ** 0.5)
        return self.pm.comm.allreduce(complex(r.sum().item()))

    def cdot_vjp(self, v, metric=None):
        """ backtrace gradient of cdot against other (pm.py:977-985). """
        r = self * v
        if metric is not None:
            r.apply(lambda k, y: y * metric(k.normp() ** 0.5), out=Ellipsis)
        return r

    def c2r(self, out=None, transfer=None):
        """ complex to real transformation, unnormalised (pm.py:987-1019).

            transfer : optional :class:`pmesh_amd.transfer.Transfer` (an extension): the
            result is ``self.apply(transfer).c2r(out)``, with the multiplication fused into
            the first pass of the inverse transform when the column-FFT path is active
            (the complex field is then read once less).  `self` is left untouched unless
            the transform is in place (``out=Ellipsis``). """
        T = 'U' if isinstance(self, UntransposedComplexField) else 'T'
        if transfer is not None and not isinstance(transfer, Transfer):
            raise TypeError('transfer must be a pmesh_amd.transfer.Transfer')
        oop = self.pm.plans['backward' + T].fills_output()
        if out is None:
            out = _blank(RealField, self.pm) if oop and self.pm.comm.size == 1 else RealField(self.pm)
        elif is_inplace(out) or out is self:
            out = RealField(self.pm, self._base)                           # the real field over this spectrum's buffer
        assert isinstance(out, RealField)
        inplace = out._base in self._base and self._base in out._base
        src = self
        fusable = transfer is not None and transfer.fusable()
        if not inplace and self.pm.comm.size == 1:
            if transfer is not None and not (fusable and self.pm.plans['ipbackward' + T].can_fuse()):
                # a transfer function that is a kernel of its own moves the spectrum while it multiplies: self ->
                # the buffer of `out`, transformed in place there
                src = self.pm.create(type=_gettype(self), base=out._base)
                self.apply(transfer, out=src)
                transfer = None
                inplace = True
            elif not oop:
                # rocFFT may overwrite the input of an out-of-place real inverse; the reference
                # plans with PRESERVE_INPUT (pm.py:1335): transform a copy, in place in `out`
                src = self.pm.create(type=_gettype(self), base=out._base, value=self.value)
                inplace = True
            # else: the first pass of the LDS kernels reads `self` and writes `out` (with the transfer riding on it)
        plan = self.pm.plans[('ipbackward' if inplace else 'backward') + T]
        fused = None
        if transfer is not None:
            if fusable and plan.can_fuse():
                fused = (transfer._cstruct(), src.start, src.Nmesh, src.BoxSize)
            elif src is self and not inplace:
                src = self.apply(transfer)            # several ranks: the slab path copies anyway
            else:
                src.apply(transfer, out=Ellipsis)
        plan.execute(src._base, out._base, transfer=fused)
        return out

    def r2c_vjp(v, out=None):
        """ Back-propagate the gradient of r2c to self (pm.py:1021-1026). """
        out = v.c2r(out)
        out.value[...] *= float(numpy.prod(out.pm.Nmesh ** -1.0))
        return out

    def decompress_vjp(v, out=None):
        """ Back-propagate the gradient of decompress from self to out (pm.py:1028-1045). """
        if out is None:
            out = v.pm.create(type=_gettype(v))
        if is_inplace(out):
            out = v
        mask = torch.ones(v.shape, dtype=torch.bool, device=v.value.device)
        for ii, n in zip(out.i, out.Nmesh):
            n = int(n)
            mask &= ((n - ii) % n == ii)
        out.value[...] = torch.where(mask, v.value, 2 * v.value)
        return out

    def apply(self, func, kind="wavenumber", out=None):
        """ apply a function func(k, y) to the field (pm.py:1047-1070); kind is 'wavenumber'
            ([-2 pi/L N/2, 2 pi/L N/2)), 'circular' ([-pi, pi)) or 'index'.  `func` may be a
            fused :class:`pmesh_amd.transfer.Transfer`. """
        assert kind in ['wavenumber', 'circular', 'index']
        return Field.apply(self, func, kind, out)


class UntransposedComplexField(BaseComplexField):
    """ A complex field with untransposed representation (pm.py:1072-1078). """
    def __init__(self, pm, base=None):
        Field.__init__(self, pm, base)


class TransposedComplexField(BaseComplexField):
    """ A complex field with transposed representation. Faster for r2c/c2r (pm.py:1080-1086). """
    def __init__(self, pm, base=None):
        Field.__init__(self, pm, base)


# backward-compatbility, alias TranposedComplexField to ComplexField
ComplexField = TransposedComplexField


def _blank(cls, pm):
    """a new field on uninitialised memory, for whoever is about to write all of it (the padding between the rows and
    planes of the one-rank layout is never read as values)"""
    part = pm._get_partition(cls)
    return cls(pm, base=torch.empty(part.alloc_reals, dtype=torch_dtype(pm._rdtype), device=backend.get().device))


def _zeros_like(a):
    return torch.zeros_like(a) if is_tensor(a) else numpy.zeros_like(a)


def _copy(a):
    return a.clone() if is_tensor(a) else a.copy()


def _mul(a, b):
    if is_tensor(a) and not is_tensor(b):
        b = torch.as_tensor(numpy.asarray(b), device=a.device)
    if is_tensor(b) and not is_tensor(a):
        a = torch.as_tensor(numpy.asarray(a), device=b.device)
    return a * b


#: 'auto': paint/readout with a layout keep the caller's own particles in place and exchange
#: only the ghosts when the layout's routing covers the window; 'never': always the literal
#: exchange -> local operation -> gather of the reference (pm.py:1857-1868, 783-791)
GHOSTS_ONLY = 'auto'


def _is_scalar(value):
    return value is None or numpy.isscalar(value) or (hasattr(value, 'ndim') and value.ndim == 0)


def _ghosts_only(layout, resampler, transform, hsml):
    """ True when painting/reading the caller's own array in place plus the ghosts received
    from other ranks is the same set of (particle, cell) contributions as the reference's
    exchange-everything scheme: the layout must have been built by ParticleMesh.decompose for
    the same scaling and with a smoothing that covers the window (then a particle that was
    *not* routed to this rank cannot touch the local block, and one that was routed to its
    own rank is painted exactly once, in place). """
    route = getattr(layout, '_route', None)
    if GHOSTS_ONLY == 'never' or route is None or hsml is not None:
        return False
    smoothing, scale, translate, period = route
    same = lambda a, b: tuple(float(x) for x in numpy.asarray(a).ravel()) == b
    # a shifted or re-wrapped transform moves windows relative to the domains the particles were
    # routed by: only the literal exchange reproduces the reference then
    if not (same(transform.scale, scale) and same(transform.translate, translate) and same(transform.period, period)):
        return False
    return bool(numpy.all(smoothing >= 0.5 * resampler.support))


def build_index(indices, fullshape):
    """ Build a linear index array based on indices on an array of fullshape, similar to
        numpy.ravel_multi_index; an index of -1 on any axis gives -1 (pm.py:1091-1126). """
    localshape = [len(i) for i in indices]
    ndim = len(localshape)
    ind = numpy.zeros(localshape, dtype='i8')
    mask = numpy.zeros(localshape, dtype='?')
    for d in range(ndim):
        i = numpy.asarray(indices[d]).reshape([-1 if dd == d else 1 for dd in range(ndim)])
        ind[...] *= int(fullshape[d])
        ind[...] += i
        mask |= i == -1
    ind[mask] = -1
    return ind


def reindex(Nsrc, Ndest):
    """ the index in the frequency array of Nsrc for the corresponding k of Ndest; -1 for
        those of Ndest that do not exist in Nsrc (pm.py:1128-1144):
        reindex(8, 4) -> [0, 1, 2, 7];  reindex(4, 8) -> [0, 1, 2, -1, -1, -1, -1, 3] """
    r = numpy.arange(Ndest)
    r[Ndest // 2 + 1:] = numpy.arange(Nsrc - Ndest // 2 + 1, Nsrc, 1)
    r[Nsrc // 2 + 1: Ndest - Nsrc // 2 + 1] = -1
    return r


# ---- global C-order gather / scatter over the ranks (what the reference uses mpsort for) ----
def _flat_offsets(comm, n):
    """ offsets of the ranks' consecutive pieces of a global flat array """
    sizes = comm.allgather(int(n))
    return numpy.concatenate([[0], numpy.cumsum(sizes)]).astype('i8')


def _as_rows(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _route(comm, dest, payloads):
    """ send row k of every payload to rank dest[k]; returns the received payloads and what is
        needed to send answers back in the original order """
    order = torch.argsort(dest, stable=True)
    counts = torch.bincount(dest, minlength=comm.size).cpu().numpy().astype('i8')
    recvcounts = numpy.asarray(comm.alltoall_counts(counts)).astype('i8')
    nrecv = int(recvcounts.sum())
    got = []
    for p in payloads:
        rows = _as_rows(p[order].contiguous())
        r = torch.empty((nrecv,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
        comm.alltoallv(rows, counts, r, recvcounts)
        got.append(torch.view_as_complex(r) if p.is_complex() else r)
    return got, order, counts, recvcounts


def _cpush(comm, values, gidx, out, offs):
    """ out[g - offs[rank]] = v on the rank whose piece [offs[r], offs[r+1]) contains g """
    edges = torch.as_tensor(offs[1:], device=gidx.device)
    dest = torch.bucketize(gidx, edges, right=True)
    (g, v), _, _, _ = _route(comm, dest, [gidx, values])
    out[g - int(offs[comm.rank])] = v


def _ctake(comm, flat, offs, gidx):
    """ the values at global positions gidx of the flat array whose pieces the ranks hold """
    edges = torch.as_tensor(offs[1:], device=gidx.device)
    dest = torch.bucketize(gidx, edges, right=True)
    (g,), order, counts, recvcounts = _route(comm, dest, [gidx])
    ans = _as_rows(flat[g - int(offs[comm.rank])].contiguous())
    back = torch.empty((int(gidx.numel()),) + tuple(ans.shape[1:]), dtype=ans.dtype, device=ans.device)
    comm.alltoallv(ans, recvcounts, back, counts)
    if flat.is_complex():
        back = torch.view_as_complex(back)
    res = torch.empty_like(back)
    res[order] = back
    return res


def exchange(layout, value):
    """ pm.py:1146-1157: scalars are not exchanged """
    if value is None:
        return None
    if numpy.isscalar(value):
        return value
    if hasattr(value, 'ndim') and value.ndim == 0:
        return value
    return layout.exchange(value)


def _typestr_to_type(typestr):
    """ field class from its name or itself (pm.py:1159-1176): same names, same exceptions """
    names = {'real': RealField, 'complex': ComplexField, 'transposedcomplex': TransposedComplexField,
             'untransposedcomplex': UntransposedComplexField}
    cls = typestr if isinstance(typestr, type) else names.get(typestr)
    if cls is None:
        raise ValueError('mode must be real or complex, or ')
    if not issubclass(cls, Field):
        raise TypeError("mode must be a subclass of %s" % str(Field))
    return cls


def _block_coords(starts, shapes, Nmesh, BoxSize, dtype, device, spectral):
    """ per axis the global indices of a rank's block and their coordinates, each shaped to broadcast along its own
    axis: positions `i L / N` of the real side (pm.py:1178-1198) or wavenumbers `2 pi i / L` of the spectral side
    (pm.py:1200-1226) — indices at and beyond N // 2 count as negative, so the Nyquist mode is reported negative.
    Returns (coordinates, indices) as lists of device tensors; the arithmetic is done on the host in `dtype` with the
    reference's sequence of roundings. """
    ndim = len(shapes)
    coords, indices = [], []
    for d in range(ndim):
        n, first = int(shapes[d]), starts[d]
        along = [n if dd == d else 1 for dd in range(ndim)]
        index = numpy.arange(n, dtype='intp') + first
        signed = numpy.arange(n, dtype=dtype) + first
        signed[signed >= Nmesh[d] // 2] -= Nmesh[d]
        if spectral:
            signed *= (2 * numpy.pi / Nmesh[d])                     # radians per cell first, as the reference does
            c = (signed * Nmesh[d] / BoxSize[d]).astype(dtype)
        else:
            c = signed * BoxSize[d] / Nmesh[d]
        indices.append(torch.from_numpy(index.reshape(along)).to(device))
        coords.append(torch.from_numpy(numpy.ascontiguousarray(c.reshape(along))).to(device))
    return coords, indices


def _init_i_coords(partition, Nmesh, BoxSize, dtype, device):
    return _block_coords(partition.local_i_start, partition.local_i_shape, Nmesh, BoxSize, dtype, device, False)


def _init_o_coords(partition, Nmesh, BoxSize, dtype, device):
    return _block_coords(partition.local_o_start, partition.local_o_shape, Nmesh, BoxSize, dtype, device, True)


# ParticleMesh objects by (Nmesh, communicator, process mesh, dtype, plan method): a new object that
# matches a living one shares its process mesh and plans (pm.py:1362-1404: `_pm_cache`)
_pm_cache = weakref.WeakValueDictionary()


#: The halo merge of a tile-binned paint (csrc/pmx_binned.hip: halo_merge_kernel) left to the forward transform:
#: 'fresh' (default): when ParticleMesh.paint makes the field itself (out=None, hold=False, no layout) — r2c on one rank
#: then adds the staged halos inside its row pass, any other reader of the field runs the merge first; 'never';
#: 'always': also on a caller's `out` field (views of out.value taken BEFORE the paint then miss the halos until the
#: field is read through the field object — for callers that know they hold none, e.g. bench.py --out-field).
HALO_DEFER = os.environ.get('PMESH_AMD_HALO_DEFER', 'fresh')


class ParticleMesh(object):
    """
    ParticleMesh provides an interface to solver for forces with particle mesh method
    (pm.py:1245-1293).  It does not deal with memory: use RealField(pm) and ComplexField(pm)
    (or pm.create) for buffers, which live in HBM.

    Attributes: np, comm, Nmesh, ndim, BoxSize, dtype, domain, procmesh, partition, affine,
    affine_grid, resampler, plans.
    """

    def __init__(self, Nmesh, BoxSize=1.0, comm=None, np=None, dtype='f8',
                 plan_method='estimate', resampler='cic'):
        """ create a PM object (pm.py:1295-1488).

            plan_method : accepted for compatibility (`estimate`, `exhaustive`, `measure`);
                rocFFT has one planner.
            resampler : string or ResampleWindow, the default window
            np : the process mesh; None -> as the reference (pm.py:1317-1325): 3-d meshes get the
                pencil decomposition pfft.split_size_2d(comm.size) (8 ranks: [2, 4]), 2-d meshes a
                slab.  [comm.size] asks for a slab: one global transpose per FFT instead of two,
                the faster choice on 8 fully connected GPUs (bench.py uses it).
            Nmesh : tuple or alike; len(Nmesh) is the dimension of the system.
        """
        if comm is None:
            comm = default_comm()
        self.comm = comm
        if len(Nmesh) == 1 and self.comm.size != 1:
            raise ValueError("Running 1d transforms on multiple ranks is not supported")
        if plan_method not in ('estimate', 'measure', 'exhaustive'):
            raise KeyError(plan_method)
        if np is None:
            # the reference's default (pm.py:1317-1325): a 2-d process mesh for 3-d meshes, the
            # most square factorisation of the communicator; a slab for 2-d meshes
            if len(Nmesh) > 3:
                # [r6] meshes of 4 dimensions on several ranks: slabs along axis 0 (the reference hands PFFT a 2-d process
                # mesh here too, pm.py:1319; its test only builds such a mesh, test_pm.py:381-384) — the local stage of
                # a slab is one batched rocFFT plan over the trailing axes
                np = [self.comm.size]
            elif len(Nmesh) >= 3:
                np = list(_fft.split_size_2d(self.comm.size))
                if np[1] == 1:
                    # [P, 1] distributes axis 0 alone: exactly the slab [P], one transpose per transform
                    np = [self.comm.size]
                # ([1, P] — what split_size_2d gives for P = 3, 5, 7, ... — distributes axis 1 of the real field, as
                # PFFT lays it out; callers that read pm.partition see the reference's edges.  Rounds 1-3 built the
                # slab [P] here instead.  `np=[P]` asks for the slab explicitly.)
            elif len(Nmesh) == 2:
                np = [self.comm.size]
            else:
                np = []
        self.np = list(np)
        self._use_padded = True
        dtype = numpy.dtype(dtype)
        if dtype not in (numpy.dtype('f8'), numpy.dtype('f4'), numpy.dtype('c16'), numpy.dtype('c8')):
            raise ValueError("dtype must be f8, f4, c16 or c8")
        # a complex dtype makes the transforms complex-to-complex (pm.py:1270, 1326-1331): the
        # configuration-space field holds complex values and the spectrum is not compressed
        is_c2c = dtype.kind == 'c'
        rdtype = numpy.dtype('f%d' % (dtype.itemsize // 2)) if is_c2c else dtype
        self.Nmesh = numpy.array(Nmesh, dtype='i8')
        self.ndim = len(self.Nmesh)
        if self.ndim > _abi.PMX_MAXDIM_ND:
            raise NotImplementedError('meshes of more than %d dimensions' % _abi.PMX_MAXDIM_ND)
        self.BoxSize = numpy.empty(len(Nmesh), dtype='f8')
        self.BoxSize[:] = BoxSize
        self.dtype = dtype

        # A living ParticleMesh of the same mesh, communicator, process mesh and dtype lends its
        # process mesh (sub-communicators are a limited resource) and its plans (work buffers,
        # rocFFT plans): pm.py:1346-1404.  Collective: every rank must agree that it has one.
        cache_key = (tuple(int(x) for x in self.Nmesh), id(comm), comm.rank, comm.size, tuple(self.np),
                     dtype.str, plan_method, bool(_fft.PLANE_PAD),
                     id(backend._current) if backend._current is not None else id(self))
        template = _pm_cache.get(cache_key)
        if comm.size > 1:
            has = comm.allgather(template is not None)
            if not all(has):
                template = None
        self._cache_key = cache_key
        if template is not None:
            procmesh = template.procmesh
            plans = template.plans
        else:
            procmesh = _fft.ProcMesh(self.np, comm) if len(self.np) else _fft.ProcMesh([1], comm)
            plans = self._make_plans(procmesh, is_c2c, rdtype)
        self._rdtype = rdtype
        self._finish_init(plans, procmesh, resampler)
        _pm_cache[cache_key] = self

    def _make_plans(self, procmesh, is_c2c, rdtype):
        plans = OrderedDict()
        plans['partitionT'] = _fft.Partition(self.Nmesh, procmesh, transposed=True, is_c2c=is_c2c,
                                             itemsize=rdtype.itemsize)
        plans['partitionU'] = _fft.Partition(self.Nmesh, procmesh, transposed=False, is_c2c=is_c2c,
                                             itemsize=rdtype.itemsize)
        for T in 'TU':
            part = plans['partition' + T]
            plans['forward' + T] = _fft.Plan(part, True, rdtype, inplace=False)
            plans['backward' + T] = _fft.Plan(part, False, rdtype, inplace=False)
            plans['ipforward' + T] = _fft.Plan(part, True, rdtype, inplace=True)
            plans['ipbackward' + T] = _fft.Plan(part, False, rdtype, inplace=True)
        for k in ('forward', 'backward'):
            # out of place in both cases: the transposed plan works into / out of a scratch buffer
            plans[k + 'U'].sibling = plans[k + 'T']
            plans['ip' + k + 'U'].sibling = plans[k + 'T']
        return plans

    def _finish_init(self, plans, procmesh, resampler):
        # use the transposed partition for configuration space edges (pm.py:1443-1461);
        # here rank r owns block r in C order, so DomainAssign is the identity ramp
        partition = plans['partitionT']
        edges = partition.i_edges
        shape = numpy.array([len(g) - 1 for g in edges], dtype='int32')
        size = int(numpy.prod(shape))
        DomainAssign = numpy.empty(size, dtype='int32')
        for irank in range(self.comm.size):
            start = irank * size // self.comm.size
            end = (irank + 1) * size // self.comm.size
            DomainAssign[start:end] = irank
        self.domain = domain.GridND(edges, comm=self.comm, DomainAssign=DomainAssign)
        self.procmesh = procmesh

        # Transform from simulation unit to local grid unit.
        self.affine = Affine(partition.ndim, translate=-partition.local_i_start,
                             scale=1.0 * self.Nmesh / self.BoxSize, period=self.Nmesh)
        # Transform from global grid unit to local grid unit.
        self.affine_grid = Affine(partition.ndim, translate=-partition.local_i_start,
                                  scale=1.0, period=self.Nmesh)
        self.resampler = FindResampler(resampler)
        self.plans = plans
        self._coords = {}
        self._field_meta = {}

    def _get_partition(self, field_type):
        if issubclass(field_type, RealField):
            return self.plans['partitionT']
        elif issubclass(field_type, UntransposedComplexField):
            return self.plans['partitionU']
        elif issubclass(field_type, TransposedComplexField):
            return self.plans['partitionT']
        raise TypeError("not support type, internall Error")

    def create_coords(self, field_type, return_indices=False):
        """ coordinate arrays (device tensors broadcastable to the field; floats in the
            dtype of the ParticleMesh, indices int64) — pm.py:1505-1531. """
        field_type = _typestr_to_type(field_type)
        if field_type not in self._coords:
            partition = self._get_partition(field_type)
            dev = backend.get().device
            if issubclass(field_type, RealField):
                self._coords[field_type] = _init_i_coords(partition, self.Nmesh, self.BoxSize, self._rdtype, dev)
            else:
                self._coords[field_type] = _init_o_coords(partition, self.Nmesh, self.BoxSize, self._rdtype, dev)
        x, i = self._coords[field_type]
        if return_indices:
            return [ii.clone() for ii in i]
        return [xx.clone() for xx in x]

    @property
    def partition(self):
        return self.plans['partitionT']

    def reshape(self, Nmesh=None, BoxSize=None):
        """ a ParticleMesh of a different resolution, or even dimension (pm.py:1541-1573) """
        def per_axis(value, default, ndim):
            # None: what this mesh has; a scalar: the same on every axis
            if value is None:
                return default
            return [value] * ndim if numpy.isscalar(value) else value
        Nmesh = per_axis(Nmesh, self.Nmesh, self.ndim)
        BoxSize = per_axis(BoxSize, self.BoxSize[:len(Nmesh)], len(Nmesh))
        if len(BoxSize) != len(Nmesh):
            raise ValueError("Dimension of BoxSize (%d) doesn't agree with Nmesh (%d); provide BoxSize explicitly." % (len(BoxSize), len(Nmesh)))
        if len(self.np) > len(Nmesh):
            # the reference hands its process mesh on (pm.py:1568-1573) and PFFT refuses one of more dimensions than
            # the mesh: pm.reshape(Nmesh=[8]) of a mesh made with np=[1, 1] raises (pmesh/tests/test_pm.py:376-379)
            raise ValueError("a process mesh of %d dimensions cannot decompose a mesh of %d" % (len(self.np), len(Nmesh)))
        return ParticleMesh(BoxSize=BoxSize, Nmesh=Nmesh, dtype=self.dtype, comm=self.comm,
                            resampler=self.resampler, np=self.np if len(Nmesh) == self.ndim else None)

    def resize(self, Nmesh):
        # the older spelling (pm.py:1533-1539)
        warnings.warn("ParticleMesh.resize method is deprecated. Use reshape method with full Nmesh as a tuple.", DeprecationWarning, stacklevel=2)
        return self.reshape(Nmesh=Nmesh)

    def respawn(self, comm, np=None):
        """ the same geometry on a new communicator (pm.py:1575-1600) """
        return ParticleMesh(BoxSize=self.BoxSize, Nmesh=self.Nmesh, dtype=self.dtype, comm=comm,
                            resampler=self.resampler, np=np)

    def create(self, type=None, base=None, value=None, mode=None):
        """
            Create a field object (pm.py:1602-1634).

            type: 'real', 'complex', 'untransposedcomplex', or the classes
            base : reuse the physical memory of an existing field (`obj._base`)
            value : initialize the field with the values.
        """
        if mode is not None:
            # the old name of `type`; giving both is a mistake
            if type is not None:
                raise ValueError("both mode and type are specified, possiblity arguments are arranged in wrong order")
            warnings.warn("argument mode is deprecated. use type=%s instead" % mode, DeprecationWarning, stacklevel=2)
            type = mode
        field = _typestr_to_type(type)(self, base=base)
        if value is not None:
            field[...] = value
        return field

    def mesh_coordinates(self, dtype=None):
        """ integer coordinates of the local mesh points, (N, ndim) on the device (pm.py:1698-1703) """
        partition = self.plans['partitionT']
        dev = backend.get().device
        tdt = torch_dtype(dtype) if dtype is not None else torch.float64
        axes = [torch.arange(int(n), device=dev, dtype=tdt) + int(s)
                for n, s in zip(partition.local_i_shape, partition.local_i_start)]
        grid = torch.meshgrid(*axes, indexing='ij')
        return torch.stack([g.reshape(-1) for g in grid], dim=-1)

    def unravel(self, type, flatiter):
        """ Unravel c-ordered field values into a new field of `type` (pm.py:1636-1654). """
        r = self.create(type=type)
        r.unravel(flatiter)
        return r

    def generate_whitenoise(self, seed, unitary=False, mean=0, type=None, mode=None, base=None):
        """ Generate white noise to the field with the given seed (pm.py:1656-1696).

            The scheme is compatible with Gadget / N-GenIC when the field is three-dimensional
            (csrc/pmx_whitenoise.hip): the same seed gives the same modes whatever the domain
            decomposition, and the same large scales whatever the mesh size.

            seed : int; mean : the mean of the field (the k = 0 mode); unitary : True for a
            unitary white noise where the amplitude is fixed to 1 and only the phase is random;
            type : 'complex' (default), 'real', 'transposedcomplex', 'untransposedcomplex'.
        """
        from .whitenoise import generate
        if mode is not None:
            warnings.warn("mode argument is deprecated, use type", DeprecationWarning, stacklevel=2)
            type = mode
        if type is None:
            type = TransposedComplexField
        type = _typestr_to_type(type)
        if type is RealField:
            # the reference goes through the untransposed layout (pm.py:1679-1680); the modes do
            # not depend on the layout, and pencils only have the transposed one
            complex_type = UntransposedComplexField if len(self.np) <= 1 else TransposedComplexField
        else:
            complex_type = type
        complex = self.create(type=complex_type, base=base)
        generate(complex.value, complex.start, complex.Nmesh, seed, bool(unitary))
        # the mean: the k = 0 mode, held by the rank whose block starts at the origin
        if all(int(s) == 0 for s in complex.start) and complex.value.numel():
            complex.value[(0,) * self.ndim] = mean
        return complex.cast(type=type, out=None if type is RealField else complex)

    def generate_uniform_particle_grid(self, shift=None, dtype=None, return_id=False):
        """
            uniform grid of particles, one per grid point, in BoxSize coordinate
            (pm.py:1705-1752).  Returned as a device tensor; float64 unless dtype is given
            (quirk Q5: the reference's `dtype == self.dtype` is a no-op comparison).
        """
        if shift is None:
            warnings.warn("calling generate_uniform_particle_grid without a shift argument is deprecated."
                          "use shift=0.5 for the previous default behavior. ", DeprecationWarning, 2)
            shift = 0.5
        shift = numpy.broadcast_to(shift, self.ndim)
        source = self.mesh_coordinates(dtype)
        dev = source.device
        source += torch.as_tensor(numpy.ascontiguousarray(shift), dtype=source.dtype, device=dev)
        source *= torch.as_tensor(self.BoxSize / self.Nmesh, dtype=source.dtype, device=dev)
        if not return_id:
            return source
        isource = self.mesh_coordinates('i8')
        id = isource[:, 0].clone()
        for i in range(1, self.ndim):
            id *= int(self.Nmesh[i])
            id += isource[:, i]
        return source, id

    def stage(self, array):
        """Register a host (numpy) array for repeated use: returns a handle to pass wherever the array
        would go (`paint`, `readout`, `decompose`, `Layout.exchange`).  The array is uploaded once; the
        calls that follow find its device copy — and the bin plan and layout memos keyed on it — instead
        of moving it over PCIe again.  `force()` of examples/nbody.py:199-218 hands the same positions to
        one paint and three readouts: with `X = pm.stage(X)` they cross the link once.  Results still
        come back as numpy arrays.  After changing the host array in place call `handle.refresh()`."""
        from ._arrays import Staged
        if isinstance(array, Staged) or is_tensor(array):
            return array
        return Staged(array, backend.get().device)

    def readout(self, fields, pos, out=None, resampler=None, transform=None, gradient=None, layout=None):
        """ Read several real fields of this mesh at the same positions (an extension; the reference has no
            counterpart: its callers read field by field into the columns of their array, examples/nbody.py:214-216).

            fields : sequence of RealField (e.g. the three components of the force); pos : (n, ndim);
            out : (n, len(fields)) device tensor or None (a new float64 one).  Returns out[i, f] = fields[f] at pos[i] —
            on one rank from one launch that writes every row of `out` once (ResampleWindow.readout_many); with a
            `layout` field by field through RealField.readout (the partial sums of the ghosts travel per field). """
        fields = list(fields)
        for f in fields:
            if not isinstance(f, RealField) or f.pm is not self:
                raise TypeError('fields must be RealField objects of this ParticleMesh')
        transform = transform or self.affine
        resampler = FindResampler(self.resampler if resampler is None else resampler)
        if layout is None:
            return resampler.readout_many([f.value for f in fields], pos, out=out, diffdir=gradient, transform=transform)
        be = backend.get()
        if out is None:
            out = torch.empty((len(pos), len(fields)), dtype=torch.float64, device=be.device)
        for k, f in enumerate(fields):
            f.readout(pos, out=out[:, k], resampler=resampler, transform=transform, gradient=gradient, layout=layout)
        return out

    def tile_order(self, pos, transform=None):
        """ A permutation of the rows of `pos` that makes them spatially coherent (an extension;
            the reference has no counterpart).

            The tiled paint / readout kernels keep the caller's rows where they are and lean on
            neighbouring rows being neighbouring particles — what a simulation that stores its
            particles in ID (lattice) order has at the start, and loses by degrees as the flow mixes
            them (scripts/nbody_long.py: the readout of a 512^3 run goes from 1.1 to 3.3 ms).
            Reordering the particle arrays every few steps,

                o = pm.tile_order(pos);  pos = pos[o];  vel = vel[o];  ...

            restores it.  The order is tile by tile (8 x 16 x 32 cells, C order of the tiles of this
            rank's block); INSIDE a tile the rows are not sorted by cell (on the device they stand in the
            order of the bin plan's list, which changes from build to build) — sorting them by cell as
            well would put the particles of a crowded cell into neighbouring lanes of the paint
            kernel, the worst case of its LDS atomics (measured on an evolved 512^3 state: paint 4.2 ms
            cell-sorted against 2.2 as the run left the rows and 1.4 in random order; the readout
            wants the tile order alone).  [r6] The permutation is read off the bin plan of `pos`
            (pmx_binplan_order: a scan and a copy, ~0.5 ms for 134 M rows — and the plan is the one
            the next paint of these positions would have built anyway); rows that touch no cell of
            this rank's block come last.  Returns an int64 device tensor. """
        be = backend.get()
        dpos, _ = to_device(pos, be.device, 'pos')
        if transform is None:
            transform = self.affine
        nd = self.ndim
        n = dpos.shape[0]
        resampler = FindResampler(self.resampler)
        if be.name == 'hip' and nd == 3 and n and hasattr(be.lib, 'pmx_binplan_order'):
            from .window import _binned_ok, bin_cache
            part = self._get_partition(RealField)
            es = numpy.dtype(self._rdtype).itemsize
            block = _BlockGeometry([int(x) for x in part.local_i_shape], [int(x) for x in part.i_strides], es)
            painter = resampler._painter(block, (0, 0, 0), transform)
            if dpos.dim() == 2 and _binned_ok(be, painter, dpos, n, None):
                pv = vec(dpos)
                plan = bin_cache().lookup(be, dpos, painter, pv, n)
                order = torch.empty(n, dtype=torch.int64, device=be.device)
                be.call('binplan_order', plan, order.data_ptr(), be.stream())
                return order
        # (meshes of other dimensions, batches the tile kernels do not take: the same order from a stable sort by tile)
        scale = torch.as_tensor(numpy.broadcast_to(numpy.asarray(transform.scale, dtype='f8'), (nd,)).copy(),
                                device=be.device)
        cell = torch.floor(dpos[:, :nd].to(torch.float64) * scale).to(torch.int64)
        tile = (8, 16, 32)[-nd:] if nd <= 3 else (8,) * nd
        key = torch.zeros(dpos.shape[0], dtype=torch.int64, device=be.device)
        for d in range(nd):
            m = int(self.Nmesh[d])
            key = key * (-(-m // tile[d])) + torch.div(torch.remainder(cell[:, d], m), tile[d], rounding_mode='floor')
        return torch.argsort(key, stable=True)

    def decompose(self, pos, smoothing=None, transform=None):
        """
        Create a domain decompose layout for particles at given coordinates (pm.py:1754-1793).

        smoothing : None, float, array_like, string, or ResampleWindow
            if given as a string or ResampleWindow, use 0.5 * support: the size of the buffer
            region around a domain.  Default: None, use self.resampler
        """
        # a window (object or registered name) stands for half its support; numbers pass through
        window = self.resampler if smoothing is None else smoothing
        try:
            smoothing = 0.5 * FindResampler(window).support
        except TypeError:
            smoothing = window
        transform = self.affine if transform is None else transform
        # Transform from simulation unit to global grid unit: transform0(x) = scale * x; the
        # shift is local per processor, thus not used.  The scaling runs inside the kernel.
        layout = self.domain.decompose(pos, smoothing=smoothing, _scale=transform.scale)
        # what the routing guarantees (see _ghosts_only): every particle was sent to every rank
        # that holds a cell within `smoothing` cells of it
        flat = lambda a: tuple(float(x) for x in numpy.asarray(a).ravel())
        layout._route = (numpy.broadcast_to(numpy.asarray(smoothing, dtype='f8'), (self.ndim,)).copy(),
                         flat(transform.scale), flat(self.affine.translate), flat(self.affine.period))
        return layout

    def paint(self, pos, hsml=None, mass=1.0, resampler=None, transform=None, hold=False,
              gradient=None, layout=None, out=None):
        """
        Paint particles into a real field (pm.py:1795-1869).

        pos : (, ndim) positions in simulation unit; hsml : window scaling per particle or None;
        mass : scalar or (,) array; hold : if true, do not clear the current value in the field;
        gradient : None or the direction of the window derivative; resampler : window, default
        pm.resampler; layout : domain decomposition, particles are routed first; out : RealField.

        The painter operation conserves the total mass. It is not the density.
        """
        transform = transform or self.affine
        resampler = FindResampler(self.resampler if resampler is None else resampler)
        if layout is not None and layout.comm.size == 1 and _ghosts_only(layout, resampler, transform, hsml):
            # one rank, nothing to receive: `pm.paint(x, layout=pm.decompose(x))` — how callers of the reference write
            # every paint (examples/nbody.py:203-204) — is the paint of the caller's own array.  The reference's
            # exchange would have refused an array of another length than the layout was built for (domain.py:177-179)
            if len(pos) != layout.sendlength:
                raise ValueError('the length of data does not match that used to build the layout')
            layout = None
        fresh = out is None
        part = self._get_partition(RealField)
        ghosts = layout is not None and _ghosts_only(layout, resampler, transform, hsml)
        if fresh and (layout is None or ghosts) and not hold and not getattr(part, 'is_c2c', False) and backend.get().name == 'hip':
            # a field of this call's own making that the paint overwrites cell by cell: no zero fill of the buffer
            # (complex-to-complex meshes: the paint writes the real parts only, the imaginary ones must read 0)
            out = RealField(self, base=torch.empty(part.alloc_reals, dtype=torch_dtype(self._rdtype),
                                                   device=backend.get().device))
        elif fresh:
            out = self.create(type=RealField)
        if layout is None:
            # hold=False: "out.value[...] = 0" (pm.py:1852-1853) is folded into the kernel.
            # HALO_DEFER: the tile kernels' halo merge is left to the forward transform that usually follows
            # (window._HaloDebt) — only on a field nobody else holds a view of yet ('fresh'), as a caller's own
            # field must be complete when this call returns (in the reference `value` is a plain array).
            defer = None
            if not hold and (HALO_DEFER == 'always' or (HALO_DEFER == 'fresh' and fresh)):
                defer = out._base.storage
            resampler.paint(out.value, pos, hsml=hsml, mass=mass, transform=transform, diffdir=gradient,
                            _overwrite=not hold, _defer_to=defer)
            return out
        if ghosts:
            # the caller's own particles are painted where they lie (those whose window misses
            # the local block fall under the drop-outside rule, _window_generics.h:144-167);
            # only the ghosts received from other ranks are exchanged
            be = backend.get()
            dpos, _ = to_device(pos, be.device, 'pos')
            dmass = mass
            if not _is_scalar(mass):
                dmass, _ = to_device(mass, be.device, 'mass')
            remote = layout.remote_recvlength or layout.comm.size > 1
            handle = None
            if remote:
                # the rows bound for other ranks leave first (one all-to-all-v for positions and masses, on
                # RCCL's stream) and travel while the caller's own particles are painted
                if _is_scalar(mass):
                    handle = layout.exchange_remote(dpos, async_op=True)
                else:
                    handle = layout.exchange_remote(dpos, dmass, async_op=True)
            # HALO_DEFER as on one rank: the merge of the tile kernels' halos is left to the row pass of the forward
            # transform (fft.Plan._slab_row_forward).  What the ghosts add afterwards are atomic adds to the same
            # cells: the order does not matter, so they go into the field as it is (`_value`: no settling)
            defer = None
            if not hold and (HALO_DEFER == 'always' or (HALO_DEFER == 'fresh' and fresh)):
                defer = out._base.storage
            resampler.paint(out.value, dpos, mass=dmass, transform=transform, diffdir=gradient,
                            _overwrite=not hold, _defer_to=defer)
            if remote:
                if _is_scalar(mass):
                    rpos, rmass = handle.wait(), dmass
                else:
                    rpos, rmass = handle.wait()
                if len(rpos):
                    owed = getattr(out._base.storage, '_pmx_halo', None) is not None
                    # (a halo merge left to r2c's row pass stays owed: the ghosts go into the field as it is, through
                    # the direct kernels — a bin plan for a large ghost batch would settle the debt in its lookup and
                    # the deferral would be lost exactly where it saves most)
                    resampler.paint(out._value if owed else out.value, rpos, mass=rmass, transform=transform,
                                    diffdir=gradient, _direct=owed)
            return out
        localpos = layout.exchange(pos)
        localmass = exchange(layout, mass)
        localhsml = exchange(layout, hsml)
        return self.paint(localpos, mass=localmass, hsml=localhsml, resampler=resampler,
                          transform=transform, hold=hold, gradient=gradient, layout=None, out=out)

    def paint_jvp(self, pos, mass=1.0, v_pos=None, v_mass=None, resampler=None, transform=None,
                  gradient=None, layout=None, out=None):
        """ A_q = W_qi M_i (pm.py:1872-1888) """
        assert gradient is None  # second order is not supported yet
        out = self.create(type=RealField) if out is None else out
        out[...] = 0
        # one held paint per tangent: the position tangents through the window's derivative, the mass tangent plainly
        terms = [] if v_pos is None else [(_mul(v_pos[..., d], mass), d) for d in range(pos.shape[1])]
        if v_mass is not None:
            terms.append((v_mass, None))
        for weight, direction in terms:
            self.paint(pos, mass=weight, resampler=resampler, transform=transform, gradient=direction,
                       hold=True, layout=layout, out=out)
        return out

    def paint_vjp(self, v, pos, mass=1.0, resampler=None, transform=None, gradient=None,
                  out_pos=None, out_mass=None, layout=None):
        """ back-propagate the gradient of paint from v (pm.py:1890-1935). """
        if out_pos is not False:
            out_pos, pos = _position_gradient_target(out_pos, pos, gradient)
            for d in range(pos.shape[1]):
                r = v.readout(pos, resampler=resampler, transform=transform, gradient=d, layout=layout)
                out_pos[..., d] = _mul(r, mass) if not numpy.isscalar(mass) else r * mass
        if out_mass is not False:
            r = v.readout(pos, resampler=resampler, transform=transform, gradient=gradient, layout=layout)
            if out_mass is None:
                out_mass = r
            elif is_inplace(out_mass):
                mass[...] = r
                out_mass = mass
            else:
                out_mass[...] = r
        return out_pos, out_mass


def _pm_upsample(self, source, resampler=None, keep_mean=False):
    """ Resample an image with the upsample method: read out the value of the image at the
        pixel positions of this pm (pm.py:1937-1986).  keep_mean conserves the mean rather than
        the total mass in the overlapped region.  Returns a new RealField. """
    assert isinstance(source, RealField)
    q = self.mesh_coordinates(dtype=self._rdtype)
    # transform from my mesh to source's mesh
    transform = Affine(self.ndim, translate=-source.start, scale=1.0 * source.Nmesh / self.Nmesh,
                       period=source.Nmesh)
    # quirk Q5: the reference computes the layout twice; the second, with a hard-coded
    # smoothing of 1.6, is the one that is used (pm.py:1971-1972)
    layout = source.pm.decompose(q, smoothing=1.6, transform=transform)
    f = source.readout(q, resampler=resampler, layout=layout, transform=transform)
    if not keep_mean:
        f = f * float((source.pm.Nmesh.prod() / source.pm.BoxSize.prod()) /
                      (self.Nmesh.prod() / self.BoxSize.prod()))
    # all are on the grid. NGB is faster, and no need to decompose
    return self.paint(q, mass=f, resampler='nnb', transform=self.affine_grid)


def _pm_downsample(self, source, resampler=None, keep_mean=False):
    """ Resample an image with the downsample method: paint the value of the image at the
        pixel positions of the source (pm.py:1988-2027).  Returns a new RealField. """
    assert isinstance(source, RealField)
    q = source.pm.mesh_coordinates(dtype=self._rdtype)
    f = source.readout(q, resampler='nnb', transform=source.pm.affine_grid)
    # transform from source's mesh to my mesh
    transform = self.affine_grid.rescale(1.0 * self.Nmesh / source.Nmesh)
    if keep_mean:
        f = f / float((source.pm.Nmesh.prod() / source.pm.BoxSize.prod()) /
                      (self.Nmesh.prod() / self.BoxSize.prod()))
    layout = self.decompose(q, smoothing=resampler, transform=transform)
    return self.paint(q, mass=f, layout=layout, resampler=resampler, transform=transform)


ParticleMesh.upsample = _pm_upsample
ParticleMesh.downsample = _pm_downsample


def _smoke_cycle(O):
    """One small PM cycle on the GPU checked against the oracle (__graft_entry__.smoke)."""
    N, L = 32, 1000.0
    pm = ParticleMesh([N, N, N], BoxSize=L, dtype='f8', resampler='cic')
    pos_h = O.synth_uniform(N, L)
    pos = torch.from_numpy(pos_h).to(backend.get().device)
    rho = pm.paint(pos)
    rhok = rho.r2c(out=Ellipsis)
    T = Transfer(laplace_pow=-1, grad_dir=0)
    f = rhok.apply(T, out=Ellipsis).c2r(out=Ellipsis).readout(pos)
    t = O.make_transfer(laplace_pow=-1, grad_dir=0, grad_kind=0)
    real, ck, back, out = O.pm_cycle(N, L, pos_h, kind='tunedcic', transfer=t)
    err = abs(f.cpu().numpy() - out).max() / max(abs(out).max(), 1e-300)
    assert err < 1e-11, err
    # the production form of the cycle at the smallest mesh the LDS FFT kernels take: tile-binned
    # paint/readout, row + column FFT kernels on the padded layout, transfer fused into c2r
    from . import window as _window
    Nmesh, L = [64, 64, 128], 500.0
    pm = ParticleMesh(Nmesh, BoxSize=L, dtype='f8', resampler='tsc')
    pos_h = numpy.random.RandomState(7).uniform(0, L, size=(200000, 3))
    pos = torch.from_numpy(pos_h).to(backend.get().device)
    old = _window.BINNED
    _window.BINNED = 'always'
    try:
        f = pm.paint(pos).r2c(out=Ellipsis).c2r(out=Ellipsis, transfer=Transfer.dx1(1)).readout(pos)
        assert any(e[3] for e in _window.bin_cache().entries), 'the tile-binned kernels did not run'
    finally:
        _window.BINNED = old
    t = O.make_transfer(laplace_pow=-1, grad_dir=1, grad_kind=0)
    aff = O.Affine(3, scale=[n / L for n in Nmesh], period=Nmesh)
    real = numpy.zeros(Nmesh)
    O.Window('tunedtsc').paint(real, pos_h, transform=aff)
    ck = O.apply_transfer(t, O.r2c(real), (0, 0, 0), Nmesh, (L, L, L))
    want = O.Window('tunedtsc').readout(O.c2r(ck, Nmesh), pos_h, transform=aff)
    err = abs(f.cpu().numpy() - want).max() / max(abs(want).max(), 1e-300)
    assert err < 1e-11, err
