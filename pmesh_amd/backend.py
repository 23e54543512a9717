"""Kernel backend: the one place where the host layer meets native code.

The product backend is :class:`HipBackend`: it binds ``libpmesh_amd.so`` (the
C ABI of include/pmesh_amd.h, hand-written HIP kernels for gfx950 + rocFFT)
through the Cython shim ``pmesh_amd._pmx`` and runs on a real GPU.  There is NO CPU implementation in this package: if the
library or the GPU is missing, :func:`get` raises — it never falls back.

``use(backend)`` exists so that tests can drive the host logic (argument
handling, layouts, the distributed FFT schedule, torch.distributed collectives
over gloo) against the CPU oracle on machines without a GPU; the object they
install lives in tests/, not here.
"""
import ctypes as C
import os

import torch

from . import _abi, _arrays

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBNAME = 'libpmesh_amd.so'


class PmxError(RuntimeError):
    def __init__(self, what, code, msg=''):
        self.code = code
        RuntimeError.__init__(self, '%s failed: %s%s' % (
            what, _abi.STATUS_NAMES.get(code, code), (' — ' + msg) if msg else ''))


def library_path():
    # PMESH_AMD_LIBRARY: another build of the same ABI (A/B timing of compile-time switches)
    return os.environ.get('PMESH_AMD_LIBRARY') or os.path.join(_HERE, LIBNAME)


def load_library(path=None, binding=None):
    """Load the C ABI and bind every entry point of include/pmesh_amd.h; raises if the library is missing or lacks a
    symbol the header declares.  The binding is the Cython shim `pmesh_amd._pmx` (generated from the header by
    csrc/gen_pyx.py, built by the same `make`): the returned object has one callable `pmx_<name>` per entry point.
    PMESH_AMD_BINDING=ctypes binds the same library through the ctypes table of _abi.py instead (the binding the
    tests' CPU double uses; ~10 us slower per call) — a debugging aid, never a fallback: a missing shim raises."""
    path = path or library_path()
    if not os.path.exists(path):
        raise ImportError(
            '%s not found: build it with `make -C pmesh_amd/csrc` (hipcc, gfx950). '
            'There is no CPU fallback.' % path)
    binding = binding or os.environ.get('PMESH_AMD_BINDING', 'cython')
    if binding == 'ctypes':
        lib = C.CDLL(path)
        missing = _abi.declare(lib, 'pmx_', _abi.PROTOTYPES)
        missing += _abi.declare(lib, 'pmx_', _abi.DEVICE_ONLY)
    else:
        try:
            from . import _pmx as lib
        except ImportError as e:
            raise ImportError('the Cython shim pmesh_amd/_pmx is not built (`make -C pmesh_amd/csrc`): %s' % e)
        missing = lib.bind(path)
    if missing:
        raise ImportError('%s lacks symbols declared in include/pmesh_amd.h: %s' % (path, missing))
    return lib


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
if _raw_stream is None:
    def _raw_stream(index):
        return torch.cuda.current_stream(index).cuda_stream


def _byte_strides(t):
    """the strides of tensor t in bytes, padded to three axes"""
    es = t.element_size()
    return _abi.i64arr([s * es for s in t.stride()], 3)


def _mesh_args(start, nmesh, boxsize):
    """start, Nmesh and BoxSize of a block as the three consecutive array arguments of the C ABI"""
    return _abi.i64arr(start, 3), _abi.i64arr(nmesh, 3), _abi.f64arr(boxsize, 3)


class HipBackend(object):
    """libpmesh_amd.so on cuda:<index> (ROCm)."""
    name = 'hip'
    prefix = 'pmx_'

    def __init__(self, device_index=None):
        self.lib = load_library()
        if self.lib.pmx_device_count() < 1 or not torch.cuda.is_available():
            raise RuntimeError('pmesh_amd needs an AMD GPU (gfx950): no HIP device is visible. '
                               'There is no CPU fallback.')
        if device_index is None:
            device_index = torch.cuda.current_device()
        self.device = torch.device('cuda', device_index)

    # -- plumbing ---------------------------------------------------------
    def stream(self):
        # (the raw handle of torch's current stream: torch.cuda.current_stream() builds a Stream object per call,
        # 6 us of the host's ~15 us per kernel launch)
        return C.c_void_p(_raw_stream(self.device.index))

    def call(self, name, *args):
        rc = getattr(self.lib, 'pmx_' + name)(*args)
        if rc != 0:
            raise PmxError('pmx_' + name, rc, self.lib.pmx_last_error().decode())

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    # -- FFT plans --------------------------------------------------------
    def fft_create(self, kind, elsize, n, istride, idist, ostride, odist, batch, scale, inplace):
        plan = C.c_void_p()
        nd = len(n)
        self.call('fft_create', C.byref(plan), kind, elsize, nd, _abi.i64arr(n), _abi.i64arr(istride),
                  idist, _abi.i64arr(ostride), odist, batch, float(scale), int(bool(inplace)))
        return plan

    def fft_execute(self, plan, tin, tout):
        self.call('fft_execute', plan, tin.data_ptr(), tout.data_ptr(), self.stream())

    def fft_destroy(self, plan):
        self.call('fft_destroy', plan)

    # -- LDS-resident column FFT -----------------------------------------
    def colfft_supported(self, n, elsize):
        return self.lib.pmx_colfft_supported(int(n), int(elsize)) == 0

    def colfft(self, elsize, inverse, data, A, N, B, scale=1.0, transfer=None, n1=1, n2=1,
               start=(0, 0, 0), nmesh=(1, 1, 1), boxsize=(1.0, 1.0, 1.0), a_stride=0, n_stride=0):
        """in-place FFT along the middle axis of the (A, N, B) complex array in `data`
        (a_stride / n_stride: padded strides between successive a / lines n, 0 = dense)"""
        self.call('colfft', elsize, int(bool(inverse)), data.data_ptr(), A, N, B, float(scale),
                  C.byref(transfer) if transfer is not None else None, n1, n2,
                  *_mesh_args(start, nmesh, boxsize),
                  int(a_stride), int(n_stride), self.stream())

    def colfft_configure(self, persistent):
        """process-wide: persistent (prefetching) column passes where a tile fills a CU, or one workgroup per tile
        (for transforms that overlap with collectives) — pmx_colfft_configure"""
        self.call('colfft_configure', int(bool(persistent)))

    def colfft_roundtrip_supported(self, n, elsize):
        return self.lib.pmx_colfft_roundtrip_supported(int(n), int(elsize)) == 0

    def colfft_roundtrip(self, elsize, data, N, B, scale=1.0, transfer=None, n1=1, n2=1,
                         start=(0, 0, 0), nmesh=(1, 1, 1), boxsize=(1.0, 1.0, 1.0), n_stride=0):
        """forward column FFT x scale [x transfer] x inverse column FFT in one kernel, in place on (N, B)"""
        self.call('colfft_roundtrip', elsize, data.data_ptr(), N, B, float(scale),
                  C.byref(transfer) if transfer is not None else None, n1, n2,
                  *_mesh_args(start, nmesh, boxsize), int(n_stride), self.stream())

    def colfft_split(self, elsize, inverse, src, dst, A, N, B, nsplit, scale=1.0, plain_pitch=0):
        """column FFT fused with the slab pack (forward: plain -> split) / unpack (inverse);
        plain_pitch: elements per line of the plain side (0 = B)"""
        self.call('colfft_split', elsize, int(bool(inverse)), src.data_ptr(), dst.data_ptr(), A, N, B,
                  int(nsplit), float(scale), int(plain_pitch), self.stream())

    def colfft_resplit(self, elsize, inverse, src, dst, A, N, B, nsplit_in, nsplit_out, scale=1.0):
        """column FFT between two split layouts (the axis-1 pass of a pencil transform with the
        unpack before and the pack after it fused in); nsplit 0 = plain"""
        self.call('colfft_resplit', elsize, int(bool(inverse)), src.data_ptr(), dst.data_ptr(), A, N, B,
                  int(nsplit_in), int(nsplit_out), float(scale), self.stream())

    def colfft_chunk(self, elsize, inverse, chunk, full, N, n1, cw, pitch, coff, to_full, scale=1.0,
                     transfer=None, start=(0, 0, 0), nmesh=(1, 1, 1), boxsize=(1.0, 1.0, 1.0)):
        """axis-0 pass on the columns [coff, coff+cw) of the (N, n1, pitch) block `full`, through the
        dense (N, n1, cw) buffer `chunk` (pipelined slab transposes)"""
        self.call('colfft_chunk', elsize, int(bool(inverse)), chunk.data_ptr(), full.data_ptr(), N, n1, cw,
                  pitch, coff, int(bool(to_full)), float(scale),
                  C.byref(transfer) if transfer is not None else None,
                  *_mesh_args(start, nmesh, boxsize), self.stream())

    def rowfft_supported(self, n, elsize):
        return self.lib.pmx_rowfft_supported(int(n), int(elsize)) == 0

    def rowfft(self, elsize, inverse, data, nrows, n, pitch, scale=1.0, rows_per_plane=0, plane_pitch=0):
        """in-place r2c / c2r of `nrows` rows of n reals at a pitch of `pitch` complex elements
        (rows_per_plane > 0: planes of that many rows, `plane_pitch` complex elements apart)"""
        self.call('rowfft', elsize, int(bool(inverse)), data.data_ptr(), nrows, n, pitch, float(scale),
                  int(rows_per_plane), int(plane_pitch), self.stream())

    def rowfft_halo(self, elsize, data, nrows, n, pitch, rows_per_plane, plane_pitch, plan, canvas_ptr, x0, last,
                    scale=1.0, dst=None):
        """the forward rowfft on planes x0 ... of a canvas whose paint left its halo merge to this pass
        (pmx_paint_binned_defer): the staged halos are added to the rows as they are loaded; last: the plan is
        released; dst: where the rows are written (None: in place)"""
        self.call('rowfft_halo', elsize, data.data_ptr(), dst.data_ptr() if dst is not None else None, nrows, n, pitch,
                  float(scale), int(rows_per_plane), int(plane_pitch), plan, C.c_void_p(canvas_ptr), int(x0),
                  int(bool(last)), self.stream())

    def rowfft_to(self, elsize, inverse, src, dst, nrows, n, pitch, scale=1.0, rows_per_plane=0, plane_pitch=0):
        """rowfft from `src` into `dst` (same layout)"""
        self.call('rowfft_to', elsize, int(bool(inverse)), src.data_ptr(), dst.data_ptr(), nrows, n, pitch, float(scale),
                  int(rows_per_plane), int(plane_pitch), self.stream())

    def colfft_to(self, elsize, inverse, src, dst, A, N, B, scale=1.0, transfer=None, n1=1, n2=1,
                  start=(0, 0, 0), nmesh=(1, 1, 1), boxsize=(1.0, 1.0, 1.0), a_stride=0, n_stride=0):
        """colfft from `src` into `dst` (same layout)"""
        self.call('colfft_to', elsize, int(bool(inverse)), src.data_ptr(), dst.data_ptr(), A, N, B, float(scale),
                  C.byref(transfer) if transfer is not None else None, n1, n2,
                  *_mesh_args(start, nmesh, boxsize),
                  int(a_stride), int(n_stride), self.stream())

    # -- slab transposes --------------------------------------------------
    def rowfft_split_supported(self, n, elsize, nparts):
        return self.lib.pmx_rowfft_split_supported(int(n), int(elsize), int(nparts)) == 0

    def rowfft_split(self, elsize, inverse, src, dst, nrows, n, pitch, offsets, scale=1.0):
        """the row pass with the last-axis split of a pencil transform's first transpose on it (forward: rows ->
        blocks by mode range; inverse: blocks -> rows); out of place"""
        self.call('rowfft_split', elsize, int(bool(inverse)), src.data_ptr(), dst.data_ptr(), nrows, n, pitch, float(scale),
                  _abi.i64arr(offsets), len(offsets) - 1, self.stream())

    def slab_pack(self, src, dst, n0, n1, n2, n1_offsets, elbytes, inverse=False):
        """(n0, n1, n2) -> blocks by n1 range (inverse: blocks -> (n0, n1, n2))"""
        self.call('slab_unpack' if inverse else 'slab_pack', src.data_ptr(), dst.data_ptr(), n0, n1, n2,
                  _abi.i64arr(n1_offsets), len(n1_offsets) - 1, elbytes, self.stream())

    # -- binned power spectrum ---------------------------------------------
    def power_project(self, params, a, b, start, nmesh, boxsize, kedges, muedges, acc):
        """add the binned sums of the local complex block `a` (times conj(b); b None: the auto spectrum) into the
        float64 device vector `acc` (layout: include/pmesh_amd.h, pmx_power_project)"""
        if a.numel() == 0:
            return
        es = a.element_size()
        nd = a.dim()
        self.call('power_project', C.byref(params), nd, es // 2, a.data_ptr(), _byte_strides(a),
                  b.data_ptr() if b is not None else None,
                  _byte_strides(b) if b is not None else None,
                  _abi.i64arr(a.shape, 3), *_mesh_args(start, nmesh, boxsize),
                  kedges.data_ptr(), muedges.data_ptr() if muedges is not None else None, acc.data_ptr(),
                  self.stream())

    def power_vjp(self, params, a, b, grad_a, grad_b, start, nmesh, boxsize, kedges, muedges, coef):
        """grad_a (and grad_b; b, grad_b None: the auto spectrum) = the adjoint of power_project for the coefficient
        table `coef`, a float64 device vector (layout: include/pmesh_amd.h, pmx_power_vjp)"""
        if a.numel() == 0:
            return
        es = a.element_size()

        def strides(t):
            return _byte_strides(t) if t is not None else None

        def ptr(t):
            return t.data_ptr() if t is not None else None
        self.call('power_vjp', C.byref(params), a.dim(), es // 2, ptr(a), strides(a), ptr(b), strides(b), ptr(grad_a),
                  strides(grad_a), ptr(grad_b), strides(grad_b), _abi.i64arr(a.shape, 3),
                  *_mesh_args(start, nmesh, boxsize), kedges.data_ptr(),
                  muedges.data_ptr() if muedges is not None else None, coef.data_ptr(), self.stream())

    # -- binned bispectrum ---------------------------------------------------
    def bispec_shells(self, a, outs, start, nmesh, boxsize, kedges, deconv_pow=0, unit=False):
        """outs[s] = the modes of the local complex block `a` in shell s (divided by the window; with unit: 1 there,
        and `a` is not read), 0 elsewhere, for the len(outs) shells of the float64 device vector `kedges`; the outputs
        share one shape, dtype and set of strides and may be raw memory (pmx_bispec_shells)"""
        o = outs[0]
        if o.numel() == 0:
            return
        es = o.element_size()
        ptrs = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        self.call('bispec_shells', o.dim(), es // 2, len(outs), int(deconv_pow), int(bool(unit)),
                  None if unit else a.data_ptr(), None if unit else _byte_strides(a), ptrs,
                  _byte_strides(o), _abi.i64arr(o.shape, 3), *_mesh_args(start, nmesh, boxsize), kedges.data_ptr(),
                  self.stream())

    def bispec_reduce(self, fields, triangles, acc, work=None):
        """acc[t] += sum over the cells of fields[i] * fields[j] * fields[l] for (i, j, l) = triangles[t]: real blocks
        of one shape, dtype and set of strides, an int32 device array (ntri, 3), a float64 device vector; work: a
        float64 device vector for the per-workgroup partial sums (None: allocated here) (pmx_bispec_reduce)"""
        f = fields[0]
        ntri = int(triangles.shape[0])
        if f.numel() == 0 or ntri == 0:
            return
        es = f.element_size()
        if work is None:
            work = torch.empty(self.bispec_work(ntri, f.numel()), dtype=torch.float64, device=self.device)
        ptrs = (C.c_void_p * len(fields))(*[t.data_ptr() for t in fields])
        self.call('bispec_reduce', f.dim(), es, len(fields), ptrs, _byte_strides(f),
                  _abi.i64arr(f.shape, 3), ntri, triangles.data_ptr(), acc.data_ptr(), work.data_ptr(), work.numel(),
                  self.stream())

    @staticmethod
    def bispec_work(ntri, ncells):
        """doubles of work for bispec_reduce: a row per workgroup, up to 512 rows and 64 MB, no more rows than
        chunks of 128 cells"""
        rows = max(1, min(512, (1 << 23) // max(ntri, 1), (ncells + 127) // 128))
        return rows * ntri

    def bispec_pairsum(self, fields, outs, offsets, pairs, weights):
        """outs[s] = sum over the entries e of offsets[s] .. offsets[s + 1] of weights[e] * fields[pairs[e][0]] *
        fields[pairs[e][1]]: real blocks of one shape, dtype and set of strides (outs[s] may be fields[s]), an int32
        device vector of len(fields) + 1 offsets, an int32 device array (npairs, 2), a float64 device vector
        (pmx_bispec_pairsum)"""
        f = fields[0]
        if f.numel() == 0:
            return
        nb = len(fields)
        if len(outs) != nb or any(o.shape != f.shape or o.stride() != f.stride() or o.dtype != f.dtype
                                  for o in list(fields) + list(outs)):
            raise ValueError('bispec_pairsum: the fields and the outputs share one shape, dtype and set of strides')
        npairs = int(pairs.shape[0])
        if offsets.numel() != nb + 1 or weights.numel() != npairs or offsets.dtype != torch.int32 or \
                pairs.dtype != torch.int32 or weights.dtype != torch.float64 or not pairs.is_contiguous():
            raise ValueError('bispec_pairsum: int32 offsets (nb + 1), int32 pairs (npairs, 2), float64 weights (npairs)')
        fp = (C.c_void_p * nb)(*[t.data_ptr() for t in fields])
        op = (C.c_void_p * nb)(*[t.data_ptr() for t in outs])
        self.call('bispec_pairsum', f.dim(), f.element_size(), nb, fp, op, _byte_strides(f), _abi.i64arr(f.shape, 3),
                  npairs, offsets.data_ptr(), pairs.data_ptr() if npairs else None,
                  weights.data_ptr() if npairs else None, self.stream())

    def bispec_shells_vjp(self, ins, out, start, nmesh, boxsize, kedges, deconv_pow=0):
        """out = the modes of ins[s] in shell s, divided by the window, 0 in no shell: the adjoint of bispec_shells
        over local complex blocks; the inputs share one shape, dtype and set of strides, `out` may be raw memory
        (pmx_bispec_shells_vjp)"""
        if out.numel() == 0:
            return
        es = out.element_size()
        ptrs = (C.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
        self.call('bispec_shells_vjp', out.dim(), es // 2, len(ins), int(deconv_pow), ptrs, _byte_strides(ins[0]),
                  out.data_ptr(), _byte_strides(out), _abi.i64arr(out.shape, 3), *_mesh_args(start, nmesh, boxsize),
                  kedges.data_ptr(), self.stream())

    # -- initial conditions: tabulated transfer, 2LPT ----------------------
    def apply_ktable(self, table, v, out, start, nmesh, boxsize):
        """out = T(|k|) v over the local complex block v (pmx_apply_ktable; `table` a _abi.KTable whose x / y are
        float64 device arrays kept alive by the caller); out may be v"""
        es = v.element_size()
        self.call('apply_ktable', C.byref(table), v.dim(), es // 2, v.data_ptr(), _byte_strides(v),
                  out.data_ptr(), _byte_strides(out), _abi.i64arr(v.shape, 3),
                  *_mesh_args(start, nmesh, boxsize), self.stream())

    def ktable_vjp(self, table, hermitian, field, v, start, nmesh, boxsize, grad):
        """grad[i] += sum_m w_m Re(conj(v_m) field_m) e_i(|k_m|) over the local complex blocks (pmx_ktable_vjp; grad:
        float64 device vector of table.n entries)"""
        es = field.element_size()
        self.call('ktable_vjp', C.byref(table), int(bool(hermitian)), field.dim(), es // 2, field.data_ptr(),
                  _byte_strides(field), v.data_ptr(), _byte_strides(v), _abi.i64arr(field.shape, 3),
                  *_mesh_args(start, nmesh, boxsize), grad.data_ptr(), self.stream())

    def apply_ktable_jvp(self, table, dy, v, out, start, nmesh, boxsize):
        """out = T'(|k|) v, the tangent of apply_ktable along the table values (pmx_apply_ktable_jvp; dy: float64
        device vector of table.n entries); out may be v"""
        es = v.element_size()
        self.call('apply_ktable_jvp', C.byref(table), dy.data_ptr(), v.dim(), es // 2, v.data_ptr(),
                  _byte_strides(v), out.data_ptr(), _byte_strides(out), _abi.i64arr(v.shape, 3),
                  *_mesh_args(start, nmesh, boxsize), self.stream())

    # -- survey multipoles: the harmonic passes ------------------------------
    def ylm_weight(self, ell, m, v, out, start, nmesh, boxsize, origin):
        """out = v * Y_lm(r_hat) over the local real block v, r_hat the direction from `origin` to each cell
        (pmx_ylm_weight); out may be v or raw memory"""
        if v.numel() == 0:
            return
        self.call('ylm_weight', int(ell), int(m), v.dim(), v.element_size(), v.data_ptr(), _byte_strides(v),
                  out.data_ptr(), _byte_strides(out), _abi.i64arr(v.shape, 3), *_mesh_args(start, nmesh, boxsize),
                  _abi.f64arr(origin, 3), self.stream())

    def ylm_accumulate(self, ell, m, beta, v, acc, start, nmesh, boxsize):
        """acc = beta * acc + (4 pi / (2 ell + 1)) Y_lm(k_hat) v over the local complex block v, beta 0 or 1
        (pmx_ylm_accumulate); with beta = 0 acc may be raw memory"""
        if v.numel() == 0:
            return
        es = v.element_size()
        self.call('ylm_accumulate', int(ell), int(m), int(beta), v.dim(), es // 2, v.data_ptr(), _byte_strides(v),
                  acc.data_ptr(), _byte_strides(acc), _abi.i64arr(v.shape, 3), *_mesh_args(start, nmesh, boxsize),
                  self.stream())

    # -- interlaced painting: the combine pass ---------------------------------
    def phase_combine(self, v, acc, start, nmesh, shift, a, b, deconv_pow=0):
        """acc = (a * acc + b * exp(i sum_d shift_d w_d) * v) / prod_d sinc(w_d / 2)^deconv_pow over the local complex
        block v (pmx_phase_combine); v and acc must not overlap, and with a = 0 acc may be raw memory"""
        if v.numel() == 0:
            return
        es = v.element_size()
        self.call('phase_combine', v.dim(), es // 2, v.data_ptr(), _byte_strides(v), acc.data_ptr(),
                  _byte_strides(acc), _abi.i64arr(v.shape, 3), _abi.i64arr(start, 3), _abi.i64arr(nmesh, 3),
                  _abi.f64arr(shift, 3), float(a), float(b), int(deconv_pow), self.stream())

    # -- binned correlation function ------------------------------------------
    def corr_project(self, params, x, start, nmesh, boxsize, redges, muedges, acc):
        """add the binned sums of the local real block `x` over the separations of its cells into the float64 device
        vector `acc` (layout: include/pmesh_amd.h, pmx_corr_project)"""
        if x.numel() == 0:
            return
        self.call('corr_project', C.byref(params), x.dim(), x.element_size(), x.data_ptr(), _byte_strides(x),
                  _abi.i64arr(x.shape, 3), *_mesh_args(start, nmesh, boxsize), redges.data_ptr(),
                  muedges.data_ptr() if muedges is not None else None, acc.data_ptr(), self.stream())

    def corr_vjp(self, params, g, start, nmesh, boxsize, redges, muedges, coef):
        """every cell of the local real block `g` (may be raw memory) = the adjoint of corr_project for the coefficient
        table `coef`, a float64 device vector (layout: include/pmesh_amd.h, pmx_corr_vjp)"""
        if g.numel() == 0:
            return
        self.call('corr_vjp', C.byref(params), g.dim(), g.element_size(), g.data_ptr(), _byte_strides(g),
                  _abi.i64arr(g.shape, 3), *_mesh_args(start, nmesh, boxsize), redges.data_ptr(),
                  muedges.data_ptr() if muedges is not None else None, coef.data_ptr(), self.stream())

    def spectral_product(self, x, y, out, start, nmesh, scale=1.0, conj_y=False, accumulate=False, deconv_pow=0):
        """out = [out +] scale * x * (conj(y) or y) / prod_d sinc(w_d / 2)^deconv_pow over the local complex blocks
        (pmx_spectral_product); out may be x or y itself, and without `accumulate` raw memory"""
        if x.numel() == 0:
            return
        es = x.element_size()
        self.call('spectral_product', x.dim(), es // 2, x.data_ptr(), _byte_strides(x), y.data_ptr(), _byte_strides(y),
                  out.data_ptr(), _byte_strides(out), _abi.i64arr(x.shape, 3), _abi.i64arr(start, 3),
                  _abi.i64arr(nmesh, 3), float(scale), int(bool(conj_y)), int(bool(accumulate)), int(deconv_pow),
                  self.stream())

    # -- Poisson-sampled particles ---------------------------------------------
    def poisson_rate_sum(self, x, mode, scale, bias, total):
        """total[0] += the sum of the rates of the local real block `x` (pmx_poisson_rate_sum); total is a float64
        device tensor of one element"""
        if x.numel() == 0:
            return
        self.call('poisson_rate_sum', x.dim(), x.element_size(), x.data_ptr(), _byte_strides(x),
                  _abi.i64arr(x.shape, 3), int(mode), float(scale), float(bias), total.data_ptr(), self.stream())

    def poisson_count(self, x, start, nmesh, mode, scale, bias, seed, counts, seg_sums, flagged):
        """the Poisson counts of the local real block `x` into the contiguous uint32 tensor `counts`, their sums per
        segment of PMX_POISSON_SEGMENT cells into the int64 tensor `seg_sums`, the number of refused cells added to
        the int64 tensor `flagged` of one element (pmx_poisson_count)"""
        if x.numel() == 0:
            return
        self.call('poisson_count', x.dim(), x.element_size(), x.data_ptr(), _byte_strides(x), _abi.i64arr(x.shape, 3),
                  _abi.i64arr(start, 3), _abi.i64arr(nmesh, 3), int(mode), float(scale), float(bias), int(seed),
                  counts.data_ptr(), seg_sums.data_ptr(), flagged.data_ptr(), self.stream())

    def poisson_scan(self, seg_sums, total):
        """the exclusive scan of the int64 tensor `seg_sums` in place, its total into the int64 tensor `total` of one
        element (pmx_poisson_scan)"""
        self.call('poisson_scan', seg_sums.data_ptr() if seg_sums.numel() else None, seg_sums.numel(),
                  total.data_ptr(), self.stream())

    def poisson_emit(self, shape, start, nmesh, boxsize, seed, counts, seg_offsets, pos, cell=None):
        """the particles of the counts into the rows of the (n, ndim) float64 tensor `pos` and, when given, their
        global cell indices into the int64 tensor `cell` (pmx_poisson_emit)"""
        if pos.shape[0] == 0:
            return
        self.call('poisson_emit', len(shape), _abi.i64arr(shape, 3), *_mesh_args(start, nmesh, boxsize), int(seed),
                  counts.data_ptr(), seg_offsets.data_ptr(), pos.shape[0], pos.data_ptr(),
                  cell.data_ptr() if cell is not None else None, self.stream())

    # -- friends-of-friends groups -----------------------------------------------
    def fof_cells(self, pos, boxsize, origin, inv_side, ncell, periodic, wpos, cell_of, counts, flagged):
        """the wrapped rows of the (n, ndim) tensor `pos` into `wpos` (float64), their flat cells into `cell_of`
        (int32), the rows per cell added to the zeroed `counts` (int32), the rows that are not finite to the int64
        tensor `flagged` of one element (pmx_fof_cells)"""
        if pos.shape[0] == 0:
            return
        pv = _arrays.vec(pos)
        self.call('fof_cells', len(ncell), C.byref(pv), pos.shape[0], _abi.f64arr(boxsize, 3), _abi.f64arr(origin, 3),
                  _abi.f64arr(inv_side, 3), _abi.i64arr(ncell, 3), int(periodic), wpos.data_ptr(), cell_of.data_ptr(),
                  counts.data_ptr(), flagged.data_ptr(), self.stream())

    def fof_fill(self, wpos, cell_of, cell_start, cursor, order, spos):
        """the rows in cell order: `order` (int32) and the wrapped rows sorted into `spos`; `cursor` is a zeroed int32
        tensor of one entry per cell (pmx_fof_fill)"""
        if wpos.shape[0] == 0:
            return
        self.call('fof_fill', wpos.shape[1], wpos.shape[0], wpos.data_ptr(), cell_of.data_ptr(), cell_start.data_ptr(),
                  cursor.data_ptr(), order.data_ptr(), spos.data_ptr(), self.stream())

    def fof_link(self, spos, order, cell_of, cell_start, ncell, periodic, boxsize, b2, parent):
        """the union-find of the friends into the int32 tensor `parent` (pmx_fof_link)"""
        if spos.shape[0] == 0:
            return
        self.call('fof_link', spos.shape[1], spos.shape[0], spos.data_ptr(), order.data_ptr(), cell_of.data_ptr(),
                  cell_start.data_ptr(), _abi.i64arr(ncell, 3), int(periodic), _abi.f64arr(boxsize, 3), float(b2),
                  parent.data_ptr(), self.stream())

    def fof_flatten(self, parent):
        """parent[i] = the root of row i, in place (pmx_fof_flatten)"""
        if parent.numel():
            self.call('fof_flatten', parent.numel(), parent.data_ptr(), self.stream())

    def fof_minlabel(self, root, val, work, changed):
        """the int64 tensor `val` replaced by its minimum over every component of `root`, the number of rows that
        changed added to the int64 tensor `changed` of one element; `work` is int64 scratch (pmx_fof_minlabel)"""
        if val.numel():
            self.call('fof_minlabel', val.numel(), root.data_ptr(), val.data_ptr(), work.data_ptr(),
                      changed.data_ptr(), self.stream())

    def fof_group_sums(self, pos, labels, mass, vel, ref, boxsize, out):
        """the sums per label of (mass, mass x displacement from ref, mass x vel) added into the zeroed float64 tensor
        `out` of shape (ngroups + 1, 1 + 2 ndim) (pmx_fof_group_sums)"""
        if pos.shape[0] == 0 or out.shape[0] <= 1:
            return
        pv, mv, vv = _arrays.vec(pos), _arrays.vec(mass), _arrays.vec(vel)
        self.call('fof_group_sums', ref.shape[1], pos.shape[0], C.byref(pv), labels.data_ptr(),
                  C.byref(mv) if mass is not None else None, C.byref(vv) if vel is not None else None,
                  ref.data_ptr(), out.shape[0] - 1, _abi.f64arr(boxsize, 3), out.data_ptr(), self.stream())

    # -- binned pair counts ------------------------------------------------------
    def pair_counts(self, mode, los, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                    periodic, boxsize, e2, sub, npairs, wnpairs, rsum):
        """the binned sums over the pairs of the primaries (spos1, order1, cell_of1: what fof_cells / fof_fill left of
        them) with the secondaries (spos2, order2, cell_start2, of the same grid) added into the zeroed tensors `npairs`
        (int64), `wnpairs` and `rsum` (float64) of nr * nsub entries.  mode: PMX_PAIRS_*; e2: the nr + 1 squared edges
        on the device; sub: the nsub + 1 squared mu edges or pi edges on the device, None in the mode 1D; weight1 /
        weight2: (n,) or (n, 1) float tensors in row order, or None (pmx_pair_counts).  In the three velocity modes
        (PMX_PAIRS_1D_VELOCITY, PMX_PAIRS_PROJECTED_VELOCITY, PMX_PAIRS_1D_LOS) weight1 / weight2 are the (n, 1 + ndim)
        or (n, 2) blocks of columns of the two sets and `rsum` has 4 * nr * nsub entries.  In the modes by row labels
        (PMX_PAIRS_SPLIT | m, PMX_PAIRS_JACKKNIFE | m) they are the (n, 2) blocks (w, label), and `npairs` and `wnpairs`
        have 2 (split) or 1 + 2 K (jackknife, K = (PMX_PAIRS_LABEL_SLOTS / nbins - 2) / 2) blocks of nbins entries,
        `rsum` 2 or 1.  In the two alignment modes (PMX_PAIRS_ALIGN | PMX_PAIRS_1D, PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED)
        they are the (n, 1 + ndim) blocks (w, a) or the (n, 3) blocks (w, g1, g2), and `rsum` has 4 or 7 times nr * nsub
        entries.  In the moments mode (PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS) weight1 is the (n1, 2) block (w, s2),
        weight2 the (n2, 1) block (m) or the (n2, 1 + ndim) block (m, v), `sub` is None, `npairs` and `wnpairs` have
        n1 * nr entries and `rsum` NS * n1 * nr, NS = 1 + ndim + ndim (ndim + 1), with velocities ndim + 1 + (3 if ndim
        == 3 else 1) more"""
        if spos1.shape[0] == 0 or spos2.shape[0] == 0:
            return
        if int(mode) in (_abi.PMX_PAIRS_1D_VELOCITY, _abi.PMX_PAIRS_PROJECTED_VELOCITY, _abi.PMX_PAIRS_1D_LOS):
            nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
            if rsum.numel() < 4 * nbins or min(npairs.numel(), wnpairs.numel()) < nbins:
                raise ValueError('the velocity modes need rsum of 4 * nr * nsub entries')
            for w, s in ((weight1, spos1), (weight2, spos2)):
                if w is None or w.dim() != 2 or w.shape[0] != s.shape[0]:
                    raise ValueError('the velocity modes need weight1 and weight2 as (n, ncol) blocks of the rows')
        if int(mode) in (_abi.PMX_PAIRS_ALIGN | _abi.PMX_PAIRS_1D, _abi.PMX_PAIRS_ALIGN | _abi.PMX_PAIRS_PROJECTED):
            # the alignment modes: (n, 1 + ndim) or (n, 3) blocks; rsum of 4 or 7 times nbins entries
            nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
            nsums = 7 if int(mode) & 7 == _abi.PMX_PAIRS_PROJECTED else 4
            if rsum.numel() < nsums * nbins or min(npairs.numel(), wnpairs.numel()) < nbins:
                raise ValueError('the alignment modes need rsum of %d * nr * nsub entries' % nsums)
            for w, s in ((weight1, spos1), (weight2, spos2)):
                if w is None or w.dim() != 2 or w.shape[0] != s.shape[0]:
                    raise ValueError('the alignment modes need weight1 and weight2 as (n, ncol) blocks of the rows')
        if int(mode) == _abi.PMX_PAIRS_MOMENTS | _abi.PMX_PAIRS_1D_ROWS:
            # the moments mode: (n1, 2) against (n2, 1) or (n2, 1 + ndim); rsum of NS * n1 * nr entries; no sub axis
            nd, n1, nr = spos1.shape[1], spos1.shape[0], e2.numel() - 1
            if sub is not None:
                raise ValueError('the moments mode takes no sub axis')
            if nr > _abi.PMX_PAIRS_MOMENTS_MAX_BINS:
                raise ValueError('the moments mode takes at most %d bins' % _abi.PMX_PAIRS_MOMENTS_MAX_BINS)
            if weight1 is None or weight1.dim() != 2 or tuple(weight1.shape) != (n1, 2):
                raise ValueError('the moments mode needs weight1 as the (n1, 2) block (w, s2)')
            if weight2 is None or weight2.dim() != 2 or weight2.shape[0] != spos2.shape[0] \
                    or weight2.shape[1] not in (1, 1 + nd):
                raise ValueError('the moments mode needs weight2 as the (n2, 1) block (m) or the (n2, 1 + ndim) block '
                                 '(m, v)')
            nsums = 1 + nd + nd * (nd + 1) + ((nd + 1 + (3 if nd == 3 else 1)) if weight2.shape[1] > 1 else 0)
            if rsum.numel() < nsums * n1 * nr or min(npairs.numel(), wnpairs.numel()) < n1 * nr:
                raise ValueError('the moments mode needs npairs and wnpairs of n1 * nr entries and rsum of %d * n1 * nr'
                                 % nsums)
        split, jack = int(mode) & ~7 == _abi.PMX_PAIRS_SPLIT, int(mode) & ~7 == _abi.PMX_PAIRS_JACKKNIFE
        if split or jack:
            # the modes by row labels: (n, 2) blocks (w, label); 2 or 1 + 2 K blocks of nbins entries (rsum: 2 or 1)
            nbins = (e2.numel() - 1) * (sub.numel() - 1 if sub is not None else 1)
            K = (_abi.PMX_PAIRS_LABEL_SLOTS // nbins - 2) // 2
            if K < 1:
                raise ValueError('the modes by row labels take at most %d bins' % (_abi.PMX_PAIRS_LABEL_SLOTS // 4))
            ncount, nrsum = (2 * nbins, 2 * nbins) if split else ((1 + 2 * K) * nbins, nbins)
            if min(npairs.numel(), wnpairs.numel()) < ncount or rsum.numel() < nrsum:
                raise ValueError('the modes by row labels need npairs and wnpairs of %d entries and rsum of %d here'
                                 % (ncount, nrsum))
            for w, s in ((weight1, spos1), (weight2, spos2)):
                if w is None or w.dim() != 2 or w.shape[0] != s.shape[0] or w.shape[1] != 2:
                    raise ValueError('the modes by row labels need weight1 and weight2 as (n, 2) blocks (w, label)')
        wv1, wv2 = _arrays.vec(weight1), _arrays.vec(weight2)
        self.call('pair_counts', spos1.shape[1], int(mode), int(los), spos1.shape[0], spos1.data_ptr(),
                  order1.data_ptr(), cell_of1.data_ptr(), C.byref(wv1) if weight1 is not None else None,
                  spos2.shape[0], spos2.data_ptr(), order2.data_ptr(), cell_start2.data_ptr(),
                  C.byref(wv2) if weight2 is not None else None, _abi.i64arr(ncell, 3), int(periodic),
                  _abi.f64arr(boxsize, 3), e2.numel() - 1, e2.data_ptr(), sub.numel() - 1 if sub is not None else 1,
                  sub.data_ptr() if sub is not None else None, npairs.data_ptr(), wnpairs.data_ptr(), rsum.data_ptr(),
                  self.stream())

    def threept_multipoles(self, spos1, order1, cell_of1, weight1, spos2, order2, cell_start2, weight2, ncell,
                           periodic, boxsize, e2, lmax, zeta, diag, wpairs, npairs):
        """the sums of the three-point multipoles of the primaries with the secondaries (as in pair_counts, three
        columns) added into the zeroed tensors `zeta` (float64, (lmax + 1, nr, nr)), `diag`, `wpairs` (float64, nr) and
        `npairs` (int64, nr).  e2: the nr + 1 squared edges on the device (pmx_threept_multipoles)"""
        if spos1.shape[0] == 0 or spos2.shape[0] == 0:
            return
        wv1, wv2 = _arrays.vec(weight1), _arrays.vec(weight2)
        self.call('threept_multipoles', spos1.shape[0], spos1.data_ptr(), order1.data_ptr(), cell_of1.data_ptr(),
                  C.byref(wv1) if weight1 is not None else None, spos2.shape[0], spos2.data_ptr(), order2.data_ptr(),
                  cell_start2.data_ptr(), C.byref(wv2) if weight2 is not None else None, _abi.i64arr(ncell, 3),
                  int(periodic), _abi.f64arr(boxsize, 3), e2.numel() - 1, e2.data_ptr(), int(lmax), zeta.data_ptr(),
                  diag.data_ptr(), wpairs.data_ptr(), npairs.data_ptr(), self.stream())

    def short_range(self, spos1, order1, cell_of1, spos2, order2, cell_start2, mass2, ncell, periodic, boxsize, G,
                    r_split, rc2, eps2, acc, pot=None, neighbours=None):
        """the short-range pair force of the primaries from the sources (as in pair_counts, three columns) written to
        the rows of `acc` (float64, (n1, 3)), `pot` (float64, n1) and `neighbours` (int64, n1), the last two or None,
        in row order: overwritten, not added to.  mass2: an (n2,) or (n2, 1) float tensor in row order, or None
        (pmx_short_range)"""
        if spos1.shape[0] == 0:
            return
        mv = _arrays.vec(mass2)
        self.call('short_range', spos1.shape[0], spos1.data_ptr(), order1.data_ptr(), cell_of1.data_ptr(),
                  spos2.shape[0], spos2.data_ptr(), order2.data_ptr(), cell_start2.data_ptr(),
                  C.byref(mv) if mass2 is not None else None, _abi.i64arr(ncell, 3), int(periodic),
                  _abi.f64arr(boxsize, 3), float(G), float(r_split), float(rc2), float(eps2), acc.data_ptr(),
                  pot.data_ptr() if pot is not None else None,
                  neighbours.data_ptr() if neighbours is not None else None, self.stream())

    def knn(self, spos1, order1, cell_of1, spos2, order2, cell_start2, ncell, periodic, boxsize, r2max, k, dist2,
            index=None, count=None):
        """the k smallest r2 < r2max of the primaries among the sources (as in pair_counts, ndim columns) written to
        the rows of `dist2` (float64, (n1, k), ascending, +inf where there are fewer), the local source rows to `index`
        (int32, (n1, k), -1 where inf) and the number of sources with r2 < r2max to `count` (int64, n1), the last two
        or None, in row order: overwritten (pmx_knn)"""
        if spos1.shape[0] == 0:
            return
        self.call('knn', spos1.shape[1], spos1.shape[0], spos1.data_ptr(), order1.data_ptr(), cell_of1.data_ptr(),
                  spos2.shape[0], spos2.data_ptr(), order2.data_ptr(), cell_start2.data_ptr(), _abi.i64arr(ncell, 3),
                  int(periodic), _abi.f64arr(boxsize, 3), float(r2max), int(k), dist2.data_ptr(),
                  index.data_ptr() if index is not None else None,
                  count.data_ptr() if count is not None else None, self.stream())

    def lpt_hessian(self, v, pairs, outs, start, nmesh, boxsize):
        """outs[p] = k_i k_j / k^2 v for (i, j) = pairs[p], 1-3 outputs, over the local complex block v
        (pmx_lpt_hessian)"""
        es = v.element_size()
        n = len(outs)
        ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        strides = _abi.i64arr([s * es for o in outs for s in (list(o.stride()) + [0] * 3)[:3]])
        flat = (C.c_int32 * (2 * n))(*[int(x) for p in pairs for x in p])
        self.call('lpt_hessian', v.dim(), es // 2, v.data_ptr(), _byte_strides(v), n, flat,
                  ptrs, strides, _abi.i64arr(v.shape, 3), *_mesh_args(start, nmesh, boxsize), self.stream())

    def lpt2_source(self, ins, out, scale):
        """out = scale * S(phi_ij) over real blocks: ins = the diagonal, then the off-diagonal components
        (pmx_lpt2_source); out may be ins[0]"""
        es = out.element_size()
        ptrs = (C.c_void_p * len(ins))(*[a.data_ptr() for a in ins])
        strides = _abi.i64arr([s * es for a in ins for s in (list(a.stride()) + [0] * 3)[:3]])
        self.call('lpt2_source', out.dim(), es, ptrs, strides, out.data_ptr(),
                  _byte_strides(out), _abi.i64arr(out.shape, 3), float(scale),
                  self.stream())

    @staticmethod
    def _ptr_set(ts, es):
        ptrs = (C.c_void_p * len(ts))(*[a.data_ptr() for a in ts])
        strides = _abi.i64arr([s * es for a in ts for s in (list(a.stride()) + [0] * 3)[:3]])
        return ptrs, strides

    def lpt_contract(self, ins, factors, out, accumulate, start, nmesh, boxsize):
        """out = (accumulate ? out : 0) + sum_c f_c(k) ins[c] over local complex blocks, 1-6 inputs; factors[c] = (i, j)
        for k_i k_j / k^2 or (d, -1) for -i k_d / k^2 (pmx_lpt_contract); out may be ins[0]"""
        es = out.element_size()
        ptrs, strides = self._ptr_set(ins, es)
        flat = (C.c_int32 * (2 * len(ins)))(*[int(x) for f in factors for x in f])
        self.call('lpt_contract', out.dim(), es // 2, len(ins), ptrs, strides, flat, int(bool(accumulate)),
                  out.data_ptr(), _byte_strides(out), _abi.i64arr(out.shape, 3),
                  *_mesh_args(start, nmesh, boxsize), self.stream())

    def lpt2_source_vjp(self, g, ins, outs, scale):
        """outs[p] = scale * g * dS / d ins[p] over real blocks, components in the order of lpt2_source
        (pmx_lpt2_source_vjp); outs[p] may be ins[p]"""
        es = g.element_size()
        ip, istr = self._ptr_set(ins, es)
        op, ostr = self._ptr_set(outs, es)
        self.call('lpt2_source_vjp', g.dim(), es, g.data_ptr(), _byte_strides(g), ip,
                  istr, op, ostr, _abi.i64arr(g.shape, 3), float(scale), self.stream())

    def lpt2_source_jvp(self, ins, tangents, out, scale):
        """out = scale * dS(ins; tangents) over real blocks (pmx_lpt2_source_jvp); out may be tangents[0]"""
        es = out.element_size()
        ip, istr = self._ptr_set(ins, es)
        tp, tstr = self._ptr_set(tangents, es)
        self.call('lpt2_source_jvp', out.dim(), es, ip, istr, tp, tstr, out.data_ptr(),
                  _byte_strides(out), _abi.i64arr(out.shape, 3), float(scale),
                  self.stream())


_current = None


def use(backend):
    """Install a backend object (tests only; see module docstring)."""
    global _current
    _current = backend
    return backend


def get():
    """The active backend; creates the HIP backend on first use and raises if
    that is impossible."""
    global _current
    if _current is None:
        _current = HipBackend()
    return _current


def reset():
    global _current
    _current = None
