"""The case table of tests/test_streams.py: one small object per operation of the library.

A case builds its plans, fields and output buffers once (its constructor), and has four methods:

    make(seed)            the input tensors of the operation, drawn from `seed`: finite, inside the box, valid in every
                          respect, of the same shapes and row counts for every seed
    load(inputs, values)  copies `values` (what another make() returned) into the tensors `inputs`, in place
    run(inputs)           the operation on `inputs`; returns its output tensors (the case's own buffers where the
                          operation has an out= form: a later run overwrites them, so a caller clones what it keeps)
    bound()               None where the operation is documented as deterministic (the outputs of two runs are equal bit
                          for bit), else a function of the outputs `want` that returns one array of absolute bounds per
                          output: TWICE the bound the operation's own test module uses against its reference (both
                          sides of a comparison here are device results, each within that bound of the same reference).
                          The function is called right after the run that made `want`, before any other run

and three attributes: `host_async` (the call returns without waiting for the device: set from include/pmesh_amd.h and
from the code of the Python layer, not from observation), `graph` (the warm code path makes no allocation, no
synchronous copy and no stream synchronisation: the case is also captured into a graph) and `entries`, the pmx_* names
the case is there for: those it enqueues BEFORE its first read-back to the host.  A read-back waits for the stream, and
with it for the delayed copy of the inputs, so a kernel behind it is not tested by the delay: such an entry is named by
another case that launches it with nothing read in front of it.

Producers.  An entry without an input tensor (white noise from a seed, the synthetic particle sets) writes a buffer that
`load` fills first and whose result is multiplied by an input afterwards, both with torch on the current stream: run
on another stream than the caller's, its result is overwritten by that fill.

Everything a kernel can read holds valid data at all times: the inputs of either seed.  No case hands an entry an
index array that it has not filled.
"""
import contextlib
import ctypes as C

import numpy
import torch

from pmesh_amd import _abi, domain, window
from pmesh_amd._arrays import vec
from pmesh_amd.pm import ParticleMesh

BOX = 1000.0
NROWS = 20000            # rows of the paint and readout cases
NPART = 4096             # rows of the particle modules, in a unit box
MESH = (32, 32, 32)      # rocFFT transforms
TILE = (16, 32, 64)      # as many cells, and the smallest mesh the tile kernels take: a tile of 8 x 16 x 32 cells and its
                         # halo must fit every axis (pmx_binplan_supported)
OWN = (64, 64, 128)      # the smallest mesh whose three passes are all the LDS row / column kernels


@contextlib.contextmanager
def flags(**kw):
    """module-level switches of pmesh_amd.window for the length of a call"""
    old = {k: getattr(window, k) for k in kw}
    for k, v in kw.items():
        setattr(window, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(window, k, v)


def rng(seed, salt=0):
    return numpy.random.RandomState(1000 * salt + seed)


def tdtype(dtype, complex_=False):
    if complex_:
        return torch.complex128 if dtype == 'f8' else torch.complex64
    return torch.float64 if dtype == 'f8' else torch.float32


class Case(object):
    host_async = True
    graph = False
    entries = ()

    def __init__(self, be):
        self.be = be
        self.dev = be.device

    def t(self, a, dtype=None):
        x = torch.from_numpy(numpy.ascontiguousarray(a)).to(self.dev)
        return x if dtype is None else x.to(dtype)

    def make(self, seed):
        raise NotImplementedError

    def load(self, inputs, values):
        assert len(inputs) == len(values)
        for a, b in zip(inputs, values):
            assert a.shape == b.shape and a.dtype == b.dtype
            a.copy_(b)

    def run(self, inputs):
        raise NotImplementedError

    def bound(self):
        return None

    # what a capture must find untouched: the buffers the run writes (default: its outputs)
    def written(self, outputs):
        return outputs


def scale_bound(tol, floor=1.0):
    """twice tol * max(floor, max |want|), per output: the rule of tests/test_window.py (check_paint) and
    tests/test_bin_blocks.py (close_paint)"""
    def f(want):
        out = []
        for w in want:
            a = numpy.abs(host(w))
            m = float(numpy.nanmax(a)) if a.size and numpy.isfinite(a).any() else 0.0
            out.append(numpy.full(a.shape, 2 * tol * max(floor, m)))
        return out
    return f


def host(t):
    """an output as a numpy array of real numbers or integers"""
    if isinstance(t, numpy.ndarray):
        a = t
    else:
        a = t.detach().cpu()
        if a.is_complex():
            a = torch.view_as_real(a.contiguous())
        if a.dtype == torch.uint32:
            a = a.to(torch.int64)
        a = a.numpy()
    if numpy.iscomplexobj(a):
        a = numpy.ascontiguousarray(a).view(a.real.dtype).reshape(a.shape + (2,))
    return a


def as_tensor(a):
    """a numpy result of the Python layer as a (host) tensor"""
    a = numpy.ascontiguousarray(a)
    if numpy.iscomplexobj(a):
        a = a.view(a.real.dtype).reshape(a.shape + (2,))
    return torch.from_numpy(a.copy())


# ---- mesh: paint and readout ------------------------------------------------------------------------------------------

def paint_tol(dtype):
    from tests.test_window import TOL_F4, TOL_F8
    return TOL_F8 if dtype == 'f8' else TOL_F4


class Paint(Case):
    """pm.paint into a field of the caller's: the tile kernels (BINNED 'always': pmx_binplan_build, pmx_paint_binned,
    pmx_mass_stats with a mass tensor) or the direct ones of csrc/pmx_window.hip (pmx_paint)"""

    def __init__(self, be, kind, dtype, path='tile', mass=False, gradient=None, deterministic=False, rows=NROWS):
        Case.__init__(self, be)
        self.rows = rows
        self.pm = ParticleMesh(TILE if path == 'tile' else MESH, BoxSize=BOX, dtype=dtype, resampler=kind)
        self.rho = self.pm.create(type='real')
        self.kind, self.dtype, self.path, self.mass, self.gradient = kind, dtype, path, mass, gradient
        self.deterministic = deterministic
        if path == 'tile':
            self.entries = ('pmx_binplan_build', 'pmx_paint_binned') + (('pmx_mass_stats',) if mass else ())
        else:
            self.entries = ('pmx_paint',)

    def make(self, seed):
        r = rng(seed, 1)
        ins = [self.t(r.uniform(0, BOX, size=(self.rows, 3)))]
        if self.mass:
            ins.append(self.t(r.uniform(0.5, 1.5, size=self.rows)))
        return ins

    def run(self, ins):
        with flags(BINNED='always' if self.path == 'tile' else 'never', DETERMINISTIC=self.deterministic):
            self.pm.paint(ins[0], mass=ins[1] if self.mass else 1.0, gradient=self.gradient, out=self.rho)
        return [self.rho.value]

    def bound(self):
        # the deterministic mode is pinned bit for bit (tests/test_binned.py); the default mode adds with float atomics
        return None if self.deterministic else scale_bound(paint_tol(self.dtype))


class Readout(Case):
    """RealField.readout / ParticleMesh.readout (readout_many) into a buffer of the caller's: bit for bit"""

    def __init__(self, be, kind, dtype, path='tile', gradient=None, many=False, rows=NROWS):
        Case.__init__(self, be)
        self.rows = rows
        self.nmesh = TILE if path == 'tile' else MESH
        self.pm = ParticleMesh(self.nmesh, BoxSize=BOX, dtype=dtype, resampler=kind)
        self.fields = [self.pm.create(type='real') for _ in range(3 if many else 1)]
        self.out = torch.empty((rows, 3) if many else (rows,), dtype=torch.float64, device=self.dev)
        self.path, self.gradient, self.many, self.dtype = path, gradient, many, dtype
        if path == 'tile':
            self.entries = ('pmx_binplan_build', 'pmx_readout_binned_multi' if many else 'pmx_readout_binned')
        else:
            self.entries = ('pmx_readout',)

    def make(self, seed):
        r = rng(seed, 2)
        return [self.t(r.uniform(0, BOX, size=(self.rows, 3)))] + \
               [self.t(r.normal(size=self.nmesh), tdtype(self.dtype)) for _ in self.fields]

    def run(self, ins):
        for f, v in zip(self.fields, ins[1:]):
            f.value.copy_(v)
        with flags(BINNED='always' if self.path == 'tile' else 'never'):
            if self.many:
                self.pm.readout(self.fields, ins[0], out=self.out, gradient=self.gradient)
            else:
                self.fields[0].readout(ins[0], out=self.out, gradient=self.gradient)
        return [self.out]


class PaintReadoutND(Case):
    """a 4-d mesh: pmx_paint_nd and pmx_readout_nd (the generic per-particle kernels)"""
    entries = ('pmx_paint_nd', 'pmx_readout_nd')

    def __init__(self, be):
        Case.__init__(self, be)
        self.canvas = torch.zeros((8, 8, 8, 8), dtype=torch.float64, device=self.dev)
        self.out = torch.empty(NPART, dtype=torch.float64, device=self.dev)
        self.aff = window.Affine(4, period=8)

    def make(self, seed):
        return [self.t(rng(seed, 3).uniform(0, 8, size=(NPART, 4)))]

    def run(self, ins):
        self.canvas.zero_()
        window.CIC.paint(self.canvas, ins[0], transform=self.aff)
        window.CIC.readout(self.canvas, ins[0], out=self.out, transform=self.aff)
        return [self.canvas, self.out]

    def bound(self):
        from tests.test_window import TOL_F8
        return scale_bound(TOL_F8)


class Interlaced(Case):
    """paint_interlaced: two displaced paints, their transforms and pmx_phase_combine.  The paints run in the
    deterministic mode, so the whole chain is bit for bit"""
    entries = ('pmx_phase_combine', 'pmx_binplan_build')

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(TILE, BoxSize=BOX, dtype=dtype)
        self.out = self.pm.create(type='complex')

    def make(self, seed):
        r = rng(seed, 4)
        return [self.t(r.uniform(0, BOX, size=(NROWS, 3))), self.t(r.uniform(0.5, 1.5, size=NROWS))]

    def run(self, ins):
        from pmesh_amd.interlace import paint_interlaced
        with flags(DETERMINISTIC=True):
            paint_interlaced(self.pm, ins[0], mass=ins[1], compensate=True, out=self.out)
        return [self.out.value]


class TileOrder(Case):
    """pm.tile_order.  The permutation is tile-major, but the order of the rows inside a tile is that of the plan's
    list and changes from build to build: what is compared is, per row, the tile in whose range the permutation puts
    it (the ranges from the tile populations of the positions themselves)"""
    entries = ('pmx_binplan_build', 'pmx_binplan_order')

    def __init__(self, be):
        Case.__init__(self, be)
        self.pm = ParticleMesh(TILE, BoxSize=BOX)
        self.scale = self.t(numpy.array(TILE) / BOX)
        self.nt = [n // t for n, t in zip(TILE, (8, 16, 32))]
        self.tile = self.t(numpy.array([8, 16, 32]))

    def make(self, seed):
        return [self.t(rng(seed, 5).uniform(0, BOX, size=(NROWS, 3)))]

    def run(self, ins):
        with flags(BINNED='always'):
            o = self.pm.tile_order(ins[0])
        # the tile of the first cell of a row's CIC stencil
        t = torch.div(torch.floor(ins[0] * self.scale).to(torch.int64), self.tile, rounding_mode='floor')
        tid = (t[:, 0] * self.nt[1] + t[:, 1]) * self.nt[2] + t[:, 2]
        # (scatter_add_, not bincount: that one reads the largest value back to the host)
        counts = torch.zeros(self.nt[0] * self.nt[1] * self.nt[2], dtype=torch.int64, device=self.dev)
        counts.scatter_add_(0, tid, torch.ones_like(tid))
        ends = torch.cumsum(counts, 0)
        rank = torch.empty_like(o)
        rank[o] = torch.arange(NROWS, dtype=torch.int64, device=self.dev)
        return [torch.searchsorted(ends, rank, right=True)]


class DeferredPaint(Case):
    """a paint into a field of its own making leaves its halo merge to the reader: r2c adds the staged halos in its
    row pass (pmx_paint_binned_defer, pmx_rowfft_halo), anyone else runs pmx_halo_merge.  Deterministic inputs: the
    rows sit on multiples of 1/8 cell and the masses are multiples of 1/8, so every CIC weight, product and sum is
    exact and the order of the additions does not matter"""
    entries = ('pmx_paint_binned_defer', 'pmx_rowfft_halo', 'pmx_halo_merge')

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(OWN, BoxSize=[64., 64., 128.], dtype=dtype)
        self.dtype = dtype

    def make(self, seed):
        r = rng(seed, 6)
        pos = r.randint(0, 8 * numpy.array(OWN), size=(NROWS, 3)) / 8.0
        return [self.t(pos), self.t(r.randint(1, 17, size=NROWS) / 8.0)]

    def run(self, ins):
        with flags(BINNED='always'):
            spectrum = self.pm.paint(ins[0], mass=ins[1]).r2c(out=Ellipsis)
            merged = self.pm.paint(ins[0], mass=ins[1])
            return [spectrum.value, merged.value]


# ---- mesh: transforms and transfer functions --------------------------------------------------------------------------

class FFT(Case):
    """r2c and c2r through the public API, in place and out of place, with and without a transfer function: on OWN the
    LDS kernels (pmx_rowfft, pmx_rowfft_to, pmx_colfft, pmx_colfft_to, pmx_colfft_roundtrip), on MESH rocFFT
    (pmx_fft_execute) with the transfer function as a kernel of its own (pmx_apply_transfer)"""

    def __init__(self, be, dtype, nmesh):
        Case.__init__(self, be)
        from pmesh_amd.transfer import Transfer
        self.pm = ParticleMesh(nmesh, BoxSize=BOX, dtype=dtype)
        self.a, self.b = self.pm.create(type='real'), self.pm.create(type='real')
        self.c = self.pm.create(type='complex')
        self.T = Transfer.dx1(1)
        self.dtype, self.nmesh = dtype, nmesh
        if tuple(nmesh) == OWN:
            self.entries = ('pmx_rowfft', 'pmx_rowfft_to', 'pmx_colfft', 'pmx_colfft_to', 'pmx_colfft_roundtrip')
        else:
            self.entries = ('pmx_fft_execute', 'pmx_apply_transfer')

    def make(self, seed):
        return [self.t(rng(seed, 7).normal(size=self.nmesh), tdtype(self.dtype))]

    def run(self, ins):
        self.a.value.copy_(ins[0])
        self.b.value.copy_(ins[0])
        spec = self.a.r2c(out=self.c)                                   # out of place, into the caller's field
        back = spec.c2r(out=self.a, transfer=self.T)                    # out of place, the transfer on the first pass
        same = self.b.r2c(out=Ellipsis).c2r(out=Ellipsis, transfer=self.T)   # in place: the fused middle pass
        fresh = self.a.r2c().c2r()                                      # fields of the calls' own making
        return [spec.value, back.value, same.value, fresh.value]


class ApplyTransfer(Case):
    entries = ('pmx_apply_transfer',)
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        from pmesh_amd.transfer import Transfer
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.src, self.dst = self.pm.create(type='complex'), self.pm.create(type='complex')
        self.T = Transfer(amplitude=1.5, laplace_pow=-1, grad_dir=2, grad_kind='finite4', deconv_pow=2, gauss_r=20.0)
        self.dtype = dtype

    def make(self, seed):
        r = rng(seed, 8)
        shape = tuple(self.src.value.shape)
        return [self.t(r.normal(size=shape) + 1j * r.normal(size=shape), tdtype(self.dtype, True))]

    def run(self, ins):
        self.src.value.copy_(ins[0])
        self.src.apply(self.T, out=self.dst)
        return [self.dst.value]


class Tabulated(Case):
    """Tabulated.apply_vjp: the transfer applied to the cotangent and pmx_ktable_vjp, whose sums come back as a host
    array (not host-asynchronous; both kernels are enqueued before that read).  With vjp=False Field.apply(Tabulated)
    alone, which is asynchronous"""
    host_async = False

    def __init__(self, be, dtype, vjp=True):
        Case.__init__(self, be)
        from pmesh_amd.transfer import Tabulated as Tab
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        k = numpy.geomspace(2 * numpy.pi / BOX * 0.9, numpy.pi * 32 / BOX * 2, 24)
        self.tab = Tab(k, 1.0 / (1.0 + (k / 0.05) ** 2), loglog=True, left=1.0)
        self.f, self.v = self.pm.create(type='complex'), self.pm.create(type='complex')
        self.out = self.pm.create(type='complex')
        self.dtype, self.vjp = dtype, vjp
        self.host_async = not vjp
        self.entries = ('pmx_apply_ktable', 'pmx_ktable_vjp') if vjp else ('pmx_apply_ktable',)

    def make(self, seed):
        r = rng(seed, 9)
        shape = tuple(self.f.value.shape)
        return [self.t(r.normal(size=shape) + 1j * r.normal(size=shape), tdtype(self.dtype, True)) for _ in range(2)]

    def run(self, ins):
        self.f.value.copy_(ins[0])
        self.v.value.copy_(ins[1])
        if not self.vjp:
            self.f.apply(self.tab, out=self.out)
            return [self.out.value]
        grad_field, grad_t = self.tab.apply_vjp(self.f, self.v)
        return [grad_field.value, as_tensor(grad_t)]

    def bound(self):
        if not self.vjp:
            return None
        # the table gradient is a sum with float atomics: tests/test_tabulated_gradients.py
        # (test_kernels_against_restatement) holds it to test_power's RTOL of its largest entry
        rtol = power_rtol()

        def f(want):
            g = numpy.abs(host(want[1]))
            return [numpy.zeros(host(want[0]).shape), numpy.full(g.shape, 2 * rtol * g.max())]
        return f


class WhiteNoise(Case):
    """pmx_whitenoise on the host-seed path (it waits for the copy of its seed tables: not host-asynchronous).  A
    producer: see the module docstring"""
    entries = ('pmx_whitenoise',)
    host_async = False

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.c = self.pm.create(type='complex')
        self.dtype = dtype

    def make(self, seed):
        r = rng(seed, 10)
        shape = tuple(self.c.value.shape)
        return [self.t(r.normal(size=shape) + 1j * r.normal(size=shape), tdtype(self.dtype, True)),
                self.t(r.uniform(0.5, 1.5, size=shape), tdtype(self.dtype))]

    def run(self, ins):
        from pmesh_amd.whitenoise import generate
        self.c.value.copy_(ins[0])
        generate(self.c.value, self.c.start, self.c.Nmesh, 12345, False)
        return [self.c.value * ins[1]]


class Synth(Case):
    """the synthetic particle sets of bench.py: producers"""
    entries = ('pmx_synth_uniform', 'pmx_synth_clustered')

    def __init__(self, be):
        Case.__init__(self, be)
        self.pos = [torch.empty((NROWS, 3), dtype=torch.float64, device=self.dev) for _ in range(2)]
        self.modes = numpy.array([[1, 0, 2, 0.6, 0.0, 0.8, 0.3, 0.5], [0, 2, 1, 0.0, 1.0, 0.0, 0.2, 1.5]], dtype='f8')

    def make(self, seed):
        r = rng(seed, 11)
        return [self.t(r.uniform(0, BOX, size=(NROWS, 3))), self.t(r.uniform(0.5, 1.5, size=(NROWS, 3)))]

    def run(self, ins):
        be = self.be
        for p in self.pos:
            p.copy_(ins[0])
        pv = [vec(p) for p in self.pos]
        be.call('synth_uniform', C.byref(pv[0]), 32, BOX, 7, 0, NROWS, be.stream())
        be.call('synth_clustered', C.byref(pv[1]), 32, BOX, self.modes.ctypes.data_as(C.POINTER(C.c_double)),
                len(self.modes), 0.25, 0, NROWS, be.stream())
        return [self.pos[0] * ins[1], self.pos[1] * ins[1]]


class PMCycle(Case):
    """the cycle of scripts/graph_probe.py: paint without mass, r2c, c2r with a transfer function, readout, all into
    the caller's buffers, the bin plan rebuilt every time.  CIC on rows at multiples of 1/8 cell: the paint's sums are
    exact, the rest is deterministic"""
    entries = ('pmx_binplan_build', 'pmx_paint_binned', 'pmx_readout_binned', 'pmx_colfft', 'pmx_colfft_roundtrip')
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        from pmesh_amd.transfer import Transfer
        self.pm = ParticleMesh((64, 64, 64), BoxSize=64.0, dtype=dtype)
        self.rho = self.pm.create(type='real')
        self.out = torch.empty(NROWS, dtype=torch.float64, device=self.dev)
        self.T = Transfer.dx1(0)

    def make(self, seed):
        return [self.t(rng(seed, 12).randint(0, 8 * 64, size=(NROWS, 3)) / 8.0)]

    def run(self, ins):
        with flags(BINNED='always'):
            window.clear_bin_cache()
            self.pm.paint(ins[0], hold=False, out=self.rho)
            back = self.rho.r2c(out=Ellipsis).c2r(out=Ellipsis, transfer=self.T)
            back.readout(ins[0], out=self.out)
        return [self.out]

    def written(self, outputs):
        # (the whole buffer behind the field, its padding included: `value` is a view of a part of it)
        return [self.out, self.rho._base.storage]


# ---- mesh: the passes of the split and pencil transforms, at entry level ------------------------------------------

class Passes(Case):
    """the LDS passes as the several-rank schedules call them (tests/test_fft_kernels.py has their forms): in place
    ones on a copy of the input, so that a run never consumes it"""
    graph = True

    def __init__(self, be, dtype, which):
        Case.__init__(self, be)
        self.es = 8 if dtype == 'f8' else 4
        self.cdt = tdtype(dtype, True)
        self.which = which
        self.entries = {'col': ('pmx_colfft', 'pmx_colfft_to'), 'row': ('pmx_rowfft', 'pmx_rowfft_to'),
                        'split': ('pmx_colfft_split', 'pmx_colfft_resplit'), 'rowsplit': ('pmx_rowfft_split',),
                        'chunk': ('pmx_colfft_chunk',), 'pack': ('pmx_slab_pack', 'pmx_slab_unpack')}[which]
        # (A, N, B) columns; rows of n reals
        self.A, self.N, self.B = 3, 64, 40
        self.nrows, self.n = 48, 128
        self.pitch = self.n // 2 + 1
        shape = {'col': (self.A, self.N, self.B), 'split': (self.A, self.N, self.B), 'chunk': (self.N, 4, 24),
                 'row': (self.nrows, self.pitch), 'rowsplit': (self.nrows, self.pitch), 'pack': (6, 20, 9)}[which]
        self.shape = shape
        self.work = [torch.zeros(shape, dtype=self.cdt, device=self.dev) for _ in range(4)]
        self.full = torch.zeros((self.N, 4, 40), dtype=self.cdt, device=self.dev)

    def make(self, seed):
        r = rng(seed, 13)
        x = r.normal(size=self.shape) + 1j * r.normal(size=self.shape)
        if self.which in ('row', 'rowsplit'):
            # rows of reals in the layout of an in-place transform: n reals in n / 2 complex slots, the last one padding
            x[:, -1] = 0
        return [self.t(x, self.cdt)]

    def run(self, ins):
        be, es, w = self.be, self.es, self.work
        x = ins[0]
        A, N, B = self.A, self.N, self.B
        if self.which == 'col':
            w[0].copy_(x)
            be.colfft(es, False, w[0], A, N, B, scale=0.5)
            be.colfft_to(es, True, w[0], w[1], A, N, B)
            return [w[0], w[1]]
        if self.which == 'row':
            w[0].copy_(x)
            be.rowfft(es, False, w[0], self.nrows, self.n, self.pitch)
            be.rowfft_to(es, True, w[0], w[1], self.nrows, self.n, self.pitch, scale=1.0 / self.n)
            return [w[0], w[1][:, :self.n // 2]]            # (the inverse writes n reals: the last slot is padding)
        if self.which == 'split':
            be.colfft_split(es, False, x, w[0], A, N, B, 16)
            be.colfft_split(es, True, w[0], w[1], A, N, B, 16, scale=1.0 / N)
            be.colfft_resplit(es, False, w[0], w[2], A, N, B, 16, 32)
            return [w[0], w[1], w[2]]
        if self.which == 'rowsplit':
            offsets = [0, 20, 20, 50, self.pitch]
            be.rowfft_split(es, False, x, w[0], self.nrows, self.n, self.pitch, offsets)
            be.rowfft_split(es, True, w[0], w[1], self.nrows, self.n, self.pitch, offsets, scale=1.0 / self.n)
            return [w[0], w[1][:, :self.n // 2]]
        if self.which == 'chunk':
            # the chunk's transform scattered into columns [8, 32) of the full block, and gathered back from there
            w[0].copy_(x)
            be.colfft_chunk(es, False, w[0], self.full, N, 4, 24, 40, 8, True, scale=0.25)
            be.colfft_chunk(es, True, w[1], self.full, N, 4, 24, 40, 8, False)
            return [self.full[:, :, 8:32], w[1]]
        offsets = [0, 7, 7, 20]
        be.slab_pack(x, w[0], 6, 20, 9, offsets, 2 * es)
        be.slab_pack(w[0], w[1], 6, 20, 9, offsets, 2 * es, inverse=True)
        return [w[0], w[1]]

    def written(self, outputs):
        if self.which == 'chunk':
            return [self.full[:, :, 8:32], self.work[1]]
        return outputs


# ---- spectral statistics --------------------------------------------------------------------------------------------

def complex_input(case, shape, dtype, seed, salt):
    r = rng(seed, salt)
    return case.t(r.normal(size=shape) + 1j * r.normal(size=shape), tdtype(dtype, True))


class LPT(Case):
    """lpt (1LPT, 2LPT), lpt_vjp and lpt_jvp at the rows q; the paints of lpt_vjp in the deterministic mode"""

    def __init__(self, be, dtype, what):
        Case.__init__(self, be)
        self.pm = ParticleMesh(TILE, BoxSize=BOX, dtype=dtype)
        self.d, self.u = self.pm.create(type='complex'), self.pm.create(type='complex')
        self.dtype, self.what = dtype, what
        self.entries = {'lpt1': (), 'lpt2': ('pmx_lpt_hessian', 'pmx_lpt2_source'),
                        'vjp': ('pmx_lpt_contract', 'pmx_lpt2_source_vjp', 'pmx_paint_binned_defer'),
                        'jvp': ('pmx_lpt2_source_jvp',)}[what]

    def spectrum(self, seed, salt):
        """the spectrum of a real field, its Nyquist planes included as r2c leaves them"""
        f = self.pm.create(type='real')
        f.value.copy_(self.t(rng(seed, salt).normal(size=TILE), tdtype(self.dtype)))
        return f.r2c().value.clone()

    def make(self, seed):
        r = rng(seed, 14)
        return [self.spectrum(seed, 15), self.spectrum(seed, 16), self.t(r.uniform(0, BOX, size=(NROWS, 3))),
                self.t(r.normal(size=(NROWS, 3))), self.t(r.normal(size=(NROWS, 3)))]

    def run(self, ins):
        from pmesh_amd.lpt import lpt, lpt_jvp, lpt_vjp
        self.d.value.copy_(ins[0])
        self.u.value.copy_(ins[1])
        q, v1, v2 = ins[2:]
        with flags(DETERMINISTIC=True):
            if self.what == 'lpt1':
                return [lpt(self.d, q, order=1)[0]]
            if self.what == 'lpt2':
                return list(lpt(self.d, q, order=2))
            if self.what == 'vjp':
                g, gq = lpt_vjp(self.d, q, v1, v2, order=2, out_q=True)
                return [g.value, gq]
            return list(lpt_jvp(self.d, q, self.u, v1, order=2))


class LPTEntries(Case):
    """pmx_lpt_hessian, pmx_lpt2_source and pmx_lpt_contract on blocks of the caller's"""
    entries = ('pmx_lpt_hessian', 'pmx_lpt2_source', 'pmx_lpt_contract')
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.dtype = dtype
        self.shape = (32, 32, 17)
        cdt, rdt = tdtype(dtype, True), tdtype(dtype)
        self.h = [torch.zeros(self.shape, dtype=cdt, device=self.dev) for _ in range(3)]
        self.acc = torch.zeros(self.shape, dtype=cdt, device=self.dev)
        self.src = torch.zeros(MESH, dtype=rdt, device=self.dev)

    def make(self, seed):
        r = rng(seed, 17)
        return [complex_input(self, self.shape, self.dtype, seed, 18)] + \
               [self.t(r.normal(size=MESH), tdtype(self.dtype)) for _ in range(6)]

    def run(self, ins):
        be = self.be
        geom = ([0, 0, 0], list(MESH), [BOX] * 3)
        be.lpt_hessian(ins[0], [(0, 0), (0, 1), (1, 2)], self.h, *geom)
        be.lpt_contract(self.h, [(0, 0), (2, -1), (1, 2)], self.acc, False, *geom)
        be.lpt2_source(ins[1:], self.src, 0.5)
        return self.h + [self.acc, self.src]


def value_columns(nb, s1, first1, nmu, s2, first2):
    """the indices of the value columns of an accumulator of nb rows of s1 sums, then nb x nmu cells of s2 sums: from
    column first1 / first2 on (the counts and the sums of |x| and mu in front of them depend on the geometry alone)"""
    one = (numpy.arange(nb)[:, None] * s1 + numpy.arange(first1, s1)[None, :]).reshape(-1)
    two = nb * s1 + (numpy.arange(nb * nmu)[:, None] * s2 + numpy.arange(first2, s2)[None, :]).reshape(-1)
    return numpy.concatenate([one, two])


def power_rtol():
    """the bound of tests/test_power.py (assert_same)"""
    from tests.test_power import RTOL
    return RTOL


def power_bound(rtol, npoles, two_d):
    """assert_same's rule for the value columns [power, poles ..., power2d]: rtol |want| + rtol times the largest
    |want| of the column (the poles: (2 l + 1) times the largest |power|), doubled"""
    def f(want, ells):
        h = [host(w) for w in want]
        pscale = float(numpy.nanmax(numpy.abs(h[0]))) if numpy.isfinite(h[0]).any() else 1.0
        out = [2 * rtol * (numpy.abs(h[0]) + pscale)]
        for ell, p in zip(ells, h[1:1 + npoles]):
            out.append(2 * rtol * (numpy.abs(p) + (2 * ell + 1) * pscale))
        if two_d:
            s2 = float(numpy.nanmax(numpy.abs(h[-1]))) if numpy.isfinite(h[-1]).any() else 1.0
            out.append(2 * rtol * (numpy.abs(h[-1]) + s2))
        return out
    return f


class Power(Case):
    """power_spectrum in 1-d bins with multipoles and in (k, mu) bins.  The sums come back to the host: not
    host-asynchronous (the kernel is enqueued before that read)"""
    entries = ('pmx_power_project',)
    host_async = False

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.a, self.b = self.pm.create(type='complex'), self.pm.create(type='complex')
        kf = 2 * numpy.pi / BOX
        self.ke = numpy.arange(0.5, 28.5, 1.0) * kf
        self.me = numpy.linspace(-1, 1, 5)
        self.ells = (0, 2)
        self.dtype = dtype

    def make(self, seed):
        shape = tuple(self.a.value.shape)
        return [complex_input(self, shape, self.dtype, seed, 20), complex_input(self, shape, self.dtype, seed, 21)]

    def run(self, ins):
        from pmesh_amd.power import power_spectrum
        self.a.value.copy_(ins[0])
        self.b.value.copy_(ins[1])
        kw = dict(other=self.b, muedges=self.me, los=[0.3, -0.5, 0.8], poles=self.ells)
        r = power_spectrum(self.a, self.ke, **kw)
        return [as_tensor(r.power)] + [as_tensor(r.poles[ell]) for ell in self.ells] + [as_tensor(r.power2d)]

    def bound(self):
        rule = power_bound(power_rtol(), len(self.ells), True)
        return lambda want: rule(want, self.ells)


class PowerProject(Case):
    """pmx_power_project on a block of the caller's, with the reference and the bound of
    tests/test_spectrum_kernels.py (restate_sums)"""
    entries = ('pmx_power_project',)
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        from tests import test_spectrum_kernels as K
        self.K = K
        self.geom = ([32, 32, 17], [0, 0, 0], [32, 32, 32])
        self.ps = K.param_sets(self.geom)[1]
        self.cdt = 'c16' if dtype == 'f8' else 'c8'
        self.dtype = dtype
        self.params = K.power_params(3, self.ps)
        self.ke, self.me = K.dev_f8(be, self.ps['ke']), K.dev_f8(be, self.ps['me'])
        nk, nmu = len(self.ps['ke']) - 1, len(self.ps['me']) - 1
        s1 = 4 + 2 * len(self.ps['ells'])
        self.acc = torch.zeros(nk * s1 + nk * nmu * 5, dtype=torch.float64, device=self.dev)
        self.cols = value_columns(nk, s1, 2, nmu, 5, 3)
        self.tcols = self.t(self.cols)
        self._bound = None

    def make(self, seed):
        shape = tuple(self.geom[0])
        ins = [complex_input(self, shape, self.dtype, seed, 22), complex_input(self, shape, self.dtype, seed, 23)]
        if seed == 1 and self._bound is None:
            want, bound, counts = self.K.restate_sums(ins[0].cpu().numpy(), ins[1].cpu().numpy(), self.geom, self.ps)
            self._bound = 2 * bound[self.cols]
        return ins

    def run(self, ins):
        shape, start, nmesh = self.geom
        self.acc.zero_()
        self.be.power_project(self.params, ins[0], ins[1], start, nmesh, self.K.BOX, self.ke, self.me, self.acc)
        return [self.acc[self.tcols]]

    def written(self, outputs):
        return [self.acc]

    def bound(self):
        return lambda want: [self._bound]


class Bispectrum(Case):
    """bispectrum: the shell split, the transforms and the reduction in fixed order are deterministic
    (include/pmesh_amd.h).  The sums come back to the host (the first set is enqueued before that read)"""
    entries = ('pmx_bispec_shells', 'pmx_bispec_reduce')
    host_async = False

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.a = self.pm.create(type='complex')
        self.ke = 2 * numpy.pi / BOX * numpy.array([0.5, 2.5, 4.5, 6.5, 8.5])
        self.dtype = dtype

    def make(self, seed):
        f = self.pm.create(type='real')
        f.value.copy_(self.t(rng(seed, 24).normal(size=MESH), tdtype(self.dtype)))
        return [f.r2c().value.clone()]

    def run(self, ins):
        from pmesh_amd.bispectrum import bispectrum
        self.a.value.copy_(ins[0])
        return [as_tensor(bispectrum(self.a, self.ke, deconv_pow=2).sums)]


class Correlation(Case):
    """correlation_function: pmx_spectral_product, c2r and pmx_corr_project, all enqueued before the sums come back"""
    entries = ('pmx_spectral_product', 'pmx_corr_project')
    host_async = False

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.f = self.pm.create(type='real')
        H = BOX / 32
        self.re = numpy.arange(0.5, 16.5, 1.0) * H
        self.ells = (0, 2)
        self.dtype = dtype

    def make(self, seed):
        return [self.t(rng(seed, 26).normal(size=MESH), tdtype(self.dtype))]

    def run(self, ins):
        from pmesh_amd.correlation import correlation_function
        self.f.value.copy_(ins[0])
        c = self.f.r2c()
        r = correlation_function(c, self.re, poles=self.ells)
        return [as_tensor(r.corr)] + [as_tensor(r.poles[ell]) for ell in self.ells]

    def bound(self):
        """the rule of tests/test_correlation.py (assert_result): the difference times the count within the bound of
        ref_project on the raw sum of the bin; a pole of order l within (2 l + 1)^2 times that"""
        from pmesh_amd.correlation import correlation_field
        from tests.test_correlation import ref_project

        def f(want):
            xi = correlation_field(self.f.r2c())
            acc, b = ref_project(xi.value.cpu().numpy(), xi.start, self.pm.Nmesh, self.pm.BoxSize, self.re,
                                 ells=list(self.ells))
            nr, s1 = len(self.re) - 1, 3 + len(self.ells)
            acc, b = acc.reshape(nr, s1), b.reshape(nr, s1)
            n = numpy.maximum(acc[:, 0], 1)
            return [2 * b[:, 2] / n] + [2 * (2 * ell + 1) ** 2 * b[:, 2] / n for ell in self.ells]
        return f


class CorrEntries(Case):
    """pmx_spectral_product and pmx_corr_project on blocks of the caller's"""
    entries = ('pmx_spectral_product', 'pmx_corr_project')
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        from pmesh_amd.power import _Binning
        from pmesh_amd.correlation import CorrResult
        self.dtype = dtype
        self.shape = (32, 32, 17)
        self.prod = torch.zeros(self.shape, dtype=tdtype(dtype, True), device=self.dev)
        self.re = numpy.arange(0.5, 16.5, 1.0) * (BOX / 32)
        self.bins = _Binning(3, 'redges', self.re, numpy.linspace(-1, 1, 5), [0.3, -0.5, 0.8], (0, 2), CorrResult)
        self.acc = self.bins.zeros()
        self.cols = value_columns(len(self.re) - 1, self.bins.s1, 2, 4, self.bins.s2, 3)
        self.tcols = self.t(self.cols)
        self._bound = None

    def make(self, seed):
        r = rng(seed, 27)
        ins = [complex_input(self, self.shape, self.dtype, seed, 28), complex_input(self, self.shape, self.dtype, seed, 29),
               self.t(r.normal(size=MESH), tdtype(self.dtype))]
        if seed == 1 and self._bound is None:
            from tests.test_correlation import ref_project, unit
            _, b = ref_project(ins[2].cpu().numpy(), [0, 0, 0], MESH, [BOX] * 3, self.re, self.bins.me,
                               unit([0.3, -0.5, 0.8]), list(self.bins.ells))
            self._bound = 2 * b[self.cols]
        return ins

    def run(self, ins):
        be, b = self.be, self.bins
        be.spectral_product(ins[0], ins[1], self.prod, [0, 0, 0], list(MESH), scale=0.5, conj_y=True, deconv_pow=2)
        self.acc.zero_()
        be.corr_project(b.p, ins[2], [0, 0, 0], list(MESH), [BOX] * 3, b.et, b.mt, self.acc)
        return [self.prod, self.acc[self.tcols]]

    def written(self, outputs):
        return [self.prod, self.acc]

    def bound(self):
        return lambda want: [numpy.zeros(host(want[0]).shape), self._bound]


class Survey(Case):
    """survey_multipoles: pmx_ylm_weight, r2c, pmx_ylm_accumulate and one cross power_spectrum per order"""
    entries = ('pmx_power_project',)      # (what is enqueued before the first sums come back; the harmonic passes have
    host_async = False                    # the case Harmonics)

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.f = self.pm.create(type='real')
        self.ke = numpy.arange(0.5, 16.5, 1.0) * 2 * numpy.pi / BOX
        self.dtype = dtype

    def make(self, seed):
        return [self.t(rng(seed, 30).normal(size=MESH), tdtype(self.dtype))]

    def run(self, ins):
        from pmesh_amd.survey import survey_multipoles
        self.f.value.copy_(ins[0])
        r = survey_multipoles(self.f, self.ke, (-300., 400., -2500.))
        # (the field is real: the imaginary parts are rounding noise around 0)
        return [as_tensor(r.poles[ell].real) for ell in (0, 2, 4)]

    def bound(self):
        # every order is a multiple of the `power` of one power_spectrum call: its rule, on the scale of that order
        rule = power_bound(power_rtol(), 0, False)
        return lambda want: [rule([w], ())[0] for w in want]


class Harmonics(Case):
    """pmx_ylm_weight and pmx_ylm_accumulate on blocks of the caller's, and pmx_phase_combine: elementwise, bit for bit"""
    entries = ('pmx_ylm_weight', 'pmx_ylm_accumulate', 'pmx_phase_combine')
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.dtype = dtype
        self.cshape = (32, 32, 17)
        self.w = torch.zeros(MESH, dtype=tdtype(dtype), device=self.dev)
        self.acc = [torch.zeros(self.cshape, dtype=tdtype(dtype, True), device=self.dev) for _ in range(2)]

    def make(self, seed):
        return [self.t(rng(seed, 31).normal(size=MESH), tdtype(self.dtype)),
                complex_input(self, self.cshape, self.dtype, seed, 32), complex_input(self, self.cshape, self.dtype, seed, 33)]

    def run(self, ins):
        be = self.be
        geom = ([0, 0, 0], list(MESH), [BOX] * 3)
        be.ylm_weight(2, -1, ins[0], self.w, *geom, (-300., 400., -2500.))
        be.ylm_accumulate(4, 3, 0, ins[1], self.acc[0], *geom)
        be.ylm_accumulate(2, 0, 1, ins[2], self.acc[0], *geom)
        self.acc[1].copy_(ins[2])
        be.phase_combine(ins[1], self.acc[1], [0, 0, 0], list(MESH), (0.5, 0.5, 0.5), 0.5, 0.5, deconv_pow=2)
        return [self.w] + self.acc


# ---- particle modules ---------------------------------------------------------------------------------------------------
# Rows on the 2^-12 lattice of the unit box and weights that are multiples of 1/8: differences, squares, products and
# their sums are exact (tests/test_paircount.py: lattice_rows, dyadic_weights), so sums of them are equal bit for bit
# whatever the order.  The Python layer of every module counts the rows that are not finite on the host first: none of
# these calls is host-asynchronous.

def lattice_rows(seed, salt, n=NPART):
    return rng(seed, salt).randint(0, 4096, size=(n, 3)) / 4096.0


def dyadic(seed, salt, n=NPART):
    return rng(seed, salt).randint(1, 17, size=n) / 8.0


def unit_mesh():
    return ParticleMesh([8, 8, 8], BoxSize=[1.0, 1.0, 1.0])


class Poisson(Case):
    """poisson_sample: rate sum, counts, scan (the total is read on the host to allocate the rows) and emit.  The rates
    are multiples of 1/8: their sum is exact.  Of the rows the first HEAD are returned (every seed gives more)"""
    entries = ('pmx_poisson_rate_sum', 'pmx_poisson_count', 'pmx_poisson_scan')     # (emit follows the read: PoissonEmit)
    host_async = False
    HEAD = 180000

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.f = self.pm.create(type='real')
        self.dtype = dtype

    def make(self, seed):
        return [self.t(rng(seed, 34).randint(16, 81, size=MESH) / 8.0, tdtype(self.dtype))]

    def run(self, ins):
        from pmesh_amd.mock import poisson_sample
        self.f.value.copy_(ins[0])
        s = poisson_sample(self.f, scale=1.0, seed=23, return_cells=True)
        assert s.size >= self.HEAD, s.size
        return [s.counts.to(torch.int64), s.pos[:self.HEAD], s.cells[:self.HEAD],
                torch.tensor([s.expected], dtype=torch.float64)]


class Lognormal(Case):
    """lognormal_catalog: white noise, the tabulated transfer, c2r, the rate sum and the sampling.  Its input is the
    table of the transfer function on the device"""
    entries = ('pmx_whitenoise',)      # (it waits for the stream itself: what follows it has cases of its own)
    host_async = False
    HEAD = 60000

    def __init__(self, be):
        Case.__init__(self, be)
        from pmesh_amd.transfer import Tabulated as Tab
        self.pm = ParticleMesh(MESH, BoxSize=BOX)
        self.k = numpy.geomspace(2 * numpy.pi / BOX * 0.9, numpy.pi * 32 / BOX * 2, 24)
        self.tab = Tab(self.k, numpy.full(len(self.k), 0.01), loglog=True)

    def make(self, seed):
        # ln t of a power law whose amplitude and slope depend on the seed
        amp, slope = {1: (0.006, -0.3), 2: (0.01, -0.2)}.get(seed, (0.008, -0.25))
        return [self.t(numpy.log(amp * (self.k / self.k[0]) ** slope))]

    def run(self, ins):
        from pmesh_amd.mock import lognormal_catalog
        # (the device copy of the table, which the kernel reads: the public API takes host arrays only)
        self.tab._table(self.dev)[1].copy_(ins[0])
        cat = lognormal_catalog(self.pm, self.tab, 80000.0 / BOX ** 3, 77, bias=1.5)
        assert cat.size >= self.HEAD, cat.size
        return [cat.counts.to(torch.int64), cat.pos[:self.HEAD], cat.delta_k.value]


class FOF(Case):
    """fof and fof_catalog; per row: the smallest row of its group, and the mass and centre of its group"""
    # (the five passes are enqueued before fof reads its flag; the catalogue's sums follow it: GroupSums)
    entries = ('pmx_fof_cells', 'pmx_fof_fill', 'pmx_fof_link', 'pmx_fof_flatten', 'pmx_fof_minlabel')
    host_async = False

    def __init__(self, be):
        Case.__init__(self, be)
        self.pm = unit_mesh()

    def make(self, seed):
        return [self.t(lattice_rows(seed, 35)), self.t(dyadic(seed, 36)),
                self.t(rng(seed, 37).randint(-64, 65, size=(NPART, 3)) / 8.0)]

    def run(self, ins):
        from pmesh_amd.fof import fof, fof_catalog
        res = fof(self.pm, ins[0], 0.05, nmin=2)
        cat = fof_catalog(self.pm, ins[0], res, mass=ins[1], vel=ins[2])
        return [res.minid, cat.Mass[res.labels], cat.CMPosition[res.labels], cat.CMVelocity[res.labels]]


# The entries below are launched through the device-only layer of their modules (paircount.local_counts and its
# siblings, Backend methods): the public calls count the rows that are not finite on the host first, and a kernel
# enqueued behind such a read finds the real inputs in place on whatever stream it runs.

UNIT_BOX = [1.0, 1.0, 1.0]


class Pairs(Case):
    """pmx_pair_counts (paircount.local_counts: the cell sort and the kernel), auto with weights: npairs and wnpairs
    exact; rsum, a sum of positive terms w1 w2 sqrt(q), within the bound of tests/test_paircount.py (check): (M + 4)
    2^-52 times the sum, M the pairs of the bin"""
    entries = ('pmx_fof_cells', 'pmx_fof_fill', 'pmx_pair_counts')

    def __init__(self, be, mode):
        Case.__init__(self, be)
        from pmesh_amd.fof import cell_grid
        self.mode = mode
        edges = numpy.linspace(0.0, 0.1, 9)
        self.grid = cell_grid(NPART, 0.1, UNIT_BOX)
        self.e2 = self.t(edges * edges)
        self.sub = self.t(numpy.linspace(0.0, 1.0, 5) ** 2) if mode == '2d' else None

    def make(self, seed):
        return [self.t(lattice_rows(seed, 38)), self.t(dyadic(seed, 39))]

    def run(self, ins):
        from pmesh_amd.paircount import local_counts
        return list(local_counts(self.be, self.mode, 2, ins[0], ins[1], None, None, self.grid, UNIT_BOX, self.e2,
                                 self.sub))

    def bound(self):
        from tests.test_paircount import U

        def f(want):
            M = host(want[0]).astype('f8')                  # (the self pairs of bin (0, 0) included: the entry counts them)
            return [numpy.zeros(M.shape), numpy.zeros(M.shape), 2 * (M + 4) * U * numpy.abs(host(want[2]))]
        return f


class ThreePoint(Case):
    """pmx_threept_multipoles (threept.local_multipoles) with unit weights: npairs, zeta_0, diag and wpairs are sums of
    integers, exact (the header; tests/test_threept.py compares them by equality).  The higher orders come from the
    same launch"""
    entries = ('pmx_threept_multipoles',)

    def __init__(self, be):
        Case.__init__(self, be)
        from pmesh_amd.fof import cell_grid
        edges = numpy.array([0.02, 0.05, 0.08, 0.1])
        self.grid = cell_grid(NPART, 0.1, UNIT_BOX)
        self.e2 = self.t(edges * edges)

    def make(self, seed):
        return [self.t(lattice_rows(seed, 40))]

    def run(self, ins):
        from pmesh_amd.threept import local_multipoles
        zeta, diag, wpairs, npairs = local_multipoles(self.be, ins[0], None, None, None, self.grid, UNIT_BOX, self.e2, 2)
        return [npairs, zeta[0], diag, wpairs]


class ShortRange(Case):
    """pmx_short_range (shortrange.local_force) with potential and neighbour counts: neighbours exact; acc and pot
    within the bound of tests/test_shortrange.py (check) on the sums its restatement (force_core) returns"""
    entries = ('pmx_short_range',)
    R_SPLIT, R_CUT, SOFT = 0.02, 0.08, 0.001

    def __init__(self, be):
        Case.__init__(self, be)
        from pmesh_amd.fof import cell_grid
        self.grid = cell_grid(NPART, self.R_CUT, UNIT_BOX)
        self._ref = None

    def make(self, seed):
        ins = [self.t(rng(seed, 41).uniform(0, 1, size=(NPART, 3))), self.t(rng(seed, 42).uniform(0.5, 1.5, size=NPART))]
        if seed == 1 and self._ref is None:
            from tests.test_shortrange import ref_force
            self._ref = ref_force(ins[0].cpu().numpy(), UNIT_BOX, self.R_SPLIT, self.R_CUT,
                                  mass=ins[1].cpu().numpy(), softening=self.SOFT)
        return ins

    def run(self, ins):
        from pmesh_amd.shortrange import local_force
        return list(local_force(self.be, ins[0], None, ins[1], self.grid, UNIT_BOX, 1.0, self.R_SPLIT,
                                self.R_CUT ** 2, self.SOFT ** 2, True, True))

    def bound(self):
        from tests.test_shortrange import U, ULPS

        def f(want):
            ref = self._ref
            M = ref['neighbours'].astype('f8')
            return [2 * (M[:, None] + ULPS) * U * ref['Sacc'], 2 * (M + ULPS) * U * ref['Spot'], numpy.zeros(M.shape)]
        return f


class KNN(Case):
    """pmx_knn (knn.local_knn: one launch at a fixed radius): dist2, index and count are defined bit for bit (no ties
    among random rows)"""
    entries = ('pmx_knn',)
    RADIUS = 0.1

    def __init__(self, be):
        Case.__init__(self, be)
        from pmesh_amd.fof import cell_grid
        self.grid = cell_grid(NPART, self.RADIUS, UNIT_BOX)

    def make(self, seed):
        return [self.t(rng(seed, 43).uniform(0, 1, size=(NPART, 3)))]

    def run(self, ins):
        from pmesh_amd.knn import local_knn
        return list(local_knn(self.be, ins[0], None, self.grid, UNIT_BOX, self.RADIUS ** 2, 9, True))


class GroupSums(Case):
    """pmx_fof_group_sums on labels and reference rows of the caller's: 64 groups of lattice rows with masses and
    velocities in eighths, so every product and sum is exact"""
    entries = ('pmx_fof_group_sums',)
    NG = 64

    def __init__(self, be):
        Case.__init__(self, be)
        self.out = torch.zeros((self.NG + 1, 7), dtype=torch.float64, device=self.dev)

    def make(self, seed):
        r = rng(seed, 46)
        return [self.t(lattice_rows(seed, 47)), self.t(r.randint(0, self.NG + 1, size=NPART).astype('i8')),
                self.t(dyadic(seed, 48)), self.t(r.randint(-64, 65, size=(NPART, 3)) / 8.0),
                self.t(lattice_rows(seed, 49, self.NG + 1))]

    def run(self, ins):
        pos, labels, mass, vel, ref = ins
        self.out.zero_()
        self.be.fof_group_sums(pos, labels, mass, vel, ref, UNIT_BOX, self.out)
        return [self.out]


class PoissonEmit(Case):
    """pmx_poisson_emit on counts and segment offsets of the caller's.  Every seed permutes the same counts: the number
    of rows is the same, and the rows and cells are draws, deterministic"""
    entries = ('pmx_poisson_emit',)
    SEGMENT = 4096

    def __init__(self, be):
        Case.__init__(self, be)
        self.base = numpy.arange(int(numpy.prod(MESH))) % 7
        n = int(self.base.sum())
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=self.dev)
        self.cells = torch.zeros(n, dtype=torch.int64, device=self.dev)

    def make(self, seed):
        counts = rng(seed, 50).permutation(self.base)
        sums = counts.reshape(-1, self.SEGMENT).sum(axis=1)
        # (the counts are uint32 in the entry; int32 storage holds the same bits)
        return [self.t(counts.astype('i4')), self.t((numpy.cumsum(sums) - sums).astype('i8'))]

    def run(self, ins):
        self.be.poisson_emit(MESH, [0, 0, 0], MESH, [BOX] * 3, 23, ins[0], ins[1], self.pos, self.cells)
        return [self.pos, self.cells]


class Gradients(Case):
    """the adjoint and tangent entries on blocks of the caller's, each enqueued with nothing read back in front of it:
    pmx_power_vjp, pmx_corr_vjp, pmx_bispec_pairsum, pmx_bispec_shells_vjp and pmx_apply_ktable_jvp.  All are
    documented as deterministic.  Every edge set covers the whole block: no element is 0 whatever the inputs"""
    entries = ('pmx_power_vjp', 'pmx_corr_vjp', 'pmx_bispec_pairsum', 'pmx_bispec_shells_vjp', 'pmx_apply_ktable_jvp')
    graph = True

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        from pmesh_amd.correlation import CorrResult
        from pmesh_amd.power import _Binning
        from pmesh_amd.transfer import Tabulated as Tab
        from tests import test_spectrum_kernels as K
        self.K, self.dtype = K, dtype
        cdt, rdt = tdtype(dtype, True), tdtype(dtype)
        self.cshape = (32, 32, 17)
        self.geom = (list(self.cshape), [0, 0, 0], list(MESH))
        kmin, kmax = K.krange(self.geom)
        self.ps = dict(cross=True, ke=numpy.linspace(0, kmax * 1.0001, 13), me=K.MUEDGES,
                       los=numpy.array([0.3, -0.5, 0.8]) / numpy.sqrt(0.98), ells=(0, 2), deconv_pow=2, hermitian=True)
        self.params = K.power_params(3, self.ps)
        self.ke, self.me = K.dev_f8(be, self.ps['ke']), K.dev_f8(be, self.ps['me'])
        self.ncoef = 12 * (2 + 2 * 2) + 12 * (len(K.MUEDGES) - 1) * 2
        self.ga, self.gb, self.shell_out, self.tangent = [torch.zeros(self.cshape, dtype=cdt, device=self.dev)
                                                          for _ in range(4)]
        # the correlation binning over every separation of the mesh
        re = numpy.arange(0, 29) * (BOX / 32)
        self.bins = _Binning(3, 'redges', re, numpy.linspace(-1, 1, 5), [0.3, -0.5, 0.8], (0, 2), CorrResult)
        self.ccoef = 28 * 3 + 28 * 4
        self.g = torch.zeros(MESH, dtype=rdt, device=self.dev)
        # three shells over every mode; pair lists of the three fields
        self.kshell = K.dev_f8(be, numpy.linspace(0, kmax * 1.0001, 4))
        self.offsets = self.t(numpy.array([0, 2, 4, 6], dtype='i4'))
        self.pairs = self.t(numpy.array([[0, 0], [1, 2], [0, 1], [2, 2], [0, 2], [1, 1]], dtype='i4'))
        self.outs = [torch.zeros(MESH, dtype=rdt, device=self.dev) for _ in range(3)]
        k = numpy.geomspace(2 * numpy.pi / 120. * 0.5, 3.0, 24)
        self.tab = Tab(k, 1.0 / (1.0 + k ** 2), loglog=True, left=1.0)

    def make(self, seed):
        r = rng(seed, 51)
        f8 = torch.float64
        return [complex_input(self, self.cshape, self.dtype, seed, 52 + i) for i in range(3)] + \
               [self.t(r.normal(size=MESH), tdtype(self.dtype)) for _ in range(3)] + \
               [self.t(r.uniform(0.5, 1.5, size=self.ncoef), f8), self.t(r.uniform(0.5, 1.5, size=self.ccoef), f8),
                self.t(r.uniform(0.5, 1.5, size=6), f8), self.t(r.uniform(0.5, 1.5, size=24), f8)]

    def run(self, ins):
        be, K = self.be, self.K
        spectra, fields = ins[0:3], ins[3:6]
        coef, ccoef, weights, dy = ins[6:]
        shape, start, nmesh = self.geom
        be.power_vjp(self.params, spectra[0], spectra[1], self.ga, self.gb, start, nmesh, K.BOX, self.ke, self.me, coef)
        b = self.bins
        be.corr_vjp(b.p, self.g, [0, 0, 0], list(MESH), [BOX] * 3, b.et, b.mt, ccoef)
        be.bispec_pairsum(fields, self.outs, self.offsets, self.pairs, weights)
        be.bispec_shells_vjp(spectra, self.shell_out, start, nmesh, K.BOX, self.kshell, deconv_pow=2)
        # (the pmx_ktable struct of the table's device copy: the public apply_jvp uploads its tangent from the host)
        table = self.tab._table(self.dev)[2]
        be.apply_ktable_jvp(table, dy, spectra[2], self.tangent, start, nmesh, K.BOX)
        return [self.ga, self.gb, self.g, self.shell_out, self.tangent] + self.outs


class CorrelationField(Case):
    """correlation_field into a field of the caller's: pmx_spectral_product and c2r, asynchronous"""
    entries = ('pmx_spectral_product',)

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.pm = ParticleMesh(MESH, BoxSize=BOX, dtype=dtype)
        self.c, self.xi = self.pm.create(type='complex'), self.pm.create(type='real')
        self.dtype = dtype

    def make(self, seed):
        return [complex_input(self, tuple(self.c.value.shape), self.dtype, seed, 60)]

    def run(self, ins):
        from pmesh_amd.correlation import correlation_field
        self.c.value.copy_(ins[0])
        correlation_field(self.c, deconv_pow=2, out=self.xi)
        return [self.xi.value]


# ---- decomposition ----------------------------------------------------------------------------------------------------------

class FakeComm(object):
    """a communicator of `size` ranks with no peers: what GridND needs to lay out its domains"""
    def __init__(self, size, rank=0):
        self.size, self.rank = size, rank

    def allgather(self, x):
        return [x] * self.size

    def allreduce(self, x, op='sum'):
        return x

    def bcast(self, x):
        return x


class Decompose(Case):
    """pmx_decompose_count, then pmx_decompose_fill with the offsets of its counts (scanned on the device: no host
    read).  Without smoothing every row goes to exactly one of the 8 ranks: the index list holds every row once"""
    entries = ('pmx_decompose_count', 'pmx_decompose_fill')

    def __init__(self, be):
        Case.__init__(self, be)
        edges = [numpy.linspace(0, 8, 3)] * 3
        self.grid = domain.GridND(edges, comm=FakeComm(8))
        self.masks = torch.zeros(NROWS, dtype=torch.int64, device=self.dev)
        self.counts = torch.zeros(8, dtype=torch.int64, device=self.dev)
        self.indices = torch.zeros(NROWS, dtype=torch.int32, device=self.dev)
        self.one = numpy.ones(3)
        self.zero = numpy.zeros(3)

    def make(self, seed):
        return [self.t(rng(seed, 44).uniform(0, 8, size=(NROWS, 3)))]

    def run(self, ins):
        be = self.be
        g = self.grid._cgrid(be)            # (the pmx_grid struct: GridND.decompose reads its counts on the host)
        pv = vec(ins[0])
        be.call('decompose_count', C.byref(g), C.byref(pv), _abi.f64arr(self.one, 3), _abi.f64arr(self.zero, 3), NROWS,
                self.masks.data_ptr(), self.counts.data_ptr(), be.stream())
        offsets = torch.cumsum(self.counts, 0) - self.counts
        be.call('decompose_fill', 8, self.masks.data_ptr(), NROWS, offsets.data_ptr(), self.indices.data_ptr(), 4,
                be.stream())
        return [self.masks, self.counts, self.indices]


class Rows(Case):
    """pmx_take_rows, pmx_pack_rows and pmx_scatter_add with index arrays that the case fills itself; the values are
    multiples of 1/8: the sums of scatter_add are exact"""
    entries = ('pmx_take_rows', 'pmx_pack_rows', 'pmx_scatter_add')
    NSRC = 3001

    def __init__(self, be, dtype):
        Case.__init__(self, be)
        self.rdt = tdtype(dtype)
        self.es = 8 if dtype == 'f8' else 4
        self.taken = torch.zeros((NROWS, 3), dtype=self.rdt, device=self.dev)
        self.packed = torch.zeros((NROWS, 5), dtype=self.rdt, device=self.dev)
        self.summed = torch.zeros((self.NSRC, 3), dtype=self.rdt, device=self.dev)

    def make(self, seed):
        r = rng(seed, 45)
        return [self.t(r.randint(-64, 65, size=(self.NSRC, 3)) / 8.0, self.rdt),
                self.t(r.randint(0, self.NSRC, size=NROWS).astype('i4')),
                self.t(r.randint(-64, 65, size=(NROWS, 3)) / 8.0, self.rdt)]

    def run(self, ins):
        be, es = self.be, self.es
        src, idx, vals = ins
        be.call('take_rows', src.data_ptr(), 3 * es, 3 * es, idx.data_ptr(), 4, NROWS, self.taken.data_ptr(),
                be.stream())
        self.packed.zero_()
        be.call('pack_rows', src.data_ptr(), 3 * es, 3 * es, idx.data_ptr(), 4, NROWS,
                self.packed.data_ptr() + es, 5 * es, be.stream())
        be.call('scatter_add', vals.data_ptr(), es, 3, idx.data_ptr(), 4, NROWS, self.summed.data_ptr(), self.NSRC,
                be.stream())
        return [self.taken, self.packed, self.summed]


# ---- the table ------------------------------------------------------------------------------------------------------------------

def _table():
    """(name, class, arguments) of every case; the attributes host_async and graph are the class's"""
    T = []

    def add(name, cls, *args, **kw):
        T.append((name, cls, args, kw))
    for dt in ('f8', 'f4'):
        for kind in ('cic', 'tsc', 'pcs'):
            add('paint-tile-%s-%s' % (kind, dt), Paint, kind, dt)
            add('readout-tile-%s-%s' % (kind, dt), Readout, kind, dt)
        add('paint-tile-mass-%s' % dt, Paint, 'cic', dt, mass=True)
        add('paint-tile-gradient-%s' % dt, Paint, 'tsc', dt, gradient=1)
        add('paint-tile-deterministic-%s' % dt, Paint, 'pcs', dt, mass=True, deterministic=True)
        add('readout-tile-gradient-%s' % dt, Readout, 'tsc', dt, gradient=2)
        add('readout-many-%s' % dt, Readout, 'cic', dt, many=True)
        for kind in ('quadratic', 'lanczos2'):
            add('paint-direct-%s-%s' % (kind, dt), Paint, kind, dt, path='direct', mass=True)
            add('readout-direct-%s-%s' % (kind, dt), Readout, kind, dt, path='direct')
        add('paint-interlaced-%s' % dt, Interlaced, dt)
        add('paint-deferred-%s' % dt, DeferredPaint, dt)
        add('fft-own-%s' % dt, FFT, dt, OWN)
        add('fft-rocfft-%s' % dt, FFT, dt, MESH)
        add('apply-transfer-%s' % dt, ApplyTransfer, dt)
        add('tabulated-apply-%s' % dt, Tabulated, dt, vjp=False)
        add('tabulated-vjp-%s' % dt, Tabulated, dt)
        add('whitenoise-%s' % dt, WhiteNoise, dt)
        add('pm-cycle-%s' % dt, PMCycle, dt)
        for which in ('col', 'row', 'split', 'rowsplit', 'chunk', 'pack'):
            add('pass-%s-%s' % (which, dt), Passes, dt, which)
        for what in ('lpt1', 'lpt2', 'vjp', 'jvp'):
            add('lpt-%s-%s' % (what, dt), LPT, dt, what)
        add('lpt-entries-%s' % dt, LPTEntries, dt)
        add('power-%s' % dt, Power, dt)
        add('power-project-%s' % dt, PowerProject, dt)
        add('bispectrum-%s' % dt, Bispectrum, dt)
        add('correlation-%s' % dt, Correlation, dt)
        add('corr-entries-%s' % dt, CorrEntries, dt)
        add('correlation-field-%s' % dt, CorrelationField, dt)
        add('gradients-%s' % dt, Gradients, dt)
        add('survey-%s' % dt, Survey, dt)
        add('harmonics-%s' % dt, Harmonics, dt)
        add('poisson-%s' % dt, Poisson, dt)
        add('rows-%s' % dt, Rows, dt)
    # 2^16 rows and more in no order: the builds that measure the coherence of the rows and keep a tile-ordered copy
    add('paint-tile-70000-rows', Paint, 'cic', 'f8', rows=70000)
    add('readout-tile-70000-rows', Readout, 'cic', 'f8', rows=70000)
    add('tile-order', TileOrder)
    add('paint-readout-4d', PaintReadoutND)
    add('synth', Synth)
    add('lognormal', Lognormal)
    add('fof', FOF)
    add('group-sums', GroupSums)
    add('poisson-emit', PoissonEmit)
    add('pairs-1d', Pairs, '1d')
    add('pairs-2d', Pairs, '2d')
    add('threept', ThreePoint)
    add('short-range', ShortRange)
    add('knn', KNN)
    add('decompose', Decompose)
    return T


TABLE = _table()
NAMES = [row[0] for row in TABLE]
GRAPH_NAMES = [row[0] for row in TABLE if row[1].graph]


def build(name, be):
    """the case `name` on the backend `be`"""
    _, cls, args, kw = TABLE[NAMES.index(name)]
    case = cls(be, *args, **kw)
    case.name = name
    return case
