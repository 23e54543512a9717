"""Domain decomposition: the host-side mirror of ``pmesh/domain.py``.

``GridND.decompose`` and ``Layout.exchange`` / ``Layout.gather`` keep the
reference's signatures and results (pmesh/domain.py:82-318, 320-652): the same
``sendcounts`` and the same rank-major, index-ascending ``indices``; ghosts are
created for every domain within ``smoothing`` of a particle and reduced on the
way back.  What changes is where the work happens:

* the classification (numpy in 49152-row chunks, domain.py:605-630) and the two
  serial ``gridnd_fill`` passes (pmesh/_domain.pyx:9-122) are HIP kernels
  (csrc/pmx_domain.hip) working on device-resident positions;
* ``take`` + ``Alltoallv`` (domain.py:188-202) is a gather kernel followed by an
  RCCL all-to-all-v on device buffers, no host staging, no Barriers;
* the ghost reduction (bincountv, domain.py:26-48) is a scatter-add kernel.

Counts and indices are int32 as in the reference while they fit, int64 beyond
2^31 particles per rank (the reference asserts there, domain.py:590).
"""
import ctypes as C
import weakref

import numpy
import torch

from . import _abi, backend
from ._arrays import touched, to_device, vec, is_tensor, torch_dtype, numpy_dtype, to_numpy, version_of
from .comm import default_comm


def bincountv(x, weights, minlength=None, dtype=None, out=None):
    """ bincount with vector weights (domain.py:26-48), on the device. """
    be = backend.get()
    x, _ = to_device(x, be.device, 'x', allow_int=True)
    w, host = to_device(weights, be.device, 'weights')
    if minlength is None:
        minlength = int(x.max()) + 1 if x.numel() else 0
    r = _scatter_add(be, w, x, int(minlength))
    if dtype is not None:
        r = r.to(torch_dtype(dtype))
    if out is not None:
        if is_tensor(out):
            out.copy_(r)
        else:
            to_numpy(r, out=out)
        return out
    return to_numpy(r) if host else r


def _scatter_add(be, values, indices, nout):
    values = values.contiguous()
    indices = indices.contiguous()
    if indices.dtype not in (torch.int32, torch.int64):
        indices = indices.to(torch.int64)
    ncol = 1
    for s in values.shape[1:]:
        ncol *= s
    if values.dtype not in (torch.float32, torch.float64):
        # pmx_scatter_add adds float / double bit patterns; integer (and any other) payloads are
        # reduced by torch's index_add_, as the reference's bincountv does for them
        # (domain.py:30-47): exact, order independent
        if values.dtype == torch.bool or values.is_complex():
            raise TypeError('cannot sum rows of dtype %s' % (values.dtype,))
        out = torch.zeros((nout,) + tuple(values.shape[1:]), dtype=values.dtype, device=be.device)
        out.index_add_(0, indices.to(torch.int64), values)
        return out
    out = torch.empty((nout,) + tuple(values.shape[1:]), dtype=values.dtype, device=be.device)
    be.call('scatter_add', values.data_ptr(), values.element_size(), ncol, indices.data_ptr(),
            indices.element_size(), values.shape[0], out.data_ptr(), nout, be.stream())
    return out


#: 'collective' (the reference, domain.py:50-57): every Layout.exchange / gather first broadcasts the
#: root's dtype and trailing shape (one small object broadcast instead of the reference's two);
#: 'static': the caller guarantees that all ranks pass the same dtype and shape, nothing is sent.
#: The ghosts-only routing of ParticleMesh.paint / readout (Layout.exchange_remote) never promotes:
#: it ships the caller's position / mass tensors, whose types the ranks share by construction.
PROMOTE = 'collective'


def promote(data, comm):
    """domain.py:50-57: every rank adopts the dtype of the root's array (e.g. an empty rank whose
    array came out with a default dtype); a trailing shape that differs from the root's raises
    ValueError on the ranks where it differs."""
    if getattr(comm, 'size', 1) == 1 or PROMOTE != 'collective':
        return data
    if not (is_tensor(data) or isinstance(data, numpy.ndarray)):
        data = numpy.asarray(data)
    name = numpy_dtype(data.dtype).str if is_tensor(data) else data.dtype.str
    sig = (name, tuple(int(x) for x in data.shape[1:]))
    root = comm.bcast(sig)
    if root[0] != sig[0]:
        data = data.to(torch_dtype(numpy.dtype(root[0]))) if is_tensor(data) else data.astype(root[0])
    if tuple(root[1]) != sig[1]:
        raise ValueError('the shape of the data does not match across ranks.')
    return data


def pack_arrays(seq):
    """
    Copy a sequence of host arrays of equal length into one structured array, one field per
    array, each field keeping the trailing shape of its column (domain.py:59-80; what
    Layout.exchange(pack=True) ships in the reference; here the device rows are packed as bytes,
    Layout._exchange_packed).
    """
    cols = [numpy.asarray(a) for a in seq]
    lengths = set(c.shape[0] for c in cols)
    if len(lengths) > 1:
        raise ValueError('the shape of the data does not match across different columns.')
    dt = numpy.dtype([('', (c.dtype, c.shape[1:])) for c in cols])
    out = numpy.empty(lengths.pop() if lengths else 0, dtype=dt)
    for name, c in zip(dt.names, cols):
        out[name] = c
    return out


#: An exchange whose rows add up to this many bytes or more sends its arrays ONE BY ONE, each straight from its
#: gathered rows into the tensor the caller receives (no packed copy on either side: the packing exists to save
#: collectives, and a collective of hundreds of megabytes is not latency bound); below it the arrays of
#: exchange(pack=True) / exchange_remote travel packed side by side in one all-to-all-v.
PACK_BYTES_MAX = 256 << 20


class _Scratch(object):
    """Send / receive staging of the exchanges of one communicator (held on the communicator object: a rank has
    one, a thread rank of the tests its own).  The reference keeps one send and one receive buffer per call
    (domain.py:185-206); a time-stepping caller builds a new Layout every step, so the buffers outlive the
    layouts: sized from what the previous steps needed plus a quarter, reused, never shrunk.  A buffer that an
    asynchronous exchange is still reading or writing is waited for before it is handed out again."""

    def __init__(self):
        self.buffers = {}      # name -> [uint8 tensor, handle of the exchange that uses it or None]
        self.private = {}      # name -> whether the last get() handed out memory of the caller's own

    def get(self, name, nbytes, device):
        e = self.buffers.get(name)
        self.private[name] = False
        if e is not None and isinstance(e[1], _InUse) and not e[1].released:
            # the consumer of what an asynchronous exchange left in this buffer has not run yet (received rows whose
            # columns are still to be extracted, results still to be added): this exchange gets memory of its own
            self.private[name] = True
            return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        if e is not None and e[1] is not None:
            e[1].wait()
            e[1] = None
        if e is None or e[0].numel() < nbytes or e[0].device != device:
            if e is not None:
                e[0] = None                      # (free before the larger one is made)
            # a quarter of slack for what the next steps may need, at most 64 MB of it (ghost counts of a time-stepping
            # caller wander by per cents; a buffer of gigabytes must not cost another quarter of itself)
            slack = min(int(nbytes) // 4, 64 << 20) + 256
            e = self.buffers[name] = [torch.empty(int(nbytes) + slack, dtype=torch.uint8, device=device), None]
        return e[0][:nbytes]

    def busy(self, name, work):
        # (an exchange that was given memory of its own has nothing of the pool to protect — and the hold of the
        # exchange that still owns the pooled buffer must stay: replaced by this one's, a THIRD exchange would be
        # handed the buffer the first has not read yet)
        if work is None or name not in self.buffers or self.private.get(name):
            return
        e = self.buffers[name]
        if isinstance(e[1], _InUse) and not e[1].released and e[1] is not work:
            return
        e[1] = work

    def nbytes(self):
        return sum(e[0].numel() for e in self.buffers.values() if e[0] is not None)

    def clear(self):
        """give the staging back (after a one-off exchange much larger than what the steps that follow need: the
        migration of every particle to its owner)"""
        for e in self.buffers.values():
            if e[1] is not None:
                e[1].wait()
        self.buffers = {}


class _InUse(object):
    """what _Scratch.busy() remembers for a buffer whose CONSUMER must have run before it is reused: the handle of the
    exchange (waited for as before) and whether the consumer — enqueued on the stream every later use is enqueued
    on — has been issued."""

    def __init__(self, work):
        self.work, self.released = work, False

    def wait(self):
        if self.work is not None:
            self.work.wait()

    def release(self):
        self.released = True


def release_staging(comm):
    """free the exchange staging of `comm` (it is rebuilt at the size the next exchanges need)"""
    s = getattr(comm, '_pmx_scratch', None)
    if s is not None:
        s.clear()


def _scratch_of(comm):
    s = getattr(comm, '_pmx_scratch', None)
    if s is None:
        s = comm._pmx_scratch = _Scratch()
    return s


def _row_bytes(t):
    rb = t.element_size()
    for n in t.shape[1:]:
        rb *= n
    return rb


def _typed(buf, dtype, shape):
    """a contiguous byte buffer as a tensor of `dtype` and `shape` (views only)"""
    return buf.view(dtype).reshape(shape)


class Layout(object):
    """
    The communication layout of a domain decomposition (domain.py:82-318).

    Do not create a Layout object directly. Always use :py:meth:`GridND.decompose`.
    Useful methods are :py:meth:`exchange`, and :py:meth:`gather`.
    """
    def __init__(self, comm, sendlength, sendcounts, indices, recvcounts=None):
        self.comm = comm
        assert self.comm.size == len(sendcounts)
        self.sendcounts = numpy.array(sendcounts, order='C')
        if recvcounts is None:
            # ! Alltoall (domain.py:113), without the Barriers.  The counts take the type of this rank's own while
            # they fit it: a count of 2^31 or more, sent by a rank with more particles, arrives as int64
            rc = numpy.asarray(self.comm.alltoall_counts(self.sendcounts))
            if self.sendcounts.dtype == numpy.int32 and len(rc) and int(rc.max()) >= 2 ** 31:
                self.recvcounts = rc.astype('i8')
            else:
                self.recvcounts = rc.astype(self.sendcounts.dtype)
        else:
            self.recvcounts = numpy.array(recvcounts, order='C')
        # offsets are int64 whatever the counts: int32 counts add up past 2^31 (ghosts; the rows a rank receives)
        self.sendoffsets = numpy.zeros(len(self.sendcounts), dtype='i8')
        self.recvoffsets = numpy.zeros(len(self.recvcounts), dtype='i8')
        self.sendoffsets[1:] = numpy.cumsum(self.sendcounts, dtype='i8')[:-1]
        self.recvoffsets[1:] = numpy.cumsum(self.recvcounts, dtype='i8')[:-1]
        self.sendlength = sendlength
        self.recvlength = int(self.recvcounts.sum())
        # device tensor, int32/int64 — or a callable that makes it the first time somebody asks (the identity
        # layout of one periodic domain on one rank: paint and readout never read it)
        self._indices = indices
        self._agreed = set()       # directions whose length check has been held collectively

    @property
    def indices(self):
        if callable(self._indices):
            self._indices = self._indices()
        return self._indices

    @indices.setter
    def indices(self, value):
        self._indices = value

    def _wrong_length(self, n, expected, direction, message):
        """The reference allgathers the verdict of the length check on every call, so that every
        rank raises (domain.py:177-179, 240-242).  Here the ranks agree on it collectively the
        first time a layout is used in a direction (one integer all-reduce) — a wrong array then
        raises ValueError everywhere, as in the reference.  Later calls check locally and return
        True on a mismatch: the caller then takes part in the exchange with rows of zeros before
        it raises, so the other ranks are never left waiting in the all-to-all."""
        bad = int(n) != int(expected)
        if self.comm.size > 1 and direction not in self._agreed:
            self._agreed.add(direction)
            if int(self.comm.allreduce(int(bad), op='max')):
                raise ValueError(message)
            return False
        if bad and self.comm.size == 1:
            raise ValueError(message)
        return bad

    def get_exchange_cost(self):
        """ exchange cost per rank: items sent to any other rank (domain.py:125-136). """
        mask = numpy.arange(self.comm.size) != self.comm.rank
        sendcount = int(numpy.sum(self.sendcounts[mask]))
        return numpy.array(self.comm.allgather(sendcount))

    def exchange(self, *args, pack=True):
        """
        Delievers data to the intersecting domains (domain.py:138-171).

        Every data item shall have the length and ordering of the positions that built the
        layout.  Ghosts are created if a particle intersects multiple domains.  pack=True (the
        default, as in the reference): the rows of all arrays travel in ONE all-to-all-v, packed
        side by side as bytes; pack=False: one exchange per array.
        """
        if not args:
            return None
        if len(args) == 1:
            return self._exchange(args[0])
        if pack and self.comm.size > 1:
            return self._exchange_packed(args)
        return tuple(self._exchange(a) for a in args)

    def _exchange(self, data):
        be = backend.get()
        # The PM cycle routes the same positions before paint and before every readout
        # (pm.py:1859, 784): remember the last exchanged device array and hand it back while
        # the source tensor is unchanged (same storage, same version counter).
        memo_key = None
        if is_tensor(data) and data.device == be.device:
            memo_key = (data.data_ptr(), version_of(data), tuple(data.shape), data.stride(), data.dtype)
            memo = getattr(self, '_memo', None)
            if memo is not None and memo[0] == memo_key:
                return memo[2]
        r = self._exchange_impl(be, data)
        if memo_key is not None:
            self._memo = (memo_key, data, r)
        return r

    def forget(self):
        """drop the remembered result of the last exchange: for a caller that exchanges new values every round from
        tensors that may share an address (all empty tensors do)"""
        self._memo = None

    def _exchange_packed(self, args):
        """exchange(pack=True): the gathered rows of every array side by side in one byte row per
        item, one all-to-all-v for all of them (domain.py:161-166, pack_arrays).  Every column is gathered
        straight into its place in the packed rows (pmx_pack_rows) of a reused send buffer; large exchanges go
        array by array instead (PACK_BYTES_MAX)."""
        be = backend.get()
        cols, hosts = [], []
        message = 'the length of data does not match that used to build the layout'
        for a in args:
            a = promote(a, self.comm)
            t, host = to_device(a, be.device, 'data', allow_int=True)
            cols.append(t)
            hosts.append(host)
        if len(set(len(t) for t in cols)) > 1:
            raise ValueError('the shape of the data does not match across different columns.')
        wrong = self._wrong_length(len(cols[0]), self.sendlength, 'exchange', message)
        if wrong:
            cols = [torch.zeros((self.sendlength,) + tuple(t.shape[1:]), dtype=t.dtype, device=be.device) for t in cols]
        nsend = int(self.sendcounts.sum())
        width = sum(_row_bytes(t) for t in cols)
        if max(nsend, self.recvlength) * width >= PACK_BYTES_MAX:
            out = []
            for t, host in zip(cols, hosts):
                r = self._exchange_impl(be, t, checked=True)
                out.append(to_numpy(r) if host else r)
            if wrong:
                raise ValueError(message)
            return tuple(out)
        scratch = _scratch_of(self.comm)
        packed = scratch.get('send', nsend * width, be.device).view(nsend, width)
        off = 0
        for t in cols:
            self._take(be, t, self.indices, nsend, out=packed, out_offset=off)
            off += _row_bytes(t)
        recv = scratch.get('recv', self.recvlength * width, be.device).view(self.recvlength, width)
        self.comm.alltoallv(packed, self.sendcounts, recv, self.recvcounts)
        if wrong:
            raise ValueError(message)
        out, off = [], 0
        for t, host in zip(cols, hosts):
            rb = _row_bytes(t)
            r = self._column(be, recv, off, rb, t.dtype, tuple(t.shape[1:]))
            off += rb
            out.append(to_numpy(r) if host else r)
        return tuple(out)

    @staticmethod
    def _column(be, packed, offset, row_bytes, dtype, trailing):
        """the column at byte `offset` of packed rows as a dense tensor of its own"""
        n = packed.shape[0]
        r = torch.empty((n,) + trailing, dtype=dtype, device=packed.device)
        if n:
            be.call('pack_rows', packed.data_ptr() + offset, packed.shape[1], row_bytes, None, 4, n,
                    r.data_ptr(), row_bytes, be.stream())
        return r

    @staticmethod
    def _take(be, data, indices, nrows, out=None, out_offset=0):
        """rows `indices` of data, contiguous (data.take(indices, axis=0), domain.py:188) — or, with `out` (packed
        byte rows, (nrows, width) uint8), written as the column at byte `out_offset` of those rows"""
        trailing = tuple(data.shape[1:])
        row_bytes = _row_bytes(data)
        if data.dim() > 1 and not data[0:1].is_contiguous() and data.shape[0] > 0:
            data = data.contiguous()
        if nrows and row_bytes % 4:
            raise TypeError('rows must be a multiple of 4 bytes')
        stride0 = data.stride(0) * data.element_size() if data.shape[0] > 1 else row_bytes
        if out is not None:
            if nrows:
                be.call('pack_rows', data.data_ptr(), stride0, row_bytes, indices.data_ptr(), indices.element_size(),
                        nrows, out.data_ptr() + out_offset, out.shape[1], be.stream())
            return out
        buffer = torch.empty((nrows,) + trailing, dtype=data.dtype, device=be.device)
        if nrows:
            be.call('take_rows', data.data_ptr(), stride0, row_bytes, indices.data_ptr(),
                    indices.element_size(), nrows, buffer.data_ptr(), be.stream())
        return buffer

    def _exchange_impl(self, be, data, checked=False):
        message = 'the length of data does not match that used to build the layout'
        wrong = False
        host = False
        if not checked:
            data = promote(data, self.comm)
            data, host = to_device(data, be.device, 'data', allow_int=True)
            wrong = self._wrong_length(len(data), self.sendlength, 'exchange', message)
            if wrong:
                data = torch.zeros((self.sendlength,) + tuple(data.shape[1:]), dtype=data.dtype, device=be.device)
        trailing = tuple(data.shape[1:])
        nsend = int(self.sendcounts.sum())
        if self.comm.size == 1:
            recvbuffer = self._take(be, data, self.indices, nsend)
        else:
            # the gathered rows live in the communicator's send buffer (reused from call to call, domain.py:185-190)
            rb = _row_bytes(data)
            send = _scratch_of(self.comm).get('send', nsend * rb, be.device).view(nsend, rb)
            self._take(be, data, self.indices, nsend, out=send)
            recvbuffer = torch.empty((self.recvlength,) + trailing, dtype=data.dtype, device=be.device)
            self.comm.alltoallv(_typed(send, data.dtype, (nsend,) + trailing), self.sendcounts, recvbuffer, self.recvcounts)
        if wrong:
            raise ValueError(message)
        return to_numpy(recvbuffer) if host else recvbuffer

    # ---- ghosts-only routing --------------------------------------------------------
    # The rows a rank sends to itself are usually almost all of them (particles live on the
    # rank that owns their cells; only the ghosts within the smoothing length of a domain
    # face and the migrating few travel).  paint/readout with a layout therefore work on the
    # caller's own array in place and exchange only the rows bound for *other* ranks; the
    # two methods below are that remote half of exchange()/gather(mode='sum').
    def _remote(self, be):
        rem = getattr(self, '_remote_tables', None)
        if rem is None:
            r = self.comm.rank
            s0 = int(self.sendoffsets[r])
            s1 = s0 + int(self.sendcounts[r])
            idx = torch.cat([self.indices[:s0], self.indices[s1:]]) if s1 > s0 else self.indices
            sc = self.sendcounts.copy()
            rc = self.recvcounts.copy()
            sc[r] = 0
            rc[r] = 0
            rem = self._remote_tables = (idx.contiguous(), sc, rc, int(sc.sum()), int(rc.sum()))
        return rem

    @property
    def remote_recvlength(self):
        return self._remote(backend.get())[4]

    def exchange_remote(self, data, *more, async_op=False):
        """ rows of `data` received from the other ranks (ordered by source rank).  Several arrays
        (positions and per-particle masses of a paint) travel side by side in ONE all-to-all-v, as
        Layout.exchange(pack=True) sends them; results are remembered per source tensor, so the
        readouts that follow a paint find the positions already exchanged.  async_op: returns a handle
        whose wait() gives the arrays — the exchange then runs (on RCCL's stream) under whatever the
        caller enqueues in between: the paint of its own particles. """
        state = self._exchange_remote_begin((data,) + more, async_op)
        if async_op:
            return _RemoteExchange(self, state)
        return self._exchange_remote_end(state)

    def _exchange_remote_begin(self, arrays_in, async_op):
        be = backend.get()
        idx, sc, rc, nsend, nrecv = self._remote(be)
        arrays = [to_device(a, be.device, 'data', allow_int=True)[0] for a in arrays_in]
        keys = [(a.data_ptr(), version_of(a), tuple(a.shape), a.stride(), a.dtype) for a in arrays]
        memo = getattr(self, '_memo_remote', None)
        if not isinstance(memo, dict):
            memo = self._memo_remote = {}
        missing = [i for i, k in enumerate(keys) if k not in memo or memo[k][0]() is not arrays[i]]
        st = dict(arrays=arrays, keys=keys, memo=memo, missing=missing, many=len(arrays_in) > 1, works=[], wrong=False)
        if not missing:
            return st
        message = 'the length of data does not match that used to build the layout'
        wrong = False
        for i in missing:
            wrong = self._wrong_length(len(arrays[i]), self.sendlength, 'exchange', message) or wrong
        src = []
        for i in missing:
            a = arrays[i]
            if wrong:
                a = torch.zeros((self.sendlength,) + tuple(a.shape[1:]), dtype=a.dtype, device=be.device)
            src.append(a)
        width = sum(_row_bytes(a) for a in src)
        scratch = _scratch_of(self.comm)
        got = []
        if len(src) == 1 or max(nsend, nrecv) * width >= PACK_BYTES_MAX:
            # array by array, each from the communicator's send buffer straight into the tensor the kernels will
            # read (the received rows are kept — the readouts after a paint find them — so that tensor has to exist
            # anyway; nothing else is allocated)
            for k, a in enumerate(src):
                rb = _row_bytes(a)
                name = 'send%d' % k
                send = scratch.get(name, nsend * rb, be.device).view(nsend, rb)
                self._take(be, a, idx, nsend, out=send)
                recv = torch.empty((nrecv,) + tuple(a.shape[1:]), dtype=a.dtype, device=be.device)
                if self.comm.size > 1:
                    w = self.comm.alltoallv(_typed(send, a.dtype, (nsend,) + tuple(a.shape[1:])), sc, recv, rc, async_op=async_op)
                    st['works'].append(w)
                    scratch.busy(name, w)
                got.append(recv)
            st.update(packed=None)
        else:
            send = scratch.get('send0', nsend * width, be.device).view(nsend, width)
            off = 0
            for a in src:
                self._take(be, a, idx, nsend, out=send, out_offset=off)
                off += _row_bytes(a)
            recv = scratch.get('recv', nrecv * width, be.device).view(nrecv, width)
            if self.comm.size > 1:
                w = self.comm.alltoallv(send, sc, recv, rc, async_op=async_op)
                st['works'].append(w)
                scratch.busy('send0', w)
                if async_op:
                    # the received rows stay in the communicator's buffer until _exchange_remote_end has taken the
                    # columns out of them: no other exchange may receive into it in between
                    st['hold'] = _InUse(w)
                    scratch.busy('recv', st['hold'])
            st.update(packed=recv)
        st.update(wrong=wrong, message=message, src=src, got=got, nrecv=nrecv)
        return st

    def _exchange_remote_end(self, st):
        memo, keys = st['memo'], st['keys']
        if st['missing']:
            be = backend.get()
            got = st['got']
            try:
                for w in st['works']:
                    if w is not None:
                        w.wait()
                if st['wrong']:
                    raise ValueError(st['message'])
                if st['packed'] is not None:
                    off = 0
                    for a in st['src']:
                        rb = _row_bytes(a)
                        got.append(self._column(be, st['packed'], off, rb, a.dtype, tuple(a.shape[1:])))
                        off += rb
            finally:
                # (also when the lengths were wrong: a hold never released would make every later exchange
                # allocate memory of its own)
                _drop_hold(st.get('hold'))
            for i, r in zip(st['missing'], got):
                # (a weak reference to the source tensor: the memo must not keep a caller's array alive, and an
                # address reused by another tensor must not pass for the old one)
                try:
                    ref = weakref.ref(st['arrays'][i])
                except TypeError:
                    ref = (lambda t: (lambda: t))(st['arrays'][i])
                memo[keys[i]] = (ref, r)
            # ONE received set per source tensor, and no more than the arrays of this call plus what is small:
            # received rows of earlier position sets are dropped first (they are the caller's old time steps)
            current = set(keys)
            budget = max(PACK_BYTES_MAX, sum(memo[k][1].numel() * memo[k][1].element_size() for k in current if k in memo))
            def held():
                return sum(v[1].numel() * v[1].element_size() for v in memo.values())
            for k in list(memo):
                if k in current:
                    continue
                if memo[k][0]() is None or len(memo) > 4 or held() > budget:
                    memo.pop(k)
            st['missing'] = []
        for k in [k for k, v in memo.items() if v[0]() is None]:
            memo.pop(k)                            # (rows received for a tensor that no longer exists)
        res = []
        for i, k in enumerate(keys):
            ref, r = memo[k]
            res.append(r)
        return tuple(res) if st['many'] else res[0]

    def gather_remote_add(self, data, out, async_op=False):
        """ send the per-ghost results `data` (rows as exchange_remote delivered them) back to
        their owners and add them into `out` (one row per original item) in place.  async_op: returns a
        handle; the results travel while the caller reads out its own particles, wait() adds them. """
        be = backend.get()
        idx, sc, rc, nsend, nrecv = self._remote(be)
        message = 'the length of data does not match result of exchange_remote'
        wrong = self._wrong_length(len(data), nrecv, 'gather_remote', message)
        if self.comm.size == 1:
            return _Finished(out) if async_op else out
        if wrong:
            data = torch.zeros((nrecv,) + tuple(data.shape[1:]), dtype=data.dtype, device=be.device)
        data = data.contiguous()
        scratch = _scratch_of(self.comm)
        # (the buffer the rows were sent FROM takes what comes back for them: the outward exchange is long over —
        # get() waits for it if not — and the results are never wider than the positions)
        back = _typed(scratch.get('send0', nsend * _row_bytes(data), be.device), data.dtype, (nsend,) + tuple(data.shape[1:]))
        work = self.comm.alltoallv(data, rc, back, sc, async_op=async_op)
        # (async: what comes back lives in 'send0' until finish() has added it — a second exchange before wait(out)
        # must not gather its rows into the same buffer)
        hold = _InUse(work) if async_op else work
        scratch.busy('send0', hold)

        def finish(target):
            if work is not None:
                work.wait()
            try:
                if wrong:
                    raise ValueError(message)
                if nsend:
                    b = back if back.dtype == target.dtype else back.to(target.dtype)
                    ncol = 1
                    for s in b.shape[1:]:
                        ncol *= s
                    # nout = 0: accumulate into `out` without clearing it (include/pmesh_amd.h).  pmx_scatter_add
                    # writes a DENSE out (out[i * ncol + c]): a strided target — a column F[:, d] of a force array —
                    # and the integer payloads take torch's strided index_add_
                    if target.dtype not in (torch.float32, torch.float64) or not target.is_contiguous():
                        target.index_add_(0, idx.to(torch.int64), b)
                        return target
                    be.call('scatter_add', b.data_ptr(), b.element_size(), ncol, idx.data_ptr(),
                            idx.element_size(), nsend, target.data_ptr(), 0, be.stream())
                    touched(target)
                return target
            finally:
                if async_op:
                    hold.release()
        if async_op:
            return _Pending2(finish, data, hold)
        return finish(out)

    def gather(self, data, mode='sum', out=None):
        """
        Pull the data from other ranks back to its original hosting rank (domain.py:208-318).

        mode : 'sum', 'any', 'mean', 'all', 'local', 'min'
            'all' returns all results, local and ghosts, without any reduction;
            'sum' reduces the ghosts to the local with sum; 'local' keeps only the local
            copy; 'any' uses any one of local or ghost; 'mean' the mean over copies;
            'min' the minimum over copies, on the device (what mode=numpy.minimum computes
            through the host: the label merge of pmesh_amd.fof).
        """
        be = backend.get()
        data = promote(data, self.comm)
        data, host = to_device(data, be.device, 'data', allow_int=True)
        message = 'the length of data does not match result of a domain.exchange'
        wrong = self._wrong_length(len(data), self.recvlength, 'gather', message)
        if wrong:
            if mode == 'local':
                raise ValueError(message)              # no communication in this mode
            data = torch.zeros((self.recvlength,) + tuple(data.shape[1:]), dtype=data.dtype, device=be.device)
        trailing = tuple(data.shape[1:])

        def finish(r):
            if out is not None:
                if is_tensor(out):
                    out.copy_(r)
                else:
                    to_numpy(r, out=out)
                return out
            return to_numpy(r) if host else r

        if mode == 'local':
            res = torch.empty((self.sendlength,) + trailing, dtype=data.dtype, device=be.device)
            start2 = int(self.sendoffsets[self.comm.rank])
            end2 = start2 + int(self.sendcounts[self.comm.rank])
            ind = self.indices[start2:end2].to(torch.int64)
            start1 = int(self.recvoffsets[self.comm.rank])
            end1 = start1 + int(self.recvcounts[self.comm.rank])
            res[ind] = data[start1:end1]
            return finish(res)

        data = data.contiguous()
        if self.comm.size == 1:
            recvbuffer = data
        else:
            recvbuffer = torch.empty((len(self.indices),) + trailing, dtype=data.dtype, device=be.device)
            self.comm.alltoallv(data, self.recvcounts, recvbuffer, self.sendcounts)
        if wrong:
            raise ValueError(message)

        if self.sendlength == 0:
            return finish(torch.empty((0,) + trailing, dtype=data.dtype, device=be.device))
        if mode == 'all':
            return finish(recvbuffer)
        if mode == 'sum':
            return finish(_scatter_add(be, recvbuffer, self.indices, self.sendlength))
        if mode == 'mean':
            s = _scatter_add(be, recvbuffer, self.indices, self.sendlength)
            ones = torch.ones(len(self.indices), dtype=torch.float64, device=be.device)
            N = _scatter_add(be, ones, self.indices, self.sendlength)
            N = N.reshape([self.sendlength] + [1] * (recvbuffer.dim() - 1))
            return finish((s / N).to(s.dtype))
        if mode == 'any':
            res = torch.zeros((self.sendlength,) + trailing, dtype=data.dtype, device=be.device)
            res[self.indices.to(torch.int64)] = recvbuffer
            return finish(res)
        if mode == 'min':
            # every item has at least one copy (its own row or a ghost); amin without the initial value
            res = torch.empty((self.sendlength,) + trailing, dtype=data.dtype, device=be.device)
            idx = self.indices.to(torch.int64).reshape([-1] + [1] * (recvbuffer.dim() - 1)).expand_as(recvbuffer)
            res.scatter_reduce_(0, idx, recvbuffer, 'amin', include_self=False)
            return finish(res)
        if isinstance(mode, numpy.ufunc):
            # host path: ufunc.reduceat over index-sorted copies (domain.py:297-303)
            idx = self.indices.cpu().numpy()
            rb = recvbuffer.cpu().numpy()
            arg = idx.argsort(kind='stable')
            rb = rb[arg]
            N = numpy.bincount(idx, minlength=self.sendlength)
            offset = numpy.zeros(self.sendlength, 'intp')
            offset[1:] = numpy.cumsum(N)[:-1]
            r = mode.reduceat(rb, offset)
            return finish(torch.from_numpy(r).to(be.device))
        raise NotImplementedError


def _drop_hold(hold):
    if hold is not None:
        hold.release()          # (the next get() of the buffer waits for the exchange itself)


class _RemoteExchange(object):
    """handle of Layout.exchange_remote(async_op=True)"""
    def __init__(self, layout, state):
        self.layout, self.state = layout, state

    def wait(self):
        return self.layout._exchange_remote_end(self.state)

    def __del__(self):
        # a handle dropped without wait(): the staging goes back to the pool
        try:
            _drop_hold(self.state.get('hold'))
        except Exception:
            pass


class _Pending2(object):
    """handle of Layout.gather_remote_add(async_op=True): wait(out) adds what came back into `out`"""
    def __init__(self, finish, keepalive, hold=None):
        self.finish, self.keepalive, self.hold = finish, keepalive, hold

    def wait(self, out):
        return self.finish(out)

    def __del__(self):
        try:
            _drop_hold(self.hold)
        except Exception:
            pass


class _Finished(object):
    def __init__(self, out):
        self.out = out

    def wait(self, out):
        return out


class GridND(object):
    """
    GridND is domain decomposition on a uniform grid of N dimensions (domain.py:320-407).

    The total number of domains is prod([ len(dir) - 1 for dir in edges]).

    Attributes
    ----------
    edges   : list  (Ndim); edges[i] includes 0 and BoxSize.
    comm    : communicator (pmesh_amd.comm), default the world communicator
    periodic : boolean; if so, edges[i][-1] is the period.
    """

    @classmethod
    def uniform(cls, BoxSize, comm=None, periodic=True):
        """ a grid over the box [0, BoxSize) with about one domain per rank, the domains as close to cubes as the
        rank count allows (domain.py:340-360): per axis `side x (BoxSize[d] / min BoxSize)` domains, rounded down,
        where side^ndim x the box's aspect = comm.size; the axis with the most domains then takes every rank the
        others leave. """
        comm = default_comm() if comm is None else comm
        box = [float(b) for b in BoxSize]
        shortest = min(box)
        side = (1.0 * comm.size / numpy.prod(BoxSize) * shortest) ** (1.0 / len(box))
        wanted = numpy.array([side * (b / shortest) for b in box])
        longest = int(wanted.argmax())
        shape = numpy.maximum(numpy.int32(wanted), 1)
        shape[longest] = 1
        shape[longest] = comm.size // numpy.prod(shape)
        assert numpy.prod(shape) <= comm.size
        return cls([numpy.linspace(0, b, n + 1, endpoint=True) for b, n in zip(BoxSize, shape)], comm, periodic)

    def __init__(self, edges, comm=None, periodic=True, DomainAssign=None):
        """ DomainAssign records each domain is assigned to which rank """
        if comm is None:
            comm = default_comm()
        self.shape = numpy.array([len(g) - 1 for g in edges], dtype='int32')
        self.ndim = len(self.shape)
        self.edges = [numpy.asarray(g, dtype='f8') for g in edges]
        self.periodic = periodic
        self.comm = comm
        self.size = int(numpy.prod(self.shape))

        if DomainAssign is None:
            # domain k of a grid with more domains than ranks goes to the rank r with r * size // P <= k < (r + 1) *
            # size // P (contiguous, near-equal runs; domain.py:381-388); with ranks to spare, domain k to rank k
            k = numpy.arange(self.size, dtype='i8')
            if comm.size >= self.size:
                DomainAssign = k
            else:
                bounds = numpy.arange(1, comm.size + 1, dtype='i8') * self.size // comm.size
                DomainAssign = numpy.searchsorted(bounds, k, side='right')
        self.DomainAssign = numpy.asarray(DomainAssign, dtype='int32')

        # a domain is degenerate when it has zero width along some axis (domain.py:392-400)
        flat_axes = [numpy.diff(e) == 0 for e in self.edges]
        degenerate = numpy.zeros(tuple(self.shape), dtype=bool)
        for axis, flat in enumerate(flat_axes):
            sel = [None] * self.ndim
            sel[axis] = slice(None)
            degenerate |= flat[tuple(sel)]
        self.DomainDegenerate = degenerate.ravel().astype('int16')
        self._dev = None
        self._update_primary_regions()

    # device copies of the small tables the kernels read
    def _device_tables(self, be):
        if self._dev is None or self._dev['device'] != be.device or self._dev['stamp'] is not self.DomainAssign:
            edges = [torch.from_numpy(numpy.ascontiguousarray(e)).to(be.device) for e in self.edges]
            assign = torch.from_numpy(numpy.ascontiguousarray(self.DomainAssign)).to(be.device)
            # quirk Q3 (the table is indexed by rank after the lookup): pad so that any
            # rank id < nranks is a valid index even when there are fewer domains
            n = max(self.size, self.comm.size)
            deg = numpy.zeros(n, dtype='int16')
            deg[:self.size] = self.DomainDegenerate
            degen = torch.from_numpy(deg).to(be.device)
            self._dev = dict(device=be.device, edges=edges, assign=assign, degen=degen,
                             stamp=self.DomainAssign)
        return self._dev

    def _split_axes(self):
        """how many leading axes the classification has to look at: a grid of more dimensions than the ABI's
        pmx_grid holds (PMX_MAXDIM) is classified by its first axes if all the others are ONE periodic domain — what
        ParticleMesh makes for a mesh of 4 or more dimensions (slabs along axis 0): the flat index of a domain is
        then its index over the leading axes"""
        nd = self.ndim
        if nd <= _abi.PMX_MAXDIM:
            return nd
        k = max([d + 1 for d in range(nd) if int(self.shape[d]) > 1] or [1])
        if k > _abi.PMX_MAXDIM or not self.periodic:
            raise NotImplementedError('a domain grid of %d dimensions is decomposed along its first %d axes only, '
                                      'periodic' % (nd, _abi.PMX_MAXDIM))
        return k

    def _cgrid(self, be):
        t = self._device_tables(be)
        g = _abi.Grid()
        g.ndim = self._split_axes()
        g.periodic = int(bool(self.periodic))
        g.nranks = self.comm.size
        for d in range(g.ndim):
            g.shape[d] = int(self.shape[d])
            g.edges[d] = t['edges'][d].data_ptr()
        g.assign = t['assign'].data_ptr()
        g.degenerate = t['degen'].data_ptr()
        return g

    def load(self, pos, transform=None, gamma=2):
        """ load of each domain, N^gamma with N the particles in it (domain.py:409-466). """
        be = backend.get()
        pos, _ = to_device(pos, be.device, 'pos')
        assert pos.shape[1] >= self.ndim
        x = self._transform(pos, transform, be)
        if len(pos):
            flat = torch.zeros(len(pos), dtype=torch.int64, device=be.device)
            for j in range(self.ndim):
                e = torch.from_numpy(self.edges[j]).to(be.device)
                c = x[:, j].to(torch.float64)
                if self.periodic:
                    c = torch.remainder(c, float(self.edges[j][-1]))
                sil = torch.bucketize(c, e, right=True) - 1
                if self.periodic:
                    if ((sil < 0) | (sil >= int(self.shape[j]))).any():
                        raise ValueError('invalid entry in coordinates array')
                else:
                    sil = sil.clamp(0, int(self.shape[j]) - 1)
                flat = flat * int(self.shape[j]) + sil
            tmp = torch.bincount(flat, minlength=self.size).cpu().numpy().astype('f8')
        else:
            tmp = numpy.zeros(self.size)
        domainload = numpy.asarray(self.comm.allreduce(tmp))
        return domainload ** gamma

    def loadbalance(self, domainload):
        """ Balance the load of the ranks given the load of each domain; the result is
            recorded in self.DomainAssign (domain.py:469-501). """
        if self.size <= self.comm.size:
            return
        # longest-processing-time greedy (domain.py:485-498): domains in order of decreasing (load, index), each to
        # the rank that carries the least so far, the lowest such rank on a tie
        load = numpy.asarray(domainload, dtype='f8')
        order = numpy.lexsort((numpy.arange(self.size), load))[::-1]
        carried = numpy.zeros(self.comm.size, dtype='f8')
        assign = self.DomainAssign.copy()
        for k in order:
            r = int(numpy.argmin(carried))
            carried[r] += load[k]
            assign[k] = r
        self.DomainAssign = assign
        self._update_primary_regions()

    def _update_primary_regions(self):
        """primary_region: the lower and upper corners of the domains of this rank, (N, ndim) each, or None if it
        has none (domain.py:503-517)"""
        mine = numpy.flatnonzero(self.DomainAssign == self.comm.rank)
        if len(mine) == 0:
            self.primary_region = None
            return
        cells = numpy.unravel_index(mine, tuple(self.shape))
        self.primary_region = {
            'start': numpy.stack([e[c] for e, c in zip(self.edges, cells)], axis=1).astype('f8'),
            'end': numpy.stack([e[c + 1] for e, c in zip(self.edges, cells)], axis=1).astype('f8'),
        }

    def isprimary(self, pos, transform=None):
        """ True where the position falls into the primary region of this rank
            (domain.py:519-559). """
        be = backend.get()
        pos, host = to_device(pos, be.device, 'pos')
        if self.primary_region is None:
            r = torch.zeros(len(pos), dtype=torch.bool, device=be.device)
            return to_numpy(r) if host else r
        chunk = self._transform(pos, transform, be)[..., :self.ndim].to(torch.float64)
        if self.periodic:
            box = torch.tensor([self.edges[j][-1] for j in range(self.ndim)], dtype=torch.float64,
                               device=be.device)
            chunk = torch.remainder(chunk, box)
        r = torch.zeros(len(pos), dtype=torch.bool, device=be.device)
        x0 = torch.from_numpy(self.primary_region['start']).to(be.device)
        x1 = torch.from_numpy(self.primary_region['end']).to(be.device)
        for j in range(len(x0)):
            r |= ((chunk >= x0[j]) & (chunk < x1[j])).all(dim=-1)
        return to_numpy(r) if host else r

    @staticmethod
    def _transform(pos, transform, be):
        if transform is None:
            return pos
        try:
            return transform(pos)
        except TypeError:
            # a numpy-only callable: evaluate on the host
            return torch.from_numpy(numpy.asarray(transform(pos.cpu().numpy()))).to(be.device)

    def decompose(self, pos, smoothing=0, transform=None, _scale=None):
        """
        Decompose particles into domains (domain.py:561-652).

        Parameters
        ----------
        pos       :  array_like (, ndim)
            position of particles; more columns than the dimensions of the domains are
            allowed, only the first few directions are used.
        smoothing : float, or array_like
            Any particle that intersects a domain within `smoothing` (in the coordinate system
            of the edges) will be transported to the domain; per dimension if array_like.
        transform : callable
            transform(pos[:, 3]) -> domain_pos[:, 3], applied before the decompostion.
            (ParticleMesh passes its pure scaling via `_scale` so it runs inside the kernel.)

        Returns
        -------
        layout :  :py:class:`Layout` object that can be used to exchange data
        """
        be = backend.get()
        pos, _ = to_device(pos, be.device, 'pos')
        # we can't deal with too many points per rank with 32-bit indices: switch to 64-bit
        index_dtype = torch.int32 if len(pos) < 1024 * 1024 * 1024 * 2 else torch.int64
        sm = numpy.empty(self.ndim, dtype='f8')
        sm[:] = smoothing
        if pos.dim() != 2 or pos.shape[1] < self.ndim:
            raise AssertionError('pos.shape[1] >= self.ndim')
        if transform is not None:
            pos = self._transform(pos, transform, be)
        scale = numpy.ones(self.ndim, dtype='f8')
        if _scale is not None:
            scale[:] = _scale
        Npoint = len(pos)
        P = self.comm.size
        counts_dtype = 'int32' if index_dtype == torch.int32 else 'int64'
        if (P == 1 and self.periodic and self.size == 1 and int(self.DomainAssign[0]) == 0
                and not int(self.DomainDegenerate[0])):
            # ONE periodic domain on one rank: every position — finite or not, whatever the smoothing — resolves to
            # it exactly once (the wrapped patch of gridnd_fill, _domain.pyx:62-118, names domain 0 however often
            # and the targets are unique): sendcounts = [N], indices = 0 .. N - 1, nothing to classify
            return Layout(comm=self.comm, sendlength=Npoint, sendcounts=numpy.array([Npoint], dtype=counts_dtype),
                          indices=lambda: torch.arange(Npoint, dtype=index_dtype, device=be.device),
                          recvcounts=numpy.array([Npoint], dtype=counts_dtype))
        if Npoint != 0:
            masks = torch.empty(Npoint, dtype=torch.int64, device=be.device)
            counts = torch.zeros(P, dtype=torch.int64, device=be.device)
            g = self._cgrid(be)
            pv = vec(pos)
            be.call('decompose_count', C.byref(g), C.byref(pv), _abi.f64arr(scale[:g.ndim], 3),
                    _abi.f64arr(sm[:g.ndim], 3), Npoint, masks.data_ptr(), counts.data_ptr(), be.stream())
            hcounts = counts.cpu().numpy()          # the one host sync of decompose
            offsets = numpy.zeros(P, dtype='i8')
            offsets[1:] = numpy.cumsum(hcounts)[:-1]
            doff = torch.from_numpy(offsets).to(be.device)
            indices = torch.empty(int(hcounts.sum()), dtype=index_dtype, device=be.device)
            be.call('decompose_fill', P, masks.data_ptr(), Npoint, doff.data_ptr(),
                    indices.data_ptr(), indices.element_size(), be.stream())
            counts = hcounts.astype(counts_dtype)
        else:
            counts = numpy.zeros(P, dtype=counts_dtype)
            indices = torch.empty(0, dtype=index_dtype, device=be.device)
        return Layout(comm=self.comm, sendlength=Npoint, sendcounts=counts, indices=indices)
