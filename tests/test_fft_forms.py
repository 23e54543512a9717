"""The column / row kernel forms that only long lines select (csrc/pmx_colfft.hip, dispatch_logn), against numpy.fft
in complex128, at every built length and at the batch shapes of config 5 (2048^3 on a 2 x 4 pencil mesh): lines of
B = 257 / 254 complex elements (off 128-byte boundaries: tiles in XCD order), 64-byte half-line tiles and the half
twiddle table at N = 2048, persistent prefetching workgroups once the tiles outnumber the CUs (with a ragged last
tile), and the one-workgroup-per-tile form of the same kernels, which must give the same bits.  The small batches of
tests/test_fft_kernels.py never reach most of these.

Under -m gpu against the HIP library; otherwise against the numpy double of tests/oracle_backend.py, without the
batches that exist for the persistent form only (which then checks the test's own layouts and references)."""
import numpy
import pytest
import torch

from pmesh_amd.transfer import Transfer

TOL = {8: 2e-15, 4: 1e-6}
CDT = {8: 'c16', 4: 'c8'}
LENGTHS = [(N, es) for es in (8, 4) for N in (64, 128, 256, 512, 1024, 2048, 192, 384, 768, 1536, 320, 640, 1280)
           if not (es == 4 and N in (1536, 1280))]          # (float 1536 / 1280 are not built)
CUS = 256                                                   # compute units of an MI355X


def rel(a, b):
    return numpy.sqrt((abs(a - b) ** 2).sum() / max((abs(b) ** 2).sum(), 1e-300))


def worst_line(got, want, axis):
    """the largest relative L2 error of one line along `axis`"""
    e = (abs(got - want) ** 2).sum(axis=axis)
    w = numpy.maximum((abs(want) ** 2).sum(axis=axis), 1e-300)
    return float(numpy.sqrt(e / w).max())


def tile_width(N, es):
    """columns per tile of the column kernel (dispatch_logn): 64-byte row segments at 2048 and at the lengths whose
    128-byte tile would not fit the LDS (1536 / 1280 in double, 768 / 640 in float), 128-byte ones elsewhere"""
    half = N == 2048 or (es == 8 and N in (1536, 1280)) or (es == 4 and N in (768, 640))
    return (64 if half else 128) // (2 * es)


def p2(n):
    """the largest power of two dividing n (split ranges are powers of two)"""
    return n & -n


def batches(be, N, es):
    """(A, B): config 5's lines of 257 complex elements in more than 2 x 256 tiles with a ragged last one in every
    plane — where the length's kernel is persistent (ColPipe: N = 640 ... 2048 in double, 1024 in float) its
    workgroups walk several tiles each, elsewhere there is one workgroup per tile and the two forms coincide; 254 with a small A (one tile per
    workgroup); and a narrow batch"""
    out = [(2, 254), (3, 9)]
    if be.name == 'hip':
        per = -(-257 // tile_width(N, es))
        out.insert(0, (-(-(2 * CUS + 1) // per), 257))
    return out


def both_forms(be, run):
    """run() with persistent column passes and with one workgroup per tile: the same bits; the persistent result"""
    be.colfft_configure(1)
    try:
        one = run()
        be.colfft_configure(0)
        two = run()
    finally:
        be.colfft_configure(1)
    assert torch.equal(one, two)
    return one


def to_split(a, ns):
    """(A, N, B) -> the split layout of ranges of ns lines: [range][a][line in range][b] (0: plain)"""
    A, N, B = a.shape
    return a if ns == 0 else numpy.ascontiguousarray(a.reshape(A, N // ns, ns, B).transpose(1, 0, 2, 3))


def from_split(flat, A, N, B, ns):
    if ns == 0:
        return flat.reshape(A, N, B)
    return flat.reshape(N // ns, A, ns, B).transpose(1, 0, 2, 3).reshape(A, N, B)


def dev(be, x):
    return torch.view_as_real(torch.from_numpy(numpy.ascontiguousarray(x))).reshape(-1).to(be.device)


def host(t, cdt):
    return t.cpu().numpy().view(cdt)


def line_energy(t, A, N, B, ns):
    """sum |z|^2 of every line (a, b), in float64 on the device"""
    v = t.view(-1, 2)[:A * N * B].double()
    e = (v * v).sum(dim=1)
    if ns == 0:
        return e.view(A, N, B).sum(dim=1)
    return e.view(N // ns, A, ns, B).sum(dim=(0, 2))


def check_lines(be, got_t, x, y, A, N, B, ns, es, what):
    """got_t (device, layout ns) against y (complex128 (A, N, B)); Parseval of every line against the input x"""
    tol = TOL[es] * numpy.log2(N)
    got = from_split(host(got_t, CDT[es]).reshape(-1), A, N, B, ns)
    assert rel(got, y) < tol, what
    assert worst_line(got, y, 1) < 4 * tol, what
    ein = (abs(x.astype('c16')) ** 2).sum(axis=1)
    eout = line_energy(got_t, A, N, B, ns).cpu().numpy()
    assert float(abs(eout / (N * ein) - 1).max()) < 4 * tol, what


@pytest.mark.parametrize('N,es', LENGTHS)
def test_colfft_layout_forms(be, N, es):
    """colfft_resplit between split layouts (config 5 at N = 2048: 512 lines a range in, 1024 out, and back),
    colfft_split (plain <-> split) and colfft_to (out of place), forward and inverse"""
    cdt = CDT[es]
    q, h = p2(N // 4), p2(N // 2)
    splits = [(q, h), (h, q), (0, h), (q, 0)]
    if N == 2048:
        assert (512, 1024) in splits and (1024, 512) in splits
    rs = numpy.random.RandomState(N * 10 + es)
    for A, B in batches(be, N, es):
        x = (rs.normal(size=(A, N, B)) + 1j * rs.normal(size=(A, N, B))).astype(cdt)
        xd = x.astype('c16')
        for inverse in (False, True):
            y = numpy.fft.ifft(xd, axis=1) * N if inverse else numpy.fft.fft(xd, axis=1)
            ys = y * 0.5
            for nin, nout in splits:
                src = dev(be, to_split(x, nin))
                keep = src.clone()

                def run():
                    dst = torch.zeros_like(src)
                    be.colfft_resplit(es, inverse, src, dst, A, N, B, nin, nout, scale=0.5)
                    return dst
                got = both_forms(be, run)
                assert torch.equal(src, keep)
                check_lines(be, got, x * 0.5, ys, A, N, B, nout, es, ('resplit', A, B, inverse, nin, nout))
            # plain -> split (forward) / split -> plain (inverse): the slab transform's axis-1 pass
            ns = q
            src = dev(be, to_split(x, ns) if inverse else x)

            def run():
                dst = torch.zeros_like(src)
                be.colfft_split(es, inverse, src, dst, A, N, B, ns, scale=0.5)
                return dst
            got = both_forms(be, run)
            check_lines(be, got, x * 0.5, ys, A, N, B, 0 if inverse else ns, es, ('split', A, B, inverse))
            # out of place, plain layout
            src = dev(be, x)

            def run():
                dst = torch.zeros_like(src)
                be.colfft_to(es, inverse, src, dst, A, N, B, scale=0.5)
                return dst
            got = both_forms(be, run)
            check_lines(be, got, x * 0.5, ys, A, N, B, 0, es, ('to', A, B, inverse))


@pytest.mark.parametrize('N,es', LENGTHS)
def test_colfft_chunk_forms(be, N, es):
    """the axis-0 pass on columns [coff, coff + cw) of an (N, n1, pitch) block, with coff / cw off the tile width and
    the pitches of config 5's half spectrum (1025) and of a 512-point one (257), in more tiles than CUs (several per
    workgroup where the length's kernel is persistent); scatter (to_full) and gather; the block outside the chunk untouched"""
    cdt, tdt = CDT[es], (torch.complex128 if es == 8 else torch.complex64)
    W = tile_width(N, es)
    tol = TOL[es] * numpy.log2(N)
    rs = numpy.random.RandomState(N * 7 + es)
    for pitch, coff, cw in ((1025, W + 1, 1019 - W), (257, 3, 250)):
        assert coff % W and cw % W and coff + cw <= pitch
        n1 = -(-(CUS + 40) * W // cw) if be.name == 'hip' else 2
        full_h = (rs.normal(size=(N, n1, pitch)) + 1j * rs.normal(size=(N, n1, pitch))).astype(cdt)
        chunk_h = (rs.normal(size=(N, n1, cw)) + 1j * rs.normal(size=(N, n1, cw))).astype(cdt)
        mask = numpy.ones(pitch, bool)
        mask[coff:coff + cw] = False
        for inverse in (False, True):
            c = chunk_h.astype('c16')
            want = (numpy.fft.ifft(c, axis=0) * N if inverse else numpy.fft.fft(c, axis=0)) * 0.5
            chunk = torch.from_numpy(chunk_h).to(be.device)

            def run():
                full = torch.from_numpy(full_h).to(be.device)
                be.colfft_chunk(es, inverse, torch.view_as_real(chunk).reshape(-1), torch.view_as_real(full).reshape(-1),
                                N, n1, cw, pitch, coff, True, scale=0.5)
                return full
            got = both_forms(be, run).cpu().numpy()
            assert rel(got[:, :, coff:coff + cw], want) < tol, (pitch, inverse)
            assert worst_line(got[:, :, coff:coff + cw], want, 0) < 4 * tol, (pitch, inverse)
            assert numpy.array_equal(got[:, :, mask], full_h[:, :, mask])
            # gather
            f = full_h[:, :, coff:coff + cw].astype('c16')
            want = numpy.fft.ifft(f, axis=0) * N if inverse else numpy.fft.fft(f, axis=0)
            full = torch.from_numpy(full_h).to(be.device)

            def run():
                out = torch.zeros((N, n1, cw), dtype=tdt, device=be.device)
                be.colfft_chunk(es, inverse, torch.view_as_real(out).reshape(-1), torch.view_as_real(full).reshape(-1),
                                N, n1, cw, pitch, coff, False)
                return out
            got = both_forms(be, run).cpu().numpy()
            assert rel(got, want) < tol, (pitch, inverse)
            assert worst_line(got, want, 0) < 4 * tol, (pitch, inverse)
            assert numpy.array_equal(full.cpu().numpy(), full_h)


def _fused_transfers():
    return [('dx1', d, Transfer.dx1(d)) for d in range(3)] + [('force', d, Transfer.force(d)) for d in range(3)] + \
           [('potential', -1, Transfer.potential()), ('laplace+1', -1, Transfer(laplace_pow=1))]


@pytest.mark.parametrize('N,es', [(2048, 8), (2048, 4), (1024, 8), (1024, 4), (1536, 8), (1280, 8), (768, 8),
                                  (640, 4), (64, 8)])
def test_colfft_fused_transfer_forms(be, oracle, N, es):
    """the inverse axis-0 pass with the transfer function fused in, through colfft, colfft_chunk and
    colfft_roundtrip: a block of config 5's complex layout (nmesh 2048 along axes 1 and 2) at start[1] != 0 in the
    last mode range of the last axis (771 ... 1024, which holds the Nyquist index N2 / 2), n1 scaled with the tile
    width to more tiles than CUs — so that, where the plain pass of this length is persistent (ColPipe: 1024 / 768 /
    640 / 1536 / 1280 / 2048 in double), the fused one walks several tiles per workgroup; in float the launcher keeps
    the fused pass at one workgroup per tile, and both forms are that one.  The finite-difference gradient along
    axis 0 is not fusable: refused"""
    from pmesh_amd.backend import PmxError
    cdt = CDT[es]
    tol = TOL[es] * numpy.log2(N)
    nmesh, box = (N, 2048, 2048), (1000.0, 700.0, 1300.0)
    n2 = 254
    n1 = -(-(CUS + 40) * tile_width(N, es) // n2) if be.name == 'hip' else 1
    start = (0, 1021, 771)
    assert start[2] + n2 == nmesh[2] // 2 + 1
    B = n1 * n2
    rs = numpy.random.RandomState(N + es)
    x = (rs.normal(size=(N, n1, n2)) + 1j * rs.normal(size=(N, n1, n2))).astype(cdt)
    xd = x.astype('c16')
    # chunk: the block is columns [coff, coff + n2) of an (N, n1, pitch) array, start[2] that of the array
    coff, pitch = 3, n2 + 7
    full_h = numpy.zeros((N, n1, pitch), dtype=cdt)
    full_h[:, :, coff:] = rs.normal(size=(N, n1, pitch - coff))
    full_h[:, :, coff:coff + n2] = x
    cstart = (start[0], start[1], start[2] - coff)
    for name, d, T in _fused_transfers():
        t = T._cstruct()
        if not T.fusable():
            if be.name == 'hip':
                with pytest.raises(PmxError):
                    be.colfft(es, True, dev(be, x), 1, N, B, transfer=t, n1=n1, n2=n2, start=start, nmesh=nmesh,
                              boxsize=box)
            continue
        tk = oracle.apply_transfer(t, xd, start, nmesh, box)
        want = numpy.fft.ifft(tk, axis=0) * N
        src = dev(be, x)

        def run():
            d_ = src.clone()
            be.colfft(es, True, d_, 1, N, B, transfer=t, n1=n1, n2=n2, start=start, nmesh=nmesh, boxsize=box)
            return d_
        got = host(both_forms(be, run), cdt).reshape(N, n1, n2)
        assert rel(got, want) < tol, ('colfft', name, d)
        assert worst_line(got, want, 0) < 4 * tol, ('colfft', name, d)
        full = torch.from_numpy(full_h).to(be.device)

        def run():
            out = torch.zeros((N, n1, n2), dtype=full.dtype, device=be.device)
            be.colfft_chunk(es, True, torch.view_as_real(out).reshape(-1), torch.view_as_real(full).reshape(-1),
                            N, n1, n2, pitch, coff, False, transfer=t, start=cstart, nmesh=nmesh, boxsize=box)
            return out
        got = both_forms(be, run).cpu().numpy()
        assert rel(got, want) < tol, ('chunk', name, d)
        assert worst_line(got, want, 0) < 4 * tol, ('chunk', name, d)
        if not be.colfft_roundtrip_supported(N, es):
            continue
        # forward, x 1/N, transfer, inverse in one kernel: on the spectrum X of x, back to T * X in configuration space
        want = numpy.fft.ifft(oracle.apply_transfer(t, numpy.fft.fft(xd, axis=0) / N, start, nmesh, box), axis=0) * N

        def run():
            d_ = src.clone()
            be.colfft_roundtrip(es, d_, N, B, scale=1.0 / N, transfer=t, n1=n1, n2=n2, start=start, nmesh=nmesh,
                                boxsize=box)
            return d_
        got = host(both_forms(be, run), cdt).reshape(N, n1, n2)
        assert rel(got, want) < 2 * tol, ('roundtrip', name, d)
        assert worst_line(got, want, 0) < 8 * tol, ('roundtrip', name, d)


@pytest.mark.parametrize('es', [8, 4])
@pytest.mark.parametrize('nrows', [4096, 4096 + 37])
@pytest.mark.parametrize('pitch', [1025, 1032])
def test_rowfft_split_config5_rows(be, es, nrows, pitch):
    """the row pass of a config-5 rank: rows of 2048 reals, their 1025 modes cut into blocks of 257 / 257 / 257 / 254
    (fft.block_edges(1025, 4)); block q dense (nrows, m_q) at element nrows * offsets[q]; the inverse ignores the
    imaginary parts of the DC and Nyquist modes, as irfft does"""
    from pmesh_amd.fft import block_edges
    n, M1 = 2048, 1025
    e = [0, 257, 514, 771, 1025]
    assert e == [int(v) for v in block_edges(M1, 4)]
    assert be.rowfft_split_supported(n, es, 4)
    rdt, cdt = ('f8', 'c16') if es == 8 else ('f4', 'c8')
    tol = TOL[es] * numpy.log2(n)
    rs = numpy.random.RandomState(nrows + pitch + es)
    buf = numpy.zeros((nrows, 2 * pitch), dtype=rdt)
    x = rs.normal(size=(nrows, n)).astype(rdt)
    buf[:, :n] = x
    src = torch.from_numpy(buf).reshape(-1).to(be.device)
    keep = src.clone()
    tail = 64
    dst = torch.full((2 * (nrows * M1 + tail),), 7.0, dtype=src.dtype, device=be.device)
    be.rowfft_split(es, False, src, dst, nrows, n, pitch, e, scale=2.0)
    assert torch.equal(src, keep)
    assert bool((dst[2 * nrows * M1:] == 7.0).all())                 # nothing written past the blocks
    got = host(dst, cdt)[:nrows * M1]
    want = numpy.fft.rfft(x.astype('f8'), axis=1) * 2.0
    for q in range(4):
        blk = got[nrows * e[q]:nrows * e[q + 1]].reshape(nrows, e[q + 1] - e[q])
        assert rel(blk, want[:, e[q]:e[q + 1]]) < tol, q
        assert worst_line(blk, want[:, e[q]:e[q + 1]], 1) < 4 * tol, q
    # element by element: mode k of row r belongs at nrows * e[q] + r * m_q + (k - e[q]), q the block holding k; every
    # mode there within a bound on the row's scale (a misplaced or missing element is off by the row's rms or more)
    k = numpy.arange(M1)
    q = numpy.searchsorted(e, k, side='right') - 1
    ea, m = numpy.array(e)[q], numpy.diff(e)[q]
    idx = nrows * ea[None, :] + numpy.arange(nrows)[:, None] * m[None, :] + (k - ea)[None, :]
    assert numpy.array_equal(numpy.sort(idx.reshape(-1)), numpy.arange(nrows * M1))
    scale = numpy.sqrt((abs(want) ** 2).mean(axis=1))[:, None]
    assert float((abs(got[idx] - want) / scale).max()) < 8 * tol
    # inverse: blocks -> rows, with imaginary parts on the DC (block 0, column 0) and Nyquist (block 3, last column)
    spec = got.copy()
    spec[0:nrows * 257:257] += 1j * rs.normal(size=nrows).astype(rdt)                    # (row r: element 257 r)
    spec[nrows * 771 + 253:nrows * M1:254] += 1j * rs.normal(size=nrows).astype(rdt)     # (row r: 771 n + 254 r + 253)
    full = numpy.empty((nrows, M1), dtype='c16')
    for q in range(4):
        full[:, e[q]:e[q + 1]] = spec[nrows * e[q]:nrows * e[q + 1]].reshape(nrows, e[q + 1] - e[q])
    assert numpy.array_equal(full[:, 0].imag != 0, numpy.ones(nrows, bool))
    assert numpy.array_equal(full[:, -1].imag != 0, numpy.ones(nrows, bool))
    sd = torch.view_as_real(torch.from_numpy(spec)).reshape(-1).to(be.device)
    back = torch.full_like(keep, 3.0)
    be.rowfft_split(es, True, sd, back, nrows, n, pitch, e, scale=1.0 / (2.0 * n))
    want = numpy.fft.irfft(full, n=n, axis=1) / 2.0
    b = back.cpu().numpy().reshape(nrows, 2 * pitch)
    assert (b[:, n:] == 3.0).all()                                      # the pitch padding of the rows not written
    assert rel(b[:, :n], want) < 2 * tol
    assert worst_line(b[:, :n], want, 1) < 8 * tol
    assert rel(want, x) < 2 * tol
