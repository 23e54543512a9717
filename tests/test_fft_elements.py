"""The LDS row / column FFT kernels (csrc/pmx_colfft.hip) element by element, never through a norm: impulses against
closed forms, metamorphic checks bit for bit, and the fused transfer function at its special modes.

Under -m gpu against the HIP library; under -m "not gpu" the same tests run against the numpy double of
tests/oracle_backend.py, which checks the references, bounds and block geometry written here (the tests on tile
structure, placement and isolation, concern the HIP kernels alone and carry the gpu mark themselves).

The reference is a closed form in numpy.longdouble (80-bit: asserted at import), no O(N^2) matrix anywhere.  A phase
is exp(-+ 2 pi i ((j k) mod N) / N) with the integer product reduced before the division and pi = 4 arctan(1).
u = 2^-53 for elsize 8, 2^-24 for elsize 4.

1. Impulses.  Every line holds one non-zero element amp at position j, so every output is a twiddle in the clear:

       |got[k] - amp scale phase(j, k)| <= 4 u log2(N) |amp scale|

   With one non-zero input every butterfly of every pass has one non-zero leg and its additions are exact.  A path
   collects per pass one stored twiddle (rounded to at most u) and one complex multiply (at most sqrt(5) u), and
   inside a radix-8 or radix-4 butterfly at most one multiplication by a w8 constant (about 1.5 u; -+ i is exact):
   under 5 u for three binary stages.  A radix-3 or radix-5 pass costs under 9 u (log2(5) * 4 = 9.3), and the first
   pass has no twiddle.  The row kernel
   (r2c / c2r) runs the half-length complex transform plus the X <-> Z step, which adds two non-zero terms: log2(n) + 2
   in place of log2(N); c2r is bounded on the sum of the magnitudes of its terms.

   The worst error seen, in units of u log2(N) |amp scale| (u (log2(n) + 2) times the magnitudes for the rows; the
   assertion is <= 4), over all lengths, forward and inverse, on an MI355X:

       entry            complex128 / float64    complex64 / float32
       colfft           1.30                    0.82
       rowfft r2c       0.89                    0.48
       rowfft c2r       0.29                    0.22

   (colfft_to returns the bits of colfft.)  The numpy double of the CPU mode, in the same units: 0.72 / 0.16,
   0.51 / 0.10 and 0.37 / 0.09.  What the bound can and cannot see: a twiddle entry moved by 64 units in the last
   place fails it at every length in both precisions (while every norm-based test of the kernels passes); one moved
   by a single unit moves an output by u |amp scale|, inside any bound that admits the rounding of a correct kernel.

2. Metamorphic checks, bit for bit, on dense Gaussian lines: scaling a line by a power of two scales its output (it
   commutes with every rounding; nothing under- or overflows) and a zero line gives exact zeros; on the HIP kernels
   a line's output does not depend on where in the batch it stands (whole and ragged tiles, first and later tiles of
   a persistent workgroup, every column of a tile) nor on a NaN or an infinite line in its tile.

3. The fused transfer at its special modes: a block that holds global index 0 along axes 1 and 2, their Nyquist
   indices and the negative half (and one that holds none of them), lines that are non-zero at i0 in {0, 1, N/2 - 1,
   N/2, N/2 + 1, N - 1} only, every fusable form, against sum_j f_j x_j phase(j, n) with f from the restatement of
   tests/test_transfer_kernel.py:

       |got - want| <= sum_j [(4 log2(N) + 2) u + 1e-14] bound_j |x_j|

   (bound_j: the restatement's; 1e-14: the stand-alone kernel's tolerance for the factor, which the fused kernel also
   forms in double in both precisions; 2 u: the rounding of T x to storage precision before the first pass.)  The
   round-trip kernel is then held bit for bit to the two passes it replaces at every length it is built for.
"""
import numpy
import pytest
import torch

from pmesh_amd.backend import PmxError
from pmesh_amd.transfer import Transfer
from tests.test_fft_forms import LENGTHS, batches, both_forms, dev, host, tile_width
from tests.test_transfer_kernel import mode_numbers, restate

LD, CLD = numpy.longdouble, numpy.clongdouble
assert numpy.finfo(LD).eps < 2 ** -60, 'the bounds of this module need an 80-bit reference'
PI = 4 * numpy.arctan(LD(1))

U = {8: 2.0 ** -53, 4: 2.0 ** -24}
CDT = {8: 'c16', 4: 'c8'}
RDT = {8: 'f8', 4: 'f4'}
ALL = [(N, es) for es in (8, 4) for N in (64, 128, 256, 512, 1024, 2048, 192, 384, 768, 1536, 320, 640, 1280)]
ROWS = [128, 256, 512, 1024, 2048, 384, 768, 1536, 640, 1280]
RADICES = {64: (8, 8), 128: (8, 4, 4), 256: (8, 8, 4), 512: (8, 8, 8), 1024: (8, 8, 4, 4), 2048: (8, 8, 8, 4),
           192: (8, 8, 3), 384: (8, 4, 4, 3), 768: (8, 8, 4, 3), 1536: (8, 8, 8, 3),
           320: (8, 8, 5), 640: (8, 4, 4, 5), 1280: (8, 8, 4, 5)}          # Radices<LOGN> of the kernels
SHIFTS = {8: (0, -40, 40, -7, 13), 4: (0, -12, 12, -7, 5)}
SCALE = 0.5
GOLD = 0.6180339887498949


# ---- the reference --------------------------------------------------------------------------------------------------

def phases(js, N, inverse, nk=None):
    """(len(js), nk) clongdouble: exp(-+ 2 pi i ((j k) mod N) / N) for k = 0 .. nk - 1 (nk: N)"""
    k = numpy.arange(N if nk is None else nk, dtype='i8')
    m = (numpy.asarray(js, dtype='i8')[:, None] * k[None, :]) % N
    a = 2 * PI * m.astype(LD) / N
    out = numpy.empty(m.shape, dtype=CLD)
    out.real = numpy.cos(a)
    out.imag = numpy.sin(a) if inverse else -numpy.sin(a)
    return out


def strides(N):
    """the partial products of the length's radix schedule: the strides of its Stockham passes"""
    out, s = [], 1
    for r in RADICES[N][:-1]:
        s *= r
        out.append(s)
    return out


def positions(N):
    p = [0, 1, 2, 3, 5, 7, N // 2 - 1, N // 2, N // 2 + 1, N - 1, N // 3, N // 5, N // 8 + 1] + strides(N)
    return sorted(set(p))


def amplitudes(n, dt):
    """n fixed non-dyadic numbers of magnitude 0.8 ... 1.2, no two alike, in the storage type (complex or real)"""
    i = numpy.arange(n)
    r = 0.8 + 0.4 * ((i * GOLD) % 1)
    if numpy.dtype(dt).kind == 'c':
        return (r * numpy.exp(1j * (0.3 + 0.7 * i))).astype(dt)
    return (r * (1 - 2 * (i % 2))).astype(dt)


def same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def report(entry, es, worst):
    print('RATIO %s es=%d %.3f' % (entry, es, worst))


def col_built(be, N, es):
    """the lengths colfft is offered for are exactly LENGTHS (float 1536 / 1280 are not built): a kernel that stops
    being offered fails here, it does not skip"""
    built = [(n, e) for n, e in ALL if be.colfft_supported(n, e)]
    assert built == LENGTHS
    assert set(ALL) - set(built) == {(1536, 4), (1280, 4)}
    if (N, es) not in built:
        pytest.skip('length not built for this precision')


def row_built(be):
    assert all(be.rowfft_supported(n, es) for n in ROWS for es in (8, 4))


@pytest.fixture
def hip():
    """the HIP backend alone, for what concerns the tiles of its kernels"""
    from pmesh_amd import backend
    backend.reset()
    b = backend.get()
    assert b.name == 'hip'
    yield b
    backend.reset()


# ---- 1. impulses ----------------------------------------------------------------------------------------------------

def impulse_error(got, amp, pidx, P, scale):
    """max over the elements of the lines (rows of `got`, (lines, nk)) of |got - amp scale P[pidx]| / |amp scale|, in
    long double; NaN if an element is"""
    ar, ai = amp.real.astype(LD)[:, None] * scale, amp.imag.astype(LD)[:, None] * scale
    Pr, Pi = P.real[pidx], P.imag[pidx]
    dr = got.real.astype(LD) - (ar * Pr - ai * Pi)
    di = got.imag.astype(LD) - (ar * Pi + ai * Pr)
    return float(numpy.sqrt(((dr * dr + di * di) / (ar * ar + ai * ai)).max()))


@pytest.mark.parametrize('N,es', ALL)
def test_colfft_impulses(be, N, es):
    """one non-zero element per line, forward and inverse, on two planes of 2 W + 3 columns and (hip) on the batch of
    more than two tiles per CU with a ragged last tile in every plane; colfft_to: the same bits, its source kept"""
    col_built(be, N, es)
    cdt, W = CDT[es], tile_width(N, es)
    pos = positions(N)
    shapes = [(2, 2 * W + 3)] + (batches(be, N, es)[:1] if be.name == 'hip' else [])
    worst = 0.0
    for A, B in shapes:
        amp = amplitudes(A * B, cdt).reshape(A, B)
        pidx = (numpy.arange(A * B) % len(pos)).reshape(A, B)
        x = numpy.zeros((A, N, B), dtype=cdt)
        a_, b_ = numpy.meshgrid(numpy.arange(A), numpy.arange(B), indexing='ij')
        x[a_, numpy.array(pos)[pidx], b_] = amp
        src = dev(be, x)
        keep = src.clone()
        for inverse in (False, True):
            P = phases(pos, N, inverse)

            def run():
                d = src.clone()
                be.colfft(es, inverse, d, A, N, B, scale=SCALE)
                return d
            got_t = both_forms(be, run)
            got = host(got_t, cdt).reshape(A, N, B)
            for a in range(A):
                e = impulse_error(got[a].T, amp[a], pidx[a], P, SCALE) / (U[es] * numpy.log2(N))
                worst = max(worst, e) if e == e else e
                assert e <= 4, ('colfft', A, B, a, inverse, e)

            def run():
                d = torch.full_like(src, float('nan'))
                be.colfft_to(es, inverse, src, d, A, N, B, scale=SCALE)
                return d
            assert torch.equal(both_forms(be, run), got_t), ('colfft_to', A, B, inverse)
            assert torch.equal(src, keep)
    report('colfft', es, worst)


@pytest.mark.parametrize('es', [8, 4])
@pytest.mark.parametrize('n', ROWS)
def test_rowfft_impulses(be, n, es):
    """r2c of real impulses: every mode 0 .. n/2 a twiddle; c2r of a sparse half spectrum (k = 0, 1, n/4, n/2 - 1,
    n/2, the DC and Nyquist entries with imaginary parts that must be ignored) against its closed form"""
    row_built(be)
    rdt, cdt, M1 = RDT[es], CDT[es], n // 2 + 1
    pos = sorted(set(positions(n) + [2 * s + o for s in strides(n // 2) for o in (0, 1)]))
    tol = U[es] * (numpy.log2(n) + 2)
    assert len(pos) <= 24
    worst = [0.0, 0.0]
    for nrows, pitch in ((5, n // 2 + 1), (19, n // 2 + 8)):
        # r2c
        amp = amplitudes(nrows, rdt)
        pidx = (numpy.arange(nrows) + (0 if nrows == 5 else 5)) % len(pos)      # (the 24 rows: every position)
        buf = numpy.zeros((nrows, 2 * pitch), dtype=rdt)
        buf[numpy.arange(nrows), numpy.array(pos)[pidx]] = amp
        t = torch.from_numpy(buf).reshape(-1).to(be.device)
        be.rowfft(es, False, t, nrows, n, pitch, scale=SCALE)
        got = t.cpu().numpy().view(cdt).reshape(nrows, pitch)[:, :M1]
        e = impulse_error(got, amp.astype(cdt), pidx, phases(pos, n, False, M1), SCALE) / tol
        worst[0] = max(worst[0], e) if e == e else e
        assert e <= 4, ('r2c', nrows, pitch, e)
        # c2r
        ks = [0, 1, n // 4, n // 2 - 1, n // 2]
        X = amplitudes(nrows * len(ks), cdt).reshape(nrows, len(ks))
        assert (X[:, 0].imag != 0).all() and (X[:, -1].imag != 0).all()
        spec = numpy.zeros((nrows, pitch), dtype=cdt)
        spec[:, ks] = X
        t = torch.view_as_real(torch.from_numpy(spec)).reshape(-1).to(be.device)
        be.rowfft(es, True, t, nrows, n, pitch, scale=SCALE)
        got = t.cpu().numpy().view(rdt).reshape(nrows, 2 * pitch)[:, :n].astype(LD)
        P = phases(ks[1:-1], n, True)                                   # (3, n): exp(+ 2 pi i k m / n)
        sign = 1 - 2 * (numpy.arange(n) % 2)
        Xl = X.astype(CLD)
        want = Xl[:, :1].real + sign[None, :] * Xl[:, -1:].real + 2 * (Xl[:, 1:-1] @ P).real
        mag = abs(Xl[:, 0].real) + abs(Xl[:, -1].real) + 2 * abs(Xl[:, 1:-1]).sum(axis=1)
        e = float((abs(got - want * SCALE) / (mag[:, None] * SCALE)).max()) / tol
        worst[1] = max(worst[1], e) if e == e else e
        assert e <= 4, ('c2r', nrows, pitch, e)
    report('rowfft_r2c', es, worst[0])
    report('rowfft_c2r', es, worst[1])


# ---- 2. metamorphic checks, bit for bit -----------------------------------------------------------------------------

def gaussian(rs, shape, dt):
    if numpy.dtype(dt).kind == 'c':
        return (rs.normal(size=shape) + 1j * rs.normal(size=shape)).astype(dt)
    return rs.normal(size=shape).astype(dt)


def scaled_lines(base, es, nlines):
    """(nlines, len(base)): line l = base * 2^s_l, s_l cycling through SHIFTS (s_0 = 0), one line all zeros; s, the
    zero line's index"""
    s = numpy.array([SHIFTS[es][i % 5] for i in range(nlines)])
    zero = nlines - 2
    rdt = RDT[es]
    x = numpy.ldexp(base.view(rdt)[None, :], s[:, None]).astype(rdt)
    x[zero] = 0
    return x.view(base.dtype), s, zero


def assert_scaled(got, s, zero, es, what, ref=None):
    """lines `got` (nlines, m): line l is line 0 (or line l of `ref`, the output of the unscaled lines) times 2^s_l to
    the bit, the zero line exactly zero"""
    rdt = RDT[es]
    for i in range(len(s)):
        base = numpy.ascontiguousarray(got[0] if ref is None else ref[i]).view(rdt)
        assert numpy.isfinite(base).all() and (base != 0).any(), what
        line = numpy.ascontiguousarray(got[i]).view(rdt)
        if i == zero:
            assert (line == 0).all(), what + (i, 'zero line')
        else:
            assert same_bits(line, numpy.ldexp(base, s[i]).astype(rdt)), what + (i, int(s[i]))


@pytest.mark.parametrize('N,es', ALL)
def test_colfft_powers_of_two(be, N, es):
    col_built(be, N, es)
    cdt, B = CDT[es], 2 * tile_width(N, es) + 3
    rs = numpy.random.RandomState(N + es)
    lines, s, zero = scaled_lines(gaussian(rs, N, cdt), es, B)
    src = dev(be, lines.T)                                               # (1, N, B)
    for inverse in (False, True):
        d = src.clone()
        be.colfft(es, inverse, d, 1, N, B, scale=SCALE)
        assert_scaled(host(d, cdt).reshape(N, B).T, s, zero, es, ('colfft', inverse))


@pytest.mark.parametrize('es', [8, 4])
@pytest.mark.parametrize('n', ROWS)
def test_rowfft_powers_of_two(be, n, es):
    row_built(be)
    rdt, cdt, M1 = RDT[es], CDT[es], n // 2 + 1
    nrows, pitch = 19, n // 2 + 8
    rs = numpy.random.RandomState(n + es)
    lines, s, zero = scaled_lines(gaussian(rs, n, rdt), es, nrows)
    buf = numpy.zeros((nrows, 2 * pitch), dtype=rdt)
    buf[:, :n] = lines
    t = torch.from_numpy(buf).reshape(-1).to(be.device)
    be.rowfft(es, False, t, nrows, n, pitch, scale=SCALE)
    assert_scaled(t.cpu().numpy().view(cdt).reshape(nrows, pitch)[:, :M1], s, zero, es, ('r2c',))
    lines, s, zero = scaled_lines(gaussian(rs, M1, cdt), es, nrows)      # (imaginary parts on DC and Nyquist)
    spec = numpy.zeros((nrows, pitch), dtype=cdt)
    spec[:, :M1] = lines
    t = torch.view_as_real(torch.from_numpy(spec)).reshape(-1).to(be.device)
    be.rowfft(es, True, t, nrows, n, pitch, scale=SCALE)
    assert_scaled(t.cpu().numpy().view(rdt).reshape(nrows, 2 * pitch)[:, :n], s, zero, es, ('c2r',))


def PLACES(W, B):
    return [(0, 0), (0, W - 1), (0, W), (1, 2 * W), (1, B - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('N,es', ALL)
def test_colfft_placement_and_isolation(hip, N, es):
    """one fixed line among random ones, in the small batch and in the one of more tiles than CUs, in both forms: the
    same output bits at every place; and with a NaN and a +inf column in the tile of the first place, every finite
    column as without them"""
    be = hip
    col_built(be, N, es)
    cdt, W = CDT[es], tile_width(N, es)
    rs = numpy.random.RandomState(3 * N + es)
    line = gaussian(rs, N, cdt)
    outs = {False: [], True: []}
    for A, B in [(2, 2 * W + 3)] + batches(be, N, es)[:1]:
        assert A >= 2 and B > 2 * W and W >= 4
        x = gaussian(rs, (A, N, B), cdt)
        for a, b in PLACES(W, B):
            x[a, :, b] = line
        bad = x.copy()
        bad[0, :, 1] = complex(float('nan'), float('nan'))
        bad[0, :, 2] = complex(float('inf'), float('inf'))
        finite = numpy.ones((A, B), bool)
        finite[0, 1:3] = False
        src, srcbad = dev(be, x), dev(be, bad)
        for inverse in (False, True):
            def run(s=src):
                d = s.clone()
                be.colfft(es, inverse, d, A, N, B, scale=SCALE)
                return d
            got = host(both_forms(be, run), cdt).reshape(A, N, B)
            assert numpy.isfinite(got).all()
            outs[inverse] += [got[a, :, b].copy() for a, b in PLACES(W, B)]
            # (as integers: the comparison of the two forms is of bits, NaN included)
            other = host(both_forms(be, lambda: run(srcbad).view(torch.int64)), cdt).reshape(A, N, B)
            assert same_bits(other.transpose(0, 2, 1)[finite], got.transpose(0, 2, 1)[finite]), (A, B, inverse)
            assert not numpy.isfinite(other[0, :, 1:3]).any()
    for inverse in (False, True):
        assert len(outs[inverse]) == 10
        for i, o in enumerate(outs[inverse]):
            assert same_bits(o, outs[inverse][0]), (inverse, i)


@pytest.mark.gpu
@pytest.mark.parametrize('es', [8, 4])
@pytest.mark.parametrize('n', ROWS)
def test_rowfft_placement_and_isolation(hip, n, es):
    """a fixed row at rows 0, 1 and nrows - 1 of 5, 19 and 67: the same bits everywhere; a NaN row and a +inf row
    beside them change no finite row"""
    be = hip
    row_built(be)
    rdt, cdt, M1 = RDT[es], CDT[es], n // 2 + 1
    rs = numpy.random.RandomState(5 * n + es)
    fixed = {False: gaussian(rs, n, rdt), True: gaussian(rs, M1, cdt)}
    outs = {False: [], True: []}
    for nrows in (5, 19, 67):
        pitch = n // 2 + 8
        places = [0, 1, nrows - 1]
        finite = numpy.ones(nrows, bool)
        finite[2:4] = False
        for inverse in (False, True):
            if inverse:
                buf = numpy.zeros((nrows, pitch), dtype=cdt)
                buf[:, :M1] = gaussian(rs, (nrows, M1), cdt)
                buf[places, :M1] = fixed[True]
                bad = buf.copy()
                bad[2, :M1] = complex(float('nan'), float('nan'))
                bad[3, :M1] = complex(float('inf'), float('inf'))
            else:
                buf = numpy.zeros((nrows, 2 * pitch), dtype=rdt)
                buf[:, :n] = gaussian(rs, (nrows, n), rdt)
                buf[places, :n] = fixed[False]
                bad = buf.copy()
                bad[2, :n] = float('nan')
                bad[3, :n] = float('inf')

            def run(h):
                t = torch.from_numpy(h.view(rdt)).reshape(-1).to(be.device)
                be.rowfft(es, inverse, t, nrows, n, pitch, scale=SCALE)
                r = t.cpu().numpy().reshape(nrows, 2 * pitch)
                return r[:, :n] if inverse else r[:, :2 * M1]
            got, other = run(buf), run(bad)
            assert numpy.isfinite(got).all()
            outs[inverse] += [got[r].copy() for r in places]
            assert same_bits(other[finite], got[finite]), (nrows, inverse)
            assert not numpy.isfinite(other[2:4]).any()
    for inverse in (False, True):
        assert len(outs[inverse]) == 9
        for i, o in enumerate(outs[inverse]):
            assert same_bits(o, outs[inverse][0]), (inverse, i)


# ---- 3. the fused transfer at its special modes ----------------------------------------------------------------------

NMESH12, BOX = (12, 16), (100.0, 50.0, 70.0)
BLOCKS = {'A': ((0, 0, 0), 12, 9),          # axis 1 whole, the half spectrum of axis 2: index 0, the Nyquist indices
          'B': ((0, 5, 3), 4, 5)}           # 6 and 8, the negative half; B: no zero index, the Nyquist in the middle


def fused_transfers():
    return [('dx1(%d)' % d, Transfer.dx1(d)) for d in range(3)] + \
           [('force(%d)' % d, Transfer.force(d)) for d in (1, 2)] + \
           [('potential', Transfer.potential()), ('laplace+1', Transfer(laplace_pow=1)),
            ('amplitude', Transfer(amplitude=-2.5)),
            ('dx1(2) x -0.5', Transfer(amplitude=-0.5, laplace_pow=-1, grad_dir=2))]


def special_rows(N):
    return [0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1]


def sparse_block(N, n1, n2, cdt):
    """lines along axis 0 that are non-zero at special_rows(N) only: fixed non-dyadic values of magnitude 0.1 .. 10"""
    x = numpy.zeros((N, n1, n2), dtype=cdt)
    c = numpy.arange(n1 * n2).reshape(n1, n2)
    for q, j in enumerate(special_rows(N)):
        t = 1 + q + 6 * c
        x[j] = 0.1 * 100.0 ** ((t * GOLD) % 1) * numpy.exp(1j * (0.3 + 0.7 * t))
    assert x[0, 0, 0] != 0 and 0.1 <= abs(x[special_rows(N)]).min() and abs(x).max() <= 10
    return x


def test_block_geometry():
    """block A holds index 0, both Nyquist indices and the negative half of axis 1; block B none of the zeros"""
    (_, i1, i2) = mode_numbers((1, 12, 9), BLOCKS['A'][0], (64,) + NMESH12)
    assert i1.min() == -6 and i1.max() == 5 and 0 in i1 and i2.min() == -8 and 0 in i2
    (_, i1, i2) = mode_numbers((1, 4, 5), BLOCKS['B'][0], (64,) + NMESH12)
    assert list(i1.reshape(-1)) == [5, -6, -5, -4] and list(i2.reshape(-1)) == [3, 4, 5, 6, 7]


@pytest.mark.parametrize('N,es', ALL)
def test_colfft_fused_transfer_elements(be, N, es):
    col_built(be, N, es)
    cdt, u = CDT[es], U[es]
    nmesh = (N,) + NMESH12
    J = special_rows(N)
    P = phases(J, N, True)                                               # (6, N)
    if be.name == 'hip':                                                 # the finite difference along axis 0: not fusable
        x = sparse_block(N, 12, 9, cdt)
        assert not Transfer.force(0).fusable()
        with pytest.raises(PmxError):
            be.colfft(es, True, dev(be, x), 1, N, 108, transfer=Transfer.force(0)._cstruct(), n1=12, n2=9,
                      start=(0, 0, 0), nmesh=nmesh, boxsize=BOX)
    for blk, (start, n1, n2) in sorted(BLOCKS.items()):
        x = sparse_block(N, n1, n2, cdt)
        xs = x[J].reshape(len(J), -1).astype(CLD)
        src = dev(be, x)
        modes = mode_numbers((N, n1, n2), start, nmesh)
        for name, T in fused_transfers():
            assert T.fusable()
            t = T._cstruct()
            f, gradient, bound = restate(T, (N, n1, n2), start, nmesh, BOX)
            g = xs * f[J].reshape(len(J), -1).astype(LD)
            if gradient:
                g = g * 1j
            want = P.T @ g                                               # (N, columns)
            lim = (((4 * numpy.log2(N) + 2) * u + 1e-14) * bound[J].reshape(len(J), -1).astype(LD) * abs(xs)).sum(axis=0)

            def run():
                d = src.clone()
                be.colfft(es, True, d, 1, N, n1 * n2, transfer=t, n1=n1, n2=n2, start=start, nmesh=nmesh, boxsize=BOX)
                return d
            got = host(both_forms(be, run), cdt).reshape(N, n1, n2)
            err = abs(got.reshape(N, -1).astype(CLD) - want)
            bad = ~(err <= lim[None, :])
            assert not bad.any(), (blk, name, int(bad.sum()), numpy.argwhere(bad)[0], float((err / lim[None, :]).max()))
            if gradient and T.grad_dir > 0:                              # k_d = 0: exact zeros
                zero = modes[T.grad_dir].reshape(-1) == 0
                assert zero.any() == (blk == 'A')
                lines = got[:, zero, :] if T.grad_dir == 1 else got[:, :, zero]
                assert (lines == 0).all(), (blk, name)
    # scaling by powers of two through the fused pass (the factor of dx1(0) = i k_0 / k^2 differs from column to
    # column: every column against itself, unscaled, in a second run)
    start, n1, n2 = BLOCKS['A']
    B = n1 * n2
    lines, s, zero = scaled_lines(gaussian(numpy.random.RandomState(N + es), N, cdt), es, B)
    outs = []
    for x in (numpy.repeat(lines[:1], B, axis=0), lines):
        d = dev(be, x.T)
        be.colfft(es, True, d, 1, N, B, scale=SCALE, transfer=Transfer.dx1(0)._cstruct(), n1=n1, n2=n2, start=start,
                  nmesh=nmesh, boxsize=BOX)
        outs.append(host(d, cdt).reshape(N, B).T)
    assert_scaled(outs[1], s, zero, es, ('fused dx1(0)',), ref=outs[0])


@pytest.mark.parametrize('N,es', ALL)
def test_colfft_roundtrip_is_two_passes(be, N, es):
    """forward x 1/N, transfer, inverse in one kernel: the bits of the two passes, at every length it is built for,
    every fusable form, blocks A and B, both forms; the element-by-element bound of the fused pass then holds for it"""
    col_built(be, N, es)
    unbuilt = set(p for p in ALL if not be.colfft_roundtrip_supported(*p))
    if be.name == 'hip':
        assert unbuilt == set(ALL) - set(LENGTHS) | {(1536, 8), (1280, 8)}
    if (N, es) in unbuilt:
        pytest.skip('the round-trip kernel is not built for this length')
    cdt = CDT[es]
    nmesh = (N,) + NMESH12
    rs = numpy.random.RandomState(7 * N + es)
    for blk, (start, n1, n2) in sorted(BLOCKS.items()):
        B = n1 * n2
        src = dev(be, gaussian(rs, (N, n1, n2), cdt))
        for name, T in fused_transfers():
            t = T._cstruct()
            kw = dict(transfer=t, n1=n1, n2=n2, start=start, nmesh=nmesh, boxsize=BOX)

            def one():
                d = src.clone()
                be.colfft_roundtrip(es, d, N, B, scale=1.0 / N, **kw)
                return d

            def two():
                d = src.clone()
                be.colfft(es, False, d, 1, N, B, scale=1.0 / N)
                be.colfft(es, True, d, 1, N, B, **kw)
                return d
            a, b = both_forms(be, one), both_forms(be, two)
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (blk, name)
