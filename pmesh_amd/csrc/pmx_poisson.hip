// pmx_poisson.hip — Poisson-sampled particles from a real mesh (include/pmesh_amd.h: pmx_poisson_rate_sum,
// pmx_poisson_count, pmx_poisson_scan, pmx_poisson_emit; pmesh_amd/mock.py).
//
// Replaces what a caller of the reference does on the host for a mock catalogue (nbodykit's LogNormalCatalog: numpy
// Poisson counts of the mesh, numpy.repeat of the cell coordinates and uniform offsets).  The sampling rule is written
// down in the header: every random number is one Philox4x32-10 call whose counter holds the GLOBAL cell index, so a
// cell's count and the positions of its particles depend on no block, rank or launch shape.  The local cells, in the C
// order of the block, are cut into segments of PMX_POISSON_SEGMENT cells, a constant of the ABI:
//   rate_sum_kernel   the sum of the rates of the block (one double atomic per segment)
//   count_kernel      one lane per cell: the rate, its chunks, one inversion per chunk; the counts, the sum of every
//                     segment (reduced in LDS) and the number of cells whose rate is refused
//   scan_kernel       exclusive scan of the segment sums: one workgroup walks the array (chunk_scan_kernel of
//                     pmx_domain.hip), nothing waits on another workgroup
//   emit_kernel       one workgroup per segment: its counts scanned in LDS, then one lane per PARTICLE — the lane finds
//                     its cell by binary search in the LDS offsets — so consecutive lanes write consecutive rows and a
//                     cell of thousands of particles is shared by the whole workgroup
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

constexpr int QSEG = PMX_POISSON_SEGMENT;       // cells per segment
constexpr int QBLOCK = 256;                     // threads per segment
constexpr int QPER = QSEG / QBLOCK;             // cells per thread
constexpr int QSCAN = 1024;                     // threads of the scan over the segment sums
static_assert(QSEG % QBLOCK == 0 && QPER % 4 == 0, "a thread scans its cells four at a time");

struct Philox {
    uint32_t w[4];
};

// Philox4x32-10 (Salmon et al. 2011) of the counter (c0, c1, c2, c3) under the key (k0, k1)
__device__ __forceinline__ Philox philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    Philox p;
    p.w[0] = c0;
    p.w[1] = c1;
    p.w[2] = c2;
    p.w[3] = c3;
    return p;
}

// the local block in its logical (C) order: the extents of the two fast axes, the start and the mesh (axes beyond ndim:
// extent 1, start 0, N = 1, so that 1-d and 2-d blocks are 3-d blocks with trailing unit axes)
struct QGeom {
    int64_t ncells;
    int64_t start[3], nmesh[3];
    uint32_t n1, n2;
};

// the cell `c` of segment `seg` (local C-order index seg * QSEG + c): its local index per axis.  The first cell of the
// segment is unravelled in 64 bits, uniformly over the workgroup; the cells after it in 32 bits.
struct QBase {
    uint32_t b0, b1, b2;
};
__device__ __forceinline__ QBase seg_base(const QGeom &q, int64_t seg)
{
    const int64_t first = seg * QSEG;
    const int64_t t = first / q.n2;
    QBase b;
    b.b2 = (uint32_t)(first - t * q.n2);
    b.b0 = (uint32_t)(t / q.n1);
    b.b1 = (uint32_t)(t - (int64_t)b.b0 * q.n1);
    return b;
}
__device__ __forceinline__ void seg_cell(const QGeom &q, const QBase &b, uint32_t c, int64_t *idx)
{
    const uint32_t t2 = b.b2 + c, q2 = t2 / q.n2;
    const uint32_t t1 = b.b1 + q2, q1 = t1 / q.n1;
    idx[2] = t2 - q2 * q.n2;
    idx[1] = t1 - q1 * q.n1;
    idx[0] = b.b0 + q1;
}
// the global C-order index of the cell over the mesh
__device__ __forceinline__ uint64_t global_cell(const QGeom &q, const int64_t *idx)
{
    return (uint64_t)(((idx[0] + q.start[0]) * q.nmesh[1] + (idx[1] + q.start[1])) * q.nmesh[2] + (idx[2] + q.start[2]));
}

template <typename T, bool EXP>
__device__ __forceinline__ double cell_rate(const char *x, const BlockStr &xs, const int64_t *idx, double scale,
                                            double bias)
{
    const double v = (double)*(const T *)(x + xs.off(idx));
    return EXP ? scale * exp(bias * v) : scale * v;
}

// the sum of `v` over the workgroup, in thread 0 (a fixed tree: the same sum for the same values)
template <typename V> __device__ __forceinline__ V block_sum(V v, V *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = QBLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

template <typename T, bool EXP>
__global__ void __launch_bounds__(QBLOCK) rate_sum_kernel(QGeom q, const char *__restrict__ x, BlockStr xs,
                                                          double scale, double bias, double *__restrict__ total)
{
    __shared__ double sh[QBLOCK];
    const int64_t seg = blockIdx.x;
    const QBase b = seg_base(q, seg);
    const int64_t left = q.ncells - seg * QSEG;
    double s = 0;
#pragma unroll 4
    for (int i = 0; i < QPER; i++) {
        const uint32_t c = i * QBLOCK + threadIdx.x;
        if (c < left) {
            int64_t idx[3];
            seg_cell(q, b, c, idx);
            s += cell_rate<T, EXP>(x, xs, idx, scale, bias);
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) atomicAdd(total, s);
}

// the count of one cell of rate lam (0 <= lam <= PMX_POISSON_MAX_RATE): the sum of one inversion per chunk
__device__ __forceinline__ uint32_t poisson_draw(double lam, uint64_t g, uint32_t k0, uint32_t k1)
{
    const double nd = ceil(lam / PMX_POISSON_CHUNK_RATE);
    const uint32_t n = nd < 1 ? 1u : (uint32_t)nd;
    const double lj = lam / n;
    const double p0 = exp(-lj);
    uint32_t count = 0;
    for (uint32_t j = 0; j < n; j++) {
        const Philox r = philox((uint32_t)g, (uint32_t)(g >> 32), j, 0u, k0, k1);
        const double u = ((double)(r.w[0] >> 5) * 67108864.0 + (double)(r.w[1] >> 6) + 1.0) * 0x1p-53;
        uint32_t k = 0;
        double p = p0, s = p0;
        while (u > s && k < PMX_POISSON_MAX_STEPS) {
            k += 1;
            p = p * lj / k;
            s += p;
        }
        count += k;
    }
    return count;
}

template <typename T, bool EXP>
__global__ void __launch_bounds__(QBLOCK) count_kernel(QGeom q, const char *__restrict__ x, BlockStr xs, double scale,
                                                       double bias, uint32_t k0, uint32_t k1,
                                                       uint32_t *__restrict__ counts, int64_t *__restrict__ seg_sums,
                                                       int64_t *__restrict__ flagged)
{
    __shared__ int64_t sh[QBLOCK];
    const int64_t seg = blockIdx.x;
    const QBase b = seg_base(q, seg);
    const int64_t first = seg * QSEG, left = q.ncells - first;
    int64_t sum = 0;
    uint32_t bad = 0;
    for (int i = 0; i < QPER; i++) {
        const uint32_t c = i * QBLOCK + threadIdx.x;
        if (c >= left) break;
        int64_t idx[3];
        seg_cell(q, b, c, idx);
        const double lam = cell_rate<T, EXP>(x, xs, idx, scale, bias);
        uint32_t n = 0;
        if (lam >= 0 && lam <= PMX_POISSON_MAX_RATE) n = poisson_draw(lam, global_cell(q, idx), k0, k1);
        else bad += 1;                           // NaN, negative, infinite or too large
        counts[first + c] = n;
        sum += n;
    }
    sum = block_sum(sum, sh);
    if (threadIdx.x == 0) seg_sums[seg] = sum;
    __syncthreads();
    const int64_t nbad = block_sum((int64_t)bad, sh);
    if (threadIdx.x == 0 && nbad) atomicAdd((unsigned long long *)flagged, (unsigned long long)nbad);
}

// exclusive scan in place, the total into *total: one workgroup, tiles of QSCAN sums one after the other
__global__ void __launch_bounds__(QSCAN) scan_kernel(int64_t *__restrict__ sums, int64_t nseg,
                                                     int64_t *__restrict__ total)
{
    __shared__ int64_t sh[QSCAN];
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nseg; base += QSCAN) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < nseg ? sums[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < QSCAN; off <<= 1) {
            const int64_t t = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        const int64_t incl = sh[threadIdx.x];
        if (i < nseg) sums[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == QSCAN - 1) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

template <int NDIM, bool CELL>
__global__ void __launch_bounds__(QBLOCK) emit_kernel(QGeom q, double h0, double h1, double h2, double L0, double L1,
                                                      double L2, uint32_t k0, uint32_t k1,
                                                      const uint32_t *__restrict__ counts,
                                                      const int64_t *__restrict__ seg_offsets, int64_t npart,
                                                      double *__restrict__ pos, int64_t *__restrict__ cell)
{
    __shared__ __align__(16) uint32_t off[QSEG];             // the counts of the segment, then their exclusive scan
    __shared__ uint32_t part[QBLOCK];            // the inclusive scan of the threads' sums
    const int tid = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t first = seg * QSEG, left = q.ncells - first;
    for (int i = 0; i < QPER; i++) {
        const uint32_t c = i * QBLOCK + tid;
        off[c] = c < left ? counts[first + c] : 0u;
    }
    __syncthreads();
    // every thread scans QPER consecutive cells, the threads' sums are scanned across the workgroup
    uint32_t v[QPER];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < QPER; i += 4) {
        const uint4 t = *(const uint4 *)&off[tid * QPER + i];
        v[i] = t.x;
        v[i + 1] = t.y;
        v[i + 2] = t.z;
        v[i + 3] = t.w;
        mine += t.x + t.y + t.z + t.w;
    }
    part[tid] = mine;
    __syncthreads();
    for (int o = 1; o < QBLOCK; o <<= 1) {
        const uint32_t t = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    uint32_t run = part[tid] - mine;
#pragma unroll
    for (int i = 0; i < QPER; i++) {
        off[tid * QPER + i] = run;
        run += v[i];
    }
    const uint32_t total = part[QBLOCK - 1];
    __syncthreads();
    if (total == 0) return;

    const QBase b = seg_base(q, seg);
    const int64_t row0 = seg_offsets[seg];
    for (uint32_t p = tid; p < total; p += QBLOCK) {
        // the last cell c with off[c] <= p: cells without particles share the offset of the next one and are passed
        uint32_t lo = 0, hi = QSEG;
        while (hi - lo > 1) {
            const uint32_t m = (lo + hi) >> 1;
            if (off[m] <= p) lo = m;
            else hi = m;
        }
        int64_t idx[3];
        seg_cell(q, b, lo, idx);
        const uint64_t g = global_cell(q, idx);
        const Philox r = philox((uint32_t)g, (uint32_t)(g >> 32), p - off[lo], 1u, k0, k1);
        const int64_t row = row0 + p;
        if (row >= npart) continue;              // (never, with the counts the offsets were made of)
        double *out = pos + row * NDIM;
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            const double h = d == 0 ? h0 : (d == 1 ? h1 : h2), L = d == 0 ? L0 : (d == 1 ? L1 : L2);
            const double u = ((double)r.w[d] + 0.5) * 0x1p-32;
            double xd = (((double)(idx[d] + q.start[d]) - 0.5) + u) * h;
            if (xd < 0) xd += L;
            if (xd >= L) xd = 0;                 // (-tiny + L rounds to L)
            out[d] = xd;
        }
        if (CELL) cell[row] = (int64_t)g;
    }
}

}  // namespace pmx

using namespace pmx;

// the block in C order, checked
static int poisson_geom(int32_t ndim, const int64_t *shape, const int64_t *start, const int64_t *nmesh, QGeom &q,
                        int64_t *nseg)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    PMX_REQUIRE(shape, PMX_EINVAL, "bad arguments");
    int64_t sh[3];
    q.ncells = 1;
    for (int d = 0; d < 3; d++) {
        const bool on = d < ndim;
        sh[d] = on ? shape[d] : 1;
        q.start[d] = on && start ? start[d] : 0;
        q.nmesh[d] = on && nmesh ? nmesh[d] : sh[d];
        PMX_REQUIRE(sh[d] >= 0 && q.start[d] >= 0 && q.nmesh[d] >= 1 && q.start[d] + sh[d] <= (sh[d] ? q.nmesh[d] : INT64_MAX),
                    PMX_EINVAL, "the block does not lie inside the mesh");
        PMX_REQUIRE(sh[d] < (1ll << 31) - QSEG, PMX_EUNSUPPORTED, "an axis of 2^31 cells or more");
        q.ncells *= sh[d];
    }
    for (int d = 0; d < 3; d++) PMX_REQUIRE(q.nmesh[d] < (1ll << 31), PMX_EUNSUPPORTED, "an axis of 2^31 cells or more");
    q.n1 = (uint32_t)(sh[1] ? sh[1] : 1);
    q.n2 = (uint32_t)(sh[2] ? sh[2] : 1);
    *nseg = (q.ncells + QSEG - 1) / QSEG;
    PMX_REQUIRE(*nseg < (1ll << 31), PMX_EUNSUPPORTED, "more than 2^31 segments");
    return PMX_OK;
}

static int poisson_rate_args(int32_t elsize, const void *x, const int64_t *x_strides, int32_t mode, double scale,
                             double bias)
{
    PMX_REQUIRE(x && x_strides, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(mode == PMX_POISSON_LINEAR || mode == PMX_POISSON_EXP, PMX_EINVAL, "mode must be LINEAR or EXP");
    PMX_REQUIRE(isfinite(scale) && isfinite(bias), PMX_EINVAL, "scale and bias must be finite");
    return PMX_OK;
}

extern "C" int pmx_poisson_rate_sum(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides,
                                    const int64_t *shape, int32_t mode, double scale, double bias, double *total,
                                    void *stream)
{
    QGeom q;
    int64_t nseg;
    int rc = poisson_geom(ndim, shape, nullptr, nullptr, q, &nseg);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(total, PMX_EINVAL, "bad arguments");
    if (nseg == 0) return PMX_OK;
    rc = poisson_rate_args(elsize, x, x_strides, mode, scale, bias);
    if (rc != PMX_OK) return rc;
    const BlockStr xs = make_str(ndim, x_strides);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mode == PMX_POISSON_EXP, [&](auto e) {
            rate_sum_kernel<T, e><<<(unsigned)nseg, QBLOCK, 0, st>>>(q, (const char *)x, xs, scale, bias, total);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_poisson_count(int32_t ndim, int32_t elsize, const void *x, const int64_t *x_strides,
                                 const int64_t *shape, const int64_t *start, const int64_t *nmesh, int32_t mode,
                                 double scale, double bias, uint64_t seed, uint32_t *counts, int64_t *seg_sums,
                                 int64_t *flagged, void *stream)
{
    PMX_REQUIRE(start && nmesh, PMX_EINVAL, "bad arguments");
    QGeom q;
    int64_t nseg;
    int rc = poisson_geom(ndim, shape, start, nmesh, q, &nseg);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(flagged, PMX_EINVAL, "bad arguments");
    if (nseg == 0) return PMX_OK;
    rc = poisson_rate_args(elsize, x, x_strides, mode, scale, bias);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(counts && seg_sums, PMX_EINVAL, "bad arguments");
    const BlockStr xs = make_str(ndim, x_strides);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(mode == PMX_POISSON_EXP, [&](auto e) {
            count_kernel<T, e><<<(unsigned)nseg, QBLOCK, 0, st>>>(q, (const char *)x, xs, scale, bias, k0, k1, counts,
                                                                 seg_sums, flagged);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_poisson_scan(int64_t *seg_sums, int64_t nseg, int64_t *total, void *stream)
{
    PMX_REQUIRE(total && nseg >= 0 && (seg_sums || nseg == 0), PMX_EINVAL, "bad arguments");
    scan_kernel<<<1, QSCAN, 0, (hipStream_t)stream>>>(seg_sums, nseg, total);
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_poisson_emit(int32_t ndim, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                const double *boxsize, uint64_t seed, const uint32_t *counts,
                                const int64_t *seg_offsets, int64_t npart, double *pos, int64_t *cell, void *stream)
{
    PMX_REQUIRE(start && nmesh && boxsize, PMX_EINVAL, "bad arguments");
    QGeom q;
    int64_t nseg;
    const int rc = poisson_geom(ndim, shape, start, nmesh, q, &nseg);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(npart >= 0, PMX_EINVAL, "bad arguments");
    if (nseg == 0 || npart == 0) return PMX_OK;
    PMX_REQUIRE(counts && seg_offsets && pos, PMX_EINVAL, "bad arguments");
    double L[3] = {1, 1, 1}, h[3] = {1, 1, 1};
    for (int d = 0; d < ndim; d++) {
        PMX_REQUIRE(boxsize[d] > 0 && isfinite(boxsize[d]), PMX_EINVAL, "bad boxsize");
        L[d] = boxsize[d];
        h[d] = boxsize[d] / (double)q.nmesh[d];
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    with_count<3>(ndim, [&](auto nd) {
        with_bool(cell != nullptr, [&](auto wc) {
            emit_kernel<nd, wc><<<(unsigned)nseg, QBLOCK, 0, st>>>(q, h[0], h[1], h[2], L[0], L[1], L[2], k0, k1, counts,
                                                                  seg_offsets, npart, pos, cell);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
