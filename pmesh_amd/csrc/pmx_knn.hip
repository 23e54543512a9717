// pmx_knn.hip — the k nearest sources of every primary inside a radius (include/pmesh_amd.h: pmx_knn;
// pmesh_amd/knn.py).
//
// What callers do today with a kd-tree on the host (nbodykit's KDDensity, MP-Gadget's smoothing lengths, the kNN-CDF
// statistics): a fixed-radius top-k over the cell grid.  The rule, restated from the header:
//   rows        (n, ndim) rows wrapped into [0, L_d) by FoF's rule; dx_d = x_i,d - x_j,d the minimum image of the
//               wrapped rows (pair_image); all arithmetic in double, every operation rounded once; r2 = sum_d dx_d^2
//               accumulated in the order d = 0, 1, 2
//   candidates  source j is a candidate of primary i when r2 < r2max (strict); no square root decides anything
//   result      dist2[i, :] the k smallest candidate r2 ascending, +inf where there are fewer: a multiset, so defined
//               bit for bit whatever the order of the walk; index[i, c] a source with that r2 (the local row, through
//               order2), -1 where inf, distinct within a row, unspecified among ties; count[i] the number of
//               candidates, not capped at k
// The pass: knn_kernel, one wave per slot of the primaries in cell order, four consecutive slots per workgroup (they
// sit in one cell or in adjacent ones and read the same sources from cache).  Lane nb reads the range of slots of the
// nb-th of the 3^ndim neighbouring cells; the ranges laid end to end are walked as one: the lanes of the wave stride
// over them 64 at a time (each finds its cell by bisection over a prefix sum held in the lanes; coalesced loads of
// spos2 within a cell), form dx and r2; count grows by the population of the ballot of r2 < r2max.  A candidate is
// kept when r2 < tau: tau starts at r2max and, once the wave's list holds k finite entries, is the k-th smallest so far
// (strict: a tie with the k-th changes no output value).  The wave compacts what it keeps — (r2, slot), at the place a
// ballot and a prefix count give — into a ring of 128 entries in LDS that belongs to it alone: no LDS atomic, no
// barrier.
// The merge: the best list lives in registers, lane l holding the l-th smallest, padded with +inf.  When the ring
// holds 64 entries, and once at the end, every lane takes one entry; a bitonic network of lane exchanges sorts the 64
// new entries, min(best[l], new[63 - l]) keeps the 64 smallest of both as a bitonic sequence, six merge stages put
// them in order, and tau is read from lane k - 1.  A selection per lane (64 heaps of k entries) would need k registers
// per lane indexed at run time, which is scratch memory, and a k-way merge at the end; here the list costs three
// registers and every exchange is a full-wave operation.  An exchange takes the partner's entry only on a strict
// comparison, so of two entries with equal r2 each lane keeps its own: no entry is lost or doubled.
// At the end lane l < k writes dist2[i, l] and index[i, l], lane 0 the count, through order1: no global atomic.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_cells_dev.h"
#include "pmx_common.h"

namespace pmx {

constexpr int KBLOCK = 256;
constexpr int KWAVES = KBLOCK / 64;              // primaries per workgroup
constexpr int KRING = 128;                       // entries of a wave's ring: at most 63 left over plus 64 new ones

struct KArgs {
    FGeom g;
    int64_t n1, n2, ncells;
    const double *spos1, *spos2;
    const int32_t *order1, *cell_of1, *order2, *cell_start2;
    double r2max;
    int32_t k;
    double *dist2;
    int32_t *index;
    long long *count;
};

// one exchange with the lane `lane ^ j`: this lane keeps the smaller entry of the two (smaller) or the larger; the
// partner decides the opposite on the same two entries, and on a tie both keep their own
__device__ __forceinline__ void knn_exchange(double &v, int32_t &s, int j, bool smaller)
{
    const double ov = __shfl_xor(v, j, 64);
    const int32_t os = __shfl_xor(s, j, 64);
    if (smaller ? ov < v : ov > v) {
        v = ov;
        s = os;
    }
}

template <int NDIM> __global__ void __launch_bounds__(KBLOCK) knn_kernel(KArgs a)
{
    __shared__ double qr[KWAVES][KRING];
    __shared__ int32_t qs[KWAVES][KRING];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * KWAVES + wave;
    if (p >= a.n1) return;                                       // (the whole wave: there is no barrier below)
    const int32_t i = a.order1[p];
    if (i < 0 || i >= a.n1) return;                              // (never, with the order fill_kernel left)
    const int32_t flat = a.cell_of1[i];
    const FGeom &g = a.g;
    double x[NDIM], quarter[NDIM];
#pragma unroll
    for (int d = 0; d < NDIM; d++) {
        x[d] = a.spos1[p * NDIM + d];
        quarter[d] = 0.25 * g.L[d];
    }
    double best = INFINITY;                                      // the l-th smallest so far, in lane l
    int32_t best_slot = -1;
    double tau = a.r2max;                                        // the same in every lane
    long long found = 0;                                         // the same in every lane
    unsigned head = 0, fill = 0;                                 // the ring: its first entry and how many it holds

    // every lane below `live` takes the entry head + lane, the others +inf
    auto merge = [&](unsigned live) {
        double v = INFINITY;
        int32_t s = -1;
        if (lane < (int)live) {
            const unsigned e = (head + lane) & (KRING - 1);
            v = qr[wave][e];
            s = qs[wave][e];
        }
        head = (head + live) & (KRING - 1);
        fill -= live;
        // the new entries ascending over the lanes
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
            for (int j = size >> 1; j > 0; j >>= 1) knn_exchange(v, s, j, ((lane & size) == 0) == ((lane & j) == 0));
        }
        // the 64 smallest of both lists: a bitonic sequence
        const double ov = __shfl(v, 63 - lane, 64);
        const int32_t os = __shfl(s, 63 - lane, 64);
        if (ov < best) {
            best = ov;
            best_slot = os;
        }
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) knn_exchange(best, best_slot, j, (lane & j) == 0);
        tau = fmin(a.r2max, __shfl(best, a.k - 1, 64));
    };

    if (a.n2 > 0 && flat >= 0 && flat < a.ncells) {              // (the cell: always)
        int32_t c[3];
        fof_cell_axes<NDIM>(g, flat, c);
        constexpr int NB = fof_neighbours<NDIM>();
        // lane nb < NB holds the slots of the nb-th neighbouring cell: one load for all of them, not one per cell
        int32_t first = 0, len = 0;
        if (lane < NB) {
            int32_t cell;
            if (fof_neighbour<NDIM>(g, c, lane, cell)) {
                int32_t s0 = a.cell_start2[cell], s1 = a.cell_start2[cell + 1];
                if (s0 < 0) s0 = 0;
                if ((int64_t)s1 > a.n2) s1 = (int32_t)a.n2;
                if (s1 > s0) {
                    first = s0;
                    len = s1 - s0;
                }
            }
        }
        // end[l]: the slots of the cells 0 .. l.  The cells are distinct, so the total is at most n2 < 2^31.
        uint32_t end = (uint32_t)len;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const uint32_t v = __shfl_up(end, o, 64);
            if (lane >= o) end += v;
        }
        const uint32_t total = __shfl(end, 31, 64);
        // the ranges of the cells laid end to end are walked as one, 64 slots at a time: a stride may span several
        // cells, and an empty cell costs nothing.  (The turn at t0 >= total walks nothing and merges what is left:
        // one merge in the code.)
        for (uint32_t t0 = 0;; t0 += 64) {
            const bool last = t0 >= total;
            const uint32_t t = t0 + (uint32_t)lane;
            // the cell of t: the first l with t < end[l], by bisection over the 32 lanes (every lane takes part)
            int l = 0;
#pragma unroll
            for (int step = 16; step > 0; step >>= 1) {
                if (t >= __shfl(end, l + step - 1, 64)) l += step;
            }
            const uint32_t s = (uint32_t)__shfl(first, l, 64) + (t - (__shfl(end, l, 64) - (uint32_t)__shfl(len, l, 64)));
            bool inside = false, keep = false;
            double r2 = 0;
            if (t < total && (int64_t)s < a.n2) {                // (s < n2: always)
#pragma unroll
                for (int d = 0; d < NDIM; d++) {
                    const double dx = pair_image(x[d] - a.spos2[(int64_t)s * NDIM + d], g.L[d], quarter[d]);
                    r2 += dx * dx;
                }
                inside = r2 < a.r2max;
                keep = r2 < tau;
            }
            found += __popcll(__ballot(inside));
            const unsigned long long mask = __ballot(keep);
            if (keep) {
                const unsigned e = (head + fill + __popcll(mask & ((1ull << lane) - 1ull))) & (KRING - 1);
                qr[wave][e] = r2;
                qs[wave][e] = (int32_t)s;
            }
            fill += __popcll(mask);
            // the ring belongs to this wave: its stores are in order before its loads, and no lane of another
            // wave touches them
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const unsigned live = fill >= 64 ? 64u : (last ? fill : 0u);
            if (live) {
                merge(live);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (last) break;
        }
    }
    if (lane < a.k) {
        const int64_t o = (int64_t)i * a.k + lane;
        a.dist2[o] = best;
        if (a.index) a.index[o] = (best_slot >= 0 && (int64_t)best_slot < a.n2) ? a.order2[best_slot] : -1;
    }
    if (lane == 0 && a.count) a.count[i] = found;
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_knn(int32_t ndim, int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1,
                       int64_t n2, const double *spos2, const int32_t *order2, const int32_t *cell_start2,
                       const int64_t *ncell, int32_t periodic, const double *boxsize, double r2max, int32_t k,
                       double *dist2, int32_t *index, int64_t *count, void *stream)
{
    KArgs a;
    const int rc = fof_geom(ndim, boxsize, nullptr, nullptr, ncell, periodic, a.g, &a.ncells);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(n1 >= 0 && n2 >= 0, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(n1 <= PMX_FOF_MAX_ROWS && n2 <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED,
                "more than 2^31 - 1 rows: slots are 32-bit");
    PMX_REQUIRE(k >= 1 && k <= PMX_KNN_MAX_K, PMX_EINVAL, "k must be in 1 .. PMX_KNN_MAX_K");
    PMX_REQUIRE(r2max > 0 && isfinite(r2max), PMX_EINVAL, "r2max must be finite and positive");
    if (n1 == 0) return PMX_OK;
    PMX_REQUIRE(dist2 && spos1 && order1 && cell_of1, PMX_EINVAL, "bad arguments");
    // (without sources the kernel walks nothing and writes the padding: the outputs are overwritten all the same)
    PMX_REQUIRE(n2 == 0 || (spos2 && order2 && cell_start2), PMX_EINVAL, "bad arguments");
    a.n1 = n1;
    a.n2 = n2;
    a.spos1 = spos1;
    a.spos2 = spos2;
    a.order1 = order1;
    a.cell_of1 = cell_of1;
    a.order2 = order2;
    a.cell_start2 = cell_start2;
    a.r2max = r2max;
    a.k = k;
    a.dist2 = dist2;
    a.index = index;
    a.count = (long long *)count;
    const unsigned grid = (unsigned)((n1 + KWAVES - 1) / KWAVES);
    hipStream_t st = (hipStream_t)stream;
    with_count<3>(ndim, [&](auto nd) { knn_kernel<decltype(nd)::value><<<grid, KBLOCK, 0, st>>>(a); });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
