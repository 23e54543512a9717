// pmx_pairs_dev.h — what the pair-count kernels of pmx_pairs.hip (the line of sight along a box axis) and of
// pmx_pairs_survey.hip (the line of sight of the pair itself) share: the arguments of a launch, the workgroup's
// histogram in LDS (its set-up, the atomics of one pair, its flush), the edge tables and the walk of one lane over the
// 3^ndim neighbouring cells of its row in the secondaries.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_cells_dev.h"
#include "pmx_common.h"

namespace pmx {

constexpr int PBLOCK = 256;
constexpr int PAIRS_SLOTS_SMALL = 1024;          // the bins of the histogram of the small form: 12 / 20 KB
constexpr int PAIRS_SLOTS_BIG = PMX_PAIRS_MAX_BINS;   // of the form for many bins: 48 / 80 KB, two workgroups per CU
constexpr int PAIRS_EDGES_LDS = 128;             // up to this many bins along an axis, its edges are searched in LDS
// the secondaries of one launch: 256 lanes x 2^23 slots = 2^31 pairs at most per workgroup and 32-bit count
constexpr int64_t PAIRS_WINDOW = (int64_t)1 << 23;

struct PArgs {
    FGeom g;
    int64_t n1, n2;
    int32_t slo, shi;                            // the slots of the secondaries of this launch
    const double *spos1, *spos2;
    const int32_t *order1, *cell_of1, *order2, *cell_start2;
    DVec w1, w2;
    int64_t ncells;
    int32_t nr, nsub, nbins, los;
    const double *e2, *sub;
    unsigned long long *npairs;
    double *wnpairs, *rsum;
};

// the edges of an axis searched in LDS: none in the weighted form for many bins, which fills its 80 KB with the
// histogram and searches the edges in global memory
template <bool WEIGHTED, int SLOTS> constexpr int pair_edges_lds()
{
    return WEIGHTED && SLOTS > PAIRS_SLOTS_SMALL ? 0 : PAIRS_EDGES_LDS;
}

// the number of k in 1 .. n - 1 with z2 >= tab[k] * r2 (the products do not decrease with k: the test holds for a
// prefix of them)
template <typename P> __device__ __forceinline__ int pair_mu_bin(P tab, int n, double z2, double r2)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (z2 >= tab[mid] * r2) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the histogram of the workgroup zeroed up to `used` bins (the caller's barrier follows)
template <bool WEIGHTED>
__device__ __forceinline__ void pair_hist_zero(uint32_t *hcount, double *hrsum, double *hwsum, int used, int tid)
{
    for (int s = tid; s < used; s += PBLOCK) {
        hcount[s] = 0;
        hrsum[s] = 0;
        if (WEIGHTED) hwsum[s] = 0;
    }
}

// the n + 1 edges of an axis copied to LDS
__device__ __forceinline__ void pair_edges_load(double *dst, const double *src, int n, int tid)
{
    for (int s = tid; s <= n; s += PBLOCK) dst[s] = src[s];
}

// the slot of the primaries of this lane: its row i and flat cell, or false where the lane has none
__device__ __forceinline__ bool pair_primary(const PArgs &a, int64_t k, int32_t &i, int32_t &flat)
{
    i = -1;
    flat = -1;
    if (k < a.n1) i = a.order1[k];
    if (i >= 0 && i < a.n1) flat = a.cell_of1[i];                   // (always, with the order fill_kernel left)
    return flat >= 0 && flat < a.ncells;
}

// f(s, y, dx) for every slot s of the secondaries of this launch in the 3^NDIM cells around c[]: y its wrapped row,
// dx the minimum image of x - y (zero beyond NDIM)
template <int NDIM, typename F>
__device__ __forceinline__ void pair_walk(const PArgs &a, const int32_t c[3], const double *x, const double *quarter,
                                          F &&f)
{
    const FGeom &g = a.g;
    for (int nb = 0; nb < fof_neighbours<NDIM>(); nb++) {
        int32_t cell;
        if (!fof_neighbour<NDIM>(g, c, nb, cell)) continue;
        const int32_t s0 = max(a.cell_start2[cell], a.slo), s1 = min(a.cell_start2[cell + 1], a.shi);
        for (int32_t s = s0; s < s1; s++) {
            double y[3] = {0, 0, 0}, dx[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < NDIM; d++) {
                y[d] = a.spos2[(int64_t)s * NDIM + d];
                dx[d] = pair_image(x[d] - y[d], g.L[d], quarter[d]);
            }
            f(s, y, dx);
        }
    }
}

// one pair of the primary of weight w1 with the slot s of the secondaries at distance r into the bin `slot`
template <bool WEIGHTED>
__device__ __forceinline__ void pair_hist_add(const PArgs &a, uint32_t *hcount, double *hrsum, double *hwsum,
                                              int slot, int32_t s, double w1, double r)
{
    if (WEIGHTED) {
        double w = w1;
        if (a.w2.data) {
            const int32_t j = a.order2[s];
            if (j < 0 || j >= a.n2) return;                         // (never, with the order fill_kernel left)
            w = w1 * a.w2.get(j, 0);
        }
        atomicAdd(&hcount[slot], 1u);
        atomicAdd(&hwsum[slot], w);
        atomicAdd(&hrsum[slot], w * r);
    } else {
        atomicAdd(&hcount[slot], 1u);
        atomicAdd(&hrsum[slot], r);
    }
}

// the histogram of the workgroup added to the global arrays: one atomic per array and non-zero bin (after the
// caller's barrier)
template <bool WEIGHTED>
__device__ __forceinline__ void pair_hist_flush(const PArgs &a, const uint32_t *hcount, const double *hrsum,
                                                const double *hwsum, int used, int tid)
{
    for (int b = tid; b < used; b += PBLOCK) {
        const unsigned long long n = hcount[b];
        if (n == 0) continue;
        atomicAdd(&a.npairs[b], n);
        atomicAdd(&a.wnpairs[b], WEIGHTED ? hwsum[b] : (double)n);
        atomicAdd(&a.rsum[b], hrsum[b]);
    }
}

// pmx_pairs_survey.hip: the launch of one window of the secondaries in the modes PMX_PAIRS_2D_MIDPOINT and
// PMX_PAIRS_PROJECTED_MIDPOINT (pmx_pair_counts has checked the arguments and filled `a`)
void pairs_survey_launch(const PArgs &a, int mode, bool weighted, unsigned grid, hipStream_t st);

// pmx_pairs_rows.hip: the launch of one window of the secondaries in the modes PMX_PAIRS_1D_ROWS and
// PMX_PAIRS_PROJECTED_ROWS, one wave per slot of the primaries (pmx_pair_counts has checked the arguments and filled
// `a`; ndim: the columns of the rows, which `a` does not hold)
void pairs_rows_launch(const PArgs &a, int ndim, int mode, bool weighted, hipStream_t st);

// pmx_pairs_vel.hip: the launch of one window of the secondaries in the modes PMX_PAIRS_1D_VELOCITY,
// PMX_PAIRS_PROJECTED_VELOCITY and PMX_PAIRS_1D_LOS (pmx_pair_counts has checked the arguments and filled `a`: w1 and
// w2 hold the 1 + ndim or 2 columns of the two sets, rsum has 4 * nbins entries)
void pairs_vel_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);

// pmx_pairs_labels.hip: the launch of one window of the secondaries in the modes PMX_PAIRS_SPLIT | m and
// PMX_PAIRS_JACKKNIFE | m, m a base mode (pmx_pair_counts has checked the arguments and filled `a`: w1 and w2 hold the
// columns (w, label) of the two sets, nbins <= PMX_PAIRS_LABEL_SLOTS / 4, the arrays have the lengths of the header)
void pairs_labels_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);

// pmx_pairs_align.hip: the launch of one window of the secondaries in the modes PMX_PAIRS_ALIGN | PMX_PAIRS_1D and
// PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED (pmx_pair_counts has checked the arguments and filled `a`: w1 and w2 hold the
// 1 + ndim or 3 columns of the two sets, nbins <= PMX_PAIRS_ALIGN_MAX_BINS, rsum has 4 or 7 times nbins entries)
void pairs_align_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);

}  // namespace pmx
