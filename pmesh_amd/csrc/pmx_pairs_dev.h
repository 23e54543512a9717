// pmx_pairs_dev.h — what the pair-count kernels of pmx_pairs*.hip share: the arguments of a launch, the rule that says
// whether a pair is counted and in which bin (pair_rule), the edge tables in LDS, the lane's primary, the walk of one
// lane over the 3^ndim neighbouring cells of its row in the secondaries, and the workgroup's histogram in LDS (its
// set-up, the atomics of one pair, its flush).  pairs_kernel, survey_pairs_kernel and rows_kernel are built on all of
// it; vel_kernel, labels_kernel and align_kernel use the arguments, pair_primary, the walk and the bin searches, and
// state the rule themselves, as they did before pair_rule: on top of it they measured 0.1 to 2.6 % slower.
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

// the edge tables of a workgroup in LDS, of up to EL bins along an axis (EL == 0: none, both are searched in global
// memory); `sub` where the base mode has a sub axis
template <int BASE, int EL = PAIRS_EDGES_LDS> struct PairEdges {
    double e2[EL + 1];
    double sub[BASE == PMX_PAIRS_1D ? 1 : EL + 1];
};

// what a lane holds of the edges: which tables are in LDS, the outer edges of q, the outer edge of the sub axis
// (projected modes) and the radial prefilter of PMX_PAIRS_PROJECTED_MIDPOINT
struct PairLimits {
    bool e_lds, s_lds;
    double qlo, qhi, submax, pre;
};

// the tables copied to LDS where they fit (the caller's barrier follows)
template <int BASE, int EL>
__device__ __forceinline__ void pair_edges_init(const PArgs &a, PairEdges<BASE, EL> &ed, int tid)
{
    if (EL > 0 && a.nr <= EL)
        for (int s = tid; s <= a.nr; s += PBLOCK) ed.e2[s] = a.e2[s];
    if (BASE != PMX_PAIRS_1D && EL > 0 && a.nsub <= EL)
        for (int s = tid; s <= a.nsub; s += PBLOCK) ed.sub[s] = a.sub[s];
}

// the limits of this launch, read by a lane that has a primary, behind its own loads and just before its walk: where
// the kernels had them before they shared this (read before the barrier they cost the velocity kernels 0.1 to 0.8 %)
template <int BASE, int EL>
__device__ __forceinline__ PairLimits pair_limits(const PArgs &a, const PairEdges<BASE, EL> &)
{
    constexpr bool PROJ = BASE == PMX_PAIRS_PROJECTED || BASE == PMX_PAIRS_PROJECTED_MIDPOINT;
    PairLimits lim;
    lim.e_lds = EL > 0 && a.nr <= EL;
    lim.s_lds = EL > 0 && a.nsub <= EL;
    lim.qlo = a.e2[0];
    lim.qhi = a.e2[a.nr];
    lim.submax = PROJ ? a.sub[a.nsub] : 0.0;
    lim.pre = BASE == PMX_PAIRS_PROJECTED_MIDPOINT ? lim.qhi + lim.submax : lim.qhi;
    return lim;
}

// The rule of every mode of pmx_pair_counts (include/pmesh_amd.h), by its base mode.  Whether the pair of the wrapped
// rows x (primary) and y (secondary) with the minimum image dx of x - y is counted, its bin, and q, whose root rsum
// adds.  All arithmetic in double, every operation rounded once (-ffp-contract=off); the edges are squared on the
// host and no square root chooses a bin; the order of the operations below is part of the rule.
//   1D, 2D     q = r2 = sum_d dx_d^2 from 0 in ascending d; counted when e2[0] <= q < e2[nr]; the r-bin k has
//              e2[k] <= q < e2[k + 1]
//   2D         the mu-bin is the number of k in 1 .. nsub - 1 with dx_los^2 >= sub[k] * r2, sub[k] = muedges[k]^2;
//              r2 == 0 goes to mu-bin 0
//   PROJECTED  q = rp2, the sum without d = los; sub = piedges: |dx_los| >= sub[nsub] is not counted, the pi-bin is
//              the number of k in 1 .. nsub - 1 with |dx_los| >= sub[k]
//   midpoint   the observer is the centre of the box: l_d = (x_d + y_d) - L_d, two roundings, twice the offset of the
//              pair's midpoint from it; r2, p = dx . l and l2 = l . l each as (t0 + t1) + t2; p2 = p * p
//   2D_MIDPOINT         q = r2; t = r2 * l2; the mu-bin is the number of k with p2 >= sub[k] * t; t == 0 goes to 0
//   PROJECTED_MIDPOINT  pi2 = p2 / l2, 0 where l2 == 0; q = rp2 = r2 - pi2, 0 where that is negative;
//                       sub[k] = piedges[k]^2: pi2 >= sub[nsub] is not counted, the pi-bin is the number of k with
//                       pi2 >= sub[k].  Before any of it, r2 <= e2[nr] + sub[nsub] is required: a counted pair has
//                       rp2 = fl(r2 - pi2) < e2[nr] and pi2 < sub[nsub], hence r2 < e2[nr] + sub[nsub] in real
//                       numbers and r2 <= the rounded sum, the rounding being monotone; the test decides nothing, it
//                       only spares the arithmetic.
// bin = r-bin * nsub + sub-bin.  dx may have NDIM entries only: the index of dx_los never passes NDIM - 1.
template <int NDIM, int BASE, int EL>
__device__ __forceinline__ bool pair_rule(const PArgs &a, const PairLimits &lim, const PairEdges<BASE, EL> &ed,
                                          const double *x, const double *y, const double *dx, double &q, int &bin)
{
    q = 0;
    int m = 0;
    if constexpr (BASE == PMX_PAIRS_2D_MIDPOINT || BASE == PMX_PAIRS_PROJECTED_MIDPOINT) {
        const double r2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2];
        if (BASE == PMX_PAIRS_2D_MIDPOINT) {
            if (!(r2 >= lim.qlo && r2 < lim.qhi)) return false;
        } else {
            if (!(r2 <= lim.pre)) return false;
        }
        double l[3];
#pragma unroll
        for (int d = 0; d < 3; d++) l[d] = (x[d] + y[d]) - a.g.L[d];
        const double p = (dx[0] * l[0] + dx[1] * l[1]) + dx[2] * l[2];
        const double l2 = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];
        const double p2 = p * p;
        q = r2;
        if (BASE == PMX_PAIRS_2D_MIDPOINT) {
            const double t = r2 * l2;
            if (t != 0) m = lim.s_lds ? pair_mu_bin(ed.sub, a.nsub, p2, t) : pair_mu_bin(a.sub, a.nsub, p2, t);
        } else {
            const double pi2 = l2 == 0 ? 0.0 : p2 / l2;
            q = r2 - pi2;
            if (q < 0) q = 0;
            if (!(q >= lim.qlo && q < lim.qhi) || !(pi2 < lim.submax)) return false;
            // (pi2 >= 0 = sub[0] where the edges are the rule's; anything below the first edge goes to bin 0)
            m = lim.s_lds ? pair_bin(ed.sub, a.nsub, pi2) : pair_bin(a.sub, a.nsub, pi2);
        }
    } else {
#pragma unroll
        for (int d = 0; d < NDIM; d++)
            if (BASE != PMX_PAIRS_PROJECTED || d != a.los) q += dx[d] * dx[d];
        if (!(q >= lim.qlo && q < lim.qhi)) return false;
        if constexpr (BASE != PMX_PAIRS_1D) {
            const double z = a.los == 0 ? dx[0] : (a.los == 1 ? dx[NDIM > 1 ? 1 : 0] : dx[NDIM > 2 ? 2 : 0]);
            if (BASE == PMX_PAIRS_2D) {
                const double z2 = z * z;
                if (q > 0) m = lim.s_lds ? pair_mu_bin(ed.sub, a.nsub, z2, q) : pair_mu_bin(a.sub, a.nsub, z2, q);
            } else {
                const double az = fabs(z);
                if (!(az < lim.submax)) return false;
                // (az >= 0 = sub[0], as above)
                m = lim.s_lds ? pair_bin(ed.sub, a.nsub, az) : pair_bin(a.sub, a.nsub, az);
            }
        }
    }
    // an edge table is searched where it lies, in two branches: one pointer chosen at run time would be a flat one,
    // and the reads of LDS flat loads
    bin = lim.e_lds ? pair_bin(ed.e2, a.nr, q) : pair_bin(a.e2, a.nr, q);
    if (BASE != PMX_PAIRS_1D) bin = bin * a.nsub + m;
    return true;
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

// the primary of a lane (rows_kernel: of a wave): its row i, its wrapped position x, the axes c of its cell, and a
// quarter of the box (pair_image)
template <int NDIM> struct PairLane {
    int32_t i, flat, c[3];
    double x[NDIM], quarter[NDIM];
};

// the primary in the slot k of the primaries, or false where there is none.  `quarter` is left to the kernel, which
// fills it in its own body, for the compiler's sake: as long as the kernel itself holds a loop over a member array of
// `a` that is not yet unrolled when the copy of the kernel's argument is taken apart, the members are loaded from the
// argument segment where they are used; with that loop in here, which is unrolled before it is inlined, they are all
// loaded at the kernel's entry and held in SGPRs: 4 more on most kernels, and one wave per SIMD fewer on
// pairs_kernel<3, PROJECTED, false, 1024>.  This rests on the order of SROA, inlining and unrolling in
// the compiler of ROCm 7: compare the kernels' resources with and without the loop in here when the compiler changes.
template <int NDIM> __device__ __forceinline__ bool pair_lane(const PArgs &a, int64_t k, PairLane<NDIM> &p)
{
    if (!pair_primary(a, k, p.i, p.flat)) return false;
#pragma unroll
    for (int d = 0; d < NDIM; d++) p.x[d] = a.spos1[k * NDIM + d];
    return true;
}

// the axes of the primary's cell (rows_kernel, whose lanes read them; pair_walk works them out itself)
template <int NDIM> __device__ __forceinline__ void pair_lane_cell(const PArgs &a, PairLane<NDIM> &p)
{
    fof_cell_axes<NDIM>(a.g, p.flat, p.c);
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

// the same around the primary p
template <int NDIM, typename F> __device__ __forceinline__ void pair_walk(const PArgs &a, const PairLane<NDIM> &p, F &&f)
{
    int32_t c[3];
    fof_cell_axes<NDIM>(a.g, p.flat, c);
    pair_walk<NDIM>(a, c, p.x, p.quarter, f);
}

// the n + 1 edges of an axis copied to LDS (vel_kernel, labels_kernel and align_kernel, which keep their own prologue
// and their own statement of the rule: DESIGN.md 5.7)
__device__ __forceinline__ void pair_edges_load(double *dst, const double *src, int n, int tid)
{
    for (int s = tid; s <= n; s += PBLOCK) dst[s] = src[s];
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

// The launches of one window of the secondaries by the other files (pmx_pair_counts has checked the arguments, the
// bin limit and the columns of w1 and w2 that the header states for the mode, and filled `a`).  ndim: the columns of
// the rows, which `a` does not hold; mode: the mode word of the entry.
void pairs_survey_launch(const PArgs &a, int mode, bool weighted, unsigned grid, hipStream_t st);
void pairs_rows_launch(const PArgs &a, int ndim, int mode, bool weighted, hipStream_t st);   // (one wave per primary)
void pairs_vel_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);
void pairs_labels_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);
void pairs_align_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st);
void pairs_moments_launch(const PArgs &a, int ndim, bool vel, hipStream_t st);               // (one wave per primary)

}  // namespace pmx
