// pmx_pairs_moments.hip — the moment sums of the sources about every primary row: the mode PMX_PAIRS_MOMENTS |
// PMX_PAIRS_1D_ROWS (517) of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/moments.py).
//
// What callers do today with a kd-tree ball query per halo and numpy outer products: the inertia tensor, the centre of
// mass, the momentum, the kinetic energy and the angular momentum of the rows inside spheres about every centre.
// The rule, restated from the header, on top of that of PMX_PAIRS_1D_ROWS (rows, wrapping, the minimum image dx =
// centre - source, q = sum_d dx_d^2 in ascending d, double arithmetic, every operation rounded once, no square root
// choosing a bin, exact npairs, no row identity):
//   columns  weight1 = (w_i, s2_i), s2_i the square of the centre's scale; weight2 = (m_j) or (m_j, v_0 .. v_{ndim-1})
//   bins     E_k = e2[k] * s2_i, one rounding; the pair is in bin k when E_k <= q < E_{k+1}; nr <= 64
//   sums     with m = w_i * m_j and s_d = -dx_d, per (row i, bin b): npairs += 1, wnpairs += m, and
//            rsum[(i * nr + b) * NS + k] += m sqrt(q) | m s_d | m s_a s_b (a <= b: 00 01 02 11 12 22) | the same over q
//            (0 where q == 0) | with velocities: m v_d | m sum_d v_d^2 | m (s x v)
// The pass is that of rows_kernel (pmx_pairs_rows.hip): one wave per slot of the primaries in cell order, RWAVES of
// them per workgroup, lane nb holding the range of slots of the nb-th neighbouring cell inside the window of the
// launch, the ranges laid end to end and walked 64 slots at a time; at its end the wave adds the non-zero bins to its
// row's bins in global memory with plain loads and stores.  No global atomic.  What differs:
//   - the wave keeps its own scaled edges E in LDS, built once s2_i is read, so there is no barrier of the workgroup
//     at all: nothing in LDS is shared between waves;
//   - the histogram of the wave holds a 32-bit count and 1 + NS doubles per slot (m first), component by component
//     over MSLOTS = 64 slots: slot = bin * copies + lane % copies, copies the largest power of two with copies * nr <=
//     64 (at most MOMENTS_COPIES_MAX), so that the lanes of a stride that fall into one bin meet on `copies` addresses
//     in consecutive banks;
//   - a source's columns are read only after the pair has passed the edge tests, and the one division (m / q, shared
//     by the terms of the reduced tensor) and the square root are taken only then.
// The form kept: one 32-bit and 1 + NS double LDS atomics per counted pair.  The other candidate, summing the lanes
// that fall into one bin across the wave before one lane adds (sums_kernel of pmx_fof.hip), is what an experiment
// build with -DPMX_MOMENTS_REDUCE=1 has; DESIGN.md 5.7 has the measurements of both.
#include "pmx_pairs_dev.h"

#ifndef PMX_MOMENTS_REDUCE
#define PMX_MOMENTS_REDUCE 0
#endif
#ifndef PMX_MOMENTS_COPIES_MAX
#define PMX_MOMENTS_COPIES_MAX 16
#endif

namespace pmx {

constexpr int MBLOCK = PBLOCK;
constexpr int MWAVES = MBLOCK / 64;              // primaries per workgroup, as in rows_kernel
constexpr int MSLOTS = PMX_PAIRS_MOMENTS_MAX_BINS;   // bins x copies of one wave
constexpr int MOMENTS_COPIES_MAX = PMX_MOMENTS_COPIES_MAX;

// the sums of rsum per (row, bin): 16 or 23 in three dimensions, 9 or 13 in two
template <int NDIM, bool VEL> constexpr int moments_sums()
{
    return 1 + NDIM + NDIM * (NDIM + 1) + (VEL ? NDIM + 1 + (NDIM == 3 ? 3 : 1) : 0);
}

__device__ __forceinline__ double moments_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int NDIM, bool VEL>
__global__ void __launch_bounds__(MBLOCK) moments_kernel(PArgs a, int copies)
{
    constexpr int NS = moments_sums<NDIM, VEL>();
    constexpr int NV = 1 + NS;                   // m and the sums of rsum
    __shared__ uint32_t hcount[MWAVES][MSLOTS];
    __shared__ double hsum[MWAVES][NV][MSLOTS];  // 4 x 24 x 64 x 8 = 48 KB in three dimensions with velocities
    __shared__ double sedge[MWAVES][MSLOTS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *hc = hcount[wave];
    double(*hs)[MSLOTS] = hsum[wave];
    double *E = sedge[wave];
    const int nr = min(a.nr, MSLOTS);                            // (a.nr itself: pmx_pair_counts has checked it)
    const int used = min(nr * copies, MSLOTS);

    PairLane<NDIM> p;                                            // (of the whole wave)
    if (!pair_lane(a, (int64_t)blockIdx.x * MWAVES + wave, p)) return;
    const FGeom &g = a.g;
#pragma unroll
    for (int d = 0; d < NDIM; d++) p.quarter[d] = 0.25 * g.L[d];   // (here, not in pair_lane: see there)
    const int32_t i = p.i;
    const double w1 = a.w1.get(i, 0), s2 = a.w1.get(i, 1);
    // the histogram and the scaled edges of this wave, which no other wave touches
    for (int s = lane; s < used; s += 64) {
        hc[s] = 0;
#pragma unroll
        for (int m = 0; m < NV; m++) hs[m][s] = 0;
    }
    for (int s = lane; s <= nr; s += 64) E[s] = a.e2[s] * s2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const double qlo = E[0], qhi = E[nr];
    const int copy = lane & (copies - 1);

    pair_lane_cell(a, p);

    constexpr int NB = fof_neighbours<NDIM>();
    // lane nb < NB holds the slots of the nb-th neighbouring cell inside the window of this launch
    int32_t first = 0, len = 0;
    if (lane < NB) {
        int32_t cell;
        if (fof_neighbour<NDIM>(g, p.c, lane, cell)) {
            const int32_t s0 = max(a.cell_start2[cell], a.slo), s1 = min(a.cell_start2[cell + 1], a.shi);
            if (s1 > s0) {
                first = s0;
                len = s1 - s0;
            }
        }
    }
    // end[l]: the slots of the cells 0 .. l.  The cells are distinct, so the total is at most shi - slo <= 2^23.
    uint32_t end = (uint32_t)len;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t v = __shfl_up(end, o, 64);
        if (lane >= o) end += v;
    }
    const uint32_t total = __shfl(end, 31, 64);
    // one slot s of the secondaries against the row of this wave: its bin, or -1, and the NV terms of a counted pair
    auto visit = [&](int32_t s, double *t) -> int {
        double dx[NDIM], q = 0;
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            dx[d] = pair_image(p.x[d] - a.spos2[(int64_t)s * NDIM + d], g.L[d], p.quarter[d]);
            q += dx[d] * dx[d];
        }
        if (!(q >= qlo && q < qhi)) return -1;
        const int bin = pair_bin(E, nr, q);
        if (bin < 0 || bin >= nr) return -1;                     // (never: 0 <= bin < nr)
        const int32_t j = a.order2[s];
        if (j < 0 || j >= a.n2) return -1;                       // (never, with the order fill_kernel left)
        const double m = w1 * a.w2.get(j, 0);
        const double mq = q > 0 ? m / q : 0.0;
        double sv[NDIM];
        int k = 0;
        t[k++] = m;
        t[k++] = m * sqrt(q);
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            sv[d] = -dx[d];                                      // the source as seen from the centre
            t[k++] = m * sv[d];
        }
#pragma unroll
        for (int c = 0; c < NDIM; c++)
#pragma unroll
            for (int e = c; e < NDIM; e++) t[k++] = (m * sv[c]) * sv[e];
#pragma unroll
        for (int c = 0; c < NDIM; c++)
#pragma unroll
            for (int e = c; e < NDIM; e++) t[k++] = (mq * sv[c]) * sv[e];
        if constexpr (VEL) {
            double v[NDIM], v2 = 0;
#pragma unroll
            for (int d = 0; d < NDIM; d++) {
                v[d] = a.w2.get(j, 1 + d);
                v2 += v[d] * v[d];
                t[k++] = m * v[d];
            }
            t[k++] = m * v2;
            if constexpr (NDIM == 3) {
                t[k++] = m * (sv[1] * v[2] - sv[2] * v[1]);
                t[k++] = m * (sv[2] * v[0] - sv[0] * v[2]);
                t[k++] = m * (sv[0] * v[1] - sv[1] * v[0]);
            } else {
                t[k++] = m * (sv[0] * v[1] - sv[1] * v[0]);
            }
        }
        return bin;
    };
    // the ranges of the cells laid end to end are walked as one, 64 slots at a time: a stride may span several cells,
    // and an empty cell costs nothing
    for (uint32_t t0 = 0; t0 < total; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        // the cell of t: the first l with t < end[l], by bisection over the 32 lanes (every lane takes part)
        int l = 0;
#pragma unroll
        for (int step = 16; step > 0; step >>= 1) {
            if (t >= __shfl(end, l + step - 1, 64)) l += step;
        }
        const int32_t s = (int32_t)((uint32_t)__shfl(first, l, 64) + (t - (__shfl(end, l, 64) - (uint32_t)__shfl(len, l, 64))));
        double term[NV];
        int bin = -1;
        if (t < total && s >= a.slo && s < a.shi) bin = visit(s, term);   // (s in the window: always, where t < total)
#if PMX_MOMENTS_REDUCE
        // the bins of the stride one after the other (the loop is uniform over the wave): the lanes of the bin sum
        // their terms, the first of them adds the sums; one copy of the histogram
        unsigned long long todo = __ballot(bin >= 0);
        while (todo) {
            const int src = __ffsll(todo) - 1;
            const int lead = __shfl(bin, src, 64);
            const bool mine = bin == lead;
            const unsigned long long who = __ballot(mine);
            todo &= ~who;
            if (lane == src) hc[lead * copies] += (uint32_t)__popcll(who);
#pragma unroll
            for (int m = 0; m < NV; m++) {
                const double sum = moments_wave_sum(mine ? term[m] : 0.0);
                if (lane == src) hs[m][lead * copies] += sum;
            }
        }
#else
        if (bin >= 0) {
            const int slot = bin * copies + copy;
            if (slot < used) {                                   // (always: copies * nr <= MSLOTS)
                atomicAdd(&hc[slot], 1u);
#pragma unroll
                for (int m = 0; m < NV; m++) atomicAdd(&hs[m][slot], term[m]);
            }
        }
#endif
    }
    // the histogram belongs to this wave: its atomics are in order before its loads, and no lane of another wave
    // touches them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int nb = min(nr, used / copies);
    for (int b = lane; b < nb; b += 64) {
        unsigned long long n = 0;
        for (int k = 0; k < copies; k++) n += hc[b * copies + k];
        if (n == 0) continue;
        const int64_t o = (int64_t)i * a.nr + b;
        a.npairs[o] += n;
#pragma unroll
        for (int m = 0; m < NV; m++) {
            double v = 0;
            for (int k = 0; k < copies; k++) v += hs[m][b * copies + k];
            if (m == 0) a.wnpairs[o] += v;
            else a.rsum[o * NS + (m - 1)] += v;
        }
    }
}

void pairs_moments_launch(const PArgs &a, int ndim, bool vel, hipStream_t st)
{
    // (never: pmx_pair_counts has checked all of it)
    if (a.nr < 1 || a.nr > MSLOTS || a.nsub != 1 || ndim < 2 || ndim > 3 || !a.w1.data || !a.w2.data) return;
    int copies = 1;
    while (copies < MOMENTS_COPIES_MAX && 2 * copies * a.nr <= MSLOTS) copies *= 2;
    const unsigned grid = (unsigned)((a.n1 + MWAVES - 1) / MWAVES);
    with_bool(vel, [&](auto v) {
        if (ndim == 3) moments_kernel<3, decltype(v)::value><<<grid, MBLOCK, 0, st>>>(a, copies);
        else moments_kernel<2, decltype(v)::value><<<grid, MBLOCK, 0, st>>>(a, copies);
    });
}

}  // namespace pmx
