// pmx_pairs_rows.hip — the pair counts with one histogram per primary row: the modes PMX_PAIRS_1D_ROWS and
// PMX_PAIRS_PROJECTED_ROWS of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/profiles.py).
//
// What callers do today with a kd-tree on the host, or with one pair count per centre: the radial profile, the
// enclosed mass and Sigma(R) of the rows around every centre.  Which pair is counted and in which bin: pair_rule
// (pmx_pairs_dev.h), in the base modes 1D and PROJECTED; the sums are those of pmx_pairs.hip, with one change: the bin
// of a pair is (i * nr + rbin) * nsub + subbin, i the ROW of the primary.
// The pass: rows_kernel, one wave per slot of the primaries in cell order, four consecutive slots per workgroup (they
// sit in one cell or in adjacent ones and read the same secondaries from cache), the shape of pmx_knn.hip.  Lane nb
// reads the range of slots of the nb-th of the 3^ndim neighbouring cells, clipped to the window [slo, shi) of the
// launch; the ranges laid end to end are walked as one, the lanes striding over them 64 at a time (each finds its cell
// by bisection over a prefix sum held in the lanes; coalesced loads of spos2 within a cell), so a sparse neighbourhood
// does not cost one trip of the wave per cell.  Every pair inside the edges makes one 32-bit integer and one
// (weighted: two) double LDS atomic on the histogram of the wave, which no other wave touches.  64 lanes that add into
// a few tens of bins, the neighbours in a sorted cell often into the same one, would meet on one address: the wave
// keeps `copies` histograms, the largest power of two with copies * nbins <= 256 (at most ROWS_COPIES_MAX), and the
// lane adds into the copy lane % copies; the slot of (bin, copy) is bin * copies + copy, so the copies of one bin lie
// in consecutive banks.  At its end the wave sums the copies of every bin and adds the non-zero bins to the row's bins
// in global memory with plain loads and stores: it is the only writer of that row in this launch, and the launches of
// one call follow each other on one stream.  No global atomic; one barrier, behind the load of the edge tables.
#include "pmx_pairs_dev.h"

#ifndef PMX_ROWS_COPIES_MAX
#define PMX_ROWS_COPIES_MAX 16                   // (an experiment build with -DPMX_ROWS_COPIES_MAX=1 has one histogram)
#endif

namespace pmx {

constexpr int RBLOCK = PBLOCK;                   // (pair_edges_init strides by PBLOCK)
constexpr int RWAVES = RBLOCK / 64;              // primaries per workgroup
constexpr int RSLOTS = PMX_PAIRS_ROWS_MAX_BINS;  // bins x copies of one wave: 4 x 256 x 12 (weighted: 20) bytes = 12 / 20 KB
constexpr int ROWS_COPIES_MAX = PMX_ROWS_COPIES_MAX;

template <int NDIM, int MODE, bool WEIGHTED>
__global__ void __launch_bounds__(RBLOCK) rows_kernel(PArgs a, int copies)
{
    constexpr int BASE = MODE == PMX_PAIRS_PROJECTED_ROWS ? PMX_PAIRS_PROJECTED : PMX_PAIRS_1D;
    __shared__ uint32_t hcount[RWAVES][RSLOTS];
    __shared__ double hrsum[RWAVES][RSLOTS];
    __shared__ double hwsum[WEIGHTED ? RWAVES : 1][WEIGHTED ? RSLOTS : 1];
    __shared__ PairEdges<BASE> ed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *hc = hcount[wave];
    double *hr = hrsum[wave], *hw = hwsum[WEIGHTED ? wave : 0];
    const int used = min(a.nbins * copies, RSLOTS);
    for (int s = lane; s < used; s += 64) {
        hc[s] = 0;
        hr[s] = 0;
        if (WEIGHTED) hw[s] = 0;
    }
    pair_edges_init(a, ed, tid);
    __syncthreads();                                             // (the only barrier: every wave has come here)

    PairLane<NDIM> p;                                            // (of the whole wave)
    if (!pair_lane(a, (int64_t)blockIdx.x * RWAVES + wave, p)) return;
    const FGeom &g = a.g;
#pragma unroll
    for (int d = 0; d < NDIM; d++) p.quarter[d] = 0.25 * g.L[d];   // (here, not in pair_lane: see there)
    const int32_t i = p.i;
    double w1 = 1.0;
    if (WEIGHTED && a.w1.data) w1 = a.w1.get(i, 0);
    const PairLimits lim = pair_limits(a, ed);
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
    // one slot s of the secondaries against the row of this wave
    auto visit = [&](int32_t s) {
        double y[NDIM], dx[NDIM], q;
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            y[d] = a.spos2[(int64_t)s * NDIM + d];
            dx[d] = pair_image(p.x[d] - y[d], g.L[d], p.quarter[d]);
        }
        int bin;
        if (!pair_rule<NDIM>(a, lim, ed, p.x, y, dx, q, bin)) return;
        if (bin < 0 || bin >= a.nbins) return;                   // (never: 0 <= bin < nbins)
        const int slot = bin * copies + copy;
        if (slot >= used) return;                                // (never: copies * nbins <= RSLOTS)
        pair_hist_add<WEIGHTED>(a, hc, hr, hw, slot, s, w1, sqrt(q));
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
        if (t < total && s >= a.slo && s < a.shi) visit(s);      // (s in the window: always, where t < total)
    }
    // the histogram belongs to this wave: its atomics are in order before its loads, and no lane of another wave
    // touches them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int nb = min(a.nbins, used / copies);
    for (int b = lane; b < nb; b += 64) {
        unsigned long long n = 0;
        double r = 0, w = 0;
        for (int k = 0; k < copies; k++) {
            n += hc[b * copies + k];
            r += hr[b * copies + k];
            if (WEIGHTED) w += hw[b * copies + k];
        }
        if (n == 0) continue;
        const int64_t o = (int64_t)i * a.nbins + b;
        a.npairs[o] += n;
        a.wnpairs[o] += WEIGHTED ? w : (double)n;
        a.rsum[o] += r;
    }
}

template <int NDIM, int MODE> static void rows_launch(const PArgs &a, bool weighted, hipStream_t st)
{
    int copies = 1;
    while (copies < ROWS_COPIES_MAX && 2 * copies * a.nbins <= RSLOTS) copies *= 2;
    const unsigned grid = (unsigned)((a.n1 + RWAVES - 1) / RWAVES);
    with_bool(weighted, [&](auto w) { rows_kernel<NDIM, MODE, decltype(w)::value><<<grid, RBLOCK, 0, st>>>(a, copies); });
}

void pairs_rows_launch(const PArgs &a, int ndim, int mode, bool weighted, hipStream_t st)
{
    if (a.nbins < 1 || a.nbins > RSLOTS) return;                 // (never: pmx_pair_counts has checked it)
    if (mode == PMX_PAIRS_PROJECTED_ROWS) rows_launch<3, PMX_PAIRS_PROJECTED_ROWS>(a, weighted, st);
    else with_count<3>(ndim, [&](auto nd) { rows_launch<decltype(nd)::value, PMX_PAIRS_1D_ROWS>(a, weighted, st); });
}

}  // namespace pmx
