// pmx_pairs_survey.hip — the pair counts whose line of sight is the pair's own: the modes PMX_PAIRS_2D_MIDPOINT and
// PMX_PAIRS_PROJECTED_MIDPOINT of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/surveypairs.py).
//
// What nbodykit's SurveyDataPairCount does on the host with Corrfunc's DDsmu_mocks and DDrppi_mocks.  Which pair is
// counted and in which bin: pair_rule (pmx_pairs_dev.h), in the two midpoint base modes; the sums are those of
// pmx_pairs.hip, rsum adding w sqrt(rp2) in the projected mode.
// The pass is that of pairs_kernel: one lane per slot of the primaries, the walk over the 27 neighbouring cells with
// broadcast loads of the secondaries, the workgroup's histogram in LDS, one global atomic per array and non-zero bin
// at the end (pmx_pairs_dev.h); no barrier beyond the two around the walk.  On top of it, per pair that passes the
// radial prefilter (pair_rule says why it decides nothing): three adds and three subtracts for l, two three-term sums,
// the product t and, in the projected mode, one division.
#include "pmx_pairs_dev.h"

namespace pmx {

template <int MODE, bool WEIGHTED, int SLOTS>
__global__ void __launch_bounds__(PBLOCK) survey_pairs_kernel(PArgs a)
{
    __shared__ uint32_t hcount[SLOTS];
    __shared__ double hrsum[SLOTS];
    __shared__ double hwsum[WEIGHTED ? SLOTS : 1];
    __shared__ PairEdges<MODE, pair_edges_lds<WEIGHTED, SLOTS>()> ed;
    const int tid = threadIdx.x;
    const int used = min(a.nbins, SLOTS);
    pair_hist_zero<WEIGHTED>(hcount, hrsum, hwsum, used, tid);
    pair_edges_init(a, ed, tid);
    __syncthreads();

    PairLane<3> p;
    if (pair_lane(a, (int64_t)blockIdx.x * PBLOCK + tid, p)) {
#pragma unroll
        for (int d = 0; d < 3; d++) p.quarter[d] = 0.25 * a.g.L[d];         // (here, not in pair_lane: see there)
        double w1 = 1.0;
        if (WEIGHTED && a.w1.data) w1 = a.w1.get(p.i, 0);
        const PairLimits lim = pair_limits(a, ed);
        pair_walk(a, p, [&](int32_t s, const double *y, const double *dx) {
            double q;
            int bin;
            if (!pair_rule<3>(a, lim, ed, p.x, y, dx, q, bin)) return;
            if (bin < 0 || bin >= used) return;                    // (never: 0 <= bin < nbins)
            pair_hist_add<WEIGHTED>(a, hcount, hrsum, hwsum, bin, s, w1, sqrt(q));
        });
    }
    __syncthreads();
    pair_hist_flush<WEIGHTED>(a, hcount, hrsum, hwsum, used, tid);
}

template <int MODE> static void survey_launch(const PArgs &a, bool weighted, unsigned grid, hipStream_t st)
{
    const bool big = a.nbins > PAIRS_SLOTS_SMALL;
    with_bool(weighted, [&](auto w) {
        if (big) survey_pairs_kernel<MODE, decltype(w)::value, PAIRS_SLOTS_BIG><<<grid, PBLOCK, 0, st>>>(a);
        else survey_pairs_kernel<MODE, decltype(w)::value, PAIRS_SLOTS_SMALL><<<grid, PBLOCK, 0, st>>>(a);
    });
}

void pairs_survey_launch(const PArgs &a, int mode, bool weighted, unsigned grid, hipStream_t st)
{
    if (mode == PMX_PAIRS_2D_MIDPOINT) survey_launch<PMX_PAIRS_2D_MIDPOINT>(a, weighted, grid, st);
    else survey_launch<PMX_PAIRS_PROJECTED_MIDPOINT>(a, weighted, grid, st);
}

}  // namespace pmx
