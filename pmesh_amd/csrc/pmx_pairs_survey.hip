// pmx_pairs_survey.hip — the pair counts whose line of sight is the pair's own: the modes PMX_PAIRS_2D_MIDPOINT and
// PMX_PAIRS_PROJECTED_MIDPOINT of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/surveypairs.py).
//
// What nbodykit's SurveyDataPairCount does on the host with Corrfunc's DDsmu_mocks and DDrppi_mocks.  The rule,
// restated from the header, on top of that of pmx_pairs.hip (double arithmetic, every operation rounded once, squared
// edges, no square root choosing a bin, exact npairs, double sums in no particular order):
//   observer  the centre of the box, o_d = L_d / 2.  For wrapped rows w_i, w_j: dx_d as in pmx_pairs.hip;
//             l_d = (w_i,d + w_j,d) - L_d, two roundings: twice the offset of the midpoint from the observer
//             p = dx_0 l_0 + dx_1 l_1 + dx_2 l_2, l2 = l_0^2 + l_1^2 + l_2^2, r2 = dx_0^2 + dx_1^2 + dx_2^2, each sum in
//             that order; p2 = p * p
//   2D        the r-bin from q = r2; t = r2 * l2; the mu-bin is the number of k in 1 .. nsub - 1 with
//             p2 >= sub[k] * t, sub[k] = muedges[k]^2; t == 0 goes to mu-bin 0
//   projected pi2 = p2 / l2, 0 where l2 == 0; rp2 = r2 - pi2, 0 where that is negative; the r-bin from q = rp2;
//             sub[k] = piedges[k]^2; the pi-bin is the number of k in 1 .. nsub - 1 with pi2 >= sub[k];
//             pi2 >= sub[nsub] is not counted; rsum adds w sqrt(rp2)
// The pass is that of pairs_kernel: one lane per slot of the primaries, the walk over the 27 neighbouring cells with
// broadcast loads of the secondaries, the workgroup's histogram in LDS, one global atomic per array and non-zero bin
// at the end (pmx_pairs_dev.h); no barrier beyond the two around the walk.  On top of it, per pair that passes the
// radial prefilter: three adds and three subtracts for l, two three-term sums, the product t and, in the projected
// mode, one division.  The prefilter of the projected mode is r2 <= e2[nr] + sub[nsub]: a counted pair has
// rp2 = fl(r2 - pi2) < e2[nr] and pi2 < sub[nsub], hence r2 < e2[nr] + sub[nsub] in real numbers and r2 <= the rounded
// sum, the rounding being monotone; it decides nothing, it only spares the arithmetic.
#include "pmx_pairs_dev.h"

namespace pmx {

template <int MODE, bool WEIGHTED, int SLOTS>
__global__ void __launch_bounds__(PBLOCK) survey_pairs_kernel(PArgs a)
{
    __shared__ uint32_t hcount[SLOTS];
    __shared__ double hrsum[SLOTS];
    __shared__ double hwsum[WEIGHTED ? SLOTS : 1];
    constexpr int EL = pair_edges_lds<WEIGHTED, SLOTS>();
    __shared__ double se2[EL + 1];
    __shared__ double ssub[EL + 1];
    const int tid = threadIdx.x;
    const int used = min(a.nbins, SLOTS);
    pair_hist_zero<WEIGHTED>(hcount, hrsum, hwsum, used, tid);
    const bool e_lds = EL > 0 && a.nr <= EL, s_lds = EL > 0 && a.nsub <= EL;
    if (e_lds) pair_edges_load(se2, a.e2, a.nr, tid);
    if (s_lds) pair_edges_load(ssub, a.sub, a.nsub, tid);
    __syncthreads();

    const int64_t k = (int64_t)blockIdx.x * PBLOCK + tid;
    int32_t i, flat;
    if (pair_primary(a, k, i, flat)) {
        const FGeom &g = a.g;
        double x[3], quarter[3];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            x[d] = a.spos1[k * 3 + d];
            quarter[d] = 0.25 * g.L[d];
        }
        double w1 = 1.0;
        if (WEIGHTED && a.w1.data) w1 = a.w1.get(i, 0);
        const double qlo = a.e2[0], qhi = a.e2[a.nr];
        const double pi2max = a.sub[a.nsub];
        const double pre = MODE == PMX_PAIRS_PROJECTED_MIDPOINT ? qhi + pi2max : qhi;
        int32_t c[3];
        fof_cell_axes<3>(g, flat, c);
        pair_walk<3>(a, c, x, quarter, [&](int32_t s, const double *y, const double *dx) {
            const double r2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2];
            if (MODE == PMX_PAIRS_2D_MIDPOINT) {
                if (!(r2 >= qlo && r2 < qhi)) return;
            } else {
                if (!(r2 <= pre)) return;
            }
            double l[3];
#pragma unroll
            for (int d = 0; d < 3; d++) l[d] = (x[d] + y[d]) - g.L[d];
            const double p = (dx[0] * l[0] + dx[1] * l[1]) + dx[2] * l[2];
            const double l2 = (l[0] * l[0] + l[1] * l[1]) + l[2] * l[2];
            const double p2 = p * p;
            double q = r2;
            int m = 0;
            if (MODE == PMX_PAIRS_2D_MIDPOINT) {
                const double t = r2 * l2;
                if (t != 0) m = s_lds ? pair_mu_bin(ssub, a.nsub, p2, t) : pair_mu_bin(a.sub, a.nsub, p2, t);
            } else {
                const double pi2 = l2 == 0 ? 0.0 : p2 / l2;
                q = r2 - pi2;
                if (q < 0) q = 0;
                if (!(q >= qlo && q < qhi) || !(pi2 < pi2max)) return;
                // (pi2 >= 0 = sub[0] where the edges are the rule's; anything below the first edge goes to bin 0)
                m = s_lds ? pair_bin(ssub, a.nsub, pi2) : pair_bin(a.sub, a.nsub, pi2);
            }
            const int bin = (e_lds ? pair_bin(se2, a.nr, q) : pair_bin(a.e2, a.nr, q)) * a.nsub + m;
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
