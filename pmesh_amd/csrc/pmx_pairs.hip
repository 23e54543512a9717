// pmx_pairs.hip — binned pair counts of particles (include/pmesh_amd.h: pmx_pair_counts; pmesh_amd/paircount.py).
//
// Replaces what a caller of the reference does on the host for xi(r) of a catalogue (nbodykit's SimulationBoxPairCount:
// Corrfunc over the rows copied over PCIe).  The rule, restated from the header:
//   rows     (n, ndim) rows wrapped into [0, L_d) by FoF's rule; dx_d the minimum image of the wrapped rows; all
//            arithmetic in double, every operation rounded once; r2 = sum_d dx_d^2 in the order d = 0, 1, 2
//   edges    a pair is in r-bin k when e2[k] <= q < e2[k + 1], e2 the squared edges formed on the host; q = r2 (1D, 2D)
//            or rp2, the sum of the two dx_d^2 with d != los in ascending d (projected); no square root chooses a bin
//   mu       the mu-bin is the number of k in 1 .. nmu - 1 with dx_los^2 >= m2[k] * r2; r2 == 0 goes to mu-bin 0
//   pi       the pi-bin is the number of k in 1 .. npi - 1 with |dx_los| >= piedges[k]; |dx_los| >= piedges[npi] is
//            not counted
//   sums     npairs exact; wnpairs = sum w1 w2 and rsum = sum w1 w2 sqrt(q) in double, in no particular order
// The pass: pairs_kernel, one lane per slot of the primaries in cell order.  The lane walks the 3^ndim neighbouring
// cells of its row in the secondaries (the walk of link_kernel, pmx_cells_dev.h); the lanes of a wave sit in one cell
// or in adjacent ones, so they read the same secondaries at the same time: broadcast loads from cache.  Every pair
// inside the edges makes one 32-bit integer and one (weighted: two) double LDS atomic on the workgroup's histogram;
// at its end the workgroup makes one global atomic per array and non-zero bin.  (Replicating the histogram over the
// lanes, slot = bin * R + lane % R, so that the lanes of a wave that meet in one outer bin do not meet on one address,
// measured nothing at 20 bins, and neither did removing the LDS atomics altogether: DESIGN.md 5.7.)  No lane waits for
// another: the only barriers are the two around the walk.  The histogram, the walk and the arguments are those of
// pmx_pairs_dev.h; the modes whose line of sight is the pair's own (PMX_PAIRS_2D_MIDPOINT, PMX_PAIRS_PROJECTED_MIDPOINT)
// have their kernels in pmx_pairs_survey.hip and are launched from pmx_pair_counts below, and so are the modes with one
// histogram per primary row (PMX_PAIRS_1D_ROWS, PMX_PAIRS_PROJECTED_ROWS), whose kernels are in pmx_pairs_rows.hip, and
// the modes with pairwise velocity sums (PMX_PAIRS_1D_VELOCITY, PMX_PAIRS_PROJECTED_VELOCITY, PMX_PAIRS_1D_LOS), whose
// kernels are in pmx_pairs_vel.hip, and the modes by row labels (PMX_PAIRS_SPLIT | m, PMX_PAIRS_JACKKNIFE | m), whose
// kernels are in pmx_pairs_labels.hip, and the modes with intrinsic-alignment sums (PMX_PAIRS_ALIGN | PMX_PAIRS_1D,
// PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED), whose kernels are in pmx_pairs_align.hip.
#include "pmx_pairs_dev.h"

namespace pmx {

template <int NDIM, int MODE, bool WEIGHTED, int SLOTS>
__global__ void __launch_bounds__(PBLOCK) pairs_kernel(PArgs a)
{
    __shared__ uint32_t hcount[SLOTS];
    __shared__ double hrsum[SLOTS];
    __shared__ double hwsum[WEIGHTED ? SLOTS : 1];
    constexpr int EL = pair_edges_lds<WEIGHTED, SLOTS>();
    __shared__ double se2[EL + 1];
    __shared__ double ssub[MODE == PMX_PAIRS_1D ? 1 : EL + 1];
    const int tid = threadIdx.x;
    const int used = min(a.nbins, SLOTS);
    pair_hist_zero<WEIGHTED>(hcount, hrsum, hwsum, used, tid);
    const bool e_lds = EL > 0 && a.nr <= EL, s_lds = EL > 0 && a.nsub <= EL;
    if (e_lds) pair_edges_load(se2, a.e2, a.nr, tid);
    if (MODE != PMX_PAIRS_1D && s_lds) pair_edges_load(ssub, a.sub, a.nsub, tid);
    __syncthreads();

    const int64_t k = (int64_t)blockIdx.x * PBLOCK + tid;
    int32_t i, flat;
    if (pair_primary(a, k, i, flat)) {
        const FGeom &g = a.g;
        double x[NDIM], quarter[NDIM];
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            x[d] = a.spos1[k * NDIM + d];
            quarter[d] = 0.25 * g.L[d];
        }
        double w1 = 1.0;
        if (WEIGHTED && a.w1.data) w1 = a.w1.get(i, 0);
        const double qlo = a.e2[0], qhi = a.e2[a.nr];
        const double pimax = MODE == PMX_PAIRS_PROJECTED ? a.sub[a.nsub] : 0.0;
        int32_t c[3];
        fof_cell_axes<NDIM>(g, flat, c);
        pair_walk<NDIM>(a, c, x, quarter, [&](int32_t s, const double *, const double *dx) {
            double q = 0, z = 0;
            if (MODE == PMX_PAIRS_PROJECTED) {
#pragma unroll
                for (int d = 0; d < NDIM; d++)
                    if (d != a.los) q += dx[d] * dx[d];
            } else {
#pragma unroll
                for (int d = 0; d < NDIM; d++) q += dx[d] * dx[d];
            }
            if (!(q >= qlo && q < qhi)) return;
            if (MODE != PMX_PAIRS_1D) z = a.los == 0 ? dx[0] : (a.los == 1 ? dx[1] : dx[2]);
            int bin = e_lds ? pair_bin(se2, a.nr, q) : pair_bin(a.e2, a.nr, q);
            if (MODE == PMX_PAIRS_2D) {
                const double z2 = z * z;
                int m = 0;
                if (q > 0) m = s_lds ? pair_mu_bin(ssub, a.nsub, z2, q) : pair_mu_bin(a.sub, a.nsub, z2, q);
                bin = bin * a.nsub + m;
            }
            if (MODE == PMX_PAIRS_PROJECTED) {
                const double az = fabs(z);
                if (!(az < pimax)) return;
                // (az >= 0 = piedges[0] where the edges are the rule's; anything below the first edge goes to bin 0)
                bin = bin * a.nsub + (s_lds ? pair_bin(ssub, a.nsub, az) : pair_bin(a.sub, a.nsub, az));
            }
            if (bin < 0 || bin >= used) return;                    // (never: 0 <= bin < nbins)
            pair_hist_add<WEIGHTED>(a, hcount, hrsum, hwsum, bin, s, w1, sqrt(q));
        });
    }
    __syncthreads();
    pair_hist_flush<WEIGHTED>(a, hcount, hrsum, hwsum, used, tid);
}

}  // namespace pmx

using namespace pmx;

template <int NDIM, int MODE> static void pairs_launch(const PArgs &a, bool weighted, unsigned grid, hipStream_t st)
{
    const bool big = a.nbins > PAIRS_SLOTS_SMALL;
    with_bool(weighted, [&](auto w) {
        if (big) pairs_kernel<NDIM, MODE, decltype(w)::value, PAIRS_SLOTS_BIG><<<grid, PBLOCK, 0, st>>>(a);
        else pairs_kernel<NDIM, MODE, decltype(w)::value, PAIRS_SLOTS_SMALL><<<grid, PBLOCK, 0, st>>>(a);
    });
}

extern "C" int pmx_pair_counts(int32_t ndim, int32_t mode, int32_t los, int64_t n1, const double *spos1,
                               const int32_t *order1, const int32_t *cell_of1, const pmx_vec *weight1, int64_t n2,
                               const double *spos2, const int32_t *order2, const int32_t *cell_start2,
                               const pmx_vec *weight2, const int64_t *ncell, int32_t periodic, const double *boxsize,
                               int32_t nr, const double *e2, int32_t nsub, const double *sub, int64_t *npairs,
                               double *wnpairs, double *rsum, void *stream)
{
    PArgs a;
    const int rc = fof_geom(ndim, boxsize, nullptr, nullptr, ncell, periodic, a.g, &a.ncells);
    if (rc != PMX_OK) return rc;
    // the modes by row labels: one of the two flags above a base mode 0 .. 4, which says how the pair is binned
    const bool labels = (mode == (PMX_PAIRS_SPLIT | (mode & 7)) || mode == (PMX_PAIRS_JACKKNIFE | (mode & 7))) &&
                        (mode & 7) <= PMX_PAIRS_PROJECTED_MIDPOINT;
    const int entry_mode = mode;
    if (labels) mode &= 7;
    // the modes with alignment sums: the flag PMX_PAIRS_ALIGN above the base mode 1D or projected and nothing else (the
    // test is on the whole word: `mode & 7` of the label flags above never sees 128 | m as a label mode)
    const bool align = entry_mode == (PMX_PAIRS_ALIGN | PMX_PAIRS_1D) || entry_mode == (PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED);
    if (align) mode &= 7;
    const bool midpoint = mode == PMX_PAIRS_2D_MIDPOINT || mode == PMX_PAIRS_PROJECTED_MIDPOINT;
    const bool rows = mode == PMX_PAIRS_1D_ROWS || mode == PMX_PAIRS_PROJECTED_ROWS;
    const bool vel = mode == PMX_PAIRS_1D_VELOCITY || mode == PMX_PAIRS_PROJECTED_VELOCITY || mode == PMX_PAIRS_1D_LOS;
    const bool one = mode == PMX_PAIRS_1D || mode == PMX_PAIRS_1D_ROWS || mode == PMX_PAIRS_1D_VELOCITY ||
                     mode == PMX_PAIRS_1D_LOS;                       // (align: its base mode)
    PMX_REQUIRE(mode == PMX_PAIRS_1D || mode == PMX_PAIRS_2D || mode == PMX_PAIRS_PROJECTED || midpoint || rows || vel,
                PMX_EINVAL, "bad mode");
    PMX_REQUIRE(one || midpoint || (ndim == 3 && los >= 0 && los <= 2), PMX_EINVAL,
                "the modes 2D and projected need three dimensions and a line of sight along one of them");
    PMX_REQUIRE(!midpoint || ndim == 3, PMX_EINVAL, "the midpoint modes need three dimensions");
    PMX_REQUIRE(mode != PMX_PAIRS_1D_LOS || ndim == 3, PMX_EINVAL, "the mode 1D_LOS needs three dimensions");
    PMX_REQUIRE(!align || ndim == 2 || ndim == 3, PMX_EINVAL, "the alignment modes need two or three dimensions");
    PMX_REQUIRE(nr >= 1 && nsub >= 1 && (!one || nsub == 1), PMX_EINVAL, "bad bin counts");
    PMX_REQUIRE((int64_t)nr * nsub <= PMX_PAIRS_MAX_BINS, PMX_EINVAL, "more than PMX_PAIRS_MAX_BINS bins");
    PMX_REQUIRE(!rows || (int64_t)nr * nsub <= PMX_PAIRS_ROWS_MAX_BINS, PMX_EINVAL,
                "more than PMX_PAIRS_ROWS_MAX_BINS bins per row");
    PMX_REQUIRE(!vel || (int64_t)nr * nsub <= PMX_PAIRS_VELOCITY_MAX_BINS, PMX_EINVAL,
                "more than PMX_PAIRS_VELOCITY_MAX_BINS bins");
    PMX_REQUIRE(!align || (int64_t)nr * nsub <= PMX_PAIRS_ALIGN_MAX_BINS, PMX_EINVAL,
                "more than PMX_PAIRS_ALIGN_MAX_BINS bins");
    PMX_REQUIRE(!labels || (int64_t)nr * nsub <= PMX_PAIRS_LABEL_SLOTS / 4, PMX_EINVAL,
                "more than PMX_PAIRS_LABEL_SLOTS / 4 bins in a mode by row labels");
    PMX_REQUIRE(n1 >= 0 && n2 >= 0, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(n1 <= PMX_FOF_MAX_ROWS && n2 <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED,
                "more than 2^31 - 1 rows: slots are 32-bit");
    if (n1 == 0 || n2 == 0) return PMX_OK;
    PMX_REQUIRE(spos1 && order1 && cell_of1 && spos2 && order2 && cell_start2, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(e2 && (one || sub) && npairs && wnpairs && rsum, PMX_EINVAL, "bad arguments");
    const bool has1 = weight1 && weight1->data, has2 = weight2 && weight2->data;
    PMX_REQUIRE(!has1 || vec_ok(weight1), PMX_EINVAL, "weight1 must be float or double");
    PMX_REQUIRE(!has2 || vec_ok(weight2), PMX_EINVAL, "weight2 must be float or double");
    // the velocity modes: both sets bring (w, v_0 .. v_{ndim-1}), or (w, s) in the mode 1D_LOS
    const int32_t vcol = mode == PMX_PAIRS_1D_LOS ? 2 : 1 + ndim;
    PMX_REQUIRE(!vel || (has1 && has2 && weight1->ncol == vcol && weight2->ncol == vcol), PMX_EINVAL,
                "the velocity modes need weight1 and weight2 of 1 + ndim columns (1D_LOS: 2)");
    // the alignment modes: (w, a_0 .. a_{ndim-1}) above 1D, (w, g1, g2) above projected
    const int32_t acol = mode == PMX_PAIRS_PROJECTED ? 3 : 1 + ndim;
    PMX_REQUIRE(!align || (has1 && has2 && weight1->ncol == acol && weight2->ncol == acol), PMX_EINVAL,
                "the alignment modes need weight1 and weight2 of 1 + ndim columns (projected: 3)");
    PMX_REQUIRE(!labels || (has1 && has2 && weight1->ncol == 2 && weight2->ncol == 2), PMX_EINVAL,
                "the modes by row labels need weight1 and weight2 of 2 columns (w, label)");
    a.n1 = n1;
    a.n2 = n2;
    a.spos1 = spos1;
    a.spos2 = spos2;
    a.order1 = order1;
    a.cell_of1 = cell_of1;
    a.order2 = order2;
    a.cell_start2 = cell_start2;
    a.w1 = dvec(has1 ? weight1 : nullptr);
    a.w2 = dvec(has2 ? weight2 : nullptr);
    a.nr = nr;
    a.nsub = nsub;
    a.nbins = nr * nsub;
    a.los = one || midpoint ? 0 : los;
    a.e2 = e2;
    a.sub = sub;
    a.npairs = (unsigned long long *)npairs;
    a.wnpairs = wnpairs;
    a.rsum = rsum;
    const unsigned grid = (unsigned)((n1 + PBLOCK - 1) / PBLOCK);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t lo = 0; lo < n2; lo += PAIRS_WINDOW) {
        a.slo = (int32_t)lo;
        a.shi = (int32_t)(lo + PAIRS_WINDOW < n2 ? lo + PAIRS_WINDOW : n2);
        if (labels) pairs_labels_launch(a, ndim, entry_mode, grid, st);
        else if (align) pairs_align_launch(a, ndim, entry_mode, grid, st);
        else if (midpoint) pairs_survey_launch(a, mode, has1 || has2, grid, st);
        else if (rows) pairs_rows_launch(a, ndim, mode, has1 || has2, st);
        else if (vel) pairs_vel_launch(a, ndim, mode, grid, st);
        else if (mode == PMX_PAIRS_2D) pairs_launch<3, PMX_PAIRS_2D>(a, has1 || has2, grid, st);
        else if (mode == PMX_PAIRS_PROJECTED) pairs_launch<3, PMX_PAIRS_PROJECTED>(a, has1 || has2, grid, st);
        else with_count<3>(ndim, [&](auto nd) { pairs_launch<decltype(nd)::value, PMX_PAIRS_1D>(a, has1 || has2, grid, st); });
    }
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
