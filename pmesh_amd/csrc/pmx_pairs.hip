// pmx_pairs.hip — binned pair counts of particles (include/pmesh_amd.h: pmx_pair_counts; pmesh_amd/paircount.py).
//
// Replaces what a caller of the reference does on the host for xi(r) of a catalogue (nbodykit's SimulationBoxPairCount:
// Corrfunc over the rows copied over PCIe).  Which pair is counted and in which bin: pair_rule (pmx_pairs_dev.h), in the
// base modes 1D, 2D and PROJECTED.  The sums: npairs exact; wnpairs = sum w1 w2 and rsum = sum w1 w2 sqrt(q) in double,
// in no particular order.
// The pass: pairs_kernel, one lane per slot of the primaries in cell order.  The lane walks the 3^ndim neighbouring
// cells of its row in the secondaries (the walk of link_kernel, pmx_cells_dev.h); the lanes of a wave sit in one cell
// or in adjacent ones, so they read the same secondaries at the same time: broadcast loads from cache.  Every pair
// inside the edges makes one 32-bit integer and one (weighted: two) double LDS atomic on the workgroup's histogram;
// at its end the workgroup makes one global atomic per array and non-zero bin.  (Replicating the histogram over the
// lanes, slot = bin * R + lane % R, so that the lanes of a wave that meet in one outer bin do not meet on one address,
// measured nothing at 20 bins, and neither did removing the LDS atomics altogether: DESIGN.md 5.7.)  No lane waits for
// another: the only barriers are the two around the walk.
// pmx_pair_counts below checks the arguments of every mode and launches the kernels of
//   this file               PMX_PAIRS_1D, _2D, _PROJECTED
//   pmx_pairs_survey.hip    PMX_PAIRS_2D_MIDPOINT, _PROJECTED_MIDPOINT: the line of sight is the pair's own
//   pmx_pairs_rows.hip      PMX_PAIRS_1D_ROWS, _PROJECTED_ROWS: one histogram per primary row
//   pmx_pairs_vel.hip       PMX_PAIRS_1D_VELOCITY, _PROJECTED_VELOCITY, _1D_LOS: pairwise velocity sums
//   pmx_pairs_labels.hip    PMX_PAIRS_SPLIT | m, PMX_PAIRS_JACKKNIFE | m, m a base mode 0 .. 4: by row labels
//   pmx_pairs_align.hip     PMX_PAIRS_ALIGN | PMX_PAIRS_1D, | PMX_PAIRS_PROJECTED: intrinsic-alignment sums
//   pmx_pairs_moments.hip   PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS: moment sums per primary row, bins in its own scale
#include "pmx_pairs_dev.h"

namespace pmx {

template <int NDIM, int MODE, bool WEIGHTED, int SLOTS>
__global__ void __launch_bounds__(PBLOCK) pairs_kernel(PArgs a)
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

    PairLane<NDIM> p;
    if (pair_lane(a, (int64_t)blockIdx.x * PBLOCK + tid, p)) {
#pragma unroll
        for (int d = 0; d < NDIM; d++) p.quarter[d] = 0.25 * a.g.L[d];      // (here, not in pair_lane: see there)
        double w1 = 1.0;
        if (WEIGHTED && a.w1.data) w1 = a.w1.get(p.i, 0);
        const PairLimits lim = pair_limits(a, ed);
        pair_walk(a, p, [&](int32_t s, const double *y, const double *dx) {
            double q;
            int bin;
            if (!pair_rule<NDIM>(a, lim, ed, p.x, y, dx, q, bin)) return;
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

// What a mode word asks for (the header lists the valid ones), decoded once; pmx_pair_counts checks the call against it.
enum { PAIRS_PLAIN, PAIRS_SURVEY, PAIRS_ROWS, PAIRS_VEL, PAIRS_LABELS, PAIRS_ALIGN, PAIRS_MOMENTS };
// per family: the most bins nr * nsub, what to say above them, and what to say of weights without the family's columns
static const struct {
    int64_t max_bins;
    const char *bins_text, *ncol_text;
} pair_families[] = {
    {PMX_PAIRS_MAX_BINS, "more than PMX_PAIRS_MAX_BINS bins", ""},
    {PMX_PAIRS_MAX_BINS, "more than PMX_PAIRS_MAX_BINS bins", ""},
    {PMX_PAIRS_ROWS_MAX_BINS, "more than PMX_PAIRS_ROWS_MAX_BINS bins per row", ""},
    {PMX_PAIRS_VELOCITY_MAX_BINS, "more than PMX_PAIRS_VELOCITY_MAX_BINS bins",
     "the velocity modes need weight1 and weight2 of 1 + ndim columns (1D_LOS: 2)"},
    {PMX_PAIRS_LABEL_SLOTS / 4, "more than PMX_PAIRS_LABEL_SLOTS / 4 bins in a mode by row labels",
     "the modes by row labels need weight1 and weight2 of 2 columns (w, label)"},
    {PMX_PAIRS_ALIGN_MAX_BINS, "more than PMX_PAIRS_ALIGN_MAX_BINS bins",
     "the alignment modes need weight1 and weight2 of 1 + ndim columns (projected: 3)"},
    {PMX_PAIRS_MOMENTS_MAX_BINS, "more than PMX_PAIRS_MOMENTS_MAX_BINS bins per row in the moments mode",
     "the moments mode needs weight1 of 2 columns (w, s2) and weight2 of 1 or 1 + ndim columns (m, v)"}};
struct PairMode {
    int family;                                  // whose kernels count: the files listed above, a row of pair_families
    int base;                                    // how a pair is binned: one of the five base modes of pair_rule
    bool one;                                    // no sub axis: nsub == 1, `sub` is not read
    bool axis;                                   // the line of sight is the box axis `los`: ndim == 3, los in {0, 1, 2}
    int32_t min_ndim;                            // the fewest dimensions otherwise, and what to say below them
    const char *ndim_text;
    int32_t ncol;                                // the columns weight1 and weight2 must both have; 0: both optional
    int32_t ncol2;                               // the other count weight2 may have instead (the moments mode); 0: none
};

static bool pair_mode(int32_t mode, int32_t ndim, PairMode &m)
{
    static const int low[10][2] = {{PAIRS_PLAIN, PMX_PAIRS_1D},       {PAIRS_PLAIN, PMX_PAIRS_2D},
                                   {PAIRS_PLAIN, PMX_PAIRS_PROJECTED}, {PAIRS_SURVEY, PMX_PAIRS_2D_MIDPOINT},
                                   {PAIRS_SURVEY, PMX_PAIRS_PROJECTED_MIDPOINT}, {PAIRS_ROWS, PMX_PAIRS_1D},
                                   {PAIRS_ROWS, PMX_PAIRS_PROJECTED},  {PAIRS_VEL, PMX_PAIRS_1D},
                                   {PAIRS_VEL, PMX_PAIRS_PROJECTED},   {PAIRS_VEL, PMX_PAIRS_1D}};
    const int32_t flags = mode & ~7, under = mode & 7;
    if (mode >= 0 && mode <= PMX_PAIRS_1D_LOS) {
        m.family = low[mode][0];
        m.base = low[mode][1];
    } else if ((flags == PMX_PAIRS_SPLIT || flags == PMX_PAIRS_JACKKNIFE) && under <= PMX_PAIRS_PROJECTED_MIDPOINT) {
        m.family = PAIRS_LABELS;                 // one of the two flags above a base mode 0 .. 4
        m.base = under;
    } else if (flags == PMX_PAIRS_ALIGN && (under == PMX_PAIRS_1D || under == PMX_PAIRS_PROJECTED)) {
        m.family = PAIRS_ALIGN;                  // the flag above 1D or projected and nothing else
        m.base = under;
    } else if (mode == (PMX_PAIRS_MOMENTS | PMX_PAIRS_1D_ROWS)) {
        m.family = PAIRS_MOMENTS;                // the flag above 1D_ROWS and nothing else
        m.base = PMX_PAIRS_1D;
    } else {
        return false;
    }
    m.one = m.base == PMX_PAIRS_1D;
    m.axis = m.base == PMX_PAIRS_2D || m.base == PMX_PAIRS_PROJECTED;
    m.min_ndim = 1;
    m.ndim_text = "";
    m.ncol = 0;
    if (m.base == PMX_PAIRS_2D_MIDPOINT || m.base == PMX_PAIRS_PROJECTED_MIDPOINT) {
        m.min_ndim = 3;
        m.ndim_text = "the midpoint modes need three dimensions";
    } else if (mode == PMX_PAIRS_1D_LOS) {
        m.min_ndim = 3;
        m.ndim_text = "the mode 1D_LOS needs three dimensions";
    } else if (m.family == PAIRS_ALIGN) {
        m.min_ndim = 2;
        m.ndim_text = "the alignment modes need two or three dimensions";
    } else if (m.family == PAIRS_MOMENTS) {
        m.min_ndim = 2;
        m.ndim_text = "the moments mode needs two or three dimensions";
    }
    // the columns: (w, v_0 .. v_{ndim-1}), or (w, s) in the mode 1D_LOS; (w, label); (w, a_0 .. a_{ndim-1}) above 1D,
    // (w, g1, g2) above projected; (w, s2) against (m) or (m, v_0 .. v_{ndim-1}) in the moments mode
    if (m.family == PAIRS_VEL) m.ncol = mode == PMX_PAIRS_1D_LOS ? 2 : 1 + ndim;
    if (m.family == PAIRS_LABELS) m.ncol = 2;
    if (m.family == PAIRS_ALIGN) m.ncol = m.base == PMX_PAIRS_PROJECTED ? 3 : 1 + ndim;
    m.ncol2 = 0;
    if (m.family == PAIRS_MOMENTS) {
        m.ncol = 2;
        m.ncol2 = 1 + ndim;
    }
    return true;
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
    PairMode m;
    PMX_REQUIRE(pair_mode(mode, ndim, m), PMX_EINVAL, "bad mode");
    PMX_REQUIRE(!m.axis || (ndim == 3 && los >= 0 && los <= 2), PMX_EINVAL,
                "the modes 2D and projected need three dimensions and a line of sight along one of them");
    PMX_REQUIRE(ndim >= m.min_ndim, PMX_EINVAL, m.ndim_text);
    PMX_REQUIRE(nr >= 1 && nsub >= 1 && (!m.one || nsub == 1), PMX_EINVAL, "bad bin counts");
    PMX_REQUIRE(m.family != PAIRS_MOMENTS || !sub, PMX_EINVAL, "the moments mode takes no sub axis: sub must be NULL");
    PMX_REQUIRE((int64_t)nr * nsub <= PMX_PAIRS_MAX_BINS, PMX_EINVAL, "more than PMX_PAIRS_MAX_BINS bins");
    PMX_REQUIRE((int64_t)nr * nsub <= pair_families[m.family].max_bins, PMX_EINVAL,
                pair_families[m.family].bins_text);
    PMX_REQUIRE(n1 >= 0 && n2 >= 0, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(n1 <= PMX_FOF_MAX_ROWS && n2 <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED,
                "more than 2^31 - 1 rows: slots are 32-bit");
    if (n1 == 0 || n2 == 0) return PMX_OK;
    PMX_REQUIRE(spos1 && order1 && cell_of1 && spos2 && order2 && cell_start2, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(e2 && (m.one || sub) && npairs && wnpairs && rsum, PMX_EINVAL, "bad arguments");
    const bool has1 = weight1 && weight1->data, has2 = weight2 && weight2->data;
    PMX_REQUIRE(!has1 || vec_ok(weight1), PMX_EINVAL, "weight1 must be float or double");
    PMX_REQUIRE(!has2 || vec_ok(weight2), PMX_EINVAL, "weight2 must be float or double");
    PMX_REQUIRE(m.ncol == 0 || (has1 && has2 && weight1->ncol == m.ncol &&
                                (m.ncol2 ? weight2->ncol == 1 || weight2->ncol == m.ncol2 : weight2->ncol == m.ncol)),
                PMX_EINVAL, pair_families[m.family].ncol_text);
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
    a.los = m.axis ? los : 0;
    a.e2 = e2;
    a.sub = sub;
    a.npairs = (unsigned long long *)npairs;
    a.wnpairs = wnpairs;
    a.rsum = rsum;
    const unsigned grid = (unsigned)((n1 + PBLOCK - 1) / PBLOCK);
    hipStream_t st = (hipStream_t)stream;
    const bool weighted = has1 || has2;
    for (int64_t lo = 0; lo < n2; lo += PAIRS_WINDOW) {
        a.slo = (int32_t)lo;
        a.shi = (int32_t)(lo + PAIRS_WINDOW < n2 ? lo + PAIRS_WINDOW : n2);
        switch (m.family) {
        case PAIRS_SURVEY: pairs_survey_launch(a, mode, weighted, grid, st); break;
        case PAIRS_ROWS: pairs_rows_launch(a, ndim, mode, weighted, st); break;
        case PAIRS_VEL: pairs_vel_launch(a, ndim, mode, grid, st); break;
        case PAIRS_LABELS: pairs_labels_launch(a, ndim, mode, grid, st); break;
        case PAIRS_ALIGN: pairs_align_launch(a, ndim, mode, grid, st); break;
        case PAIRS_MOMENTS: pairs_moments_launch(a, ndim, weight2->ncol > 1, st); break;
        default:
            if (m.base == PMX_PAIRS_2D) pairs_launch<3, PMX_PAIRS_2D>(a, weighted, grid, st);
            else if (m.base == PMX_PAIRS_PROJECTED) pairs_launch<3, PMX_PAIRS_PROJECTED>(a, weighted, grid, st);
            else with_count<3>(ndim, [&](auto nd) { pairs_launch<decltype(nd)::value, PMX_PAIRS_1D>(a, weighted, grid, st); });
        }
    }
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
