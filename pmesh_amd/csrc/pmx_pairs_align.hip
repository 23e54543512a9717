// pmx_pairs_align.hip — the pair counts with intrinsic-alignment sums: the modes PMX_PAIRS_ALIGN | PMX_PAIRS_1D (128) and
// PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED (130) of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/alignments.py).
//
// What halotools-ia does on the host as ed_3d, ee_3d, gi_plus_projected, ii_plus_projected and their minus partners.
// The rule, restated from the header, on top of that of pmx_pairs.hip (double arithmetic, every operation rounded once,
// squared edges, no square root choosing a bin, exact npairs, double sums in no particular order).  Per counted pair,
// with w = w1_i * w2_j:
//   128  columns (w, a_0 .. a_{ndim-1}); a the primary's vector, c the secondary's; a2, c2, pa = dx.a, pc = dx.c and
//        ac = a.c each summed over d < ndim in ascending d
//        t1 = (r2 > 0 && a2 > 0) ? (pa * pa) / (a2 * r2) : 0, t2 = (r2 > 0 && c2 > 0) ? (pc * pc) / (c2 * r2) : 0,
//        t3 = (r2 > 0 && a2 > 0 && c2 > 0) ? (ac * ac) / (a2 * c2) : 0
//        S1 += w * t1, S2 += w * t2, S3 += w * t3
//   130  columns (w, g1, g2), referred to the axes A < B other than los; rp2 = q;
//        cc = dx_A * dx_A - dx_B * dx_B, ss = 2.0 * (dx_A * dx_B)
//        p = rp2 > 0 ? (g1 * cc + g2 * ss) / rp2 : 0, x = rp2 > 0 ? (g1 * ss - g2 * cc) / rp2 : 0 for either row
//        S1 += w * p1, S2 += w * p2, S3 += (w * p1) * p2, S4 += (w * x1) * x2, S5 += w * x1, S6 += w * x2
//   rsum[m * nbins + b]: m = 0 the sum of w sqrt(q), m = 1 .. NS the sums S1 .. S_NS
// The pass is that of vel_kernel (pmx_pairs_vel.hip): one lane per slot of the primaries in cell order, the walk over
// the 3^ndim neighbouring cells with broadcast loads of the secondaries, the workgroup's histogram in LDS, one global
// atomic per array and non-zero bin at the end (pmx_pairs_dev.h); no barrier beyond the two around the walk.  The
// histogram holds a 32-bit count and 2 + NS doubles (w, w r, S1 .. S_NS) per bin over PMX_PAIRS_ALIGN_MAX_BINS = 1024
// bins: 44 KB in mode 128, the layout of vel_kernel, three workgroups in the 160 KB of a CU; 68 KB in mode 130, two
// workgroups, like the big form of pairs_kernel.  The edges are searched in LDS up to 128 bins along an axis.  The
// primary's columns (and a2) are loaded once per lane before the walk; a secondary's columns are read only after the
// pair has passed the edge tests, and the divisions are taken only then.
// The form kept: one 32-bit and 2 + NS double LDS atomics per counted pair, six in mode 128 as in
// PMX_PAIRS_1D_VELOCITY, nine in mode 130 against the six of PMX_PAIRS_PROJECTED_VELOCITY.  Measured on 10^6 uniform
// rows, auto, in turn with the velocity kernel on the same rows and edges (scripts/pairs_probe.py --align; DESIGN.md
// 5.7): mode 128 at 1.02 times PMX_PAIRS_1D_VELOCITY (40 bins), mode 130 at 1.28 to 1.39 times
// PMX_PAIRS_PROJECTED_VELOCITY (40 x 25 bins), below its 9 / 6 atomics.  Not tried: a histogram sized by nbins (fewer
// bytes of LDS and a third workgroup per CU in mode 130 at few bins); the replicated histogram that measured nothing on
// vel_kernel was not tried again.
#include "pmx_pairs_dev.h"

namespace pmx {

constexpr int ASLOTS = PMX_PAIRS_ALIGN_MAX_BINS;
constexpr int ALIGN_1D = PMX_PAIRS_ALIGN | PMX_PAIRS_1D, ALIGN_PROJECTED = PMX_PAIRS_ALIGN | PMX_PAIRS_PROJECTED;

template <int NDIM, int MODE>
__global__ void __launch_bounds__(PBLOCK) align_kernel(PArgs a)
{
    constexpr bool PROJECTED = MODE == ALIGN_PROJECTED;
    constexpr int NS = PROJECTED ? 6 : 3;        // the sums behind w and w r
    constexpr int NV = PROJECTED ? 2 : NDIM;     // the columns behind the weight
    __shared__ uint32_t hcount[ASLOTS];
    __shared__ double hsum[2 + NS][ASLOTS];
    __shared__ double se2[PAIRS_EDGES_LDS + 1];
    __shared__ double ssub[PROJECTED ? PAIRS_EDGES_LDS + 1 : 1];
    const int tid = threadIdx.x;
    const int used = min(a.nbins, ASLOTS);
    for (int s = tid; s < used; s += PBLOCK) {
        hcount[s] = 0;
#pragma unroll
        for (int m = 0; m < 2 + NS; m++) hsum[m][s] = 0;
    }
    const bool e_lds = a.nr <= PAIRS_EDGES_LDS, s_lds = a.nsub <= PAIRS_EDGES_LDS;
    if (e_lds) pair_edges_load(se2, a.e2, a.nr, tid);
    if (PROJECTED && s_lds) pair_edges_load(ssub, a.sub, a.nsub, tid);
    __syncthreads();

    const int64_t k = (int64_t)blockIdx.x * PBLOCK + tid;
    int32_t i, flat;
    if (pair_primary(a, k, i, flat)) {
        const FGeom &g = a.g;
        double x[NDIM], quarter[NDIM], v1[NV];
#pragma unroll
        for (int d = 0; d < NDIM; d++) {
            x[d] = a.spos1[k * NDIM + d];
            quarter[d] = 0.25 * g.L[d];
        }
        const double w1 = a.w1.get(i, 0);
        double a2 = 0;                                              // (128) the squared length of the primary's vector
#pragma unroll
        for (int d = 0; d < NV; d++) {
            v1[d] = a.w1.get(i, 1 + d);
            if (!PROJECTED) a2 += v1[d] * v1[d];
        }
        const double qlo = a.e2[0], qhi = a.e2[a.nr];
        const double pimax = PROJECTED ? a.sub[a.nsub] : 0.0;
        int32_t c[3];
        fof_cell_axes<NDIM>(g, flat, c);
        pair_walk<NDIM>(a, c, x, quarter, [&](int32_t s, const double *, const double *dx) {
            double q = 0;
#pragma unroll
            for (int d = 0; d < NDIM; d++)
                if (!PROJECTED || d != a.los) q += dx[d] * dx[d];
            if (!(q >= qlo && q < qhi)) return;
            int bin = e_lds ? pair_bin(se2, a.nr, q) : pair_bin(a.e2, a.nr, q);
            if (PROJECTED) {
                const double z = a.los == 0 ? dx[0] : (a.los == 1 ? dx[1] : dx[2]);
                const double az = fabs(z);
                if (!(az < pimax)) return;
                // (az >= 0 = piedges[0] where the edges are the rule's; anything below the first edge goes to bin 0)
                bin = bin * a.nsub + (s_lds ? pair_bin(ssub, a.nsub, az) : pair_bin(a.sub, a.nsub, az));
            }
            if (bin < 0 || bin >= used) return;                    // (never: 0 <= bin < nbins)
            const int32_t j = a.order2[s];
            if (j < 0 || j >= a.n2) return;                         // (never, with the order fill_kernel left)
            const double w = w1 * a.w2.get(j, 0);
            double v2[NV];
#pragma unroll
            for (int d = 0; d < NV; d++) v2[d] = a.w2.get(j, 1 + d);
            double t[NS];
            if (PROJECTED) {
                // the axes A < B other than los
                const double da = a.los == 0 ? dx[1] : dx[0], db = a.los == 2 ? dx[1] : dx[2];
                const double cc = da * da - db * db, ss = 2.0 * (da * db);
                double p1 = 0, x1 = 0, p2 = 0, x2 = 0;
                if (q > 0) {
                    p1 = (v1[0] * cc + v1[1] * ss) / q;
                    x1 = (v1[0] * ss - v1[1] * cc) / q;
                    p2 = (v2[0] * cc + v2[1] * ss) / q;
                    x2 = (v2[0] * ss - v2[1] * cc) / q;
                }
                t[0] = w * p1;
                t[1] = w * p2;
                t[2] = (w * p1) * p2;
                t[3] = (w * x1) * x2;
                t[4] = w * x1;
                t[5] = w * x2;
            } else {
                double c2 = 0, pa = 0, pc = 0, ac = 0;
#pragma unroll
                for (int d = 0; d < NDIM; d++) {
                    c2 += v2[d] * v2[d];
                    pa += dx[d] * v1[d];
                    pc += dx[d] * v2[d];
                    ac += v1[d] * v2[d];
                }
                const double t1 = (q > 0 && a2 > 0) ? (pa * pa) / (a2 * q) : 0.0;
                const double t2 = (q > 0 && c2 > 0) ? (pc * pc) / (c2 * q) : 0.0;
                const double t3 = (q > 0 && a2 > 0 && c2 > 0) ? (ac * ac) / (a2 * c2) : 0.0;
                t[0] = w * t1;
                t[1] = w * t2;
                t[2] = w * t3;
            }
            atomicAdd(&hcount[bin], 1u);
            atomicAdd(&hsum[0][bin], w);
            atomicAdd(&hsum[1][bin], w * sqrt(q));
#pragma unroll
            for (int m = 0; m < NS; m++) atomicAdd(&hsum[2 + m][bin], t[m]);
        });
    }
    __syncthreads();
    for (int b = tid; b < used; b += PBLOCK) {
        const unsigned long long n = hcount[b];
        if (n == 0) continue;
        atomicAdd(&a.npairs[b], n);
        atomicAdd(&a.wnpairs[b], hsum[0][b]);
#pragma unroll
        for (int m = 0; m < 1 + NS; m++) atomicAdd(&a.rsum[(int64_t)m * a.nbins + b], hsum[1 + m][b]);
    }
}

void pairs_align_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st)
{
    if (a.nbins < 1 || a.nbins > ASLOTS || !a.w1.data || !a.w2.data) return;   // (never: pmx_pair_counts has checked it)
    if (mode == ALIGN_PROJECTED && ndim == 3) align_kernel<3, ALIGN_PROJECTED><<<grid, PBLOCK, 0, st>>>(a);
    else if (mode == ALIGN_1D && ndim == 3) align_kernel<3, ALIGN_1D><<<grid, PBLOCK, 0, st>>>(a);
    else if (mode == ALIGN_1D && ndim == 2) align_kernel<2, ALIGN_1D><<<grid, PBLOCK, 0, st>>>(a);
}

}  // namespace pmx
