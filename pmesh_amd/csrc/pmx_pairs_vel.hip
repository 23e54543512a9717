// pmx_pairs_vel.hip — the pair counts with pairwise velocity sums: the modes PMX_PAIRS_1D_VELOCITY,
// PMX_PAIRS_PROJECTED_VELOCITY and PMX_PAIRS_1D_LOS of pmx_pair_counts (include/pmesh_amd.h; pmesh_amd/pairvel.py).
//
// What halotools does on the host as mean_radial_velocity_vs_r, radial_pvd_vs_r, mean_los_velocity_vs_rp and
// los_pvd_vs_rp, and the pairwise estimator of Ferreira et al. (1999) for one line-of-sight scalar per row.  The rule,
// restated from the header, on top of that of pmx_pairs.hip (double arithmetic, every operation rounded once, squared
// edges, no square root choosing a bin, exact npairs, double sums in no particular order).  Per counted pair, with
// w = w1_i * w2_j:
//   1D_VELOCITY         dv_d = v_i,d - v_j,d; h = dx_0 dv_0 + dx_1 dv_1 + dx_2 dv_2 and dv2 = dv_0^2 + dv_1^2 + dv_2^2,
//                       each summed in that order over d < ndim; r = sqrt(r2); u = h / r where r2 > 0, else 0
//                       S1 += (w u), S2 += (w u) u, S3 += w dv2
//   PROJECTED_VELOCITY  u = dx_los < 0 ? -dv_los : dv_los; S1, S2, S3 as above, dv2 over all three axes; the m = 0 sum
//                       adds w sqrt(rp2)
//   1D_LOS              o_d = 0.5 * L_d; a_d = w_i,d - o_d, b_d = w_j,d - o_d; a2, b2, pa = dx.a, pb = dx.b summed over
//                       d = 0, 1, 2 in order; ta = a2 > 0 ? pa / sqrt(a2) : 0, tb likewise; c = r2 > 0 ?
//                       0.5 * ((ta + tb) / r) : 0; ds = s_i - s_j; S1 += (w c) ds, S2 += (w c) c, S3 += (w ds) ds
//   rsum[m * nbins + b]: m = 0 the sum of w sqrt(q), m = 1, 2, 3 the sums S1, S2, S3
// The pass is that of pairs_kernel: one lane per slot of the primaries in cell order, the walk over the 3^ndim
// neighbouring cells with broadcast loads of the secondaries, the workgroup's histogram in LDS, one global atomic per
// array and non-zero bin at the end (pmx_pairs_dev.h); no barrier beyond the two around the walk.  The histogram holds
// a 32-bit count and five doubles (w, w r, S1, S2, S3) per bin: 44 KB at PMX_PAIRS_VELOCITY_MAX_BINS = 1024 bins, three
// workgroups in the 160 KB of a CU; the edges are searched in LDS up to 128 bins along an axis, as in the small form of
// pairs_kernel.  The primary's columns are loaded once per lane before the walk; a secondary's columns are read only
// after the pair has passed the edge tests, and the square roots and the divisions are taken only then.
// The form kept: one 32-bit and five double LDS atomics per counted pair, the plain extension of the weighted kernel's
// three.  Measured at 1.5 to 1.8 times the weighted pairs_kernel on the same rows and edges (scripts/pairs_probe.py
// --velocity).  Tried and dropped: the histogram replicated over the lanes for few bins (rows_kernel's
// copies, slot = bin * copies + lane % copies, sixteen copies at 40 bins): 113.4 ms against 113.3, nothing, as on
// pairs_kernel.  Not tried: a pre-sum over the lanes of a wave that hit the same bin: the lanes are not converged at a
// counted pair (each walks its own cells), so it needs a match loop per pair over five doubles, and with the conflicts
// measured at nothing it has nothing to win.
#include "pmx_pairs_dev.h"

namespace pmx {

constexpr int VSLOTS = PMX_PAIRS_VELOCITY_MAX_BINS;
constexpr int VSUMS = 5;                         // w, w r, S1, S2, S3

template <int NDIM, int MODE>
__global__ void __launch_bounds__(PBLOCK) vel_kernel(PArgs a)
{
    constexpr bool PROJECTED = MODE == PMX_PAIRS_PROJECTED_VELOCITY, LOS = MODE == PMX_PAIRS_1D_LOS;
    constexpr int NV = LOS ? 1 : NDIM;           // the columns behind the weight
    __shared__ uint32_t hcount[VSLOTS];
    __shared__ double hsum[VSUMS][VSLOTS];
    __shared__ double se2[PAIRS_EDGES_LDS + 1];
    __shared__ double ssub[PROJECTED ? PAIRS_EDGES_LDS + 1 : 1];
    const int tid = threadIdx.x;
    const int used = min(a.nbins, VSLOTS);
    for (int s = tid; s < used; s += PBLOCK) {
        hcount[s] = 0;
#pragma unroll
        for (int m = 0; m < VSUMS; m++) hsum[m][s] = 0;
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
#pragma unroll
        for (int d = 0; d < NV; d++) v1[d] = a.w1.get(i, 1 + d);
        // (1D_LOS) the primary from the observer, and its length
        double o[3] = {0, 0, 0}, av[3] = {0, 0, 0}, a2 = 0, ra = 0;
        if (LOS) {
#pragma unroll
            for (int d = 0; d < NDIM; d++) {
                o[d] = 0.5 * g.L[d];
                av[d] = x[d] - o[d];
                a2 += av[d] * av[d];
            }
            ra = sqrt(a2);
        }
        const double qlo = a.e2[0], qhi = a.e2[a.nr];
        const double pimax = PROJECTED ? a.sub[a.nsub] : 0.0;
        int32_t c[3];
        fof_cell_axes<NDIM>(g, flat, c);
        pair_walk<NDIM>(a, c, x, quarter, [&](int32_t s, const double *y, const double *dx) {
            double q = 0;
#pragma unroll
            for (int d = 0; d < NDIM; d++)
                if (!PROJECTED || d != a.los) q += dx[d] * dx[d];
            if (!(q >= qlo && q < qhi)) return;
            int bin = e_lds ? pair_bin(se2, a.nr, q) : pair_bin(a.e2, a.nr, q);
            double z = 0;
            if (PROJECTED) {
                z = a.los == 0 ? dx[0] : (a.los == 1 ? dx[1] : dx[2]);
                const double az = fabs(z);
                if (!(az < pimax)) return;
                // (az >= 0 = piedges[0] where the edges are the rule's; anything below the first edge goes to bin 0)
                bin = bin * a.nsub + (s_lds ? pair_bin(ssub, a.nsub, az) : pair_bin(a.sub, a.nsub, az));
            }
            if (bin < 0 || bin >= used) return;                    // (never: 0 <= bin < nbins)
            const int32_t j = a.order2[s];
            if (j < 0 || j >= a.n2) return;                         // (never, with the order fill_kernel left)
            const double w = w1 * a.w2.get(j, 0);
            double dv[NV];
#pragma unroll
            for (int d = 0; d < NV; d++) dv[d] = v1[d] - a.w2.get(j, 1 + d);
            const double r = sqrt(q);                               // (1D_VELOCITY, 1D_LOS: q = r2)
            double s1, s2, s3;
            if (LOS) {
                double bv[3] = {0, 0, 0}, b2 = 0, pa = 0, pb = 0;
#pragma unroll
                for (int d = 0; d < NDIM; d++) {
                    bv[d] = y[d] - o[d];
                    b2 += bv[d] * bv[d];
                    pa += dx[d] * av[d];
                    pb += dx[d] * bv[d];
                }
                const double ta = a2 > 0 ? pa / ra : 0.0;
                const double tb = b2 > 0 ? pb / sqrt(b2) : 0.0;
                const double cc = q > 0 ? 0.5 * ((ta + tb) / r) : 0.0;
                const double ds = dv[0], wc = w * cc;
                s1 = wc * ds;
                s2 = wc * cc;
                s3 = (w * ds) * ds;
            } else {
                double h = 0, dv2 = 0;
#pragma unroll
                for (int d = 0; d < NDIM; d++) {
                    h += dx[d] * dv[d];
                    dv2 += dv[d] * dv[d];
                }
                double u;
                if (PROJECTED) {
                    const double dvz = a.los == 0 ? dv[0] : (a.los == 1 ? dv[NDIM > 1 ? 1 : 0] : dv[NDIM > 2 ? 2 : 0]);
                    u = z < 0 ? -dvz : dvz;
                } else {
                    u = q > 0 ? h / r : 0.0;
                }
                s1 = w * u;
                s2 = s1 * u;
                s3 = w * dv2;
            }
            atomicAdd(&hcount[bin], 1u);
            atomicAdd(&hsum[0][bin], w);
            atomicAdd(&hsum[1][bin], w * r);
            atomicAdd(&hsum[2][bin], s1);
            atomicAdd(&hsum[3][bin], s2);
            atomicAdd(&hsum[4][bin], s3);
        });
    }
    __syncthreads();
    for (int b = tid; b < used; b += PBLOCK) {
        const unsigned long long n = hcount[b];
        if (n == 0) continue;
        atomicAdd(&a.npairs[b], n);
        atomicAdd(&a.wnpairs[b], hsum[0][b]);
#pragma unroll
        for (int m = 0; m < 4; m++) atomicAdd(&a.rsum[(int64_t)m * a.nbins + b], hsum[1 + m][b]);
    }
}

void pairs_vel_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st)
{
    if (a.nbins < 1 || a.nbins > VSLOTS || !a.w1.data || !a.w2.data) return;   // (never: pmx_pair_counts has checked it)
    if (mode == PMX_PAIRS_PROJECTED_VELOCITY) vel_kernel<3, PMX_PAIRS_PROJECTED_VELOCITY><<<grid, PBLOCK, 0, st>>>(a);
    else if (mode == PMX_PAIRS_1D_LOS) vel_kernel<3, PMX_PAIRS_1D_LOS><<<grid, PBLOCK, 0, st>>>(a);
    else with_count<3>(ndim, [&](auto nd) { vel_kernel<decltype(nd)::value, PMX_PAIRS_1D_VELOCITY><<<grid, PBLOCK, 0, st>>>(a); });
}

}  // namespace pmx
