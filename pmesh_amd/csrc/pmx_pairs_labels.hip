// pmx_pairs_labels.hip — the pair counts whose bin depends on an integer label of each of the two rows: the modes
// PMX_PAIRS_SPLIT | m and PMX_PAIRS_JACKKNIFE | m of pmx_pair_counts, m one of the five base modes
// (include/pmesh_amd.h; pmesh_amd/pairlabels.py).
//
// What halotools does on the host as tpcf_one_two_halo_decomp and tpcf_jackknife, and pycorr's jackknife estimators:
// the pairs of rows of one host apart from the others, and the sums from which every delete-one realisation of a
// jackknife over K regions follows, in one walk over the pairs instead of K + 1.  The rule, restated from the header.
// Rows, wrapping, the minimum image, r2, q, the squared edges, the r-, mu- and pi-bin and the pimax cut are exactly those
// of the base mode (pmx_pairs.hip for 1D, 2D and PROJECTED, pmx_pairs_survey.hip for the two midpoint modes: double
// arithmetic, every operation rounded once, no square root choosing a bin); the bin choice is restated
// below, not taken from pair_rule of pmx_pairs_dev.h: on top of it this kernel measured 0.1 to 1.5 % slower (DESIGN.md
// 5.7), and the tests hold npairs of `32 | m` to that of `m` exactly.  Both sets bring the columns
// (w, label).  Per counted pair of bin b with the labels a (primary) and c (secondary), w = w1_i * w2_j:
//   SPLIT      kind = (a == c and a is a label) ? 1 : 0; npairs[kind * nbins + b] += 1, wnpairs[...] += w,
//              rsum[...] += w * sqrt(q).  A label is a finite value >= 0.
//   JACKKNIFE  K = (PMX_PAIRS_LABEL_SLOTS / nbins - 2) / 2; a label is in range when it is below K.
//              all[b] gets (1, w, w sqrt(q)); if a is in range, side[a][b] gets (1, w); if c is in range, side[c][b]
//              gets (1, w), so a pair with a == c adds 2 and 2w (w + w, exact); if a == c and in range, same[a][b] gets
//              (1, w).  npairs and wnpairs in blocks of nbins: block 0 all, block 1 + k side[k], block 1 + K + k same[k].
// The test of a label is a comparison that is false for NaN; a row without a label indexes nothing and is the same as
// no row.
// The pass is that of pairs_kernel and vel_kernel: one lane per slot of the primaries in cell order, the walk over the
// 3^ndim neighbouring cells with broadcast loads of the secondaries, the workgroup's histogram in LDS, one global atomic
// per array and non-zero slot at the end (pmx_pairs_dev.h); no barrier beyond the two around the walk.  The histogram
// holds a 32-bit count and one double per slot over PMX_PAIRS_LABEL_SLOTS = 4096 slots, 48 KB; with the two edge tables
// 50 KB, three workgroups in the 160 KB of a CU.  The slots: JACKKNIFE, the (1 + 2 K) blocks of (count, w) as they leave
// and one block more whose double is the r-sum of `all` (the "- 2" in K: one block for all, one for its r-sum); SPLIT,
// nbins <= 1024: two blocks of (count, w) and two whose double is the r-sum.  The primary's w and label are loaded once
// per lane before the walk; the secondary's two columns are read only after the pair has passed the edge tests.  LDS
// atomics per counted pair: SPLIT three; JACKKNIFE at most seven: all 3, side 2 (a == c: one update of (2, w + w), the
// common pair where the regions are spatial and the primaries of a workgroup are cell-sorted) or 2 x 2, same 2.
// Measured at 1.46 to 1.80 (jackknife, 50 labels) and 1.41 to 1.73 (split) times the weighted pairs_kernel on the same
// rows and edges, 24 to 35 times faster than the K + 1 weighted calls one jackknife call replaces
// (scripts/pairs_probe.py --labels).
#include "pmx_pairs_dev.h"

namespace pmx {

constexpr int LSLOTS = PMX_PAIRS_LABEL_SLOTS;

template <int NDIM, int BASE, bool JACK>
__global__ void __launch_bounds__(PBLOCK) labels_kernel(PArgs a)
{
    constexpr bool MID = BASE == PMX_PAIRS_2D_MIDPOINT || BASE == PMX_PAIRS_PROJECTED_MIDPOINT;
    constexpr bool SUB = BASE != PMX_PAIRS_1D;
    __shared__ uint32_t hcount[LSLOTS];
    __shared__ double hsum[LSLOTS];
    __shared__ double se2[PAIRS_EDGES_LDS + 1];
    __shared__ double ssub[SUB ? PAIRS_EDGES_LDS + 1 : 1];
    const int tid = threadIdx.x;
    const int nbins = a.nbins;
    // (pairs_labels_launch has checked 1 <= nbins <= LSLOTS / 4: K >= 1 and every block below fits)
    const int K = JACK ? (LSLOTS / nbins - 2) / 2 : 0;
    const int blocks = JACK ? 1 + 2 * K : 2;                        // the blocks of (count, w) that leave
    const int rbase = blocks * nbins;                               // the first slot whose double is an r-sum
    const int used = min((JACK ? blocks + 1 : 4) * nbins, LSLOTS);
    for (int s = tid; s < used; s += PBLOCK) {
        hcount[s] = 0;
        hsum[s] = 0;
    }
    const bool e_lds = a.nr <= PAIRS_EDGES_LDS, s_lds = a.nsub <= PAIRS_EDGES_LDS;
    if (e_lds) pair_edges_load(se2, a.e2, a.nr, tid);
    if (SUB && s_lds) pair_edges_load(ssub, a.sub, a.nsub, tid);
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
        const double w1 = a.w1.get(i, 0), la = a.w1.get(i, 1);
        // the primary's label: in range (JACKKNIFE: below K; SPLIT: finite), false for NaN
        const bool has_a = JACK ? (la >= 0 && la < (double)K) : (la >= 0 && la < INFINITY);
        const int ka = JACK && has_a ? (int)la : 0;
        const double qlo = a.e2[0], qhi = a.e2[a.nr];
        const double submax = BASE == PMX_PAIRS_PROJECTED || BASE == PMX_PAIRS_PROJECTED_MIDPOINT ? a.sub[a.nsub] : 0.0;
        const double pre = BASE == PMX_PAIRS_PROJECTED_MIDPOINT ? qhi + submax : qhi;
        int32_t c[3];
        fof_cell_axes<NDIM>(g, flat, c);
        pair_walk<NDIM>(a, c, x, quarter, [&](int32_t s, const double *y, const double *dx) {
            double q = 0;
            int m = 0;
            if constexpr (MID) {
                // pmx_pairs_survey.hip, operation by operation
                const double r2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2];
                if (BASE == PMX_PAIRS_2D_MIDPOINT) {
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
                q = r2;
                if (BASE == PMX_PAIRS_2D_MIDPOINT) {
                    const double t = r2 * l2;
                    if (t != 0) m = s_lds ? pair_mu_bin(ssub, a.nsub, p2, t) : pair_mu_bin(a.sub, a.nsub, p2, t);
                } else {
                    const double pi2 = l2 == 0 ? 0.0 : p2 / l2;
                    q = r2 - pi2;
                    if (q < 0) q = 0;
                    if (!(q >= qlo && q < qhi) || !(pi2 < submax)) return;
                    m = s_lds ? pair_bin(ssub, a.nsub, pi2) : pair_bin(a.sub, a.nsub, pi2);
                }
            } else {
                // pmx_pairs.hip, operation by operation
#pragma unroll
                for (int d = 0; d < NDIM; d++)
                    if (BASE != PMX_PAIRS_PROJECTED || d != a.los) q += dx[d] * dx[d];
                if (!(q >= qlo && q < qhi)) return;
                if (SUB) {
                    const double z = a.los == 0 ? dx[0] : (a.los == 1 ? dx[1] : dx[2]);
                    if (BASE == PMX_PAIRS_2D) {
                        const double z2 = z * z;
                        if (q > 0) m = s_lds ? pair_mu_bin(ssub, a.nsub, z2, q) : pair_mu_bin(a.sub, a.nsub, z2, q);
                    } else {
                        const double az = fabs(z);
                        if (!(az < submax)) return;
                        m = s_lds ? pair_bin(ssub, a.nsub, az) : pair_bin(a.sub, a.nsub, az);
                    }
                }
            }
            int bin = e_lds ? pair_bin(se2, a.nr, q) : pair_bin(a.e2, a.nr, q);
            if (SUB) bin = bin * a.nsub + m;
            if (bin < 0 || bin >= nbins) return;                    // (never: 0 <= bin < nbins)
            const int32_t j = a.order2[s];
            if (j < 0 || j >= a.n2) return;                         // (never, with the order fill_kernel left)
            const double w = w1 * a.w2.get(j, 0), lc = a.w2.get(j, 1);
            const double wr = w * sqrt(q);
            if (JACK) {
                const bool has_c = lc >= 0 && lc < (double)K;
                const int kc = has_c ? (int)lc : 0;
                // every slot below is under (2 + 2 K) * nbins <= LSLOTS: 0 <= ka, kc < K, 0 <= bin < nbins
                atomicAdd(&hcount[bin], 1u);
                atomicAdd(&hsum[bin], w);
                atomicAdd(&hsum[rbase + bin], wr);
                if (has_a && has_c && ka == kc) {
                    const int side = (1 + ka) * nbins + bin, same = (1 + K + ka) * nbins + bin;
                    atomicAdd(&hcount[side], 2u);
                    atomicAdd(&hsum[side], w + w);
                    atomicAdd(&hcount[same], 1u);
                    atomicAdd(&hsum[same], w);
                } else {
                    if (has_a) {
                        const int side = (1 + ka) * nbins + bin;
                        atomicAdd(&hcount[side], 1u);
                        atomicAdd(&hsum[side], w);
                    }
                    if (has_c) {
                        const int side = (1 + kc) * nbins + bin;
                        atomicAdd(&hcount[side], 1u);
                        atomicAdd(&hsum[side], w);
                    }
                }
            } else {
                const int slot = (has_a && la == lc ? nbins : 0) + bin;     // under 2 * nbins; its r-sum under 4 * nbins
                atomicAdd(&hcount[slot], 1u);
                atomicAdd(&hsum[slot], w);
                atomicAdd(&hsum[rbase + slot], wr);
            }
        });
    }
    __syncthreads();
    // the blocks of (count, w), and the r-sums: of `all` alone (JACKKNIFE) or of both kinds (SPLIT); a slot with no
    // pair has nothing in either
    const int out = blocks * nbins;
    for (int s = tid; s < min(out, LSLOTS); s += PBLOCK) {
        const unsigned long long n = hcount[s];
        if (n == 0) continue;
        atomicAdd(&a.npairs[s], n);
        atomicAdd(&a.wnpairs[s], hsum[s]);
        if (s < (JACK ? nbins : out) && rbase + s < LSLOTS) atomicAdd(&a.rsum[s], hsum[rbase + s]);
    }
}

template <bool JACK> static void labels_launch(const PArgs &a, int ndim, int base, unsigned grid, hipStream_t st)
{
    if (base == PMX_PAIRS_2D) labels_kernel<3, PMX_PAIRS_2D, JACK><<<grid, PBLOCK, 0, st>>>(a);
    else if (base == PMX_PAIRS_PROJECTED) labels_kernel<3, PMX_PAIRS_PROJECTED, JACK><<<grid, PBLOCK, 0, st>>>(a);
    else if (base == PMX_PAIRS_2D_MIDPOINT) labels_kernel<3, PMX_PAIRS_2D_MIDPOINT, JACK><<<grid, PBLOCK, 0, st>>>(a);
    else if (base == PMX_PAIRS_PROJECTED_MIDPOINT)
        labels_kernel<3, PMX_PAIRS_PROJECTED_MIDPOINT, JACK><<<grid, PBLOCK, 0, st>>>(a);
    else with_count<3>(ndim, [&](auto nd) { labels_kernel<decltype(nd)::value, PMX_PAIRS_1D, JACK><<<grid, PBLOCK, 0, st>>>(a); });
}

void pairs_labels_launch(const PArgs &a, int ndim, int mode, unsigned grid, hipStream_t st)
{
    // (never: pmx_pair_counts has checked it)
    if (a.nbins < 1 || a.nbins > LSLOTS / 4 || !a.w1.data || !a.w2.data) return;
    const int base = mode & (PMX_PAIRS_SPLIT - 1);
    if (base > PMX_PAIRS_PROJECTED_MIDPOINT || (base != PMX_PAIRS_1D && ndim != 3)) return;
    if (mode & PMX_PAIRS_JACKKNIFE) labels_launch<true>(a, ndim, base, grid, st);
    else labels_launch<false>(a, ndim, base, grid, st);
}

}  // namespace pmx
