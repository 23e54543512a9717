// pmx_threept.hip — multipoles of the three-point function of particles (include/pmesh_amd.h: pmx_threept_multipoles;
// pmesh_amd/threept.py).
//
// Replaces what a caller of the reference does on the host for the isotropic three-point function of a catalogue
// (nbodykit's SimulationBox3PCF: a kd-tree over the rows copied over PCIe).  The rule, restated from the header:
//   rows     (n, 3) rows wrapped into [0, L_d) by FoF's rule; dx_d the minimum image of the wrapped rows; all arithmetic
//            in double; r2 = dx_0^2 + dx_1^2 + dx_2^2 in that order
//   bins     row j is a neighbour of i in bin b when e2[b] <= r2 < e2[b + 1], e2 the squared edges formed on the host;
//            a pair with r2 == 0 is never a neighbour: it has no direction
//   dir      r = sqrt(r2), u_d = dx_d / r
//   sums     zeta_l[b1, b2] = sum_i w_i sum_{j in N_i(b1)} sum_{k in N_i(b2)} w_j w_k P_l(u_ij . u_ik), j == k included;
//            diag[b] = sum_i w_i sum_j w_j^2, wpairs[b] = sum_i w_i sum_j w_j, npairs[b] = sum_i |N_i(b)| (exact)
//   how      per primary A_{l,c}(b) = sum_j w_j Y_{l,c}(u_ij) over the 2 l + 1 real components Y = N_lm Q_l^m(u_z)
//            Re / Im (u_x + i u_y)^m, N_lm = sqrt(eps_m (l - m)! / (l + m)!), Q_l^m = P_l^m / sin^m by its recurrence
//            in l; by the addition theorem zeta_l += w_i sum_c A_{l,c}(b1) A_{l,c}(b2)
// The pass: threept_kernel.  One workgroup of 256 lanes takes `run` consecutive slots of the primaries in cell order
// and treats them one after another.  For one primary
//   walk     the slots of its 27 neighbouring cells are one flat range (their starts and a running sum in LDS, laid
//            again only when the cell changes); the lanes stride over it, 256 slots at a time.  A lane whose slot
//            passes the edge test appends (u_x, u_y, u_z, w, bin) to the chunk in LDS, at the place a wave ballot and
//            the counts of the waves before it give: the order of the chunk is the order of the slots.
//   flush    when the chunk is full, and at the end of the walk: (a) lane (entry, m mod MG) runs the recurrence of
//            Q_l^m in l for its m and stores w Y to the tile [entry][component]; (b) lane (component, g) walks the
//            entries whose bin is g mod G and adds the tile's value into A[bin][component]: every word of A has one
//            owner, so these are plain read-modify-writes in the order of the entries.  The lanes below nr count the
//            entries of their bin (and sum w^2 where there are weights).
//   output   lane t owns the pairs of bins b1 >= b2 numbered t, t + 256 and t + 512, every l of each, in registers for
//            the whole run (register arrays with compile-time bounds; few pairs are shared by several lanes, each
//            taking some of the l); it adds w_i sum_c A[b1][c] A[b2][c] where both bins hold a neighbour.
// At its end the workgroup makes one global atomic per non-zero output b1 >= b2 and bin; threept_mirror_kernel then
// copies the lower triangle of every zeta_l to the upper one, so that the matrix is symmetric to the last bit.  No
// 32-bit counter spans more than one primary, and a primary has fewer than 2^31 neighbours because n2 < 2^31: the
// secondaries need no launch windows.  Barriers stand only between the phases.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_cells_dev.h"
#include "pmx_common.h"

namespace pmx {

constexpr int TBLOCK = 256;
constexpr int TWAVES = TBLOCK / 64;
constexpr int TBINS = PMX_THREEPT_MAX_BINS;
constexpr int TTRI = TBINS * (TBINS + 1) / 2;    // the pairs b1 >= b2 of 32 bins
constexpr int TCELLS = 27;
constexpr int KPAIR = (TTRI + TBLOCK - 1) / TBLOCK;       // the pairs of bins a lane owns: 3

struct TArgs {
    FGeom g;
    int64_t n1, n2;
    const double *spos1, *spos2;
    const int32_t *order1, *cell_of1, *order2, *cell_start2;
    DVec w1, w2;
    int64_t ncells;
    int32_t nr, lmax, run;
    const double *e2;
    double *zeta, *diag, *wpairs;
    unsigned long long *npairs;
};

// LMAX: the class of the call, 4 or 10: the stride of the components, the length of the chunk and the accumulators of
// a lane are compile-time; the lmax of the call (<= LMAX) bounds the loops.
template <int LMAX> struct TShape {
    static constexpr int NC = (LMAX + 1) * (LMAX + 1);           // 25 or 121 components: odd strides in LDS
    static constexpr int CH = LMAX <= 4 ? 64 : 32;               // entries of a chunk
    static constexpr int MG = TBLOCK / CH;                       // lanes per entry in phase (a)
};

// (the low class is held to the registers of three waves per SIMD, three workgroups per CU, which its 24 KB of LDS admit; the
// high class is at two by its LDS)
template <bool WEIGHTED, int LMAX>
__global__ void __launch_bounds__(TBLOCK) __attribute__((amdgpu_waves_per_eu(LMAX <= 4 ? 3 : 2)))
threept_kernel(TArgs a)
{
    using S = TShape<LMAX>;
    constexpr int NC = S::NC, CH = S::CH, MG = S::MG;
    __shared__ double A[TBINS * NC];
    __shared__ double tile[CH * NC];
    __shared__ double cu[CH][4];                                 // u_x, u_y, u_z, w of an entry
    __shared__ int32_t cbin[CH];                                 // bin | (bin mod G) << 8
    __shared__ double se2[TBINS + 1];
    __shared__ double norm[(PMX_THREEPT_MAX_ELL + 1) * (PMX_THREEPT_MAX_ELL + 1)];   // N_lm at [l * 11 + m]
    __shared__ uint16_t tri[TTRI];                               // b1 << 8 | b2 of the pair numbered b1 (b1 + 1) / 2 + b2
    __shared__ int32_t seg_start[TCELLS], seg_pref[TCELLS + 1];
    __shared__ int32_t wtot[2][TWAVES];
    __shared__ int32_t hit[TBINS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr = a.nr, lmax = a.lmax;
    const int ncomp = (lmax + 1) * (lmax + 1);
    const int ntri = nr * (nr + 1) / 2;
    int G = TBLOCK / ncomp;                                      // groups of bins in phase (b)
    if (G > nr) G = nr;

    for (int s = tid; s <= nr; s += TBLOCK) se2[s] = a.e2[s];
    if (tid < nr)
        for (int b2 = 0; b2 <= tid; b2++) tri[tid * (tid + 1) / 2 + b2] = (uint16_t)(tid << 8 | b2);
    for (int s = tid; s < (PMX_THREEPT_MAX_ELL + 1) * (PMX_THREEPT_MAX_ELL + 1); s += TBLOCK) {
        const int l = s / (PMX_THREEPT_MAX_ELL + 1), m = s % (PMX_THREEPT_MAX_ELL + 1);
        double v = 0;
        if (m <= l) {
            double p = 1.0;                                      // (l + m)! / (l - m)!
            for (int k = l - m + 1; k <= l + m; k++) p *= (double)k;
            v = sqrt((m == 0 ? 1.0 : 2.0) / p);
        }
        norm[s] = v;
    }
    __syncthreads();

    // the outputs of this lane: the pairs b1 >= b2 numbered tid, tid + 256 and tid + 512, every l of each.  Where the
    // pairs fill half the lanes or less, nsplit lanes share a pair: lane (pair, part) takes the l with l mod nsplit == part
    int nsplit = ntri <= TBLOCK / 2 ? TBLOCK / ntri : 1;
    if (nsplit > lmax + 1) nsplit = lmax + 1;
    const int part = nsplit > 1 ? tid / ntri : 0;
    int32_t code[KPAIR];                                         // b1 << 8 | b2, or -1
    double acc[KPAIR][LMAX + 1];
#pragma unroll
    for (int j = 0; j < KPAIR; j++) {
        const int t = j == 0 && nsplit > 1 ? tid % ntri : tid + TBLOCK * j;
        code[j] = t < ntri && part < nsplit ? (int32_t)tri[t] : -1;
#pragma unroll
        for (int l = 0; l <= LMAX; l++) acc[j][l] = 0;
    }
    unsigned long long tot_n = 0;                                // of bin tid, where tid < nr
    double tot_diag = 0, tot_wp = 0;

    const FGeom &g = a.g;
    const double quarter[3] = {0.25 * g.L[0], 0.25 * g.L[1], 0.25 * g.L[2]};
    const double qlo = a.e2[0], qhi = a.e2[nr];
    const int64_t k0 = (int64_t)blockIdx.x * a.run;
    const int64_t k1 = k0 + a.run < a.n1 ? k0 + a.run : a.n1;
    int32_t curcell = -1;
    int parity = 0;

    for (int64_t k = k0; k < k1; k++) {
        // (everything that decides a branch around a barrier is the same in every lane: it comes from k alone)
        const int32_t i = a.order1[k];
        if (i < 0 || i >= a.n1) continue;                        // (never, with the order fill_kernel left)
        const int32_t flat = a.cell_of1[i];
        if (flat < 0 || flat >= a.ncells) continue;              // (never)
        const double x[3] = {a.spos1[k * 3], a.spos1[k * 3 + 1], a.spos1[k * 3 + 2]};
        double w1 = 1.0;
        if (WEIGHTED && a.w1.data) w1 = a.w1.get(i, 0);

        if (flat != curcell) {
            curcell = flat;
            if (tid < TCELLS) {
                int32_t c[3], cell;
                fof_cell_axes<3>(g, flat, c);
                int32_t s0 = 0, len = 0;
                if (fof_neighbour<3>(g, c, tid, cell)) {
                    s0 = a.cell_start2[cell];
                    int32_t s1 = a.cell_start2[cell + 1];
                    if (s0 < 0) s0 = 0;
                    if ((int64_t)s1 > a.n2) s1 = (int32_t)a.n2;
                    len = s1 > s0 ? s1 - s0 : 0;
                }
                seg_start[tid] = s0;
                seg_pref[tid + 1] = len;
            }
            __syncthreads();
            if (tid == 0) {
                int32_t sum = 0;                                 // (at most n2 < 2^31: the cells are distinct)
                seg_pref[0] = 0;
                for (int c = 0; c < TCELLS; c++) {
                    sum += seg_pref[c + 1];
                    seg_pref[c + 1] = sum;
                }
            }
        }
        for (int s = tid; s < nr * NC; s += TBLOCK) A[s] = 0;
        if (tid < nr) hit[tid] = 0;
        __syncthreads();
        const int32_t total = seg_pref[TCELLS];
        int count = 0;                                           // the entries of the chunk
        int found = 0;                                           // whether this primary has a neighbour at all
        uint32_t pn = 0;                                         // of bin tid: the neighbours of this primary
        double pd = 0;                                           // and the sum of their w^2

        // one flush of the chunk: phases (a) and (b); ends with a barrier
        auto flush = [&]() {
            __syncthreads();
            {
                const int e = tid % CH, mg = tid / CH;
                if (e < count) {
                    const double ux = cu[e][0], uy = cu[e][1], uz = cu[e][2], w = cu[e][3];
                    double *out = &tile[e * NC];
                    for (int m = mg; m <= lmax; m += MG) {
                        double re = 1.0, im = 0.0;               // (u_x + i u_y)^m
                        double qmm = 1.0;                        // Q_m^m = (2 m - 1)!!
                        for (int t = 1; t <= m; t++) {
                            const double nre = re * ux - im * uy;
                            im = re * uy + im * ux;
                            re = nre;
                            qmm *= (double)(2 * t - 1);
                        }
                        double q2 = 0.0, q1 = qmm;               // Q_{l-2}^m, Q_{l-1}^m on entering l; q1 is Q_l^m below
                        for (int l = m; l <= lmax; l++) {
                            if (l == m + 1) {
                                const double q = (double)(2 * m + 1) * uz * qmm;
                                q2 = q1;
                                q1 = q;
                            } else if (l > m + 1) {
                                const double q = ((double)(2 * l - 1) * uz * q1 - (double)(l + m - 1) * q2) / (double)(l - m);
                                q2 = q1;
                                q1 = q;
                            }
                            const double nq = norm[l * (PMX_THREEPT_MAX_ELL + 1) + m] * q1;
                            if (m == 0) {
                                out[l * l] = w * (nq * re);
                            } else {
                                out[l * l + 2 * m - 1] = w * (nq * re);
                                out[l * l + 2 * m] = w * (nq * im);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            {
                const int c = tid % ncomp, grp = tid / ncomp;
                if (grp < G)
                    for (int e = 0; e < count; e++) {
                        const int32_t cb = cbin[e];
                        if ((cb >> 8) == grp) A[(cb & 255) * NC + c] += tile[e * NC + c];
                    }
                if (WEIGHTED && tid < nr)
                    for (int e = 0; e < count; e++)
                        if ((cbin[e] & 255) == tid) {
                            const double w = cu[e][3];
                            pn++;
                            pd += w * w;
                        }
            }
            count = 0;
            __syncthreads();
        };

        for (int32_t base = 0; base < total; base += TBLOCK) {
            const int32_t t = base + tid;
            bool accept = false;
            double ux = 0, uy = 0, uz = 0, w = 1.0;
            int bin = 0;
            if (t < total) {
                int c = 0;                                       // the segment of t: the last with seg_pref[c] <= t
                if (t >= seg_pref[16]) c = 16;
                if (t >= seg_pref[c + 8]) c += 8;
                if (c + 4 <= TCELLS - 1 && t >= seg_pref[c + 4]) c += 4;
                if (c + 2 <= TCELLS - 1 && t >= seg_pref[c + 2]) c += 2;
                if (c + 1 <= TCELLS - 1 && t >= seg_pref[c + 1]) c += 1;
                const int32_t s = seg_start[c] + (t - seg_pref[c]);
                if (s >= 0 && (int64_t)s < a.n2) {               // (always)
                    double dx[3];
#pragma unroll
                    for (int d = 0; d < 3; d++)
                        dx[d] = pair_image(x[d] - a.spos2[(int64_t)s * 3 + d], g.L[d], quarter[d]);
                    double q = 0;
#pragma unroll
                    for (int d = 0; d < 3; d++) q += dx[d] * dx[d];
                    if (q >= qlo && q < qhi && q > 0) {
                        accept = true;
                        if (WEIGHTED && a.w2.data) {
                            const int32_t j = a.order2[s];
                            if (j < 0 || j >= a.n2) accept = false;        // (never)
                            else w = a.w2.get(j, 0);
                        }
                        bin = pair_bin(se2, nr, q);
                        if (bin < 0 || bin >= nr) accept = false;          // (never)
                        const double r = sqrt(q);
                        ux = dx[0] / r;
                        uy = dx[1] / r;
                        uz = dx[2] / r;
                    }
                }
            }
            // the place of this lane's entry among the accepted of the stride
            const unsigned long long mask = __ballot(accept);
            if (lane == 0) wtot[parity][wave] = __popcll(mask);
            __syncthreads();
            int rank = __popcll(mask & ((1ull << lane) - 1ull)), T = 0;
#pragma unroll
            for (int v = 0; v < TWAVES; v++) {
                const int n = wtot[parity][v];
                if (v < wave) rank += n;
                T += n;
            }
            parity ^= 1;
            if (T) found = 1;
            int placed = 0;
            while (placed < T) {
                const int room = CH - count;
                if (accept && rank >= placed && rank < placed + room) {
                    const int e = count + rank - placed;
                    cu[e][0] = ux;
                    cu[e][1] = uy;
                    cu[e][2] = uz;
                    cu[e][3] = w;
                    cbin[e] = bin | (bin % G) << 8;
                    hit[bin] = 1;
                }
                const int added = T - placed < room ? T - placed : room;
                count += added;
                placed += added;
                if (count == CH) flush();
            }
        }
        if (count) flush();
        else __syncthreads();

        if (found) {
#pragma unroll
            for (int j = 0; j < KPAIR; j++) {
                const int32_t cd = code[j];
                if (cd < 0) continue;
                const int b1 = cd >> 8, b2 = cd & 255;
                if (!(hit[b1] && hit[b2])) continue;
                const double *p1 = &A[b1 * NC], *p2 = &A[b2 * NC];
#pragma unroll
                for (int l = 0; l <= LMAX; l++) {
                    if (l > lmax || (nsplit > 1 && l % nsplit != part)) continue;
                    double sum = 0;
#pragma unroll
                    for (int c = l * l; c < (l + 1) * (l + 1); c++) sum += p1[c] * p2[c];
                    acc[j][l] += w1 * sum;
                }
            }
            if (tid < nr && hit[tid]) {
                const double s0 = A[tid * NC];                   // sum of w_j: N_00 Q_0^0 = 1
                if (WEIGHTED) {
                    tot_n += pn;
                    tot_diag += w1 * pd;
                    tot_wp += w1 * s0;
                } else {
                    tot_n += (unsigned long long)s0;             // a sum of ones: an integer below 2^31
                    tot_diag += s0;
                    tot_wp += s0;
                }
            }
        }
        __syncthreads();                                         // before A, hit and the segments are laid again
    }

#pragma unroll
    for (int j = 0; j < KPAIR; j++) {
        const int32_t cd = code[j];
        if (cd < 0) continue;
        const int b1 = cd >> 8, b2 = cd & 255;
#pragma unroll
        for (int l = 0; l <= LMAX; l++) {
            if (l > lmax || acc[j][l] == 0) continue;
            double *z = a.zeta + (int64_t)l * nr * nr;
            atomicAdd(&z[b1 * nr + b2], acc[j][l]);
        }
    }
    if (tid < nr && tot_n) {
        atomicAdd(&a.npairs[tid], tot_n);
        atomicAdd(&a.diag[tid], tot_diag);
        atomicAdd(&a.wpairs[tid], tot_wp);
    }
}

// zeta[l, b2, b1] = zeta[l, b1, b2] for b1 > b2: the two halves are equal to the last bit, whatever the order in which
// the workgroups added into the lower one
__global__ void threept_mirror_kernel(double *zeta, int nr, int total)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int b2 = t % nr, b1 = (t / nr) % nr;
    if (b1 > b2) zeta[(int64_t)(t / (nr * nr)) * nr * nr + b2 * nr + b1] = zeta[t];
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_threept_multipoles(int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1,
                                      const pmx_vec *weight1, int64_t n2, const double *spos2, const int32_t *order2,
                                      const int32_t *cell_start2, const pmx_vec *weight2, const int64_t *ncell,
                                      int32_t periodic, const double *boxsize, int32_t nr, const double *e2,
                                      int32_t lmax, double *zeta, double *diag, double *wpairs, int64_t *npairs,
                                      void *stream)
{
    TArgs a;
    const int rc = fof_geom(3, boxsize, nullptr, nullptr, ncell, periodic, a.g, &a.ncells);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(nr >= 1 && nr <= PMX_THREEPT_MAX_BINS, PMX_EINVAL, "nr must be 1 .. PMX_THREEPT_MAX_BINS");
    PMX_REQUIRE(lmax >= 0 && lmax <= PMX_THREEPT_MAX_ELL, PMX_EINVAL, "lmax must be 0 .. PMX_THREEPT_MAX_ELL");
    PMX_REQUIRE(n1 >= 0 && n2 >= 0, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(n1 <= PMX_FOF_MAX_ROWS && n2 <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED,
                "more than 2^31 - 1 rows: slots are 32-bit");
    if (n1 == 0 || n2 == 0) return PMX_OK;
    PMX_REQUIRE(spos1 && order1 && cell_of1 && spos2 && order2 && cell_start2, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(e2 && zeta && diag && wpairs && npairs, PMX_EINVAL, "bad arguments");
    const bool has1 = weight1 && weight1->data, has2 = weight2 && weight2->data;
    PMX_REQUIRE(!has1 || vec_ok(weight1), PMX_EINVAL, "weight1 must be float or double");
    PMX_REQUIRE(!has2 || vec_ok(weight2), PMX_EINVAL, "weight2 must be float or double");
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
    a.lmax = lmax;
    a.e2 = e2;
    a.zeta = zeta;
    a.diag = diag;
    a.wpairs = wpairs;
    a.npairs = (unsigned long long *)npairs;
    // the run of a workgroup: at most 4096 workgroups (their atomics at the end meet on nr nr (lmax + 1) words), at
    // least 16 primaries each
    int64_t run = (n1 + 4095) / 4096;
    if (run < 16) run = 16;
    a.run = (int32_t)run;
    const unsigned grid = (unsigned)((n1 + run - 1) / run);
    hipStream_t st = (hipStream_t)stream;
    with_bool(has1 || has2, [&](auto w) {
        if (lmax <= 4) threept_kernel<decltype(w)::value, 4><<<grid, TBLOCK, 0, st>>>(a);
        else threept_kernel<decltype(w)::value, 10><<<grid, TBLOCK, 0, st>>>(a);
    });
    const int total = (lmax + 1) * nr * nr;
    threept_mirror_kernel<<<(total + TBLOCK - 1) / TBLOCK, TBLOCK, 0, st>>>(zeta, nr, total);
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
