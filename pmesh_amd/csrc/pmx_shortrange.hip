// pmx_shortrange.hip — the short-range pair force of particles (include/pmesh_amd.h: pmx_short_range;
// pmesh_amd/shortrange.py).
//
// The other half of a TreePM / P3M force: what MP-Gadget sums over the nodes of its tree below the mesh scale, here
// summed over the pairs of the cell grid.  Its sum with the mesh force filtered by exp(-k^2 r_split^2) is Newton's.
// The rule, restated from the header:
//   rows     (n, 3) rows wrapped into [0, L_d) by FoF's rule; dx_d = x_i,d - x_j,d the minimum image of the wrapped
//            rows (pair_image); all arithmetic in double; r2 = dx_0^2 + dx_1^2 + dx_2^2 in that order
//   cut      source j is a neighbour of primary i when 0 < r2 < rc2, rc2 = r_cut^2 formed on the host; no square root
//            decides it; r2 == 0 (the row itself, a coincident row) contributes nothing
//   force    r = sqrt(r2), u = r / (2 r_split), s2 = r2 + eps2; fac = erfc(u) + (2 / sqrt(pi)) u exp(-u^2);
//            acc_i,d = -G sum_j m_j dx_d fac / (s2 sqrt(s2)); pot_i = -G sum_j m_j erfc(u) / sqrt(s2);
//            neighbours_i = the number of neighbours (exact); erfc and exp are the device's double functions
//   sums     double sums in no particular order; neighbours never varies
// The pass: short_kernel, one wave per slot of the primaries in cell order, four consecutive slots per workgroup (they
// sit in one cell or in adjacent ones and read the same sources from cache).  The lanes of the wave stride over the
// slots of the 27 neighbouring cells, 64 at a time (coalesced loads of spos2), form dx and r2 and test the cut; only
// about 4.19 / 27 of them pass.  The wave compacts those that do — (dx_0, dx_1, dx_2, slot), at the place a ballot and
// a prefix count give — into a ring of 128 entries in LDS that belongs to it alone: no LDS atomic, no barrier.  When
// the ring holds 64 entries, and once at the end, every lane takes one entry and evaluates the force: the erfc, the
// exp, the square roots and the divisions run on full waves.  Four double accumulators per lane are reduced by a
// fixed shuffle tree; the count is the sum of the ballots' populations, the same in every lane.  Lane 0 writes the
// row, through order1: no global atomic, nothing that spans more than one primary, nothing that can overflow.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_cells_dev.h"
#include "pmx_common.h"

namespace pmx {

constexpr int SBLOCK = 256;
constexpr int SWAVES = SBLOCK / 64;              // primaries per workgroup
constexpr int SRING = 128;                       // entries of a wave's ring: at most 63 left over plus 64 new ones

struct SArgs {
    FGeom g;
    int64_t n1, n2, ncells;
    const double *spos1, *spos2;
    const int32_t *order1, *cell_of1, *order2, *cell_start2;
    DVec m2;
    double G, two_rs, rc2, eps2;
    double *acc, *pot;
    long long *neighbours;
};

// the sum over the 64 lanes, in every lane: a fixed tree
__device__ __forceinline__ double short_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool MASS> __global__ void __launch_bounds__(SBLOCK) short_kernel(SArgs a)
{
    // (one array per component: the lanes of a wave write and read consecutive doubles)
    __shared__ double qx[SWAVES][3][SRING];
    __shared__ int32_t qs[SWAVES][SRING];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * SWAVES + wave;
    if (k >= a.n1) return;                                       // (the whole wave: there is no barrier below)
    const int32_t i = a.order1[k];
    if (i < 0 || i >= a.n1) return;                              // (never, with the order fill_kernel left)
    const int32_t flat = a.cell_of1[i];
    const FGeom &g = a.g;
    const double x[3] = {a.spos1[k * 3], a.spos1[k * 3 + 1], a.spos1[k * 3 + 2]};
    const double quarter[3] = {0.25 * g.L[0], 0.25 * g.L[1], 0.25 * g.L[2]};
    const double two_over_sqrt_pi = 1.1283791670955126;
    double ax = 0, ay = 0, az = 0, ap = 0;
    long long found = 0;                                         // the same in every lane
    unsigned head = 0, count = 0;                                // the ring: its first entry and how many it holds

    // every lane below `live` takes the entry head + lane
    auto flush = [&](unsigned live) {
        if (lane < (int)live) {
            const unsigned e = (head + lane) & (SRING - 1);
            const double d0 = qx[wave][0][e], d1 = qx[wave][1][e], d2 = qx[wave][2][e];
            double r2 = 0;
            r2 += d0 * d0;
            r2 += d1 * d1;
            r2 += d2 * d2;
            double m = 1.0;
            if (MASS) {
                const int32_t s = qs[wave][e];
                const int32_t j = a.order2[s];
                m = (j >= 0 && j < a.n2) ? a.m2.get(j, 0) : 0.0;           // (always in range)
            }
            const double s2 = r2 + a.eps2;
            const double ss = sqrt(s2);
            const double r = a.eps2 == 0 ? ss : sqrt(r2);
            const double u = r / a.two_rs;
            const double ec = erfc(u);
            const double fac = ec + two_over_sqrt_pi * u * exp(-(u * u));
            const double f = m * fac / (s2 * ss);
            ax += d0 * f;
            ay += d1 * f;
            az += d2 * f;
            if (a.pot) ap += m * ec / ss;
        }
        head = (head + live) & (SRING - 1);
        count -= live;
    };

    if (flat >= 0 && flat < a.ncells) {                          // (always)
        int32_t c[3];
        fof_cell_axes<3>(g, flat, c);
        // (nb == 27 is the turn after the last cell: it walks nothing and flushes what is left; one flush in the code)
        for (int nb = 0; nb <= 27; nb++) {
            const bool last = nb == 27;
            int32_t s0 = 0, s1 = 0;
            if (!last) {
                int32_t cell;
                if (!fof_neighbour<3>(g, c, nb, cell)) continue;
                s0 = a.cell_start2[cell];
                s1 = a.cell_start2[cell + 1];
                if (s0 < 0) s0 = 0;
                if ((int64_t)s1 > a.n2) s1 = (int32_t)a.n2;
                if (s1 <= s0) continue;
            }
            uint32_t base = (uint32_t)s0;                      // (s1 < 2^31: base + lane stays below 2^32)
            do {
                const uint32_t s = base + (uint32_t)lane;
                bool accept = false;
                double dx[3] = {0, 0, 0};
                if (s < (uint32_t)s1) {
#pragma unroll
                    for (int d = 0; d < 3; d++) dx[d] = pair_image(x[d] - a.spos2[(int64_t)s * 3 + d], g.L[d], quarter[d]);
                    double r2 = 0;
#pragma unroll
                    for (int d = 0; d < 3; d++) r2 += dx[d] * dx[d];
                    accept = r2 > 0 && r2 < a.rc2;
                }
                const unsigned long long mask = __ballot(accept);
                if (accept) {
                    const unsigned e = (head + count + __popcll(mask & ((1ull << lane) - 1ull))) & (SRING - 1);
                    qx[wave][0][e] = dx[0];
                    qx[wave][1][e] = dx[1];
                    qx[wave][2][e] = dx[2];
                    if (MASS) qs[wave][e] = (int32_t)s;
                }
                const unsigned n = __popcll(mask);
                count += n;
                found += n;
                // the ring belongs to this wave: its stores are in order before its loads, and no lane of another
                // wave touches them
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const unsigned live = count >= 64 ? 64u : (last ? count : 0u);
                if (live) {
                    flush(live);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                base += 64;
            } while (base < (uint32_t)s1);
        }
    }
    ax = short_wave_sum(ax);
    ay = short_wave_sum(ay);
    az = short_wave_sum(az);
    if (a.pot) ap = short_wave_sum(ap);
    if (lane == 0) {
        a.acc[(int64_t)i * 3] = -a.G * ax;
        a.acc[(int64_t)i * 3 + 1] = -a.G * ay;
        a.acc[(int64_t)i * 3 + 2] = -a.G * az;
        if (a.pot) a.pot[i] = -a.G * ap;
        if (a.neighbours) a.neighbours[i] = found;
    }
}

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_short_range(int64_t n1, const double *spos1, const int32_t *order1, const int32_t *cell_of1,
                               int64_t n2, const double *spos2, const int32_t *order2, const int32_t *cell_start2,
                               const pmx_vec *mass2, const int64_t *ncell, int32_t periodic, const double *boxsize,
                               double G, double r_split, double rc2, double eps2, double *acc, double *pot,
                               int64_t *neighbours, void *stream)
{
    SArgs a;
    const int rc = fof_geom(3, boxsize, nullptr, nullptr, ncell, periodic, a.g, &a.ncells);
    if (rc != PMX_OK) return rc;
    PMX_REQUIRE(n1 >= 0 && n2 >= 0, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(n1 <= PMX_FOF_MAX_ROWS && n2 <= PMX_FOF_MAX_ROWS, PMX_EUNSUPPORTED,
                "more than 2^31 - 1 rows: slots are 32-bit");
    PMX_REQUIRE(isfinite(G) && r_split > 0 && isfinite(r_split) && rc2 > 0 && isfinite(rc2) && eps2 >= 0 &&
                isfinite(eps2), PMX_EINVAL, "G, r_split, rc2 and eps2 must be finite, r_split and rc2 positive");
    if (n1 == 0) return PMX_OK;
    PMX_REQUIRE(acc, PMX_EINVAL, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (n2 == 0) {
        // the outputs are overwritten: no source, no force
        PMX_HIP_CHECK(hipMemsetAsync(acc, 0, sizeof(double) * 3 * n1, st));
        if (pot) PMX_HIP_CHECK(hipMemsetAsync(pot, 0, sizeof(double) * n1, st));
        if (neighbours) PMX_HIP_CHECK(hipMemsetAsync(neighbours, 0, sizeof(int64_t) * n1, st));
        return PMX_OK;
    }
    PMX_REQUIRE(spos1 && order1 && cell_of1 && spos2 && order2 && cell_start2, PMX_EINVAL, "bad arguments");
    const bool mass = mass2 && mass2->data;
    PMX_REQUIRE(!mass || vec_ok(mass2), PMX_EINVAL, "mass2 must be float or double");
    a.n1 = n1;
    a.n2 = n2;
    a.spos1 = spos1;
    a.spos2 = spos2;
    a.order1 = order1;
    a.cell_of1 = cell_of1;
    a.order2 = order2;
    a.cell_start2 = cell_start2;
    a.m2 = dvec(mass ? mass2 : nullptr);
    a.G = G;
    a.two_rs = 2.0 * r_split;
    a.rc2 = rc2;
    a.eps2 = eps2;
    a.acc = acc;
    a.pot = pot;
    a.neighbours = (long long *)neighbours;
    const unsigned grid = (unsigned)((n1 + SWAVES - 1) / SWAVES);
    with_bool(mass, [&](auto m) { short_kernel<decltype(m)::value><<<grid, SBLOCK, 0, st>>>(a); });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
