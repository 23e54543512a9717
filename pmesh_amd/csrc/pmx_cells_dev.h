// pmx_cells_dev.h — the cell grid of particles that pmx_fof.hip and pmx_pairs.hip share: the wrapping rule, the minimum
// image, the cell of a row and the walk over the 3^ndim neighbouring cells (include/pmesh_amd.h, "The grid").
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"

namespace pmx {

struct FGeom {
    double L[3], origin[3], inv[3], extent[3];
    int32_t nc[3];
    int32_t periodic;                            // bit d: axis d wraps
};

// x wrapped into [0, L): the rule of the header
__device__ __forceinline__ double fof_wrap(double x, double L)
{
    double w = x - L * floor(x / L);
    if (w < 0) w += L;
    if (!(w < L)) w = 0;                         // (-tiny + L rounds to L; a coordinate that is not finite)
    return w;
}

// the minimum image of dx
__device__ __forceinline__ double fof_image(double dx, double L) { return dx - L * rint(dx / L); }

// the cell of the wrapped coordinate w along axis d
__device__ __forceinline__ int32_t fof_cell(const FGeom &g, int d, double w)
{
    double r = w - g.origin[d];
    if (r < 0) r += g.L[d];
    const int32_t last = g.nc[d] - 1;
    if (!((g.periodic >> d) & 1) && r >= g.extent[d])
        return (g.L[d] - r < r - g.extent[d]) ? 0 : last;     // beyond an open axis: the nearer end
    const double t = r * g.inv[d];
    if (!(t >= 0)) return 0;
    return t >= (double)last ? last : (int32_t)t;
}

// the per-axis cell c[] of the flat (C order) cell index
template <int NDIM> __device__ __forceinline__ void fof_cell_axes(const FGeom &g, int32_t flat, int32_t c[3])
{
    c[0] = c[1] = c[2] = 0;
#pragma unroll
    for (int d = NDIM - 1; d >= 0; d--) {
        c[d] = flat % g.nc[d];
        flat /= g.nc[d];
    }
}

// the nb-th of the 3^NDIM neighbours of the cell c[] (nb = 0 .. 3^NDIM - 1, the cell itself among them): its flat
// index into `cell`, or false where there is none — beyond an open axis, or a cell that another nb names already:
// along a periodic axis of one cell the cell itself once; of two cells the other one once (offset -1, not +1 as well)
template <int NDIM>
__device__ __forceinline__ bool fof_neighbour(const FGeom &g, const int32_t c[3], int nb, int32_t &cell)
{
    const int o[3] = {nb % 3 - 1, NDIM > 1 ? (nb / 3) % 3 - 1 : 0, NDIM > 2 ? nb / 9 - 1 : 0};
    bool skip = false;
    cell = 0;
#pragma unroll
    for (int d = 0; d < NDIM; d++) {
        const int32_t nc = g.nc[d];
        int32_t cc = c[d] + o[d];
        if ((g.periodic >> d) & 1) {
            if ((nc == 1 && o[d] != 0) || (nc == 2 && o[d] == 1)) skip = true;
            if (cc < 0) cc += nc;
            if (cc >= nc) cc -= nc;
        } else if (cc < 0 || cc >= nc) {
            skip = true;
        }
        cell = cell * nc + cc;
    }
    return !skip;
}

template <int NDIM> constexpr int fof_neighbours() { return NDIM == 1 ? 3 : (NDIM == 2 ? 9 : 27); }

// the bins of an axis: up to this many are searched by a linear walk from the outermost, more by bisection
constexpr int PAIRS_LINEAR = 8;

// the minimum image of dx = w - w', both in [0, L): fof_image without its division where the quotient is known.
// |dx| <= L / 4 (exact: a power of two times L) gives |dx / L| <= 1/4 after rounding, rint of it 0, and dx - L * 0 = dx.
__device__ __forceinline__ double pair_image(double dx, double L, double quarter)
{
    return fabs(dx) <= quarter ? dx : fof_image(dx, L);
}

// the largest k in 0 .. n - 1 with q >= tab[k], given q >= tab[0]; tab increasing
template <typename P> __device__ __forceinline__ int pair_bin(P tab, int n, double q)
{
    if (n <= PAIRS_LINEAR) {
        int k = n - 1;
        while (k > 0 && q < tab[k]) k--;
        return k;
    }
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (q >= tab[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the grid of a launch, checked (origin and inv_side may be NULL for the passes that only walk cells)
static inline int fof_geom(int32_t ndim, const double *boxsize, const double *origin, const double *inv_side,
                           const int64_t *ncell, int32_t periodic, FGeom &g, int64_t *ncells)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3, PMX_EINVAL, "ndim must be 1, 2 or 3");
    PMX_REQUIRE(boxsize && ncell, PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(periodic >= 0 && periodic < (PMX_FOF_PERIODIC_X << 3), PMX_EINVAL, "bad periodic mask");
    g.periodic = periodic;
    *ncells = 1;
    for (int d = 0; d < 3; d++) {
        const bool on = d < ndim;
        g.L[d] = on ? boxsize[d] : 1.0;
        g.origin[d] = on && origin ? origin[d] : 0.0;
        g.inv[d] = on && inv_side ? inv_side[d] : 1.0;
        g.nc[d] = 1;
        PMX_REQUIRE(g.L[d] > 0 && isfinite(g.L[d]), PMX_EINVAL, "bad boxsize");
        PMX_REQUIRE(isfinite(g.origin[d]) && g.inv[d] > 0 && isfinite(g.inv[d]), PMX_EINVAL, "bad grid");
        if (on) {
            PMX_REQUIRE(ncell[d] >= 1 && ncell[d] <= PMX_FOF_MAX_ROWS, PMX_EINVAL, "bad cell count");
            g.nc[d] = (int32_t)ncell[d];
        }
        g.extent[d] = (double)g.nc[d] / g.inv[d];
        PMX_REQUIRE(*ncells <= PMX_FOF_MAX_ROWS / g.nc[d], PMX_EUNSUPPORTED, "more than 2^31 - 1 cells");
        *ncells *= g.nc[d];
    }
    return PMX_OK;
}

}  // namespace pmx
