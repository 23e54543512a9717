// pmx_lpt_dev.h — what the streaming kernels over spectra and real blocks of pmx_lpt.hip, pmx_lpt_grad.hip and
// pmx_ktable_grad.hip share: the block geometry in logical order with its memory-order walk (PMX_LPT_LOOP), the
// wavevector of an element from its index (pmx_common.h: wavenumber, the roundings of transfer_kernel), complex loads
// and stores of f4 / f8 storage into double, the search and interpolation of a pmx_ktable, and the host side that
// builds the geometry and the launch grid.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"

namespace pmx {

struct LGeom {
    int64_t shape[3], start[3], nmesh[3];   // logical order
    double dw[3], nl[3];                    // 2 pi / N and N / L per axis
    int32_t ax[3];                          // memory-order permutation: ax[2] varies fastest
    int32_t ndim;
};

struct LStr {
    int64_t s[3];                           // byte strides, logical order
    __device__ __forceinline__ int64_t off(const int64_t *idx) const { return idx[0] * s[0] + idx[1] * s[1] + idx[2] * s[2]; }
};

// grid.y walks the slowest memory axis, grid.x / threads the flattened two fast axes (as transfer_kernel): 32-bit
// index arithmetic inside a plane, consecutive threads on consecutive elements
#define PMX_LPT_LOOP(g)                                                                                            \
    const uint32_t n1_ = (uint32_t)(g).shape[(g).ax[1]], n2_ = (uint32_t)(g).shape[(g).ax[2]];                     \
    const uint32_t inner_ = n1_ * n2_;                                                                             \
    for (int64_t i0_ = blockIdx.y; i0_ < (g).shape[(g).ax[0]]; i0_ += gridDim.y)                                   \
    for (uint32_t q_ = blockIdx.x * blockDim.x + threadIdx.x; q_ < inner_; q_ += gridDim.x * blockDim.x)

__device__ __forceinline__ void block_index(const LGeom &g, int64_t i0, uint32_t q, int64_t *idx)
{
    const uint32_t n2 = (uint32_t)g.shape[g.ax[2]];
    const uint32_t i1 = q / n2;
    const int64_t v0 = i0, v1 = i1, v2 = q - i1 * n2;
#pragma unroll
    for (int d = 0; d < 3; d++) idx[d] = (g.ax[0] == d) ? v0 : ((g.ax[1] == d) ? v1 : v2);
}

// k_d per axis (0 beyond ndim) and k^2 = (k_0^2 + k_1^2) + k_2^2
__device__ __forceinline__ double wavevector(const LGeom &g, const int64_t *idx, double *kk)
{
    double k2 = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        kk[d] = 0;
        if (d >= g.ndim) continue;
        kk[d] = wavenumber(idx[d] + g.start[d], g.nmesh[d], g.dw[d], g.nl[d]);
        k2 += kk[d] * kk[d];
    }
    return k2;
}

template <typename T> struct CLoad;
template <> struct CLoad<double> {
    static __device__ __forceinline__ void get(const char *p, double &re, double &im)
    {
        double2 v = *(const double2 *)p;
        re = v.x;
        im = v.y;
    }
    static __device__ __forceinline__ void put(char *p, double re, double im) { *(double2 *)p = make_double2(re, im); }
};
template <> struct CLoad<float> {
    static __device__ __forceinline__ void get(const char *p, double &re, double &im)
    {
        float2 v = *(const float2 *)p;
        re = v.x;
        im = v.y;
    }
    static __device__ __forceinline__ void put(char *p, double re, double im)
    {
        *(float2 *)p = make_float2((float)re, (float)im);
    }
};

// j with x[j] <= u < x[j + 1] for x[0] < u < x[n - 1] (the table search of pmx_apply_ktable and its gradients): binary
// search, started from the closed-form guess j = (u - x[0]) * inv_step of a uniform table (inv_step > 0), which
// narrows the search to one side of the guess and ends it at once when the guess holds
__device__ __forceinline__ int table_find(const double *x, int n, double inv_step, double u)
{
    int lo = 0, hi = n - 1;     // x[lo] <= u < x[hi]
    if (inv_step > 0) {
        const double t = (u - x[0]) * inv_step;
        const int g = t < 0 ? 0 : (t > n - 2 ? n - 2 : (int)t);
        if (x[g] <= u) {
            lo = g;
            if (u < x[g + 1]) hi = g + 1;
        } else {
            hi = g;
        }
    }
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (x[m] <= u) lo = m;
        else hi = m;
    }
    return lo;
}

// numpy.interp(u, x, y) with its end values outside [x[0], x[n-1]]
__device__ __forceinline__ double table_interp(const double *x, const double *y, int n, double inv_step, double u)
{
    if (u <= x[0]) return y[0];
    if (u >= x[n - 1]) return y[n - 1];
    const int lo = table_find(x, n, inv_step, u);
    const double xl = x[lo], yl = y[lo];
    if (xl == u) return yl;
    const double s = (y[lo + 1] - yl) / (x[lo + 1] - xl);
    return s * (u - xl) + yl;
}

// the block geometry, axes ordered by decreasing |stride| of `order` (the rule of pmx_apply_transfer)
static LGeom make_geom(int32_t ndim, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                       const double *boxsize, const int64_t *order)
{
    LGeom g;
    g.ndim = ndim;
    int64_t os[3];
    for (int d = 0; d < 3; d++) {
        const bool on = d < ndim;
        g.shape[d] = on ? shape[d] : 1;
        g.start[d] = on && start ? start[d] : 0;
        g.nmesh[d] = on && nmesh ? nmesh[d] : 1;
        const double L = on && boxsize ? boxsize[d] : 1.0;
        g.dw[d] = 2 * M_PI / g.nmesh[d];
        g.nl[d] = g.nmesh[d] / L;
        os[d] = on ? order[d] : 0;
    }
    int ax[3] = {0, 1, 2};
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++) {
            int64_t sa = llabs(os[ax[a]]), sb = llabs(os[ax[b]]);
            bool swap = sa < sb || (sa == sb && g.shape[ax[a]] == 1 && g.shape[ax[b]] != 1);
            if (swap) { int tmp = ax[a]; ax[a] = ax[b]; ax[b] = tmp; }
        }
    for (int a = 0; a < 3; a++) g.ax[a] = ax[a];
    return g;
}

static LStr make_str(int32_t ndim, const int64_t *s)
{
    LStr r;
    for (int d = 0; d < 3; d++) r.s[d] = d < ndim ? s[d] : 0;
    return r;
}

// 0: nothing to do; -1: a plane too large for the 32-bit index
static int grid_of(const LGeom &g, dim3 &grid)
{
    if (g.shape[0] * g.shape[1] * g.shape[2] == 0) return 0;
    const int64_t inner = g.shape[g.ax[1]] * g.shape[g.ax[2]];
    if (inner >= (1ll << 31)) return -1;
    const int64_t n0 = g.shape[g.ax[0]];
    grid = dim3((unsigned)((inner + 255) / 256), (unsigned)(n0 < 65535 ? n0 : 65535));
    return 1;
}

}  // namespace pmx
