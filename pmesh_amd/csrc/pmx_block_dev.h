// pmx_block_dev.h — how a strided block of a spectrum or of a real field is walked, one element per thread, and what
// wavenumber a mode has.  Every streaming kernel over such a block (pmx_transfer.hip, pmx_lpt.hip, pmx_lpt_grad.hip,
// pmx_ktable_grad.hip, the shell split of pmx_bispec.hip) takes its geometry, its loop, its wavevector and its complex
// loads from here; pmx_power_dev.h, whose tiles walk differently, takes the axis order, the wavenumber, the sinc power
// and the loads.  Also the search and interpolation of a pmx_ktable.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"

namespace pmx {

struct BlockGeom {
    int64_t shape[3], start[3], nmesh[3];   // logical order (axes beyond ndim: extent 1, start 0, N = 1)
    double boxsize[3];                      // L per axis (1 beyond ndim)
    double dw[3], nl[3];                    // 2 pi / N and N / L per axis
    int32_t ax[3];                          // memory-order permutation: ax[2] varies fastest
    int32_t ndim;
};

struct BlockStr {
    int64_t s[3];                           // byte strides, logical order
    __device__ __forceinline__ int64_t off(const int64_t *idx) const { return idx[0] * s[0] + idx[1] * s[1] + idx[2] * s[2]; }
};

// grid.y walks the slowest memory axis (a row loop: grid_of caps grid.y), grid.x / threads the flattened two fast axes:
// 32-bit index arithmetic inside a plane, consecutive threads on consecutive elements
#define PMX_BLOCK_LOOP(g)                                                                                          \
    const uint32_t n1_ = (uint32_t)(g).shape[(g).ax[1]], n2_ = (uint32_t)(g).shape[(g).ax[2]];                     \
    const uint32_t inner_ = n1_ * n2_;                                                                             \
    for (int64_t i0_ = blockIdx.y; i0_ < (g).shape[(g).ax[0]]; i0_ += gridDim.y)                                   \
    for (uint32_t q_ = blockIdx.x * blockDim.x + threadIdx.x; q_ < inner_; q_ += gridDim.x * blockDim.x)

__device__ __forceinline__ void block_index(const BlockGeom &g, int64_t i0, uint32_t q, int64_t *idx)
{
    const uint32_t n2 = (uint32_t)g.shape[g.ax[2]];
    const uint32_t i1 = q / n2;
    const int64_t v0 = i0, v1 = i1, v2 = q - i1 * n2;
#pragma unroll
    for (int d = 0; d < 3; d++) idx[d] = (g.ax[0] == d) ? v0 : ((g.ax[1] == d) ? v1 : v2);
}

// ---- wavenumbers -------------------------------------------------------------------------------------------------
// w = 2 pi / n (gi - n [gi >= n / 2]) of global index gi along an axis of n cells (Nyquist negative), dw = 2 pi / n.
// k = w N / L is rounded in two ways, and both are kept on purpose: callers that must put a mode at the same k (in the
// same bin, under the same table entry, the same bits fused or stand-alone) use the same one.
//   k_scaled   w * (N / L) with nl = N / L formed on the host: the sequence of the transfer kernels, stand-alone here
//              and fused into the column FFT (pmx_colfft.hip).  apply_transfer, apply_ktable and its gradients
//              (ktable_vjp, apply_ktable_jvp), the LPT kernels (lpt_hessian, lpt_contract): a Tabulated transfer sees
//              the k of apply_transfer.  It is within an ulp of ComplexField.x, not equal to it.
//   k_divided  (w * N) / L, the Python expression `w * Nmesh[d] / BoxSize[d]` of pm.py:_block_coords (what
//              ComplexField.x returns on an f8 mesh).  power_project, power_vjp, bispec_shells: the bispectrum's
//              shells are power_spectrum's bins, and both are the bins numpy makes of ComplexField.x.
__device__ __forceinline__ double mode_w(int64_t gi, int64_t n, double dw)
{
    double wi = (double)gi;
    if (gi >= n / 2) wi -= n;
    return wi * dw;
}
__device__ __forceinline__ double k_scaled(double w, double nl) { return w * nl; }
__device__ __forceinline__ double k_divided(double w, double n, double L) { return (w * n) / L; }

// k_d per axis (0 beyond ndim) into kk, w_d into ww when asked, and k^2 = (k_0^2 + k_1^2) + k_2^2
template <bool DIVIDED = false>
__device__ __forceinline__ double wavevector(const BlockGeom &g, const int64_t *idx, double *kk, double *ww = nullptr)
{
    double k2 = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        kk[d] = 0;
        if (ww) ww[d] = 0;
    }
    // (break, not continue: with continue the general transfer_kernel reloads more spilled scalar registers and is
    // 3-4% slower at 512^3, profiles/kspace_block/timing.txt)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (d >= g.ndim) break;
        const double w = mode_w(idx[d] + g.start[d], g.nmesh[d], g.dw[d]);
        if (ww) ww[d] = w;
        kk[d] = DIVIDED ? k_divided(w, (double)g.nmesh[d], g.boxsize[d]) : k_scaled(w, g.nl[d]);
        k2 += kk[d] * kk[d];
    }
    return k2;
}

// sinc(w / 2)^p for p >= 1, the window deconvolution factor of one axis; a Taylor series next to zero
__device__ __forceinline__ double sinc_pow(double w, int p)
{
    const double x = 0.5 * w;
    double s;
    if (x < 1e-5 && x > -1e-5) { double x2 = x * x; s = 1.0 - x2 / 6. + x2 * x2 / 120.; }
    else s = sin(x) / x;
    double sp = s;
    for (int e = 1; e < p; e++) sp *= s;
    return sp;
}

// ---- complex elements of f4 / f8 storage, as doubles ---------------------------------------------------------------
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

// ---- host ----------------------------------------------------------------------------------------------------------

// The memory order of the axes: ax[0] slowest .. ax[2] fastest by decreasing |stride|.  The two rules differ in where
// an axis of extent 1 goes, which decides the thread-to-element map of degenerate shapes and the summation order of
// the power spectrum; an entry point keeps the rule it was written with.
//   AXES_BY_STRIDE     by |stride| alone; on equal strides an extent-1 axis takes the faster position of the two
//   AXES_UNIT_SLOWEST  axes of extent 1 first (slowest), the others by |stride|
enum AxisRule { AXES_BY_STRIDE, AXES_UNIT_SLOWEST };

static void axis_order(AxisRule rule, const int64_t *shape, const int64_t *stride, int32_t *ax)
{
    for (int a = 0; a < 3; a++) ax[a] = a;
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++) {
            const int x = ax[a], y = ax[b];
            const bool ux = shape[x] == 1, uy = shape[y] == 1;
            const int64_t sx = llabs(stride[x]), sy = llabs(stride[y]);
            bool swap;
            if (rule == AXES_UNIT_SLOWEST) swap = ux != uy ? uy : sx < sy;
            else swap = sx < sy || (sx == sy && ux && !uy);
            if (swap) { ax[a] = y; ax[b] = x; }
        }
}

// the block geometry, axes ordered by the byte strides `order` (start, nmesh, boxsize may be null: a real block)
static BlockGeom make_geom(int32_t ndim, const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                           const double *boxsize, const int64_t *order, AxisRule rule = AXES_BY_STRIDE)
{
    BlockGeom g;
    g.ndim = ndim;
    int64_t os[3];
    for (int d = 0; d < 3; d++) {
        const bool on = d < ndim;
        g.shape[d] = on ? shape[d] : 1;
        g.start[d] = on && start ? start[d] : 0;
        g.nmesh[d] = on && nmesh ? nmesh[d] : 1;
        g.boxsize[d] = on && boxsize ? boxsize[d] : 1.0;
        g.dw[d] = 2 * M_PI / g.nmesh[d];
        g.nl[d] = g.nmesh[d] / g.boxsize[d];
        os[d] = on ? order[d] : 0;
    }
    axis_order(rule, g.shape, os, g.ax);
    return g;
}

// (s null: all zero, a block that is not read)
static BlockStr make_str(int32_t ndim, const int64_t *s)
{
    BlockStr r;
    for (int d = 0; d < 3; d++) r.s[d] = s && d < ndim ? s[d] : 0;
    return r;
}

// The launch grid of PMX_BLOCK_LOOP with 256 threads.  0: nothing to do; -1: a plane too large for the 32-bit index.
// grid.y is capped at 65535, the limit of the launch: the row loop takes the rest.
static int grid_of(const BlockGeom &g, dim3 &grid)
{
    if (g.shape[0] * g.shape[1] * g.shape[2] == 0) return 0;
    const int64_t inner = g.shape[g.ax[1]] * g.shape[g.ax[2]];
    if (inner >= (1ll << 31)) return -1;
    const int64_t n0 = g.shape[g.ax[0]];
    grid = dim3((unsigned)((inner + 255) / 256), (unsigned)(n0 < 65535 ? n0 : 65535));
    return 1;
}

}  // namespace pmx
