// pmx_ktable_grad.hip — the gradients of the tabulated transfer of pmx_lpt.hip with respect to its table values
// (include/pmesh_amd.h: pmx_ktable_vjp, pmx_apply_ktable_jvp).
//
// A caller of the reference fits band powers or transfer-function nodes through numpy.interp inside Field.apply and has
// no gradient of it at all.  Both kernels stream over the complex block like ktable_kernel, wavenumbers recomputed from
// the index and the table searched by the same table_find (pmx_block_dev.h).
//   ktable_vjp:  reads in and v once; a mode between two table entries adds its two interpolation weights times
//                w Re(conj(v) in) into a copy of the table's sums in LDS (n doubles, sized to the table).  Neighbouring
//                modes of a wave mostly share an entry, and LDS atomics on one address run one lane after another: a
//                wave first sums each run of lanes with the same entry by shuffles and only the head of a run adds.
//                A workgroup walks many rows and adds its non-zero sums to the global ones once, at its end.
//   ktable_jvp:  ktable_kernel with a second table of values, the tangent of the first.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

constexpr int KV_BLOCKS = 2048;     // workgroups of ktable_vjp: a few per CU, each flushes its sums once

// the sum of v over the run of lanes [lane, end) in the run's first lane (other lanes: partial sums)
__device__ __forceinline__ double run_sum(double v, int lane, int end)
{
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(v, d, 64);
        if (lane + d < end) v += o;
    }
    return v;
}

template <typename T, bool LOG>
__global__ void __launch_bounds__(256) ktable_vjp_kernel(pmx_ktable t, BlockGeom g, int hermitian, const char *in, BlockStr is,
                                                         const char *v, BlockStr vs, double *__restrict__ grad)
{
    extern __shared__ double tab[];                 // t.n sums
    for (int i = threadIdx.x; i < t.n; i += 256) tab[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int last = g.ndim - 1;
    const uint32_t n1_ = (uint32_t)g.shape[g.ax[1]], n2_ = (uint32_t)g.shape[g.ax[2]];
    const uint32_t inner_ = n1_ * n2_;
    // (whole waves take every step of the walk: the shuffles below need all 64 lanes)
    const uint32_t span_ = (inner_ + 63u) & ~63u;
    for (int64_t i0_ = blockIdx.y; i0_ < g.shape[g.ax[0]]; i0_ += gridDim.y)
        for (uint32_t q_ = blockIdx.x * 256 + threadIdx.x; q_ < span_; q_ += gridDim.x * 256) {
            int key = -1;
            double wa = 0, wb = 0;
            if (q_ < inner_) {
                int64_t idx[3];
                block_index(g, i0_, q_, idx);
                double kk[3];
                const double k = sqrt(wavevector(g, idx, kk));
                if (k >= t.kmin && k <= t.kmax) {
                    double ar, ai, vr, vi;
                    CLoad<T>::get(in + is.off(idx), ar, ai);
                    CLoad<T>::get(v + vs.off(idx), vr, vi);
                    double r = vr * ar + vi * ai;
                    if (hermitian) {
                        const int64_t il = idx[last] + g.start[last];
                        if (il != 0 && il != g.nmesh[last] / 2) r = 2.0 * r;
                    }
                    const double u = LOG ? log(k) : k;
                    double f, lnT = 0;              // lnT: table_interp(x, y, u) from the entry already found
                    if (u <= t.x[0]) {
                        key = 0;
                        f = 0;
                        if (LOG) lnT = t.y[0];
                    } else if (u >= t.x[t.n - 1]) {
                        key = t.n - 2;
                        f = 1;
                        if (LOG) lnT = t.y[t.n - 1];
                    } else {
                        key = table_find(t.x, t.n, t.inv_step, u);
                        const double xl = t.x[key], dx = t.x[key + 1] - xl;
                        f = (u - xl) / dx;
                        if (LOG) {
                            const double yl = t.y[key];
                            lnT = xl == u ? yl : ((t.y[key + 1] - yl) / dx) * (u - xl) + yl;
                        }
                    }
                    if (LOG) r *= exp(lnT);
                    wa = (1.0 - f) * r;
                    wb = f * r;
                }
            }
            // runs of lanes with one entry: the head of each adds the run's two sums
            const int prev = __shfl_up(key, 1, 64);
            const bool head = lane == 0 || prev != key;
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int end = above ? lane + 1 + __ffsll((long long)above) - 1 : 64;
            wa = run_sum(wa, lane, end);
            wb = run_sum(wb, lane, end);
            if (head && key >= 0) {
                if (wa != 0) atomicAdd(tab + key, wa);
                if (wb != 0) atomicAdd(tab + key + 1, wb);
            }
        }
    __syncthreads();
    for (int i = threadIdx.x; i < t.n; i += 256)
        if (tab[i] != 0) unsafeAtomicAdd(grad + i, tab[i]);
}

template <typename T, bool LOG>
__global__ void __launch_bounds__(256) ktable_jvp_kernel(pmx_ktable t, const double *__restrict__ dy, BlockGeom g,
                                                         const char *in, BlockStr is, char *out, BlockStr os)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3];
        const double k = sqrt(wavevector(g, idx, kk));
        double f = 0;
        if (k >= t.kmin && k <= t.kmax) {
            const double u = LOG ? log(k) : k;
            // one search, two interpolations (each what table_interp returns)
            if (u <= t.x[0]) {
                f = dy[0];
                if (LOG) f = exp(t.y[0]) * f;
            } else if (u >= t.x[t.n - 1]) {
                f = dy[t.n - 1];
                if (LOG) f = exp(t.y[t.n - 1]) * f;
            } else {
                const int lo = table_find(t.x, t.n, t.inv_step, u);
                const double xl = t.x[lo], dx = t.x[lo + 1] - xl, dl = dy[lo];
                f = xl == u ? dl : ((dy[lo + 1] - dl) / dx) * (u - xl) + dl;
                if (LOG) {
                    const double yl = t.y[lo];
                    f = exp(xl == u ? yl : ((t.y[lo + 1] - yl) / dx) * (u - xl) + yl) * f;
                }
            }
        }
        f = t.amplitude * f;
        double re, im;
        CLoad<T>::get(in + is.off(idx), re, im);
        CLoad<T>::put(out + os.off(idx), f * re, f * im);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_ktable_vjp(const pmx_ktable *t, int32_t hermitian, int32_t ndim, int32_t elsize, const void *in,
                              const int64_t *in_strides, const void *v, const int64_t *v_strides, const int64_t *shape,
                              const int64_t *start, const int64_t *nmesh, const double *boxsize, double *grad,
                              void *stream)
{
    PMX_REQUIRE(t && ndim >= 1 && ndim <= 3 && in && v && in_strides && v_strides && shape && start && nmesh &&
                    boxsize && grad,
                PMX_EINVAL, "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(t->n >= 2 && t->n <= PMX_KTABLE_MAX, PMX_EUNSUPPORTED, "table of 2 .. PMX_KTABLE_MAX entries");
    PMX_REQUIRE(t->x && (t->y || !t->loglog), PMX_EINVAL, "table pointers");
    BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, in_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    // a few workgroups per CU, each walking many rows: grid.x over the plane, grid.y over the slowest axis
    if (grid.x > (unsigned)KV_BLOCKS) grid.x = KV_BLOCKS;
    const unsigned ny = KV_BLOCKS / grid.x;
    if (grid.y > ny) grid.y = ny;
    const BlockStr is = make_str(ndim, in_strides), vs = make_str(ndim, v_strides);
    hipStream_t st = (hipStream_t)stream;
    const char *a = (const char *)in, *b = (const char *)v;
    const size_t lds = sizeof(double) * (size_t)t->n;
    const int h = hermitian ? 1 : 0;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(t->loglog != 0, [&](auto lg) {
            ktable_vjp_kernel<T, lg><<<grid, 256, lds, st>>>(*t, g, h, a, is, b, vs, grad);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_apply_ktable_jvp(const pmx_ktable *t, const double *dy, int32_t ndim, int32_t elsize, const void *in,
                                    const int64_t *in_strides, void *out, const int64_t *out_strides,
                                    const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                    const double *boxsize, void *stream)
{
    PMX_REQUIRE(t && dy && ndim >= 1 && ndim <= 3 && in && out && in_strides && out_strides && shape, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(t->n >= 2 && t->n <= PMX_KTABLE_MAX, PMX_EUNSUPPORTED, "table of 2 .. PMX_KTABLE_MAX entries");
    PMX_REQUIRE(t->x && (t->y || !t->loglog), PMX_EINVAL, "table pointers");
    BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    const char *a = (const char *)in;
    char *b = (char *)out;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(t->loglog != 0, [&](auto lg) {
            ktable_jvp_kernel<T, lg><<<grid, 256, 0, st>>>(*t, dy, g, a, is, b, os);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
