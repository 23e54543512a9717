// pmx_lpt.hip — initial conditions: a tabulated transfer T(|k|), the Hessian spectra k_i k_j / k^2 of the linear
// density and the second-order LPT source built from them (include/pmesh_amd.h: pmx_apply_ktable, pmx_lpt_hessian,
// pmx_lpt2_source).
//
// Replaces the host slab loop Field.apply falls back to for a numpy.interp transfer (the reference's
// examples/nbody.py:245-282) and the chain of per-component apply calls and products of the reference's
// nbody/genic.py:121-166.  All three kernels stream: one read and one write per element (the Hessian kernel one read
// and up to three writes, the source kernel one read of each of its 3 or 6 inputs), one thread per element in memory
// order (PMX_BLOCK_LOOP), wavenumbers recomputed from the index with the roundings of transfer_kernel
// (pmx_block_dev.h: k_scaled).
// The table of pmx_apply_ktable stays in device memory: a wave's neighbouring modes walk the same few lines of it,
// which the L1 / L2 serve, and no workgroup pays for loading a whole table into LDS.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

struct HOut {
    char *p[3];
    BlockStr s[3];
    int32_t i[3], j[3];
};

struct SIn {
    const char *p[6];
    BlockStr s[6];
};

template <typename T, bool LOG>
__global__ void __launch_bounds__(256) ktable_kernel(pmx_ktable t, BlockGeom g, const char *in, BlockStr is, char *out, BlockStr os)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3];
        const double k = sqrt(wavevector(g, idx, kk));
        double f;
        if (k < t.kmin) f = t.left;
        else if (k > t.kmax) f = t.right;
        else if (LOG) f = exp(table_interp(t.x, t.y, t.n, t.inv_step, log(k)));
        else f = table_interp(t.x, t.y, t.n, t.inv_step, k);
        f = t.amplitude * f;
        double re, im;
        CLoad<T>::get(in + is.off(idx), re, im);
        CLoad<T>::put(out + os.off(idx), f * re, f * im);
    }
}

template <typename T, int NOUT>
__global__ void __launch_bounds__(256) hessian_kernel(BlockGeom g, const char *in, BlockStr is, HOut o)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3];
        const double k2 = wavevector(g, idx, kk);
        double re, im;
        CLoad<T>::get(in + is.off(idx), re, im);
#pragma unroll
        for (int p = 0; p < NOUT; p++) {
            const double f = (k2 == 0) ? 0.0 : (kk[o.i[p]] * kk[o.j[p]]) / k2;
            CLoad<T>::put(o.p[p] + o.s[p].off(idx), f * re, f * im);
        }
    }
}

template <typename T> __device__ __forceinline__ double rget(const SIn &a, int q, const int64_t *idx)
{
    return (double)*(const T *)(a.p[q] + a.s[q].off(idx));
}

template <typename T, int ND>
__global__ void __launch_bounds__(256) lpt2_source_kernel(BlockGeom g, SIn a, char *out, BlockStr os, double scale)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double s;
        if (ND == 2) {
            const double p00 = rget<T>(a, 0, idx), p11 = rget<T>(a, 1, idx), p01 = rget<T>(a, 2, idx);
            s = p00 * p11 - p01 * p01;
        } else {
            const double p00 = rget<T>(a, 0, idx), p11 = rget<T>(a, 1, idx), p22 = rget<T>(a, 2, idx);
            const double p01 = rget<T>(a, 3, idx), p02 = rget<T>(a, 4, idx), p12 = rget<T>(a, 5, idx);
            s = p00 * p11 + p11 * p22;
            s = s + p22 * p00;
            s = s - p01 * p01;
            s = s - p02 * p02;
            s = s - p12 * p12;
        }
        *(T *)(out + os.off(idx)) = (T)(scale * s);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_apply_ktable(const pmx_ktable *t, int32_t ndim, int32_t elsize, const void *in,
                                const int64_t *in_strides, void *out, const int64_t *out_strides,
                                const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                const double *boxsize, void *stream)
{
    PMX_REQUIRE(t && ndim >= 1 && ndim <= 3 && in && out && in_strides && out_strides && shape, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(t->n >= 2 && t->n <= PMX_KTABLE_MAX, PMX_EUNSUPPORTED, "table of 2 .. PMX_KTABLE_MAX entries");
    PMX_REQUIRE(t->x && t->y, PMX_EINVAL, "table pointers");
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
            ktable_kernel<T, lg><<<grid, 256, 0, st>>>(*t, g, a, is, b, os);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_lpt_hessian(int32_t ndim, int32_t elsize, const void *in, const int64_t *in_strides, int32_t nout,
                               const int32_t *pairs, void *const *out, const int64_t *out_strides,
                               const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                               const double *boxsize, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && in && in_strides && pairs && out && out_strides && shape, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nout >= 1 && nout <= 3, PMX_EINVAL, "1 .. 3 outputs");
    HOut o;
    for (int p = 0; p < 3; p++) {
        const bool on = p < nout;
        o.p[p] = on ? (char *)out[p] : nullptr;
        o.s[p] = make_str(ndim, on ? out_strides + 3 * p : in_strides);
        o.i[p] = on ? pairs[2 * p] : 0;
        o.j[p] = on ? pairs[2 * p + 1] : 0;
        PMX_REQUIRE(!on || (o.p[p] && o.i[p] >= 0 && o.i[p] < ndim && o.j[p] >= 0 && o.j[p] < ndim), PMX_EINVAL,
                    "output pointer or pair out of range");
    }
    BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, in_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides);
    hipStream_t st = (hipStream_t)stream;
    const char *a = (const char *)in;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_count<3>(nout, [&](auto n) { hessian_kernel<T, n><<<grid, 256, 0, st>>>(g, a, is, o); });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_lpt2_source(int32_t ndim, int32_t elsize, const void *const *in, const int64_t *in_strides,
                               void *out, const int64_t *out_strides, const int64_t *shape, double scale, void *stream)
{
    PMX_REQUIRE((ndim == 2 || ndim == 3) && in && in_strides && out && out_strides && shape, PMX_EINVAL,
                "bad arguments (ndim 2 or 3)");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    const int nin = ndim == 2 ? 3 : 6;
    SIn a;
    for (int q = 0; q < 6; q++) {
        const bool on = q < nin;
        a.p[q] = on ? (const char *)in[q] : nullptr;
        a.s[q] = make_str(ndim, on ? in_strides + 3 * q : out_strides);
        PMX_REQUIRE(!on || a.p[q], PMX_EINVAL, "input pointer");
    }
    BlockGeom g = make_geom(ndim, shape, nullptr, nullptr, nullptr, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 elements");
    if (r == 0) return PMX_OK;
    const BlockStr os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    char *b = (char *)out;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(ndim == 2, [&](auto two) {
            lpt2_source_kernel<T, two ? 2 : 3><<<grid, 256, 0, st>>>(g, a, b, os, scale);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
