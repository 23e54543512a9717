// pmx_lpt_grad.hip — the adjoint and the tangent of the second-order LPT chain of pmx_lpt.hip (include/pmesh_amd.h:
// pmx_lpt_contract, pmx_lpt2_source_vjp, pmx_lpt2_source_jvp).
//
// Replaces the chains of the reference's pmesh/abopt.py (the transfer vjp of apply_transfer and the c2r / r2c vjps
// composed per component) that a caller of Field.apply would spell for the gradient of 2LPT.  The three kernels stream
// like those of pmx_lpt.hip: one thread per element in memory order, wavenumbers recomputed from the index
// (pmx_block_dev.h: k_scaled), double arithmetic over f4 / f8 storage.
//   contract:   out = (accumulate ? out : 0) + sum_c f_c(k) in_c over 1..6 spectra, f_c = k_i k_j / k^2 (a Hessian
//               factor) or -i k_d / k^2 (the conjugate of the gradient factor of Transfer.dx1)
//   source_vjp: the 3 or 6 products scale g dQ/dphi_p, written over the Hessian components when asked
//   source_jvp: scale dQ(phi; phi'), the bilinear form of the source
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

struct CIn {
    const char *p[6];
    BlockStr s[6];
    int32_t a[6], b[6];     // factor c: k_a k_b / k^2 (b >= 0) or -i k_a / k^2 (b < 0)
};

struct RSet {
    const char *p[6];
    BlockStr s[6];
};

struct WSet {
    char *p[6];
    BlockStr s[6];
};

template <typename T, int NIN>
__global__ void __launch_bounds__(256) contract_kernel(BlockGeom g, CIn in, char *out, BlockStr os, int accumulate)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3];
        const double k2 = wavevector(g, idx, kk);
        char *o = out + os.off(idx);
        double re = 0, im = 0;
        if (accumulate) CLoad<T>::get(o, re, im);
#pragma unroll
        for (int c = 0; c < NIN; c++) {
            double x, y;
            CLoad<T>::get(in.p[c] + in.s[c].off(idx), x, y);
            if (in.b[c] >= 0) {
                const double f = (k2 == 0) ? 0.0 : (kk[in.a[c]] * kk[in.b[c]]) / k2;
                re = re + f * x;
                im = im + f * y;
            } else {                                    // (-i f) (x + i y) = f y - i f x
                const double f = (k2 == 0) ? 0.0 : kk[in.a[c]] / k2;
                re = re + f * y;
                im = im - f * x;
            }
        }
        CLoad<T>::put(o, re, im);
    }
}

template <typename T> __device__ __forceinline__ double rload(const RSet &a, int q, const int64_t *idx)
{
    return (double)*(const T *)(a.p[q] + a.s[q].off(idx));
}

template <typename T> __device__ __forceinline__ void rstore(const WSet &a, int q, const int64_t *idx, double v)
{
    *(T *)(a.p[q] + a.s[q].off(idx)) = (T)v;
}

// every input of the element is read before the first write: an output may be its own input
template <typename T, int ND>
__global__ void __launch_bounds__(256) lpt2_source_vjp_kernel(BlockGeom g, const char *gp, BlockStr gs, RSet h, WSet o,
                                                              double scale)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        const double a = scale * (double)*(const T *)(gp + gs.off(idx));
        if (ND == 2) {
            const double p00 = rload<T>(h, 0, idx), p11 = rload<T>(h, 1, idx), p01 = rload<T>(h, 2, idx);
            rstore<T>(o, 0, idx, a * p11);
            rstore<T>(o, 1, idx, a * p00);
            rstore<T>(o, 2, idx, a * (-2.0 * p01));
        } else {
            const double p00 = rload<T>(h, 0, idx), p11 = rload<T>(h, 1, idx), p22 = rload<T>(h, 2, idx);
            const double p01 = rload<T>(h, 3, idx), p02 = rload<T>(h, 4, idx), p12 = rload<T>(h, 5, idx);
            rstore<T>(o, 0, idx, a * (p11 + p22));
            rstore<T>(o, 1, idx, a * (p22 + p00));
            rstore<T>(o, 2, idx, a * (p00 + p11));
            rstore<T>(o, 3, idx, a * (-2.0 * p01));
            rstore<T>(o, 4, idx, a * (-2.0 * p02));
            rstore<T>(o, 5, idx, a * (-2.0 * p12));
        }
    }
}

template <typename T, int ND>
__global__ void __launch_bounds__(256) lpt2_source_jvp_kernel(BlockGeom g, RSet h, RSet t, char *out, BlockStr os,
                                                              double scale)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double s;
        if (ND == 2) {
            const double p00 = rload<T>(h, 0, idx), p11 = rload<T>(h, 1, idx), p01 = rload<T>(h, 2, idx);
            const double q00 = rload<T>(t, 0, idx), q11 = rload<T>(t, 1, idx), q01 = rload<T>(t, 2, idx);
            s = (p00 * q11 + q00 * p11) - 2.0 * (p01 * q01);
        } else {
            const double p00 = rload<T>(h, 0, idx), p11 = rload<T>(h, 1, idx), p22 = rload<T>(h, 2, idx);
            const double p01 = rload<T>(h, 3, idx), p02 = rload<T>(h, 4, idx), p12 = rload<T>(h, 5, idx);
            const double q00 = rload<T>(t, 0, idx), q11 = rload<T>(t, 1, idx), q22 = rload<T>(t, 2, idx);
            const double q01 = rload<T>(t, 3, idx), q02 = rload<T>(t, 4, idx), q12 = rload<T>(t, 5, idx);
            s = (p00 * q11 + q00 * p11) + (p11 * q22 + q11 * p22);
            s = s + (p22 * q00 + q22 * p00);
            s = s - 2.0 * (p01 * q01);
            s = s - 2.0 * (p02 * q02);
            s = s - 2.0 * (p12 * q12);
        }
        *(T *)(out + os.off(idx)) = (T)(scale * s);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

extern "C" int pmx_lpt_contract(int32_t ndim, int32_t elsize, int32_t nin, const void *const *in,
                                const int64_t *in_strides, const int32_t *factors, int32_t accumulate, void *out,
                                const int64_t *out_strides, const int64_t *shape, const int64_t *start,
                                const int64_t *nmesh, const double *boxsize, void *stream)
{
    PMX_REQUIRE(ndim >= 1 && ndim <= 3 && in && in_strides && factors && out && out_strides && shape, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(nin >= 1 && nin <= 6, PMX_EINVAL, "1 .. 6 inputs");
    CIn c;
    for (int q = 0; q < 6; q++) {
        const bool on = q < nin;
        c.p[q] = on ? (const char *)in[q] : nullptr;
        c.s[q] = make_str(ndim, on ? in_strides + 3 * q : out_strides);
        c.a[q] = on ? factors[2 * q] : 0;
        c.b[q] = on ? factors[2 * q + 1] : 0;
        PMX_REQUIRE(!on || (c.p[q] && c.a[q] >= 0 && c.a[q] < ndim && c.b[q] < ndim), PMX_EINVAL,
                    "input pointer or factor out of range");
        if (on && c.b[q] < 0) c.b[q] = -1;
    }
    BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr os = make_str(ndim, out_strides);
    hipStream_t st = (hipStream_t)stream;
    char *o = (char *)out;
    const int acc = accumulate ? 1 : 0;
    with_canvas(elsize, [&](auto tc) {
        using T = typename decltype(tc)::type;
        with_count<6>(nin, [&](auto n) { contract_kernel<T, n><<<grid, 256, 0, st>>>(g, c, o, os, acc); });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

static int real_set(int32_t ndim, int n, const void *const *p, const int64_t *strides, const int64_t *fallback,
                    const char **ptr, BlockStr *str)
{
    for (int q = 0; q < 6; q++) {
        const bool on = q < n;
        ptr[q] = on ? (const char *)p[q] : nullptr;
        str[q] = make_str(ndim, on ? strides + 3 * q : fallback);
        if (on && !ptr[q]) return 0;
    }
    return 1;
}

extern "C" int pmx_lpt2_source_vjp(int32_t ndim, int32_t elsize, const void *g, const int64_t *g_strides,
                                   const void *const *in, const int64_t *in_strides, void *const *out,
                                   const int64_t *out_strides, const int64_t *shape, double scale, void *stream)
{
    PMX_REQUIRE((ndim == 2 || ndim == 3) && g && g_strides && in && in_strides && out && out_strides && shape,
                PMX_EINVAL, "bad arguments (ndim 2 or 3)");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    const int n = ndim == 2 ? 3 : 6;
    RSet h;
    WSet o;
    const char *op[6];
    PMX_REQUIRE(real_set(ndim, n, in, in_strides, g_strides, h.p, h.s), PMX_EINVAL, "input pointer");
    PMX_REQUIRE(real_set(ndim, n, (const void *const *)out, out_strides, g_strides, op, o.s), PMX_EINVAL,
                "output pointer");
    for (int q = 0; q < 6; q++) o.p[q] = (char *)op[q];
    BlockGeom geo = make_geom(ndim, shape, nullptr, nullptr, nullptr, g_strides);
    dim3 grid;
    const int r = grid_of(geo, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 elements");
    if (r == 0) return PMX_OK;
    const BlockStr gs = make_str(ndim, g_strides);
    hipStream_t st = (hipStream_t)stream;
    const char *gp = (const char *)g;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(ndim == 2, [&](auto two) {
            lpt2_source_vjp_kernel<T, two ? 2 : 3><<<grid, 256, 0, st>>>(geo, gp, gs, h, o, scale);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_lpt2_source_jvp(int32_t ndim, int32_t elsize, const void *const *in, const int64_t *in_strides,
                                   const void *const *tangent, const int64_t *tangent_strides, void *out,
                                   const int64_t *out_strides, const int64_t *shape, double scale, void *stream)
{
    PMX_REQUIRE((ndim == 2 || ndim == 3) && in && in_strides && tangent && tangent_strides && out && out_strides &&
                shape, PMX_EINVAL, "bad arguments (ndim 2 or 3)");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    const int n = ndim == 2 ? 3 : 6;
    RSet h, t;
    PMX_REQUIRE(real_set(ndim, n, in, in_strides, out_strides, h.p, h.s), PMX_EINVAL, "input pointer");
    PMX_REQUIRE(real_set(ndim, n, tangent, tangent_strides, out_strides, t.p, t.s), PMX_EINVAL, "tangent pointer");
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
            lpt2_source_jvp_kernel<T, two ? 2 : 3><<<grid, 256, 0, st>>>(g, h, t, b, os, scale);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
