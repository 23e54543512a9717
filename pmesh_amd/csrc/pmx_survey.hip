// pmx_survey.hip — the two harmonic passes of the survey power multipoles with a local line of sight, the FFT form
// of the Yamamoto estimator (include/pmesh_amd.h: pmx_ylm_weight, pmx_ylm_accumulate; pmesh_amd/survey.py).
//
// Replaces the Field.apply slab loops over RealField.x / ComplexField.x a caller of the reference needs for them (14
// passes for ell = 2 and 4, each materialising coordinate arrays).  Both kernels stream: one thread per element in
// memory order (PMX_BLOCK_LOOP), one read and one write per cell (the accumulating form two reads), positions and
// wavevectors recomputed from the index.  Y_lm is a Cartesian polynomial of the unit vector: no trigonometric calls,
// one sqrt and one division per element; (ell, m) are kernel arguments, so the switch over them is a scalar branch
// the whole wave takes together, and the normalisation (with the 4 pi / (2 ell + 1) of the accumulation) is folded
// into one factor on the host.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pmx_common.h"
#include "pmx_block_dev.h"

namespace pmx {

// Y_lm(v) / norm for the real orthonormal harmonics without the Condon-Shortley phase, v = (x, y, z) a unit vector:
// d^|m| P_l / dz^|m| times Re (m >= 0) or Im (m < 0) of (x + i y)^|m|; norm = N_lm, times sqrt 2 for m != 0
// (ylm_norm below).  ell in {0, 2, 4}, |m| <= ell.
__device__ __forceinline__ double ylm_poly(int ell, int m, double x, double y, double z)
{
    const double zz = z * z;
    const double c2 = x * x - y * y, s2 = 2.0 * (x * y);
    switch (ell * 16 + m + 4) {
    case 0 * 16 + 4: return 1.0;
    case 2 * 16 + 4: return 1.5 * zz - 0.5;
    case 2 * 16 + 5: return 3.0 * (z * x);
    case 2 * 16 + 3: return 3.0 * (z * y);
    case 2 * 16 + 6: return 3.0 * c2;
    case 2 * 16 + 2: return 3.0 * s2;
    case 4 * 16 + 4: return (35.0 * zz - 30.0) * zz * 0.125 + 0.375;
    case 4 * 16 + 5: return (17.5 * zz - 7.5) * (z * x);
    case 4 * 16 + 3: return (17.5 * zz - 7.5) * (z * y);
    case 4 * 16 + 6: return (52.5 * zz - 7.5) * c2;
    case 4 * 16 + 2: return (52.5 * zz - 7.5) * s2;
    case 4 * 16 + 7: return 105.0 * z * (x * (x * x - 3.0 * (y * y)));
    case 4 * 16 + 1: return 105.0 * z * (y * (3.0 * (x * x) - y * y));
    case 4 * 16 + 8: return 105.0 * (c2 * c2 - s2 * s2);
    default: return 105.0 * (2.0 * (c2 * s2));      // 4 * 16 + 0
    }
}

// norm * Y_lm / norm of the direction of v; a zero vector has Y_00 alone
__device__ __forceinline__ double ylm_of(int ell, int m, double norm, const double *v)
{
    const double r2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (r2 == 0) return ell == 0 ? norm : 0.0;
    const double inv = 1.0 / sqrt(r2);
    return norm * ylm_poly(ell, m, v[0] * inv, v[1] * inv, v[2] * inv);
}

struct Origin {
    double o[3];
};

// out = in * Y_lm(r_hat), r = x - origin, x_d = (g_d * L_d) / N_d of the global cell index g
template <typename T>
__global__ void __launch_bounds__(256) ylm_weight_kernel(int ell, int m, double norm, Origin org, BlockGeom g, const char *in,
                                                         BlockStr is, char *out, BlockStr os)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double r[3];
#pragma unroll
        for (int d = 0; d < 3; d++)
            r[d] = ((double)(idx[d] + g.start[d]) * g.boxsize[d]) / (double)g.nmesh[d] - org.o[d];
        const double w = ylm_of(ell, m, norm, r);
        const double f = (double)*(const T *)(in + is.off(idx));
        *(T *)(out + os.off(idx)) = (T)(f * w);
    }
}

// acc = (BETA ? acc : 0) + scale * Y_lm(k_hat) * in; norm holds scale * the harmonic's own factor
template <typename T, bool BETA>
__global__ void __launch_bounds__(256) ylm_accumulate_kernel(int ell, int m, double norm, BlockGeom g, const char *in,
                                                             BlockStr is, char *acc, BlockStr as)
{
    PMX_BLOCK_LOOP(g) {
        int64_t idx[3];
        block_index(g, i0_, q_, idx);
        double kk[3];
        wavevector(g, idx, kk);
        const double w = ylm_of(ell, m, norm, kk);
        double re, im;
        CLoad<T>::get(in + is.off(idx), re, im);
        re *= w;
        im *= w;
        char *p = acc + as.off(idx);
        if (BETA) {
            double ar, ai;
            CLoad<T>::get(p, ar, ai);
            re += ar;
            im += ai;
        }
        CLoad<T>::put(p, re, im);
    }
}

#undef PMX_BLOCK_LOOP

}  // namespace pmx

using namespace pmx;

// N_lm = sqrt((2 l + 1) / (4 pi) (l - |m|)! / (l + |m|)!), times sqrt 2 for m != 0
static double ylm_norm(int ell, int m)
{
    const int am = m < 0 ? -m : m;
    double ratio = 1.0;     // (l - |m|)! / (l + |m|)!
    for (int j = ell - am + 1; j <= ell + am; j++) ratio /= j;
    return sqrt((2 * ell + 1) / (4 * M_PI) * ratio) * (am ? sqrt(2.0) : 1.0);
}

static bool ylm_ok(int ell, int m) { return (ell == 0 || ell == 2 || ell == 4) && m >= -ell && m <= ell; }

extern "C" int pmx_ylm_weight(int32_t ell, int32_t m, int32_t ndim, int32_t elsize, const void *in,
                              const int64_t *in_strides, void *out, const int64_t *out_strides, const int64_t *shape,
                              const int64_t *start, const int64_t *nmesh, const double *boxsize, const double *origin,
                              void *stream)
{
    PMX_REQUIRE(ndim == 3 && ylm_ok(ell, m), PMX_EUNSUPPORTED, "3-d blocks, ell in {0, 2, 4}, |m| <= ell");
    PMX_REQUIRE(in && in_strides && out && out_strides && shape && start && nmesh && boxsize && origin, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, out_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 cells");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), os = make_str(ndim, out_strides);
    Origin org;
    for (int d = 0; d < 3; d++) org.o[d] = origin[d];
    const double norm = ylm_norm(ell, m);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        ylm_weight_kernel<T><<<grid, 256, 0, st>>>(ell, m, norm, org, g, (const char *)in, is, (char *)out, os);
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_ylm_accumulate(int32_t ell, int32_t m, int32_t beta, int32_t ndim, int32_t elsize, const void *in,
                                  const int64_t *in_strides, void *acc, const int64_t *acc_strides,
                                  const int64_t *shape, const int64_t *start, const int64_t *nmesh,
                                  const double *boxsize, void *stream)
{
    PMX_REQUIRE(ndim == 3 && ylm_ok(ell, m), PMX_EUNSUPPORTED, "3-d blocks, ell in {0, 2, 4}, |m| <= ell");
    PMX_REQUIRE(in && in_strides && acc && acc_strides && shape && start && nmesh && boxsize, PMX_EINVAL,
                "bad arguments");
    PMX_REQUIRE(elsize == 4 || elsize == 8, PMX_EINVAL, "elsize must be 4 or 8");
    PMX_REQUIRE(beta == 0 || beta == 1, PMX_EINVAL, "beta must be 0 or 1");
    const BlockGeom g = make_geom(ndim, shape, start, nmesh, boxsize, acc_strides);
    dim3 grid;
    const int r = grid_of(g, grid);
    PMX_REQUIRE(r >= 0, PMX_EUNSUPPORTED, "plane of more than 2^31 modes");
    if (r == 0) return PMX_OK;
    const BlockStr is = make_str(ndim, in_strides), as = make_str(ndim, acc_strides);
    const double norm = 4 * M_PI / (2 * ell + 1) * ylm_norm(ell, m);
    hipStream_t st = (hipStream_t)stream;
    with_canvas(elsize, [&](auto c) {
        using T = typename decltype(c)::type;
        with_bool(beta != 0, [&](auto b) {
            ylm_accumulate_kernel<T, b><<<grid, 256, 0, st>>>(ell, m, norm, g, (const char *)in, is, (char *)acc, as);
        });
    });
    PMX_HIP_CHECK(hipGetLastError());
    return PMX_OK;
}
